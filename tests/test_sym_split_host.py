"""CPU tests of the split layout of the symmetric path (flat sphere layouts: A~ = diag(E, O)).

The structure itself on the oracle: in the real-harmonic basis a ball's cosine combinations are even and its sine combinations odd under
reflection of the LAST canonical coordinate, so with every centre at the same last canonical coordinate no entry of W^H M W couples a
cosine slot to a sine slot (<= 1e-13 max |A~|); one centre 0.5 off the plane, or a layout flat in another coordinate, couples them
(>= 1e-3; measured 3.9e-2 to 0.22).  Then the host side of the library: biem_plan_split_order, the two new ABI entries, the workspace
size that serves both forms, and the register budget of the split fill kernel.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from biem_helmholtz_sphere_amd import _build, _lib
from oracle import biem_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cos_sin_coupling(name, cen, n_end, k=1.7):
    """max |cosine-sine entry| / max |A~| of R W^H M W R^-1 for Dirichlet balls of radius 1 (W: cosine combinations first, then sine)."""
    tr = O.tree(name)
    cen = np.array(cen, float)
    B = len(cen)
    A, tabs = O.assemble(tr, n_end, k, 1.0, cen, np.ones(B), np.ones(B, complex), np.zeros(B, complex))
    idx = tr._canon().index(n_end) if tr.base else tr.index(n_end)
    H = len(idx)
    pos = {t: i for i, t in enumerate(idx)}
    cosv, sinv = [], []
    for h, t in enumerate(idx):
        p = pos[t[:-1] + (-t[-1],)]
        if h > p:
            continue
        e = np.zeros(H, complex)
        if h == p:
            e[h] = 1
            cosv.append(e)
        else:
            c = e.copy(); c[h] = c[p] = 2**-0.5; cosv.append(c)
            s = e.copy(); s[p] = 1j * 2**-0.5; s[h] = -1j * 2**-0.5; sinv.append(s)
    W = np.array(cosv + sinv).T
    nc = len(cosv)
    Wb = np.kron(np.eye(B), W)
    deg = tr.degrees(n_end)
    degW = np.array([deg[np.argmax(np.abs(W[:, j]))] for j in range(H)])
    rW = np.concatenate([1 / np.sqrt(tabs[b][0][degW] * tabs[b][1][degW]) for b in range(B)])
    At = (Wb.conj().T @ A.reshape(B * H, B * H) @ Wb) * rW[:, None] / rW[None, :]
    A4 = At.reshape(B, H, B, H)
    cs = max(np.abs(A4[:, :nc, :, nc:]).max(), np.abs(A4[:, nc:, :, :nc]).max())
    return cs / np.abs(At).max(), nc, H


# three balls; `last` = the caller's coordinate that is the last canonical one (bpa, bpbpa: x0 through their canonical axes)
LAYOUTS = {"a": (2, 1), "ba": (3, 2), "bba": (4, 3), "bpa": (3, 0), "bpbpa": (4, 0)}
BASE = np.array([[0.0, 0.0, 0.0, 0.0], [3.0, 1.0, 2.6, -2.8], [-2.5, 4.0, -3.1, 3.3]])


def _centres(tree, plane=0.3, off=None, flat_in=None):
    d, last = LAYOUTS[tree]
    cen = BASE[:, :d].copy()
    if tree == "a":
        cen[:, 0] = [0.0, 3.0, -2.5]
    cen[:, last if flat_in is None else flat_in] = plane
    if off is not None:
        cen[1, last] += off
    return cen


@pytest.mark.parametrize("tree,n_end", [("a", 6), ("ba", 5), ("bba", 4), ("bpa", 5), ("bpbpa", 4)])
def test_flat_centres_decouple_cosine_and_sine_slots(tree, n_end):
    flat, nc, H = _cos_sin_coupling(tree, _centres(tree), n_end)
    off, _, _ = _cos_sin_coupling(tree, _centres(tree, off=0.5), n_end)
    print(f"{tree} n_end={n_end} H={H} cosine={nc}: flat {flat:.2e}, one centre 0.5 off the plane {off:.2e}")
    assert flat <= 1e-13, (tree, flat)
    assert off >= 1e-3, (tree, off)


@pytest.mark.parametrize("tree,n_end,other", [("bpa", 5, 2), ("ba", 5, 1), ("bba", 4, 2), ("bpbpa", 4, 3)])
def test_flat_in_another_coordinate_does_not_decouple(tree, n_end, other):
    """Only the last canonical coordinate carries the parity: centres in a plane of another coordinate (bpa: x2, the plane of ba) couple."""
    v, _, _ = _cos_sin_coupling(tree, _centres(tree, flat_in=other), n_end)
    print(f"{tree} n_end={n_end} flat in x{other} only: {v:.2e}")
    assert v >= 1e-3, (tree, v)


def _plan(lib, tree, n_end):
    plan = C.c_void_p()
    if tree.startswith("chain"):
        _lib.check(lib.biem_plan_create_chain_host(int(tree[5:]), n_end, C.byref(plan)))
    else:
        _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS[tree], n_end, C.byref(plan)))
    return plan


def _split_order(lib, plan, B):
    h = C.c_int()
    _lib.check(lib.biem_plan_info(plan, None, C.byref(h), None, None, None))
    H = h.value
    v = [C.c_int() for _ in range(5)]
    rows = np.full((B, H), -1, dtype=np.int32)
    _lib.check(lib.biem_plan_split_order(plan, B, *[C.byref(x) for x in v], rows.ctypes.data))
    return H, [x.value for x in v], rows


@pytest.mark.parametrize("tree,n_end,B", [("a", 6, 3), ("ba", 5, 1), ("ba", 13, 4), ("ba", 20, 16), ("bba", 7, 2), ("bba", 10, 8), ("caa", 3, 2),
                                          ("chain5", 4, 3)])
def test_split_order_is_a_permutation_onto_the_two_blocks(tree, n_end, B):
    lib = _lib.load()
    plan = _plan(lib, tree, n_end)
    H, (U, nE, nO, npE, npO), rows = _split_order(lib, plan, B)
    partner, slot = np.zeros(H, np.int32), np.zeros(H, np.int32)
    _lib.check(lib.biem_plan_symmetric_order(plan, partner.ctypes.data, slot.ctypes.data))
    lib.biem_plan_destroy(plan)
    units = int(np.sum(partner >= np.arange(H)))                       # one unit per harmonic h <= its partner
    assert U == units and nE == B * U and nO == B * (H - U)
    assert npE % 64 == 0 and npO % 64 == 0 and 0 <= npE - nE < 64 and 0 <= npO - nO < 64
    assert sorted(rows.ravel().tolist()) == list(range(nE)) + list(range(npE, npE + nO))
    for b in range(B):
        assert rows[b, :U].tolist() == list(range(b * U, (b + 1) * U))                                  # cosine run of ball b in E
        assert rows[b, U:].tolist() == list(range(npE + b * (H - U), npE + (b + 1) * (H - U)))          # sine run in O
    if (tree, n_end, B) == ("ba", 20, 16):
        assert (U, H - U, nE, npE, nO, npO) == (210, 190, 3360, 3392, 3040, 3072)
    if (tree, n_end, B) == ("bba", 10, 8):
        assert (U, H - U, nE, npE, nO, npO) == (220, 165, 1760, 1792, 1320, 1344)
    if (tree, n_end, B) == ("ba", 13, 4):
        assert (nE, npE, nO, npO) == (364, 384, 312, 320)


def test_new_entries_in_header_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("biem_plan_split_order", 8), ("biem_last_solve_split", 2)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(lib, name)
    a, b = C.c_int(7), C.c_int(7)
    _lib.check(lib.biem_last_solve_split(C.byref(a), C.byref(b)))
    assert a.value % 64 == 0 and b.value % 64 == 0 and (a.value == 0) == (b.value == 0)     # (0, 0), or the blocks of an earlier solve


@pytest.mark.parametrize("tree,n_end,B,nrhs", [("ba", 13, 4, 1), ("ba", 13, 4, 9), ("ba", 20, 16, 1), ("bba", 7, 2, 3), ("ba", 11, 2, 1), ("a", 6, 3, 2)])
def test_workspace_size_covers_both_forms(tree, n_end, B, nrhs):
    """One size is asked for before the geometry is looked at: it holds the augmented matrices, the factorisation workspace and the
    pivot indices of the larger of the two forms, and the split form's second array of codes."""
    lib = _lib.load()
    plan = _plan(lib, tree, n_end)
    H, (U, nE, nO, npE, npO), _ = _split_order(lib, plan, B)
    nb = 5
    total = lib.biem_solve_workspace_bytes(plan, nb, B, nrhs, nb)
    ldr = (nrhs + 7) // 8 * 8
    up = lambda v: (v + 255) // 256 * 256
    for n_pad in (lib.biem_lu_npad(B * H), npE + npO):
        need = up(nb * B * 3 * n_end * 16) + up(nb * n_pad * (n_pad + ldr) * 16) + up(lib.biem_fill_workspace_bytes(plan, nb, B)) + \
            up(lib.biem_lu_workspace_bytes(nb, n_pad, nrhs)) + up(nb * n_pad * 4) + up(nb * 4)
        assert total >= need, (n_pad, total, need)
    lib.biem_plan_destroy(plan)


def test_split_fill_kernels_use_no_scratch():
    """The split instantiations of the fill kernel that production shapes run (one or two table rows per thread, two combinations per
    iteration) and the split diagonal kernel: no scratch, no spills - and none in the unsplit instantiations of the same sizes beside them."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    if not objdump or not readelf:
        pytest.skip("llvm-objdump / llvm-readelf not found")
    _lib.load()
    metas = {}
    with tempfile.TemporaryDirectory(prefix="biem_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        for f in os.listdir(tmp):
            if "gfx950" in f:
                metas.update(_build._kernel_meta(readelf, os.path.join(tmp, f)))
    seen = 0
    for n, m in metas.items():
        if re.search(r"k_fill_redILi[12]ELi2ELb[01]E", n) or "k_fill_sym_diag_split" in n:
            seen += 1
            assert int(m["private_segment_fixed_size"]) == 0 and int(m["vgpr_spill_count"]) == 0 and int(m["sgpr_spill_count"]) == 0, (n, m)
    assert seen == 5, sorted(n for n in metas if "k_fill" in n)
