"""CPU tests of biem_force(): the identities that pin the yardstick (tests/force_yardstick.py) on the oracle by two independent routes
- the stress tensor integrated from field values alone, and the momentum balance from the powers and the far-field pattern -, the
plan's coupling table, the public surface, the argument checks that run before any device work, and the C declarations.

The coefficient form sees the field another ball throws on this one only up to degree n_end - 1, so both comparisons with it are
limited by truncation and fall with n_end; the two routes against each other are not (see the tests for the measured figures).
"""
import contextlib
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _build, _lib
from oracle import biem_oracle as O

import force_yardstick as FY
from test_chain_trees_host import chain
from test_power_host import COEFFICIENTS, K, _params, _result, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENDS = (6, 8, 10)
STEP = 1e-4
MOMENTUM_RULE = {"a": 40, "ba": 24, "bba": 14}       # resolves |F|^2 x^ to 6e-15 of max |Phi| (against the rule of 6 more points)
SURFACE_RULE = {"a": 24, "ba": 14, "bba": 12}

# |Phi - route| / max |Phi| at n_end = 10, measured when the feature was written (the asserted bound is three times this)
MEASURED_MOMENTUM = {("a", "soft"): 3.5e-8, ("a", "robin"): 5.5e-8, ("a", "per_ball"): 4.4e-7,
                     ("ba", "soft"): 3.2e-8, ("ba", "robin"): 1.9e-8, ("ba", "per_ball"): 3.7e-7,
                     ("bba", "soft"): 2.7e-8, ("bba", "robin"): 5.7e-9, ("bba", "per_ball"): 2.2e-7}
MEASURED_SURFACE = {("a", "soft"): 3.7e-8, ("a", "robin"): 5.6e-8, ("a", "per_ball"): 4.3e-7,
                    ("ba", "soft"): 3.3e-8, ("ba", "robin"): 1.8e-8, ("ba", "per_ball"): 3.7e-7,
                    ("bba", "soft"): 2.8e-8, ("bba", "robin"): 4.0e-9, ("bba", "per_ball"): 2.2e-7}


@contextlib.contextmanager
def registered(name):
    """The oracle with the standard chain `name` as a registered tree (the construction of tests/test_gpu_power.py)."""
    new = name not in O._TREES
    if new:
        O._TREES[name] = chain(len(name) + 1)
    try:
        yield O.tree(name)
    finally:
        if new:
            del O._TREES[name]


_SOLVED, _COUPLING, _SURFACE = {}, {}, {}


def coupling(tree, n_end):
    """The yardstick's dense table (computed once per (tree, n_end), never modified)."""
    key = (tree, n_end)
    if key not in _COUPLING:
        with registered(tree) as tr:
            _COUPLING[key] = FY.coupling(tr, n_end)
        _COUPLING[key].setflags(write=False)
    return _COUPLING[key]


def solved(tree, case, n_end):
    """(OracleResult, uin, uin_grad, p, Phi[B, d], momentum balance [d]) of the geometry of tests/test_power_host.py."""
    key = (tree, case, n_end)
    if key not in _SOLVED:
        cen, rad, p = geometry(O.tree(tree).d)
        uin, ugr = O.plane_wave(K, p)
        a, b = COEFFICIENTS[case]
        res = O.solve_biem(tree, centers=cen, radii=rad, k=K, n_end=n_end, alpha=a, beta=b, uin=uin, uin_grad=ugr)
        phi = FY.force(res, a, b, coupling(tree, n_end))
        _SOLVED[key] = (res, uin, ugr, p, phi, FY.momentum_balance(res, uin, ugr, p, a, b, MOMENTUM_RULE[tree]))
    return _SOLVED[key]


def surface(tree, case, n_end):
    key = (tree, case, n_end)
    if key not in _SURFACE:
        res, uin = solved(tree, case, n_end)[:2]
        _SURFACE[key] = FY.surface_force(res, uin, 1.02, SURFACE_RULE[tree], STEP, with_scale=True)
    return _SURFACE[key]


# ---------------------------------------------------------------------------- the yardstick, pinned by two independent routes
@pytest.mark.parametrize("case", sorted(COEFFICIENTS))
@pytest.mark.parametrize("tree", ["a", "ba", "bba"])
def test_sum_of_forces_is_the_momentum_balance(tree, case):
    """sum_b Phi_b against P_ext p^ - int |F|^2 x^ dOmega, relative to max |Phi|.  Measured at n_end = 6 / 8 / 10:
        a    soft 3.9e-5 / 9.8e-7 / 3.5e-8   robin 1.3e-4 / 1.5e-6 / 5.4e-8   per_ball 3.9e-4 / 1.2e-5 / 4.3e-7
        ba   soft 3.6e-5 / 9.0e-7 / 3.1e-8   robin 3.5e-5 / 4.5e-7 / 1.8e-8   per_ball 3.3e-4 / 9.7e-6 / 3.7e-7
        bba  soft 2.6e-5 / 7.2e-7 / 2.7e-8   robin 7.9e-6 / 1.1e-7 / 5.6e-9   per_ball 1.6e-4 / 5.4e-6 / 2.2e-7
    the truncation of the field one ball throws on the other at degree n_end - 1."""
    errs = []
    for n_end in N_ENDS:
        _, _, _, _, phi, balance = solved(tree, case, n_end)
        errs.append(np.abs(phi.sum(0) - balance).max() / np.abs(phi).max())
    print(f"{tree} {case}: sum Phi {phi.sum(0)}  momentum balance, n_end {N_ENDS}: " + " ".join(f"{e:.2e}" for e in errs))
    assert errs[0] > errs[1] > errs[2]
    assert errs[2] <= 3 * MEASURED_MOMENTUM[tree, case]


@pytest.mark.parametrize("tree,case", sorted(MEASURED_SURFACE))
def test_force_is_the_stress_tensor_of_the_near_field(tree, case):
    """Phi_b against the quadrature of the stress tensor on the spheres of radius 1.02 rho_b from values of the oracle's field alone
    (central differences of step 1e-4), relative to max |Phi|.  Measured at n_end = 6 / 8 / 10:
        a    soft 4.3e-5 / 1.0e-6 / 3.6e-8   robin 1.2e-4 / 1.5e-6 / 5.5e-8   per_ball 3.7e-4 / 1.1e-5 / 4.3e-7
        ba   soft 3.9e-5 / 9.2e-7 / 3.2e-8   robin 3.2e-5 / 4.4e-7 / 1.7e-8   per_ball 3.3e-4 / 9.6e-6 / 3.7e-7
        bba  soft 2.8e-5 / 7.7e-7 / 2.8e-8   robin 7.5e-6 / 1.2e-7 / 4.0e-9   per_ball 1.6e-4 / 5.4e-6 / 2.2e-7
    the same truncation; the difference error sits below it (bba robin at n_end 10 is within a factor 2 of it: the two routes differ
    by 3e-9 of max |Phi| there, see test_stress_tensor_against_momentum_balance)."""
    errs = []
    for n_end in N_ENDS:
        phi = solved(tree, case, n_end)[4]
        errs.append(np.abs(phi - surface(tree, case, n_end)[0]).max() / np.abs(phi).max())
    print(f"{tree} {case}: Phi {phi.tolist()}  stress tensor, n_end {N_ENDS}: " + " ".join(f"{e:.2e}" for e in errs))
    assert errs[0] > errs[1] > errs[2]
    assert errs[2] <= 3 * MEASURED_SURFACE[tree, case]


@pytest.mark.parametrize("tree,case", sorted(MEASURED_SURFACE))
def test_stress_tensor_against_momentum_balance(tree, case):
    """The two routes against each other share no truncation of the coefficient form.  A central difference of a field of wavenumber
    k is short by the fraction (k step)^2 / 6, a product of two gradients by (k step)^2 / 3: that fraction of the gradient terms of the
    integrand, S = (1 / 2k^2) oint (|grad u|^2 + 2 |grad u| |d_n u|) dS summed over the balls, plus the energy-balance bound 1e-9 of
    tests/test_power_host.py on the scale of the forces (the construction of its _flux_bound)."""
    for n_end in (8, 10):
        phi, balance = solved(tree, case, n_end)[4:]
        sf, scale = surface(tree, case, n_end)
        bound = (K * STEP) ** 2 / 3.0 * scale.sum() + 1e-9 * np.abs(phi).max()
        err = np.abs(sf.sum(0) - balance).max()
        print(f"{tree} {case} n_end {n_end}: |sum surface - balance| {err:.2e}  bound {bound:.2e}  (S {scale.sum():.3f}, max |Phi| {np.abs(phi).max():.3f})")
        assert err <= bound


# ---------------------------------------------------------------------------- one ball, symmetric pairs
@pytest.mark.parametrize("case", ["robin", "soft"])
@pytest.mark.parametrize("tree,n_end", [("a", 12), ("ba", 12), ("bba", 11)])
def test_one_ball_at_the_origin(tree, n_end, case):
    """The force of a plane wave on one ball is along p^ and equals the momentum balance to rounding: no translation, nothing is
    truncated once the degrees the wave excites are all there (k rho = 1.3: the products c_n c_{n+1} from degree 10 on are below
    1e-16 of the leading one).  Measured over the two cases: transverse parts at most 4e-16 (a), 2.1e-15 (ba), 1.1e-15 (bba) of the
    force, momentum balance 8.2e-16 (a), 2.3e-15 (ba), 5.5e-15 (bba).  (The chain d = 5 is left to the table test and the GPU tests:
    the harness of its harmonics is itself good to 1e-14 only.)"""
    d = O.tree(tree).d
    p = geometry(d)[2]
    uin, ugr = O.plane_wave(K, p)
    a, b = COEFFICIENTS[case]
    res = O.solve_biem(tree, centers=np.zeros((1, d)), radii=[1.0], k=K, n_end=n_end, alpha=a, beta=b, uin=uin, uin_grad=ugr)
    phi = FY.force(res, a, b, coupling(tree, n_end))[0]
    balance = FY.momentum_balance(res, uin, ugr, p, a, b, n_end + 2)
    along = phi @ p
    across = np.abs(phi - along * p).max()
    err = np.abs(phi - balance).max() / along
    print(f"{tree} {case}: Phi {phi}  transverse / parallel {across / along:.1e}  momentum balance {err:.1e}")
    assert along > 0 and across <= 1e-14 * along
    assert err <= 10 * {"a": 8.2e-16, "ba": 2.3e-15, "bba": 5.5e-15}[tree]


@pytest.mark.parametrize("tree", ["a", "ba"])
def test_mirror_symmetric_pair(tree):
    """Two equal balls on the first axis, the wave across it: the axial forces are equal and opposite (the secondary Bjerknes force),
    the transverse ones equal.  The mirror image of the solution solves the same system, so the two differ by the rounding of the
    solve: 1e-12 of the force leaves four digits to its conditioning."""
    d = O.tree(tree).d
    cen = np.zeros((2, d))
    cen[0, 0], cen[1, 0] = -1.4, 1.4
    p = np.eye(d)[1]
    uin, ugr = O.plane_wave(K, p)
    res = O.solve_biem(tree, centers=cen, radii=[0.8, 0.8], k=K, n_end=8, uin=uin, uin_grad=ugr)
    phi = FY.force(res, 1.0, 0.0, coupling(tree, 8))
    print(tree, phi)
    scale = np.abs(phi).max()
    assert abs(phi[0, 0]) > 1e-3 * scale                                           # there is an interaction force to compare
    assert abs(phi[0, 0] + phi[1, 0]) <= 1e-12 * scale
    assert np.abs(phi[0, 1:] - phi[1, 1:]).max() <= 1e-12 * scale


# ---------------------------------------------------------------------------- the plan's coupling table
def _host_plan(lib, tree, n_end):
    p = C.c_void_p()
    if tree in _lib.TREE_IDS:
        _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS[tree], n_end, C.byref(p)), "biem_plan_create_host")
    else:
        _lib.check(lib.biem_plan_create_chain_host(len(tree) + 1, n_end, C.byref(p)), "biem_plan_create_chain_host")
    return p


def _force_terms(lib, plan):
    d, H = C.c_int(), C.c_int()
    _lib.check(lib.biem_plan_info(plan, C.byref(d), C.byref(H), None, None, None))
    n = C.c_longlong(-1)
    _lib.check(lib.biem_plan_force_terms(plan, C.byref(n), None, None, None, None), "biem_plan_force_terms")
    ptr = np.zeros(H.value + 1, dtype=np.int64)
    col, comp = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
    val = np.zeros(n.value, dtype=np.complex128)
    _lib.check(lib.biem_plan_force_terms(plan, None, ptr.ctypes.data, col.ctypes.data, comp.ctypes.data, val.ctypes.data), "biem_plan_force_terms")
    return d.value, H.value, ptr, col, comp, val


# every tree the plans cover: the four built trees and the chains d = 5 .. 10 (d >= 7 up to n_end 2: beyond, the harness' dense table
# is the cost; the pruning of candidates by label entries is exercised by every label position of the longest chain there)
@pytest.mark.parametrize("tree,n_end", [(tr, n) for tr in ("a", "ba", "bba", "caa", "bbba", "bbbba") for n in (1, 2, 5)]
                         + [("b" * (d - 2) + "a", n) for d in (7, 8, 9, 10) for n in (1, 2)])
def test_coupling_table_of_the_plan(tree, n_end):
    lib = _lib.load()
    plan = _host_plan(lib, tree, n_end)
    try:
        d, H, ptr, col, comp, val = _force_terms(lib, plan)
    finally:
        lib.biem_plan_destroy(plan)
    ref = coupling(tree, n_end)
    with registered(tree) as tr:
        deg = tr.degrees(n_end)
    assert ref.shape == (d, H, H) and ptr[0] == 0 and ptr[-1] == len(col) and (np.diff(ptr) >= 0).all()
    rows = np.repeat(np.arange(H), np.diff(ptr))
    dense = np.zeros((d, H, H), dtype=np.complex128)
    dense[comp, rows, col] = val
    assert len(set(zip(comp.tolist(), rows.tolist(), col.tolist()))) == len(col)                    # no entry twice
    key = (rows.astype(np.int64) * d + comp) * H + col
    assert (np.diff(key) > 0).all()                                                                # ordered by (row, component, column)
    err = np.abs(dense - ref).max() if H else 0.0
    print(f"{tree} n_end {n_end}: {len(col)} entries of {d * H * H}, |plan - yardstick| {err:.1e}")
    assert err <= 1e-13
    assert (np.abs(deg[rows] - deg[col]) == 1).all()                                               # nothing off |n - n'| = 1
    assert (np.abs(val) > 1e-14).all()
    assert np.abs(dense - np.conj(np.swapaxes(dense, 1, 2))).max() <= 1e-13                        # Hermitian in (h', h)
    if n_end == 1:
        assert len(col) == 0 and H == 1                                                            # one harmonic: no neighbour degree, no force


# ---------------------------------------------------------------------------- public surface and argument checks
def test_exported_and_method_of_the_calculator():
    assert "biem_force" in amd.__all__ and callable(amd.biem_force)
    assert callable(amd.BIEMResultCalculator.force)
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")
    doc = amd.biem_force.__doc__
    assert "uin_grad" in doc and "rho_0 omega^2" in doc                            # needs no incident field; the physical force


def test_argument_errors_come_before_any_device_work():
    with pytest.raises(ValueError, match="Invalid kind: inner"):
        amd.biem_force(_result(kind="inner"))
    with pytest.raises(ValueError, match="Im k must be zero"):
        amd.biem_force(_result(k=np.array(1.0 + 0.1j)))
    with pytest.raises(ValueError, match="Im k must be zero"):
        amd.biem_force(_result(k=np.array([1.0, 1.0 + 1e-300j])))                 # any system
    with pytest.raises(ValueError) as e:
        amd.biem_force(_result(density=None))
    assert str(e.value) == "The BIEMResult does not have density."
    with pytest.raises(ValueError, match="alpha_n"):
        amd.biem_force(_result(), alpha=2.0, alpha_n=np.ones((1, 3)))             # _validate_degree_bc: not both forms
    with pytest.raises(TypeError):
        amd.biem_force(_result(), 1.0)                                             # the coefficients are keywords
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types("ba"), centers=np.zeros((3, 1)), radii=np.ones(1), k=np.array(1.0),
                                    n_end=3, eta=np.array(1.0), kind="outer")
    with pytest.raises(ValueError, match="does not have density"):
        calc.force()


# ---------------------------------------------------------------------------- the C ABI
def test_header_declares_the_entries_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    plain, per_degree = _params(hdr, "biem_force"), _params(hdr, "biem_force_n")
    assert len(plain) == len(per_degree) == len(_lib.SIGNATURES["biem_force"][1]) == 15
    assert _lib.SIGNATURES["biem_force"] == _lib.SIGNATURES["biem_force_n"]
    assert [p[:-1] for p in plain] == [p[:-1] for p in per_degree]                 # the same types
    names = [p[-1].lstrip("*") for p in plain]
    assert names == ["plan", "nb", "B", "nrhs", "d_k", "d_eta", "d_radii", "geom_batched", "d_alpha", "d_beta", "ab_batched", "d_tab",
                     "d_density", "d_out", "stream"]
    assert [p[-1].lstrip("*") for p in per_degree] == [n + "_n" if n in ("d_alpha", "d_beta") else n for n in names]
    for (types_, name), ctype in zip(((p[:-1], p[-1]) for p in plain), _lib.SIGNATURES["biem_force"][1]):
        assert (ctype is _lib._i) == (types_ == ["int"]), (name, types_)         # ints are ints, everything else a pointer
    terms = _params(hdr, "biem_plan_force_terms")
    assert [p[-1].lstrip("*") for p in terms] == ["plan", "n_entries", "h_ptr", "h_col", "h_comp", "h_val"]
    assert len(_lib.SIGNATURES["biem_plan_force_terms"][1]) == len(terms)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "biem_force" in text and "biem_force_n" in text and "biem_plan_force_terms" in text


def test_library_cross_compiles_and_exports_the_entries():
    _build.build(force=False)                       # every translation unit for gfx950 (a no-op when the library matches the sources)
    assert not _build.is_stale()
    assert "kernels_force.hip" in _build.SOURCES
    lib = _lib.load()
    for name in ("biem_force", "biem_force_n"):
        fn = getattr(lib, name)
        rc = fn(*([None, 1, 1, 1] + [None] * 3 + [0] + [None] * 2 + [0] + [None] * 4))        # no plan: an argument error, no device touched
        assert rc == 1 and b"plan" in lib.biem_last_error() and name.encode() in lib.biem_last_error()
    assert lib.biem_plan_force_terms(None, None, None, None, None, None) == 1 and b"plan" in lib.biem_last_error()


def test_force_kernel_uses_no_scratch():
    """k_force in the gfx950 code object: no private segment (one accumulator per component pass, j_n in LDS), no spills."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    assert objdump and readelf
    _lib.load()
    with tempfile.TemporaryDirectory(prefix="biem_force_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        metas = {}
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            metas.update(_build._kernel_meta(readelf, os.path.join(tmp, o)))
    force = [m for n, m in metas.items() if "k_force" in n]
    assert len(force) == 1, sorted(metas)
    print(force[0])
    assert int(force[0]["private_segment_fixed_size"]) == 0 and int(force[0]["vgpr_spill_count"]) == 0 and int(force[0]["sgpr_spill_count"]) == 0
