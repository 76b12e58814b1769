"""CPU tests of uscat_hess(): the public surface, the argument checks that run before any device work, the C declaration, the code
object of the ladder kernel (cross-compiled for gfx950), and the yardsticks of tests/test_gpu_field_hessian.py: the NumPy twin of the
coefficient ladder (tests/hess_yardstick.py, with the plan's own coupling table) and the 40-digit fixture
tests/golden/hess_fields.npz (tools/make_hess_fixtures.py), tied to each other and to the golden-pinned fp64 oracle.
"""
import json
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _biem, _build, _lib
from biem_helmholtz_sphere_amd._coords import harm_count
from oracle import biem_oracle as O

import hess_yardstick as HY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hess_fields.npz")
PARITY_TOL = 1e-10                      # the project's parity contract
C8 = (4.0 / 5.0, -1.0 / 5.0, 4.0 / 105.0, -1.0 / 280.0)


def load_cases():
    """{id: namespace(tree, kind, n_end, k, eta, centers, radii, density, x, valid, hess)} of the fixture (read once, never modified)."""
    out = {}
    with np.load(FIXTURE, allow_pickle=False) as z:
        for cid in json.loads(str(z["cases"])):
            meta = json.loads(str(z[cid + "/meta"]))
            k = complex(*meta["k"])
            rec = types.SimpleNamespace(id=cid, tree=meta["tree"], kind=meta["kind"], n_end=meta["n_end"], k=k if k.imag else k.real,
                                        eta=meta["eta"], **{n: z[f"{cid}/{n}"] for n in ("centers", "radii", "density", "x", "valid", "hess")})
            out[cid] = rec
    return out


CASES = load_cases() if os.path.exists(FIXTURE) else {}


def _result(bt, n_end, **kw):
    c = amd.create_from_branching_types(bt)
    d = c.c_ndim
    base = dict(c=c, centers=np.zeros((d, 1)), radii=np.ones(1), k=np.float64(1.0), eta=np.float64(1.0), kind="outer",
                density=np.ones((1, harm_count(bt, n_end)), dtype=np.complex128))
    base.update(kw)
    return types.SimpleNamespace(**base)


# ---------------------------------------------------------------------------- the public surface
def test_exported_and_a_method_of_the_calculator():
    assert "biem_u_hess" in amd.__all__ and "biem_u_hess" in _biem.__all__ and callable(amd.biem_u_hess)
    assert callable(amd.BIEMResultCalculator.uscat_hess) and callable(amd.BIEMResultCalculatorProtocol.uscat_hess)
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")
    with pytest.raises(TypeError):
        amd.biem_u_hess(_result("ba", 3), np.zeros((3, 2)), far_field=True)      # a pattern has no Hessian in space: not an argument


def test_argument_errors_come_before_any_device_work():
    x = np.zeros((3, 2))
    with pytest.raises(ValueError) as e:
        amd.biem_u_hess(_result("ba", 3, density=None), x)
    assert str(e.value) == "The BIEMResult does not have density."
    with pytest.raises(ValueError, match="Invalid kind: middle"):
        amd.biem_u_hess(_result("ba", 3, kind="middle"), x)
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types("ba"), centers=np.zeros((3, 1)), radii=np.ones(1), k=1.0, n_end=3,
                                    eta=1.0, kind="outer")
    with pytest.raises(ValueError, match="does not have density"):
        calc.uscat_hess(x)
    with pytest.raises(NotImplementedError) as e:                                # 2 (159 + 2) = 322 > 320, the radial tables
        amd.biem_u_hess(_result("ba", 159), x)
    assert "n_end + 2 = 161" in str(e.value) and "322" in str(e.value)


# ---------------------------------------------------------------------------- the C entry
def _params(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split() for p in m.group(1).split(",")]


def test_header_declares_the_entry_with_the_arguments_of_biem_uscat():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    hess, val = _params(hdr, "biem_uscat_hess"), _params(hdr, "biem_uscat")
    assert len(hess) == len(_lib.SIGNATURES["biem_uscat_hess"][1]) == 16
    assert [p[-1] for p in hess] == [p[-1] for p in val]                         # the names
    assert [p[:-1] for p in hess[1:]] == [p[:-1] for p in val[1:]]               # the types ...
    assert hess[0][:-1] == ["biem_plan*"] and val[0][:-1] == ["const", "biem_plan*"]   # ... but the plan: the first call builds its force table
    assert _lib.SIGNATURES["biem_uscat_hess"] == _lib.SIGNATURES["biem_uscat"]
    assert re.search(r"\bsize_t biem_uscat_hess_workspace_bytes\(const biem_plan\* plan, int nb, int B\);", hdr)
    assert len(_lib.SIGNATURES["biem_uscat_hess_workspace_bytes"][1]) == 3
    assert "biem_uscat_hess" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_library_cross_compiles_and_exports_the_entry():
    _build.build(force=False)                       # every translation unit for gfx950 (a no-op when the library matches the sources)
    assert not _build.is_stale() and "kernels_ladder.hip" in _build.SOURCES
    lib = _lib.load()
    rc = lib.biem_uscat_hess(None, 1, 1, 1, None, None, None, None, 0, None, None, 0, None, None, 0, None)   # no plan: no device touched
    assert rc != _lib.BIEM_OK and b"plan" in lib.biem_last_error() and b"biem_uscat_hess" in lib.biem_last_error()
    assert lib.biem_uscat_hess_workspace_bytes(None, 1, 1) == 0


def test_ladder_kernel_uses_no_scratch():
    """k_coef_ladder in the gfx950 code object: one instance, no private segment, no spills; its name matches none of the substrings
    other tests count kernels by."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    assert objdump and readelf
    _lib.load()
    with tempfile.TemporaryDirectory(prefix="biem_hess_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        metas = {}
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            metas.update(_build._kernel_meta(readelf, os.path.join(tmp, o)))
    mine = {n: m for n, m in metas.items() if "k_coef_ladder" in n}
    assert len(mine) == 1, sorted(mine)
    (name, m), = mine.items()
    print(name, m)
    assert not any(s in name for s in ("k_uscat_grad_fast", "k_uscat_fastI", "k_uinterior", "k_interior_coef", "k_power", "k_force"))
    assert int(m["vgpr_spill_count"]) == 0 and int(m["sgpr_spill_count"]) == 0 and int(m["private_segment_fixed_size"]) == 0, m


# ---------------------------------------------------------------------------- the twin: the ladder in coefficient space
# (tree of the plan, n_end of c, k); bpa and bpbpa are ba and bba in permuted axes (one plan each), so they run the ladder of the
# canonical tree at another order and wavenumber
TRACE_CASES = [("a", "a", 5, 1.3), ("ba", "ba", 4, 1.3), ("bpa", "ba", 5, 1.1 + 0.2j), ("bba", "bba", 3, 1.3), ("bpbpa", "bba", 2, 0.7),
               ("caa", "caa", 3, 1.3), ("bbba", "bbba", 3, 1.3), ("bbbba", "bbbba", 2, 1.3)]
TRACE_TOL = 10 * 2.6e-14          # ten times the largest figure measured (docstring below): the sum is rounding only


@pytest.mark.parametrize("name,tree,n_end,k", TRACE_CASES, ids=[c[0] for c in TRACE_CASES])
def test_ladder_twice_is_the_helmholtz_operator(name, tree, n_end, k):
    """sum_i D_i D_i c = -k^2 c and D_j D_i c = D_i D_j c with the plan's own table and random c (two sets; real and imaginary parts
    standard normal, |c_h| ~ 1); D_i c fills the degree n_end and nothing above it.  Rounding only.  Measured, max over h in units of
    |k|^2, residual / commutator: a 1.1e-15 / 6.5e-16, ba 8.4e-15 / 2.1e-15, bpa 3.3e-15 / 1.9e-15, bba 1.1e-14 / 3.2e-15, bpbpa 3.7e-15 /
    9.6e-16, caa 1.1e-14 / 9.7e-15, bbba 2.0e-14 / 1.1e-14, bbbba 2.6e-14 / 1.4e-14 (with the oracle's table in place of the plan's the
    residual was 6.8e-15).  The bound is ten times the largest, 2.6e-13."""
    rng = np.random.default_rng([n_end, len(tree)])
    d, _, deg2, T = HY.plan_table(tree, n_end + 2)
    H = len(HY.plan_table(tree, n_end)[2])
    c = rng.normal(size=(2, H)) + 1j * rng.normal(size=(2, H))
    c2, hc = HY.hessian_coefs(tree, n_end, k, c)
    assert hc.shape == (d, d, 2, len(deg2))
    res = np.abs(sum(hc[i, i] for i in range(d)) + k * k * c2).max() / abs(k) ** 2
    com = np.abs(hc - hc.transpose(1, 0, 2, 3)).max() / abs(k) ** 2
    g = np.stack([HY.ladder(T, deg2, k, c2, i, n_end) for i in range(d)])
    print(f"  {name}: |sum D_i D_i c + k^2 c| = {res:.2e} k^2, |D_j D_i c - D_i D_j c| = {com:.2e} k^2")
    assert (g[..., deg2 > n_end] == 0).all() and np.abs(g[..., deg2 == n_end]).max() > 0.1     # one degree longer, no more
    assert (c2[..., deg2 >= n_end] == 0).all()
    assert res <= TRACE_TOL and com <= TRACE_TOL, (res, com)


# ---------------------------------------------------------------------------- the twin's field against the 40-digit fixture
def test_fixture_holds_the_cases_of_the_issue():
    assert sorted(CASES) == sorted(
        [f"outer-{t}-k1.3" for t in ("a", "ba", "bpa", "bba", "bpbpa", "caa")] + ["outer-a-k1.3+0.2i", "outer-bpbpa-k1.2+0.15i"]
        + [f"inner-{t}-k1.3" for t in ("a", "ba", "bba", "caa")])
    assert os.path.getsize(FIXTURE) < 100 * 1024
    for rec in CASES.values():
        d = rec.x.shape[1]
        assert rec.hess.shape == (d, d, len(rec.x)) and rec.valid[:-1].all() and not rec.valid[-1]
        assert np.isnan(rec.hess[:, :, ~rec.valid]).all() and np.isfinite(rec.hess[:, :, rec.valid]).all()
        assert np.array_equal(rec.hess, rec.hess.transpose(1, 0, 2), equal_nan=True)
        if rec.kind == "inner":
            assert (np.abs(rec.x - rec.centers[0]).max(axis=1) == 0).any()                       # the centre is among the points


@pytest.mark.parametrize("cid", sorted(CASES))
def test_twin_against_the_fixture(cid):
    """The ladder's field - the plan's table, the oracle's radial functions and harmonics at order n_end + 2, all fp64 - against the
    second differences of the 40-digit series: |twin - fixture| <= 1e-10 max |H| (the contract).  Measured: at most 9.6e-15 (outer, caa) and
    2.1e-14 (kind inner, caa) over the twelve cases - the figure of DESIGN.md 5j."""
    rec = CASES[cid]
    got = HY.hessian(rec.tree, rec.n_end, rec.k, rec.eta, rec.kind, rec.centers, rec.radii, rec.density, rec.x[rec.valid])
    want = rec.hess[:, :, rec.valid]
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print(f"  {cid}: |twin - fixture| = {err:.2e} of max|H| = {scale:.3e}")
    assert err <= PARITY_TOL, err


# ---------------------------------------------------------------------------- the fixture against the golden-pinned fp64 oracle
def _oracle_record(rec, mask_factor):
    """The record as an OracleResult whose mask is drawn at mask_factor * rho: the same outgoing coefficients c = density blc_n(rho),
    restated as a density on the sphere of the other radius, so that a stencil around a point near a surface stays unmasked."""
    tr = O.tree(rec.tree)
    radii = rec.radii * mask_factor
    c = HY.near_coefs(rec.tree, rec.n_end, rec.k, rec.eta, rec.radii, rec.density, rec.kind)
    unit = HY.near_coefs(rec.tree, rec.n_end, rec.k, rec.eta, radii, np.ones_like(rec.density), rec.kind)
    return O.OracleResult(tr, rec.n_end, rec.k, rec.eta, rec.centers, radii, c / unit, None, None, None, rec.kind)


def _nested_stencil(res, x, h):
    """[d, d, P]: the 8th-order central first difference of O.uscat applied twice."""
    P, d = x.shape
    offs = [(s * q * h, s * cq / h) for q, cq in enumerate(C8, start=1) for s in (1.0, -1.0)]
    H = np.zeros((d, d, P), dtype=np.complex128)
    for i in range(d):
        for j in range(i, d):
            pts = np.stack([x + a * np.eye(d)[i] + b * np.eye(d)[j] for a, _ in offs for b, _ in offs])
            w = np.array([wa * wb for _, wa in offs for _, wb in offs])
            H[i, j] = H[j, i] = np.tensordot(w, O.uscat(res, pts), axes=1)
    return H


STENCIL_TOL = 1e-9                # the two stencils among themselves; measured at most 5.6e-10 (docstring below)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_fixture_against_the_oracle_stencil(cid):
    """Ties the 40-digit values to the fp64 oracle that the reference's goldens pin.  The nested 8th-order stencil of O.uscat at h = 1e-2
    and at h = 5e-3 must agree with each other within 1e-9 of max |H|, then the fixture with the stencil at h = 5e-3 within ten times
    that.  Measured (agreement / fixture against h = 5e-3): 2-D 2.0e-11 / 2.1e-11 at most, 3-D 5.6e-10 / 5.2e-10 (kind inner, ba; outer
    2.1e-10 / 1.9e-10), 4-D 5.4e-10 / 5.1e-10 (kind inner, bba; outer 1.5e-10 / 1.5e-10).  Both figures are the rounding eps / h^2 of the
    smaller step (the fixture lies as far from it as the larger step does): the stencil's own error, not the fixture's."""
    rec = CASES[cid]
    res = _oracle_record(rec, 0.5 if rec.kind == "outer" else 2.0)
    x = rec.x[rec.valid]
    assert np.abs(O.uscat(res, x) - O.uscat(_oracle_record(rec, 1.0), x)).max() <= 1e-13 * np.abs(O.uscat(res, x)).max()   # the same field
    h1, h2 = _nested_stencil(res, x, 1e-2), _nested_stencil(res, x, 5e-3)
    want = rec.hess[:, :, rec.valid]
    scale = np.abs(want).max()
    agree, err = np.abs(h1 - h2).max() / scale, np.abs(h2 - want).max() / scale
    print(f"  {cid}: stencils h=1e-2 / 5e-3 agree within {agree:.2e}, |fixture - stencil(5e-3)| = {err:.2e} of max|H| = {scale:.3e}")
    assert np.isfinite(h2).all()
    assert agree <= STENCIL_TOL, agree
    assert err <= 10 * STENCIL_TOL, err
