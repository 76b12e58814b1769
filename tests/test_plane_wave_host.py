"""CPU tests of plane-wave incidence in closed form: the yardstick (tests/plane_wave_yardstick.py) against the oracle's projection under
a fine rule, the same closed form on the chain trees through the plan's host tables, the argument checks of
``plane_wave_direction`` that run before any device work, and the C declarations.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _build, _lib
from oracle import biem_oracle as O

import plane_wave_yardstick as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = {"a": 8, "ba": 6, "bpa": 6, "bba": 4, "bpbpa": 4, "caa": 4}       # tree -> n_end
KS = (1.3, 0.9 + 0.3j)
RHO = 0.7


def ball(d):
    """A ball off the origin and a direction with every component non-zero."""
    return 0.3 + 0.25 * np.arange(d), np.array([0.6, -0.5, 0.4, 0.3])[:d]


# ---------------------------------------------------------------------------- the yardstick on the oracle
@pytest.mark.parametrize("tree", sorted(TREES))
def test_closed_form_is_the_projection_under_a_fine_rule(tree):
    """U and V of the closed form against the oracle's projection with the 4 n_end-point rule: 1e-13 of max |U| and max |V| (measured when
    the feature was written: 1.8e-14).  The oracle's own n_end-point rule, what the sampled path computes, is off by more than 1e-9 at
    k = 1.3: the reason for the closed form."""
    tr, n_end = O.tree(tree), TREES[tree]
    c, p = ball(tr.d)
    for k in KS:
        U, V = PW.projections(tr, n_end, k, c, RHO, p)
        Uf, Vf = PW.quadrature_projections(tr, n_end, k, c, RHO, p, 4 * n_end)
        Uc, Vc = PW.quadrature_projections(tr, n_end, k, c, RHO, p, n_end)
        eu, ev = np.abs(U - Uf).max() / np.abs(Uf).max(), np.abs(V - Vf).max() / np.abs(Vf).max()
        au, av = np.abs(Uc - Uf).max() / np.abs(Uf).max(), np.abs(Vc - Vf).max() / np.abs(Vf).max()
        print(f"{tree} n_end {n_end} k {k}: closed form vs fine rule {eu:.1e} {ev:.1e}; n_end-point rule vs fine rule {au:.1e} {av:.1e}")
        assert eu <= 1e-13 and ev <= 1e-13
        if k == 1.3:
            assert max(au, av) > 1e-9


def test_rhs_is_minus_alpha_u_minus_beta_v_with_scalar_ball_and_degree_coefficients():
    tr, n_end, k = O.tree("ba"), 6, 0.9 + 0.3j
    cen, rad, p = np.array([[0.1, 0.2, 0.3], [2.5, 0.5, 0.0]]), np.array([1.0, 0.7]), np.array([0.6, -0.5, 0.4])
    deg = tr.degrees(n_end)
    rng = np.random.default_rng(3)
    for al, be in ((1.0 + 0.5j, 0.3 - 0.2j), (np.array([0.4 + 0.1j, 1.0]), np.array([1.0, 0.0])),
                   (rng.normal(size=(2, n_end)) + 1j * rng.normal(size=(2, n_end)), rng.normal(size=(2, n_end)) + 0j)):
        f = PW.rhs(tr, n_end, k, cen, rad, al, be, p)
        for b in range(2):
            U, V = PW.projections(tr, n_end, k, cen[b], rad[b], p)
            a_, b_ = (np.broadcast_to(np.asarray(v)[b] if np.ndim(v) else v, (n_end,) if np.ndim(v) == 2 else ()) for v in (al, be))
            a_, b_ = (v[deg] if np.ndim(v) else v for v in (a_, b_))
            assert np.abs(f[b] + a_ * U + b_ * V).max() <= 1e-14 * np.abs(f[b]).max()


# ---------------------------------------------------------------------------- chain trees: the plan's host tables
def _chain_closed_form_error(d, n_end=8, k=0.8, rho=0.5, cut=4):
    """Project e^{i k p^.(c + rho y_q)} with the plan's W (k rho = 0.4) and compare the degrees < cut with C_d i^n z_n conj(Y_h(p^)) e^{i k p^.c},
    p^ a node of the plan's own rule, so that conj(Y_h(p^)) = W[q*][h] / w_q* needs no second implementation of the chain harmonics.
    Returns the difference relative to the largest coefficient."""
    lib = _lib.load()
    plan = C.c_void_p()
    _lib.check(lib.biem_plan_create_chain_host(d, n_end, C.byref(plan)), "biem_plan_create_chain_host")
    try:
        dd, H, Q = C.c_int(), C.c_int(), C.c_int()
        _lib.check(lib.biem_plan_info(plan, C.byref(dd), C.byref(H), C.byref(Q), None, None))
        H, Q = H.value, Q.value
        deg = np.zeros(H, dtype=np.int32)
        _lib.check(lib.biem_plan_labels_n(plan, d - 1, None, deg.ctypes.data))
        y, w = np.zeros((Q, d)), np.zeros(Q)
        _lib.check(lib.biem_plan_quadrature(plan, y.ctypes.data, w.ctypes.data))
        W = np.zeros((Q, H), dtype=np.complex128)
        _lib.check(lib.biem_plan_projection(plan, W.ctypes.data))
    finally:
        lib.biem_plan_destroy(plan)
    low = deg < cut
    W = W[:, low]
    qs = int(np.argmax(np.min(np.abs(y), axis=1)))                    # the node furthest from every coordinate plane
    p, c = y[qs], 0.3 + 0.25 * np.arange(d)
    Yc = W[qs] / w[qs]
    proj = np.exp(1j * k * ((c[None, :] + rho * y) @ p)) @ W
    z = O.radial_h(cut - 1, d, k * rho)[0]
    closed = PW.c_d(d) * 1j ** deg[low] * z[deg[low]] * Yc * np.exp(1j * k * (p @ c))
    return float(np.abs(proj - closed).max() / np.abs(closed).max())


CHAIN_BA_MEASURED = 4.1e-16        # _chain_closed_form_error(3), measured when the feature was written
CHAIN_TOLERANCE = 4 * CHAIN_BA_MEASURED


@pytest.mark.parametrize("d", [5, 6])
def test_closed_form_on_chain_trees_through_the_plan_s_tables(d):
    """The comparison of _chain_closed_form_error on ba through biem_plan_create_chain_host(3, 8), where the twin is pinned by the test
    above, gives CHAIN_BA_MEASURED = 4.1e-16 (measured: 4.03e-16); d = 5 and d = 6 are held to four times that, 1.64e-15 (measured:
    5.6e-16 at d = 5)."""
    base = _chain_closed_form_error(3)
    err = _chain_closed_form_error(d)
    print(f"d {d}: {err:.2e}  (ba through the same route: {base:.2e})")
    assert base <= CHAIN_TOLERANCE
    assert err <= CHAIN_TOLERANCE


# ---------------------------------------------------------------------------- argument checks
def test_argument_errors_come_before_any_device_work():
    c = amd.create_from_branching_types("ba")
    kw = dict(centers=np.zeros((2, 3)), radii=np.ones(2), k=np.array(1.0), n_end=3)
    wave = lambda x: np.ones(x.shape[1:])
    for extra in (dict(uin=wave), dict(uin_grad=wave), dict(uin=wave, uin_grad=wave)):
        with pytest.raises(ValueError, match="plane_wave_direction replaces uin / uin_grad"):
            amd.biem(c, plane_wave_direction=np.ones(3), **extra, **kw)
    with pytest.raises(ValueError, match="c.c_ndim=3"):
        amd.biem(c, plane_wave_direction=np.ones(2), **kw)
    with pytest.raises(ValueError, match="is not k.ndim \\+ 1"):
        amd.biem(c, plane_wave_direction=np.ones((3, 2)), **kw)
    with pytest.raises(ValueError, match="zero vector"):
        amd.biem(c, plane_wave_direction=np.zeros(3), **kw)
    with pytest.raises(ValueError, match="zero vector"):
        amd.biem(c, plane_wave_direction=np.array([[1, 0], [0, 0], [0, 0]]), **{**kw, "k": np.array([1.0])})      # any column
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            amd.biem(c, plane_wave_direction=np.array([1.0, bad, 0.0]), **kw)
    assert "plane_wave_direction" in amd.biem.__doc__ and "plane_wave_direction" in amd.BIEMFactorization.solve.__doc__


# ---------------------------------------------------------------------------- the C ABI
def _params(text, ret, name):
    m = re.search(r"\b%s %s\(([^;]*?)\);" % (ret, name), text, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split() for p in m.group(1).split(",")]


def test_header_declares_the_entries_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    names = lambda ps: [p[-1].lstrip("*") for p in ps]
    whole = ["plan", "nb", "B", "nrhs", "d_k", "d_eta", "d_centers", "d_radii", "geom_batched", "d_alpha", "d_beta", "ab_batched", "per_degree",
             "d_dirs", "dirs_batched", "d_density", "d_info", "chunk", "d_work", "work_bytes", "stream"]
    expected = {
        "biem_rhs_plane_wave": ["plan", "nb", "B", "nrhs", "d_k", "d_centers", "geom_batched", "d_tab", "d_dirs", "dirs_batched", "d_f",
                                "sys_stride", "elem_stride", "rhs_stride", "d_work", "work_bytes", "stream"],
        "biem_solve_pw": whole,
        "biem_solve_ldlt_pw": whole,
        "biem_solve_factored_pw": ["plan", "nb", "B", "nrhs", "d_F", "lda", "sys_stride", "d_tab", "d_k", "d_centers", "geom_batched", "d_alpha",
                                   "d_beta", "ab_batched", "per_degree", "d_dirs", "dirs_batched", "d_density", "d_work", "work_bytes", "stream"],
    }
    for name, want in expected.items():
        ps = _params(hdr, "int", name)
        assert names(ps) == want, name
        ctypes_ = _lib.SIGNATURES[name][1]
        assert len(ctypes_) == len(ps)
        for p, ct in zip(ps, ctypes_):
            kind = _lib._i if p[:-1] == ["int"] else _lib._ll if p[:-1] == ["long", "long"] else _lib._sz if p[:-1] == ["size_t"] else _lib._vp
            assert ct is kind, (name, p)
    assert _lib.SIGNATURES["biem_solve_pw"] == _lib.SIGNATURES["biem_solve_ldlt_pw"]
    ps = _params(hdr, "size_t", "biem_rhs_plane_wave_workspace_bytes")
    assert names(ps) == ["plan", "nb", "nrhs", "dirs_batched"] and _lib.SIGNATURES["biem_rhs_plane_wave_workspace_bytes"][0] is _lib._sz
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in list(expected) + ["biem_rhs_plane_wave_workspace_bytes"]:
        assert name in text, name


def test_library_cross_compiles_and_exports_the_entries():
    _build.build(force=False)
    assert not _build.is_stale()
    assert "kernels_rhs_pw.hip" in _build.SOURCES
    lib = _lib.load()
    assert lib.biem_rhs_plane_wave_workspace_bytes(None, 4, 5, 0) == 0
    for name in ("biem_rhs_plane_wave", "biem_solve_pw", "biem_solve_ldlt_pw", "biem_solve_factored_pw"):
        args = [0 if t is _lib._i or t is _lib._ll or t is _lib._sz else None for t in _lib.SIGNATURES[name][1]]
        rc = getattr(lib, name)(*args)                                   # no plan, no directions: an argument error, no device touched
        assert rc == 1 and name.encode() in lib.biem_last_error(), (name, lib.biem_last_error())
