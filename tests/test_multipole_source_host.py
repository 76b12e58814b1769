"""CPU tests of multipole incidence in closed form: the yardstick (tests/multipole_source_yardstick.py) against the projection of the
sampled multipole under fine rules, the index of degree 0 against the point-source yardstick, the same closed form on the chain trees
through the plan's own term lists, the argument checks of ``multipole_source_position`` / ``multipole_source_index`` that run before any
device work, and the C declarations.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.special as sp

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _build, _lib
from oracle import biem_oracle as O

import chain_yardstick as CY
import multipole_source_yardstick as MS
import point_source_yardstick as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1.3, 0.9 + 0.3j)
RHO, DIST = 0.7, 1.58
N_END = {"a": 6, "ba": 5, "bba": 4, "caa": 3}


def ball_and_source(d):
    """A ball off the origin and a source DIST from its centre, every component of c - s non-zero."""
    c, t = 0.3 + 0.25 * np.arange(d), np.array([1.1, -0.9, 0.7, 0.5])[:d]
    return c, c - DIST * t / np.linalg.norm(t)


# ---------------------------------------------------------------------------- a. the yardstick on the oracle
@pytest.mark.parametrize("tree", ["a", "ba", "bba", "caa"])
def test_closed_form_is_the_projection_under_fine_rules(tree):
    """U of the closed form, row h' of O.translation_SR times j_n(k rho), against the projection of the sampled multipole under the
    10 n_end-point rule, for sources of degree 0, of degree 1, the conjugate partner and the top degree: 1e-12 of the row's largest entry
    (measured on the oracle when the feature was written, real k: at most 1.2e-14).  The n_end-point rule's defect, what the sampled
    path would compute, is printed."""
    tr, n_end = O.tree(tree), N_END[tree]
    c, s = ball_and_source(tr.d)
    assert (np.abs(c - s) > 0.3).all()
    z = np.linspace(0.4, 3.0, 7)
    for k in KS:
        for n in (0, 1, n_end - 1):                                              # the whole-array radial function is O.radial_h's
            slow = np.array([O.radial_h(max(n, 1), tr.d, k * v)[1][n] for v in z])
            assert np.abs(MS.outgoing_radial(n, tr.d, k * z) - slow).max() <= 1e-14 * np.abs(slow).max()
        worst = 0.0
        for hp in MS.source_indices(tr, n_end):
            U, _ = MS.projections(tr, n_end, k, c, RHO, s, hp)
            fine = MS.quadrature_projections(tr, n_end, k, c, RHO, s, hp, 10 * n_end)
            coarse = MS.quadrature_projections(tr, n_end, k, c, RHO, s, hp, n_end)
            err = np.abs(U - fine).max() / np.abs(fine).max()
            worst = max(worst, err)
            print(f"{tree} k {k} h' {hp} (degree {tr.degrees(n_end)[hp]}): closed form vs the 10 n_end rule {err:.1e}; "
                  f"the n_end rule's defect {np.abs(coarse - fine).max() / np.abs(fine).max():.1e}")
            assert err <= 1e-12, (tree, k, hp, err)
        print(f"{tree} k {k}: worst {worst:.1e}")


@pytest.mark.parametrize("tree", ["a", "ba", "bba", "caa"])
def test_index_of_degree_zero_is_the_point_source_times_y0(tree):
    tr, n_end = O.tree(tree), N_END[tree]
    d = tr.d
    cen = np.stack([0.3 + 0.25 * np.arange(d), 2.4 - 0.2 * np.arange(d)])
    rad = np.array([0.7, 0.5])
    s = cen[0] + 1.58 * np.array([1.1, -0.9, 0.7, 0.5])[:d] / np.linalg.norm(np.array([1.1, -0.9, 0.7, 0.5])[:d])
    Y0 = tr.harmonics(np.eye(d)[:1], 1)[0, 0]
    assert abs(Y0 - 1.0 / np.sqrt(2.0 * np.pi ** (d / 2.0) / math.gamma(d / 2.0))) <= 1e-15
    h0 = MS.source_indices(tr, n_end)[0]
    for k in KS:
        for al, be in ((1.0 + 0.5j, 0.3 - 0.2j), (np.array([0.4 + 0.1j, 1.0]), np.array([1.0, 0.0]))):
            f = MS.rhs(tr, n_end, k, cen, rad, al, be, s, h0)
            want = Y0 * PS.rhs(tr, n_end, k, cen, rad, al, be, s)
            err = np.abs(f - want).max() / np.abs(want).max()
            print(f"{tree} k {k}: degree-0 multipole vs Y_0 x point source {err:.1e}")
            assert err <= 1e-12


# ---------------------------------------------------------------------------- b. chain trees: the plan's own term lists
def _outgoing(nmax, d, z):
    """h_0 .. h_nmax of dimension d at a real z.  Odd d: h_n = h^sph_{n + (d-3)/2}(z) / z^{(d-3)/2} by SciPy's spherical functions, good to
    1e-16; O.radial_h takes jv / yv of half-integer order there, which at d = 5 and z = 8 (this test's k |t|) are off by 4e-15 .. 9e-15
    against 40-digit values - more than the tolerance below.  Even d: O.radial_h (integer orders: 1e-16)."""
    if d % 2 == 0:
        return O.radial_h(max(nmax, 1), d, z)[1][:nmax + 1]
    m = np.arange(nmax + 1) + (d - 3) // 2
    return (sp.spherical_jn(m, z) + 1j * sp.spherical_yn(m, z)) / z ** ((d - 3) // 2)


def _chain_closed_form_error(d, n_end=6, k=0.8, rho=0.25, dist=10.0, cut=3):
    """The comparison of test_point_source_host._chain_closed_form_error for a source of degree 1: project the sampled dipole
    h_1(k |x - s|) Y_h'((x - s)^), x = c + rho y_q, with the plan's W and compare the degrees < cut with
    U_h = j_n(k rho) sum_p coef[p] T[tidx[p]] over the plan's term list of entry e = h H + h', T = C_d h_n''(k |t|) Y_l(t^) at t = c - s
    (the labels and harmonics of tests/chain_yardstick.table, the radial functions of _outgoing).  rho / |t| = 0.025 and k rho = 0.2: the rule of order 6 is exact to degree 11, and the content of the
    dipole in degree n falls like 0.025^n, so the aliased degrees >= 10 lie below 1e-15 of the leading one.  h': the last label of degree
    1 (m = 1).  Returns the difference relative to the largest coefficient."""
    lib = _lib.load()
    plan = C.c_void_p()
    _lib.check(lib.biem_plan_create_chain_host(d, n_end, C.byref(plan)), "biem_plan_create_chain_host")
    try:
        dd, H, Q, H2, nt = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(lib.biem_plan_info(plan, C.byref(dd), C.byref(H), C.byref(Q), C.byref(H2), C.byref(nt)))
        H, Q, H2, nt = H.value, Q.value, H2.value, nt.value
        lab, deg = np.zeros((H, d - 1), dtype=np.int32), np.zeros(H, dtype=np.int32)
        _lib.check(lib.biem_plan_labels_n(plan, d - 1, lab.ctypes.data, deg.ctypes.data))
        y, w = np.zeros((Q, d)), np.zeros(Q)
        _lib.check(lib.biem_plan_quadrature(plan, y.ctypes.data, w.ctypes.data))
        W = np.zeros((Q, H), dtype=np.complex128)
        _lib.check(lib.biem_plan_projection(plan, W.ctypes.data))
        ptr, coef, tidx = np.zeros(H * H + 1, dtype=np.int64), np.zeros(nt), np.zeros(nt, dtype=np.int32)
        _lib.check(lib.biem_plan_terms(plan, ptr.ctypes.data, coef.ctypes.data, tidx.ctypes.data))
    finally:
        lib.biem_plan_destroy(plan)
    ch = CY.chain(d)
    assert [tuple(v) for v in lab.tolist()] == [tuple(v) for v in ch.index(n_end)]            # the yardstick's harmonics are the plan's axis
    hp = int(np.nonzero(deg == 1)[0][-1])
    low = np.nonzero(deg < cut)[0]
    c = 0.3 + 0.25 * np.arange(d)
    v = np.array([0.6, -0.5, 0.4, 0.3, -0.35, 0.45, 0.25, -0.3, 0.2, 0.5])[:d]
    s = c - dist * v / np.linalg.norm(v)
    rel = c[None, :] + rho * y - s[None, :]
    r = np.linalg.norm(rel, axis=-1)
    h1 = np.array([_outgoing(1, d, k * ri)[1] for ri in r])
    proj = (h1 * ch.harmonics(rel / r[:, None], n_end)[hp]) @ W[:, low]
    g = CY.gaunt(d, n_end)
    t = c - s
    T = PS.c_d(d) * _outgoing(g.n2 - 1, d, k * dist)[g.deg2] * ch.harmonics((t / dist)[None, :], g.n2)[:, 0]
    assert T.shape == (H2,) and abs(np.linalg.norm(t) - dist) <= 1e-14
    row = np.array([coef[ptr[h * H + hp]:ptr[h * H + hp + 1]] @ T[tidx[ptr[h * H + hp]:ptr[h * H + hp + 1]]] for h in low])
    closed = row * O.radial_h(cut - 1, d, k * rho)[0][deg[low]]
    return float(np.abs(proj - closed).max() / np.abs(closed).max())


CHAIN_BA_MEASURED = 5.6e-16        # _chain_closed_form_error(3), measured when the feature was written (5.55e-16)
CHAIN_TOLERANCE = 4 * CHAIN_BA_MEASURED


@pytest.mark.parametrize("d", [5, 6])
def test_closed_form_on_chain_trees_through_the_plan_s_tables(d):
    """The comparison of _chain_closed_form_error on ba through biem_plan_create_chain_host(3, 6), where the twin is pinned by the tests
    above, gives CHAIN_BA_MEASURED = 5.6e-16 (measured: 5.55e-16); d = 5 and d = 6 are held to four times that, 2.2e-15 (measured:
    1.85e-15 at d = 5, 1.02e-15 at d = 6; with O.radial_h's own h_n at d = 5, off by 5e-15 at this argument, 3.85e-15)."""
    base = _chain_closed_form_error(3)
    err = _chain_closed_form_error(d)
    print(f"d {d}: {err:.2e}  (ba through the same route: {base:.2e})")
    assert base <= CHAIN_TOLERANCE
    assert err <= CHAIN_TOLERANCE


# ---------------------------------------------------------------------------- c. argument checks
def test_argument_errors_come_before_any_device_work():
    c = amd.create_from_branching_types("ba")
    kw = dict(centers=np.zeros((2, 3)), radii=np.ones(2), k=np.array(1.0), n_end=3)
    wave = lambda x: np.ones(x.shape[1:])
    far = np.array([5.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="must be given together"):
        amd.biem(c, multipole_source_position=far, **kw)
    with pytest.raises(ValueError, match="must be given together"):
        amd.biem(c, multipole_source_index=1, **kw)
    for extra in (dict(uin=wave), dict(uin_grad=wave), dict(plane_wave_direction=np.ones(3)), dict(point_source_position=far)):
        with pytest.raises(ValueError, match="multipole_source_position replaces uin / uin_grad / plane_wave_direction / point_source_position"):
            amd.biem(c, multipole_source_position=far, multipole_source_index=1, **extra, **kw)
    for bad in (1.0, np.array([1.5]), np.array([True])):
        with pytest.raises(ValueError, match="integer"):
            amd.biem(c, multipole_source_position=far, multipole_source_index=bad, **kw)
    for bad in (9, -1, np.array(12)):
        with pytest.raises(ValueError, match=r"\[0, H\) with H=9"):
            amd.biem(c, multipole_source_position=far, multipole_source_index=bad, **kw)
    with pytest.raises(ValueError, match="c.c_ndim=3"):
        amd.biem(c, multipole_source_position=np.ones(2), multipole_source_index=1, **kw)
    with pytest.raises(ValueError, match="is not k.ndim \\+ 1"):
        amd.biem(c, multipole_source_position=np.full((3, 2), 5.0), multipole_source_index=1, **kw)
    with pytest.raises(ValueError, match="not broadcastable"):
        amd.biem(c, multipole_source_position=far, multipole_source_index=np.array([1, 2]), **kw)
    with pytest.raises(ValueError, match="real array"):
        amd.biem(c, multipole_source_position=far + 0j, multipole_source_index=1, **kw)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            amd.biem(c, multipole_source_position=np.array([5.0, bad, 0.0]), multipole_source_index=1, **kw)
    for name in ("multipole_source_position", "multipole_source_index"):
        assert name in amd.biem.__doc__ and name in amd.BIEMFactorization.solve.__doc__
    assert "harmonic_labels" in amd.__all__ and "multipole_source" in amd.__all__
    assert "orthonormal" in amd.multipole_source.__doc__ and "Y_0" in amd.multipole_source.__doc__


# ---------------------------------------------------------------------------- d. the C ABI
def _params(text, ret, name):
    m = re.search(r"\b%s %s\(([^;]*?)\);" % (ret, name), text, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split() for p in m.group(1).split(",")]


ENTRIES = {"biem_rhs_multipole": "biem_rhs_point_source", "biem_solve_ms": "biem_solve_ps", "biem_solve_ldlt_ms": "biem_solve_ldlt_ps",
           "biem_solve_factored_ms": "biem_solve_factored_ps"}


def test_header_declares_the_entries_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    names = lambda ps: [p[-1].lstrip("*") for p in ps]
    kind_of = lambda p: _lib._i if p[:-1] == ["int"] else _lib._ll if p[:-1] == ["long", "long"] else _lib._sz if p[:-1] == ["size_t"] else _lib._vp
    for name, twin in ENTRIES.items():
        ps, tw = _params(hdr, "int", name), _params(hdr, "int", twin)
        at = names(tw).index("src_batched") + 1
        assert names(ps) == names(tw)[:at] + ["d_idx"] + names(tw)[at:], name      # the _ps twin argument for argument, d_idx after src_batched
        assert ps[at][:-1] == ["const", "int*"], ps[at]
        ctypes_ = _lib.SIGNATURES[name][1]
        assert len(ctypes_) == len(ps)
        for p, ct in zip(ps, ctypes_):
            assert ct is kind_of(p), (name, p)
        t_ret, t_args = _lib.SIGNATURES[twin]
        assert _lib.SIGNATURES[name] == (t_ret, t_args[:at] + [_lib._ip] + t_args[at:])
    assert names(_params(hdr, "size_t", "biem_rhs_multipole_workspace_bytes")) == ["plan", "nb", "B", "nrhs", "src_batched", "geom_batched"]
    assert _lib.SIGNATURES["biem_rhs_multipole_workspace_bytes"] == (_lib._sz, [_lib._vp] + [_lib._i] * 5)
    ps = _params(hdr, "int", "biem_multipole_field")
    assert names(ps) == ["plan", "nb", "P", "d_k", "d_src", "d_idx", "d_points", "flags", "grad", "d_out", "d_work", "work_bytes", "stream"]
    assert [ct is kind_of(p) for p, ct in zip(ps, _lib.SIGNATURES["biem_multipole_field"][1])] == [True] * len(ps)
    assert names(_params(hdr, "size_t", "biem_multipole_field_workspace_bytes")) == ["plan", "nb"]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in list(ENTRIES) + ["biem_rhs_multipole_workspace_bytes", "biem_multipole_field", "biem_multipole_field_workspace_bytes"]:
        assert name in text, name


def test_library_cross_compiles_and_exports_the_entries():
    _build.build(force=False)
    assert not _build.is_stale()
    assert "kernels_rhs_ms.hip" in _build.SOURCES
    lib = _lib.load()
    assert lib.biem_rhs_multipole_workspace_bytes(None, 4, 3, 5, 0, 0) == 0
    assert lib.biem_multipole_field_workspace_bytes(None, 4) == 0
    for name in list(ENTRIES) + ["biem_multipole_field"]:
        args = [0 if t is _lib._i or t is _lib._ll or t is _lib._sz else None for t in _lib.SIGNATURES[name][1]]
        rc = getattr(lib, name)(*args)                                   # no plan, no sources: an argument error, no device touched
        assert rc == 1 and name.encode() in lib.biem_last_error(), (name, lib.biem_last_error())
        dummy = np.zeros(8)
        args = [None] + [0 if t is _lib._i or t is _lib._ll or t is _lib._sz else dummy.ctypes.data for t in _lib.SIGNATURES[name][1][1:]]
        rc = getattr(lib, name)(*args)                                   # every operand but the plan: the plan is what is missing
        assert rc == 1 and b"null plan" in lib.biem_last_error(), (name, lib.biem_last_error())
