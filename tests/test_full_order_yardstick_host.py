"""CPU tests of the yardstick behind tests/test_gpu_full_order.py: the 40-digit evaluator ``oracle/mp_field.py`` and the fixture
``tests/golden/full_order_fields.npz`` that ``tools/make_full_order_fixtures.py`` writes with it.

1. At low order (the orders of tests/test_gpu_field_gradient.py, n_end <= 8) on all six trees, both kinds, real and complex k, the
   evaluator equals the golden-pinned fp64 oracle: values to 1e-12 pointwise, gradients to 1e-11 of max |grad u| against the oracle's
   8th-order stencil at h = 5e-3 (the stencil's own measured quality there).  That ties label order, normalisation, axis
   permutation and component order of the new evaluator to the oracle.
2. The interior field equals the algebraic formula of tests/test_gpu_interior_field.py (``_alg_coef`` + ``_u_from_coef``) at its SHAPES.
3. The fixture is what the generator makes (recomputed bit for bit at one point per case: mpmath on Python integers is
   deterministic), respects the generator's caps, and sits at the orders the launchers' LDS formulas give.
"""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import test_gpu_field_gradient as G  # noqa: E402  (its geometry, points and stencil; nothing in it runs at import)
import test_gpu_interior_field as IF  # noqa: E402
from oracle import biem_oracle as O  # noqa: E402
from oracle import full_order_fixture as FX  # noqa: E402
from oracle import mp_field as M  # noqa: E402

TREES = ("a", "ba", "bpa", "bba", "bpbpa", "caa")
CASES = FX.load()


# ---------------------------------------------------------------------------- 1. low order against the oracle
def _low_order(bt, kind, k):
    d, n_end = G.DIM[bt], G.N_END[bt]
    if kind == "outer":
        cen, rad = G._geometry(d)
        x = np.concatenate([G._points(bt, cen, rad), [cen[0] + 0.5 * rad[0] * G._unit(np.ones(d))]])       # the last one is masked
    else:
        cen, rad = np.array([[0.3, -0.2, 0.1, 0.2]])[:, :d], np.array([2.0])
        e = np.eye(d)
        pts = [cen[0], cen[0] + 0.9 * e[G.ROOT_AXIS[bt]], cen[0] - 1.1 * e[0], cen[0] + 1.2 * G._unit(np.array([0.3, -0.8, 0.45, 0.6])[:d]),
               cen[0] + 1.9 * G._unit(np.array([-0.5, 0.4, 0.6, -0.3])[:d])]
        if d == 4:
            pts += [cen[0] + 0.8 * G._unit(v) for v in ([0.6, -0.8, 0.0, 0.0], [0.0, 0.0, 0.7, 0.5], [0.0, 0.6, -0.8, 0.0])]
        x = np.array(pts + [cen[0] + 2.2 * e[0]])
    uo, go = O.plane_wave(k, G._direction(d))
    res = O.solve_biem(bt, centers=cen, radii=rad, k=k, n_end=n_end, eta=1.0, uin=uo, uin_grad=go, kind=kind)
    return res, M.MPField(bt, n_end, k, 1.0, cen, rad, res.density, kind), x


@pytest.mark.parametrize("k", [1.3, 1.3 + 0.2j], ids=["real_k", "complex_k"])
@pytest.mark.parametrize("kind", ["outer", "inner"])
@pytest.mark.parametrize("bt", TREES)
def test_low_order_equals_the_oracle(bt, kind, k):
    res, F, x = _low_order(bt, kind, k)
    for far, per_ball in ((False, False), (False, True), (True, True)):
        xs = x[1:] if far and kind == "inner" else x              # (the far field of the centre itself has no direction)
        want, got = O.uscat(res, xs, far_field=far, per_ball=per_ball), F.uscat(xs, far_field=far, per_ball=per_ball)
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)) and (far or np.isnan(want[-1]).all())
        ok = ~np.isnan(want)
        err = np.max(np.abs(got[ok] - want[ok]) / np.abs(got[ok]))
        print(f"  {bt} {kind} far={far} per_ball={per_ball}: {err:.2e} pointwise")
        assert err <= 1e-12
    xv = x[:-1]
    want = G._stencil(res, xv, 5e-3)
    got = F.uscat_grad(x)
    assert got.shape == (G.DIM[bt], len(x)) and np.isnan(got[:, -1]).all()
    scale = np.abs(want).max()
    err = np.abs(got[:, :-1] - want).max() / scale
    print(f"  {bt} {kind}: gradient {err:.2e} of max |grad u| = {scale:.3e}")
    assert err <= 1e-11


@pytest.mark.parametrize("bt", ["bpa", "bpbpa"])
def test_low_order_gradient_is_in_the_callers_axes(bt):
    """The comparison above tells the caller's component order from the canonical one."""
    res, F, x = _low_order(bt, "outer", 1.3)
    want = G._stencil(res, x[:-1], 5e-3)
    perm = list(O.tree(bt).perm)
    assert np.abs(want[perm] - want).max() > 1e-2 * np.abs(want).max()


# ---------------------------------------------------------------------------- 2. the interior field against the algebraic formula
@pytest.mark.parametrize("fluid", sorted(IF.FLUIDS))
@pytest.mark.parametrize("tree,B,n_end", IF.SHAPES)
def test_interior_equals_the_algebraic_formula(tree, B, n_end, fluid):
    tr, cen, rad = IF._dn_systems(tree, B, n_end)[:3]
    dens, s = IF._yardstick(tree, B, n_end, fluid)
    kb, delta = IF._fluid(fluid, B)
    x, ball = IF._interior_points(cen, rad)
    ref = IF._u_from_coef(tr, n_end, IF._alg_coef(tr, n_end, rad, s, kb, delta), kb, cen, x, ball)
    F = M.MPField(tree, n_end, IF.K, IF.ETA, cen, rad, dens, "outer", kb, delta)
    got = F.uscat(np.concatenate([x, [cen[0] + 1.5 * rad[0] * np.eye(tr.d)[0]]]), interior=True)
    assert np.isnan(got[-1]) and np.isfinite(got[:-1]).all()
    err = np.max(np.abs(got[:-1] - ref)) / np.max(np.abs(ref))
    print(f"  {tree} B={B} n_end={n_end} {fluid}: {err:.2e} of max |u| = {np.max(np.abs(ref)):.3f}")
    assert err <= 1e-12


def test_radial_functions_and_the_centre():
    """h by the upward and j by the downward recurrence against direct mpmath calls at the top order; the closed form at z = 0."""
    with mp.workdps(M.DPS):
        for d, z in ((2, mp.mpf(90)), (3, mp.mpc(38.4, 0.768)), (4, mp.mpf("3.1"))):
            nu0, nmax = mp.mpf(d) / 2 - 1, 320 if d == 2 else 48
            pref = mp.sqrt(mp.pi / 2) / z ** nu0
            h, j = M.radial_h(nmax, d, z), M.radial_j(nmax, d, z)
            assert abs(h[nmax] / (pref * mp.hankel1(nu0 + nmax, z)) - 1) < mp.mpf(10) ** -30
            assert abs(j[0] / (pref * mp.besselj(nu0, z)) - 1) < mp.mpf(10) ** -30
            j0 = M.radial_j(3, d, mp.mpf(0))
            assert j0[1:] == [0, 0, 0] and abs(j0[0] - M.radial_j(3, d, mp.mpf(10) ** -25)[0]) < mp.mpf(10) ** -38


# ---------------------------------------------------------------------------- 3. the fixture
def test_fixture_cases_caps_and_ceilings():
    v_max, g_max = FX.lds_row_ceiling(False), FX.lds_row_ceiling(True)
    assert (v_max, g_max) == (153, 152)           # the orders the documentation quotes, from the launchers' formulas
    want = {("outer", "a", 320), ("outer", "ba", 48), ("outer", "bpa", 48), ("outer", "bba", 14), ("outer", "bpbpa", 14), ("outer", "caa", 12),
            ("inner", "a", v_max), ("inner", "a", g_max), ("inner", "a", v_max + 1), ("inner", "a", 320), ("inner", "ba", 48),
            ("inner", "bba", 14), ("inner", "caa", 12),
            ("interior", "a", v_max), ("interior", "a", g_max), ("interior", "ba", 48), ("interior", "bpa", 48), ("interior", "bba", 14),
            ("interior", "bpbpa", 14), ("interior", "caa", 12)}
    assert {(r.kind, r.tree, r.n_end) for r in CASES.values()} == want
    for key in want:
        regimes = {r.regime for r in CASES.values() if (r.kind, r.tree, r.n_end) == key}
        assert regimes >= {"osc", "evan"} and (("cplx" in regimes) == (key[0] != "interior" and key[1] in ("ba", "bpa"))), key
    for r in CASES.values():
        v = r.valid
        assert len(r.x) % 64 != 0 and (~v).sum() == 1 and len(r.radii) == (1 if r.kind == "inner" else 2)
        assert np.isfinite(r.density).all() and np.isnan(r.value[~v]).all() and np.isfinite(r.value[v]).all()
        names = ["cond", "oracle_err"] + (["cond_ball", "cond_far", "oracle_err_ball", "oracle_err_far"] if r.kind == "outer" else [])
        for name in names:
            cap = 100.0 if name.startswith("cond") else 1e-11
            assert (getattr(r, name)[v] <= cap).all(), (r.id, name)
        if r.kind == "interior":
            assert np.iscomplexobj(r.k_interior) and r.k_interior[1].imag != 0 and r.k_interior[0] != r.k_interior[1]
        # r / rho of the points: the surface (1.02 / 0.98) and the far end (1.5 / 0.05) are among them, the centre for the kinds inside
        fr = np.min(np.linalg.norm(r.x[v][:, None, :] - r.centers[None], axis=2) / r.radii[None], axis=1)
        near, far = (1.02, 1.5) if r.kind == "outer" else (0.98, 0.05)
        assert np.isclose(fr, near, rtol=1e-12).any() and np.isclose(fr, far, rtol=1e-12).any() and ((fr == 0).any() == (r.kind != "outer")), r.id
        has_grad = not (r.tree == "a" and r.kind != "outer" and r.n_end > g_max)
        assert (r.grad is not None) == has_grad, r.id


@pytest.mark.parametrize("cid", list(CASES))
def test_fixture_is_what_the_generator_makes(cid):
    """One point per case, recomputed with mp_field from the stored inputs: bit-equal fp64.  The gradient costs 2 d B evaluations of
    the series, so the large two-ball cases recompute one component (which one rotates over the cases)."""
    r = CASES[cid]
    i = sorted(CASES).index(cid)
    p = int(np.flatnonzero(r.valid)[i % int(r.valid.sum())])
    mode = "interior" if r.kind == "interior" else "near"
    F = M.MPField(r.tree, r.n_end, r.k, r.eta, r.centers, r.radii, r.density, "inner" if r.kind == "inner" else "outer",
                  getattr(r, "k_interior", None), getattr(r, "density_ratio", None))
    vals = F.value(mode, r.x[p])
    with mp.workdps(M.DPS):
        assert complex(mp.fsum(vals)) == r.value[p]
    if r.kind == "outer":
        assert [complex(v) for v in vals] == list(r.per_ball[p])
    if r.grad is not None:
        d = r.x.shape[1]
        comps = list(range(d)) if len(r.radii) * r.density.shape[1] * d <= 3000 else [i % d]
        assert [complex(g) for g in F.gradient(mode, r.x[p], comps)] == [r.grad[c, p] for c in comps]
