"""CPU tests of the yardsticks behind tests/test_gpu_full_order_hess_force.py: ``MPField.hessian`` and ``oracle/mp_force.py`` (40 digits)
and the fixture ``tests/golden/full_order_hess_force.npz`` that ``tools/make_full_order_hess_force_fixtures.py`` writes with them.

1. ``MPField.hessian`` reproduces ``tests/golden/hess_fields.npz`` at low order bit for bit (the same rule, which moved into the
   evaluator), and that file is tied to the golden-pinned oracle and to the ladder twin by tests/test_field_hessian_host.py.
2. ``mp_force`` equals the fp64 yardstick tests/force_yardstick.py on the oracle's SOLVED problems at low order, with the yardstick's
   own dense table, on all three boundary cases: that pins its factors, signs and normalisation before it judges a kernel.
3. The fixture holds the cases, the caps (condition <= 100, fp64 twin / yardstick <= 1e-11, at least 16 valid points, no multiple
   of 64), every degree at modulus [0.5, 1.5], and is what the generator makes (one entry per case recomputed: mpmath on Python
   integers is deterministic).
"""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from oracle import biem_oracle as O  # noqa: E402
from oracle import full_order_fixture as FX  # noqa: E402
from oracle import mp_field as M  # noqa: E402
from oracle import mp_force as MF  # noqa: E402

import force_yardstick as FY  # noqa: E402
import power_yardstick as PY  # noqa: E402
from test_field_hessian_host import CASES as LOW  # noqa: E402
from test_force_host import coupling, solved  # noqa: E402
from test_power_host import COEFFICIENTS  # noqa: E402

CASES = FX.load_hess_force()
HESS = [c for c, r in CASES.items() if r.family == "hess"]
FORCE = [c for c, r in CASES.items() if r.family == "force"]
FAMILY = {"bpa": "ba", "bpbpa": "bba"}


# ---------------------------------------------------------------------------- 1. MPField.hessian at low order
@pytest.mark.parametrize("cid", sorted(LOW))
def test_mp_hessian_reproduces_the_low_order_fixture(cid):
    rec = LOW[cid]
    F = M.MPField(rec.tree, rec.n_end, rec.k, rec.eta, rec.centers, rec.radii, rec.density, rec.kind)
    for p in np.flatnonzero(rec.valid)[[0, 1, -1]]:
        got = np.array([[complex(v) for v in row] for row in F.hessian("near", rec.x[p])])
        assert np.array_equal(got, rec.hess[:, :, p]), (cid, p)


# ---------------------------------------------------------------------------- 2. mp_force at low order
@pytest.mark.parametrize("case", sorted(COEFFICIENTS))
@pytest.mark.parametrize("tree", ["a", "ba", "bba"])
def test_mp_force_equals_the_fp64_yardstick_on_solved_problems(tree, case):
    n_end = 8
    res = solved(tree, case, n_end)[0]
    a, b = COEFFICIENTS[case]
    an, bn = PY.degree_pair(a, b, len(res.radii), n_end)
    want = FY.force(res, a, b, coupling(tree, n_end))
    table = FY.independent_table(tree, n_end)
    fac = MF.factors(tree, n_end, float(res.k), res.eta, res.radii, an, bn)
    got, cond = MF.force(tree, n_end, float(res.k), res.radii, fac, res.density, table)
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"{tree} {case}: |mp - fp64 yardstick| / |Phi| per ball {err}, condition {cond}")
    assert (err <= 1e-12 * np.maximum(cond, 1.0)).all()


# ---------------------------------------------------------------------------- 3. the fixture
def test_fixture_cases_and_caps():
    hess = {(r.kind, r.tree, r.n_end) for r in CASES.values() if r.family == "hess"}
    below = [("a", 318), ("ba", 46), ("bpa", 46), ("bba", 12), ("bpbpa", 12), ("caa", 10)]
    at = [("a", 320), ("bba", 14), ("caa", 12)]
    want = {("outer", t, n) for t, n in below + at} | {("inner", t, n) for t, n in below + at if t in ("a", "ba", "bba", "caa")}
    assert hess == want
    for key in want:
        regimes = {r.regime for r in CASES.values() if r.family == "hess" and (r.kind, r.tree, r.n_end) == key}
        assert regimes == ({"osc", "evan", "cplx"} if key[1] in ("ba", "bpa") else {"osc", "evan"}), key
    for cid in HESS:
        r = CASES[cid]
        v = r.valid
        d = r.x.shape[1]
        assert len(r.x) % 64 != 0 and (~v).sum() == 1 and v.sum() >= 16 and len(r.radii) == (1 if r.kind == "inner" else 2), cid
        assert r.hess.shape == (d, d, len(v)) and np.isnan(r.hess[:, :, ~v]).all() and np.isfinite(r.hess[:, :, v]).all()
        assert np.array_equal(r.hess[:, :, v], r.hess.transpose(1, 0, 2)[:, :, v])
        assert (r.cond[v] <= 100.0).all() and (r.oracle_err[v] <= 1e-11).all(), cid
        assert (np.imag(r.k) != 0) == (r.regime == "cplx") and np.isfinite(r.density).all() and (np.abs(r.density) > 0).all()
        fr = np.min(np.linalg.norm(r.x[v][:, None, :] - r.centers[None], axis=2) / r.radii[None], axis=1)
        assert ((fr == 0).any() == (r.kind == "inner")), cid                       # the centre is among the points of kind inner
    force = {(r.tree, r.n_end, r.regime, r.bc) for r in CASES.values() if r.family == "force"}
    want = {(t, n, rg, bc) for t, n in (("a", 320), ("ba", 48), ("bpa", 48), ("bba", 14), ("bpbpa", 14), ("caa", 12)) for rg in ("osc", "evan")
            for bc in ("robin", "fluid")} | {("ba", 48, "osc", "transparent-top"), ("ba", 48, "batch", "robin")}
    assert force == want
    for cid in FORCE:
        r = CASES[cid]
        assert np.imag(r.k).max() == 0 if np.ndim(r.k) else np.imag(r.k) == 0
        computed = ~np.isnan(r.phi).any(-1)
        assert (r.cond[computed] <= 100.0).all() and (r.oracle_err[computed] <= 1e-11).all(), cid
        assert computed.all() == (r.bc != "transparent-top") and np.isfinite(r.density).all() and (np.abs(r.density) > 0).all()
        assert r.radii[..., 0].min() != r.radii[..., 1].min()                      # two balls of different radii
        if r.bc == "fluid":
            assert r.k_interior[1].imag != 0 and r.alpha_n.shape == r.beta_n.shape == (2, r.n_end)
    r = CASES["force-ba-48-osc-transparent-top"]
    assert np.isnan(r.phi[0]).all() and np.isfinite(r.phi[1]).all()
    assert (r.alpha_n[:, :-1] == r.alpha).all() and r.alpha_n[1, -1] == r.alpha and r.alpha_n[0, -1] != r.alpha      # the top degree of ball 0 alone
    r = CASES["force-ba-48-batch-robin"]
    assert r.phi.shape == (3, 2, 2, 3) and r.density.shape == (3, 2, 2, 2304) and r.radii.shape == (3, 2) and len(set(r.k.tolist())) == 3


@pytest.mark.parametrize("cid", HESS)
def test_hessian_densities_show_every_degree(cid):
    """|density blc_n z_n| of every harmonic at the reference radius (1.2 rho outside, 0.8 rho inside), with the oracle's fp64 radial
    functions: the modulus of w, in [0.5, 1.5] (to 1e-6: w is stored in single precision, the scale is rounded once)."""
    r = CASES[cid]
    tr = O.tree(r.tree)
    deg = tr.degrees(r.n_end)
    np.seterr(invalid="ignore", over="ignore")
    for b, rho in enumerate(r.radii):
        j, h, jp, hp = O.radial_h(r.n_end - 1, tr.d, r.k * rho)
        if r.kind == "inner":
            j, jp = h, hp
        blc = 1j * r.k ** (tr.d - 1) * rho ** (tr.d - 1) * jp - 1j * r.eta * (1j * r.k ** (tr.d - 2) * rho ** (tr.d - 1) * j)
        z = O.radial_h(r.n_end - 1, tr.d, r.k * rho * (0.8 if r.kind == "inner" else 1.2))[0 if r.kind == "inner" else 1]
        mod = np.abs(r.density[b] * blc[deg] * z[deg])
        assert mod.min() >= 0.5 * (1 - 1e-6) and mod.max() <= 1.5 * (1 + 1e-6), (cid, b, mod.min(), mod.max())


@pytest.mark.parametrize("cid", HESS)
def test_hessian_fixture_is_what_the_generator_makes(cid):
    """One diagonal component at one point per case (three evaluations of the series per ball), recomputed from the stored inputs with
    the generator's rule: bit-equal fp64.  Point and component rotate over the cases."""
    r = CASES[cid]
    i = HESS.index(cid)
    p = int(np.flatnonzero(r.valid)[i % int(r.valid.sum())])
    c = i % r.x.shape[1]
    F = M.MPField(r.tree, r.n_end, r.k, r.eta, r.centers, r.radii, r.density, r.kind)
    with mp.workdps(M.DPS):
        x = F._x(r.x[p])
        h = mp.mpf(M.HESS_STEPS[0])
        f = lambda s: mp.fsum(F.ball_sum("near", b, [x[q] + (s * h if q == c else 0) for q in range(F.d)]) for b in range(F.B))
        assert complex((f(1) - 2 * f(0) + f(-1)) / (h * h)) == r.hess[c, c, p]


@pytest.mark.parametrize("cid", FORCE)
def test_force_fixture_is_what_the_generator_makes(cid):
    """One component of one ball per case (of the first system and right-hand side of the launch-shape case), recomputed with
    mp_force and the independent table from the stored inputs: bit-equal fp64.  And the traces of every degree have the modulus of w."""
    r = CASES[cid]
    i = FORCE.index(cid)
    batch = r.regime == "batch"
    k, radii, dens, phi = (r.k[0], r.radii[0], r.density[0, 0], r.phi[0, 0]) if batch else (r.k, r.radii, r.density, r.phi)
    an, bn = (r.alpha_n, r.beta_n) if r.bc != "robin" else PY.degree_pair(r.alpha, r.beta, 2, r.n_end)
    b = 1 if r.bc == "transparent-top" else i % 2
    c = i % phi.shape[-1]
    fac = MF.factors(r.tree, r.n_end, float(k), r.eta, radii, an, bn)
    got, _ = MF.force(r.tree, r.n_end, float(k), radii, fac, dens, FY.independent_table(r.tree, r.n_end), skip=(1 - b,), components=[c])
    assert got[b, c] == phi[b, c], (cid, b, c)
    deg = O.tree(r.tree).degrees(r.n_end)
    with mp.workdps(M.DPS):
        mod = np.array([float(max(abs(fac[b][0][n]), abs(fac[b][1][n]))) for n in deg]) * np.abs(dens[b])
    assert mod.min() >= 0.5 * (1 - 1e-6) and mod.max() <= 1.5 * (1 + 1e-6), (cid, mod.min(), mod.max())
