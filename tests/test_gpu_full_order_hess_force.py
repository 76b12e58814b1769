"""biem_force() and uscat_hess() AT the order ceilings (a 320, ba 48, bba 14, caa 12) and two orders above them, against 40-digit values.

Both features read the plan's coupling table (tests/test_force_table_full_order_host.py pins it at these orders); the suite otherwise
runs ``k_force`` at n_end <= 10 (tree a: 40) and ``k_coef_ladder`` at n_end <= 8 on solved densities, which decay with the degree and
hide the top rows of the table, the ladder's degree cut, the embedding into the order-(n_end + 2) layout and the launch-sized LDS of
``k_force`` below any tolerance.  Every case here comes from ``tests/golden/full_order_hess_force.npz``
(``tools/make_full_order_hess_force_fixtures.py``): synthetic densities in which EVERY degree carries a term of modulus in [0.5, 1.5],
and expected values computed at 40 digits from exactly the stored fp64 inputs.  Nothing high-precision runs here.

Assertions (1e-10 is the parity contract of BASELINE.md):
* Hessian, per point: the NaN mask is the stored one, H[i, j] == H[j, i] bit for bit, |got - want|_F <= 1e-10 |want|_F, and
  |sum_i H_ii + k^2 uscat| <= 1e-10 |H|_F against the library's own uscat - through the per-lane value kernel and the generic one;
* force, per ball: |got - want|_2 <= 1e-10 |want|_2, two calls bit identical, NaN for exactly the ball whose top degree is transparent.
The generator admits a point (a ball) only if its condition number is at most 100 and the fp64 twin (yardstick) meets 1e-11 there;
both are stored and tests/test_full_order_hess_force_host.py checks them.  Every test prints the largest error it measured.

The chain trees have no 40-digit evaluator: bbba (density order 6, plan 8) and bbbba (3, plan 5) are compared with the NumPy ladder
twin (tests/hess_yardstick.py: the plan's table, the oracle's radial functions and the test-local chain harmonics) on a synthetic
every-degree density, and held to the Helmholtz trace.
"""
import time

import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd
from oracle import biem_oracle as O
from oracle import full_order_fixture as FX

import hess_yardstick as HY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY_TOL = 1e-10
SUM_TOL = 1e-12          # per-ball parts against the plain call (tests/test_gpu_field_hessian.py)
CASES = FX.load_hess_force()
HESS = [c for c, r in CASES.items() if r.family == "hess"]
FORCE = [c for c, r in CASES.items() if r.family == "force" and r.regime != "batch" and r.bc != "transparent-top"]
KERNELS = ["per_lane", "generic"]
DIM = {"a": 2, "ba": 3, "bpa": 3, "bba": 4, "bpbpa": 4, "caa": 4}


def t(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device=DEV, dtype=dtype)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _select(monkeypatch, kernel):
    if kernel == "generic":
        monkeypatch.setenv("BIEM_USCAT_GENERIC", "1")
    else:
        monkeypatch.delenv("BIEM_USCAT_GENERIC", raising=False)


def _frob(a):
    """|a|_F over the two component axes of a [d, d, ...] array."""
    return np.sqrt((np.abs(a) ** 2).sum(axis=(0, 1)))


def test_the_fixture_holds_the_orders_of_this_build():
    """Densities two orders below the ceilings (the value kernel runs at the ceiling) and at them (two above), forces at them."""
    top = amd._biem.USCAT_GRAD_N_END_MAX
    assert top == {"a": 320, "ba": 48, "bba": 14, "caa": 12}
    fam = lambda r: {"bpa": "ba", "bpbpa": "bba"}.get(r.tree, r.tree)
    for tree, n in top.items():
        assert any(r.family == "hess" and fam(r) == tree and r.n_end == n - 2 for r in CASES.values())
        assert any(r.family == "force" and fam(r) == tree and r.n_end == n for r in CASES.values())
    for tree in ("a", "bba", "caa"):
        assert any(r.family == "hess" and r.tree == tree and r.n_end == top[tree] for r in CASES.values())
    for r in CASES.values():
        if r.family == "hess":
            assert len(r.x) % 64 != 0 and r.valid.sum() >= 16


# ---------------------------------------------------------------------------- Hessian
def _hess_calc(rec, density=None, centers=None, radii=None):
    return amd.BIEMResultCalculator(c=amd.create_from_branching_types(rec.tree), centers=t((rec.centers if centers is None else centers).T),
                                    radii=t(rec.radii if radii is None else radii), k=t(rec.k), n_end=rec.n_end, eta=t(float(rec.eta)),
                                    kind=rec.kind, density=t(rec.density if density is None else density, torch.complex128))


def _check_hessian(what, rec, got):
    d, P = rec.x.shape[1], len(rec.x)
    v = rec.valid
    assert got.shape == (d, d, P) and got.dtype == np.complex128
    bad = np.isnan(got.real) | np.isnan(got.imag)
    assert np.array_equal(bad, np.broadcast_to(~v, got.shape)), f"{what}: NaN mask {bad}"
    assert _same_bits(got, got.transpose(1, 0, 2))                                       # H[i, j] == H[j, i]
    err = _frob(got[:, :, v] - rec.hess[:, :, v]) / _frob(rec.hess[:, :, v])
    print(f"  {what}: max |got - want|_F / |want|_F = {err.max():.2e} over {int(v.sum())} points "
          f"(|want|_F {_frob(rec.hess[:, :, v]).min():.1e} .. {_frob(rec.hess[:, :, v]).max():.1e})")
    assert (err <= PARITY_TOL).all(), f"{what}: {err}"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cid", HESS)
def test_hessian_and_its_trace(cid, kernel, monkeypatch):
    """uscat_hess against the 40-digit second differences, and sum_i H_ii + k^2 uscat against the same library's uscat at the same
    points, through the per-lane value kernel and (BIEM_USCAT_GENERIC=1) the harmonic-by-harmonic one."""
    rec = CASES[cid]
    _select(monkeypatch, kernel)
    x = t(rec.x.T)
    t0 = time.perf_counter()
    calc = _hess_calc(rec)
    if rec.tree == "a" and rec.kind == "inner" and rec.n_end + 2 > 320:
        # 2-D above the radial tables (order 320) is the per-lane exterior kernel's alone: uscat refuses kind inner at order 322, and
        # so does the Hessian of a density of order 320 - by name, before any launch
        with pytest.raises(NotImplementedError, match=f"n_end={rec.n_end + 2} too large"):
            calc.uscat_hess(x)
        print(f"{cid} [{kernel}]: refused, as uscat at order {rec.n_end + 2}")
        return
    got = calc.uscat_hess(x).cpu().numpy()
    u = calc.uscat(x).cpu().numpy()
    print(f"{cid} [{kernel}]: condition <= {np.nanmax(rec.cond):.0f}, fp64 twin {np.nanmax(rec.oracle_err):.1e}, "
          f"{time.perf_counter() - t0:.1f} s with the plans of a first call")
    _check_hessian("Hessian", rec, got)
    v = rec.valid
    assert np.array_equal(np.isnan(u), ~v)
    d = got.shape[0]
    res = np.abs(sum(got[i, i] for i in range(d)) + complex(rec.k) ** 2 * u)[v] / _frob(got[:, :, v])
    print(f"  trace: max |tr H + k^2 uscat| / |H|_F = {res.max():.2e}")
    assert (res <= PARITY_TOL).all(), res


@pytest.mark.parametrize("cid", [c for c in HESS if CASES[c].tree in ("bpa", "bpbpa")])
def test_components_are_in_the_callers_axes(cid):
    """The fixture itself tells the canonical axis order from the caller's: permuted the way the canonical tree sees the axes, on either
    component axis, it is far from itself - and so is the result."""
    from biem_helmholtz_sphere_amd._coords import CANONICAL

    rec = CASES[cid]
    perm = list(CANONICAL[rec.tree][1])
    v = rec.valid
    want = rec.hess[:, :, v]
    got = _hess_calc(rec).uscat_hess(t(rec.x.T)).cpu().numpy()[:, :, v]
    scale = _frob(want)
    assert (_frob(want[perm] - want) > 1e-2 * scale).any() and (_frob(want[:, perm] - want) > 1e-2 * scale).any()
    assert (_frob(got[perm][:, perm] - want) > 1e-2 * scale).any()
    assert (_frob(got - want) <= PARITY_TOL * scale).all()


@pytest.mark.parametrize("cid", ["hess-ext-a-318-osc", "hess-ext-ba-46-evan", "hess-ext-bpa-46-osc", "hess-ext-bba-12-osc", "hess-ext-bpbpa-12-evan",
                                 "hess-ext-caa-10-osc"])
def test_per_ball_parts(cid):
    """per_ball=True: every part has the mask and the symmetry, the parts sum to the plain call, and each equals its one-ball record."""
    rec = CASES[cid]
    calc, x, v = _hess_calc(rec), t(rec.x.T), rec.valid
    plain = calc.uscat_hess(x).cpu().numpy()
    pb = calc.uscat_hess(x, per_ball=True).cpu().numpy()
    B = len(rec.radii)
    assert pb.shape == plain.shape + (B,)
    assert np.isnan(pb[:, :, ~v]).all() and np.isfinite(pb[:, :, v]).all()
    assert _same_bits(pb, pb.transpose(1, 0, 2, 3))
    scale = sum(_frob(pb[:, :, v, b]) for b in range(B))
    dev = (_frob(pb[:, :, v].sum(-1) - plain[:, :, v]) / scale).max()
    print(f"{cid}: sum over balls against the plain call: {dev:.2e} of the parts' |H|_F")
    assert dev <= SUM_TOL, dev
    for b in range(B):
        # (a one-ball record does not mask the other ball's interior: compare where both are valid)
        one = _hess_calc(rec, density=rec.density[b:b + 1], centers=rec.centers[b:b + 1], radii=rec.radii[b:b + 1]).uscat_hess(x).cpu().numpy()
        dev = (_frob(one[:, :, v] - pb[:, :, v, b]) / _frob(pb[:, :, v, b])).max()
        print(f"  ball {b} against its one-ball record: {dev:.2e}")
        assert dev <= SUM_TOL, dev


# ---------------------------------------------------------------------------- Hessian on the chain trees: the NumPy ladder twin
CHAIN_CENTERS = np.array([[1.7, 0.9, -0.6, 0.5, 0.3, -0.4], [-1.4, -1.1, 0.8, -0.7, -0.4, 0.6]])
CHAIN_RADII = np.array([1.0, 0.7])
CHAIN_GEN = np.array([[0.3, -0.8, 0.45, 0.6, -0.2, 0.35], [-0.5, 0.4, 0.6, -0.3, 0.2, -0.45], [0.7, 0.2, -0.4, 0.5, 0.3, 0.25]])


def _chain_case(tree, n_end, k):
    """Two balls off every axis, a density with a term of modulus in [0.5, 1.5] in every degree at r = 1.2 rho (the construction of the
    fixture, in fp64 from the oracle's radial functions), points at 1.05 .. 1.5 rho in generic directions, on the root axis and in a
    coordinate plane, the origin, and one point inside ball 1 for the mask."""
    tr = HY.oracle_tree(tree)
    d, deg = tr.d, tr.degrees(n_end)
    cen, rad = CHAIN_CENTERS[:, :d].copy(), CHAIN_RADII
    rng = np.random.default_rng([d, n_end, 20261020])
    w = rng.uniform(0.5, 1.5, (2, len(deg))) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (2, len(deg))))
    unit = HY.near_coefs(tree, n_end, k, 1.0, rad, np.ones((2, len(deg))), "outer")                  # blc_n per harmonic
    scale = np.stack([np.abs(unit[b]) * np.abs(O.radial_h(n_end - 1, d, k * 1.2 * rho)[1][deg]) for b, rho in enumerate(rad)])
    dens = w / scale
    e = np.eye(d)
    g = [v[:d] / np.linalg.norm(v[:d]) for v in CHAIN_GEN]
    plane = np.zeros(d)
    plane[[1, d - 1]] = (0.6, -0.8)
    x = [cen[0] + 1.05 * rad[0] * g[0], cen[0] + 1.5 * rad[0] * g[1], cen[0] + 1.2 * rad[0] * e[0], cen[0] - 1.3 * rad[0] * e[0],
         cen[0] + 1.25 * rad[0] * plane, cen[1] + 1.1 * rad[1] * g[2], cen[1] + 1.4 * rad[1] * g[0], cen[1] + 1.2 * rad[1] * e[d - 1],
         cen[1] - 1.25 * rad[1] * plane, np.zeros(d), 3.5 * g[1], cen[1] + 0.5 * rad[1] * g[0]]
    return cen, rad, dens, np.array(x)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("tree,n_end", [("bbba", 6), ("bbbba", 3)])
def test_chain_hessian_against_the_ladder_twin(tree, n_end, kernel, monkeypatch):
    """bbba at the largest chain order the GPU tests run (plan 8) and bbbba (plan 5).  The twin shares the plan's table, which the
    host test pins, and none of the kernels.  |GPU - twin| <= 1e-10 max |H| over the case, the bound of the fixture comparisons of
    tests/test_gpu_field_hessian.py, and the Helmholtz trace of its chain test."""
    _select(monkeypatch, kernel)
    k = 0.8 * (n_end + 2)                                                                          # k rho_0 = 0.8 of the plan's order
    cen, rad, dens, x = _chain_case(tree, n_end, k)
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types(tree), centers=t(cen.T), radii=t(rad), k=t(k), n_end=n_end, eta=t(1.0),
                                    kind="outer", density=t(dens, torch.complex128))
    got = calc.uscat_hess(t(x.T)).cpu().numpy()
    u = calc.uscat(t(x.T)).cpu().numpy()
    d = len(tree) + 1
    assert got.shape == (d, d, len(x)) and np.isnan(got[:, :, -1]).all() and np.isfinite(got[:, :, :-1]).all() and np.isnan(u[-1])
    assert _same_bits(got, got.transpose(1, 0, 2))
    want = HY.hessian(tree, n_end, k, 1.0, "outer", cen, rad, dens, x[:-1])
    scale = np.abs(want).max()
    err = np.abs(got[:, :, :-1] - want).max() / scale
    res = (np.abs(sum(got[i, i] for i in range(d)) + k * k * u)[:-1] / _frob(got[:, :, :-1])).max()
    print(f"{tree} density order {n_end} [{kernel}]: |GPU - twin| = {err:.2e} of max |H| = {scale:.3e}; per point "
          f"{np.abs(got[:, :, :-1] - want).max(axis=(0, 1)) / scale}; |tr H + k^2 uscat| / |H|_F = {res:.2e}")
    assert err <= PARITY_TOL and res <= PARITY_TOL


# ---------------------------------------------------------------------------- force
def _force_calc(rec, k, radii, density):
    """A record around a stored density: the force reads neither centres nor points (the balls are put far apart)."""
    d, B = DIM[rec.tree], np.shape(radii)[-1]
    cen = np.zeros((d,) + (1,) * (np.ndim(radii) - 1) + (B,))
    cen[0, ..., :] = 5.0 * np.arange(B)
    return amd.BIEMResultCalculator(c=amd.create_from_branching_types(rec.tree), centers=t(cen), radii=t(radii), k=t(k), n_end=rec.n_end,
                                    eta=t(np.ones(np.shape(k))), kind="outer", density=t(density, torch.complex128))


def _pair(rec):
    if rec.bc == "robin":
        return dict(alpha=rec.alpha, beta=rec.beta)
    return dict(alpha_n=t(rec.alpha_n, torch.complex128), beta_n=t(rec.beta_n, torch.complex128))


def _check_force(what, got, want, cond, oracle_err):
    """got, want [..., B, d]: the Euclidean norm over the components, per ball."""
    err = np.linalg.norm(got - want, axis=-1) / np.linalg.norm(want, axis=-1)
    print(f"  {what}: max |got - want| / |want| per ball = {np.nanmax(err):.2e} (condition <= {np.nanmax(cond):.0f}, fp64 yardstick {np.nanmax(oracle_err):.1e}; "
          f"|want| {np.nanmin(np.linalg.norm(want, axis=-1)):.2e} .. {np.nanmax(np.linalg.norm(want, axis=-1)):.2e})")
    assert (err[~np.isnan(want).any(-1)] <= PARITY_TOL).all(), err


@pytest.mark.parametrize("cid", FORCE)
def test_force(cid):
    rec = CASES[cid]
    calc, kw = _force_calc(rec, rec.k, rec.radii, rec.density), _pair(rec)
    t0 = time.perf_counter()
    first = calc.force(**kw).cpu().numpy()
    took = time.perf_counter() - t0
    again = calc.force(**kw).cpu().numpy()
    print(f"{cid}: {took:.1f} s with the plan and table of a first call")
    assert first.shape == (DIM[rec.tree], len(rec.radii)) and np.isfinite(first).all()
    assert _same_bits(first, again)
    _check_force("Phi", first.T, rec.phi, rec.cond, rec.oracle_err)


def test_transparent_top_degree_is_nan_for_that_ball_only():
    """ba 48, the pair of the transparent sphere (k_b = k, delta = 1) in degree 47 of ball 0 alone: gj_47 vanishes to the rounding of its
    two terms, the density does not determine that ball's traces, and the ball is NaN - the other keeps its 40-digit value."""
    rec = CASES["force-ba-48-osc-transparent-top"]
    assert np.isnan(rec.phi[0]).all() and np.isfinite(rec.phi[1]).all()
    got = _force_calc(rec, rec.k, rec.radii, rec.density).force(**_pair(rec)).cpu().numpy().T
    print(got)
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()
    _check_force("Phi of the other ball", got, rec.phi, rec.cond, rec.oracle_err)


def test_launch_shape_three_systems_two_right_hand_sides_at_ba_48():
    """3 systems (k and radii batched) x 2 right-hand sides x 2 balls at H = 2304: the grid's (b, r, s) indexing where every stride is
    large, each (system, right-hand side) against its own 40-digit value; every slice equals its single call bit for bit."""
    rec = CASES["force-ba-48-batch-robin"]
    S, R, B = rec.phi.shape[:3]
    calc = _force_calc(rec, rec.k[:, None], rec.radii[:, None, :], rec.density)
    got = calc.force(**_pair(rec)).cpu().numpy()
    assert got.shape == (3, S, R, B)
    got = got.transpose(1, 2, 3, 0)
    _check_force("Phi", got, rec.phi, rec.cond, rec.oracle_err)
    assert np.linalg.norm(rec.phi[0, 0] - rec.phi[0, 1]) > 1e-2 * np.linalg.norm(rec.phi[0, 0])      # the right-hand sides differ,
    assert np.linalg.norm(rec.phi[0, 0] - rec.phi[1, 0]) > 1e-2 * np.linalg.norm(rec.phi[0, 0])      # and so do the systems
    for s in range(S):
        for r in range(R):
            one = _force_calc(rec, rec.k[s], rec.radii[s], rec.density[s, r]).force(**_pair(rec)).cpu().numpy().T
            assert _same_bits(one, got[s, r]), (s, r)
