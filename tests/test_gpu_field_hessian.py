"""uscat_hess() on the GPU: the Cartesian Hessian of the scattered field by the coefficient ladder.

The yardstick is ``tests/golden/hess_fields.npz`` (``tools/make_hess_fixtures.py``): second differences of the 40-digit field series of
small solved problems, which ``tests/test_field_hessian_host.py`` ties to the golden-pinned fp64 oracle and to the NumPy twin of the
ladder.  Every record is built directly around a stored density (no solve) unless a test says otherwise.  The contract is
|GPU - fixture| <= 1e-10 max |H| over the case, an exact NaN mask and a bitwise symmetric result.
"""
import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd

from test_field_hessian_host import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY_TOL = 1e-10
SUM_TOL = 1e-12          # per-ball parts against the plain call: the bound of the like test of uscat (tests/test_gpu_parity.py)


def t(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device=DEV, dtype=dtype)


def _same_bits(a, b):
    """a == b bit for bit (NaNs by their payload too)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _calculator(rec, density=None, centers=None, radii=None, k=None):
    """A result record built directly around a stored density (no solve)."""
    return amd.BIEMResultCalculator(c=amd.create_from_branching_types(rec.tree), centers=t((rec.centers if centers is None else centers).T),
                                    radii=t(rec.radii if radii is None else radii), k=t(rec.k if k is None else k), n_end=rec.n_end,
                                    eta=t(float(rec.eta)), kind=rec.kind, density=t(rec.density if density is None else density, torch.complex128))


def _check_case(rec, got, what):
    d, P = rec.x.shape[1], len(rec.x)
    assert got.shape == (d, d, P) and got.dtype == np.complex128
    bad = np.isnan(got.real) | np.isnan(got.imag)
    assert np.array_equal(bad, np.broadcast_to(~rec.valid, got.shape)), f"{what}: NaN mask {bad}"
    assert _same_bits(got, got.transpose(1, 0, 2))                                       # H[i, j] == H[j, i]
    want = rec.hess[:, :, rec.valid]
    scale = np.abs(want).max()
    err = np.abs(got[:, :, rec.valid] - want).max() / scale
    print(f"  {what}: |GPU - fixture| = {err:.2e} of max|H| = {scale:.3e}; per point {np.abs(got[:, :, rec.valid] - want).max(axis=(0, 1)) / scale}")
    assert err <= PARITY_TOL, err
    return err


@pytest.mark.parametrize("cid", sorted(CASES))
def test_hessian_against_the_fixture(cid):
    rec = CASES[cid]
    _check_case(rec, _calculator(rec).uscat_hess(t(rec.x.T)).cpu().numpy(), cid)


@pytest.mark.parametrize("cid", ["outer-ba-k1.3", "outer-caa-k1.3", "inner-ba-k1.3"])
def test_hessian_through_the_generic_field_kernel(cid, monkeypatch):
    """BIEM_USCAT_GENERIC=1: the ladder's coefficient sets go through the harmonic-by-harmonic kernel, the one that serves the orders
    above the per-lane ceilings."""
    monkeypatch.setenv("BIEM_USCAT_GENERIC", "1")
    rec = CASES[cid]
    _check_case(rec, _calculator(rec).uscat_hess(t(rec.x.T)).cpu().numpy(), cid + " (generic)")


@pytest.mark.parametrize("cid", ["outer-bpa-k1.3", "outer-bpbpa-k1.3"])
def test_components_are_in_the_callers_axes(cid):
    """The fixture itself tells the canonical axis order from the caller's: permuted the way the canonical tree sees the axes, on either
    component axis, it is far from itself."""
    from biem_helmholtz_sphere_amd._coords import CANONICAL

    rec = CASES[cid]
    perm = list(CANONICAL[rec.tree][1])
    want = rec.hess[:, :, rec.valid]
    got = _calculator(rec).uscat_hess(t(rec.x.T)).cpu().numpy()[:, :, rec.valid]
    scale = np.abs(want).max()
    assert np.abs(want[perm] - want).max() > 1e-2 * scale and np.abs(want[:, perm] - want).max() > 1e-2 * scale
    assert np.abs(got[perm][:, perm] - want).max() > 1e-2 * scale
    assert np.abs(got - want).max() <= PARITY_TOL * scale


def test_per_ball_parts_sum_to_the_plain_call_and_match_one_ball_records():
    rec = CASES["outer-ba-k1.3"]
    calc, x = _calculator(rec), t(rec.x.T)
    plain = calc.uscat_hess(x).cpu().numpy()
    pb = calc.uscat_hess(x, per_ball=True).cpu().numpy()
    B, v = len(rec.radii), rec.valid
    assert pb.shape == plain.shape + (B,)
    assert np.isnan(pb[:, :, ~v]).all() and np.isfinite(pb[:, :, v]).all()               # every ball, every component
    assert _same_bits(pb, pb.transpose(1, 0, 2, 3))
    scale = np.abs(plain[:, :, v]).max()
    dev = np.abs(pb[:, :, v].sum(-1) - plain[:, :, v]).max() / scale
    print(f"  sum over balls against the plain call: {dev:.2e} of max|H|")
    assert dev <= SUM_TOL, dev
    for b in range(B):
        one = _calculator(rec, density=rec.density[b:b + 1], centers=rec.centers[b:b + 1], radii=rec.radii[b:b + 1]).uscat_hess(x).cpu().numpy()
        dev = np.abs(one[:, :, v] - pb[:, :, v, b]).max() / scale
        print(f"  ball {b} against its one-ball record: {dev:.2e} of max|H|")
        assert dev <= SUM_TOL, dev


def test_expand_x_false_with_three_wavenumbers():
    """Tree a, three wavenumbers around the stored density (a coefficient array is a valid expansion at any k), each system with its own
    points: every slice equals the single-k call bit for bit."""
    rec = CASES["outer-a-k1.3"]
    ks = np.array([0.9, 1.3, 1.7])
    x = rec.x[rec.valid]
    xs = np.stack([x, x + 0.011, x * 1.01], axis=-1)                                     # [P, d, 3]
    batch = _calculator(rec, density=np.broadcast_to(rec.density, (3,) + rec.density.shape).copy(), centers=rec.centers, k=ks)
    got = batch.uscat_hess(t(xs.transpose(1, 0, 2)), expand_x=False).cpu().numpy()
    assert got.shape == (2, 2, len(x), 3) and np.isfinite(got).all()
    for s in range(3):
        one = _calculator(rec, k=ks[s]).uscat_hess(t(xs[:, :, s].T)).cpu().numpy()
        assert _same_bits(got[..., s], one), s
    shared = batch.uscat_hess(t(x.T)).cpu().numpy()                                      # expand_x=True: the points shared by the systems
    assert shared.shape == (2, 2, len(x), 3)
    assert _same_bits(shared[..., 1], _calculator(rec).uscat_hess(t(x.T)).cpu().numpy())


def test_numpy_round_trip_and_argument_errors():
    rec = CASES["outer-ba-k1.3"]
    cn = amd.BIEMResultCalculator(c=amd.create_from_branching_types(rec.tree), centers=rec.centers.T, radii=rec.radii, k=np.array(rec.k),
                                  n_end=rec.n_end, eta=np.array(1.0), kind="outer", density=rec.density)
    out = cn.uscat_hess(rec.x.T)
    assert isinstance(out, np.ndarray) and out.dtype == np.complex128 and out.shape == (3, 3, len(rec.x))
    assert np.abs(out[:, :, rec.valid] - rec.hess[:, :, rec.valid]).max() <= PARITY_TOL * np.abs(rec.hess[:, :, rec.valid]).max()
    assert isinstance(amd.biem_u_hess(cn, rec.x.T, per_ball=True), np.ndarray)
    with pytest.raises(ValueError, match="x must have shape"):
        cn.uscat_hess(np.zeros((4, 4)))


def _trace_residual(calc, x, k):
    """max |sum_i H_ii + k^2 uscat| over the valid points, in units of max |H|, both from the device."""
    H = calc.uscat_hess(x).cpu().numpy()
    u = calc.uscat(x).cpu().numpy()
    v = ~np.isnan(u)
    d = H.shape[0]
    assert np.array_equal(np.isnan(H), np.broadcast_to(~v, H.shape))
    return np.abs(sum(H[i, i] for i in range(d)) + complex(k) ** 2 * u)[v].max() / np.abs(H[:, :, v]).max()


@pytest.mark.parametrize("cid", sorted(CASES))
def test_trace_is_the_helmholtz_equation(cid):
    """sum_i H_ii + k^2 uscat = 0 against the existing uscat on the device, both kinds."""
    rec = CASES[cid]
    res = _trace_residual(_calculator(rec), t(rec.x.T), rec.k)
    print(f"  {cid}: |tr H + k^2 u| = {res:.2e} of max|H|")
    assert res <= PARITY_TOL, res


# ---------------------------------------------------------------------------- a chain tree, end to end
CHAIN = dict(bt="bbba", n_end=3, k=1.1, centers=np.array([[1.7, 0.9, -0.6, 0.5, 0.3], [-1.4, -1.1, 0.8, -0.7, -0.4]]), radii=np.array([1.0, 0.7]))
STEPS = (2e-3, 1e-3)
_chain = {}


def _chain_solve():
    if not _chain:
        d = 5
        dirn = np.array([0.9, -0.5, 0.7, 0.3, -0.4])
        k = t(CHAIN["k"])
        uin, ugr = amd.plane_wave(k=k, direction=t(dirn / np.linalg.norm(dirn)))
        calc = amd.biem(amd.create_from_branching_types(CHAIN["bt"]), centers=t(CHAIN["centers"]), radii=t(CHAIN["radii"]), k=k,
                        n_end=CHAIN["n_end"], eta=t(1.0), uin=uin, uin_grad=ugr)
        e, cen, rad = np.eye(d), CHAIN["centers"], CHAIN["radii"]
        gen = np.array([0.3, -0.8, 0.45, 0.6, -0.2])
        x = np.array([3.5 * gen / np.linalg.norm(gen), np.zeros(d), cen[1] + 1.2 * rad[1] * e[0], cen[0] - 1.3 * rad[0] * e[0],
                      cen[0] + 1.25 * rad[0] * np.array([0.0, 0.0, 0.0, 0.6, -0.8]), cen[1] + 1.25 * rad[1] * np.array([0.0, 0.6, 0.0, 0.0, 0.8]),
                      cen[0] + 1.1 * rad[0] * np.array([-0.5, 0.4, 0.6, -0.3, 0.2]) / np.linalg.norm([-0.5, 0.4, 0.6, -0.3, 0.2]),
                      cen[0] + 0.5 * rad[0] * e[2]])                                    # the last one is inside ball 0
        _chain.update(calc=calc, x=x)
    return _chain["calc"], _chain["x"]


def test_chain_tree_trace_after_a_solve():
    """bbba (d = 5), n_end 3, two balls, solved end to end by amd.biem: the Hessian runs at the chain plan of order 5."""
    calc, x = _chain_solve()
    H = calc.uscat_hess(t(x.T)).cpu().numpy()
    assert H.shape == (5, 5, len(x)) and np.isnan(H[:, :, -1]).all() and np.isfinite(H[:, :, :-1]).all()
    assert _same_bits(H, H.transpose(1, 0, 2))
    res = _trace_residual(calc, t(x.T), CHAIN["k"])
    print(f"  bbba: |tr H + k^2 u| = {res:.2e} of max|H|")
    assert res <= PARITY_TOL, res


def _second_differences(calc, x, h):
    """[d, d, P]: second central differences (diagonal) and four-point cross differences of uscat on the device."""
    P, d = x.shape
    e = np.eye(d)
    u = lambda y: calc.uscat(t(y.T)).cpu().numpy()
    u0 = u(x)
    H = np.zeros((d, d, P), dtype=np.complex128)
    for i in range(d):
        H[i, i] = (u(x + h * e[i]) - 2 * u0 + u(x - h * e[i])) / (h * h)
        for j in range(i + 1, d):
            H[i, j] = H[j, i] = (u(x + h * (e[i] + e[j])) - u(x + h * (e[i] - e[j])) - u(x - h * (e[i] - e[j])) + u(x - h * (e[i] + e[j]))) / (4 * h * h)
    return H


def test_chain_tree_against_second_differences_of_uscat():
    """The only Hessian yardstick a chain tree has: uscat_grad is not built there and the oracle has no chain tree, so the existing uscat
    on the device is differenced twice, with h = 2e-3 and h = 1e-3.  The tolerance is ten times the mutual difference of the two.  That
    is their truncation, D(2h) - D(h) = (h^2 / 4) f'''' (the rounding eps / h^2 = 2e-10 is far below it), so uscat_hess should lie a third
    of it from D(h).  Measured: mutual difference 1.15e-5 of max |H| = 8.95, |GPU - D(1e-3)| = 3.83e-6 - that third.
    The mutual difference itself must stay below 3e-5, so that the tolerance cannot grow with a broken yardstick: a term of degree
    n < 3 about a centre at distance r has f'''' / f'' ~ (n + d + 1) (n + d + 2) / r^2 <= 72 / 0.84^2 = 102 at the nearest point (1.2 rho
    from the centre of the smaller ball), and (h^2 / 4) 102 = 2.6e-5."""
    calc, x = _chain_solve()
    x = x[:-1]
    got = calc.uscat_hess(t(x.T)).cpu().numpy()
    d2, d1 = (_second_differences(calc, x, h) for h in STEPS)
    scale = np.abs(got).max()
    mutual, err = np.abs(d2 - d1).max() / scale, np.abs(got - d1).max() / scale
    print(f"  bbba: differences h=2e-3 / 1e-3 agree within {mutual:.2e}, |GPU - differences(1e-3)| = {err:.2e} of max|H| = {scale:.3e}")
    assert mutual <= 3e-5, mutual
    assert err <= 10 * mutual, (err, mutual)
