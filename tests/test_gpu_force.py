"""GPU tests of ``calc.force()`` / ``biem_force``.

The kernel's arithmetic is checked against tests/force_yardstick.py applied to the DEVICE'S OWN density copied to the host (so the
solve does not enter: 1e-12 of max |Phi| per system), end to end against the oracle's solution, and by the momentum balance from the
library's own ``calc.power()`` and ``calc.far_pattern()``.  tests/test_force_host.py pins the yardstick by two independent routes.
"""
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

import force_yardstick as FY  # noqa: E402
import power_yardstick as PY  # noqa: E402
from test_force_host import MEASURED_MOMENTUM, MOMENTUM_RULE, registered  # noqa: E402
from test_power_host import COEFFICIENTS, K, geometry  # noqa: E402

ETA = 1.0
FLUID = ((2.1, 0.9 + 0.1j), (0.5, 3.0))          # k_interior, density ratio per ball (tests/test_gpu_power.py)
KS = np.array([0.9, 1.3, 1.7])
CASES = sorted(COEFFICIENTS) + ["fluid"]
END_TO_END_MEASURED = 2.9e-15                     # |Phi - yardstick on the oracle's solution| / max |Phi|, measured on an MI355X


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), device="cuda").to(dtype).contiguous()


def tc(a):
    return t(a, torch.complex128)


@lru_cache(maxsize=None)
def _coupling(tree, n_end):
    with registered(tree) as tr:
        T = FY.coupling(tr, n_end)
    T.setflags(write=False)
    return T


def _oracle_tree(tree):
    with registered(tree) as tr:
        return tr


def yardstick(tree, n_end, k, cen, rad, density, an, bn):
    """Phi[B, d] of the yardstick for one system from a density [B, H] (the library's scaling: c = density blc)."""
    tr = _oracle_tree(tree)
    deg = tr.degrees(n_end)
    blc = np.stack([O.ball_tables(tr, n_end, float(k), ETA, rho, 1.0, 0.0)[2] for rho in rad])
    res = O.OracleResult(tr, n_end, float(k), ETA, np.asarray(cen), np.asarray(rad), density, density * blc[:, deg], None, None)
    return FY.force(res, an, bn, _coupling(tree, n_end))


# ---------------------------------------------------------------------------- 1. the kernel's arithmetic
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "bpbpa", "caa", "bbba"])
def test_force_against_yardstick_on_the_device_s_density(amd, tree, case):
    """n_end 4, 2 balls, 3 wavenumbers (systems) x 2 incidence directions (right-hand sides of one operator); the per-ball case has the
    radii batched over the wavenumbers."""
    n_end = 4
    c = amd.create_from_branching_types(tree)
    d = c.c_ndim
    cen, rad, p = geometry(d)
    p2 = np.roll(p, 1)
    kb = KS[:, None]                                                                  # (3, 1)
    dirs = np.stack([p, p2], axis=-1)[:, None, :]                                     # (d, 1, 2)
    rad_b = rad[None, None, :] * (np.array([1.0, 0.9, 1.1])[:, None, None] if case == "per_ball" else np.ones((1, 1, 1)))
    if case == "fluid":
        an, bn = amd.fluid_inclusion_bc(c_ndim=d, n_end=n_end, radii=t(rad), k_interior=tc(FLUID[0]), density_ratio=t(FLUID[1]), k=t(kb))
        kw = dict(alpha_n=an, beta_n=bn)
        pairs = [(an[i, 0].cpu().numpy(), bn[i, 0].cpu().numpy()) for i in range(3)]
    else:
        a, b = COEFFICIENTS[case]
        per_ball = lambda v: tc(np.reshape(v, (1, 1, -1))) if np.ndim(v) else v         # (..., B) with the axes of k in front
        kw = dict(alpha=per_ball(a), beta=per_ball(b))
        pairs = [PY.degree_pair(a, b, 2, n_end)] * 3
    uin, ugr = amd.plane_wave(k=t(kb), direction=t(dirs))
    calc = amd.biem(c, centers=t(cen[None, None]), radii=t(rad_b), k=t(kb), eta=t(np.ones((3, 1))), n_end=n_end, uin=uin, uin_grad=ugr, **kw)
    phi = calc.force(**kw)
    assert phi.is_cuda and phi.dtype == torch.float64 and tuple(phi.shape) == (d, 3, 2, 2)
    phi, dens = phi.cpu().numpy(), calc.density.cpu().numpy()
    assert dens.shape[:3] == (3, 2, 2)
    worst = 0.0
    for i in range(3):
        radii = np.broadcast_to(rad_b, (3, 1, 2))[i, 0]
        for j in range(2):
            ref = yardstick(tree, n_end, KS[i], cen, radii, dens[i, j], *pairs[i])               # [B, d]
            err = np.abs(phi[:, i, j, :].T - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= 1e-12, (tree, case, i, j, err)
    print(f"{tree} {case}: Phi(k={KS[0]}, first direction) {phi[:, 0, 0, :].T.tolist()}  worst error / max |Phi| {worst:.1e}")


@pytest.mark.parametrize("tree,n_end,B", [("ba", 9, 1), ("ba", 9, 3), ("a", 40, 1), ("a", 40, 3)])
def test_shapes_where_the_lane_stride_wraps(amd, tree, n_end, B):
    """More harmonics than lanes (ba: H = 81, a: H = 79), one ball and three."""
    c = amd.create_from_branching_types(tree)
    d = c.c_ndim
    cen = np.zeros((B, d))
    cen[:, 0] = 2.4 * np.arange(B)
    cen[:, 1] = 0.3 * np.arange(B) ** 2
    rad = np.array([1.0, 0.7, 0.85])[:B]
    a, b = COEFFICIENTS["robin"]
    uin, ugr = amd.plane_wave(k=t(K), direction=t(geometry(d)[2]))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=n_end, alpha=a, beta=b, uin=uin, uin_grad=ugr)
    phi = calc.force(alpha=a, beta=b).cpu().numpy()
    assert phi.shape == (d, B)
    ref = yardstick(tree, n_end, K, cen, rad, calc.density.cpu().numpy(), *PY.degree_pair(a, b, B, n_end))
    err = np.abs(phi.T - ref).max() / np.abs(ref).max()
    print(f"{tree} n_end {n_end} B {B}: Phi {phi.T.tolist()}  error / max |Phi| {err:.1e}")
    assert err <= 1e-12


# ---------------------------------------------------------------------------- 2. end to end
def test_end_to_end_against_the_oracle_s_solution(amd):
    """The library's solve and force against the oracle's solve and the yardstick (ba, n_end 8, the absorbing Robin pair).  Measured on
    an MI355X: 2.9e-15 of max |Phi| (END_TO_END_MEASURED); asserted with a factor 10, never looser than the parity contract 1e-10."""
    tree, n_end = "ba", 8
    a, b = COEFFICIENTS["robin"]
    cen, rad, p = geometry(3)
    uo, go = O.plane_wave(K, p)
    res = O.solve_biem(tree, centers=cen, radii=rad, k=K, n_end=n_end, alpha=a, beta=b, uin=uo, uin_grad=go)
    ref = FY.force(res, a, b, _coupling(tree, n_end))
    c = amd.create_from_branching_types(tree)
    uin, ugr = amd.plane_wave(k=t(K), direction=t(p))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=n_end, alpha=a, beta=b, uin=uin, uin_grad=ugr)
    phi = calc.force(alpha=a, beta=b).cpu().numpy().T
    err = np.abs(phi - ref).max() / np.abs(ref).max()
    print(f"end to end: Phi {phi.tolist()}  error / max |Phi| {err:.2e}")
    assert err <= min(10 * END_TO_END_MEASURED, 1e-10)


@pytest.mark.parametrize("case", ["soft", "robin"])
@pytest.mark.parametrize("tree", ["a", "ba", "bba"])
def test_momentum_balance_on_the_device(amd, tree, case):
    """sum_b calc.force() = P_ext p^ - int |F|^2 x^ dOmega with calc.power() and a quadrature of calc.far_pattern(): the geometry, the
    rule and the bound (three times the truncation measured at n_end 10) of tests/test_force_host.py."""
    n_end = 10
    c = amd.create_from_branching_types(tree)
    cen, rad, p = geometry(c.c_ndim)
    a, b = COEFFICIENTS[case]
    uin, ugr = amd.plane_wave(k=t(K), direction=t(p))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=n_end, alpha=a, beta=b, uin=uin, uin_grad=ugr)
    phi = calc.force(alpha=a, beta=b).cpu().numpy()                                 # (d, B)
    ext = calc.power(uin_grad=ugr, alpha=a, beta=b).extinction.cpu().numpy()
    y, w = O.tree(tree).quadrature(MOMENTUM_RULE[tree])
    F = calc.far_pattern(t(y.T)).cpu().numpy()
    balance = ext.sum() * p - np.sum((w * np.abs(F) ** 2)[:, None] * y, axis=0)
    err = np.abs(phi.sum(-1) - balance).max() / np.abs(phi).max()
    print(f"{tree} {case}: sum Phi {phi.sum(-1)}  balance {balance}  difference / max |Phi| {err:.2e}")
    assert err <= 3 * MEASURED_MOMENTUM[tree, case]


# ---------------------------------------------------------------------------- 3. individual cases
def test_bpa_is_ba_in_permuted_axes(amd):
    """bpa runs as ba with y_i = x_{perm[i]}, perm = (2, 1, 0): the same numbers, component for component (the incident samples are
    dot products summed in another order, hence rounding and not bits)."""
    perm = [2, 1, 0]
    cen, rad, p = geometry(3)
    cen[:, 2] = (0.4, -0.3)
    p = np.array([0.6, 0.64, 0.48])
    a, b = COEFFICIENTS["robin"]
    out = {}
    for tree, cc, pp in (("bpa", cen, p), ("ba", cen[:, perm], p[perm])):
        c = amd.create_from_branching_types(tree)
        uin, ugr = amd.plane_wave(k=t(K), direction=t(pp))
        calc = amd.biem(c, centers=t(cc), radii=t(rad), k=t(K), eta=t(ETA), n_end=6, alpha=a, beta=b, uin=uin, uin_grad=ugr)
        out[tree] = calc.force(alpha=a, beta=b).cpu().numpy()
    print(out)
    assert np.abs(out["bpa"][perm] - out["ba"]).max() <= 1e-13 * np.abs(out["ba"]).max()
    assert np.abs(out["ba"][2]).min() > 1e-3 * np.abs(out["ba"]).max()              # every component takes part


def test_two_calls_are_bit_identical_and_numpy_gives_numpy(amd):
    c = amd.create_from_branching_types("ba")
    cen, rad, p = geometry(3)
    kb = KS[:, None]
    dirs = np.stack([p, np.roll(p, 1)], axis=-1)[:, None, :]
    uin, ugr = amd.plane_wave(k=kb, direction=dirs)
    calc = amd.biem(c, centers=cen[None, None], radii=rad[None, None], k=kb, eta=np.ones((3, 1)), n_end=9, uin=uin, uin_grad=ugr)
    first, again = calc.force(), amd.biem_force(calc)
    assert isinstance(first, np.ndarray) and first.dtype == np.float64 and first.shape == (3, 3, 2, 2)
    assert np.isfinite(first).all() and np.array_equal(first, again)


def test_transparent_sphere_is_nan_for_that_ball_only(amd):
    """k_interior = k, density_ratio = 1: gj_n = 0 for every degree of ball 0, whose traces the density does not determine."""
    c = amd.create_from_branching_types("ba")
    cen, rad, p = geometry(3)
    an, bn = amd.fluid_inclusion_bc(c_ndim=3, n_end=6, radii=t(rad), k_interior=t([K, 2.1]), density_ratio=t([1.0, 0.5]), k=t(K))
    uin, ugr = amd.plane_wave(k=t(K), direction=t(p))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=6, uin=uin, uin_grad=ugr, alpha_n=an, beta_n=bn)
    phi = calc.force(alpha_n=an, beta_n=bn).cpu().numpy()
    print(phi)
    assert np.isnan(phi[:, 0]).all() and np.isfinite(phi[:, 1]).all() and np.abs(phi[:, 1]).max() > 0


def test_complex_k_raises_and_one_harmonic_gives_exactly_zero(amd):
    c = amd.create_from_branching_types("ba")
    cen, rad, p = geometry(3)
    k = K + 0.2j
    uin, ugr = amd.plane_wave(k=tc(k), direction=t(p))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=tc(k), eta=t(ETA), n_end=4, uin=uin, uin_grad=ugr)
    with pytest.raises(ValueError, match="Im k must be zero"):
        calc.force()
    uin, ugr = amd.plane_wave(k=t(K), direction=t(p))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=1, uin=uin, uin_grad=ugr)
    phi = calc.force()
    assert tuple(phi.shape) == (3, 2) and bool((phi == 0.0).all())               # n_end = 1: an empty coupling table
