"""GPU tests of ``calc.power()`` / ``biem_power`` and ``calc.far_pattern()`` / ``biem_far_pattern``.

Parity is against tests/power_yardstick.py (the three formulas in NumPy on the CPU oracle's solution; tests/test_power_host.py pins
that yardstick by energy balance, optical theorem and the flux of the oracle's near field) within the parity contract of BASELINE.md,
1e-10.  The oracle knows one (alpha, beta) per ball; matrix and right-hand side are linear in the pair, so every case of a tree -
the degree-dependent fluid included - is solved from ONE pair of Dirichlet / Neumann systems, assembled once per tree
(the construction of tests/test_gpu_degree_bc.py).  The second route shares no formula with the kernel: the library's own uscat and
uscat_grad on a sphere around the cluster, integrated with two rules of the oracle tree.
"""
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

import power_yardstick as PY  # noqa: E402
from test_chain_trees_host import chain  # noqa: E402
from test_power_host import COEFFICIENTS, K, geometry  # noqa: E402

ETA = 1.0
FLUID = ((2.1, 0.9 + 0.1j), (0.5, 3.0))          # k_interior, density ratio per ball: a slow drop and an absorbing light one
CASES = sorted(COEFFICIENTS) + ["fluid"]
N_END = {"bbba": 4}                               # every other tree: 8


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


def _n_end(tree):
    return N_END.get(tree, 8)


# ---------------------------------------------------------------------------- the reference: one D / N pair per tree
def _fluid_pairs(d, n_end, rad):
    """alpha_n = -k_b j_n'(k_b rho), beta_n = delta j_n(k_b rho) from the oracle's radial functions, unscaled ([B, n_end]): the powers
    do not depend on the positive scale the library's helper applies per degree."""
    an = np.zeros((len(rad), n_end), dtype=np.complex128)
    bn = np.zeros_like(an)
    for b, (kb, delta) in enumerate(zip(*FLUID)):
        z = kb * rad[b]
        j, _, jp, _ = O.radial_h(n_end - 1, d, z if np.imag(z) != 0 else float(np.real(z)))
        an[b], bn[b] = -kb * jp, delta * j
    return an, bn


@lru_cache(maxsize=None)
def _dn_systems(tree):
    n_end = _n_end(tree)
    registered = tree in O._TREES
    if not registered:                            # a standard chain: the oracle takes it as a registered tree, with its quadrature (S|R)
        O._TREES[tree] = chain(len(tree) + 1)
        O._sr_tables.cache_clear()
    try:
        tr = O.tree(tree)
        cen, rad, p = geometry(tr.d)
        sr, seen = (O.translation_SR if registered else O.translation_SR_quadrature), {}

        def sr_once(tr_, n_end_, k_, tvec):       # the Neumann assembly reuses the translations of the Dirichlet one
            key = tuple(tvec)
            if key not in seen:
                seen[key] = sr(tr_, n_end_, k_, tvec)
            return seen[key]

        one, zero = np.ones(2), np.zeros(2)
        A_D, tabs = O.assemble(tr, n_end, K, ETA, cen, rad, one, zero, sr_func=sr_once)
        A_N, _ = O.assemble(tr, n_end, K, ETA, cen, rad, zero, one, sr_func=sr_once)
        uin, ugr = O.plane_wave(K, p)
        f_D = O.rhs_expansion(tr, n_end, cen, rad, one, zero, uin, None)
        f_N = O.rhs_expansion(tr, n_end, cen, rad, zero, one, None, ugr)
    finally:
        if not registered:
            del O._TREES[tree]
            O._sr_tables.cache_clear()
    blc = np.stack([tb[2] for tb in tabs])
    for a in (A_D, A_N, f_D, f_N, blc):
        a.setflags(write=False)
    return tr, cen, rad, p, uin, ugr, A_D, A_N, f_D, f_N, blc


def _pairs(tree, case):
    tr, _, rad = _dn_systems(tree)[:3]
    if case == "fluid":
        return _fluid_pairs(tr.d, _n_end(tree), rad)
    return PY.degree_pair(*COEFFICIENTS[case], 2, _n_end(tree))


@lru_cache(maxsize=None)
def _reference(tree, case):
    """(OracleResult, P_ext[B], P_abs[B], P_sca) of the yardstick (computed once, never modified)."""
    tr, cen, rad, _, uin, ugr, A_D, A_N, f_D, f_N, blc = _dn_systems(tree)
    n_end = _n_end(tree)
    deg = tr.degrees(n_end)
    H = len(deg)
    an, bn = _pairs(tree, case)
    a, b = an[:, deg], bn[:, deg]
    A = a[:, :, None, None] * A_D + b[:, :, None, None] * A_N
    f = a * f_D + b * f_N
    dens = np.linalg.solve(A.reshape(2 * H, 2 * H), f.reshape(2 * H)).reshape(2, H)
    res = O.OracleResult(tr, n_end, K, ETA, cen, rad, dens, dens * blc[:, deg], None, f)
    return (res,) + PY.power(res, uin, ugr, an, bn)


def _coefficient_kwargs(amd, tree, case):
    d = amd.create_from_branching_types(tree).c_ndim
    rad = geometry(d)[1]
    if case == "fluid":
        an, bn = amd.fluid_inclusion_bc(c_ndim=d, n_end=_n_end(tree), radii=t(rad), k_interior=tc(FLUID[0]), density_ratio=t(FLUID[1]), k=t(K))
        return dict(alpha_n=an, beta_n=bn)
    a, b = COEFFICIENTS[case]
    return dict(alpha=tc(a) if np.ndim(a) else a, beta=tc(b) if np.ndim(b) else b)


def _solve(amd, tree, case):
    c = amd.create_from_branching_types(tree)
    cen, rad, p = geometry(c.c_ndim)
    uin, ugr = amd.plane_wave(k=t(K), direction=t(p))
    kw = _coefficient_kwargs(amd, tree, case)
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=_n_end(tree), uin=uin, uin_grad=ugr, **kw)
    return calc, ugr, kw


# ---------------------------------------------------------------------------- 1. parity with the yardstick
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "bpbpa", "caa", "bbba"])
def test_power_against_yardstick(amd, tree, case):
    _, ext0, abs0, sca0 = _reference(tree, case)
    calc, ugr, kw = _solve(amd, tree, case)
    pw = calc.power(uin_grad=ugr, **kw)
    assert isinstance(pw, amd.BIEMPower)
    ext, ab, sca = (v.cpu().numpy() for v in (pw.extinction, pw.absorption, pw.scattering))
    assert ext.shape == ab.shape == (2,) and sca.shape == () and ext.dtype == ab.dtype == sca.dtype == np.float64
    scale = np.abs(ext0).sum()
    err_e, err_a = np.abs(ext - ext0).max() / scale, np.abs(ab - abs0).max() / scale
    print(f"{tree} {case}: P_ext {ext} P_abs {ab} P_sca {sca:.12f}  errors / sum |P_ext|: {err_e:.1e} {err_a:.1e}")
    assert err_e <= 1e-10 and err_a <= 1e-10
    assert abs(sca - (ext.sum() - ab.sum())) <= 1e-14 * scale
    assert abs(sca - sca0) <= 2e-10 * scale
    if case == "soft":
        assert (ab == 0.0).all()                  # beta = 0: exactly zero, nothing divided
    else:
        assert (ab[np.abs(abs0) > 0] > 0).all()


# ---------------------------------------------------------------------------- 2. a route that shares no formula with the kernel
@pytest.mark.parametrize("case", sorted(COEFFICIENTS))
@pytest.mark.parametrize("tree", ["a", "ba", "bba", "caa"])
def test_scattered_power_is_the_flux_of_the_library_s_field(amd, tree, case):
    """(1/k) sum_q w_q R^{d-1} Im[conj(u) x^_q . grad u] at R = 4.5 from uscat and uscat_grad, with the oracle tree's rules of 32 and
    40 points per node: on the CPU, with the oracle's field, 32 already agrees with 40, 48 and 56 to 1e-12 of P_sca on every tree."""
    calc, ugr, kw = _solve(amd, tree, case)
    pw = calc.power(uin_grad=ugr, **kw)
    sca, ext = float(pw.scattering), float(pw.extinction.sum())
    R, tr, flux = 4.5, O.tree(tree), []
    for nq in (32, 40):
        y, w = tr.quadrature(nq)
        x = t(R * y.T)
        u = calc.uscat(x).cpu().numpy()
        du = np.sum(calc.uscat_grad(x).cpu().numpy() * y.T, axis=0)
        flux.append(PY.flux(K, R, y, w, u, du))
    print(f"{tree} {case}: P_sca {sca:.12f}  flux {flux[0]:.12f} {flux[1]:.12f}  rules {abs(flux[0] - flux[1]) / sca:.1e}  "
          f"difference / P_ext {abs(sca - flux[1]) / ext:.1e}")
    assert abs(flux[0] - flux[1]) <= 1e-11 * sca                                  # guards the yardstick: the rule resolves the integrand
    assert abs(sca - flux[1]) <= 1e-9 * ext


# ---------------------------------------------------------------------------- 3. far_pattern
def _directions(d, P=7):
    x = np.random.default_rng(d).normal(size=(P, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("tree", ["ba", "caa", "bbba"])
def test_far_pattern_against_yardstick(amd, tree):
    res = _reference(tree, "robin")[0]
    calc, _, _ = _solve(amd, tree, "robin")
    xh = _directions(res.tree.d)
    F0, Fb0 = PY.far_pattern(res, xh), PY.far_pattern(res, xh, per_ball=True)
    F = calc.far_pattern(t(xh.T)).cpu().numpy()
    Fb = calc.far_pattern(t(xh.T), per_ball=True).cpu().numpy()
    assert F.shape == (len(xh),) and Fb.shape == (len(xh), 2)
    scale = np.abs(F0).max()
    print(f"{tree}: {np.abs(F - F0).max() / scale:.1e}  per ball {np.abs(Fb - Fb0).max() / scale:.1e}")
    assert np.abs(F - F0).max() <= 1e-10 * scale and np.abs(Fb - Fb0).max() <= 1e-10 * scale
    # the reference's far-field formula, kept as it is, is another function off the origin
    assert np.abs(calc.uscat(t(xh.T), far_field=True).cpu().numpy() - F0).max() > 0.01 * scale


def test_far_pattern_normalises_directions_one_ball_at_the_origin_and_complex_k(amd):
    c = amd.create_from_branching_types("ba")
    xh = _directions(3)
    for k in (K, K + 0.2j):
        kt = t(k) if np.isreal(k) else tc(k)
        uin, ugr = amd.plane_wave(k=kt, direction=t([0.6, 0.8, 0.0]))
        one = amd.biem(c, centers=t(np.zeros((1, 3))), radii=t([1.0]), k=kt, eta=t(ETA), n_end=8, uin=uin, uin_grad=ugr)
        F = one.far_pattern(t(xh.T)).cpu().numpy()
        ref = one.uscat(t(xh.T), far_field=True).cpu().numpy()
        assert np.abs(F - ref).max() <= 1e-13 * np.abs(ref).max()                  # at the origin the two formulas are one
        cen, rad, p = geometry(3)
        two = amd.biem(c, centers=t(cen), radii=t(rad), k=kt, eta=t(ETA), n_end=8, uin=uin, uin_grad=ugr)
        uo, go = O.plane_wave(k, p)
        res = O.solve_biem("ba", centers=cen, radii=rad, k=k, n_end=8, uin=uo, uin_grad=go)
        F2, F0 = two.far_pattern(t(xh.T)).cpu().numpy(), PY.far_pattern(res, xh)
        assert np.abs(F2 - F0).max() <= 1e-10 * np.abs(F0).max()
    assert np.abs(two.far_pattern(t(3.0 * xh.T)).cpu().numpy() - F2).max() <= 1e-14 * np.abs(F2).max()     # a direction of length 3
    x0 = xh.T.copy()
    x0[:, 2] = 0.0
    F3 = two.far_pattern(t(x0)).cpu().numpy()                                                            # a zero vector: NaN, there only
    assert np.isnan(F3[2]) and np.isfinite(np.delete(F3, 2)).all()
    assert np.abs(np.delete(F3, 2) - np.delete(F2, 2)).max() <= 1e-14 * np.abs(F2).max()


# ---------------------------------------------------------------------------- 4. batches and right-hand sides
def test_batch_of_wavenumbers_and_incidences(amd):
    """3 wavenumbers x 4 incidence directions: the directions are right-hand sides of one factorisation per wavenumber."""
    tree, n_end, alpha, beta = "ba", 6, 1.0 + 0.5j, 0.3 - 0.2j
    c = amd.create_from_branching_types(tree)
    cen, rad, _ = geometry(3)
    ks = np.array([0.9, 1.3, 1.7])
    dirs = np.array([[0.6, 0.8, 0.0], [1.0, 0.0, 0.0], [0.0, -0.6, 0.8], [0.3, 0.4, -0.5]]).T             # (3, 4)
    kb, db = ks[:, None], dirs[:, None, :]
    op = dict(centers=cen[None, None], radii=rad[None, None], k=kb, eta=np.ones((3, 1)), n_end=n_end, alpha=alpha, beta=beta)
    uin, ugr = amd.plane_wave(k=kb, direction=db)
    got = {}
    calc = amd.biem(c, uin=uin, uin_grad=ugr, **op)
    got["biem"] = calc.power(uin_grad=ugr, alpha=alpha, beta=beta)
    again = calc.power(uin_grad=ugr, alpha=alpha, beta=beta)
    fac = amd.biem_factorize(c, **op)
    got["factorize"] = fac.solve(uin=uin, uin_grad=ugr).power(uin_grad=ugr, alpha=alpha, beta=beta)
    for name, pw in got.items():
        for v, shape in ((pw.extinction, (3, 4, 2)), (pw.absorption, (3, 4, 2)), (pw.scattering, (3, 4))):
            assert isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == shape, name          # NumPy in, NumPy out
    for f in ("extinction", "absorption", "scattering"):
        assert np.array_equal(getattr(got["biem"], f), getattr(again, f))                                 # two calls: the same bits
    F = calc.far_pattern(dirs)
    assert isinstance(F, np.ndarray) and F.shape == (4, 3, 4) and np.isfinite(F).all()                    # (directions, ...(first))
    for i, k in enumerate(ks):
        for j in range(4):
            u1, g1 = amd.plane_wave(k=t(k), direction=t(dirs[:, j]))
            one = amd.biem(c, centers=t(cen), radii=t(rad), k=t(k), eta=t(1.0), n_end=n_end, alpha=alpha, beta=beta, uin=u1, uin_grad=g1)
            p1 = one.power(uin_grad=g1, alpha=alpha, beta=beta)
            e1, a1, s1 = (v.cpu().numpy() for v in (p1.extinction, p1.absorption, p1.scattering))
            for name, pw in got.items():
                scale = np.abs(e1).sum()
                assert np.abs(pw.extinction[i, j] - e1).max() <= 1e-12 * scale, (name, i, j)
                assert np.abs(pw.absorption[i, j] - a1).max() <= 1e-12 * scale, (name, i, j)
                assert abs(pw.scattering[i, j] - s1) <= 1e-12 * scale, (name, i, j)


def test_explicit_uin_equals_the_stored_one(amd):
    calc, ugr, kw = _solve(amd, "a", "robin")
    uin, _ = amd.plane_wave(k=t(K), direction=t(geometry(2)[2]))
    a, b = calc.power(uin_grad=ugr, **kw), calc.power(uin=uin, uin_grad=ugr, **kw)
    assert torch.equal(a.extinction, b.extinction) and torch.equal(a.absorption, b.absorption) and torch.equal(a.scattering, b.scattering)
    assert a.extinction.is_cuda


# ---------------------------------------------------------------------------- 5. edge cases that must not divide
def test_lossless_fluid_at_a_degree_it_does_not_scatter(amd):
    """A lossless fluid ball whose interior wavenumber is tuned so that gj_1 = alpha_1 j_1 + beta_1 k j_1' vanishes to rounding: the
    pair is real, Im(alpha conj beta) = 0 exactly, so the absorption is exactly 0 and nothing is divided by gj."""
    from scipy.optimize import brentq

    d, n_end, delta = 3, 6, 0.5
    cen, rad, p = geometry(d)
    j, _, jp, _ = O.radial_h(n_end - 1, d, K * rad[0])

    def gj1(kb):
        ji, _, jpi, _ = O.radial_h(n_end - 1, d, kb * rad[0])
        return -kb * jpi[1] * j[1] + delta * ji[1] * K * jp[1]

    grid = np.linspace(0.5, 6.0, 200)
    vals = np.array([gj1(x) for x in grid])
    i = int(np.nonzero(np.sign(vals[:-1]) != np.sign(vals[1:]))[0][0])
    kb0 = brentq(gj1, grid[i], grid[i + 1], xtol=1e-15, rtol=1e-15)
    assert abs(gj1(kb0)) < 1e-14
    c = amd.create_from_branching_types("ba")
    an, bn = amd.fluid_inclusion_bc(c_ndim=d, n_end=n_end, radii=t(rad), k_interior=t([kb0, 2.1]), density_ratio=t([delta, 0.5]), k=t(K))
    assert not an.is_complex() or float(an.imag.abs().max()) == 0.0
    uin, ugr = amd.plane_wave(k=t(K), direction=t(p))
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(K), eta=t(ETA), n_end=n_end, uin=uin, uin_grad=ugr, alpha_n=an, beta_n=bn)
    pw = calc.power(uin_grad=ugr, alpha_n=an, beta_n=bn)
    ext, ab = pw.extinction.cpu().numpy(), pw.absorption.cpu().numpy()
    print(kb0, ext, ab, float(pw.scattering))
    assert np.isfinite(ext).all() and (ab == 0.0).all() and float(pw.scattering) == ext.sum()
    assert ext.sum() > 0
