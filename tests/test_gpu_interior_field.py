"""GPU tests of the total field inside penetrable fluid balls: ``uinterior`` / ``utotal`` (``biem_u_interior``, ``biem_u_total``) and the
coefficient entry ``biem_interior_coef``.

Three yardsticks, each with its own tolerance:

* the analytic one-sphere series from SciPy's Bessel functions (independent of the oracle and of the tree conventions): 1e-11 of max |u|;
* the algebraic coefficients a = -s delta k W / gj evaluated in NumPy from the oracle's ``radial_h`` and ``harmonics`` on the yardstick's
  density (``_yardstick``: the oracle's Dirichlet and Neumann systems combined row by row, solved by LAPACK): 1e-11 with the same density
  on both sides, 1e-10 end to end;
* the sampled-boundary route a_mat = (A_D phi - f_D) / j_n(k_b rho), which differs from the algebraic form by the oracle's discretisation
  error: the device may differ from it by no more than the algebraic form on the CPU does (plus 1e-10).

Every test prints the error it measured.
"""
import math
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), device="cuda").to(dtype).contiguous()


def _cdev(a):
    return _dev(a, torch.complex128)


# ---------------------------------------------------------------------------- geometry and fluids (those of tests/test_gpu_degree_bc.py)
_C0 = np.array([0.3, -0.2, 0.5, 0.1, -0.4])
_STEP = np.array([[1.9, 1.1, -0.7, 0.6, 0.5], [-1.2, 2.3, 0.9, -0.8, 0.3], [-2.0, -1.7, 0.4, 1.1, -0.6]])
_RADII = np.array([1.0, 0.7, 0.85, 0.6])
_DIRECTION = np.array([0.8, -0.5, 0.3, 0.45, -0.2])
K, ETA = 1.3, 1.0

FLUIDS = {
    "two_fluids": ((2.1, 0.9 + 0.1j, 2.1), (0.5, 3.0, 0.5)),
    "bubble": (4.4 * K, 1.2e-3),
}
SINGLE = [(2.1, 0.5), (0.9 + 0.1j, 3.0), (4.4 * K, 1.2e-3)]            # the three (k_b, delta) pairs, one ball each


def _geometry(d, B, spread=1.0):
    """B balls of radii 1.0, 0.7, ... off every axis and plane of the coordinate tree (no two closer than 1.15 x the sum of radii);
    spread > 1 moves the others away from the first by that factor."""
    cen = np.stack([_C0[:d]] + [_C0[:d] + spread * _STEP[i, :d] for i in range(B - 1)])
    rad = _RADII[:B].copy()
    for i in range(B):
        for j in range(i):
            assert np.linalg.norm(cen[i] - cen[j]) > 1.15 * (rad[i] + rad[j])
    return cen, rad


def _fluid(name, B):
    kb, delta = FLUIDS[name]
    kb = np.broadcast_to(np.atleast_1d(np.asarray(kb, dtype=np.complex128))[:B], (B,)).copy()
    delta = np.broadcast_to(np.atleast_1d(np.asarray(delta, dtype=np.float64))[:B], (B,)).copy()
    return kb, delta


def _rad(nmax, d, z):
    z = complex(z)
    return O.radial_h(nmax, d, z if z.imag != 0 else z.real)


def _fluid_oracle(d, n_end, rad, kb, delta):
    """alpha_n = -k_b j_n'(k_b rho), beta_n = delta j_n(k_b rho) from the oracle's radial functions, unscaled: [B, n_end] complex."""
    B = len(rad)
    an = np.zeros((B, n_end), dtype=np.complex128)
    bn = np.zeros((B, n_end), dtype=np.complex128)
    for b in range(B):
        j, _, jp, _ = _rad(n_end - 1, d, kb[b] * rad[b])
        an[b] = -kb[b] * jp
        bn[b] = delta[b] * j
    return an, bn


@lru_cache(maxsize=None)
def _dn_systems(tree, B, n_end, spread=1.0):
    """The oracle's Dirichlet and Neumann matrices and plane-wave right-hand sides of the test geometry (computed once per shape)."""
    tr = O.tree(tree)
    cen, rad = _geometry(tr.d, B, spread)
    one, zero = np.ones(B), np.zeros(B)
    A_D, tabs = O.assemble(tr, n_end, K, ETA, cen, rad, one, zero)
    A_N, _ = O.assemble(tr, n_end, K, ETA, cen, rad, zero, one)
    uin, ugr = O.plane_wave(K, _DIRECTION[:tr.d])
    f_D = O.rhs_expansion(tr, n_end, cen, rad, one, zero, uin, None)
    f_N = O.rhs_expansion(tr, n_end, cen, rad, zero, one, None, ugr)
    blc = np.stack([t[2] for t in tabs])
    for a in (A_D, A_N, f_D, f_N, blc):
        a.setflags(write=False)
    return tr, cen, rad, A_D, A_N, f_D, f_N, blc


@lru_cache(maxsize=None)
def _yardstick(tree, B, n_end, fluid, spread=1.0):
    """(density [B, H], s = density * blc [B, H]) of the fluid problem, shared and read-only."""
    tr, cen, rad, A_D, A_N, f_D, f_N, blc = _dn_systems(tree, B, n_end, spread)
    kb, delta = _fluid(fluid, B)
    an, bn = _fluid_oracle(tr.d, n_end, rad, kb, delta)
    deg = tr.degrees(n_end)
    H = len(deg)
    a, b = an[:, deg], bn[:, deg]
    A = a[:, :, None, None] * A_D + b[:, :, None, None] * A_N
    f = a * f_D + b * f_N
    dens = np.linalg.solve(A.reshape(B * H, B * H), f.reshape(B * H)).reshape(B, H)
    s = dens * blc[:, deg]
    dens.setflags(write=False)
    s.setflags(write=False)
    return dens, s


def _alg_coef(tr, n_end, rad, s, kb, delta):
    """a[b, h] = -s delta k W / gj with W = i / (k rho)^{d-1}, gj from the unscaled pair: the definition, from the oracle's radial_h."""
    d, deg = tr.d, tr.degrees(n_end)
    a = np.zeros_like(s)
    for b in range(len(rad)):
        x = K * rad[b]
        j, _, jp, _ = _rad(n_end - 1, d, x)
        jz, _, jpz, _ = _rad(n_end - 1, d, kb[b] * rad[b])
        gj = -kb[b] * jpz * j + delta[b] * jz * K * jp
        a[b] = -s[b] * (delta[b] * K * (1j / x ** (d - 1)) / gj)[deg]
    return a


def _jn_surface(tr, n_end, rad, kb):
    """j_n(k_b rho_b) per harmonic: [B, H]."""
    deg = tr.degrees(n_end)
    return np.stack([_rad(n_end - 1, tr.d, kb[b] * rad[b])[0][deg] for b in range(len(rad))])


def _u_from_coef(tr, n_end, a, kb, cen, x, ball):
    """sum_h a[b, h] j_n(k_b r) Y_h at the points x [P, d] of the balls `ball` [P]."""
    d, deg = tr.d, tr.degrees(n_end)
    out = np.zeros(len(x), dtype=np.complex128)
    for i, (p, b) in enumerate(zip(x, ball)):
        rel = p - cen[b]
        r = np.linalg.norm(rel)
        if r > 0:
            jn = _rad(n_end - 1, d, kb[b] * r)[0]
            u = rel / r
        else:                                # z_n(0) = delta_{n0} sqrt(pi/2) 2^{1-d/2} / Gamma(d/2); any direction
            jn = np.zeros(n_end, dtype=np.complex128)
            jn[0] = math.sqrt(math.pi / 2) * 2.0 ** (1 - d / 2) / math.gamma(d / 2)
            u = np.eye(d)[0]
        out[i] = np.sum(a[b] * jn[deg] * tr.harmonics(u[None], n_end)[:, 0])
    return out


def _interior_points(cen, rad, per_ball=6, seed=5):
    """per_ball points inside every ball: the centre, one at r = 0.999 rho, the others at r / rho in [0.05, 0.95]."""
    rng = np.random.default_rng(seed)
    d = cen.shape[1]
    x, ball = [], []
    for b in range(len(rad)):
        u = rng.normal(size=(per_ball, d))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        fr = np.concatenate([[0.0, 0.999], rng.uniform(0.05, 0.95, per_ball - 2)])
        x.append(cen[b] + rad[b] * fr[:, None] * u)
        ball += [b] * per_ball
    return np.concatenate(x), np.array(ball)


def _calculator(amd, tree, n_end, cen, rad, density):
    """A result record built directly around a given density (no solve)."""
    return amd.BIEMResultCalculator(c=amd.create_from_branching_types(tree), centers=_dev(cen.T), radii=_dev(rad), k=_dev(K), n_end=n_end,
                                    eta=_dev(ETA), kind="outer", density=_cdev(density))


_SOLVED = {}


def _solve(amd, tree, B, n_end, kb, delta, spread=1.0, key=None):
    """biem(alpha_n=, beta_n=) with the helper's coefficients and a plane wave; solved once per case."""
    key = key or (tree, B, n_end, tuple(np.atleast_1d(kb)), tuple(np.atleast_1d(delta)), spread)
    if key not in _SOLVED:
        d = O.tree(tree).d
        cen, rad = _geometry(d, B, spread)
        kb_d, dl_d = _cdev(np.broadcast_to(kb, (B,))), _dev(np.broadcast_to(delta, (B,)))
        an, bn = amd.fluid_inclusion_bc(c_ndim=d, n_end=n_end, radii=_dev(rad), k_interior=kb_d, density_ratio=dl_d)
        uin, ugr = amd.plane_wave(k=_dev(K), direction=_dev(_DIRECTION[:d]))
        _SOLVED[key] = amd.biem(amd.create_from_branching_types(tree), centers=_dev(cen), radii=_dev(rad), k=_dev(K), eta=_dev(ETA),
                                n_end=n_end, alpha_n=an, beta_n=bn, uin=uin, uin_grad=ugr)
    return _SOLVED[key]


# ---------------------------------------------------------------------------- 1. one sphere against the analytic series
def _series_3d(kb, delta, cen, rho, x, terms=40, radial_derivative=False):
    """u = e^{i k d.c} sum_n (2n+1) i^n [delta k W / gh_n] j_n(k_b r) P_n(cos gamma), W = i / (k rho)^2,
    gh_n = -k_b j_n'(k_b rho) h_n(k rho) + delta j_n(k_b rho) k h_n'(k rho); radial_derivative: d/dr of it (k_b j_n'(k_b r) for j_n(k_b r))."""
    import scipy.special as sp
    dv = _DIRECTION[:3] / np.linalg.norm(_DIRECTION[:3])
    n = np.arange(terms)
    xr, z = K * rho, kb * rho
    h = sp.spherical_jn(n, xr) + 1j * sp.spherical_yn(n, xr)
    hp = sp.spherical_jn(n, xr, derivative=True) + 1j * sp.spherical_yn(n, xr, derivative=True)
    gh = -kb * sp.spherical_jn(n, z, derivative=True) * h + delta * sp.spherical_jn(n, z) * K * hp
    coef = (2 * n + 1) * 1j ** n * delta * K * (1j / xr ** 2) / gh
    rel = x - cen
    r = np.linalg.norm(rel, axis=1)
    cosg = np.where(r > 0, rel @ dv / np.where(r > 0, r, 1.0), 1.0)
    u = np.zeros(len(x), dtype=np.complex128)
    for q in n:
        jq = kb * sp.spherical_jn(q, kb * r, derivative=True) if radial_derivative else sp.spherical_jn(q, kb * r)
        u += coef[q] * jq * sp.eval_legendre(q, cosg)
    return np.exp(1j * K * dv @ cen) * u


def _series_2d(kb, delta, cen, rho, x, terms=40):
    """The Jacobi-Anger analogue: u = e^{i k d.c} sum_m i^m e^{-i m t_d} [delta k W / gh_m] J_m(k_b r) e^{i m t}, W = 2 i / (pi k rho)."""
    import scipy.special as sp
    dv = _DIRECTION[:2] / np.linalg.norm(_DIRECTION[:2])
    td = math.atan2(dv[1], dv[0])
    xr, z = K * rho, kb * rho
    rel = x - cen
    r, t = np.linalg.norm(rel, axis=1), np.arctan2(rel[:, 1], rel[:, 0])
    u = np.zeros(len(x), dtype=np.complex128)
    for m in range(-terms, terms + 1):
        gh = -kb * sp.jvp(m, z) * sp.hankel1(m, xr) + delta * sp.jv(m, z) * K * sp.h1vp(m, xr)
        u += 1j ** m * np.exp(-1j * m * td) * delta * K * (2j / (math.pi * xr)) / gh * sp.jv(m, kb * r) * np.exp(1j * m * t)
    return np.exp(1j * K * dv @ cen) * u


def _single_points(d):
    """12 interior points at r / rho in [0.05, 0.999], the centre and a point on each coordinate axis through the centre that is a polar
    axis of one of the trees (x0: a, ba; the last axis: bpa)."""
    rng = np.random.default_rng(11)
    u = rng.normal(size=(12, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    fr = np.concatenate([[0.05, 0.999], rng.uniform(0.05, 0.999, 10)])
    c = _C0[:d]
    return np.concatenate([c + fr[:, None] * u, c[None], c[None] + 0.6 * np.eye(d)[[0, d - 1]], c[None] - 0.45 * np.eye(d)[[0]]])


@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("tree", ["a", "ba", "bpa"])
def test_one_sphere_against_the_analytic_series(amd, tree, case):
    kb, delta = SINGLE[case]
    d = O.tree(tree).d
    calc = _solve(amd, tree, 1, 16, kb, delta)
    x = _single_points(d)
    ref = (_series_3d if d == 3 else _series_2d)(kb, delta, _C0[:d], 1.0, x)
    u = calc.uinterior(_dev(x.T), k_interior=_cdev([kb]), density_ratio=_dev([delta])).cpu().numpy()
    err = np.max(np.abs(u - ref)) / np.max(np.abs(ref))
    print(f"{tree} k_b={kb} delta={delta}: {err:.2e} of max |u| = {np.max(np.abs(ref)):.3f}")
    assert err <= 1e-11


# ---------------------------------------------------------------------------- 2. kernel arithmetic in isolation
SHAPES = [("a", 3, 8), ("ba", 2, 6), ("bpa", 2, 6), ("bba", 2, 4), ("bpbpa", 2, 4), ("caa", 2, 4)]


@pytest.mark.parametrize("fluid", sorted(FLUIDS))
@pytest.mark.parametrize("tree,B,n_end", SHAPES)
def test_kernels_against_the_algebraic_formula_same_density(amd, tree, B, n_end, fluid):
    """The yardstick's density on both sides: only function evaluation and the H-term sums differ."""
    from biem_helmholtz_sphere_amd import _biem, _lib as L
    from biem_helmholtz_sphere_amd._coords import canonical_tree
    tr, cen, rad = _dn_systems(tree, B, n_end)[:3]
    dens, s = _yardstick(tree, B, n_end, fluid)
    kb, delta = _fluid(fluid, B)
    a = _alg_coef(tr, n_end, rad, s, kb, delta)
    x, ball = _interior_points(cen, rad)
    ref = _u_from_coef(tr, n_end, a, kb, cen, x, ball)
    calc = _calculator(amd, tree, n_end, cen, rad, dens)
    u = calc.uinterior(_dev(x.T), k_interior=_cdev(kb), density_ratio=_dev(delta)).cpu().numpy()
    err_u = np.max(np.abs(u - ref)) / np.max(np.abs(ref))
    # the coefficient entry on its own, compared as a_{b,h} j_n(k_b rho_b) (the trace: of the field's size at every degree)
    plan = _biem._plan(canonical_tree(tree)[0], n_end, torch.device("cuda", torch.cuda.current_device()))
    H = dens.shape[1]
    out = torch.zeros((1, B, H), dtype=torch.complex128, device="cuda")
    ops = [_cdev([K]), _dev([ETA]), _dev(rad), _cdev(kb), _cdev(delta), _cdev(dens)]
    L.check(L.load().biem_interior_coef(plan.handle, 1, B, ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), 0, ops[3].data_ptr(),
                                        ops[4].data_ptr(), 0, ops[5].data_ptr(), out.data_ptr(), None), "biem_interior_coef")
    torch.cuda.synchronize()
    js = _jn_surface(tr, n_end, rad, kb)
    err_a = np.max(np.abs(out[0].cpu().numpy() * js - a * js)) / np.max(np.abs(a * js))
    print(f"{tree} B={B} n_end={n_end} {fluid}: u {err_u:.2e}, a j_n(k_b rho) {err_a:.2e}")
    assert err_u <= 1e-11
    assert err_a <= 1e-11


# ---------------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("fluid", sorted(FLUIDS))
@pytest.mark.parametrize("tree,B,n_end,spread", [("ba", 3, 7, 1.3), ("a", 3, 8, 1.0)])
def test_end_to_end_against_the_yardstick(amd, tree, B, n_end, spread, fluid):
    """biem(alpha_n=, beta_n=) then uinterior, against the algebraic formula on the yardstick's density (ba: N = 147, above the
    one-launch limit of the factorisation)."""
    tr, cen, rad = _dn_systems(tree, B, n_end, spread)[:3]
    _, s = _yardstick(tree, B, n_end, fluid, spread)
    kb, delta = _fluid(fluid, B)
    x, ball = _interior_points(cen, rad)
    ref = _u_from_coef(tr, n_end, _alg_coef(tr, n_end, rad, s, kb, delta), kb, cen, x, ball)
    calc = _solve(amd, tree, B, n_end, kb, delta, spread)
    u = calc.uinterior(_dev(x.T), k_interior=_cdev(kb), density_ratio=_dev(delta)).cpu().numpy()
    err = np.max(np.abs(u - ref)) / np.max(np.abs(ref))
    print(f"{tree} B={B} n_end={n_end} {fluid}: {err:.2e} of max |u_interior| = {np.max(np.abs(ref)):.3f}")
    assert err <= 1e-10


# ---------------------------------------------------------------------------- 4. the sampled-boundary route
@pytest.mark.parametrize("fluid", sorted(FLUIDS))
@pytest.mark.parametrize("tree,B,n_end", [("ba", 2, 6), ("a", 3, 8)])
def test_sampled_boundary_route_bounds_the_difference(amd, tree, B, n_end, fluid):
    """a_mat = (A_D phi - f_D) / j_n(k_b rho): the trace of the exterior total field projected by the oracle's rule.  It differs from the
    algebraic form by the oracle's discretisation error; the device is held to that gap, computed here, not to a chosen number."""
    tr, cen, rad, A_D, _, f_D = _dn_systems(tree, B, n_end)[:6]
    dens, s = _yardstick(tree, B, n_end, fluid)
    kb, delta = _fluid(fluid, B)
    a_mat = (np.einsum("bhcg,cg->bh", A_D, dens) - f_D) / _jn_surface(tr, n_end, rad, kb)
    x, ball = _interior_points(cen, rad)
    mat = _u_from_coef(tr, n_end, a_mat, kb, cen, x, ball)
    alg = _u_from_coef(tr, n_end, _alg_coef(tr, n_end, rad, s, kb, delta), kb, cen, x, ball)
    u = _solve(amd, tree, B, n_end, kb, delta).uinterior(_dev(x.T), k_interior=_cdev(kb), density_ratio=_dev(delta)).cpu().numpy()
    scale = np.max(np.abs(alg))
    gap_gpu, gap_cpu = np.max(np.abs(u - mat)), np.max(np.abs(alg - mat))
    print(f"{tree} {fluid}: |gpu - mat| {gap_gpu / scale:.2e}, |alg_cpu - mat| {gap_cpu / scale:.2e} of max |u|")
    assert gap_gpu <= gap_cpu + 1e-10 * scale


# ---------------------------------------------------------------------------- 5. semantics
def _semantic_points(cen, rad):
    """P = 300: 70 consecutive points outside every ball (more than a wave), 130 that alternate ball 0 / ball 1 / outside from lane to
    lane, 100 inside ball 0 (the centre among them).  Returns x [P, d] and the ball of every point (-1: none)."""
    rng = np.random.default_rng(7)
    d = cen.shape[1]

    def inside(b, n):
        u = rng.normal(size=(n, d))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return cen[b] + rad[b] * rng.uniform(0.02, 0.98, n)[:, None] * u

    def outside(n):
        out = []
        while len(out) < n:
            p = cen[0] + rng.normal(size=d) * 3.0
            if all(np.linalg.norm(p - cc) > 1.01 * rr for cc, rr in zip(cen, rad)):
                out.append(p)
        return np.array(out)

    x = np.concatenate([outside(70), np.zeros((130, d)), inside(0, 100)])
    for i in range(70, 200):
        x[i] = [inside(0, 1)[0], inside(1, 1)[0], outside(1)[0]][i % 3]
    x[250] = cen[0]
    dist = np.linalg.norm(x[:, None, :] - cen[None], axis=2)
    ball = np.where(dist[:, 0] < rad[0], 0, np.where(dist[:, 1] < rad[1], 1, -1))
    assert (ball[:70] == -1).all() and (ball[200:] == 0).all() and len(x) % 64 != 0
    assert all((ball[70:200] == b).sum() >= 30 for b in (-1, 0, 1))
    return x, ball


def test_semantics_of_the_mask_and_of_utotal(amd):
    tree, B, n_end = "ba", 2, 6
    cen, rad = _geometry(3, B)
    kb, delta = _fluid("two_fluids", B)
    calc = _solve(amd, tree, B, n_end, kb, delta)
    x, ball = _semantic_points(cen, rad)
    xd = _dev(x.T)
    kw = dict(k_interior=_cdev(kb), density_ratio=_dev(delta))
    ui = calc.uinterior(xd, **kw).cpu().numpy()
    us = calc.uscat(xd).cpu().numpy()
    assert ui.shape == us.shape == (300,)
    assert (np.isnan(ui) == (ball < 0)).all()                     # NaN exactly where no ball contains the point ...
    assert (np.isnan(us) == (ball >= 0)).all()                    # ... the complement of uscat's mask
    assert np.isfinite(ui[ball >= 0]).all()
    perm = np.random.default_rng(1).permutation(300)              # the same values in any point order
    up = calc.uinterior(_dev(x[perm].T), **kw).cpu().numpy()
    assert np.array_equal(up, ui[perm], equal_nan=True)
    ut = calc.utotal(xd, **kw).cpu().numpy()
    uin = calc.uin(xd).cpu().numpy()
    assert np.isfinite(ut).all()
    assert np.array_equal(ut[ball < 0], (uin + us)[ball < 0]) and np.array_equal(ut[ball >= 0], ui[ball >= 0])
    # an impenetrable ball: NaN inside it, the other ball unaffected
    kn = kb.copy()
    kn[1] = np.nan
    un = calc.uinterior(xd, k_interior=_cdev(kn), density_ratio=_dev(delta)).cpu().numpy()
    assert np.isnan(un[ball == 1]).all() and np.array_equal(un[ball == 0], ui[ball == 0]) and np.isnan(un[ball < 0]).all()
    assert np.isnan(calc.utotal(xd, k_interior=_cdev(kn), density_ratio=_dev(delta)).cpu().numpy()).sum() == (ball == 1).sum()
    # the sound-soft limit
    u0 = calc.uinterior(xd, k_interior=_cdev(kb), density_ratio=_dev([0.0, 0.0])).cpu().numpy()
    assert (u0[ball >= 0] == 0).all() and np.isnan(u0[ball < 0]).all()
    print(f"300 points: {int((ball == 0).sum())} in ball 0, {int((ball == 1).sum())} in ball 1, {int((ball < 0).sum())} outside; "
          f"max |u_interior| {np.nanmax(np.abs(ui)):.3f}")


def test_transparent_pair_is_nan_inside_and_no_error(amd):
    """k_b = k, delta = 1: gj_n = 0, the ball scatters no degree and the density carries nothing of the interior field."""
    tree, B, n_end = "ba", 2, 6
    cen, rad = _geometry(3, B)
    calc = _solve(amd, tree, B, n_end, K, 1.0)
    x, ball = _interior_points(cen, rad)
    u = calc.uinterior(_dev(x.T), k_interior=_cdev([K, K]), density_ratio=_dev([1.0, 1.0])).cpu().numpy()
    print(f"transparent pair: {int(np.isnan(u).sum())} of {u.size} interior points NaN")
    assert np.isnan(u).all()


# ---------------------------------------------------------------------------- 6. batches and namespaces
def test_batches_and_numpy_namespace(amd):
    """3 wavenumbers, k_interior of shape (3, B), per-system points with expand_x=False, NumPy in and out: each slice equals the
    unbatched call to 1e-13."""
    tree, B, n_end = "ba", 2, 6
    c = amd.create_from_branching_types(tree)
    cen, rad = _geometry(3, B)
    ks = np.array([0.9, 1.3, 2.2])
    kb = np.array([[2.1, 0.9 + 0.1j], [1.5, 2.4], [3.0 + 0.2j, 0.7]])
    delta = np.array([0.5, 3.0])
    rng = np.random.default_rng(2)
    P = 9
    u = rng.normal(size=(3, P, 3))
    u /= np.linalg.norm(u, axis=0, keepdims=True)
    bsel = rng.integers(0, B, P)                                                              # the ball of point p (every system)
    x = cen[bsel].T[:, :, None] + (rad[bsel][:, None] * rng.uniform(0.05, 0.95, (P, 3)))[None] * u      # (d, P, 3): other points per system
    an, bn = amd.fluid_inclusion_bc(c_ndim=3, n_end=n_end, radii=rad, k_interior=kb, density_ratio=delta)
    assert isinstance(an, np.ndarray)
    dirs = np.repeat(_DIRECTION[:3, None], 3, 1)
    uin, ugr = amd.plane_wave(k=ks, direction=dirs)
    calc = amd.biem(c, centers=cen[None], radii=rad[None], k=ks, eta=np.full(3, ETA), n_end=n_end, alpha_n=an, beta_n=bn, uin=uin, uin_grad=ugr)
    got = calc.uinterior(x, k_interior=kb, density_ratio=delta, expand_x=False)
    tot = calc.utotal(x, k_interior=kb, density_ratio=delta, expand_x=False)
    assert isinstance(got, np.ndarray) and got.shape == (P, 3) and got.dtype == np.complex128
    assert np.isfinite(got).all() and np.array_equal(tot, got)
    for s in range(3):
        # the unbatched call on the slice of the same result: only the evaluation differs (two solves agree to ~1e-10 only)
        one = amd.BIEMResultCalculator(c=c, centers=calc.centers[:, 0], radii=calc.radii[0], k=np.asarray(calc.k[s]), n_end=n_end,
                                       eta=np.asarray(calc.eta[s]), kind="outer", density=calc.density[s])
        ref = one.uinterior(x[:, :, s], k_interior=kb[s], density_ratio=delta)
        assert ref.shape == (P,)
        err = np.max(np.abs(got[:, s] - ref)) / np.max(np.abs(ref))
        print(f"system {s}: {err:.2e}")
        assert err <= 1e-13


# ---------------------------------------------------------------------------- 7. continuity at the surface
@pytest.mark.parametrize("case", range(3))
def test_continuity_across_the_surface(amd, case):
    """|u_interior(rho (1 - eps)) - (u_in + u_scat)(rho (1 + eps))| <= 2 eps rho (|k_b| + k) max |u| + 1e-11 at eps = 1e-9, 8 directions: the
    first term is the field's own variation over 2 eps rho.

    max |u| is the largest modulus of the total field along the 8 radii, from the centre to one exterior wavelength beyond the surface,
    not the modulus at the surface: a field of wavenumber kappa varies at a rate of kappa times its size nearby, and the surface of a
    nearly pressure-release ball (the bubble) is a node of u where d_r u is O(k) all the same.  With the modulus at the surface the
    bound is not a property of the field: the exact solution misses it (bubble: the SciPy series gives |u| <= 0.0022 at the surface and
    |d_r u_ext| <= 2.296, a true jump of 2.299e-09 against 4.0e-11).

    The jump is also held to its first-order value -eps rho (d_r u_int + d_r u_ext) from the series, d_r u_ext = d_r u_int / delta by the
    transmission condition, to the 1e-11 of the bound (the next order is eps^2 (|k_b|^2 + k^2) |u| <= 1e-16): a field that jumped by
    less than the bound but not by the right amount would fail here.

    Measured on an MI355X, the three cases: jump 2.55e-09, 1.75e-09, 2.30e-09 against bounds of 1.16e-08, 5.25e-09, 1.80e-08 (max |u| along
    the radii 1.698, 1.187, 1.279; at the surface 1.647, 1.131, 0.002); jump minus its first-order value 6.3e-15, 2.1e-15, 2.4e-15."""
    kb, delta = SINGLE[case]
    calc = _solve(amd, "ba", 1, 16, kb, delta)
    rng = np.random.default_rng(13)
    u = rng.normal(size=(8, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    eps, rho, c = 1e-9, 1.0, _C0[:3]
    kw = dict(k_interior=_cdev([kb]), density_ratio=_dev([delta]))
    xi, xo = _dev((c + rho * (1 - eps) * u).T), _dev((c + rho * (1 + eps) * u).T)
    inner = calc.uinterior(xi, **kw).cpu().numpy()
    outer = (calc.uin(xo) + calc.uscat(xo)).cpu().numpy()
    tot = calc.utotal(xo, **kw).cpu().numpy()
    assert np.array_equal(tot, outer)
    fr = np.concatenate([np.linspace(0.0, 1 - eps, 32), np.linspace(1 + eps, 1 + 2 * math.pi / (K * rho), 32)])
    along = calc.utotal(_dev((c + rho * fr[:, None, None] * u).reshape(-1, 3).T), **kw).cpu().numpy()
    assert np.isfinite(along).all()
    umax = np.max(np.abs(along))
    jump = np.max(np.abs(inner - outer))
    bound = 2 * eps * rho * (abs(kb) + K) * umax + 1e-11
    dr_int = _series_3d(kb, delta, c, rho, c + rho * u, radial_derivative=True)
    first_order = -eps * rho * (1 + 1 / delta) * dr_int
    off = np.max(np.abs(inner - outer - first_order))
    print(f"k_b={kb} delta={delta}: jump {jump:.2e}, bound {bound:.2e}, max |u| along the radii {umax:.3f} (at the surface "
          f"{max(np.max(np.abs(inner)), np.max(np.abs(outer))):.3f}); jump - first order {off:.2e}")
    assert jump <= bound
    assert off <= 1e-11


# ---------------------------------------------------------------------------- 8. the C entry's argument checks
def test_c_entry_rejects_other_flags_and_uncovered_plans(amd):
    from biem_helmholtz_sphere_amd import _biem, _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    plan = _biem._plan("ba", 4, dev)
    B, H, P = 1, 16, 3
    ops = dict(k=_cdev([K]), eta=_dev([ETA]), cen=_dev(np.zeros((1, 3))), rad=_dev([1.0]), kb=_cdev([2.1]), dl=_cdev([0.5]),
               dens=_cdev(np.ones((1, H))), pts=_dev(np.zeros((3, P))), out=torch.zeros((P, 1), dtype=torch.complex128, device="cuda"),
               work=torch.zeros(B * H * 16, dtype=torch.uint8, device="cuda"))
    p = {n: t.data_ptr() for n, t in ops.items()}

    def call(handle, flags):
        return lib.biem_uinterior(handle, 1, B, P, p["k"], p["eta"], p["cen"], p["rad"], 0, p["kb"], p["dl"], 0, p["dens"], p["pts"], flags,
                                  p["out"], p["work"], B * H * 16, None)
    assert lib.biem_uinterior_workspace_bytes(plan.handle, 1, B) == B * H * 16
    for flags in (L.USCAT_FAR_FIELD, L.USCAT_PER_BALL, L.USCAT_KIND_INNER, L.USCAT_PER_BALL | L.USCAT_POINTS_BATCHED, 16):
        assert call(plan.handle, flags) == 1 and b"BIEM_USCAT_POINTS_BATCHED" in lib.biem_last_error()      # BIEM_ERR_ARG
    assert call(plan.handle, 0) == L.BIEM_OK
    torch.cuda.synchronize()
    assert np.isfinite(ops["out"].cpu().numpy()).all()                                  # (three times the centre of the ball)
    chain = _biem._plan("bbba", 2, dev)
    assert call(chain.handle, 0) == L.BIEM_ERR_UNSUPPORTED and b"chain" in lib.biem_last_error()
    wide = _biem._plan("a", 200, dev)                                                   # below the order ceiling, above the LDS of 64 rows
    assert call(wide.handle, 0) == L.BIEM_ERR_UNSUPPORTED and b"LDS" in lib.biem_last_error()
