"""uscat_grad() on the GPU: the Cartesian gradient of the scattered field.

The yardstick is not a NumPy twin of the kernel's formulas but the oracle's own field (``oracle.biem_oracle.uscat``, pinned on the
reference's goldens), differentiated by the 8th-order central difference
    f' ~ [4/5 (f1 - f-1) - 1/5 (f2 - f-2) + 4/105 (f3 - f-3) - 1/280 (f4 - f-4)] / h.
Every stencil test computes it with h = 1e-2 and h = 5e-3 and first asserts that the two agree within 1e-11 of max |grad u| over
the case (measured on the CPU at <= 1.8e-12 on cases of this kind; h = 2.5e-3 is already rounding-limited at 5e-12): that guards
the yardstick.  Then |GPU - stencil(5e-3)| <= 1e-10 max |grad u|, the project's parity contract.
The Neumann boundary identity needs no differencing and reaches the surface itself.  Chain trees (d >= 5) and orders above the
per-lane ceilings are not built: the error is pinned.
"""
import types

import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd
from oracle import biem_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_END = {"a": 8, "ba": 6, "bpa": 6, "bba": 5, "bpbpa": 5, "caa": 5}
DIM = {"a": 2, "ba": 3, "bpa": 3, "bba": 4, "bpbpa": 4, "caa": 4}
ROOT_AXIS = {"a": 0, "ba": 0, "bba": 0, "caa": 0, "bpa": 2, "bpbpa": 3}      # canonical axis 0 in the caller's axes
C8 = (4.0 / 5.0, -1.0 / 5.0, 4.0 / 105.0, -1.0 / 280.0)
STENCIL_TOL, PARITY_TOL = 1e-11, 1e-10


def t(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device=DEV, dtype=dtype)


def _geometry(d):
    """Two balls of different radii, off every axis and not symmetric under any axis permutation."""
    cen = np.array([[1.7, 0.9, -0.6, 0.5], [-1.4, -1.1, 0.8, -0.7]])[:, :d]
    return cen, np.array([1.0, 0.7])


def _direction(d):
    v = np.array([0.9, -0.5, 0.7, 0.3])[:d]
    return v / np.linalg.norm(v)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _points(bt, cen, rad):
    """[P, d]: a far generic point, the origin, points whose offset from a centre lies on the tree's axes, one near a surface."""
    d = DIM[bt]
    e = np.eye(d)
    gen = _unit(np.array([0.3, -0.8, 0.45, 0.6])[:d])
    pts = [3.5 * gen, np.zeros(d)]
    pts.append(cen[1] + 1.2 * rad[1] * e[ROOT_AXIS[bt]])                 # on the root axis of ball 1 (offset parallel to it)
    pts.append(cen[0] - 1.3 * rad[0] * e[ROOT_AXIS[bt]])                 # ... and of ball 0, the other pole
    pts.append(cen[1] + 1.2 * rad[1] * e[0])                             # offset along x0 in the caller's axes (the same for a, ba, bba, caa)
    if d == 4:
        # only the last two offsets zero (bba: sin t1 = 0; caa: t0 = 0), only the first two zero (caa: t0 = pi / 2), in both axis orders
        pts.append(cen[0] + 1.25 * rad[0] * _unit([0.6, -0.8, 0.0, 0.0]))
        pts.append(cen[1] + 1.25 * rad[1] * _unit([0.0, 0.0, 0.7, 0.5]))
        pts.append(cen[0] + 1.25 * rad[0] * _unit([0.0, 0.6, -0.8, 0.0]))
        pts.append(cen[1] + 1.25 * rad[1] * _unit([0.7, 0.0, 0.0, -0.5]))
    pts.append(cen[0] + 1.05 * rad[0] * _unit(np.array([-0.5, 0.4, 0.6, -0.3])[:d]))   # near the surface of the unit ball: the h = 1e-2 stencil (reach 0.04) stays outside
    return np.array(pts)


def _stencil(res, x, h):
    """8th-order central difference of the oracle's field at x[P, d] -> [d, P]."""
    P, d = x.shape
    g = np.zeros((d, P), dtype=np.complex128)
    for i in range(d):
        e = np.zeros(d)
        e[i] = h
        for q, cq in enumerate(C8, start=1):
            g[i] += cq * (O.uscat(res, x + q * e) - O.uscat(res, x - q * e))
    return g / h


def _yardstick(res, x):
    g1, g2 = _stencil(res, x, 1e-2), _stencil(res, x, 5e-3)
    scale = np.abs(g2).max()
    dev = np.abs(g1 - g2).max() / scale
    print(f"  stencils h=1e-2 / 5e-3 agree within {dev:.2e} of max|grad u| = {scale:.3e}")
    assert np.isfinite(g2).all()
    assert dev <= STENCIL_TOL, dev
    return g2, scale


def _solve_both(bt, cen, rad, k, alpha=1.0, beta=0.0, kind="outer"):
    d, n_end = DIM[bt], N_END[bt]
    dirn = _direction(d)
    uo, go = O.plane_wave(k, dirn)
    res = O.solve_biem(bt, centers=cen, radii=rad, k=k, n_end=n_end, eta=1.0, alpha=alpha, beta=beta, uin=uo, uin_grad=go, kind=kind)
    kt = t(k)
    uin, ugr = amd.plane_wave(k=kt, direction=t(dirn))
    B = len(rad)
    calc = amd.biem(amd.create_from_branching_types(bt), centers=t(cen), radii=t(rad), k=kt, n_end=n_end, eta=t(1.0), uin=uin, uin_grad=ugr,
                    alpha=t(np.full(B, alpha)), beta=t(np.full(B, beta)), kind=kind)
    return res, calc


CASES = [(bt, 1.3, 1.0, 0.0) for bt in ("a", "ba", "bpa", "bba", "bpbpa", "caa")] + [
    ("ba", 1.3, 1.0 + 0.5j, 0.3 - 0.2j),          # complex alpha / beta (Robin)
    ("bpa", 1.1, 0.4j, 1.0),
    ("a", 1.3 + 0.2j, 1.0, 0.0),                  # complex k
    ("bpbpa", 1.2 + 0.15j, 1.0, 0.0),
]


@pytest.mark.parametrize("bt,k,alpha,beta", CASES, ids=[f"{c[0]}-k{c[1]}-a{c[2]}-b{c[3]}" for c in CASES])
def test_gradient_against_oracle_stencil(bt, k, alpha, beta):
    cen, rad = _geometry(DIM[bt])
    res, calc = _solve_both(bt, cen, rad, k, alpha, beta)
    x = _points(bt, cen, rad)
    want, scale = _yardstick(res, x)
    got = calc.uscat_grad(t(x.T)).cpu().numpy()
    assert got.shape == (DIM[bt], len(x))
    err = np.abs(got - want).max() / scale
    print(f"  {bt}: |GPU - stencil| = {err:.2e} of max|grad u|; per point {np.abs(got - want).max(0) / scale}")
    assert np.isfinite(got).all(), got
    assert err <= PARITY_TOL, err


@pytest.mark.parametrize("bt", ["bpa", "bpbpa"])
def test_components_are_in_the_callers_axes(bt):
    """The yardstick itself tells canonical order from the caller's: the stencil's components, permuted the way the canonical tree
    sees them, are far from the stencil (so the parity test above fails for a result left in canonical order)."""
    from biem_helmholtz_sphere_amd._coords import CANONICAL

    cen, rad = _geometry(DIM[bt])
    res, calc = _solve_both(bt, cen, rad, 1.3)
    x = _points(bt, cen, rad)
    want, scale = _yardstick(res, x)
    got = calc.uscat_grad(t(x.T)).cpu().numpy()
    perm = list(CANONICAL[bt][1])
    assert np.abs(want[perm] - want).max() > 1e-2 * scale
    assert np.abs(got[perm] - want).max() > 1e-2 * scale
    assert np.abs(got - want).max() <= PARITY_TOL * scale


@pytest.mark.parametrize("bt", ["a", "ba", "bpa", "bba", "caa"])
def test_neumann_boundary_identity_single_ball(bt):
    """alpha = 0, beta = 1, one ball: d_n u_scat(c + rho y) = sum_h f_h Y_h(y) exactly in the retained harmonics (f: the oracle's
    right-hand side); evaluated ON the surface (the factor 1 + 1e-13 keeps rounding from masking the point), poles included."""
    d, n_end = DIM[bt], N_END[bt]
    cen, rad = np.array([[0.4, -0.3, 0.2, 0.1]])[:, :d], np.array([1.3])
    res, calc = _solve_both(bt, cen, rad, 1.3, alpha=0.0, beta=1.0)
    rng = np.random.default_rng(7)
    y = rng.normal(size=(6, d))
    e = np.eye(d)
    y = np.concatenate([y, e, -e[:1]])
    if d == 4:
        y = np.concatenate([y, [[0.6, 0.8, 0, 0], [0, 0, -0.6, 0.8], [0, 0.6, 0.8, 0]]])
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    want = res.rhs[0] @ res.tree.harmonics(y, n_end)
    x = cen[0] + rad[0] * (1.0 + 1e-13) * y
    g = calc.uscat_grad(t(x.T)).cpu().numpy()
    got = np.sum(y.T * g, axis=0)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"  {bt}: |d_n u_scat - f.Y| = {err:.2e} of max|f.Y|")
    assert np.isfinite(g).all()
    assert err <= 1e-10, err


@pytest.mark.parametrize("bt", ["a", "ba", "bpbpa", "caa"])
def test_per_ball_sums_and_mask(bt):
    d = DIM[bt]
    cen, rad = _geometry(d)
    _, calc = _solve_both(bt, cen, rad, 1.3)
    x = np.concatenate([_points(bt, cen, rad), [cen[0] + 0.5 * rad[0] * _unit(np.ones(d)), cen[1]]])   # the last two are inside a ball
    g = calc.uscat_grad(t(x.T)).cpu().numpy()
    pb = calc.uscat_grad(t(x.T), per_ball=True).cpu().numpy()
    assert pb.shape == (d, len(x), 2)
    ok = slice(0, len(x) - 2)
    assert np.abs(pb[:, ok].sum(-1) - g[:, ok]).max() <= 1e-13 * np.abs(g[:, ok]).max()
    assert np.isfinite(g[:, ok]).all() and np.isnan(g[:, -2:]).all()
    assert np.isnan(pb[:, -2:]).all()                                     # every ball, every component
    assert np.isnan(calc.uscat(t(x.T), per_ball=True).cpu().numpy()[-2:]).all()


@pytest.mark.parametrize("kind", ["outer", "inner"])
@pytest.mark.parametrize("bt", ["a", "ba", "caa"])
def test_mask_matches_uscat_on_a_grid(bt, kind):
    d = DIM[bt]
    if kind == "outer":
        cen, rad = _geometry(d)
    else:
        cen, rad = np.array([[0.3, -0.2, 0.1, 0.2]])[:, :d], np.array([2.0])
    _, calc = _solve_both(bt, cen, rad, 1.3, kind=kind)
    g = np.linspace(-3.0, 3.0, 25)
    X, Y = np.meshgrid(g, g, indexing="ij")
    x = np.stack([X, Y] + [0.1 * (i + 1) * np.ones_like(X) for i in range(d - 2)])
    x[:, 3, 4] = cen[0]                                                # a centre exactly
    u = calc.uscat(t(x)).cpu().numpy()
    gr = calc.uscat_grad(t(x)).cpu().numpy()
    assert gr.shape == (d,) + X.shape
    assert 0 < np.isnan(u).sum() < u.size
    for i in range(d):
        assert np.array_equal(np.isnan(gr[i]), np.isnan(u))
    assert np.isfinite(gr[:, ~np.isnan(u)]).all()


def test_batched_systems_expand_x_false_and_numpy_round_trip():
    bt, d, n_end = "ba", 3, 6
    cen, rad = _geometry(d)
    ks = np.array([0.9, 1.3, 1.7])
    cens = np.stack([cen, cen + 0.1])                                   # [2, B, d]: two geometries x three k
    dirs = np.broadcast_to(_direction(d)[:, None, None], (d, 2, 3)).copy()
    kk = np.broadcast_to(ks, (2, 3)).copy()
    uin, ugr = amd.plane_wave(k=t(kk), direction=t(dirs))
    c = amd.create_from_branching_types(bt)
    calc = amd.biem(c, centers=t(cens[:, None]), radii=t(rad[None, None]), k=t(kk), n_end=n_end, eta=t(np.ones((1, 1))), uin=uin, uin_grad=ugr)
    assert tuple(calc.density.shape[:2]) == (2, 3)
    xs = np.random.default_rng(3).normal(size=(d, 5, 2, 3)) * 0.2 + (3.5 * _unit([0.3, -0.8, 0.45]))[:, None, None, None]
    got = calc.uscat_grad(t(xs), expand_x=False).cpu().numpy()
    assert got.shape == (d, 5, 2, 3)
    shared = calc.uscat_grad(t(xs[:, :, 0, 0])).cpu().numpy()
    assert shared.shape == (d, 5, 2, 3)
    for i in range(2):
        for j in range(3):
            u1, g1 = amd.plane_wave(k=t(ks[j]), direction=t(_direction(d)))
            one = amd.biem(c, centers=t(cens[i]), radii=t(rad), k=t(ks[j]), n_end=n_end, eta=t(1.0), uin=u1, uin_grad=g1)
            ref = one.uscat_grad(t(xs[:, :, i, j])).cpu().numpy()
            assert np.abs(got[:, :, i, j] - ref).max() <= 1e-12 * np.abs(ref).max()
            ref0 = one.uscat_grad(t(xs[:, :, 0, 0])).cpu().numpy()
            assert np.abs(shared[:, :, i, j] - ref0).max() <= 1e-12 * np.abs(ref0).max()
    # NumPy in, NumPy out; complex64 density gives complex64
    un, gn = amd.plane_wave(k=np.array(1.3), direction=_direction(d))
    cn = amd.biem(c, centers=cen, radii=rad, k=np.array(1.3), n_end=n_end, eta=np.array(1.0), uin=un, uin_grad=gn)
    x = _points(bt, cen, rad).T
    out = cn.uscat_grad(x)
    assert isinstance(out, np.ndarray) and out.dtype == np.complex128 and out.shape == x.shape
    assert isinstance(amd.biem_u_grad(cn, x, per_ball=True), np.ndarray)
    low = types.SimpleNamespace(c=cn.c, centers=cn.centers, radii=cn.radii, k=cn.k, eta=cn.eta, kind=cn.kind, density=cn.density.astype(np.complex64))
    o32 = amd.biem_u_grad(low, x)
    assert o32.dtype == np.complex64 and np.abs(o32 - out).max() <= 1e-5 * np.abs(out).max()
    with pytest.raises(ValueError, match="x must have shape"):
        cn.uscat_grad(np.zeros((d + 1, 4)))


@pytest.mark.parametrize("bt", ["a", "ba", "bpa", "bba", "caa"])
def test_inner_kind_against_oracle_stencil(bt):
    """One ball, kind = "inner": points inside, the centre (only the degree-1 terms contribute) and the tree's axes included."""
    d = DIM[bt]
    cen, rad = np.array([[0.3, -0.2, 0.1, 0.2]])[:, :d], np.array([2.0])
    res, calc = _solve_both(bt, cen, rad, 1.3, kind="inner")
    e = np.eye(d)
    pts = [cen[0], cen[0] + 0.9 * e[ROOT_AXIS[bt]], cen[0] - 1.1 * e[0], cen[0] + 1.2 * _unit(np.array([0.3, -0.8, 0.45, 0.6])[:d]),
           cen[0] + 1.9 * _unit(np.array([-0.5, 0.4, 0.6, -0.3])[:d])]
    if d == 4:
        pts += [cen[0] + 0.8 * _unit([0.6, -0.8, 0.0, 0.0]), cen[0] + 0.8 * _unit([0.0, 0.0, 0.7, 0.5]), cen[0] + 0.8 * _unit([0.0, 0.6, -0.8, 0.0])]
    x = np.array(pts)
    want, scale = _yardstick(res, x)
    got = calc.uscat_grad(t(x.T)).cpu().numpy()
    err = np.abs(got - want).max() / scale
    print(f"  {bt} inner: |GPU - stencil| = {err:.2e} of max|grad u|; at the centre |grad u| = {np.abs(got[:, 0]).max():.3e}")
    assert np.isfinite(got).all()
    assert np.abs(got[:, 0]).max() > 1e-3 * scale                         # the centre is not a guarded zero
    assert err <= PARITY_TOL, err


def test_not_built_chain_trees_and_orders_above_the_per_lane_ceiling():
    c5 = amd.create_from_branching_types("bbba")
    uin, ugr = amd.plane_wave(k=t(1.1), direction=t(np.arange(1.0, 6.0)))
    calc = amd.biem(c5, centers=t(np.zeros((1, 5))), radii=t([1.0]), k=t(1.1), n_end=3, eta=t(1.0), uin=uin, uin_grad=ugr)
    x = t(np.full((5, 2), 1.5))
    assert torch.isfinite(calc.uscat(x).real).all()
    with pytest.raises(NotImplementedError, match=r"covered: a \(n_end <= 320\), ba \(n_end <= 48\), bba \(n_end <= 14\), caa \(n_end <= 12\)"):
        calc.uscat_grad(x)
    c4 = amd.create_from_branching_types("caa")
    uin, ugr = amd.plane_wave(k=t(1.1), direction=t(np.arange(1.0, 5.0)))
    calc = amd.biem(c4, centers=t(np.zeros((1, 4))), radii=t([1.0]), k=t(1.1), n_end=13, eta=t(1.0), uin=uin, uin_grad=ugr)
    x = t(np.full((4, 2), 1.5))
    assert torch.isfinite(calc.uscat(x).real).all()
    with pytest.raises(NotImplementedError, match="n_end=13"):
        calc.uscat_grad(x)
