"""Standard chain trees "b" * (d - 2) + "a" on the GPU: the chain path on ba / bba against the default path and the goldens, and
d >= 5 against the oracle's quadrature form with a registered test-local chain tree (no reference fixture exists beyond d = 4; the
top orders of d = 5 .. 10 against the closed-form yardstick are in test_gpu_chain_full.py)."""
import math

import numpy as np
import pytest
import scipy.special as sp
import torch

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _biem, _lib
from oracle import biem_oracle as O

from test_chain_trees_host import chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.as_tensor(np.asarray(a), device=DEV)


def _centers(d, B, pitch=3.0):
    c = np.zeros((B, d))
    for b in range(B):
        c[b, b % d] = pitch * (b // d + 1) * (1 if b % 2 == 0 else -1)
        c[b, (b + 1) % d] += 0.3 * b
    return c


def _solve(bt, d, n_end, k, cen, rad, uin_np=None, **kw):
    c = amd.create_from_branching_types(bt)
    if uin_np is None:
        uin, ugr = amd.plane_wave(k=t(k), direction=t(np.arange(1.0, d + 1.0)))
    else:
        uin, ugr = uin_np
    return amd.biem(c, centers=t(cen), radii=t(rad), k=t(k), n_end=n_end, uin=uin, uin_grad=ugr, eta=t(1.0), **kw)


def _far_points(d, P=5, R=9.0):
    x = np.random.default_rng(d).normal(size=(P, d))
    return R * x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.fixture
def chain_switch(monkeypatch):
    monkeypatch.setenv("BIEM_TREE_CHAIN", "1")
    yield
    monkeypatch.delenv("BIEM_TREE_CHAIN")


@pytest.mark.parametrize("bt,d", [("ba", 3), ("bba", 4)])
def test_chain_path_on_ba_bba_matches_default(bt, d, monkeypatch):
    cen = _centers(d, 3)
    rad = np.array([1.0, 0.8, 0.6])
    x = _far_points(d).T
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("BIEM_TREE_CHAIN", flag)
        calc = _solve(bt, d, 6, 1.3, cen, rad)
        res[flag] = (calc.density.cpu().numpy(), calc.uscat(t(x)).cpu().numpy(), calc.uscat(t(x), far_field=True).cpu().numpy(),
                     calc.uscat(t(x), per_ball=True).cpu().numpy())
        cin = _solve(bt, d, 6, 1.3, cen[:1], rad[:1], kind="inner")            # (inner: a point outside any ball is NaN)
        xin = (cen[0] + 0.5 * _far_points(d, 4, 1.0)).T
        res[flag] += (cin.uscat(t(xin)).cpu().numpy(), cin.uscat(t(cen[0][:, None])).cpu().numpy())
    assert _biem._chain_plan_dim(bt) == d
    for a, b in zip(res["0"], res["1"]):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), (bt, np.abs(a - b).max(), np.abs(a).max())


def test_chain_path_golden_ba(chain_switch):
    """The smoke()/README case (reference golden accuracy_k_ba.csv:52) through the chain path."""
    cen = np.array([[0.0, 2.0, 0.0], [0.0, -2.0, 0.0]])
    c = amd.create_from_branching_types("ba")
    uin, ugr = amd.plane_wave(k=t(1.0), direction=t([1.0, 0.0, 0.0]))
    calc = amd.biem(c, uin=uin, uin_grad=ugr, k=t(1.0), n_end=6, eta=t(1.0), centers=t(cen), radii=t(np.ones(2)))
    u = complex(calc.uscat(torch.zeros(3, dtype=torch.float64, device=DEV)).cpu())
    assert abs(u - (-0.74133301331334 - 0.6696574197988229j)) < 1e-11


CASES = [
    dict(name="soft", k=1.1),
    dict(name="robin", k=0.9, alpha=1.0 + 0.5j, beta=0.3 - 0.2j),
    dict(name="complex_k", k=1.2 + 0.1j),
    dict(name="point_source", k=1.0),
]


@pytest.mark.parametrize("d,n_end", [(5, 4), (6, 3), (7, 3)])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_chain_vs_oracle(d, n_end, case, monkeypatch):
    ch = chain(d)
    bt = ch.name
    monkeypatch.setitem(O._TREES, bt, ch)
    O._sr_tables.cache_clear()
    cen = _centers(d, 2, pitch=2.6)
    rad = np.array([1.0, 0.7])
    k = case["k"]
    alpha, beta = case.get("alpha", 1.0), case.get("beta", 0.0)
    src = np.full(d, 0.2)
    if case["name"] == "point_source":
        uin = amd.point_source(k=t(k), source=t(src), n=0)
        uo_in, uo_gr = O.point_source(k, src, 0)
    else:
        direc = np.arange(1.0, d + 1.0)
        uin = amd.plane_wave(k=t(k), direction=t(direc))
        uo_in, uo_gr = O.plane_wave(k, direc)
    c = amd.create_from_branching_types(bt)
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(k), n_end=n_end, uin=uin[0], uin_grad=uin[1], eta=t(1.0),
                    alpha=alpha, beta=beta)
    res = O.solve_biem(bt, centers=cen, radii=rad, k=k, n_end=n_end, alpha=alpha, beta=beta, uin=uo_in, uin_grad=uo_gr,
                       sr_func=O.translation_SR_quadrature)
    dens = calc.density.cpu().numpy()
    assert np.abs(dens - res.density).max() <= 1e-10 * np.abs(res.density).max()
    x = _far_points(d)
    for kw in (dict(), dict(far_field=True), dict(per_ball=True)):
        u = calc.uscat(t(x.T), **kw).cpu().numpy()
        uo = O.uscat(res, x, **kw)
        assert np.abs(u - uo).max() <= 1e-10 * np.abs(uo).max(), (kw, np.abs(u - uo).max())
    O._sr_tables.cache_clear()


def test_chain_batched_k_eta_and_inner():
    d, n_end = 5, 4
    bt = "bbba"
    c = amd.create_from_branching_types(bt)
    cen = _centers(d, 2, pitch=2.6)
    rad = np.array([1.0, 0.7])
    ks = np.array([0.7, 1.1, 1.6])
    etas = np.array([1.0, 2.0, 0.5])
    uin, ugr = amd.plane_wave(k=t(ks), direction=t(np.tile(np.arange(1.0, d + 1.0)[:, None], (1, 3))))
    calc = amd.biem(c, centers=t(cen)[None], radii=t(rad)[None], k=t(ks), n_end=n_end, uin=uin, uin_grad=ugr, eta=t(etas))
    x = _far_points(d, 3)
    ub = calc.uscat(t(x.T)).cpu().numpy()                              # (P, 3)
    for i, k in enumerate(ks):
        one = _solve(bt, d, n_end, float(k), cen, rad)
        assert np.abs(ub[..., i] - one.uscat(t(x.T)).cpu().numpy()).max() <= 1e-12 * np.abs(ub).max()
    # kind inner: finite inside the ball, centre included, NaN outside
    cin = _solve(bt, d, n_end, 1.1, cen[:1], rad[:1], kind="inner")
    xin = cen[0][:, None] + np.concatenate([np.zeros((d, 1)), 0.5 * _far_points(d, 3, 1.0).T], axis=1)
    u = cin.uscat(t(xin)).cpu().numpy()
    assert np.isfinite(u).all()
    assert np.isnan(cin.uscat(t(x.T)).cpu().numpy()).all()


def _soft_residual(n_end):
    d, bt = 5, "bbba"
    cen = np.array([[0.0, 1.6, 0.0, 0.0, 0.0], [0.0, -1.6, 0.0, 0.0, 0.0]])
    rad = np.ones(2)
    k = 1.0
    calc = _solve(bt, d, n_end, k, cen, rad)
    y = _far_points(d, 16, 1.0)
    x = (cen[0][None, :] + (1.0 + 1e-10) * y).T                             # on the sphere (the outer field's domain)
    uin, _ = amd.plane_wave(k=t(k), direction=t(np.arange(1.0, d + 1.0)))
    tot = uin(t(x)) + calc.uscat(t(x))
    return float(tot.abs().max().cpu())


def test_chain_d5_residual_falls_with_order():
    res = [_soft_residual(n) for n in (4, 6, 8)]
    print("d = 5 sound-soft boundary residual, n_end 4 / 6 / 8:", res)
    assert res[1] < res[0] and res[2] < res[1]
    assert res[2] < 5e-5                     # measured 1.1e-5 (DESIGN.md "Chain trees")


def test_chain_d5_factorize_and_lu():
    d, bt, n_end = 5, "bbba", 6
    c = amd.create_from_branching_types(bt)
    cen = _centers(d, 3, pitch=2.8)
    rad = np.array([1.0, 0.8, 0.6])
    uin, ugr = amd.plane_wave(k=t(1.2), direction=t(np.arange(1.0, d + 1.0)))
    direct = amd.biem(c, centers=t(cen), radii=t(rad), k=t(1.2), n_end=n_end, uin=uin, uin_grad=ugr, eta=t(1.0))
    fac = amd.biem_factorize(c, centers=t(cen), radii=t(rad), k=t(1.2), n_end=n_end, eta=t(1.0))
    solved = fac.solve(uin=uin, uin_grad=ugr)
    a, b = direct.density.cpu().numpy(), solved.density.cpu().numpy()
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    import os
    os.environ["BIEM_SOLVER"] = "lu"
    try:
        lu = amd.biem(c, centers=t(cen), radii=t(rad), k=t(1.2), n_end=n_end, uin=uin, uin_grad=ugr, eta=t(1.0))
    finally:
        del os.environ["BIEM_SOLVER"]
    assert np.abs(lu.density.cpu().numpy() - a).max() <= 1e-11 * np.abs(a).max()


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_radial_any_dimension(d):
    lib = _lib.load()
    nmax = 12
    xs = np.array([0.3, 1.0, 4.5, 17.0])
    x = torch.tensor(xs, dtype=torch.float64, device=DEV)
    out = torch.zeros(len(xs), 2, nmax + 1, dtype=torch.float64, device=DEV)
    _lib.check(lib.biem_radial(d, nmax, len(xs), x.data_ptr(), out.data_ptr(), None))
    z = torch.tensor(np.array([0.8 + 0.3j, 3.0 - 0.2j, 6.0 + 0.0j]), device=DEV)
    outc = torch.zeros(len(z), 2, nmax + 1, dtype=torch.complex128, device=DEV)
    _lib.check(lib.biem_radial_complex(d, nmax, len(z), z.data_ptr(), outc.data_ptr(), None))
    torch.cuda.synchronize()
    out, outc = out.cpu().numpy(), outc.cpu().numpy()
    n = np.arange(nmax + 1)
    nu = n + d / 2 - 1
    for i, xv in enumerate(xs):
        pref = math.sqrt(math.pi / 2) / xv ** (d / 2 - 1)
        j, y = pref * sp.jv(nu, xv), pref * sp.yv(nu, xv)
        env = np.abs(j + 1j * y)
        assert np.max(np.abs(out[i, 0] - j) / env) < 1e-12 and np.max(np.abs(out[i, 1] - y) / env) < 1e-12, (d, xv)
    for i, zv in enumerate(z.cpu().numpy()):
        pref = math.sqrt(math.pi / 2) / zv ** (d / 2 - 1)
        j, h = pref * sp.jv(nu, zv), pref * sp.hankel1(nu, zv)
        assert np.max(np.abs(outc[i, 0] - j) / np.abs(j)) < 1e-12, (d, zv)
        assert np.max(np.abs(outc[i, 1] - h) / np.abs(h)) < 1e-12, (d, zv)
