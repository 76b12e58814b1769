"""The chain trees d = 5 .. 10 on the GPU at the largest orders their plans build in test time, against the closed-form yardstick.

Top orders used throughout: d = 5 / 6 / 7 / 8 / 9 / 10 at n_end 7 / 5 / 4 / 4 / 4 / 3.

References (nothing here compares one GPU kernel with another, except the pair-class and solver switches at the end):
* harmonics: `Chain.harmonics` (SciPy Gegenbauer polynomials), itself equal to the oracle's ba / bba (test_chain_trees_host.py);
* matrix entries and solved densities: `O.assemble` / `O.solve_biem` with the translation coefficients of tests/chain_yardstick.py,
  which applies no selection rule and is tied to the reference goldens on ba / bba (test_chain_yardstick_host.py);
* fields: the plain double sum  sum_b sum_h c_h z_n(k r) Y_h  from `O.radial_h` and `Chain.harmonics`, on densities that give EVERY
  degree a term of modulus in [0.5, 1.5] at a reference radius (the recipe of the full-order fixture: a solved density decays with the
  degree and hides the top ones below any tolerance).
Every test prints the largest error it measured (DESIGN.md 7b holds them).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _biem, _lib
from oracle import biem_oracle as O

import chain_yardstick as CY
from test_chain_trees_host import chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOP = {5: 7, 6: 5, 7: 4, 8: 4, 9: 4, 10: 3}
DIMS = sorted(TOP)


def t(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device=DEV, dtype=dtype)


def _name(d):
    return "b" * (d - 2) + "a"


@pytest.fixture
def registered(monkeypatch):
    """Chain trees in the oracle's registry for the duration of a test."""
    for d in DIMS:
        monkeypatch.setitem(O._TREES, _name(d), chain(d))
    O._sr_tables.cache_clear()
    yield
    O._sr_tables.cache_clear()


# ---------------------------------------------------------------------------- a. harmonics
def _special_directions(d, rng, scale=1.0):
    """+-e_j for every j; trailing coordinates zero from node j on, for every j (tail = 0 in chain_angles); one trailing part of 1e-9."""
    pts = [s * np.eye(d)[j] for j in range(d) for s in (1.0, -1.0)]
    for j in range(1, d):
        v = rng.normal(size=d)
        v[j:] = 0.0
        pts.append(v / np.linalg.norm(v))
    v = rng.normal(size=d)
    v[2:] *= 1e-9 / np.linalg.norm(v[2:]) * np.linalg.norm(v[:2])
    pts.append(v / np.linalg.norm(v))
    return scale * np.array(pts)


@pytest.mark.parametrize("d", DIMS)
def test_harmonics_kernel_vs_chain(d):
    n_end = TOP[d]
    lib = _lib.load()
    plan = _biem._plan(_name(d), n_end, torch.device(DEV))
    ch = chain(d)
    rng = np.random.default_rng(d)
    u = _special_directions(d, rng)
    u = np.concatenate([u, rng.normal(size=(40 - len(u), d))])
    assert len(u) == 40
    H = ch.n_harm(n_end)
    Y = torch.zeros((len(u), H), dtype=torch.complex128, device=DEV)
    _lib.check(lib.biem_harmonics(plan.handle, len(u), t(u).contiguous().data_ptr(), Y.data_ptr(), None))
    torch.cuda.synchronize()
    want = ch.harmonics(u, n_end).T
    err = np.abs(Y.cpu().numpy() - want).max(axis=1)
    print(f"d {d} n_end {n_end}: max |Y - want| = {err.max():.2e}, max |Y| = {np.abs(want).max():.2e} (worst point {int(err.argmax())})")
    assert err.max() <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------------------- b. general fill, entrywise
def _fill_geometry(d):
    """Ball 1 lies along e_0 from ball 0 and ball 2 along e_{d-1} (both differences exact in fp64, so the zero coordinates of the
    displacement are exact zeros); that puts ball 2 - ball 1 in the plane of e_0 and e_{d-1}, so a fourth ball supplies the generic
    displacements (three balls cannot hold two axis pairs and a generic one).  Generic means no polar angle at a zero of a node
    polynomial: components in arithmetic progression put cos^2 t_3 = 0.49 / 2.94 = 1 / 6 at d = 7, the zero of Gbar_2^{(2)}, and the
    entries that hold that harmonic alone were rounding noise on both sides."""
    o = 0.25 * np.arange(1, d + 1)
    v = np.where(np.arange(d) % 2 == 0, -1.0, 1.0) * 0.45 * np.exp(0.17 * np.arange(d))
    cen = np.array([o, o + 2.5 * np.eye(d)[0], o + 2.75 * np.eye(d)[d - 1], o + 3.0 * v / np.linalg.norm(v)])
    assert (np.count_nonzero(cen[1] - cen[0]), np.count_nonzero(cen[2] - cen[0]), np.count_nonzero(cen[3] - cen[1])) == (1, 1, d)
    return cen, np.array([1.0, 0.8, 0.6, 0.7])


FILL = [(5, 4, True), (7, 4, True), (10, 3, True), (5, 7, False), (6, 5, False), (8, 4, False), (9, 4, False)]


@pytest.mark.parametrize("d,n_end,full", FILL)
def test_fill_reference_scaling_vs_yardstick(d, n_end, full, registered):
    """`calc.matrix` (k_pair_tables_chain + the list fill, reference scaling) entry by entry; the numbers of
    test_fill_reference_scaling_vs_oracle.  Full matrix where H <= 112; elsewhere the whole diagonal blocks and, in every off-diagonal
    block, 300 random entries plus the corners."""
    ch = chain(d)
    H = ch.n_harm(n_end)
    assert (H <= 112) == full
    cen, rad = _fill_geometry(d)
    B = len(rad)
    ks = np.array([0.9, 2.3 + 0.2j])
    eta = np.array([1.0, 0.6])
    alpha, beta = 1.0 + 0.25j, 0.4 - 0.1j
    c = amd.create_from_branching_types(ch.name)
    calc = amd.biem(c, centers=t(cen)[None].expand(2, B, d), radii=t(rad)[None].expand(2, B), k=t(ks), eta=t(eta), n_end=n_end,
                    alpha=alpha, beta=beta)
    M = calc.matrix.cpu().numpy()
    assert M.shape == (2, B, H, B, H)
    rng = np.random.default_rng(10 * d + n_end)
    nblocks = B * (B - 1)
    corners = np.array([(0, 0), (H - 1, H - 1), (0, H - 1), (H - 1, 0)])
    samples = [np.concatenate([corners, np.stack(np.divmod(rng.choice(H * H, size=300, replace=False), H), axis=1)]) for _ in range(nblocks)]
    worst = 0.0
    for s in range(2):
        k = ks[s] if ks[s].imag != 0 else float(ks[s].real)
        sr = CY.sr_func if full else CY.sampled_sr_func(lambda i: samples[i % nblocks])
        A, _ = O.assemble(ch, n_end, k, eta[s], cen, rad, np.full(B, alpha), np.full(B, beta), sr_func=sr)
        have = ~np.isnan(A)
        for b in range(B):
            for bp in range(B):
                assert have[b, :, bp, :].sum() >= (H * H if full or b == bp else 300)
        nz = have & (np.abs(np.where(have, A, 0)) > 1e-200)
        err = np.abs(M[s][nz] - A[nz]) / np.abs(A[nz])
        worst = max(worst, err.max())
        zero = have & ~nz
        print(f"d {d} n_end {n_end} k {k}: {int(nz.sum())} entries, max relative error {err.max():.2e}; {int(zero.sum())} exact zeros")
        assert err.max() < 5e-11, (d, s, err.max())
        assert np.all(M[s][zero] == 0)
    print(f"d {d} n_end {n_end}: worst relative entry error {worst:.2e}")


# ---------------------------------------------------------------------------- d. field kernel with a visible density
def _z0(d):
    return math.sqrt(math.pi / 2) * 2.0 ** (1 - d / 2) / math.gamma(d / 2)


def _blc(d, n_end, k, eta, rho, inner):
    j, h, jp, hp = O.radial_h(n_end - 1, d, k * rho)
    if inner:
        j, jp = h, hp
    return 1j * k ** (d - 1) * rho ** (d - 1) * jp - 1j * eta * (1j * k ** (d - 2) * rho ** (d - 1) * j)


def _visible_density(ch, n_end, ks, etas, rad, mode, rng):
    """density[s, b, h]: every term has modulus in [0.5, 1.5] at r = 1.2 rho (outer), 0.8 rho (inner) or in the far field."""
    d, deg = ch.d, ch.degrees(n_end)
    H = len(deg)
    w = rng.uniform(0.5, 1.5, (len(rad), H)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (len(rad), H)))
    dens = np.zeros((len(ks), len(rad), H), dtype=np.complex128)
    for s, (k, eta) in enumerate(zip(ks, etas)):
        for b, rho in enumerate(rad):
            blc = _blc(d, n_end, k, eta, rho, mode == "inner")
            j, h, _, _ = O.radial_h(n_end - 1, d, k * rho * (0.8 if mode == "inner" else 1.2))
            z = {"outer": h, "inner": j, "far": np.ones(n_end)}[mode]
            dens[s, b] = w[b] / (np.abs(blc) * np.abs(z))[deg]
    return dens


def _field_ref(ch, n_end, k, eta, cen, rad, dens, x, mode):
    """Plain double sum, per ball: out[P, B] and the mask of points where the near series is not valid."""
    d, deg = ch.d, ch.degrees(n_end)
    out = np.zeros((len(x), len(rad)), dtype=np.complex128)
    bad = np.zeros(len(x), dtype=bool)
    for b, rho in enumerate(rad):
        rel = x - cen[b]
        r = np.linalg.norm(rel, axis=1)
        Y = ch.harmonics(rel, n_end)                                   # [H, P] (the angles do not depend on the length)
        cf = dens[b] * _blc(d, n_end, k, eta, rho, mode == "inner")[deg]
        if mode == "far":
            out[:, b] = ((cf * (-1j) ** deg) @ Y) * np.exp(-1j * k * (x @ cen[b])) / (1j * k) ** ((d - 1) / 2.0)
            continue
        z = np.zeros((n_end, len(x)), dtype=np.complex128)
        for p, rp in enumerate(r):
            if rp == 0.0:
                z[0, p] = _z0(d) if mode == "inner" else np.nan
                continue
            j, h, _, _ = O.radial_h(n_end - 1, d, k * rp)
            z[:, p] = j if mode == "inner" else h
        out[:, b] = np.sum(cf[:, None] * z[deg] * Y, axis=0)
        bad |= (r > rho) if mode == "inner" else (r < rho)
    return out, bad


def _centers5(d):
    cen = np.zeros((5, d))
    for b in range(5):
        cen[b, b % d] = 3.2
        cen[b, (b + 2) % d] += 0.3 * (b + 1)
    cen[0] = 0.1 * np.arange(d)
    return cen


def _check_field(what, got, want, bad, worst):
    """|got - want| <= 1e-10 max |want| at every point (per system and, per ball, per ball); the NaN mask is exactly the reference's."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(got.real) | np.isnan(got.imag)
    assert np.array_equal(nan, np.broadcast_to(bad.reshape(bad.shape + (1,) * (got.ndim - 1)), got.shape)), (what, np.nonzero(nan))
    scale = np.abs(want[~bad]).max(axis=0)
    err = (np.abs(got[~bad] - want[~bad]) / scale).max()
    worst.append(err)
    print(f"  {what}: max |got - want| / max |want| = {err:.2e} over {int((~bad).sum())} points")
    assert err <= 1e-10, (what, err)


@pytest.mark.parametrize("d", DIMS)
def test_field_kernel_with_visible_density(d):
    """k_uscat_chain at the top order: B = 5 (a second trip of the four-wave ball loop with three idle waves) and B = 1; near field,
    per ball, far field, batched points, kind inner with the centre of the ball; three wavenumbers, one complex."""
    n_end = TOP[d]
    ch = chain(d)
    c = amd.create_from_branching_types(ch.name)
    rng = np.random.default_rng(50 + d)
    ks = np.array([1.1, 2.0, 1.4 + 0.3j])
    kk = [1.1, 2.0, 1.4 + 0.3j]
    etas = np.array([1.0, 0.7, 1.3])
    cen, rad = _centers5(d), np.array([1.0, 0.8, 0.6, 0.9, 0.7])
    worst = []

    def calc(cen_, rad_, dens, kind="outer"):
        return amd.BIEMResultCalculator(c=c, centers=t(cen_.T), radii=t(rad_), k=t(ks), n_end=n_end, eta=t(etas), kind=kind,
                                        density=t(dens, torch.complex128))

    def ref(cen_, rad_, dens, x, mode):
        per = [_field_ref(ch, n_end, kk[s], etas[s], cen_, rad_, dens[s], x, mode) for s in range(3)]
        return np.stack([p[0] for p in per], axis=1), per[0][1]                  # [P, 3, B], [P]

    # points: random ones in a shell, c_b +- 1.3 rho_b e_j for every j, zero trailing coordinates relative to a ball, one inside ball 2
    sp = _special_directions(d, rng)
    x = [cen[i % 5] + 1.3 * rad[i % 5] * u for i, u in enumerate(sp)]
    x += list(rng.normal(size=(12, d)) * 2.5)
    x = np.array(x + [cen[2] + 0.5 * rad[2] * np.eye(d)[1]])
    dens = _visible_density(ch, n_end, kk, etas, rad, "outer", rng)
    want, bad = ref(cen, rad, dens, x, "outer")
    assert bad[-1] and bad.sum() <= 4, np.nonzero(bad)          # (a few of the random points may fall into a ball: NaN there as well)
    cal = calc(cen, rad, dens)
    print(f"d {d} n_end {n_end}, 5 balls, {len(x)} points")
    _check_field("near", cal.uscat(t(x.T)).cpu().numpy(), want.sum(axis=2), bad, worst)
    _check_field("near, per ball", cal.uscat(t(x.T), per_ball=True).cpu().numpy(), want, bad, worst)
    xb = np.stack([x, x[::-1], np.roll(x, 3, axis=0)], axis=2)                     # [P, d, 3]: other points for every system
    wb = [ref(cen, rad, dens, xb[:, :, s], "outer") for s in range(3)]
    want_b = np.stack([wb[s][0][:, s].sum(axis=1) for s in range(3)], axis=1)
    got_b = cal.uscat(t(np.moveaxis(xb, 1, 0)), expand_x=False).cpu().numpy()
    for s in range(3):
        _check_field(f"near, batched points, system {s}", got_b[:, s], want_b[:, s], wb[s][1], worst)
    dens_far = _visible_density(ch, n_end, kk, etas, rad, "far", rng)
    want_far, _ = ref(cen, rad, dens_far, x, "far")
    none = np.zeros(len(x), dtype=bool)
    _check_field("far", calc(cen, rad, dens_far).uscat(t(x.T), far_field=True).cpu().numpy(), want_far.sum(axis=2), none, worst)
    _check_field("far, per ball", calc(cen, rad, dens_far).uscat(t(x.T), far_field=True, per_ball=True).cpu().numpy(), want_far, none, worst)
    # one ball
    x1 = np.array([cen[1] + 1.3 * rad[1] * u for u in sp] + [cen[1] + 0.3 * rad[1] * np.eye(d)[0]])
    want, bad = ref(cen[1:2], rad[1:2], dens[:, 1:2], x1, "outer")
    assert bad[-1] and bad.sum() == 1
    _check_field("one ball, near", calc(cen[1:2], rad[1:2], dens[:, 1:2]).uscat(t(x1.T)).cpu().numpy(), want.sum(axis=2), bad, worst)
    want, _ = ref(cen[1:2], rad[1:2], dens_far[:, 1:2], x1, "far")
    _check_field("one ball, far", calc(cen[1:2], rad[1:2], dens_far[:, 1:2]).uscat(t(x1.T), far_field=True).cpu().numpy(),
                 want.sum(axis=2), np.zeros(len(x1), dtype=bool), worst)
    # kind inner: inside the ball, its centre included; one point outside
    dens_in = _visible_density(ch, n_end, kk, etas, rad[3:4], "inner", rng)
    xi = np.array([cen[3]] + [cen[3] + 0.8 * rad[3] * u for u in sp] + [cen[3] + 0.4 * rad[3] * u for u in sp[::3]] + [cen[3] + 1.2 * rad[3] * sp[-1]])
    want, bad = ref(cen[3:4], rad[3:4], dens_in, xi, "inner")
    assert bad[-1] and bad.sum() == 1
    cin = calc(cen[3:4], rad[3:4], dens_in, kind="inner")
    _check_field("inner", cin.uscat(t(xi.T)).cpu().numpy(), want.sum(axis=2), bad, worst)
    _check_field("inner, per ball", cin.uscat(t(xi.T), per_ball=True).cpu().numpy(), want, bad, worst)
    print(f"d {d} n_end {n_end}: worst field error {max(worst):.2e} of max |u|")


# ---------------------------------------------------------------------------- e. end to end at d = 8, 9, 10
CASES = [
    dict(name="soft", k=1.1),
    dict(name="robin", k=0.9, alpha=1.0 + 0.5j, beta=0.3 - 0.2j),
    dict(name="complex_k", k=1.2 + 0.1j),
    dict(name="point_source", k=1.0),
]


def _far_points(d, P=5, R=9.0):
    x = np.random.default_rng(d).normal(size=(P, d))
    return R * x / np.linalg.norm(x, axis=1, keepdims=True)


def _incident(case, d):
    k = case["k"]
    if case["name"] == "point_source":
        src = np.full(d, 0.2)
        return amd.point_source(k=t(k), source=t(src), n=0), O.point_source(k, src, 0)
    direc = np.arange(1.0, d + 1.0)
    return amd.plane_wave(k=t(k), direction=t(direc)), O.plane_wave(k, direc)


@pytest.mark.parametrize("d", [8, 9, 10])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_chain_solve_vs_yardstick_oracle(d, case, registered):
    """The cases and bounds of test_chain_vs_oracle at d = 8, 9, 10, n_end 3, two balls (N = 88 / 110: the one-launch solve;
    N = 130 at d = 10: the blocked one)."""
    n_end, bt = 3, _name(d)
    cen = np.zeros((2, d))
    cen[0, 0], cen[0, 1], cen[1, 1], cen[1, 2] = 2.6, 0.0, -2.6, 0.3
    rad = np.array([1.0, 0.7])
    k, alpha, beta = case["k"], case.get("alpha", 1.0), case.get("beta", 0.0)
    uin, (uo_in, uo_gr) = _incident(case, d)
    c = amd.create_from_branching_types(bt)
    calc = amd.biem(c, centers=t(cen), radii=t(rad), k=t(k), n_end=n_end, uin=uin[0], uin_grad=uin[1], eta=t(1.0), alpha=alpha, beta=beta)
    res = O.solve_biem(bt, centers=cen, radii=rad, k=k, n_end=n_end, alpha=alpha, beta=beta, uin=uo_in, uin_grad=uo_gr, sr_func=CY.sr_func)
    err = np.abs(calc.density.cpu().numpy() - res.density).max() / np.abs(res.density).max()
    print(f"d {d} {case['name']}: density {err:.2e} of max")
    assert err <= 1e-10
    x = _far_points(d)
    for kw in (dict(), dict(far_field=True), dict(per_ball=True)):
        u = calc.uscat(t(x.T), **kw).cpu().numpy()
        uo = O.uscat(res, x, **kw)
        e = np.abs(u - uo).max() / np.abs(uo).max()
        print(f"  uscat {kw}: {e:.2e} of max")
        assert e <= 1e-10, (kw, e)


def test_d8_grid_batch_pair_classes_and_lu(registered, monkeypatch):
    """d = 8, n_end 3, four equal spheres on a 2 x 2 grid (N = 176: the blocked solve), 8 wavenumbers on one geometry: the repeated
    displacements engage the pair classes at the default threshold.  Against the yardstick oracle at two of the wavenumbers, against
    the same call without pair classes at all of them, and once more through the pivoted LU."""
    d, n_end, bt = 8, 3, _name(8)
    cen = np.zeros((4, d))
    cen[:, 0], cen[:, 1] = [-1.5, -1.5, 1.5, 1.5], [-1.5, 1.5, -1.5, 1.5]
    rad = np.ones(4)
    ks = np.array([0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0])
    direc = np.arange(1.0, d + 1.0)
    c = amd.create_from_branching_types(bt)
    uin, ugr = amd.plane_wave(k=t(ks), direction=t(np.tile(direc[:, None], (1, len(ks)))))

    def solve():
        calc = amd.biem(c, centers=t(cen)[None], radii=t(rad)[None], k=t(ks), n_end=n_end, uin=uin, uin_grad=ugr, eta=t(np.ones(len(ks))))
        return calc.density.cpu().numpy()

    monkeypatch.delenv("BIEM_FILL_NO_DEDUPE", raising=False)
    monkeypatch.delenv("BIEM_FILL_DEDUPE_MIN", raising=False)
    monkeypatch.delenv("BIEM_SOLVER", raising=False)
    dens = solve()
    assert dens.shape == (len(ks), 4, 44)
    for s in (1, 6):
        uo_in, uo_gr = O.plane_wave(float(ks[s]), direc)
        res = O.solve_biem(bt, centers=cen, radii=rad, k=float(ks[s]), n_end=n_end, uin=uo_in, uin_grad=uo_gr, sr_func=CY.sr_func)
        err = np.abs(dens[s] - res.density).max() / np.abs(res.density).max()
        print(f"k {ks[s]}: density {err:.2e} of max against the yardstick oracle")
        assert err <= 1e-10
    monkeypatch.setenv("BIEM_FILL_NO_DEDUPE", "1")
    plain = solve()
    monkeypatch.delenv("BIEM_FILL_NO_DEDUPE")
    err = max(np.abs(dens[s] - plain[s]).max() / np.abs(plain[s]).max() for s in range(len(ks)))
    print(f"pair classes against none: {err:.2e} of max")
    assert err <= 1e-12
    monkeypatch.setenv("BIEM_SOLVER", "lu")
    lu = solve()
    monkeypatch.delenv("BIEM_SOLVER")
    err = max(np.abs(lu[s] - plain[s]).max() / np.abs(plain[s]).max() for s in range(len(ks)))
    print(f"pivoted LU against the symmetric path: {err:.2e} of max")
    assert err <= 1e-12
