"""The fixtures of tests/test_gpu_full_order_rhs.py, their 40-digit yardstick and their checker (no GPU).

* the caps the generator promises: ranges, condition of P_ext, file sizes, the ceilings;
* one entry per case and group recomputed in mpmath from the stored inputs;
* the inputs rebuilt from integers are exact dyadic numbers, and the generator reproduces the small cases array by array
  (``tools/make_full_order_rhs_fixtures.py --check`` does the same for every case);
* ``oracle/mp_rhs.py`` against the fp64 yardsticks at n_end <= 6 (tests/point_source_yardstick.py, plane_wave_yardstick.py,
  power_yardstick.py, the chain harmonics of tests/test_chain_trees_host.py, ``mp_field.harmonics`` at d = 3, 4): the agreement was
  measured (TIE_MEASURED) and is asserted at 4 x that, as tests/test_force_table_full_order_host.py does;
* planted faults: the checker of the GPU tests, fed the fixture's own expectations with one fault each, must refuse every one.
"""
import importlib.util
import os
import types

import mpmath as mp
import numpy as np
import pytest

from oracle import biem_oracle as O
from oracle import full_order_rhs_fixture as FX
from oracle import mp_field as MF
from oracle import mp_rhs as R

import plane_wave_yardstick as PW
import point_source_yardstick as PS
import power_yardstick as PY
from test_chain_trees_host import chain

CASES = FX.load()
MAIN = [c for c, r in CASES.items() if r.kind == "main"]
WIDE = [c for c, r in CASES.items() if r.kind == "wide"]
EDGE = "a-150-edge"
RANGE, EDGE_RANGE = (1e-280, 1e280), (1e-300, 1e300)
ROBIN = (1.0 + 0.5j, 0.3 - 0.2j)
# largest relative disagreement between oracle/mp_rhs.py and the fp64 yardsticks at n_end <= 6, measured with the cases of the tie
# tests below (relative to the largest modulus of the compared array); asserted at 4 x
TIE_MEASURED = {"point_source": 1.1e-15, "plane_wave": 7.1e-16, "power": 5.1e-16, "chain": 2.1e-15}


def mpv(v):
    return [mp.mpf(float(x)) for x in v]


def oracle_tree(tree):
    return O.tree(tree) if tree in FX.CANONICAL else chain(FX.tree_dim(tree))


# ---------------------------------------------------------------------------- caps
def test_file_sizes_and_ceilings():
    for p in FX.PATHS:
        assert os.path.getsize(p) < 500_000, p
    import biem_helmholtz_sphere_amd as amd

    top = dict(amd._biem.USCAT_GRAD_N_END_MAX)
    top.update(FX.CHAIN_CEILINGS)
    assert sorted((CASES[c].tree, CASES[c].n_end) for c in MAIN) == sorted(top.items())
    assert sorted((CASES[c].tree, CASES[c].n_end) for c in WIDE) == [("a", 320), ("ba", 48)]
    for c in MAIN:
        assert CASES[c].B == (2 if CASES[c].tree in FX.CANONICAL else 1) and CASES[c].nb == 2
        assert CASES[c].k[0].imag == 0.0 and 0.0 < CASES[c].k[1].imag


@pytest.mark.parametrize("cid", MAIN + WIDE + [EDGE])
def test_ranges(cid):
    """gj_n, the point-source and plane-wave scales inside [1e-280, 1e280]; the edge case alone leaves it (gj_149 = 4.4e-289 and
    |h_149| = 3.2e284 at 1.02 rho: normal fp64 numbers) and stays inside [1e-300, 1e300]."""
    rec = CASES[cid]
    lo, hi = EDGE_RANGE if cid == EDGE else RANGE
    src = CASES[rec.main] if rec.kind == "wide" else rec
    for what, v in (("gj", np.abs(src.gj)), ("scale", np.abs(rec.G) * rec.st.ynorm)):
        assert lo <= v.min() and v.max() <= hi, (cid, what, v.min(), v.max())
    if cid == EDGE:
        assert np.abs(rec.gj).min() < RANGE[0] and 4e-289 < np.abs(rec.gj).min() < 5e-289       # the documented edge
        h = np.abs(rec.G[0, 0, 0, -1] / (2.0 * np.pi * rec.gj[0, 0, -1]))                       # C_2 = 2 pi
        assert 3e284 < h < 4e284
    if rec.kind == "main":
        pw = np.abs(rec.pf)[..., None] * np.abs(rec.gj)[:, None] * rec.st.ynorm
        assert lo <= pw.min() and pw.max() <= hi
        dist = np.linalg.norm(rec.src[:, None] - rec.centers[None, :rec.B], axis=-1)
        assert (dist >= 1.01 * rec.radii[None, :rec.B]).all()
        own = dist[np.arange(5), np.arange(5) % rec.B] / rec.radii[np.arange(5) % rec.B]
        assert np.allclose(own, [1.02, 1.5, 4.0, 1.5, 1.02], rtol=1e-9)
        assert (rec.k.imag[:, None, None] * dist[None]).max() < 10.0                            # Im k |t| far below 690
        assert rec.radii[0] != rec.radii[1]


@pytest.mark.parametrize("cid", MAIN)
def test_power_caps(cid):
    rec = CASES[cid]
    for sfx in ("", "_n") if rec.tree in ("a", "ba") else ("",):
        want, scale, cond = (getattr(rec, n + sfx) for n in ("pwant", "pscale", "pcond"))
        assert cond.max() <= 100.0 and (scale[..., 0] >= np.abs(want[..., 0])).all()
        assert RANGE[0] <= scale[..., 0].min() and scale.max() <= RANGE[1]
        assert (want[:, 0, 1] > 0).all() and (want[:, 1, 1] == 0).all() and (scale[:, 1, 1] == 0).all()     # lossy, lossless
    assert (rec.palpha[0] * np.conj(rec.pbeta[0])).imag != 0.0 and (rec.palpha[1] * np.conj(rec.pbeta[1])).imag == 0.0
    assert rec.pexps[:, [1, 3]].min() >= 0 and rec.pexps[:, [1, 3]].max() <= 3


def test_one_case_reaches_the_plane_wave_weight_of_5000():
    kc = max((np.abs(CASES[c].k)[:, None] * np.linalg.norm(CASES[c].centers, axis=-1)[None]).max() for c in MAIN)
    assert 4000.0 <= kc <= 6500.0


# ---------------------------------------------------------------------------- one entry per case in mpmath
def _y(rec, vec, h):
    return R.tree_harmonics(rec.tree, rec.n_end, mpv(vec))[h]


@pytest.mark.parametrize("cid", MAIN + [EDGE])
def test_one_entry_per_group_recomputed(cid):
    """The last harmonic of the top degree of the last (system, source, ball): the assembled expectation is within 4 2^-52 scale of the
    40-digit value, which is what the bound of the GPU tests adds."""
    rec = CASES[cid]
    st, s, r, b = rec.st, rec.nb - 1, len(rec.src) - 1, rec.B - 1
    h = int(_top(st)[-1])
    n = rec.n_end - 1
    k = complex(rec.k[s]) if rec.k[s].imag else float(rec.k[s].real)
    with mp.workdps(50):
        tvec = mpv(rec.src[r] - rec.centers[b])
        assert all(mp.mpf(float(a)) - mp.mpf(float(c)) == v for a, c, v in zip(rec.src[r], rec.centers[b], tvec))
        dist = mp.sqrt(mp.fsum(v * v for v in tvec))
        G, _ = R.point_source_G(st.d, rec.n_end, k, rec.gj[s, b], dist)
        y = _y(rec, rec.src[r] - rec.centers[b], h)
        f, scale, _ = FX.expected_point_source(rec)
        assert abs(complex(G[n] * mp.conj(y)) - f[s, r, b, h]) <= FX.ASSEMBLY * scale[s, r, b, h]
        Y, yscale, _ = FX.expected_harmonics(rec)
        assert abs(complex(y) - Y[r * rec.B + b, h]) <= FX.ASSEMBLY * yscale[r * rec.B + b, h]
        if rec.kind == "main":
            yp = _y(rec, rec.dirs[r], h)
            want = R.plane_wave_factor(st.d, k, rec.dirs[r], rec.centers[b]) * mp.mpc(0, 1) ** n * MF._mp(rec.gj[s, b, n]) * mp.conj(yp)
            g, gscale, _ = FX.expected_plane_wave(rec)
            assert abs(complex(want) - g[s, r, b, h]) <= FX.ASSEMBLY * gscale[s, r, b, h]


@pytest.mark.parametrize("cid", WIDE)
def test_one_entry_of_the_70_sources_recomputed(cid):
    rec = CASES[cid]
    main = CASES[rec.main]
    st, r, h = rec.st, 69, int(_top(rec.st)[0])
    with mp.workdps(50):
        tvec = mpv(rec.src[r] - main.centers[0])
        G, _ = R.point_source_G(st.d, rec.n_end, float(main.k[0].real), main.gj[0, 0], mp.sqrt(mp.fsum(v * v for v in tvec)))
        want = G[int(st.deg[h])] * mp.conj(_y(rec, rec.src[r] - main.centers[0], h))
    f, scale, _ = FX.expected_wide(rec, main)
    assert abs(complex(want) - f[0, r, 0, h]) <= FX.ASSEMBLY * scale[0, r, 0, h]
    assert len({tuple(v) for v in rec.src}) == FX.WIDE_NRHS


@pytest.mark.parametrize("cid", ["bbbba-5", "ba-48"])
def test_power_recomputed(cid):
    rec = CASES[cid]
    dens, pu, pv = FX.power_inputs(rec.st.deg, rec.pexps)
    r, b = 1, 0
    al, be = np.full(rec.n_end, rec.palpha[b]), np.full(rec.n_end, rec.pbeta[b])
    pe, pa, cond, se, sa = R.power(rec.st.d, rec.n_end, float(rec.k[0].real), rec.radii[b], al, be, rec.ptab[b], dens[r, b], pu[r, b], pv[r, b], rec.st.deg)
    assert (float(pe), float(pa)) == tuple(rec.pwant[r, b]) and (float(se), float(sa)) == tuple(rec.pscale[r, b]) and float(cond) == rec.pcond[r, b]


# ---------------------------------------------------------------------------- the rebuilt inputs
def test_rebuilt_inputs_are_exact_and_deterministic():
    rec = CASES["ba-48"]
    one, two = FX.power_inputs(rec.st.deg, rec.pexps), FX.power_inputs(rec.st.deg, rec.pexps)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    dens, pu, pv = one
    for z, e in ((dens, rec.pexps[:, 0]), (pu, np.zeros_like(rec.pexps[:, 0])), (pv, rec.pexps[:, 2])):
        for part in (np.abs(z.real), np.abs(z.imag)):
            ints = np.ldexp(part, 4 - e[None, :, :][..., rec.st.deg].astype(np.int64)[0][None])
            assert np.array_equal(ints, np.round(ints)) and ints.min() >= 1 and ints.max() <= 15
    assert np.array_equal(FX.dyadic(5, 0), np.array([1 + 13j, 15 + 14j, 14 + 15j, 13 + 1j, 12 + 2j]) / 16.0)     # the formula, pinned


def test_the_generator_reproduces_the_small_cases():
    spec = importlib.util.spec_from_file_location("make_full_order_rhs_fixtures",
                                                  os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_full_order_rhs_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with mp.workdps(40):
        for tree in ("bbbba", "bbbbbbbba"):
            cid, meta, rec = gen.main_case(tree, lambda *_: None)
            for key, v in rec.items():
                assert np.array_equal(np.asarray(v), getattr(CASES[cid], key)), (cid, key)
        cid, meta, rec = gen.edge_case(lambda *_: None)
        for key, v in rec.items():
            assert np.array_equal(np.asarray(v), getattr(CASES[cid], key)), (cid, key)


# ---------------------------------------------------------------------------- mp_rhs against the fp64 yardsticks
LOW = [("a", 6), ("ba", 6), ("bba", 4), ("caa", 4), ("bbba", 3)]
CEN = np.array([[0.4, -0.3, 0.2, 0.5, -0.1], [2.9, 0.6, -0.4, 0.3, 0.2]])
RAD = np.array([1.0, 0.7])
GEN = np.array([0.3, -0.8, 0.45, 0.6, -0.2])


def _mp_rhs(tree, n_end, k, gj, vec, dist, factor):
    """[H] complex: factor_n conj(Y_h(vec)) with factor from the point-source or the plane-wave closed form."""
    st = FX.structure(tree, n_end)
    Y = R.tree_harmonics(tree, n_end, mpv(vec))
    return np.array([complex(factor[int(n)] * mp.conj(y)) for n, y in zip(st.deg, Y)])


@pytest.mark.parametrize("k", [1.3, 0.9 + 0.3j])
@pytest.mark.parametrize("tree,n_end", LOW)
def test_point_source_and_plane_wave_against_the_yardsticks(tree, n_end, k):
    tr = oracle_tree(tree)
    d = tr.d
    cen, src = CEN[:, :d], CEN[0, :d] + 1.7 * GEN[:d] / np.linalg.norm(GEN[:d])
    p = GEN[:d] / np.linalg.norm(GEN[:d])
    want_ps = PS.rhs(tr, n_end, k, cen, RAD, *ROBIN, src)
    want_pw = PW.rhs(tr, n_end, k, cen, RAD, *ROBIN, p)
    worst_ps = worst_pw = 0.0
    with mp.workdps(40):
        for b in range(2):
            gj = O.ball_tables(tr, n_end, k, 1.0, RAD[b], np.full(n_end, ROBIN[0]), np.full(n_end, ROBIN[1]))[0]
            tvec = mpv(src) if b < 0 else [mp.mpf(float(s)) - mp.mpf(float(c)) for s, c in zip(src, cen[b])]
            G, _ = R.point_source_G(d, n_end, k, gj, mp.sqrt(mp.fsum(v * v for v in tvec)))
            got = _mp_rhs(tree, n_end, k, gj, [float(v) for v in tvec], None, G)
            worst_ps = max(worst_ps, np.abs(got - want_ps[b]).max() / np.abs(want_ps[b]).max())
            pf = R.plane_wave_factor(d, k, p, cen[b])
            got = _mp_rhs(tree, n_end, k, gj, p, None, [pf * mp.mpc(0, 1) ** n * MF._mp(gj[n]) for n in range(n_end)])
            worst_pw = max(worst_pw, np.abs(got - want_pw[b]).max() / np.abs(want_pw[b]).max())
    print(f"{tree} n_end {n_end} k {k}: mp_rhs against the yardsticks: point source {worst_ps:.1e}, plane wave {worst_pw:.1e} of max |f|")
    assert worst_ps <= 4 * TIE_MEASURED["point_source"] and worst_pw <= 4 * TIE_MEASURED["plane_wave"]


@pytest.mark.parametrize("tree,n_end", LOW)
def test_power_against_the_yardstick(tree, n_end):
    """power_yardstick.power on a record with random outgoing coefficients and the projections of a plane wave, against mp_rhs.power fed
    the same coefficients (blc = 1) and projections."""
    tr = oracle_tree(tree)
    d, k = tr.d, 1.3
    deg = tr.degrees(n_end)
    rng = np.random.default_rng(n_end)
    coef = rng.normal(size=(2, len(deg))) + 1j * rng.normal(size=(2, len(deg)))
    res = types.SimpleNamespace(tree=tr, n_end=n_end, k=k, radii=RAD, centers=CEN[:, :d], coef=coef)
    uin, ugr = O.plane_wave(k, GEN[:d] / np.linalg.norm(GEN[:d]))
    alpha, beta = np.array([ROBIN[0], 1.0]), np.array([ROBIN[1], 0.0])
    ext, ab, _ = PY.power(res, uin, ugr, alpha, beta)
    U, V = PY.projections(res, uin, ugr)
    worst = 0.0
    for b in range(2):
        j, _, jp, _ = O.radial_h(n_end - 1, d, k * RAD[b])
        tab = np.stack([alpha[b] * j + beta[b] * k * jp, np.zeros(n_end), np.ones(n_end)]).astype(np.complex128)
        pe, pa, _, se, sa = R.power(d, n_end, k, RAD[b], np.full(n_end, alpha[b]), np.full(n_end, beta[b]), tab, coef[b], U[b], V[b], deg)
        worst = max(worst, abs(float(pe) - ext[b]) / float(se), abs(float(pa) - ab[b]) / float(sa) if sa != 0 else abs(ab[b]))
    print(f"{tree} n_end {n_end}: mp_rhs.power against the yardstick {worst:.1e} of sum |terms|")
    assert worst <= 4 * TIE_MEASURED["power"]


@pytest.mark.parametrize("d,n_end", [(5, 4), (6, 4), (10, 3)])
def test_chain_harmonics_against_the_chain_yardstick(d, n_end):
    ch = chain(d)
    assert R.chain_index(d, n_end) == ch.index(n_end)
    worst = 0.0
    with mp.workdps(40):
        for v in (np.array([0.3, -0.5, 0.7, 0.2, -0.4, 0.6, 0.1, -0.2, 0.35, 0.15])[:d], np.array([-0.2, 0.1, 0.05, 0.9, 0.3, -0.6, 0.2, 0.1, -0.7, 0.4])[:d]):
            want = ch.harmonics((v / np.linalg.norm(v))[None], n_end)[:, 0]
            got = np.array([complex(y) for y in R.chain_harmonics(d, n_end, mpv(v))])
            worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f"chain d = {d}, n_end {n_end}: {worst:.1e}")
    assert worst <= 4 * TIE_MEASURED["chain"]


@pytest.mark.parametrize("d,name", [(3, "ba"), (4, "bba")])
def test_chain_harmonics_are_the_oracle_s_ba_and_bba(d, name):
    """To 1e-35: two statements of the same functions at 40 digits, directions on the axes included."""
    with mp.workdps(40):
        for v in ([0.3, -0.5, 0.7, 0.2][:d], [1.0, 0.0, 0.0, 0.0][:d], [0.0, 0.0, 0.0, 1.0][4 - d:], [0.6, -0.8, 0.0, 0.0][:d]):
            u = mpv(v)
            r = mp.sqrt(mp.fsum(x * x for x in u))
            a, b = R.chain_harmonics(d, 9, u), MF.harmonics(name, 9, [x / r for x in u])
            assert R.chain_index(d, 9) == [tuple(int(i) for i in lab) for lab in O.tree(name).index(9)]
            assert max(abs(x - y) for x, y in zip(a, b)) <= mp.mpf("1e-35")


# ---------------------------------------------------------------------------- planted faults: the checker alone
def _top(st):
    return np.flatnonzero(st.deg == st.n_end - 1)


def _faults(rec, want):
    """{name: perturbed copy of want [..., H]} for the faults a ceiling test exists to find."""
    st = rec.st
    top, below = _top(st), np.flatnonzero(st.deg == st.n_end - 2)
    out = {}
    g = want.copy()
    g[..., top] = 0.0
    out["top degree of G dropped"] = g
    # the radial row shifted by one at n_end - 1: G_{n_end-2} in place of G_{n_end-1}
    G = rec.G if rec.kind != "wide" else rec.G[np.arange(FX.WIDE_NRHS) % FX.WIDE_GROUPS][None, :, None]
    g = want.copy()
    g[..., top] = want[..., top] * (G[..., st.n_end - 2] / G[..., st.n_end - 1])[..., None]
    out["degrees shifted by one at n_end - 1"] = g
    # +-m swapped in the top degree: the harmonic with the last signed label entry negated
    lab = [tuple(l) for l in st.labels.tolist()]
    where = {l: i for i, l in enumerate(lab)}
    swap = np.array([where[lab[i][:-1] + (-lab[i][-1],)] for i in top])
    g = want.copy()
    g[..., top] = want[..., swap]
    out["+-m swapped in the top degree"] = g
    g = want.copy()
    g[..., top] = want[..., top] * (1.0 + 1e-9)
    out["h_{n_end-1} off by a relative 1e-9"] = g
    assert len(below) > 0
    return out


@pytest.mark.parametrize("cid", MAIN + [EDGE])
def test_planted_faults_in_a_point_source_result_are_refused(cid):
    rec = CASES[cid]
    want, scale, weight = FX.expected_point_source(rec)
    assert FX.within(want, want, scale, weight, FX.C["point_source"]).all()
    for name, got in _faults(rec, want).items():
        ok = FX.within(got, want, scale, weight, FX.C["point_source"])
        assert not ok.all(), (cid, name)
        print(f"{cid}: {name}: {int((~ok).sum())} entries refused, largest ratio {FX.worst(got, want, scale, weight)[0]:.3g}")
    bad = want.copy()
    bad[0, 0, 0, 0] = np.nan
    assert not FX.within(bad, want, scale, weight, FX.C["point_source"]).all()


@pytest.mark.parametrize("cid", WIDE)
def test_planted_faults_in_the_70_right_hand_sides_are_refused(cid):
    rec = CASES[cid]
    want, scale, weight = FX.expected_wide(rec, CASES[rec.main])
    assert FX.within(want, want, scale, weight, FX.C["point_source"]).all()
    faults = _faults(rec, want)
    for col in (0, 31, 63, 68):                                   # inside a tile, across the 32-wide tiles, across the wave of 64
        g = want.copy()
        g[:, [col, col + 1]] = want[:, [col + 1, col]]
        faults[f"column {col} exchanged with its neighbour"] = g
    for name, got in faults.items():
        ok = FX.within(got, want, scale, weight, FX.C["point_source"])
        assert not ok.all(), (cid, name)
        print(f"{cid}: {name}: {int((~ok).sum())} entries refused")


@pytest.mark.parametrize("cid", MAIN)
def test_planted_faults_in_harmonics_and_plane_waves_are_refused(cid):
    rec = CASES[cid]
    st = rec.st
    top = _top(st)
    lab = [tuple(l) for l in st.labels.tolist()]
    where = {l: i for i, l in enumerate(lab)}
    swap = np.array([where[lab[i][:-1] + (-lab[i][-1],)] for i in top])
    for group, (want, scale, weight) in (("harmonics", FX.expected_harmonics(rec)), ("plane_wave", FX.expected_plane_wave(rec))):
        assert FX.within(want, want, scale, weight, FX.C[group]).all()
        for name, idx, factor in (("top degree dropped", top, 0.0), ("+-m swapped in the top degree", swap, 1.0), ("top degree off by 1e-9", top, 1.0 + 1e-9)):
            got = want.copy()
            got[..., top] = want[..., idx] * factor
            assert not FX.within(got, want, scale, weight, FX.C[group]).all(), (cid, group, name)


@pytest.mark.parametrize("cid", ["a-320", "bbba-8"])
def test_planted_faults_in_the_power_are_refused(cid):
    """A relative 1e-9 of one sum, and the loss of the top degree's terms (recomputed in fp64 from the same inputs)."""
    rec = CASES[cid]
    want, scale = rec.pwant, np.where(rec.pscale == 0.0, 1e-300, rec.pscale)
    weight = np.broadcast_to(np.maximum(float(rec.n_end), rec.k[0].real * rec.radii)[None, :, None], want.shape)
    assert FX.within(want, want, scale, weight, FX.C["power"]).all()
    assert not FX.within(want * (1.0 + 1e-9), want, scale, weight, FX.C["power"]).all()
    dens, pu, pv = FX.power_inputs(rec.st.deg, rec.pexps)
    k, r, b, d, n_end = float(rec.k[0].real), 0, 0, rec.st.d, rec.n_end
    al, be = np.full(n_end, rec.palpha[b]), np.full(n_end, rec.pbeta[b])
    keep = rec.st.deg < n_end - 1
    pe, pa, *_ = R.power(d, n_end, k, rec.radii[b], al, be, rec.ptab[b], dens[r, b][keep], pu[r, b][keep], pv[r, b][keep], rec.st.deg[keep])
    got = want.copy()
    got[r, b] = (float(pe), float(pa))
    ok = FX.within(got, want, scale, weight, FX.C["power"])
    assert not ok[r, b, 0] and not ok[r, b, 1]
