"""GPU tests of incidence by expansion coefficients: ``biem_rhs_expansion`` against the NumPy yardsticks of the regular-wave
and multipole right-hand sides (neither uses the library's term lists), against the merged single-harmonic kernels, on unit vectors,
bit for bit across table slices, right-hand-side counts and the LDS budget; a plane wave by ``plane_wave_coefficients``; the whole path
(``biem`` / ``fac.solve`` on every solve path, ``cluster_coefficients`` against ``tmatrix @ p``, force and power); the fields
``regular_expansion`` / ``multipole_expansion``.  tests/test_expansion_host.py holds what needs no device."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import multipole_source_yardstick as MS  # noqa: E402
import regular_wave_yardstick as RW  # noqa: E402
from test_gpu_point_source import ETA, ROBIN, _tables, geometry, ptr, sources, t, tc  # noqa: E402
from test_gpu_regular_wave import _pair, canon, coefficients, origins, otree, plan_of, rhs_regular, ti  # noqa: E402

KS2 = (1.3, 0.9 + 0.3j)                      # one real k, one with Im k != 0
TOL = 1e-12                                  # the asserted figure of the single-index f, here of the sum of magnitudes
TREES = ["a", "ba", "bpa", "bba", "caa", "bbba"]


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def device():
    return torch.device("cuda", torch.cuda.current_device())


def outgoing_translation(tr, n_end, k, tv):
    """SR[h', h] = (S|R)_{h'->h}(t): the multipole yardstick; a chain by the closed-form Gaunt lists of tests/chain_yardstick.py with the
    outgoing table, as RW.translation_rr does with the regular one."""
    if not RW.is_chain(tr):
        return MS.translation(tr, n_end, k, tv)
    import chain_yardstick as CY

    r, u = RW._direction(tv)
    d = tr.d
    Cd = (2 * math.pi) ** (d / 2.0) * math.sqrt(2.0 / math.pi)
    g = CY.gaunt(d, n_end)
    T = Cd * RW.outgoing_radial(2 * n_end - 2, d, k * r)[g.deg2] * g.ch.harmonics(u[None, :], g.n2)[:, 0]
    out = np.zeros((g.H, g.H), dtype=np.complex128)
    for hp in range(g.H):
        for h in range(g.H):
            lab, cf = g.terms(hp, h)
            out[hp, h] = cf @ T[lab]
    return out


def xr(tr, n_end, n_in, k, tv, regular):
    """XR[h' on the axis of order n_in, h on the axis of order n_end]: the yardstick at the larger order (its entries do not depend on the
    order), rows and columns picked by label."""
    n_list = max(n_in, n_end)
    big = RW.translation_rr(tr, n_list, k, tv) if regular else outgoing_translation(tr, n_list, k, tv)
    return big[np.ix_(RW.raised_index(tr, n_in, n_list), RW.raised_index(tr, n_end, n_list))]


_XR = {}


def xr_cached(tr, n_end, n_in, k, tv, regular):
    """xr, kept: the 9 + 9 + 1 right-hand sides of a case share three origins per system."""
    key = (tr.name, n_end, n_in, complex(k), np.asarray(tv, dtype=np.float64).tobytes(), regular)
    if key not in _XR:
        if len(_XR) >= 64:
            _XR.clear()
        X = xr(tr, n_end, n_in, k, tv, regular)
        _XR[key] = (X, np.abs(X))
    return _XR[key]


def want_f(tr, n_end, n_in, k, cen, rad, alpha, beta, o, p, regular):
    """(f[B, H], scale): f = -gj sum_h' p_h' XR[h', h] of one system and one right-hand side, scale = max_{b,h} |gj_h| sum_h' |p_h'| |XR_{h'h}|."""
    B = len(rad)
    deg = RW.degrees(tr, n_end)
    an, bn = RW._full(alpha, B, n_end), RW._full(beta, B, n_end)
    out = np.zeros((B, len(deg)), dtype=np.complex128)
    scale = 0.0
    for b in range(B):
        gj = RW.ball_gj(tr, n_end, k, rad[b], an[b], bn[b])[deg]
        X, aX = xr_cached(tr, n_end, n_in, k, np.asarray(cen[b], dtype=np.float64) - np.asarray(o, dtype=np.float64), regular)
        out[b] = -gj * (p @ X)
        scale = max(scale, (np.abs(gj) * (np.abs(p) @ aX)).max())
    return out, scale


def rhs_expansion(amd, tree, n_end, n_in, regular, nb, B, k, cen, geom_b, tab, org, org_batched, P, p_batched, stage=0):
    """biem_rhs_expansion into the natural layout; org [nb or 1, n_origin, d] and P [nb or 1, nrhs, H_in] (the axis of order n_in) as
    NumPy in canonical axes; f[nb, nrhs, B, H] as NumPy.  The coefficients and the solve plan's harmonics go onto the axis of the list
    plan by label, as the binding does."""
    from biem_helmholtz_sphere_amd._plans import _label_positions

    lib = amd._biem.L.load()
    ct = canon(amd, tree)[0]
    plan, n_list = plan_of(amd, tree, n_end), max(n_in, n_end)
    lists = plan_of(amd, tree, n_list)
    H, nrhs, n_origin = plan.H, P.shape[1], org.shape[1]
    placed = np.zeros(P.shape[:2] + (lists.H,), dtype=np.complex128)
    placed[..., _label_positions(ct, n_in, n_list, device())] = P
    imap = ti(_label_positions(ct, n_end, n_list, device()))
    wb = int(lib.biem_rhs_expansion_workspace_bytes(lists.handle, nb, B, n_origin))
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    f = torch.full((nb, nrhs, B * H), 7.0, dtype=torch.complex128, device="cuda")
    ot, pt = t(org), tc(placed)
    amd._biem.L.check(lib.biem_rhs_expansion(plan.handle, nb, B, nrhs, ptr(k), ptr(cen), geom_b, ptr(tab), ptr(ot), org_batched, n_origin, ptr(pt),
                                             p_batched, lists.handle, ptr(imap), n_in, int(regular), ptr(f), nrhs * B * H, 1, B * H, stage,
                                             ptr(work), wb, 0), "biem_rhs_expansion")
    torch.cuda.synchronize()
    return f.cpu().numpy().reshape(nb, nrhs, B, H)


def random_p(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def setup(amd, tree, n_end, coef, regular, seed=0, ks=KS2):
    """Two systems (ks) with their own centres, 3 balls (2 in four and five dimensions), and per system three origins: regular - outside
    all balls, inside ball 1, on the centre of ball 0; outgoing - three sources outside."""
    tr = otree(tree)
    d, nb = tr.d, len(ks)
    B = 3 if d <= 3 else 2
    cen, rad = geometry(B, d)
    cens = np.stack([cen + 0.1 * s for s in range(nb)])
    pairs, al, be, per_degree = coefficients(amd, coef, d, n_end, rad, ks)
    k = tc(ks)
    tab = _tables(amd, plan_of(amd, tree, n_end), nb, B, k, t(rad), al, be, per_degree)
    if regular:
        org = np.stack([origins(cens[s], rad) for s in range(nb)])                               # [nb, 3, d]
    else:
        org = np.broadcast_to(sources([(cens[s], rad) for s in range(nb)], 3, seed=seed + d), (nb, 3, d)).copy()
    return tr, d, nb, B, cens, rad, pairs, k, tab, org


# ---------------------------------------------------------------------------- 1. f against the yardstick
def _orders(tree):
    return [(3, 3), (3, 6), (3, 2)] if tree == "bbba" else [(1, 1), (1, 4), (2, 2), (2, 5), (5, 5), (5, 8), (5, 2)]


CASES1 = [(tree, n_end, n_in, "fluid" if (7 * n_end + n_in + len(tree)) % 2 else "robin") for tree in TREES for n_end, n_in in _orders(tree)]


@pytest.mark.parametrize("regular", [True, False], ids=["regular", "outgoing"])
@pytest.mark.parametrize("tree,n_end,n_in,coef", CASES1, ids=[f"{a}-{b}-{c}-{e}" for a, b, c, e in CASES1])
def test_rhs_expansion_against_the_yardstick(amd, tree, n_end, n_in, coef, regular):
    """Random complex coefficient vectors of order n_in (n_end, n_end + 3, 2 under n_end 5) against f = -gj sum_h' p_h' XR[h', h] of the
    yardstick, batched geometry, Robin or degree-dependent coefficients (both occur for every tree): 9 right-hand sides (more than one
    register tile) about one origin per system - the three kinds of origin in turn over the systems and the case -, 9 about their own
    origins (the three, cycled), and 1.  Error per (system, right-hand side) relative to max_{b,h} |gj_h| sum_h' |p_h'| |XR_{h'h}|: 1e-12."""
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, coef, regular)
    _, perm = canon(amd, tree)
    H_in = len(RW.degrees(tr, n_in))
    rng = np.random.default_rng(n_end + 10 * n_in)
    P = random_p(rng, nb, 9, H_in)
    cen_t = t(cens[:, :, perm])
    worst = {}
    for form in ("shared", "own", "one"):
        if form == "own":
            Og = org[:, np.arange(9) % 3]                                                        # [nb, 9, d]
        else:
            pick = [(s + n_end + n_in) % 3 for s in range(nb)]
            Og = np.stack([org[s, pick[s]] for s in range(nb)])[:, None]                         # [nb, 1, d]
        Pf = P[:, :1] if form == "one" else P
        got = rhs_expansion(amd, tree, n_end, n_in, regular, nb, B, k, cen_t, 1, tab, Og[..., perm], 1, Pf, 1)
        assert np.isfinite(got).all()
        w = 0.0
        for s in range(nb):
            for r in range(Pf.shape[1]):
                want, scale = want_f(tr, n_end, n_in, KS2[s], cens[s], rad, *pairs[s], Og[s, r if form == "own" else 0], Pf[s, r], regular)
                w = max(w, np.abs(got[s, r] - want).max() / scale)
        worst[form] = w
    print(f"{tree} n_end {n_end} n_in {n_in} {coef} {'regular' if regular else 'outgoing'}: error / scale " +
          ", ".join(f"{f} {w:.1e}" for f, w in worst.items()))
    assert max(worst.values()) <= TOL, (tree, n_end, n_in, coef, regular, worst)


def test_shared_coefficients_and_shared_origins_are_the_batched_ones(amd):
    """coef_batched = 0 and origin_batched = 0 read one set for every system: the bits of the call that passes a copy per system."""
    tree, n_end, n_in = "ba", 3, 4
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, "robin", True)
    P = random_p(np.random.default_rng(2), 1, 9, len(RW.degrees(tr, n_in)))
    for Og in (org[:1, :1], org[:1, np.arange(9) % 3]):
        one = rhs_expansion(amd, tree, n_end, n_in, True, nb, B, k, t(cens), 1, tab, Og, 0, P, 0)
        all_ = rhs_expansion(amd, tree, n_end, n_in, True, nb, B, k, t(cens), 1, tab, np.repeat(Og, nb, axis=0), 1, np.repeat(P, nb, axis=0), 1)
        assert np.array_equal(one, all_)


# ---------------------------------------------------------------------------- 2. the merged kernels
CASES2 = [("a", 5, 5), ("ba", 5, 5), ("ba", 5, 2), ("bpa", 4, 4), ("bba", 3, 3), ("caa", 3, 3), ("bbba", 3, 3), ("bbba", 3, 2)]


def rhs_index(amd, plan, nb, B, nrhs, k, cen, tab, org, idx, regular):
    """biem_rhs_regular_wave / biem_rhs_multipole (batched origins and indices); f[nb, nrhs, B, H]."""
    if regular:
        return rhs_regular(amd, plan, nb, B, nrhs, k, cen, 1, tab, org, idx, 1)
    lib, H = amd._biem.L.load(), plan.H
    wb = int(lib.biem_rhs_multipole_workspace_bytes(plan.handle, nb, B, nrhs, 1, 1))
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    f = torch.full((nb, nrhs, B * H), 7.0, dtype=torch.complex128, device="cuda")
    amd._biem.L.check(lib.biem_rhs_multipole(plan.handle, nb, B, nrhs, ptr(k), ptr(cen), 1, ptr(tab), ptr(org), 1, ptr(idx), ptr(f),
                                             nrhs * B * H, 1, B * H, ptr(work), wb, 0), "biem_rhs_multipole")
    torch.cuda.synchronize()
    return f.cpu().numpy().reshape(nb, nrhs, B, H)


@pytest.mark.parametrize("regular", [True, False], ids=["regular", "outgoing"])
@pytest.mark.parametrize("tree,n_end,n_in", CASES2, ids=[f"{a}-{b}-{c}" for a, b, c in CASES2])
def test_rhs_expansion_is_the_sum_of_the_single_harmonic_kernels(amd, tree, n_end, n_in, regular):
    """biem_rhs_expansion(P) against sum_h' P_h' biem_rhs_regular_wave(index h') (biem_rhs_multipole) on the device, every h' of degree
    < n_in, per origin: 1e-12 of max_{b,h} sum_h' |P_h'| |f_h'[b, h]|, the scale of test 1.  P = e_h' reproduces the index call to the same
    tolerance, of max |f_h'|."""
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, "robin", regular)
    _, perm = canon(amd, tree)
    plan = plan_of(amd, tree, n_end)
    cen_t = t(cens[:, :, perm])
    where = RW.raised_index(tr, n_in, n_end) if n_in < n_end else np.arange(plan.H)            # the harmonics of degree < n_in
    H_in = len(where)
    rng = np.random.default_rng(5)
    worst = worst_unit = 0.0
    for o in range(3):
        Og = org[:, o:o + 1]
        single = rhs_index(amd, plan, nb, B, H_in, k, cen_t, tab, t(np.repeat(Og, H_in, axis=1)[..., perm]),
                           ti(np.broadcast_to(where, (nb, H_in))), regular)                        # [nb, h', B, H]
        P = random_p(rng, nb, 9, H_in)
        got = rhs_expansion(amd, tree, n_end, n_in, regular, nb, B, k, cen_t, 1, tab, Og[..., perm], 1, P, 1)
        want = np.einsum("srp,spbh->srbh", P, single)
        scale = np.einsum("srp,spbh->srbh", np.abs(P), np.abs(single)).max(axis=(2, 3))
        worst = max(worst, (np.abs(got - want).max(axis=(2, 3)) / scale).max())
        unit = rhs_expansion(amd, tree, n_end, n_in, regular, nb, B, k, cen_t, 1, tab, Og[..., perm], 1, np.eye(H_in)[None].astype(np.complex128), 0)
        worst_unit = max(worst_unit, (np.abs(unit - single).max(axis=(2, 3)) / np.abs(single).max(axis=(2, 3))).max())
    print(f"{tree} n_end {n_end} n_in {n_in} {'regular' if regular else 'outgoing'}: vs the sum of index calls {worst:.1e}, unit vectors {worst_unit:.1e}")
    assert worst <= TOL and worst_unit <= TOL, (tree, n_end, n_in, regular, worst, worst_unit)


# ---------------------------------------------------------------------------- 3. the origin on a centre
@pytest.mark.parametrize("tree", TREES)
def test_the_block_of_the_ball_the_origin_sits_on_is_minus_gj_p(amd, tree):
    """Regular, the origin on the centre of ball 0, n_in = n_end: (R|R)(0) is the identity with exact zeros off the diagonal, so that
    ball's block is -gj_n p_h, within 16 x 2^-52 relative entry by entry (the figure of the diagonal check of DESIGN.md 5o)."""
    n_end = 3 if tree == "bbba" else 5
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, "robin", True)
    _, perm = canon(amd, tree)
    plan = plan_of(amd, tree, n_end)
    P = random_p(np.random.default_rng(7), nb, 9, plan.H)
    f = rhs_expansion(amd, tree, n_end, n_end, True, nb, B, k, t(cens[:, :, perm]), 1, tab, cens[:, :1][..., perm], 1, P, 1)
    gj = tab.cpu().numpy()[:, 0, 0, :][:, plan.degrees]                                       # [nb, H]
    want = -gj[:, None, :] * P
    worst = (np.abs(f[:, :, 0, :] - want) / np.abs(want)).max()
    print(f"{tree} n_end {n_end}: block of the ball under the origin vs -gj_n p_h, worst relative error {worst / 2.0 ** -52:.1f} x 2^-52")
    assert np.isfinite(f).all() and worst <= 16 * 2.0 ** -52, (tree, worst)


# ---------------------------------------------------------------------------- 4. bit for bit
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "outgoing"])
@pytest.mark.parametrize("tree,n_end,n_in", [("ba", 4, 6), ("a", 4, 6), ("caa", 3, 2)])
def test_slices_counts_and_the_lds_budget_change_no_bit(amd, monkeypatch, tree, n_end, n_in, regular):
    """Within the shared-origin form and within the per-origin form: BIEM_RHS_TABLE_BYTES forcing at least 3 slices changes no bit (three
    systems: three slices in either form); each of 9 right-hand sides - every register slot of the first tile and the lone one of the
    second - has the bits of a call with that vector (and its origin) alone, and in the per-origin form also of a call with 2;
    BIEM_RHS_EX_LDS_BYTES=0 (table row and coefficients read from memory)
    changes no bit - both branches are the same statements in the same order of summation; and two calls agree."""
    lib = amd._biem.L.load()
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, "robin", regular, ks=(1.3, 0.9 + 0.3j, 0.9 - 0.3j))
    lists = plan_of(amd, tree, max(n_end, n_in))
    P = random_p(np.random.default_rng(11), nb, 9, len(RW.degrees(tr, n_in)))
    for form, Og in (("shared", org[:, 1:2]), ("own", org[:, np.arange(9) % 3])):
        run = lambda Pf=P, Of=Og: rhs_expansion(amd, tree, n_end, n_in, regular, nb, B, k, t(cens), 1, tab, Of, 1, Pf, 1)
        f0 = run()
        assert np.isfinite(f0).all() and np.array_equal(f0, run())
        for r in range(9):                                                                       # every register slot, both tiles
            assert np.array_equal(f0[:, r:r + 1], run(P[:, r:r + 1], Og[:, r:r + 1] if form == "own" else Og)), (form, r)
        if form == "own":                                                                        # (2 of them: the per-origin kernel itself)
            for r in (0, 3, 7):
                assert np.array_equal(f0[:, r:r + 2], run(P[:, r:r + 2], Og[:, r:r + 2])), (form, r)
        n_origin = Og.shape[1]
        if tree != "a":
            per_pair = B * lists.H2 * 16
            take = nb * n_origin // 3                                                            # 3 (system, origin) pairs: 1, 1, 1; 27: 9, 9, 9
            monkeypatch.setenv("BIEM_RHS_TABLE_BYTES", str(take * per_pair + 8))
            sliced = int(lib.biem_rhs_expansion_workspace_bytes(lists.handle, nb, B, n_origin))
            assert take * per_pair <= sliced < (take + 1) * per_pair
            assert np.array_equal(f0, run())
            monkeypatch.delenv("BIEM_RHS_TABLE_BYTES")
        else:
            assert int(lib.biem_rhs_expansion_workspace_bytes(lists.handle, nb, B, n_origin)) == 0
        monkeypatch.setenv("BIEM_RHS_EX_LDS_BYTES", "0")
        assert np.array_equal(f0, run())
        monkeypatch.delenv("BIEM_RHS_EX_LDS_BYTES")


def test_the_stages_are_the_whole(amd):
    """stage 1 (the table rows) then stage 2 (the contraction) of an unsliced call give the bits of stage 0."""
    tree, n_end, n_in = "ba", 4, 5
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, "robin", True)
    P = random_p(np.random.default_rng(3), nb, 3, len(RW.degrees(tr, n_in)))
    lib = amd._biem.L.load()
    from biem_helmholtz_sphere_amd._plans import _label_positions

    plan, lists = plan_of(amd, tree, n_end), plan_of(amd, tree, n_in)
    placed = np.zeros((nb, 3, lists.H), dtype=np.complex128)
    placed[..., _label_positions("ba", n_in, n_in, device())] = P
    imap, pt, ot, cen_t = ti(_label_positions("ba", n_end, n_in, device())), tc(placed), t(org[:, :1]), t(cens)
    wb = int(lib.biem_rhs_expansion_workspace_bytes(lists.handle, nb, B, 1))
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    H = plan.H
    out = []
    for stages in ((0,), (1, 2)):
        f = torch.full((nb, 3, B * H), 7.0, dtype=torch.complex128, device="cuda")
        for stage in stages:
            amd._biem.L.check(lib.biem_rhs_expansion(plan.handle, nb, B, 3, ptr(k), ptr(cen_t), 1, ptr(tab), ptr(ot), 1, 1, ptr(pt), 1, lists.handle,
                                                     ptr(imap), n_in, 1, ptr(f), 3 * B * H, 1, B * H, stage, ptr(work), wb, 0), "biem_rhs_expansion")
        torch.cuda.synchronize()
        out.append(f.cpu().numpy())
    assert np.isfinite(out[0]).all() and np.array_equal(*out)


def test_the_library_refuses_what_it_cannot_take(amd):
    tree, n_end = "ba", 3
    tr, d, nb, B, cens, rad, pairs, k, tab, org = setup(amd, tree, n_end, "robin", True)
    lib = amd._biem.L.load()
    plan, small = plan_of(amd, tree, n_end), plan_of(amd, tree, 2)
    f = torch.zeros((nb, 4, B * plan.H), dtype=torch.complex128, device="cuda")
    work = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    pt, ot, imap = tc(np.ones((nb, 4, plan.H))), t(org), ti(np.arange(plan.H))

    def call(lists=plan, n_in=n_end, n_origin=1, stage=0, wb=1 << 16):
        return lib.biem_rhs_expansion(plan.handle, nb, B, 4, ptr(k), ptr(t(cens)), 1, ptr(tab), ptr(ot), 1, n_origin, ptr(pt), 1, lists.handle,
                                      ptr(imap), n_in, 1, ptr(f), 4 * B * plan.H, 1, B * plan.H, stage, ptr(work), wb, 0)

    assert call() == 0
    for kw, text in ((dict(n_origin=3), b"neither 1 nor nrhs"), (dict(lists=small), b"list plan"), (dict(n_in=0), b"n_in=0"),
                     (dict(n_in=n_end + 1), b"n_in=4"), (dict(stage=3), b"stage=3"), (dict(wb=16), b"workspace too small")):
        assert call(**kw) == 1 and text in lib.biem_last_error(), (kw, lib.biem_last_error())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 5. a plane wave
def test_plane_wave_coefficients_against_the_yardsticks_harmonics(amd):
    """p_h = C_d i^n conj(Y_h(d^)) e^{i k d^.o} with the oracle's harmonics, every tree, real and complex k, unnormalised directions:
    1e-13 of max |p| (one harmonic, one exponential)."""
    for tree in TREES:
        c = amd.create_from_branching_types(tree)
        tr = otree(tree)
        d, n_in = tr.d, 4
        rng = np.random.default_rng(d)
        D, o = rng.normal(size=(d, 5)), rng.normal(size=(d, 1))
        ks = np.array([[1.3], [0.9 + 0.3j]])
        p = amd.plane_wave_coefficients(c, k=tc(ks), direction=t(D[:, None, :]), origin=t(o[:, None, :]), n_in=n_in)
        deg = RW.degrees(tr, n_in)
        assert tuple(p.shape) == (2, 5, len(deg))
        dh = D / np.linalg.norm(D, axis=0)
        Cd = (2 * math.pi) ** (d / 2.0) * math.sqrt(2.0 / math.pi)
        Y = tr.harmonics(dh.T, n_in)                                                            # [H, 5]
        want = Cd * (1j ** deg)[None, None, :] * np.conj(Y).T[None] * np.exp(1j * ks[:, :, None] * (dh * o).sum(axis=0)[None, :, None])
        err = np.abs(p.cpu().numpy() - want).max() / np.abs(want).max()
        print(f"{tree}: plane_wave_coefficients vs the oracle's harmonics {err:.1e}")
        assert err <= 1e-13, (tree, err)
    pn = amd.plane_wave_coefficients(amd.create_from_branching_types("ba"), k=1.3, direction=np.array([0.0, 0.6, 0.8]), origin=np.zeros(3), n_in=3)
    assert isinstance(pn, np.ndarray) and pn.shape == (9,)


def test_a_plane_wave_by_its_coefficients_is_the_plane_wave_solve(amd):
    """The two balls of tests/test_gpu_regular_wave.py at k = 0.3, n_end 4, P = plane_wave_coefficients(n_in=10) about their midpoint, so
    n_in > n_end: densities against biem(plane_wave_direction=).  The right-hand sides differ by the incident degrees n >= 10 about o,
    bounded on the cluster by (k R / 2)^10 / 10!, R = max_b (|c_b - o| + rho_b); a decade on it, of max |density|."""
    c = amd.create_from_branching_types("ba")
    k, n_end, n_in = 0.3, 4, 10
    cen, rad, o = _pair(k)
    dh = np.array([0.6, 0.0, 0.8])
    op = dict(centers=t(cen), radii=t(rad), k=t(k), n_end=n_end)
    want = amd.biem(c, plane_wave_direction=t(dh), **op).density.cpu().numpy()
    P = amd.plane_wave_coefficients(c, k=t(k), direction=t(dh), origin=t(o), n_in=n_in)
    assert tuple(P.shape) == (n_in * n_in,)
    got = amd.biem(c, regular_wave_origin=t(o), regular_wave_coefficients=P, **op).density.cpu().numpy()
    R = (np.linalg.norm(cen - o[None], axis=-1) + rad).max()
    bound = 10 * (k * R / 2) ** n_in / math.factorial(n_in)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"plane wave by 100 coefficients vs plane_wave_direction: {err:.1e} of max |density| (bound {bound:.1e})")
    assert got.shape == want.shape and err <= bound


# ---------------------------------------------------------------------------- 6. the whole path
#        id         B  n_end  flat   env
PATHS = [
    ("whole",      3, 5,     False, {}),
    ("lu",         3, 5,     False, {"BIEM_SOLVER": "lu"}),
    ("no_small",   3, 5,     False, {"BIEM_NO_SMALL_PATH": "1"}),
    ("split",      4, 6,     True,  {"BIEM_SYM_SPLIT": "1"}),
]


@pytest.mark.parametrize("regular", [True, False], ids=["regular", "outgoing"])
@pytest.mark.parametrize("cid,B,n_end,flat,env", PATHS, ids=[p[0] for p in PATHS])
def test_every_solve_path_solves_the_combination(amd, monkeypatch, cid, B, n_end, flat, env, regular):
    """biem(..., coefficients) and fac.solve(..., coefficients) against sum_h' P_h' density(index h'), the index solves on the same path:
    1e-12 of sum_h' |p_h'| max |density_h'| per (system, right-hand side).  Two systems (real and complex k), two coefficient vectors about
    one origin, n_in = n_end (the axis of the index solves)."""
    import ctypes as C

    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = amd.create_from_branching_types("ba")
    d, K, R = 3, len(KS2), 2
    cen, rad = geometry(B, d, flat)
    H = n_end * n_end
    if regular:
        o = origins(cen, rad)[1]
        if flat:
            o = cen[1] + 0.45 * rad[1] * np.eye(d)[0]
    else:
        o = sources([(cen, rad)], 1, seed=B)[0]                                                  # (off the plane of a flat layout: the split is the centres')
    pos, cf, ix = (("regular_wave_origin", "regular_wave_coefficients", "regular_wave_index") if regular else
                   ("multipole_source_position", "multipole_source_coefficients", "multipole_source_index"))
    op = dict(centers=t(cen[None, None]), radii=t(rad[None, None]), k=tc(np.asarray(KS2)[:, None]), eta=t(np.ones((K, 1))), n_end=n_end,
              alpha=ROBIN[0], beta=ROBIN[1])
    P = random_p(np.random.default_rng(B), K, R, H)
    Ot = t(o[:, None, None])                                                                   # (d, 1, 1): shared by the right-hand sides
    single = amd.biem(c, **{pos: t(np.broadcast_to(o[:, None, None], (d, 1, H)).copy()), ix: np.arange(H)[None, :]}, **op).density.cpu().numpy()
    direct = amd.biem(c, **{pos: Ot, cf: tc(P)}, **op)
    if cid == "split":
        npE, npO = C.c_int(), C.c_int()
        amd._biem.L.load().biem_last_solve_split(C.byref(npE), C.byref(npO))
        assert npE.value > 0 and npO.value > 0
    fac = amd.biem_factorize(c, **op)
    assert (fac.n_lu > 0) == (cid == "lu")
    factored = fac.solve(**{pos: Ot, cf: tc(P)})
    want = np.einsum("srp,spbh->srbh", P, single)
    scale = np.einsum("srp,sp->sr", np.abs(P), np.abs(single).max(axis=(2, 3)))
    for what, got in (("biem", direct.density), ("fac.solve", factored.density)):
        assert tuple(got.shape) == (K, R, B, H)
        err = (np.abs(got.cpu().numpy() - want).max(axis=(2, 3)) / scale).max()
        print(f"{cid} {'regular' if regular else 'outgoing'} {what}: error {err:.1e} of sum |p| max |density_h'|")
        assert err <= TOL, (cid, what, err)
    if cid == "whole" and regular:
        # the outgoing coefficients of the coefficient solve are T p
        T = fac.tmatrix(origin=t(o)).cpu().numpy()                                             # [K, 1, H, H]
        A = direct.cluster_coefficients(origin=t(o)).cpu().numpy()                             # [K, R, H]
        Tp = np.einsum("sah,srh->sra", T[:, 0], P)
        ascale = np.einsum("srh,sh->sr", np.abs(P), np.abs(T[:, 0]).max(axis=1))
        aerr = (np.abs(A - Tp).max(axis=2) / ascale).max()
        print(f"cluster_coefficients of the coefficient solve vs tmatrix @ p: {aerr:.1e} of sum |p| max |T column|")
        assert aerr <= TOL


@pytest.mark.parametrize("regular", [True, False], ids=["regular", "outgoing"])
def test_force_and_power_run_on_a_beam_solution(amd, regular):
    """Real k: calc.force() and calc.power(uin_grad=) of the expansion's own gradient are finite, per right-hand side; n_in > n_end, per
    right-hand-side origins."""
    c = amd.create_from_branching_types("ba")
    cen, rad = geometry(2, 3)
    n_end, n_in, R = 4, 6, 3
    org = (origins(cen, rad) if regular else sources([(cen, rad)], 3, seed=1)).T[:, None, :]                 # (d, 1, R)
    P = tc(random_p(np.random.default_rng(1), 1, R, n_in * n_in))
    kw = ({"regular_wave_origin": t(org), "regular_wave_coefficients": P} if regular else
          {"multipole_source_position": t(org), "multipole_source_coefficients": P})
    k = t([[1.3]])
    calc = amd.biem(c, centers=t(cen[None, None]), radii=t(rad[None, None]), k=k, n_end=n_end, alpha=ROBIN[0], beta=ROBIN[1], **kw)
    assert tuple(calc.density.shape) == (1, R, 2, n_end * n_end)
    F = calc.force(alpha=ROBIN[0], beta=ROBIN[1])
    make = amd.regular_expansion if regular else amd.multipole_expansion
    uin, ugr = make(c, k=k, coefficients=P, **{"origin" if regular else "source": t(org)})
    pw = calc.power(uin_grad=ugr, uin=uin, alpha=ROBIN[0], beta=ROBIN[1])
    assert F.numel() == R * 2 * 3 and torch.isfinite(F).all()
    for part in (pw.extinction, pw.absorption, pw.scattering):
        assert torch.isfinite(torch.as_tensor(part)).all()


# ---------------------------------------------------------------------------- 7. the fields
@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "caa", "bbba"])
def test_expansion_fields_against_the_yardsticks_samples(amd, tree):
    """regular_expansion / multipole_expansion at 30 points (regular: the origin itself among them) against sum_h' p_h' of the yardstick's
    samples: 1e-12 of sum |p_h'| max |term_h'|.  The gradient of the regular expansion against sum_h' p_h' grad regular_wave(index h') of the
    merged function: 1e-12 of sum |p_h'| max |grad term_h'|.  `.uin` of a coefficient solve is the expansion's callable."""
    c = amd.create_from_branching_types(tree)
    tr = otree(tree)
    d, n_in = tr.d, 3
    deg = RW.degrees(tr, n_in)
    H = len(deg)
    ks = np.array(KS2)
    o = np.array([0.3, -0.4, 0.2, 0.5, -0.1][:d])
    rng = np.random.default_rng(4)
    v = rng.normal(size=(30, d))
    x = o[None] + rng.uniform(0.3, 3.0, (30, 1)) * v / np.linalg.norm(v, axis=-1, keepdims=True)
    x[0] = o
    p = random_p(rng, 2, H)
    k, xt, ot = tc(ks), t(x.T), t(o[:, None])
    for regular in (True, False):
        make, key = (amd.regular_expansion, "origin") if regular else (amd.multipole_expansion, "source")
        uin, ugr = make(c, k=k, coefficients=tc(p), **{key: ot})
        xs = x if regular else x[1:]
        got = uin(t(xs.T)[..., None]).cpu().numpy()
        grad = ugr(t(xs.T)[..., None]).cpu().numpy()
        assert got.shape == (len(xs), 2) and grad.shape == (d, len(xs), 2) and np.isfinite(got).all() and np.isfinite(grad).all()
        for s in range(2):
            if regular:
                terms = np.stack([RW.regular_samples(tr, n_in, ks[s], o, hp, xs) for hp in range(H)])
            else:
                terms = np.stack([RW.outgoing_samples(tr, n_in, ks[s], o, np.eye(H)[hp], xs) for hp in range(H)])
            err = np.abs(got[:, s] - p[s] @ terms).max() / (np.abs(p[s]) @ np.abs(terms).max(axis=1))
            print(f"{tree} {'regular' if regular else 'outgoing'} k {ks[s]}: field {err:.1e} of sum |p| max |term|")
            assert err <= TOL, (tree, regular, s, err)
        single = amd.regular_wave if regular else amd.multipole_source
        gterms = np.stack([single(c, k=k, index=hp, n_end=n_in, **{key: ot})[1](t(xs.T)[..., None]).cpu().numpy() for hp in range(H)])  # [H, d, P, 2]
        gwant = np.einsum("sh,hdps->dps", p, gterms)
        gscale = np.einsum("sh,hs->s", np.abs(p), np.abs(gterms).max(axis=(1, 2)))
        gerr = (np.abs(grad - gwant).max(axis=(0, 1)) / gscale).max()
        print(f"{tree} {'regular' if regular else 'outgoing'}: gradient vs the sum of the single-harmonic gradients {gerr:.1e}")
        assert gerr <= TOL, (tree, regular, gerr)
    if tree in ("ba", "bpa"):
        cen, rad = geometry(2, d)
        res = amd.biem(c, centers=t(cen[None]), radii=t(rad[None]), k=k, n_end=2, regular_wave_origin=ot, regular_wave_coefficients=tc(p))
        uin = amd.regular_expansion(c, k=k, origin=ot, coefficients=tc(p))[0]
        assert tuple(res.uin(xt).shape) == (30, 2) and torch.equal(res.uin(xt), uin(xt[..., None]))
        with pytest.raises(ValueError, match="lies on or inside ball 0"):
            amd.biem(c, centers=t(cen[None]), radii=t(rad[None]), k=k, n_end=2, multipole_source_position=t(cen[0][:, None]),
                     multipole_source_coefficients=tc(p))
