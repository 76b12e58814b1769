"""biem_harmonics, biem_rhs_point_source, biem_rhs_plane_wave and biem_power AT the order ceilings (a 320, ba 48, bba 14, caa 12, bbba 8,
bbbba 5, the d = 10 chain at 3) against 40-digit values.

The suite otherwise runs ``k_harmonics`` / ``k_harmonics_chain`` at n_end <= 9, the point-source kernels at n_end <= 12 and the plane-wave
ones at n_end <= 9 relative to max |f| - a measure the top degrees, (rho / |t|)^n below the maximum, never reach - and ``k_power`` on
solved densities at n_end <= 8.  Every case here comes from ``tests/golden/full_order_rhs_a.npz`` / ``full_order_rhs.npz``
(``tools/make_full_order_rhs_fixtures.py``): factors rounded from 40 digits, multiplied by ``oracle.full_order_rhs_fixture``; the gj row
the kernels are fed is the fixture's, so the ball tables (pinned in tests/test_gpu_radial_full_order.py) do not enter.  Nothing
high-precision runs here.

Bound, per entry:  |got - want| <= (min(C 2^-52 weight, 1e-10) + 4 2^-52) scale  with
* harmonics      scale sqrt(N(d, n) / |S^{d-1}|) (the norm of the harmonics of degree n), weight n + 1;
* point source   scale |G_n| sqrt(N / |S|), G_n = -C_d gj_n h_n(k |t|), weight max(n + 1, |k| |t|);
* plane wave     scale C_d |e^{i k p.c}| |gj_n| sqrt(N / |S|), weight max(n + 1, |k| |c|)  (sincos(k p.c) loses |k| |c| units);
* power          scale sum |terms|, weight max(n_end, k rho);
1e-10 is the parity contract of BASELINE.md (a cap, not a measurement), 4 2^-52 the assembly of the stored factors.  One C per group:
8 x the largest ratio error / (2^-52 weight scale) measured on an MI355X, rounded up to a power of two (the rule of DESIGN.md 5f; the
measured ratios are FX.MEASURED and in DESIGN.md 5m).  Every test prints its largest ratio and where it sits before it asserts.
"""
import time

import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd
from oracle import full_order_rhs_fixture as FX

pytestmark = pytest.mark.gpu
CASES = FX.load()
MAIN = [c for c, r in CASES.items() if r.kind == "main"]
WIDE = [c for c, r in CASES.items() if r.kind == "wide"]
EDGE = "a-150-edge"
LAYOUTS = ["natural", "solve"]
# per group, the largest ratio measured on an MI355X and the C asserted (8 x, next power of two); kept beside the checker, which the
# planted-fault test of tests/test_full_order_rhs_host.py drives with the same constants
MEASURED = FX.MEASURED     # harmonics 8.99, point source 6.90, plane wave 5.84, power 2.90
C = FX.C                   # harmonics 128, point source 64, plane wave 64, power 32
assert all(C[g] == 2.0 ** int(np.ceil(np.log2(8.0 * MEASURED[g]))) for g in C)
BUILD_SECONDS = {}


def t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype).contiguous()


def tc(a):
    return t(a, torch.complex128)


def ptr(x):
    return int(x.data_ptr())


def plan_of(rec):
    """The plan of (tree, n_end), cached by the library for the process; the time of a first build is kept for the report."""
    key = (rec.tree, rec.n_end)
    t0 = time.perf_counter()
    plan = amd._biem._plan(rec.tree, rec.n_end, torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    BUILD_SECONDS.setdefault(key, time.perf_counter() - t0)
    width = rec.st.labels.shape[1]
    if rec.tree == "a":
        assert np.array_equal(plan.labels[:, 0], rec.st.labels[:, 0])
    else:
        assert np.array_equal(plan.labels[:, :width], rec.st.labels) and not plan.labels[:, width:].any()
    assert np.array_equal(plan.degrees, rec.st.deg) and plan.H == rec.st.H
    return plan


def report(group, what, got, want, scale, weight, names=None):
    """Print the largest ratio and where, then assert the bound on every entry."""
    ratio, where = FX.worst(got, want, scale, weight)
    err = float(np.abs(np.asarray(got)[where] - np.asarray(want)[where]))
    print(f"{what}: largest error / (2^-52 weight scale) = {ratio:.3g} at {where}{' ' + names if names else ''} "
          f"(error {err:.2e}, scale {float(np.asarray(scale)[where]):.2e}, weight {float(np.asarray(weight)[where]):.0f}); C = {C[group]:g}")
    assert np.isfinite(np.asarray(got)).all(), f"{what}: non-finite entries"
    ok = FX.within(got, want, scale, weight, C[group])
    assert ok.all(), f"{what}: {int((~ok).sum())} entries beyond the bound, largest ratio {ratio:.3g} at {where}"
    return ratio


def test_the_fixture_holds_the_ceilings_of_this_build():
    top = dict(amd._biem.USCAT_GRAD_N_END_MAX)
    assert top == {"a": 320, "ba": 48, "bba": 14, "caa": 12}
    top.update(FX.CHAIN_CEILINGS)
    assert sorted((CASES[c].tree, CASES[c].n_end) for c in MAIN) == sorted(top.items())
    assert sorted(CASES[c].tree for c in WIDE) == ["a", "ba"] and all(CASES[c].n_end == top[CASES[c].tree] for c in WIDE)
    assert CASES[EDGE].n_end == 150 and float(CASES[EDGE].k[0].real * CASES[EDGE].radii[0]) == 1.3


# ---------------------------------------------------------------------------- harmonics
@pytest.mark.parametrize("cid", MAIN + [EDGE])
def test_harmonics(cid):
    """biem_harmonics at the stored directions (the unnormalised t = source - centre of every (source, ball), then the plane-wave
    directions): every label, chains included."""
    rec = CASES[cid]
    plan = plan_of(rec)
    lib, P = amd._biem.L.load(), len(rec.hdirs)
    Y = torch.full((P, plan.H), 7.0, dtype=torch.complex128, device="cuda")
    amd._biem.L.check(lib.biem_harmonics(plan.handle, P, ptr(t(rec.hdirs)), ptr(Y), 0), "biem_harmonics")
    torch.cuda.synchronize()
    want, scale, weight = FX.expected_harmonics(rec)
    report("harmonics", f"{cid} harmonics, {P} directions", Y.cpu().numpy(), want, scale, weight)


# ---------------------------------------------------------------------------- the closed-form right-hand sides
def _gj_only(gj):
    """tab [nb, B, 3, n_end] with the fixture's gj row and NaN in the rows the right-hand sides must not read."""
    nb, B, n_end = gj.shape
    tab = np.full((nb, B, 3, n_end), np.nan + 1j * np.nan)
    tab[:, :, 0] = gj
    return tc(tab)


def _launch(entry, plan, nb, B, nrhs, k, cen, geom_batched, tab, dirs, dirs_batched, layout, wb):
    """One closed-form launcher into the natural layout [nb, nrhs, B H] or the solve layout [nb, B H, ld] (ld: nrhs rounded up to 8, the
    padding preset with a sentinel it must keep); returns f [nb, nrhs, B, H]."""
    lib, H = amd._biem.L.load(), plan.H
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    if layout == "natural":
        f = torch.full((nb, nrhs, B * H), 7.0, dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)
    else:
        ld = (nrhs + 7) // 8 * 8
        f = torch.full((nb, B * H, ld), 7.0, dtype=torch.complex128, device="cuda")
        strides = (B * H * ld, ld, 1)
    amd._biem.L.check(getattr(lib, entry)(plan.handle, nb, B, nrhs, ptr(k), ptr(cen), geom_batched, ptr(tab), ptr(dirs), dirs_batched, ptr(f),
                                          *strides, ptr(work), wb, 0), entry)
    torch.cuda.synchronize()
    f = f.cpu().numpy()
    if layout == "solve":
        assert (f[:, :, nrhs:] == 7.0).all()
        f = f[:, :, :nrhs].transpose(0, 2, 1)
    return f.reshape(nb, nrhs, B, H)


def point_source(plan, nb, B, nrhs, k, cen, geom_batched, gj, src, src_batched, layout):
    wb = int(amd._biem.L.load().biem_rhs_point_source_workspace_bytes(plan.handle, nb, B, nrhs, src_batched, geom_batched))
    return _launch("biem_rhs_point_source", plan, nb, B, nrhs, tc(k), t(cen), geom_batched, _gj_only(gj), t(src), src_batched, layout, wb)


def plane_wave(plan, nb, B, nrhs, k, cen, gj, dirs, layout):
    wb = int(amd._biem.L.load().biem_rhs_plane_wave_workspace_bytes(plan.handle, nb, nrhs, 0))
    return _launch("biem_rhs_plane_wave", plan, nb, B, nrhs, tc(k), t(cen), 0, _gj_only(gj), t(dirs), 0, layout, wb)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", MAIN + [EDGE])
def test_point_source(cid, layout):
    """Five sources (the edge: three) shared by the systems, h along the lanes, both write layouts; every entry finite and within the bound."""
    rec = CASES[cid]
    plan = plan_of(rec)
    got = point_source(plan, rec.nb, rec.B, len(rec.src), rec.k, rec.centers[:rec.B], 0, rec.gj, rec.src, 0, layout)
    report("point_source", f"{cid} point source [{layout}] (system, source, ball, harmonic)", got, *FX.expected_point_source(rec))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["a-320", "ba-48"])
def test_point_source_batched(cid, layout):
    """src_batched = geom_batched = 1: system s holds the sources rolled by s and its own copy of the centres."""
    rec = CASES[cid]
    plan = plan_of(rec)
    roll = (np.arange(5)[None, :] + np.arange(rec.nb)[:, None]) % 5                                 # [nb, 5]
    got = point_source(plan, rec.nb, rec.B, 5, rec.k, np.broadcast_to(rec.centers[:rec.B], (rec.nb,) + rec.centers[:rec.B].shape), 1, rec.gj,
                       rec.src[roll], 1, layout)
    want, scale, weight = (np.stack([v[s][roll[s]] for s in range(rec.nb)]) for v in FX.expected_point_source(rec))
    report("point_source", f"{cid} point source, batched [{layout}] (system, source, ball, harmonic)", got, want, scale, weight)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", WIDE)
def test_point_source_with_70_right_hand_sides(cid, layout):
    """70 distinct sources around one ball: in the solve layout r runs along the lanes (transpose tiles, G[n][r]), in the natural one h.
    Every entry is compared, so the top two degrees and far more than a tenth of the entries are; column r differs from its
    neighbours in the radial row (r % 7) and in the azimuth (r % 10)."""
    rec = CASES[cid]
    main = CASES[rec.main]
    plan = plan_of(rec)
    got = point_source(plan, 1, 1, FX.WIDE_NRHS, main.k[:1], main.centers[:1], 0, main.gj[:1, :1], rec.src, 0, layout)
    want, scale, weight = FX.expected_wide(rec, main)
    assert got.shape == want.shape == (1, FX.WIDE_NRHS, 1, rec.st.H)
    report("point_source", f"{cid} point source, 70 right-hand sides [{layout}] (system, source, ball, harmonic)", got, want, scale, weight)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", MAIN)
def test_plane_wave(cid, layout):
    """The five directions shared by the systems, h along the lanes, both write layouts."""
    rec = CASES[cid]
    plan = plan_of(rec)
    got = plane_wave(plan, rec.nb, rec.B, 5, rec.k, rec.centers[:rec.B], rec.gj, rec.dirs, layout)
    report("plane_wave", f"{cid} plane wave [{layout}] (system, direction, ball, harmonic)", got, *FX.expected_plane_wave(rec))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["a-320", "ba-48"])
def test_plane_wave_with_70_right_hand_sides(cid, layout):
    """70 directions of one ball and one system: the five stored ones, direction r % 5 in column r (neighbouring columns differ; the
    distinct columns are the point-source test's, which shares the transpose tiles).  Solve layout: r along the lanes."""
    rec = CASES[cid]
    plan = plan_of(rec)
    col = np.arange(FX.WIDE_NRHS) % 5
    got = plane_wave(plan, 1, 1, FX.WIDE_NRHS, rec.k[:1], rec.centers[:1], rec.gj[:1, :1], rec.dirs[col], layout)
    want, scale, weight = (v[:1, col, :1] for v in FX.expected_plane_wave(rec))
    report("plane_wave", f"{cid} plane wave, 70 right-hand sides [{layout}] (system, direction, ball, harmonic)", got, want, scale, weight)


# ---------------------------------------------------------------------------- power
def _power(rec, per_degree):
    plan = plan_of(rec)
    lib, n_end = amd._biem.L.load(), rec.n_end
    dens, pu, pv = FX.power_inputs(rec.st.deg, rec.pexps)
    if per_degree:
        al, be = FX.degree_pair(rec.palpha, rec.pbeta, n_end)
        tab, entry, sfx = rec.ptab_n, lib.biem_power_n, "_n"
    else:
        al, be, tab, entry, sfx = rec.palpha, rec.pbeta, rec.ptab, lib.biem_power, ""
    out = torch.full((1, FX.POWER_NRHS, 2, 2), 7.0, dtype=torch.float64, device="cuda")
    k = rec.k[:1].real + 0j
    args = [tc(k), t([1.0]), t(rec.radii), tc(al[None]), tc(be[None]), tc(tab[None]), tc(dens[None]), tc(pu[None]), tc(pv[None])]   # (kept alive)
    kk, eta, rad, a, b, tb, dn, u, v = (ptr(x) for x in args)
    amd._biem.L.check(entry(plan.handle, 1, 2, FX.POWER_NRHS, kk, eta, rad, 0, a, b, 0, tb, dn, u, v, ptr(out), 0), "biem_power" + sfx)
    torch.cuda.synchronize()
    got = out.cpu().numpy()[0]
    want, scale = getattr(rec, "pwant" + sfx), getattr(rec, "pscale" + sfx)
    weight = np.broadcast_to(np.maximum(float(n_end), k[0].real * rec.radii)[None, :, None], want.shape)
    assert (got[:, 1, 1] == 0.0).all()                                        # the lossless ball: the exact-0 branch in every degree
    assert (want[:, 0, 1] > 0.0).all() and getattr(rec, "pcond" + sfx).max() <= 100.0
    # (a scale of 0 admits only the exact 0; keep the ratio finite there)
    report("power", f"{rec.id} biem_power{sfx} (right-hand side, ball, P_ext / P_abs)", got, want, np.where(scale == 0.0, 1e-300, scale), weight)


@pytest.mark.parametrize("cid", MAIN)
def test_power(cid):
    """biem_power with the stored tables: ball 0 lossy (Im(alpha conj beta) = 0.35: the w != 0 branch at n = n_end - 1), ball 1 lossless
    (exactly 0), a term of modulus O(1) in every degree of both sums."""
    _power(CASES[cid], False)


@pytest.mark.parametrize("cid", ["a-320", "ba-48"])
def test_power_with_coefficients_per_degree(cid):
    _power(CASES[cid], True)


def test_zz_report_the_time_to_build_the_plans():
    print("plans built here (s): " + ", ".join(f"{tree} {n}: {s:.2f}" for (tree, n), s in BUILD_SECONDS.items())
          + f"; together {sum(BUILD_SECONDS.values()):.2f}")
