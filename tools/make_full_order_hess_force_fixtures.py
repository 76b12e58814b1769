#!/usr/bin/env python3
"""Write tests/golden/full_order_hess_force.npz: radiation forces (and, with the cases of hess_case_list, Hessians) at the order
ceilings of the kernels on densities that show every degree, evaluated at 40 digits.  CPU only (mpmath); a sibling of
tools/make_full_order_fixtures.py, whose geometry, regimes and candidate points it imports.

    python tools/make_full_order_hess_force_fixtures.py            # write the fixture
    python tools/make_full_order_hess_force_fixtures.py --check    # recompute and compare with the committed file, array by array
    python tools/make_full_order_hess_force_fixtures.py --only force-ba-48-osc-robin

Force cases: real k, kind outer, two balls of radii 1.0 / 0.7 on a 320, ba 48, bpa 48, bba 14, bpbpa 14, caa 12 at k rho_0 = 0.8 n_end
(osc) and 0.28 n_end (evan), one Robin pair and one per-degree pair of penetrable fluid spheres (the formula of fluid_inclusion_bc, one
interior wavenumber complex) evaluated at 40 digits and stored as the fp64 numbers the library is given.  The density is
w[b, h] t[b, n] (oracle/full_order_fixture.py) with t such that max(|u_h|, |v_h|) of the surface traces is |w_h|, in [0.5, 1.5].

Expected Phi (oracle/mp_force.py): the per-degree factors (j_n, k j_n', gj_n, blc_n, Wr) from the mp radial functions, T the table that is independent
of the plan (tests/force_yardstick.py: closed forms for a and ba, the oracle tree's rule otherwise), the double sum in mp.  A ball is
admitted only with cond = sum |terms| / |Phi_b| <= COND_MAX and force_yardstick.force in fp64 within ORACLE_MAX of |Phi_b|; both
are stored.  The table w of a (family, order) is drawn from the first seed that admits every case of the family.  No case may come
near the kernel's rule for a zero gj_n, except the one made for it: ba 48 with the transparent sphere's pair in the TOP degree of
ball 0 alone, whose expected output is NaN for that ball and the 40-digit value for the other.
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import biem_oracle as O  # noqa: E402
from oracle import full_order_fixture as FX  # noqa: E402

import make_full_order_fixtures as G  # noqa: E402

COND_MAX, ORACLE_MAX = G.COND_MAX, G.ORACLE_MAX
FORCE_ORDERS = (("a", 320), ("ba", 48), ("bpa", 48), ("bba", 14), ("bpbpa", 14), ("caa", 12))
ROBIN = (1.0 + 0.5j, 0.3 - 0.2j)                     # the absorbing pair of tests/test_power_host.py
DENSITY_RATIO = (0.5, 3.0)
FORCE_CANCEL = 64.0 * 2.220446049250313e-16          # kernels_force.hip: |gj| below this fraction of its two terms counts as zero
CLEAR_OF_THE_RULE = 1e3                              # ... and every ordinary case stays this factor above it
SEEDS = 20
BATCH_K = (1.0, 0.6, 0.35)                            # the launch-shape case: three systems from the oscillatory to the evanescent regime,
BATCH_RADII = (1.0, 0.9, 1.1)                         # each with its own radii, two right-hand sides (w and w rolled by one harmonic)


# --------------------------------------------------------------------------------------
# the case list
# --------------------------------------------------------------------------------------
def force_case_list():
    cases = []
    for tree, n_end in FORCE_ORDERS:
        for rg in ("osc", "evan"):
            for bc in ("robin", "fluid"):
                cases.append(dict(id=f"force-{tree}-{n_end}-{rg}-{bc}", family="force", tree=tree, n_end=n_end, regime=rg, bc=bc))
    cases.append(dict(id="force-ba-48-osc-transparent-top", family="force", tree="ba", n_end=48, regime="osc", bc="transparent-top"))
    cases.append(dict(id="force-ba-48-batch-robin", family="force", tree="ba", n_end=48, regime="batch", bc="robin"))
    return cases


HESS_BELOW = (("a", 318), ("ba", 46), ("bpa", 46), ("bba", 12), ("bpbpa", 12), ("caa", 10))     # the value kernel runs at the ceiling order
HESS_AT = (("a", 320), ("bba", 14), ("caa", 12))                                                 # ... two orders above it (plans 322 / 16 / 14)
MIN_VALID = 16


def hess_case_list():
    cases = []

    def add(kind, tree, n_end, rg):
        cases.append(dict(id=f"hess-{kind}-{tree}-{n_end}-{rg}", family="hess", kind=kind, tree=tree, n_end=n_end, regime=rg))

    for tree, n_end in HESS_BELOW + HESS_AT:
        for rg in (("osc", "evan", "cplx") if G.DIM[tree] == 3 else ("osc", "evan")):
            add("ext", tree, n_end, rg)
            if tree in ("a", "ba", "bba", "caa"):
                add("inner", tree, n_end, rg)
    return cases


def case_list():
    return force_case_list() + hess_case_list()


def hess_candidates(case, cen, rad):
    """The candidate points of tools/make_full_order_fixtures.py; kind inner has one ball, so it gets further generic points to keep
    MIN_VALID of them."""
    pts = G.candidates(case, cen, rad)
    if case["kind"] == "inner":
        d = G.DIM[case["tree"]]
        g = [G._unit(v[:d]) for v in G.GEN]
        pts += [(0, G._unit(g[i % 5] - 0.5 * g[(i + 2) % 5]), f, "both") for i, f in enumerate((0.7, 0.35, 0.9, 0.15, 0.6, 0.25, 0.85))]
    return pts


def build_hess_case(args):
    import mpmath as mp
    from oracle import mp_field as M

    import hess_yardstick as HY

    case, w = args
    t0 = time.time()
    np.seterr(invalid="ignore", over="ignore")
    tree, n_end, kind = case["tree"], case["n_end"], case["kind"]
    tr = O.tree(tree)
    d = tr.d
    ph = G.physics(case)
    cen, rad, k, eta = ph["centers"], ph["radii"], ph["k"], ph["eta"]
    B = len(rad)
    t, _ = G.scales(case, ph)
    dens = FX.density(w[:B], t, tr.degrees(n_end))
    mkind = "inner" if kind == "inner" else "outer"
    F = M.MPField(tree, n_end, k, eta, cen, rad, dens, mkind)
    rows, moves = [], 0
    for spec in hess_candidates(case, cen, rad):
        for attempt in range(G.TRIES):
            b, u, f = G.moved(spec, attempt, d)
            x = cen[b] + rad[b] * f * u
            assert F.valid("near", F._x(x)), (case["id"], spec)
            vals, sabs = F.value("near", x, with_cond=True)
            with mp.workdps(M.DPS):
                cond = float(mp.fsum(sabs) / abs(mp.fsum(vals)))
            err = np.inf
            if cond <= COND_MAX:
                with mp.workdps(M.DPS):
                    Hm = M.hessian_by_differences(F, F._x(x), M.HESS_STEPS[0])
                hess = np.array([[complex(v) for v in row] for row in Hm])
                twin = HY.hessian(tree, n_end, k, eta, mkind, cen, rad, dens, x[None], sparse_table=True)[:, :, 0]
                err = float(np.linalg.norm(twin - hess) / np.linalg.norm(hess))
                if err <= ORACLE_MAX:
                    with mp.workdps(M.DPS):                # the acceptance of MPField.hessian: the second step agrees
                        H2 = M.hessian_by_differences(F, F._x(x), M.HESS_STEPS[1])
                        worst = max(abs(Hm[i][j] - H2[i][j]) for i in range(d) for j in range(d)) / max(abs(v) for row in Hm for v in row)
                    assert worst <= M.STEP_AGREE, (case["id"], spec, float(worst))
                    rows.append(dict(x=x, hess=hess, cond=cond, oracle_err=err))
                    break
            if spec[3] == "fixed":
                raise RuntimeError(f"{case['id']}: the fixed point {spec} has condition {cond:.3g}, twin error {err:.3g}")
            moves += 1
        else:
            raise RuntimeError(f"{case['id']}: no admissible point near {spec} (last: condition {cond:.3g}, twin error {err:.3g})")
    xn = G.nan_point(case, cen, rad)
    assert not F.valid("near", F._x(xn))
    P = len(rows) + 1
    assert P % 64 != 0 and len(rows) >= MIN_VALID, (case["id"], P)
    nan = complex(np.nan, 0.0)
    arrays = dict(centers=cen, radii=rad, t=t, x=np.array([r["x"] for r in rows] + [xn]), valid=np.array([True] * len(rows) + [False]),
                  hess_upper=np.stack([r["hess"] for r in rows] + [np.full((d, d), nan)], axis=-1)[np.triu_indices(d)], cond=np.array([r["cond"] for r in rows] + [np.nan]),
                  oracle_err=np.array([r["oracle_err"] for r in rows] + [np.nan]))
    kc = complex(k)
    meta = dict(family="hess", tree=tree, kind=mkind, regime=case["regime"], n_end=n_end, k=[kc.real, kc.imag], eta=eta, w=case["w"])
    print(f"{case['id']:26s} P={P:3d} moved {moves:3d}x  max cond {arrays['cond'][:-1].max():6.1f}  twin err {arrays['oracle_err'][:-1].max():.1e}  "
          f"{time.time() - t0:5.1f}s", flush=True)
    return case["id"], meta, arrays


def force_w(family, n_end, seed):
    """w[2, H]: |w| uniform in [0.5, 1.5], phases uniform over the circle."""
    H = O.tree(family).n_harm(n_end)
    rng = np.random.default_rng([{"a": 2, "ba": 3, "bba": 4, "caa": 5}[family], n_end, 20261020, seed])
    return _single(rng.uniform(0.5, 1.5, (2, H)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (2, H))))


def hess_w(family, n_end):
    """The table of tools/make_full_order_fixtures.py for (family, order), in single precision."""
    return _single(G.shared_w(family, n_end))


def _single(w):
    """Rounded to single precision and stored so: still exact fp64 numbers of modulus in [0.5, 1.5], at half the size."""
    return w.astype(np.complex64)


# --------------------------------------------------------------------------------------
# boundary pairs (fp64 numbers: what the library is given) and the per-degree factors at 40 digits
# --------------------------------------------------------------------------------------
def boundary_pair(case, k, rad):
    """(alpha[B, n_end], beta[B, n_end]) complex128, and k_interior[B] (fluid pairs)."""
    import mpmath as mp
    from oracle import mp_field as M

    d, n_end, B = G.DIM[case["tree"]], case["n_end"], len(rad)
    an = np.full((B, n_end), ROBIN[0], dtype=np.complex128)
    bn = np.full((B, n_end), ROBIN[1], dtype=np.complex128)
    kb = None

    def fluid(kbv, delta, rho):
        """-k_b j_n'(k_b rho), delta j_n(k_b rho), scaled to max(|alpha_n|, |k beta_n|) = 1, rounded to fp64."""
        z = M._mp(kbv) * mp.mpf(float(rho))
        j, jp = M._with_derivative(M.radial_j(n_end, d, z), z)
        a = [-M._mp(kbv) * jp[n] for n in range(n_end)]
        b = [mp.mpf(float(delta)) * j[n] for n in range(n_end)]
        s = [max(abs(a[n]), abs(mp.mpf(float(k)) * b[n])) for n in range(n_end)]
        return np.array([complex(a[n] / s[n]) for n in range(n_end)]), np.array([complex(b[n] / s[n]) for n in range(n_end)])

    with mp.workdps(M.DPS):
        if case["bc"] == "fluid":
            kb = np.array([0.6 * n_end / rad[0], 0.45 * n_end / rad[1] * (1.0 + 0.02j)])
            for b in range(B):
                an[b], bn[b] = fluid(kb[b], DENSITY_RATIO[b], rad[b])
        if case["bc"] == "transparent-top":            # k_b = k, delta = 1 in the top degree of ball 0: gj_n = 0 there
            a, b = fluid(float(k), 1.0, rad[0])
            an[0, -1], bn[0, -1] = a[-1], b[-1]
    return an, bn, kb


def gj_margin(tree, n_end, k, rad, an, bn):
    """[B, n_end]: |gj_n| / (|alpha_n j_n| + |beta_n k j_n'|) in fp64 with the oracle's radial functions - what the kernel's rule tests."""
    d = G.DIM[tree]
    out = np.zeros((len(rad), n_end))
    for b, rho in enumerate(rad):
        j, _, jp, _ = O.radial_h(n_end - 1, d, k * rho)
        out[b] = np.abs(an[b] * j + bn[b] * k * jp) / (np.abs(an[b] * j) + np.abs(bn[b] * k * jp))
    return out


def fp64_force(tree, n_end, k, eta, rad, dens, an, bn, table):
    """force_yardstick.force in fp64 on the same inputs and the same table (sparse)."""
    import force_yardstick as FY

    tr = O.tree(tree)
    deg = tr.degrees(n_end)
    blc = np.stack([O.ball_tables(tr, n_end, float(k), eta, rho, 1.0, 0.0)[2] for rho in rad])
    res = O.OracleResult(tr, n_end, float(k), eta, np.zeros((len(rad), tr.d)), np.asarray(rad), dens, dens * blc[:, deg], None, None)
    return FY.force(res, an, bn, table)


_TABLES = {}


def table_of(tree, n_end):
    import force_yardstick as FY

    if (tree, n_end) not in _TABLES:
        _TABLES[tree, n_end] = FY.independent_table(tree, n_end)
    return _TABLES[tree, n_end]


def _one_system(case, k, rad, w, an, bn, skip=()):
    """(t[B, n_end], phi[B, d], cond[B], oracle_err[B]) of one system with the table w[B, H]."""
    import mpmath as mp
    from oracle import mp_field as M
    from oracle import mp_force as MF

    tree, n_end = case["tree"], case["n_end"]
    deg = O.tree(tree).degrees(n_end)
    fac = MF.factors(tree, n_end, k, 1.0, rad, an, bn)
    t = np.ones((len(rad), n_end))
    with mp.workdps(M.DPS):
        for b in range(len(rad)):
            if b not in skip:
                t[b] = [float(1 / max(abs(fac[b][0][n]), abs(fac[b][1][n]))) for n in range(n_end)]
    assert np.isfinite(t).all() and (t > 0).all()
    table = table_of(tree, n_end)
    phi, cond = [], []
    errs = []
    for wr in w:                                                   # right-hand sides
        dens = FX.density(wr, t, deg)
        p, c = MF.force(tree, n_end, k, rad, fac, dens, table, skip)
        o = fp64_force(tree, n_end, k, 1.0, rad, dens, an, bn, table)
        phi.append(p), cond.append(c)
        errs.append(np.linalg.norm(o - p, axis=1) / np.linalg.norm(p, axis=1))
    return t, np.array(phi), np.array(cond), np.array(errs)


def build_force_case(case, seed):
    """None if the seed is refused (a ball's cond or fp64 error above the caps), otherwise (id, meta, arrays)."""
    t0 = time.time()
    np.seterr(invalid="ignore", over="ignore")
    tree, n_end, bc = case["tree"], case["n_end"], case["bc"]
    _, rad = G._two_balls(G.DIM[tree])
    w = force_w(G.FAMILY[tree], n_end, seed)
    batch = case["regime"] == "batch"
    k0 = {"osc": 0.8, "evan": 0.28, "batch": 0.8}[case["regime"]] * n_end / rad[0]
    systems = [(k0 * fk, rad * fr) for fk, fr in zip(BATCH_K, BATCH_RADII)] if batch else [(k0, rad)]
    ws = [w, np.roll(w, 1, axis=1)] if batch else [w]
    skip = (0,) if bc == "transparent-top" else ()
    rows = []
    for k, r in systems:
        an, bn, kb = boundary_pair(case, k, r)
        margin = gj_margin(tree, n_end, k, r, an, bn)
        if skip:
            assert margin[0, -1] < FORCE_CANCEL / 8, margin[0, -1]            # the planted degree trips the rule, with room
            margin[0, -1] = 1.0
        assert margin.min() > CLEAR_OF_THE_RULE * FORCE_CANCEL, (case["id"], margin.min())
        t, phi, cond, err = _one_system(case, k, r, ws, an, bn, skip)
        rows.append(dict(k=k, radii=r, t=t, phi=phi, cond=cond, oracle_err=err, alpha_n=an, beta_n=bn, k_interior=kb, margin=margin.min()))
    cond = np.array([r["cond"] for r in rows])
    err = np.array([r["oracle_err"] for r in rows])
    ok = np.nanmax(cond) <= COND_MAX and np.nanmax(err) <= ORACLE_MAX
    print(f"{case['id']:34s} seed {seed}  max cond {np.nanmax(cond):6.1f}  fp64 yardstick {np.nanmax(err):.1e}  min gj margin "
          f"{min(r['margin'] for r in rows):.1e}  {'ok' if ok else 'REFUSED'}  {time.time() - t0:5.1f}s", flush=True)
    if not ok:
        return None
    stack = lambda name: np.array([r[name] for r in rows]) if batch else rows[0][name]
    arrays = dict(radii=stack("radii"), t=stack("t"), phi=stack("phi") if batch else rows[0]["phi"][0],
                  cond=stack("cond") if batch else rows[0]["cond"][0], oracle_err=stack("oracle_err") if batch else rows[0]["oracle_err"][0])
    if bc != "robin":
        arrays.update(alpha_n=stack("alpha_n"), beta_n=stack("beta_n"))
    if bc == "fluid":
        arrays.update(k_interior=stack("k_interior"), density_ratio=np.array(DENSITY_RATIO))
    meta = dict(family="force", tree=tree, kind="outer", regime=case["regime"], bc=bc, n_end=n_end, eta=1.0, seed=seed,
                k=[float(r["k"]) for r in rows] if batch else float(rows[0]["k"]), w=f"force_{G.FAMILY[tree]}_{n_end}_{seed}",
                alpha=[ROBIN[0].real, ROBIN[0].imag], beta=[ROBIN[1].real, ROBIN[1].imag])
    return case["id"], meta, arrays


def _try(args):
    return build_force_case(*args)


def build_all(cases, jobs, first_seed):
    """Every case of a (family, order) with the first seed that admits them all (a partial run starts at the seed the file holds)."""
    groups = {}
    for c in cases:
        groups.setdefault((G.FAMILY[c["tree"]], c["n_end"]), []).append(c)
    done = {}
    with multiprocessing.get_context("fork").Pool(jobs) as pool:
        pending = {key: first_seed.get(key, 0) for key in groups}
        while pending:
            work = [(c, seed) for key, seed in pending.items() for c in groups[key]]
            work.sort(key=lambda cs: -O.tree(cs[0]["tree"]).n_harm(cs[0]["n_end"]) * (6 if cs[0]["regime"] == "batch" else 1))
            res = pool.map(_try, work, chunksize=1)
            for key in list(pending):
                mine = [r for (c, _), r in zip(work, res) if (G.FAMILY[c["tree"]], c["n_end"]) == key]
                if all(r is not None for r in mine):
                    done.update({r[0]: r[1:] for r in mine})
                    del pending[key]
                else:
                    pending[key] += 1
                    if pending[key] >= SEEDS:
                        raise RuntimeError(f"no seed below {SEEDS} admits every force case of {key}")
    return done


def pack(meta, arrays):
    """What the file holds of a case: a zip member costs some 250 bytes whatever it holds, so the small geometry arrays go into the
    JSON record (Python prints and reads a float exactly) and the two admission figures into one single-precision array."""
    meta, arrays = dict(meta), dict(arrays)
    for name in ("centers", "radii", "density_ratio"):
        if name in arrays:
            meta[name] = arrays.pop(name).tolist()
    if "k_interior" in arrays:
        meta["k_interior"] = [[[z.real, z.imag] for z in row] for row in np.atleast_2d(arrays.pop("k_interior")).tolist()]
    arrays["caps"] = np.stack([arrays.pop("cond"), arrays.pop("oracle_err")]).astype(np.float32)
    return meta, arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=FX.HESS_FORCE_PATH)
    ap.add_argument("--check", action="store_true", help="recompute and compare with the file instead of writing it")
    ap.add_argument("--only", nargs="*", help="case ids (with --check: compare only these; otherwise the file holds only these)")
    ap.add_argument("--jobs", type=int, default=min(8, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    cases = [c for c in case_list() if not args.only or c["id"] in args.only]
    first_seed = {}
    if args.only and os.path.exists(args.out):
        with np.load(args.out, allow_pickle=False) as z:
            for name in z.files:
                if name.endswith("/meta") and name.startswith("force-"):
                    m = json.loads(str(z[name]))
                    first_seed[G.FAMILY[m["tree"]], m["n_end"]] = m["seed"]
    by_id = build_all([c for c in cases if c["family"] == "force"], args.jobs, first_seed)
    hess = [c for c in cases if c["family"] == "hess"]
    tables = {}
    seeds = dict(first_seed)
    seeds.update({(G.FAMILY[m["tree"]], m["n_end"]): m["seed"] for m, _ in by_id.values()})
    shared = {(G.FAMILY[tree], n_end) for tree, n_end in FORCE_ORDERS}
    for c in hess:                                       # at the ceilings the Hessian shares the table w of the force cases (the file's size)
        key = (G.FAMILY[c["tree"]], c["n_end"])
        if key in shared and key not in seeds:
            raise SystemExit(f"{c['id']} shares the table w of the force cases of {key}: build them in the same run, or into --out first")
        c["w"] = f"force_{key[0]}_{key[1]}_{seeds[key]}" if key in shared else f"hess_{key[0]}_{key[1]}"
        tables[c["w"]] = force_w(*key, seeds[key]) if key in shared else hess_w(*key)
    if hess:
        import hess_yardstick as HY

        t0 = time.time()
        for fam, n_end in sorted({(G.FAMILY[c["tree"]], c["n_end"] + s) for c in hess for s in (0, 2)}):
            HY.plan_table_sparse(fam, n_end)             # built once here: the workers inherit them
        print(f"host plans of the twin built in {time.time() - t0:.0f} s", flush=True)
        hess.sort(key=lambda c: -O.tree(c["tree"]).n_harm(c["n_end"]) * G.DIM[c["tree"]] ** 2 * (2 if c["kind"] == "ext" else 1))
        with multiprocessing.get_context("fork").Pool(args.jobs) as pool:
            by_id.update({cid: (meta, arrays) for cid, meta, arrays in pool.map(build_hess_case, [(c, tables[c["w"]]) for c in hess], chunksize=1)})
    order = [c["id"] for c in case_list() if not args.only or c["id"] in args.only]
    store = {"cases": np.array(json.dumps(order))}
    for cid in order:
        meta, arrays = pack(*by_id[cid])
        store[cid + "/meta"] = np.array(json.dumps(meta))
        store.update({f"{cid}/{name}": a for name, a in arrays.items()})
        kind_, family, order_ = meta["w"].split("_")[:3]
        store["w/" + meta["w"]] = force_w(family, int(order_), int(meta["w"].split("_")[3])) if kind_ == "force" else hess_w(family, int(order_))
    if args.check:
        bad = 0
        with np.load(args.out, allow_pickle=False) as z:
            for name, a in store.items():
                if name == "cases" and args.only:
                    continue
                if name not in z.files or not np.array_equal(z[name], a, equal_nan=a.dtype.kind in "fc"):
                    print("differs:", name)
                    bad += 1
            if not args.only:
                for name in sorted(set(z.files) - set(store)):
                    print("only in the file:", name)
                    bad += 1
        print(f"{len(store)} arrays compared, {bad} differ")
        return 1 if bad else 0
    np.savez_compressed(args.out, **store)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(order)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
