#!/usr/bin/env python3
"""Write tests/golden/full_order_fields.npz: the field, gradient and interior-field series at the order ceilings of the per-lane
kernels (n_end 320 / 48 / 14 / 12 on the trees a / ba / bba / caa), evaluated at 40 digits by oracle/mp_field.py.  CPU only.

    python tools/make_full_order_fixtures.py            # write the fixture (a few minutes on 8 cores)
    python tools/make_full_order_fixtures.py --check    # recompute and compare with the committed file, array by array
    python tools/make_full_order_fixtures.py --only ext-ba-48-osc

Densities are synthetic so that EVERY degree is visible: the term of harmonic h has modulus |w_h| in [0.5, 1.5] at a reference
radius (exterior 1.2 rho, kind inner and interior 0.8 rho; the far field has no radial factor), stored as w times a real per-degree
scale (oracle/full_order_fixture.py).  Each order runs at |k| rho = 0.8 n_end (oscillatory) and 0.28 n_end (top degrees evanescent),
the 3-D trees also at a complex k.

A case is refused if any valid point has a condition number sum |terms| / |sum| above COND_MAX in any quantity the GPU test checks
pointwise (value, per-ball value, far field), or if the fp64 oracle misses the 40-digit value there by more than ORACLE_MAX: then a
kernel that misses 1e-10 is wrong, not unlucky.  A candidate point that fails is moved (radius or direction, never its kind).
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

from oracle import biem_oracle as O  # noqa: E402
from oracle import full_order_fixture as FX  # noqa: E402

COND_MAX = 100.0
ORACLE_MAX = 1e-11
TRIES = 40
DIM = {"a": 2, "ba": 3, "bpa": 3, "bba": 4, "bpbpa": 4, "caa": 4}
ROOT_AXIS = {"a": 0, "ba": 0, "bba": 0, "caa": 0, "bpa": 2, "bpbpa": 3}      # canonical axis 0 in the caller's axes
FAMILY = {"a": "a", "ba": "ba", "bpa": "ba", "bba": "bba", "bpbpa": "bba", "caa": "caa"}
GEN = np.array([[0.3, -0.8, 0.45, 0.6], [-0.5, 0.4, 0.6, -0.3], [0.7, 0.2, -0.4, 0.5], [-0.2, -0.6, -0.7, 0.35], [0.55, 0.65, 0.3, -0.45]])
DEGENERATE = np.array([[0.6, -0.8, 0.0, 0.0], [0.0, 0.0, 0.7, 0.5], [0.0, 0.6, -0.8, 0.0], [0.7, 0.0, 0.0, -0.5]])   # the 4-D trees' degenerate azimuths


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _two_balls(d):
    """Two balls of different radii, off every axis (the geometry of tests/test_gpu_field_gradient.py)."""
    return np.array([[1.7, 0.9, -0.6, 0.5], [-1.4, -1.1, 0.8, -0.7]])[:, :d].copy(), np.array([1.0, 0.7])


def _one_ball(d):
    return np.array([[0.3, -0.2, 0.1, 0.2]])[:, :d].copy(), np.array([2.0])


# --------------------------------------------------------------------------------------
# the case list
# --------------------------------------------------------------------------------------
def case_list():
    v_max, g_max = FX.lds_row_ceiling(False), FX.lds_row_ceiling(True)
    cases = []

    def add(kind, tree, n_end, regime, grad=True):
        cases.append(dict(id=f"{kind}-{tree}-{n_end}-{regime}", kind=kind, tree=tree, n_end=n_end, regime=regime, with_grad=grad))

    def regimes(tree):
        return ("osc", "evan", "cplx") if DIM[tree] == 3 else ("osc", "evan")

    for tree, n_end in (("a", 320), ("ba", 48), ("bpa", 48), ("bba", 14), ("bpbpa", 14), ("caa", 12)):
        for rg in regimes(tree):
            add("ext", tree, n_end, rg)
    for rg in ("osc", "evan"):
        add("inner", "a", g_max, rg)                    # the largest order whose gradient rows fit the LDS
        if v_max != g_max:
            add("inner", "a", v_max, rg, grad=False)    # ... whose value rows fit
        add("inner", "a", v_max + 1, rg, grad=False)    # one above: the value falls through to the harmonic-by-harmonic kernel
        add("inner", "a", 320, rg, grad=False)          # the order ceiling, through that kernel as well
    for tree, n_end in (("ba", 48), ("bba", 14), ("caa", 12)):
        for rg in regimes(tree):
            add("inner", tree, n_end, rg)
    for rg in ("osc", "evan"):
        add("interior", "a", g_max, rg)
        if v_max != g_max:
            add("interior", "a", v_max, rg, grad=False)
    for tree, n_end in (("ba", 48), ("bpa", 48), ("bba", 14), ("bpbpa", 14), ("caa", 12)):
        for rg in ("osc", "evan"):
            add("interior", tree, n_end, rg)
    return cases


def physics(case):
    """Geometry, wavenumbers and fluids of a case (fp64 numbers; what the fixture stores)."""
    d, n_end, rg = DIM[case["tree"]], case["n_end"], case["regime"]
    frac = {"osc": 0.8, "evan": 0.28, "cplx": 0.8}[rg]
    cen, rad = _one_ball(d) if case["kind"] == "inner" else _two_balls(d)
    out = dict(centers=cen, radii=rad, eta=1.0)
    if case["kind"] == "interior":
        out["k"] = 0.5 * n_end / rad[0]                                       # the exterior medium: every j_n(k rho) in fp64 range
        kb = frac * n_end / rad
        out["k_interior"] = np.array([kb[0], kb[1] * (1.0 + 0.02j)])           # two fluids, one with a complex wavenumber
        out["density_ratio"] = np.array([0.5, 3.0])
    else:
        k = frac * n_end / rad[0]
        out["k"] = complex(k, 0.02 * k) if rg == "cplx" else float(k)
    return out


# --------------------------------------------------------------------------------------
# candidate points: (ball, direction, r / rho, what may move)
# --------------------------------------------------------------------------------------
def candidates(case, cen, rad):
    tree, d = case["tree"], DIM[case["tree"]]
    e = np.eye(d)
    root = e[ROOT_AXIS[tree]]
    g = [_unit(v[:d]) for v in GEN]
    ext = case["kind"] == "ext"
    pts = []
    for b in range(len(rad)):
        q = g[b:] + g[:b]                                                     # other generic directions per ball
        if ext:
            pts += [(b, q[0], 1.02, "dir"), (b, q[1], 1.5, "dir"), (b, q[2], 1.2, "both"), (b, q[3], 1.1, "both"), (b, q[4], 1.33, "both"),
                    (b, root, 1.2, "rad"), (b, -root, 1.3, "rad"), (b, e[0], 1.37, "rad")]
            deg_r = 1.25
        else:
            pts += [(b, q[0], 0.98, "dir"), (b, q[1], 0.05, "dir"), (b, q[2], 0.5, "both"), (b, q[3], 0.8, "both"), (b, q[4], 0.3, "both"),
                    (b, root, 0.6, "rad"), (b, -root, 0.7, "rad"), (b, e[0], 0.4, "rad"), (b, root, 0.0, "fixed")]      # ... the centre
            deg_r = 0.45
        if d == 4:
            pts += [(b, _unit(v), deg_r, "plane") for v in DEGENERATE]
        else:
            pts += [(b, _unit(q[0] + q[3]), 1.07 if ext else 0.9, "both"), (b, _unit(q[1] - q[2]), 1.45 if ext else 0.15, "both")]
    return pts


def nan_point(case, cen, rad):
    d = DIM[case["tree"]]
    u = _unit(GEN[0][:d])
    if case["kind"] == "ext":
        return cen[-1] + 0.5 * rad[-1] * u            # inside a ball
    if case["kind"] == "inner":
        return cen[0] + 1.1 * rad[0] * u              # outside the ball
    return cen[0] + 0.5 * (cen[1] - cen[0]) + 0.05 * u   # interior field: in no ball


def moved(spec, t, d):
    b, u, f, how = spec
    if t == 0 or how == "fixed":
        return b, u, f
    if how == "plane":                   # a degenerate azimuth: turn within the plane of its two non-zero components, which keeps the zeros
        u = u.copy()
        u[np.flatnonzero(u)[0]] *= 1.0 + 0.06 * t
        u = _unit(u)
    if how in ("rad", "both", "plane"):  # (a pole keeps its direction: only the zonal harmonics are non-zero there)
        f = f * (1.0 + 0.011 * t) if f > 1.0 else f * (1.0 - 0.011 * t)
    if how in ("dir", "both"):
        u = _unit(u + 0.07 * t * _unit(GEN[(t + 2) % len(GEN)][:d]))
    return b, u, f


# --------------------------------------------------------------------------------------
# fp64 yardsticks: biem_oracle.uscat, and the algebraic interior formula from the oracle's radial functions
# --------------------------------------------------------------------------------------
def _rad64(nmax, d, z):
    z = complex(z)
    return O.radial_h(nmax, d, z if z.imag != 0 else z.real)


def interior_fp64(tr, n_end, k, eta, cen, rad, dens, kb, delta, x, b):
    """a = -s delta k W / gj and sum_h a j_n(k_b r) Y_h at one point of ball b (as _alg_coef / _u_from_coef of tests/test_gpu_interior_field.py)."""
    d, deg = tr.d, tr.degrees(n_end)
    _, _, blc = O.ball_tables(tr, n_end, k, eta, rad[b], 1.0, 0.0)
    xk = k * rad[b]
    j, _, jp, _ = _rad64(n_end - 1, d, xk)
    jz, _, jpz, _ = _rad64(n_end - 1, d, kb[b] * rad[b])
    gj = -kb[b] * jpz * j + delta[b] * jz * k * jp
    a = -(dens[b] * blc[deg]) * (delta[b] * k * (1j / xk ** (d - 1)) / gj)[deg]
    rel = x - cen[b]
    r = np.linalg.norm(rel)
    if r > 0:
        jn, u = _rad64(n_end - 1, d, kb[b] * r)[0], rel / r
    else:
        import math
        jn = np.zeros(n_end, dtype=np.complex128)
        jn[0] = math.sqrt(math.pi / 2) * 2.0 ** (1 - d / 2) / math.gamma(d / 2)
        u = np.eye(d)[0]
    return np.sum(a * jn[deg] * tr.harmonics(u[None], n_end)[:, 0])


# --------------------------------------------------------------------------------------
# one case
# --------------------------------------------------------------------------------------
def shared_w(family, n_end):
    """w[2, H]: |w| uniform in [0.5, 1.5], phases uniform over the circle; seeded by (family, n_end)."""
    H = O.tree(family).n_harm(n_end)
    rng = np.random.default_rng([{"a": 2, "ba": 3, "bba": 4, "caa": 5}[family], n_end, 20260101])
    return rng.uniform(0.5, 1.5, (2, H)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (2, H)))


def scales(case, ph):
    """The real per-degree scales t (and t_far) [B, n_end] that put every term at modulus |w_h| at the reference radius."""
    import mpmath as mp
    from oracle import mp_field as M

    tree, n_end, kind = case["tree"], case["n_end"], case["kind"]
    B = len(ph["radii"])
    H = O.tree(tree).n_harm(n_end)
    F = M.MPField(tree, n_end, ph["k"], ph["eta"], ph["centers"], ph["radii"], np.zeros((B, H)), "inner" if kind == "inner" else "outer",
                  ph.get("k_interior"), ph.get("density_ratio"))
    t, t_far = np.zeros((B, n_end)), np.zeros((B, n_end))
    with mp.workdps(M.DPS):
        for b in range(B):
            rho = F.rho[b]
            if kind == "ext":
                blc, z = F.blc(b, False), M.radial_h(n_end - 1, F.d, F.k * rho * mp.mpf("1.2"))
                t_far[b] = [float(1 / abs(blc[n])) for n in range(n_end)]
            elif kind == "inner":
                blc, z = F.blc(b, True), M.radial_j(n_end - 1, F.d, F.k * rho * mp.mpf("0.8"))
            else:
                blc, z = F.interior_factor(b), M.radial_j(n_end - 1, F.d, F.kb[b] * rho * mp.mpf("0.8"))
            t[b] = [float(1 / (abs(blc[n]) * abs(z[n]))) for n in range(n_end)]
    return t, (t_far if kind == "ext" else None)


def build_case(case):
    import mpmath as mp
    from oracle import mp_field as M

    t0 = time.time()
    np.seterr(invalid="ignore", over="ignore")       # SciPy's y_n overflows at orders the kind-inner sums never read
    tree, n_end, kind = case["tree"], case["n_end"], case["kind"]
    tr = O.tree(tree)
    d = tr.d
    ph = physics(case)
    cen, rad, k, eta = ph["centers"], ph["radii"], ph["k"], ph["eta"]
    B = len(rad)
    deg = tr.degrees(n_end)
    w = shared_w(FAMILY[tree], n_end)[:B]
    t, t_far = scales(case, ph)
    dens = FX.density(w, t, deg)
    assert np.isfinite(dens).all() and np.isfinite(t).all()
    mkind = "inner" if kind == "inner" else "outer"
    mode = "interior" if kind == "interior" else "near"
    F = M.MPField(tree, n_end, k, eta, cen, rad, dens, mkind, ph.get("k_interior"), ph.get("density_ratio"))
    res = O.OracleResult(tr, n_end, k, eta, cen, rad, dens, None, None, None, mkind)
    if kind == "ext":
        dens_far = FX.density(w, t_far, deg)
        Ff = M.MPField(tree, n_end, k, eta, cen, rad, dens_far, "outer")
        resf = O.OracleResult(tr, n_end, k, eta, cen, rad, dens_far, None, None, None, "outer")

    def relerr(a, b):
        return abs(a - b) / abs(b)

    rows, moves = [], 0
    for spec in candidates(case, cen, rad):
        for attempt in range(TRIES):
            b, u, f = moved(spec, attempt, d)
            x = cen[b] + rad[b] * f * u
            assert F.valid(mode, F._x(x)), (case["id"], spec)
            vals, sabs = F.value(mode, x, with_cond=True)
            with mp.workdps(M.DPS):
                tot = mp.fsum(vals)
                row = dict(x=x, value=complex(tot), cond=float(mp.fsum(sabs) / abs(tot)))
                if kind == "ext":
                    row["per_ball"] = [complex(v) for v in vals]
                    row["cond_ball"] = [float(a / abs(v)) for v, a in zip(vals, sabs)]
                    fv, fa = Ff.value("far", x, with_cond=True)
                    ft = mp.fsum(fv)
                    row["far"], row["cond_far"] = complex(ft), float(mp.fsum(fa) / abs(ft))
            if kind == "interior":
                o = interior_fp64(tr, n_end, k, eta, cen, rad, dens, ph["k_interior"], ph["density_ratio"], x, b)
                row["oracle_err"] = relerr(o, row["value"])
            else:
                row["oracle_err"] = relerr(O.uscat(res, x[None])[0], row["value"])
            worst_c, worst_e = row["cond"], row["oracle_err"]
            if kind == "ext":
                ob = O.uscat(res, x[None], per_ball=True)[0]
                row["oracle_err_ball"] = [relerr(ob[i], row["per_ball"][i]) for i in range(B)]
                row["oracle_err_far"] = relerr(O.uscat(resf, x[None], far_field=True)[0], row["far"])
                worst_c = max([worst_c, row["cond_far"]] + row["cond_ball"])
                worst_e = max([worst_e, row["oracle_err_far"]] + row["oracle_err_ball"])
            if worst_c <= COND_MAX and worst_e <= ORACLE_MAX:
                break
            if spec[3] == "fixed":
                raise RuntimeError(f"{case['id']}: the fixed point {spec} has condition {worst_c:.3g}, oracle error {worst_e:.3g}")
            moves += 1
        else:
            raise RuntimeError(f"{case['id']}: no admissible point near {spec} (last: condition {worst_c:.3g}, oracle error {worst_e:.3g})")
        if case["with_grad"]:
            row["grad"] = [complex(v) for v in F.gradient(mode, x)]
        rows.append(row)

    xn = nan_point(case, cen, rad)
    assert not F.valid(mode, F._x(xn))
    P = len(rows) + 1
    assert P % 64 != 0
    nan = complex(np.nan, 0.0)

    def col(name, shape=()):
        return np.array([r[name] for r in rows] + [np.full(shape, nan if name in ("value", "per_ball", "far", "grad") else np.nan)])

    arrays = dict(centers=cen, radii=rad, t=t, x=np.array([r["x"] for r in rows] + [xn]), valid=np.array([True] * len(rows) + [False]),
                  value=col("value"), cond=col("cond"), oracle_err=col("oracle_err"))
    if kind == "ext":
        arrays.update(t_far=t_far, per_ball=col("per_ball", (B,)), cond_ball=col("cond_ball", (B,)), oracle_err_ball=col("oracle_err_ball", (B,)),
                      far=col("far"), cond_far=col("cond_far"), oracle_err_far=col("oracle_err_far"))
        arrays["far"][-1] = complex(mp.fsum(Ff.value("far", xn)))          # the far field has no mask
    if kind == "interior":
        arrays.update(k_interior=np.asarray(ph["k_interior"], dtype=np.complex128), density_ratio=np.asarray(ph["density_ratio"], dtype=np.float64))
    if case["with_grad"]:
        arrays["grad"] = col("grad", (d,)).T.copy()
    kc = complex(k)
    meta = dict(tree=tree, kind={"ext": "outer"}.get(kind, kind), regime=case["regime"], n_end=n_end, k=[kc.real, kc.imag], eta=eta,
                w=f"{FAMILY[tree]}_{n_end}")
    oe = [arrays["oracle_err"][:-1].max()] + ([arrays["oracle_err_ball"][:-1].max(), arrays["oracle_err_far"][:-1].max()] if kind == "ext" else [])
    cd = [arrays["cond"][:-1].max()] + ([arrays["cond_ball"][:-1].max(), arrays["cond_far"][:-1].max()] if kind == "ext" else [])
    print(f"{case['id']:26s} P={P:3d} moved {moves:3d}x  max cond {max(cd):6.1f}  oracle err {max(oe):.1e}  max|dens| {np.abs(dens).max():.1e}  "
          f"|u| {np.abs(arrays['value'][:-1]).min():.1e}..{np.abs(arrays['value'][:-1]).max():.1e}  {time.time() - t0:5.1f}s", flush=True)
    return case["id"], meta, arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=FX.PATH)
    ap.add_argument("--check", action="store_true", help="recompute and compare with the file instead of writing it")
    ap.add_argument("--only", nargs="*", help="case ids (with --check: compare only these; otherwise the file holds only these)")
    ap.add_argument("--jobs", type=int, default=min(8, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    cases = [c for c in case_list() if not args.only or c["id"] in args.only]
    cases.sort(key=lambda c: -O.tree(c["tree"]).n_harm(c["n_end"]) * DIM[c["tree"]])     # the long ones first
    with multiprocessing.get_context("fork").Pool(args.jobs) as pool:
        done = pool.map(build_case, cases, chunksize=1)
    order = [c["id"] for c in case_list() if not args.only or c["id"] in args.only]
    by_id = {cid: (meta, arrays) for cid, meta, arrays in done}
    store = {"cases": np.array(json.dumps(order))}
    for cid in order:
        meta, arrays = by_id[cid]
        store[cid + "/meta"] = np.array(json.dumps(meta))
        store.update({f"{cid}/{name}": a for name, a in arrays.items()})
        family, order_ = meta["w"].rsplit("_", 1)
        store["w/" + meta["w"]] = shared_w(family, int(order_))
    if args.check:
        bad = 0
        with np.load(args.out, allow_pickle=False) as z:
            for name, a in store.items():
                if name == "cases" and args.only:
                    continue                 # (a partial run holds a shorter list)
                if name not in z.files or not np.array_equal(z[name], a, equal_nan=a.dtype.kind in "fc"):
                    print("differs:", name)
                    bad += 1
            if not args.only:                # a full run also owns the file: nothing in it that the generator does not make
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
