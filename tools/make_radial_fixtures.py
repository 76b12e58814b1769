#!/usr/bin/env python3
"""Write tests/golden/radial_full_order.npz: radial functions to the order ceiling (nmax = 320), per-ball tables of every plan and the
factors of high-order 2-D matrices, evaluated by oracle/mp_radial.py at 40 + ceil(2 |Im z| / ln 10) digits.  CPU only.

    python tools/make_radial_fixtures.py            # write the fixture
    python tools/make_radial_fixtures.py --check    # recompute and compare with the committed file, array by array

Every stored value is computed twice, at the working digits and at 20 more, and the two must agree to 1e-30 of the scale the value is
measured against (the value itself, except for z_n below the turning point and the ball tables: J_0 at the fp64 number next to its
first zero is 1e-17, which no 40 digits give to 1e-30 of itself).

WHAT IS STORED.  Flat records (one per stored value), so that the GPU test holds no formula of the error measure:
  rad/<entry>/d<d>/   arg [A]; per record: a (argument), n (order), z, h (expected; the real entry: z, y with h = z + i y),
                      z_ratio = scale(z_n) / |z_n| (float32: >= 1, so no range trouble), weight = max(n + 1, |z|);
                      entry = real (biem_radial) | complex (biem_radial_complex)
  tab/<plan>/         k [4], eta [4], radii [3], alpha, beta [3], alpha_n, beta_n [3, n_end]; per record: s, b, n, gj, gh, blc, the
                      degree-dependent gj_n, gh_n (blc does not depend on the coefficients) and the five ratios scale / |value|, weight
  mat/                the factors of the matrix cases: H/<key> = H_mu(k |t|), E/<key> = e^{i mu phi}, mu = 0 .. 2 n_end - 2, and
                      gj/<key>, gh/<key>, blc/<key> [2, n_end]; "meta" lists the cases
A record is stored only where every value and scale in it lies in [1e-280, 1e280] (z_n(1e-6) at n = 320 is 1e-2690: no fp64 number);
the matrix cases must lie in that range ENTIRELY (the generator stops otherwise: change k, do not mask).

ORDERS.  All of 0 .. nmax for the arguments where the order dependence matters (is_full: a turning point at the top order, Im z < 0; in
d = 2, 3, whose routines every other dimension runs at shifted order), elsewhere every 8th order plus 0 .. 8 and nmax - 8 .. nmax (d >= 5:
every 8th plus 0 .. 2 and nmax - 2 .. nmax).  Tables: n_end = 320 every 16th order, n_end = 48 every 4th, each plus 8 at both ends; the
other plans every order.  The sampling is what keeps the file within the size of full_order_fields.npz.
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "radial_full_order.npz")
LO, HI = 1e-280, 1e280
AGREE = 1e-30
SIZE_LIMIT = os.path.getsize(os.path.join(ROOT, "tests", "golden", "full_order_fields.npz"))

DIMS = {2: 320, 3: 320, 4: 320, 5: 100, 6: 100, 9: 100, 10: 100}            # d -> nmax
REAL_ARGS = [1e-6, 1e-3, 1.0, 2.404825557695773, 3.141592653589793, 300.5, 318.7, 320.0, 1000.0, 4096.0, 16384.0]
FULL_REAL = {318.7, 320.0}
COMPLEX_ARGS = [1.2 + 1.6j, 1.2 + 1.61j, 2.0001 + 1e-9j, 3 + 1e-12j, 1e-3 + 1e-3j, 1e-3 - 1e-3j, 1.5j, 4096 + 0.01j, 16384 + 1e-6j, 16384 + 3j,
                300 + 40j, 150 + 150j, 200 + 300j, 10 + 600j, 20 - 8j, 50 - 3j, 300 - 2j, 300 - 40j]
FULL_COMPLEX = {20 - 8j, 300 - 40j}

PLANS = [("a", "a", 2, 320), ("ba", "ba", 3, 48), ("bba", "bba", 4, 14), ("caa", "caa", 4, 12), ("chain5", "bbba", 5, 8)]   # id, tree, d, n_end
RADII = [1.0, 0.8, 0.37]
ALPHA = [1.0, 0.0, 1.0 + 0.25j]        # soft, hard, Robin: one per ball
BETA = [0.0, 1.0, 0.4 - 0.1j]
ETAS = [1.0, 0.6, 1.0, 0.6]


def plan_ks(d):
    return [0.5, 8.0, 1024.0 if d == 2 else 64.0, 30 + 4j]


def degree_coefficients(n_end):
    """alpha_n, beta_n [3, n_end]: the scalar pairs times short exact patterns in n (no rounding: the inputs are what is stored)."""
    n = np.arange(n_end)
    fa = 1.0 + 0.25 * (n % 5) - 0.5j * (n % 2)
    fb = 1.0 - 0.125 * (n % 3) + 0.25j * (n % 4)
    an = np.array([a * fa for a in ALPHA])
    bn = np.array([b * fb for b in BETA])
    an[1] = 0.5j * (n % 3)             # (the hard ball: a Robin term in two of three degrees)
    bn[0] = 0.25 * (n % 2)             # (the soft ball likewise)
    return an, bn


MATRIX_CASES = [                        # id, n_end, k, centre of ball 1 (ball 0 at the origin); radii 1.0, 0.8
    ("n152-k20-x", 152, 20.0, (4.0, 0.0)),          # (k = 8 would put the entries of n = n' = 151, mu = 0 at 1e-357: j_151(8) j_151(6.4))
    ("n152-k20-oblique", 152, 20.0, (3.1, -2.7)),
    ("n152-k1024-oblique", 152, 1024.0, (3.1, -2.7)),
    ("n200-k40-y", 200, 40.0, (0.0, 4.0)),          # (k = 8 would put H_398(32) at 1e383 as well)
    ("n400-k256-oblique", 400, 256.0, (3.1, -2.7)),
]
MATRIX_RADII = [1.0, 0.8]


def sampled_orders(nmax, full, edge=8, step=8):
    if full:
        return list(range(nmax + 1))
    return sorted(set(range(0, edge + 1)) | set(range(0, nmax + 1, step)) | set(range(nmax - edge, nmax + 1)))


def is_full(entry, d, z):
    """Every order: d = 2, 3 (the two routines; the other dimensions are these at shifted order) at the turning-point arguments and at
    Im z < 0, and the odd d >= 5 at 20 - 8i, whose defect before the fix of bessel_jh_sph_c lay below n = 100."""
    if d in (2, 3):
        return z in (FULL_REAL if entry == "real" else FULL_COMPLEX)
    return entry == "complex" and d in (5, 9) and z == 20 - 8j


def _agree(a, b, what, scale=None):
    """|a - b| <= 1e-30 of the scale the value is measured against (default: the value itself)."""
    import mpmath as mp
    with mp.workdps(60):
        err = abs(a - b) / (mp.mpf(scale) if scale else abs(b))         # (a scale below the fp64 range arrives as 0: such a record is not stored)
        if not err <= AGREE:
            raise RuntimeError(f"{what}: {mp.nstr(err, 3)} between the working digits and 20 more")


def _in_range(*vals):
    return all(LO <= abs(v) <= HI for v in vals)


# --------------------------------------------------------------------------------------
# tasks (each runs in a worker)
# --------------------------------------------------------------------------------------
def radial_task(task):
    from oracle import mp_radial as R

    entry, d, ai, z = task
    nmax = DIMS[d]
    full = is_full(entry, d, z)
    j, h = R.radial(nmax, d, z)
    j2, h2 = R.radial(nmax, d, z, extra=20)
    sj, _, w = R.radial_scales(nmax, d, z, j, h)
    rec = []
    for n in sampled_orders(nmax, full, 8 if d <= 4 else 2):
        _agree(j[n], j2[n], f"z_{n}^({d})({z})", sj[n])
        _agree(h[n], h2[n], f"h_{n}^({d})({z})")
        zj, zh = complex(j[n]), complex(h[n])
        if _in_range(zj, zh, sj[n]) and (entry != "real" or _in_range(zh.imag)):
            rec.append((ai, n, zj, zh, sj[n] / abs(zj), w[n]))
    return ("rad", entry, d, ai), rec


def table_task(task):
    from oracle import mp_radial as R

    pid, d, n_end, s, b = task
    k, eta, rho = plan_ks(d)[s], ETAS[s], RADII[b]
    an, bn = degree_coefficients(n_end)
    t = R.ball_tables(d, n_end, k, eta, rho, ALPHA[b], BETA[b])
    t2 = R.ball_tables(d, n_end, k, eta, rho, ALPHA[b], BETA[b], extra=20)
    tn = R.ball_tables(d, n_end, k, eta, rho, an[b], bn[b])
    tn2 = R.ball_tables(d, n_end, k, eta, rho, an[b], bn[b], extra=20)
    rec = []
    for n in table_orders(n_end):
        vals, ratios = [], []
        for tt, tt2, names in ((t, t2, ("gj", "gh", "blc")), (tn, tn2, ("gj", "gh"))):
            for nm in names:
                _agree(tt[nm][n], tt2[nm][n], f"{pid} {nm}[{s},{b},{n}]", tt[nm + "_scale"][n])
                v = complex(tt[nm][n])
                vals.append(v)
                ratios.append(tt[nm + "_scale"][n] / abs(v) if v != 0 else np.inf)
        scales = [r * abs(v) for r, v in zip(ratios, vals)]
        if _in_range(*vals) and _in_range(*scales):
            rec.append((s, b, n, vals, ratios, t["weight"][n]))
    return ("tab", pid, s, b), rec


def table_orders(n_end):
    if n_end > 48:
        return sampled_orders(n_end - 1, False, 8, 16)
    return sampled_orders(n_end - 1, False, 8, 4) if n_end > 16 else list(range(n_end))


def hankel_task(task):
    from oracle import mp_radial as R

    key, n_end, k, t = task
    hk, e = R.translation_2d_factors(n_end, k, t)
    hk2, e2 = R.translation_2d_factors(n_end, k, t, extra=20)
    for mu in range(2 * n_end - 1):
        _agree(hk[mu], hk2[mu], f"H_{mu} {key}")
        _agree(e[mu], e2[mu], f"E_{mu} {key}")
    return ("mat", key), (np.array([complex(v) for v in hk]), np.array([complex(v) for v in e]))


def matrix_table_task(task):
    from oracle import mp_radial as R

    key, n_end, k = task
    out = {nm: np.zeros((2, n_end), dtype=np.complex128) for nm in ("gj", "gh", "blc")}
    for b, rho in enumerate(MATRIX_RADII):
        t = R.ball_tables(2, n_end, k, 1.0, rho, 1.0, 0.0)
        t2 = R.ball_tables(2, n_end, k, 1.0, rho, 1.0, 0.0, extra=20)
        for nm in out:
            for n in range(n_end):
                _agree(t[nm][n], t2[nm][n], f"{key} {nm}[{b},{n}]", t[nm + "_scale"][n])
            out[nm][b] = [complex(v) for v in t[nm]]
    return ("mtab", key), out


def t_key(c1):
    return f"t_{c1[0]:g}_{c1[1]:g}"


def build(jobs):
    tasks = []
    for d in DIMS:
        tasks += [(radial_task, ("real", d, i, z)) for i, z in enumerate(REAL_ARGS)]
        tasks += [(radial_task, ("complex", d, i, z)) for i, z in enumerate(COMPLEX_ARGS)]
    for pid, _, d, n_end in PLANS:
        tasks += [(table_task, (pid, d, n_end, s, b)) for s in range(4) for b in range(3)]
    hk, tb = {}, {}
    for cid, n_end, k, c1 in MATRIX_CASES:
        key = f"k{k:g}_{t_key(c1)}"
        hk[key] = max(hk.get(key, (0,))[0], n_end), k, tuple(-v for v in c1)     # t = c_0 - c_1
        kt = f"k{k:g}"
        tb[kt] = max(tb.get(kt, (0,))[0], n_end), k
    tasks += [(hankel_task, (key, n, k, t)) for key, (n, k, t) in hk.items()]
    tasks += [(matrix_table_task, (key, n, k)) for key, (n, k) in tb.items()]
    with multiprocessing.get_context("fork").Pool(jobs) as pool:
        done = dict(pool.map(_run, tasks, chunksize=1))

    store = {}
    for entry, args in (("real", REAL_ARGS), ("complex", COMPLEX_ARGS)):
        for d in DIMS:
            rec = [r for i in range(len(args)) for r in done["rad", entry, d, i]]
            p = f"rad/{entry}/d{d}/"
            store[p + "arg"] = np.array(args, dtype=np.float64 if entry == "real" else np.complex128)
            store[p + "a"] = np.array([r[0] for r in rec], dtype=np.uint8)
            store[p + "n"] = np.array([r[1] for r in rec], dtype=np.uint16)
            if entry == "complex":
                store[p + "z"] = np.array([r[2] for r in rec], dtype=np.complex128)
                store[p + "h"] = np.array([r[3] for r in rec], dtype=np.complex128)
            else:                        # h = z + i y (Re h is z only to 40 digits of |h|: not z where |y| is 1e70 times larger)
                store[p + "z"] = np.array([r[2].real for r in rec], dtype=np.float64)
                store[p + "y"] = np.array([r[3].imag for r in rec], dtype=np.float64)
            store[p + "z_ratio"] = np.array([r[4] for r in rec], dtype=np.float32)
            store[p + "weight"] = np.array([r[5] for r in rec], dtype=np.float32)
    for pid, _, d, n_end in PLANS:
        rec = [r for s in range(4) for b in range(3) for r in done["tab", pid, s, b]]
        p = f"tab/{pid}/"
        an, bn = degree_coefficients(n_end)
        store.update({p + "k": np.array(plan_ks(d), dtype=np.complex128), p + "eta": np.array(ETAS), p + "radii": np.array(RADII),
                      p + "alpha": np.array(ALPHA, dtype=np.complex128), p + "beta": np.array(BETA, dtype=np.complex128),
                      p + "alpha_n": an.astype(np.complex128), p + "beta_n": bn.astype(np.complex128)})
        store[p + "s"] = np.array([r[0] for r in rec], dtype=np.uint8)
        store[p + "b"] = np.array([r[1] for r in rec], dtype=np.uint8)
        store[p + "n"] = np.array([r[2] for r in rec], dtype=np.uint16)
        for i, nm in enumerate(("gj", "gh", "blc", "gj_n", "gh_n")):
            store[p + nm] = np.array([r[3][i] for r in rec], dtype=np.complex128)
            store[p + nm + "_ratio"] = np.array([r[4][i] for r in rec], dtype=np.float32)
        store[p + "weight"] = np.array([r[5] for r in rec], dtype=np.float32)
    cases = []
    for cid, n_end, k, c1 in MATRIX_CASES:
        hkey, kt = f"k{k:g}_{t_key(c1)}", f"k{k:g}"
        cases.append(dict(id=cid, n_end=n_end, k=k, centers=[[0.0, 0.0], list(c1)], radii=MATRIX_RADII, H="mat/H/" + hkey, E="mat/E/" + t_key(c1),
                          tab="mat/tab/" + kt))
        H, E = done["mat", hkey]
        store["mat/H/" + hkey] = H
        if len(E) > len(store.get("mat/E/" + t_key(c1), ())):
            store["mat/E/" + t_key(c1)] = E
        for nm, a in done["mtab", kt].items():
            store[f"mat/tab/{kt}/{nm}"] = a
        # the whole case must be fp64 numbers well inside the range: every factor and the extreme entries
        N = 2 * n_end - 1
        tabs = {nm: done["mtab", kt][nm][:, :n_end] for nm in ("gj", "gh", "blc")}
        for a in (H[:N], E[:N], *tabs.values()):
            if not ((np.abs(a) >= LO) & (np.abs(a) <= HI)).all():
                raise RuntimeError(f"{cid}: a factor leaves [1e-280, 1e280]: change k")
        m = np.abs(np.arange(n_end)[:, None] - np.arange(n_end)[None, :])
        for b in range(2):
            for sgn in (m, np.arange(n_end)[:, None] + np.arange(n_end)[None, :]):            # |mu| for like and unlike signs of m, m'
                ent = np.abs(H)[sgn] * np.abs(tabs["gj"][b])[:, None] * np.abs(tabs["blc"][1 - b])[None, :]
                if not ((ent >= LO) & (ent <= HI)).all():
                    raise RuntimeError(f"{cid}: an entry leaves [1e-280, 1e280] ({ent.min():.1e} .. {ent.max():.1e}): change k")
    store["meta"] = np.array(json.dumps(dict(dims={str(d): n for d, n in DIMS.items()}, plans=[dict(id=p, tree=t, d=d, n_end=n) for p, t, d, n in PLANS],
                                             matrix=cases)))
    return store


def _run(task):
    fn, arg = task
    return fn(arg)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=PATH)
    ap.add_argument("--check", action="store_true", help="recompute and compare with the file instead of writing it")
    ap.add_argument("--jobs", type=int, default=min(8, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    store = build(args.jobs)
    if args.check:
        bad = 0
        with np.load(args.out, allow_pickle=False) as z:
            for name, a in store.items():
                if name not in z.files or z[name].dtype != a.dtype or not np.array_equal(z[name], a):
                    print("differs:", name)
                    bad += 1
            for name in sorted(set(z.files) - set(store)):
                print("only in the file:", name)
                bad += 1
        size = os.path.getsize(args.out)
        print(f"{len(store)} arrays compared, {bad} differ; {size} bytes (limit {SIZE_LIMIT})")
        return 1 if bad or size > SIZE_LIMIT else 0
    np.savez_compressed(args.out, **store)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out}: {size} bytes (limit {SIZE_LIMIT}), {len(store)} arrays")
    return 0 if size <= SIZE_LIMIT else 1


if __name__ == "__main__":
    sys.exit(main())
