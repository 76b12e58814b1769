#!/usr/bin/env python3
"""Write tests/golden/full_order_rhs_a.npz and full_order_rhs.npz: harmonics, closed-form right-hand sides and power AT the order ceilings.

    python tools/make_full_order_rhs_fixtures.py            # write both files
    python tools/make_full_order_rhs_fixtures.py --check    # recompute and compare with the committed files, array by array

Cases: a 320, ba 48, bba 14, caa 12 with two balls and two systems (one real k, one complex), the chains bbba 8, bbbba 5
and d = 10 at 3 with one ball; five sources per case at |t| / rho in {1.02, 1.5, 4} along a generic direction, the first axis, the last
axis, 1e-3 off the pole and with the last coordinate exactly 0; the same five directions as plane waves; 70 sources around one ball on
a 320 and ba 48 (7 distances x 10 azimuths on the circle of radius 25: exact coordinates, shared factors); the edge a 150, k rho = 1.3;
and per tree one power case of a lossy and a lossless ball with a term of visible size in every degree.

Everything is computed by oracle/mp_rhs.py at 40 digits (more for complex k) from exactly the fp64 inputs stored, and a second time at
20 more digits: the two must round to the same fp64 numbers up to one unit in the last place.  The generator stops if a gj_n, an h_n or
a scale leaves [1e-280, 1e280] (the edge case: [1e-300, 1e300]), or if sum |terms| / |sum| of a P_ext exceeds 100.
"""
import argparse
import json
import math
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import full_order_rhs_fixture as FX  # noqa: E402
from oracle import mp_radial as MR  # noqa: E402
from oracle import mp_rhs as R  # noqa: E402
from oracle.mp_field import radial_h  # noqa: E402

RANGE = (1e-280, 1e280)
EDGE_RANGE = (1e-300, 1e300)
COND_MAX = 100.0
ROBIN = (1.0 + 0.5j, 0.3 - 0.2j)
SOFT = (1.0 + 0.0j, 0.0j)
#         n_end  B  k rho of the two balls (ball 0 has radius 1, so k = the first)   centre of ball 0 (multiples of 1/16)
SPEC = {
    "a": (320, 2, (60.0, 250.0), [64.0, -48.0]),                       # |k| |c| = 4800: the plane-wave weight
    "ba": (48, 2, (30.0, 17.0), [1.5, -0.75, 2.25]),
    "bba": (14, 2, (9.0, 5.0), [0.5, 1.25, -0.75, 0.375]),
    "caa": (12, 2, (8.0, 4.5), [-0.625, 0.75, 1.125, -0.25]),
    "bbba": (8, 1, (5.0, 3.0), [0.5, -0.25, 0.75, 0.125, -0.375]),
    "bbbba": (5, 1, (3.5, 2.0), [0.25, 0.5, -0.375, 0.125, 0.625, -0.5]),
    "bbbbbbbba": (3, 1, (2.5, 1.5), [0.25, -0.125, 0.375, 0.5, -0.25, 0.125, 0.0625, -0.3125, 0.1875, 0.4375]),
}
GENERIC = np.array([0.3, -0.8, 0.45, 0.6, -0.2, 0.35, 0.5, -0.4, 0.25, 0.15])
OTHER = np.array([-0.55, 0.4, 0.3, -0.45, 0.35, 0.2, -0.3, 0.25, 0.4, -0.1])
RATIOS = (1.02, 1.5, 4.0, 1.5, 1.02)
KINDS = ("generic", "first axis", "last axis", "1e-3 off the pole", "last coordinate 0")
GRID = 2.0 ** 40
# the circle of radius 25 through integer points: azimuth r % 10 of the 70 sources
CIRCLE = np.array([(25, 0), (24, 7), (20, 15), (15, 20), (7, 24), (0, 25), (-7, 24), (-15, 20), (-20, -15), (7, -24)], dtype=np.float64)
WIDE_RATIOS = (1.02, 1.5, 4.0, 1.1, 2.0, 3.0, 1.25)
WIDE_POLAR = (10.0, -30.0, 60.0, -5.0, 25.0, 0.0, -100.0)              # ba: first coordinate over the circle's unit (25 = 45 degrees)


def kind_dirs(d):
    """The five directions (not normalised)."""
    g = GENERIC[:d].copy()
    first, last, near, flat = np.zeros(d), np.zeros(d), np.zeros(d), OTHER[:d].copy()
    first[0], last[-1] = 1.0, 1.0
    near[0] = 1.0
    near[1:] = 1e-3 * np.array([0.8, -0.6, 0.5, 0.4, -0.3, 0.2, 0.35, -0.25, 0.15])[:d - 1]
    flat[-1] = 0.0
    if d == 2:
        flat[0] = -1.0                                                  # (2-D: the negative first axis, azimuth pi)
    return np.stack([g, first, last, near, flat])


def quant(v):
    return np.round(np.asarray(v) * GRID) / GRID


def mpv(v):
    return [mp.mpf(float(x)) for x in v]


def in_range(what, vals, rng):
    vals = np.asarray([float(abs(v)) for v in vals])
    lo, hi = vals.min(), vals.max()
    if not (rng[0] <= lo and hi <= rng[1]):
        raise SystemExit(f"{what}: {lo:.3e} .. {hi:.3e} leaves [{rng[0]:g}, {rng[1]:g}]")
    return lo, hi


def factors(tree, st, vecs):
    """amp [P, U], es [A][P, n_end] rounded from the working precision, at the directions vecs [P, d] (exact fp64 numbers)."""
    naz = st.m.shape[1]
    first = {}
    for h in range(st.H):
        if (st.m[h] >= 0).all():
            first.setdefault(int(st.aidx[h]), h)
    amp = np.zeros((len(vecs), len(st.keys)))
    es = [np.zeros((len(vecs), st.n_end), dtype=np.complex128) for _ in range(naz)]
    for p, v in enumerate(vecs):
        u = mpv(v)
        Y = R.tree_harmonics(tree, st.n_end, u)
        pw = R.azimuth_powers(tree, st.n_end, u)
        for a in range(naz):
            es[a][p] = [complex(z) for z in pw[a]]
        for key, h in first.items():
            z = Y[h]
            for a in range(naz):
                z = z * mp.conj(pw[a][int(st.m[h, a])])
            assert abs(mp.im(z)) <= mp.mpf(10) ** (-mp.mp.dps + 8) * (abs(z) + 1), (tree, key, z)
            amp[p, key] = float(mp.re(z))
    return amp, es


def radial_rows(d, n_end, k, gj, dist, rng, what):
    """G [n_end] complex128 and the figures of one (system, source, ball)."""
    G, h = R.point_source_G(d, n_end, k, gj, dist)
    in_range(what + " h_n", h, rng)
    return np.array([complex(v) for v in G])


def gj_table(d, n_end, k, rho, pair):
    t = MR.ball_tables(d, n_end, k, 1.0, rho, pair[0], pair[1])
    return np.array([complex(v) for v in t["gj"]])


def full_table(d, n_end, k, rho, alpha, beta):
    t = MR.ball_tables(d, n_end, k, 1.0, rho, alpha, beta)
    return np.array([[complex(v) for v in t[row]] for row in ("gj", "gh", "blc")])


def power_case(tree, st, k, radii, log):
    """The power records of one tree: exponents and rotations that give every degree a term of visible size and (mostly) one sign."""
    d, n_end = st.d, st.n_end
    alpha, beta = np.array([ROBIN[0], SOFT[0]]), np.array([ROBIN[1], SOFT[1]])          # ball 0 lossy, ball 1 lossless
    out = dict(palpha=alpha, pbeta=beta)
    tab = np.stack([full_table(d, n_end, k, radii[b], complex(alpha[b]), complex(beta[b])) for b in range(2)])
    exps = np.zeros((2, 4, n_end), dtype=np.int16)
    for b in range(2):
        with mp.workdps(mp.mp.dps):
            x = mp.mpf(float(k)) * mp.mpf(float(radii[b]))
            h = radial_h(n_end, d, x)
            for n in range(n_end):
                khp = mp.mpf(float(k)) * (n / x * h[n] - h[n + 1])
                blc = mp.mpc(tab[b, 2, n].real, tab[b, 2, n].imag)
                deg_of = lambda z: float(mp.arg(z)) * 180.0 / math.pi
                exps[b, 0, n] = -int(round(float(mp.log(abs(blc * h[n]), 2))))
                exps[b, 1, n] = int(round((90.0 - deg_of(blc * khp)) / 90.0)) % 4
                exps[b, 2, n] = int(round(float(mp.log(abs(khp / h[n]), 2))))
                exps[b, 3, n] = int(round((90.0 + 90.0 * exps[b, 1, n] + deg_of(blc * h[n])) / 90.0)) % 4
    dens, pu, pv = FX.power_inputs(st.deg, exps)
    out.update(ptab=tab, pexps=exps)
    variants = [("", tab, np.repeat(alpha[:, None], n_end, 1), np.repeat(beta[:, None], n_end, 1))]
    if tree in ("a", "ba"):
        an, bn = FX.degree_pair(alpha, beta, n_end)
        variants.append(("_n", np.stack([full_table(d, n_end, k, radii[b], list(an[b]), list(bn[b])) for b in range(2)]), an, bn))
        out["ptab_n"] = variants[1][1]
    for suffix, tb, an, bn in variants:
        want = np.zeros((FX.POWER_NRHS, 2, 2))
        scale = np.zeros((FX.POWER_NRHS, 2, 2))
        cond = np.zeros((FX.POWER_NRHS, 2))
        for b in range(2):
            in_range(f"{tree} power{suffix} gj ball {b}", tb[b, 0], RANGE)
            in_range(f"{tree} power{suffix} blc ball {b}", tb[b, 2], RANGE)
            for r in range(FX.POWER_NRHS):
                pe, pa, c, se, sa = R.power(d, n_end, k, radii[b], an[b], bn[b], tb[b], dens[r, b], pu[r, b], pv[r, b], st.deg)
                want[r, b], scale[r, b], cond[r, b] = (float(pe), float(pa)), (float(se), float(sa)), float(c)
                in_range(f"{tree} power{suffix} sum |terms of P_ext|", [se], RANGE)
                if sa != 0:
                    in_range(f"{tree} power{suffix} sum |terms of P_abs|", [sa], RANGE)
                if c > COND_MAX:
                    raise SystemExit(f"{tree} power{suffix} ball {b} rhs {r}: sum |terms| / |sum| = {float(c):.1f} > {COND_MAX}")
        assert (want[:, 1, 1] == 0.0).all() and (want[:, 0, 1] != 0.0).all()
        out.update({"pwant" + suffix: want, "pscale" + suffix: scale, "pcond" + suffix: cond})
        log(f"  power{suffix}: k rho {float(k) * radii[0]:g} / {float(k) * radii[1]:g}; P_ext {want[:, :, 0].ravel()}, sum |terms| / |sum| <= "
            f"{cond.max():.2f}; P_abs {want[:, :, 1].ravel()}; exponents of the density {exps[:, 0].min()} .. {exps[:, 0].max()}")
    return out


def main_case(tree, log):
    n_end, B, krho, c0 = SPEC[tree]
    st = FX.structure(tree, n_end)
    d = st.d
    radii = np.array([1.0, krho[1] / krho[0]])
    k = np.array([krho[0], 0.875 * krho[0] + 0.125j])
    nb = len(k)
    sep = math.ceil(6.0 * radii.max() + 2.0)
    off = np.array([0.75, 0.5, 0.25, 0.25, -0.25, 0.125, 0.125, -0.125, 0.0625, 0.0625])[:d] * sep / 0.75
    centers = np.stack([np.array(c0), quant(np.array(c0) + np.round(off * 16.0) / 16.0)])[:max(B, 1)]
    kd = kind_dirs(d)
    unit = kd / np.linalg.norm(kd, axis=1, keepdims=True)
    src = np.stack([centers[r % B] + quant(RATIOS[r] * radii[r % B] * unit[r]) for r in range(5)])
    T = src[:, None, :] - centers[None, :, :]                                                     # [5, B, d], exact
    for r in range(5):
        for b in range(B):
            exact = [mp.mpf(float(s)) - mp.mpf(float(c)) for s, c in zip(src[r], centers[b])]
            assert all(mp.mpf(float(t)) == e for t, e in zip(T[r, b], exact)), "src - center is not exact in fp64"
            assert np.linalg.norm(T[r, b]) >= 1.01 * radii[b], (tree, r, b)
    dirs = unit.copy()
    hdirs = np.concatenate([T.reshape(5 * B, d), dirs])
    amp, es = factors(tree, st, hdirs)
    gj = np.stack([np.stack([gj_table(d, n_end, complex(k[s]) if k[s].imag else float(k[s].real), radii[b], ROBIN) for b in range(B)])
                   for s in range(nb)])
    lo, hi = in_range(f"{tree} gj", gj.ravel(), RANGE)
    log(f"{tree} n_end {n_end}: H {st.H}, B {B}, k {list(k)}, radii {list(radii[:B])}; |gj_n| {lo:.2e} .. {hi:.2e}")
    G = np.zeros((nb, 5, B, n_end), dtype=np.complex128)
    pf = np.zeros((nb, 5, B), dtype=np.complex128)
    for s in range(nb):
        ks = complex(k[s]) if k[s].imag else float(k[s].real)
        for r in range(5):
            for b in range(B):
                dist = mp.sqrt(mp.fsum(mp.mpf(float(t)) ** 2 for t in T[r, b]))
                G[s, r, b] = radial_rows(d, n_end, ks, gj[s, b], dist, RANGE, f"{tree} s{s} r{r} b{b}")
                with mp.workdps(max(mp.mp.dps, MR.digits(complex(ks) * float(np.linalg.norm(centers[b]))))):
                    pf[s, r, b] = complex(R.plane_wave_factor(d, ks, dirs[r], centers[b]))
    scale = np.abs(G) * st.ynorm[None, None, None, :]
    lo, hi = in_range(f"{tree} point-source scale", scale.ravel(), RANGE)
    in_range(f"{tree} plane-wave scale", (np.abs(pf)[..., None] * np.abs(gj)[:, None] * st.ynorm).ravel(), RANGE)
    dist = np.linalg.norm(T, axis=-1)
    log(f"  sources: |t| / rho {np.round(dist / radii[None, :B], 3).tolist()}; point-source scale {lo:.2e} .. {hi:.2e}; |k| |t| <= "
        f"{(np.abs(k)[:, None, None] * dist[None]).max():.0f}; Im k |t| <= {(k.imag[:, None, None] * dist[None]).max():.2f}; |k| |c| <= "
        f"{(np.abs(k)[:, None] * np.linalg.norm(centers, axis=-1)[None]).max():.0f}")
    rec = dict(k=k, centers=centers, radii=radii, src=src, dirs=dirs, gj=gj, hdirs=hdirs, amp=amp, e1=es[0], G=G, pf=pf)
    if len(es) > 1:
        rec["e2"] = es[1]
    rec.update(power_case(tree, st, float(k[0].real), radii, log))
    meta = dict(kind="main", tree=tree, n_end=n_end, d=d, B=B, nb=nb, kinds=list(KINDS))
    return f"{tree}-{n_end}", meta, rec


def wide_case(tree, main, log):
    """70 sources around ball 0 of the main case, system 0: 7 groups (distance, and on ba the polar angle) x 10 azimuths."""
    n_end = SPEC[tree][0]
    st = FX.structure(tree, n_end)
    d, c0, rho, k = st.d, main["centers"][0], main["radii"][0], float(main["k"][0].real)
    vec = np.zeros((FX.WIDE_GROUPS, FX.WIDE_AZIMUTHS, d))
    for g in range(FX.WIDE_GROUPS):
        length = math.hypot(WIDE_POLAR[g], 25.0) if d == 3 else 25.0
        q = round(WIDE_RATIOS[g] * rho / length * 2 ** 20) / 2 ** 20
        for a in range(FX.WIDE_AZIMUTHS):
            vec[g, a, d - 2:] = q * CIRCLE[a]
            if d == 3:
                vec[g, a, 0] = q * WIDE_POLAR[g]
    r = np.arange(FX.WIDE_NRHS)
    src = c0[None, :] + vec[r % FX.WIDE_GROUPS, r % FX.WIDE_AZIMUTHS]
    assert np.array_equal(src - c0[None, :], vec[r % FX.WIDE_GROUPS, r % FX.WIDE_AZIMUTHS])
    assert len({tuple(v) for v in src}) == FX.WIDE_NRHS
    amp_g, _ = factors(tree, st, vec[:, 0])                           # the amplitudes depend on the group alone ...
    amp_check, es_a = factors(tree, st, vec[0])                       # ... and the phases on the azimuth alone
    assert np.array_equal(amp_check, np.repeat(amp_g[:1], FX.WIDE_AZIMUTHS, 0))
    G = np.zeros((FX.WIDE_GROUPS, n_end), dtype=np.complex128)
    for g in range(FX.WIDE_GROUPS):
        dist = mp.sqrt(mp.fsum(mp.mpf(float(t)) ** 2 for t in vec[g, 0]))
        G[g] = radial_rows(d, n_end, k, main["gj"][0, 0], dist, RANGE, f"{tree} wide g{g}")
    lo, hi = in_range(f"{tree} wide scale", (np.abs(G) * st.ynorm).ravel(), RANGE)
    log(f"{tree} n_end {n_end} wide: |t| / rho {np.round(np.linalg.norm(vec[:, 0], axis=-1) / rho, 3).tolist()}; scale {lo:.2e} .. {hi:.2e}")
    return f"{tree}-{n_end}-wide", dict(kind="wide", tree=tree, n_end=n_end, d=d, B=1, nb=1, main=f"{tree}-{n_end}"), dict(src=src, G=G, amp=amp_g, e1=es_a[0])


def edge_case(log):
    """a, n_end 150, k rho = 1.3, the soft disc: gj_n = j_n falls to 4e-289 and h_149 rises to 3e284 - normal fp64 numbers, outside the
    [1e-280, 1e280] of every other case, which is what makes this the edge."""
    tree, n_end = "a", 150
    st = FX.structure(tree, n_end)
    k, radii, centers = np.array([1.3 + 0j]), np.array([1.0]), np.array([[0.5, -0.25]])
    kd = kind_dirs(2)[[0, 2, 3]]
    unit = kd / np.linalg.norm(kd, axis=1, keepdims=True)
    src = np.stack([centers[0] + quant(RATIOS[r] * unit[r]) for r in range(3)])
    T = src - centers
    gj = gj_table(2, n_end, 1.3, 1.0, SOFT)[None, None]
    lo, hi = in_range("edge gj", gj.ravel(), EDGE_RANGE)
    amp, es = factors(tree, st, T)
    G = np.zeros((1, 3, 1, n_end), dtype=np.complex128)
    for r in range(3):
        dist = mp.sqrt(mp.fsum(mp.mpf(float(t)) ** 2 for t in T[r]))
        G[0, r, 0] = radial_rows(2, n_end, 1.3, gj[0, 0], dist, EDGE_RANGE, f"edge r{r}")
    slo, shi = in_range("edge scale", (np.abs(G) * st.ynorm).ravel(), EDGE_RANGE)
    log(f"a n_end 150 edge: |gj_n| {lo:.2e} .. {hi:.2e}; scale {slo:.2e} .. {shi:.2e}")
    meta = dict(kind="edge", tree=tree, n_end=n_end, d=2, B=1, nb=1)
    return "a-150-edge", meta, dict(k=k, centers=centers, radii=radii, src=src, gj=gj, hdirs=T, amp=amp, e1=es[0], G=G)


def build(extra, log):
    """{path: {key: array}} at 40 + extra digits."""
    stores = {p: {} for p in FX.PATHS}
    order = {p: [] for p in FX.PATHS}

    def put(path, cid, meta, rec):
        order[path].append(cid)
        stores[path][cid + "/meta"] = np.array(json.dumps(meta))
        for key, v in rec.items():
            stores[path][f"{cid}/{key}"] = np.asarray(v)

    with mp.workdps(MR.BASE_DPS + extra):
        for tree in SPEC:
            path = FX.PATHS[0] if tree == "a" else FX.PATHS[1]
            cid, meta, rec = main_case(tree, log)
            put(path, cid, meta, rec)
            if tree in ("a", "ba"):
                put(path, *wide_case(tree, rec, log))
        put(FX.PATHS[0], *edge_case(log))
    for p in FX.PATHS:
        stores[p]["cases"] = np.array(json.dumps(order[p]))
    return stores


def compare(a, b, ulps, what):
    """Arrays of the two stores agree to `ulps` units in the last place of their modulus (strings and integers exactly)."""
    bad = 0
    for path in a:
        if set(a[path]) != set(b[path]):
            print(f"{what}: {os.path.basename(path)} holds other keys: {sorted(set(a[path]) ^ set(b[path]))}")
            bad += 1
            continue
        for key, x in a[path].items():
            y = np.asarray(b[path][key])
            if x.dtype.kind in "USiu" or ulps == 0:
                same = x.shape == y.shape and np.array_equal(x, y)
            else:
                same = x.shape == y.shape and bool((np.abs(x - y) <= ulps * 2.0 ** -52 * np.abs(x)).all())
            if not same:
                print(f"{what}: {os.path.basename(path)} {key} differs")
                bad += 1
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed files instead of writing them")
    ap.add_argument("--no-second", action="store_true", help="skip the second computation at 20 more digits")
    args = ap.parse_args()
    stores = build(0, print)
    if not args.no_second:
        bad = compare(stores, build(20, lambda *_: None), 1, "40 against 60 digits")
        if bad:
            return 1
        print("the computation at 60 digits rounds to the same numbers (one unit in the last place at most)")
    if args.check:
        bad = 0
        for p in FX.PATHS:
            with np.load(p, allow_pickle=False) as z:
                bad += compare({p: stores[p]}, {p: {key: z[key] for key in z.files}}, 0, "--check")
        print("the committed files are reproduced" if not bad else f"{bad} arrays differ")
        return 1 if bad else 0
    for p in FX.PATHS:
        np.savez_compressed(p, **stores[p])
        size = os.path.getsize(p)
        print(f"wrote {p}: {size} bytes, {len(json.loads(str(stores[p]['cases'])))} cases")
        if size >= 500_000:
            raise SystemExit(f"{p} is {size} bytes: every fixture stays below 500 KB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
