#!/usr/bin/env python3
"""Polar triple integrals of the 4-D trees at 40 digits -> tests/golden/polar4_integrals.npz (offline, needs mpmath).

    python tools/make_polar4_fixtures.py              # writes the fixture, prints one summary line per case
    python tools/make_polar4_fixtures.py --probe-caa  # the long-double probe that chose the two high caa orders

bba:  A4 = int_0^pi Abar_{q'l'} Abar_{ql} Abar_{q''l''} sin^2 dt,  Abar_{ql} = sin^l Gbar_{q-l}^{(l+1)}(cos t)
caa:  I3 = int_0^{pi/2} cbar' cbar cbar'' sin cos dt,  cbar_{n,a,b} = cos^a sin^b Pbar_k^{(b,a)}(cos 2t), a'' = |m1' - m1|, b'' = |m2' - m2|

Each integrand is a polynomial times the weight of a Gauss rule (bba: sqrt(1 - x^2), x = cos t; caa: 1 in x = cos 2t), so the rule taken
in 40-digit arithmetic with enough nodes is exact.  An integral counts as vanishing when its modulus is below 1e-30.  No selection rule
is assumed: the third label runs over every label of degree < 2 n_end - 1 (caa: every degree with the azimuthal orders of the four
sign choices of (m1, m1', m2, m2')).  Only the labels with an odd l + l' + l'' are left out of bba: there the other factor of the
coefficient is the integral over S^2 of a function odd under the reflection of the polar axis - the azimuthal delta's own companion,
not a rule of this integral - and A4 never reaches a coefficient.

What is stored per case "<tree>_<n_end>": `lab` (int8; bba (q', l', q, l, q'', l''), caa (q', a', b', q, a, b, q'', a'', b'')), `val`
(rounded to float64), `zero` (the vanish flag), `pairs` (the pairs of the top block, for the tests that draw entries from them).

The top block (both labels in the top two degrees, every third label) holds 2e5 integrals that do not vanish at bba n_end 24 - 1.6 MB
of float64 for that case alone - so a fixture no larger than the largest one under tests/golden/ cannot hold the blocks whole.  Kept
per case are N_PAIRS pairs of the block with every third label: the half whose smallest non-vanishing integral is smallest (a float64
probe with the 2 n_end- and the 3 n_end + 3-node rule ranks them; an integral counts there when the two agree to 1 %), which is where a
magnitude cut goes wrong first (counted are the labels inside the triangle of the degrees that stand 100 times above the largest
modulus the same pair shows outside it, where every integral vanishes), and a seeded random half; plus N_RANDOM seeded random triples over all degrees.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), os.path.join(HERE, "..", "tests")]

import polar4_yardstick as PY   # noqa: E402   (the float64 twin: ranks the pairs, nothing of it is stored)

DIGITS = 40
VANISH = 1e-30
BBA_ORDERS = (15, 18, 22, 24)
# caa: 13 | 14 is where the general fill moves its pair table from LDS to global memory (build_entry_chunks in plan_fill.cpp: the
# budget 150 KiB - 16 (H2 + 2 H) - 4164 falls below 20480 bytes from H = 1015, H2 = 6930 on); 26 and 27 by --probe-caa: 26 is the
# first order whose top block holds non-vanishing integrals below 1e-13 (4.1e-14; 1.6e-13 at 25, 1.1e-14 at 27)
CAA_ORDERS = (13, 14, 26, 27)
N_PAIRS = {"bba": 36, "caa": 60}
N_RANDOM = 300


def bba_labels(lo, hi):
    return [(q, l) for q in range(lo, hi) for l in range(q + 1)]


def caa_labels(lo, hi):
    return [(q, a, b) for q in range(lo, hi) for a in range(q + 1) for b in range(q - a + 1) if (q - a - b) % 2 == 0]


def caa_thirds(A, B):
    return sorted({(a3, b3) for a3 in (abs(A[1] - B[1]), A[1] + B[1]) for b3 in (abs(A[2] - B[2]), A[2] + B[2])})


# ---- the float64 probe: smallest integral of a pair that does not vanish --------------------------------------------------
def probe_pairs(tree, n_end):
    """{pair: (smallest non-vanishing |integral|, number of them)} over the top block, by the 2 n_end- and 3 n_end + 3-node rules."""
    n2 = 2 * n_end - 1
    out = {}
    if tree == "bba":
        lo, hi = PY.Bba(n_end, nq=2 * n_end), PY.Bba(n_end)
        top = bba_labels(n_end - 2, n_end)
        for i, A in enumerate(top):
            for B in top[i:]:
                a, b = lo.polar(*A, *B), hi.polar(*A, *B)
                q3, l3 = np.arange(n2)[:, None], np.arange(n2)[None, :]
                even = ((l3 + A[1] + B[1]) % 2 == 0) & hi.mask                           # an odd l + l' + l'' never reaches a coefficient
                tri = (q3 >= abs(A[0] - B[0])) & (q3 <= A[0] + B[0]) & ((q3 + A[0] + B[0]) % 2 == 0)
                floor = np.abs(b[even & ~tri]).max()                                     # these vanish: what is there is rounding
                real = even & tri & (l3 >= abs(A[1] - B[1])) & (l3 <= A[1] + B[1]) & (np.abs(a - b) <= 0.01 * np.abs(b)) & (np.abs(b) > 100 * floor)
                out[(A, B)] = (np.abs(b[real]).min() if real.any() else np.inf, int(real.sum()))
    else:
        lo, hi = PY.Caa(n_end, nq=2 * n_end), PY.Caa(n_end)
        top = caa_labels(n_end - 2, n_end)
        for i, A in enumerate(top):
            for B in top[i:]:
                best, cnt = np.inf, 0
                for a3, b3 in caa_thirds(A, B):
                    (q3, a), b = lo.polar(*A, *B, a3, b3), hi.polar(*A, *B, a3, b3)[1]
                    tri = (q3 >= abs(A[0] - B[0])) & (q3 <= A[0] + B[0])
                    floor = np.abs(b[~tri]).max() if (~tri).any() else 1e-16            # these vanish: what is there is rounding
                    real = tri & (np.abs(a - b) <= 0.01 * np.abs(b)) & (np.abs(b) > 100 * floor)
                    cnt += int(real.sum())
                    if real.any():
                        best = min(best, np.abs(b[real]).min())
                out[(A, B)] = (best, cnt)
    return out


def choose_pairs(tree, n_end):
    ranked = probe_pairs(tree, n_end)
    keys = sorted(ranked, key=lambda p: (ranked[p][0], p))
    half = N_PAIRS[tree] // 2
    small = keys[:half]
    rest = keys[half:]
    rng = np.random.default_rng(4000 + n_end)
    pick = rng.choice(len(rest), size=min(N_PAIRS[tree] - half, len(rest)), replace=False)
    return sorted(small + [rest[i] for i in pick]), min(v[0] for v in ranked.values())


# ---- 40-digit node tables ------------------------------------------------------------------------------------------------
def mp_tables(tree, n_end):
    import mpmath as mpm
    mp = mpm.mp
    mp.dps = DIGITS
    n2 = 2 * n_end - 1
    nq = 2 * n_end + 1                                              # exact to degree 4 n_end + 1 >= 4 n_end - 3

    def legendre_rule(n):
        x0 = np.polynomial.legendre.leggauss(n)[0]
        xs, ws = [], []
        for g in x0:
            x = mp.mpf(float(g))
            for _ in range(8):
                p0, p1 = mp.mpf(1), x
                for k in range(2, n + 1):
                    p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
                dp = n * (x * p1 - p0) / (x * x - 1)
                x = x - p1 / dp
            p0, p1 = mp.mpf(1), x
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            dp = n * (x * p1 - p0) / (x * x - 1)
            xs.append(x)
            ws.append(2 / ((1 - x * x) * dp * dp))
        return xs, ws

    if tree == "bba":
        def gbar(kmax, lam, x):                                     # orthonormal Gegenbauer, weight (1 - x^2)^(lam - 1/2)
            h0 = mp.sqrt(mp.pi) * mp.gamma(lam + mp.mpf(1) / 2) / mp.gamma(lam + 1)
            a = lambda k: mp.sqrt(mp.mpf(k) * (k + 2 * lam - 1) / ((k + lam - 1) * (k + lam))) / 2   # noqa: E731
            p = [1 / mp.sqrt(h0)]
            if kmax >= 1:
                p.append(x * p[0] / a(1))
            for k in range(2, kmax + 1):
                p.append((x * p[k - 1] - a(k - 1) * p[k - 2]) / a(k))
            return p

        def table(xs):
            T = {}
            for i, x in enumerate(xs):
                s = mp.sqrt(1 - x * x)
                for l in range(n2):
                    g = gbar(n2 - 1 - l, l + 1, x)
                    for q in range(l, n2):
                        T.setdefault((q, l), [None] * len(xs))[i] = s ** l * g[q - l]
            return T
        th = [mp.pi * i / (nq + 1) for i in range(1, nq + 1)]
        xc, wc = [mp.cos(t) for t in th], [mp.pi / (nq + 1) * mp.sin(t) ** 2 for t in th]
        return {"even": (wc, table(xc))}
    xg, wg = legendre_rule(nq)
    cache = {}

    def cbar(q, a, b):
        v = cache.get((q, a, b))
        if v is None:
            k = (q - a - b) // 2
            h = mp.mpf(2) ** (a + b + 1) / (2 * k + a + b + 1) * mp.gamma(k + a + 1) * mp.gamma(k + b + 1) / (mp.gamma(k + 1) * mp.gamma(k + a + b + 1))
            nrm = mp.sqrt(4 * mp.mpf(2) ** (a + b) / h)
            v = []
            for x in xg:
                c, s = mp.sqrt((1 + x) / 2), mp.sqrt((1 - x) / 2)
                p0, p1 = mp.mpf(1), mp.mpf(1)                    # Jacobi P_k^{(alpha = b, beta = a)} by its three-term recurrence
                if k >= 1:
                    p1 = (b + 1) + (a + b + 2) * (x - 1) / 2
                    for m in range(1, k):
                        t = 2 * m + a + b
                        p0, p1 = p1, ((t + 1) * ((t + 2) * t * x + b * b - a * a) * p1 - 2 * (m + b) * (m + a) * (t + 2) * p0) / (2 * (m + 1) * (m + a + b + 1) * t)
                v.append(nrm * c ** a * s ** b * p1)
            cache[(q, a, b)] = v
        return v
    return {"w": [w / 4 for w in wg], "cbar": cbar}


def triple(w, fa, fb, fc):
    acc = 0
    for wi, a, b, c in zip(w, fa, fb, fc):
        acc += wi * a * b * c
    return acc


def build_case(tree, n_end):
    n2 = 2 * n_end - 1
    pairs, smallest64 = choose_pairs(tree, n_end)
    tabs = mp_tables(tree, n_end)
    rng = np.random.default_rng(7000 + n_end)
    lab, val = [], []
    if tree == "bba":
        thirds = bba_labels(0, n2)

        def one(A, B, Cc):
            w, T = tabs["even"]
            return triple(w, T[A], T[B], T[Cc])
        for A, B in pairs:
            for Cc in thirds:
                if (A[1] + B[1] + Cc[1]) % 2:
                    continue
                lab.append(A + B + Cc)
                val.append(one(A, B, Cc))
        low = bba_labels(0, n_end)
        for i in range(N_RANDOM):
            A, B = low[rng.integers(len(low))], low[rng.integers(len(low))]
            if i % 2:                                               # every other one from the labels the triangle and parity rules admit
                adm = [(q2, l2) for q2 in range(abs(A[0] - B[0]), A[0] + B[0] + 1, 2) for l2 in range(abs(A[1] - B[1]), min(A[1] + B[1], q2) + 1, 2)]
                Cc = adm[rng.integers(len(adm))]
            else:
                Cc = thirds[rng.integers(len(thirds))]
                while (A[1] + B[1] + Cc[1]) % 2:
                    Cc = thirds[rng.integers(len(thirds))]
            lab.append(A + B + Cc)
            val.append(one(A, B, Cc))
    else:
        w, cbar = tabs["w"], tabs["cbar"]
        for A, B in pairs:
            for a3, b3 in caa_thirds(A, B):
                for q3 in range(a3 + b3, n2, 2):
                    lab.append(A + B + (q3, a3, b3))
                    val.append(triple(w, cbar(*A), cbar(*B), cbar(q3, a3, b3)))
        low = caa_labels(0, n_end)
        for i in range(N_RANDOM):
            A, B = low[rng.integers(len(low))], low[rng.integers(len(low))]
            t3 = caa_thirds(A, B)
            a3, b3 = t3[rng.integers(len(t3))]
            qs = list(range(a3 + b3, n2, 2))
            if i % 2:
                qs = [q for q in qs if abs(A[0] - B[0]) <= q <= A[0] + B[0]] or qs
            q3 = qs[rng.integers(len(qs))]
            lab.append(A + B + (q3, a3, b3))
            val.append(triple(w, cbar(*A), cbar(*B), cbar(q3, a3, b3)))
    zero = np.array([abs(v) < VANISH for v in val])
    v64 = np.array([0.0 if z else float(v) for v, z in zip(val, zero)])
    live = np.abs(v64[~zero])
    print(f"{tree} n_end {n_end}: {len(pairs)} pairs, {len(val)} integrals, {int((~zero).sum())} do not vanish; smallest {live.min():.3e} "
          f"(float64 probe of the whole block: {smallest64:.3e}), {int((live < 1e-12).sum())} below 1e-12, largest vanishing modulus "
          f"{max([float(abs(v)) for v, z in zip(val, zero) if z] or [0.0]):.1e}", flush=True)
    width = len(pairs[0][0])
    return {f"{tree}_{n_end}_lab": np.array(lab, dtype=np.int8), f"{tree}_{n_end}_val": v64, f"{tree}_{n_end}_zero": zero,
            f"{tree}_{n_end}_pairs": np.array([A + B for A, B in pairs], dtype=np.int8).reshape(len(pairs), 2 * width)}


class CaaLongDouble:
    """cbar and I3 in numpy's long double (64-bit mantissa on x86) with 2 n_end + 1 nodes: the probe below needs integrals of 1e-13
    told from rounding, which float64 cannot do."""

    def __init__(self, n_end):
        ld = np.longdouble
        self.n2 = 2 * n_end - 1
        x0, _ = np.polynomial.legendre.leggauss(2 * n_end + 1)
        x = x0.astype(ld)
        n = len(x)
        for _ in range(4):                                          # Newton on P_n in long double
            p0, p1 = np.ones(n, dtype=ld), x.copy()
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            dp = n * (x * p1 - p0) / (x * x - 1)
            x = x - p1 / dp
        p0, p1 = np.ones(n, dtype=ld), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        self.x, self.w = x, (2 / ((1 - x * x) * dp * dp)) / 4
        self.c, self.s = np.sqrt((1 + x) / 2), np.sqrt((1 - x) / 2)
        self._c = {}

    def cbar(self, q, a, b):
        v = self._c.get((q, a, b))
        if v is None:
            ld = np.longdouble
            k, x = (q - a - b) // 2, self.x
            p0, p1 = np.ones(len(x), dtype=ld), np.ones(len(x), dtype=ld)
            if k >= 1:
                p1 = (b + 1) + (a + b + 2) * (x - 1) / 2
                for m in range(1, k):
                    t = ld(2 * m + a + b)
                    p0, p1 = p1, ((t + 1) * ((t + 2) * t * x + b * b - a * a) * p1 - 2 * (m + b) * (m + a) * (t + 2) * p0) / (2 * (m + 1) * (m + a + b + 1) * t)
            r = ld(2 * (2 * k + a + b + 1))
            for i in range(1, a + 1):
                r = r * (k + b + i) / (k + i)
            v = self._c[(q, a, b)] = np.sqrt(r) * self.c ** a * self.s ** b * p1
        return v

    def polar(self, A, B, a3, b3):
        st = self._c.get((a3, b3))
        if st is None:
            q3 = np.arange(a3 + b3, self.n2, 2)
            st = self._c[(a3, b3)] = (q3, np.array([self.cbar(int(n3), a3, b3) for n3 in q3]))
        return st[0], st[1] @ (self.w * self.cbar(*A) * self.cbar(*B))


def probe_caa():
    """Smallest top-block integral of caa that does not vanish, per order: long double, counted when it lies inside the triangle of the
    degrees and 100 times above the largest modulus found outside it (where every integral vanishes) at that order."""
    for n_end in range(14, 33):
        y = CaaLongDouble(n_end)
        top = caa_labels(n_end - 2, n_end)
        inside, floor = [], 0.0
        for i, A in enumerate(top):
            for B in top[i:]:
                for a3, b3 in caa_thirds(A, B):
                    q3, v = y.polar(A, B, a3, b3)
                    tri = (q3 >= abs(A[0] - B[0])) & (q3 <= A[0] + B[0])
                    v = np.abs(v).astype(np.float64)
                    inside.append(v[tri])
                    floor = max(floor, v[~tri].max() if (~tri).any() else 0.0)
        inside = np.concatenate(inside)
        live = inside[inside > 100 * floor]
        print(f"caa n_end {n_end}: smallest non-vanishing top-block integral {live.min():.3e}, {int((live < 1e-13).sum())} below 1e-13 "
              f"(rounding floor {floor:.1e}, {int((inside <= 100 * floor).sum())} of {len(inside)} inside the triangle at or below 100 floors)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe-caa", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden", "polar4_integrals.npz"))
    args = ap.parse_args()
    if args.probe_caa:
        return probe_caa()
    data = {}
    for tree, orders in (("bba", BBA_ORDERS), ("caa", CAA_ORDERS)):
        for n_end in orders:
            data.update(build_case(tree, n_end))
    np.savez_compressed(args.out, **data)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
