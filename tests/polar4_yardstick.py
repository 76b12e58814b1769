"""Translation yardstick of the 4-D trees bba and caa that shares no cut with the library or the oracle (helper module, not a test).

The Gaunt integral of three harmonics of a 4-D tree is a polar triple integral times what the remaining angles give:

    bba:  G(h', h, h'') = delta(m'' = m' - m) A4[(q'l'), (ql), (q''l'')] G3[(l'm'), (lm), l''] ,
          A4 = int_0^pi Abar_{q'l'} Abar_{ql} Abar_{q''l''} sin^2 dt ,   Abar_{ql} = sin^l Gbar_{q-l}^{(l+1)}(cos t)
          G3 = int over S^2 of Ybar_{l'm'} conj(Ybar_{lm}) conj(Ybar_{l'', m'-m})    (real)
    caa:  G(h', h, h'') = delta(m1'' = m1' - m1) delta(m2'' = m2' - m2) / (2 pi) I3 ,
          I3 = int_0^{pi/2} cbar' cbar cbar'' sin cos dt ,   cbar_{n,a,b} = cos^a sin^b Pbar_k^{(b,a)}(cos 2t), k = (n - a - b) / 2

and SR[h', h] = C_4 sum_{h''} Re(i^{n + n'' - n'}) G(h', h, h'') h_{n''}(k |t|) Y_{h''}(t^).  Everything here is float64 with a rule of
3 n_end + 3 nodes (the library and the oracle's `_theta4` / `_theta_c` use 2 n_end), and NO selection rule beyond the azimuthal deltas
is applied: every label of degree < 2 n_end - 1 with the right azimuthal orders is a candidate and the integrals are left to vanish.

* A4: for l + l' + l'' even the integrand is a polynomial times sqrt(1 - x^2), x = cos t, and Gauss-Chebyshev of the second kind is
  exact.  For an odd sum it is not, but there the integrand of G3 is odd under x -> -x and the symmetric Gauss-Legendre rule returns
  zero to rounding, so the product vanishes all the same (the argument of tests/chain_yardstick.py).
* I3: |m'| + |m| + |m' - m| is even at both azimuths, so the integrand is a polynomial in x = cos 2t (Gauss-Legendre).

The building blocks (`O._gbar`, `O._pbar`, the formula of `O._cbar`: the harmonics themselves) are the oracle's, pinned by the reference goldens;
tests/golden/polar4_integrals.npz (tools/make_polar4_fixtures.py, 40 digits) pins A4 and I3 of this module, and
tests/test_polar4_yardstick_host.py ties the assembled coefficients to `chain_yardstick` and `O._theta_c` at n_end 6.  Labels, label
order and the sign convention are those of tests/chain_yardstick.py: `all_labels(hp, h)` returns the candidate labels h'' (indices among
the labels of degree < 2 n_end - 1) and G without the sign.
"""
import math

import numpy as np

from oracle import biem_oracle as O

# `polar4_sr` does not carry coefficients below this (the rule of tests/chain_yardstick.py): the rounding of an integral that vanishes,
# 1e-17, meets table values h_{n''} of 1e16 and more at the orders the GPU tests run, and would bury the entries of low degree.  That
# is a constant cut, so `polar4_sr` is a reference only up to SR_N_END_MAX, where the smallest coefficient that does not vanish is
# 2.8e-11 (bba) / 1.6e-8 (caa), two decades and more above it; it refuses higher orders.  `coefficients`, which the term-list tests
# read, cuts nothing at any order.
G_SKIP = 1e-13
SR_N_END_MAX = 15


def nodes_of(n_end):
    return 3 * n_end + 3


def legendre_rule(n):
    """Gauss-Legendre nodes and weights: SciPy's / NumPy's nodes polished by Newton steps on P_n, and the weights 2 / ((1 - x^2) P_n'^2)
    from the polished nodes (the library routines' weights carry 5e-15, which is 3e-13 in a caa integral of order 26)."""
    x = np.polynomial.legendre.leggauss(n)[0]
    for it in range(3):
        p0, p1 = np.ones(n), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        if it < 2:
            x = x - p1 / dp
    return x, 2.0 / ((1.0 - x * x) * dp * dp)


def pair_key(A, B):
    return tuple(A) + tuple(B) if tuple(A) <= tuple(B) else tuple(B) + tuple(A)


def pin_fixture(y, lab, val, pairs):
    """Replace the polar integrals of `pairs`, which a fixture case holds whole (every third label), by its 40-digit values."""
    w = len(lab[0]) // 3
    whole = {pair_key(r[:w], r[w:]) for r in pairs.tolist()}
    keep = [pair_key(r[:w], r[w:2 * w]) in whole for r in lab.tolist()]
    lab, val = lab[keep], val[keep]
    if y.name == "bba":
        for key in {tuple(r[:2 * w]) for r in lab.tolist()}:
            y._polar[pair_key(key[:w], key[w:])] = np.zeros((y.n2, y.n2))
        for r, v in zip(lab.tolist(), val):
            y._polar[pair_key(r[:w], r[w:2 * w])][r[4], r[5]] = v
    else:
        for r, v in zip(lab.tolist(), val):
            key = pair_key(r[:w], r[w:2 * w]) + (r[7], r[8])
            if key not in y._polar:
                q3 = np.arange(r[7] + r[8], y.n2, 2)
                y._polar[key] = (q3, np.zeros(len(q3)))
            y._polar[key][1][(r[6] - r[7] - r[8]) // 2] = v


class Bba:
    name = "bba"

    def __init__(self, n_end, nq=None):
        self.n_end, self.n2 = n_end, 2 * n_end - 1
        n2 = self.n2
        nq = self.nq = nq or nodes_of(n_end)
        tr = O.tree("bba")
        self.idx, self.idx2 = tr.index(n_end), tr.index(n2)
        self.H, self.H2 = len(self.idx), len(self.idx2)
        self.deg2 = np.array([t[0] for t in self.idx2])
        self.pos2 = {lab: i for i, lab in enumerate(self.idx2)}
        self.mask = np.tril(np.ones((n2, n2), dtype=bool))                      # [q'', l''] is a label where l'' <= q''

        def table(x):
            s = np.sqrt(1.0 - x * x)
            A = np.zeros((n2, n2, len(x)))
            for l in range(n2):
                g = O._gbar(n2 - 1 - l, l + 1.0, x)
                for q in range(l, n2):
                    A[q, l] = s ** l * g[q - l]
            return A
        xc, self.wc = O._gauss_cheb2(nq)                                        # weight sqrt(1 - x^2)
        self.Ac = table(xc)
        xl, self.wg = legendre_rule(nq)
        self.P = O._pbar(n2 - 1, xl)                                            # [l, m, node]; zero where m > l
        self._polar, self._gaunt = {}, {}

    def polar(self, qp, lp, q, l):
        """A4 against every (q'', l'') at once: [n2, n2], zero above the diagonal (no such label)."""
        key = pair_key((qp, lp), (q, l))
        v = self._polar.get(key)
        if v is None:
            n2 = self.n2
            v = self._polar[key] = (self.Ac.reshape(n2 * n2, -1) @ (self.wc * self.Ac[qp, lp] * self.Ac[q, l])).reshape(n2, n2) * self.mask
        return v

    def gaunt3(self, lp, mp, l, m):
        """G3 against every l'' < n2 (zero where l'' < |m' - m|: no such harmonic)."""
        key = (lp, abs(mp), l, abs(m), abs(mp - m))
        v = self._gaunt.get(key)
        if v is None:
            v = self._gaunt[key] = self.P[:, abs(mp - m), :] @ (self.wg * self.P[lp, abs(mp)] * self.P[l, abs(m)]) / math.sqrt(2.0 * math.pi)
        return v

    def all_labels(self, hp, h):
        (qp, lp, mp), (q, l, m) = self.idx[hp], self.idx[h]
        mu = mp - m
        A4, G3 = self.polar(qp, lp, q, l), self.gaunt3(lp, mp, l, m)
        cand = np.array([self.pos2[(q2, l2, mu)] for q2 in range(abs(mu), self.n2) for l2 in range(abs(mu), q2 + 1)], dtype=np.int64)
        g = np.array([A4[q2, l2] * G3[l2] for q2 in range(abs(mu), self.n2) for l2 in range(abs(mu), q2 + 1)])
        return cand, g


class Caa:
    name = "caa"

    def __init__(self, n_end, nq=None):
        self.n_end, self.n2 = n_end, 2 * n_end - 1
        n2 = self.n2
        nq = self.nq = nq or nodes_of(n_end)
        tr = O.tree("caa")
        self.idx, self.idx2 = tr.index(n_end), tr.index(n2)
        self.H, self.H2 = len(self.idx), len(self.idx2)
        self.deg2 = np.array([t[0] for t in self.idx2])
        self.pos2 = {lab: i for i, lab in enumerate(self.idx2)}
        xg, wg = legendre_rule(nq)
        self.th, self.w = 0.5 * np.arccos(xg), wg / 4.0
        self._c, self._polar = {}, {}

    def cbar(self, q, a, b):
        """`O._cbar` with the Jacobi polynomial by its three-term recurrence and the norm as a product (eval_jacobi and exp(lgamma) lose two digits at these degrees)."""
        v = self._c.get((q, a, b))
        if v is None:
            k, x = (q - a - b) // 2, np.cos(2 * self.th)
            p0, p1 = np.ones_like(x), np.ones_like(x)
            if k >= 1:
                p1 = (b + 1) + (a + b + 2) * (x - 1) / 2                         # P_k^{(alpha = b, beta = a)}
                for m in range(1, k):
                    t = 2.0 * m + a + b
                    p0, p1 = p1, ((t + 1) * ((t + 2) * t * x + b * b - a * a) * p1 - 2 * (m + b) * (m + a) * (t + 2) * p0) / (2 * (m + 1) * (m + a + b + 1) * t)
            r = 2.0 * (2 * k + a + b + 1)                                        # norm^2 = 2 (2k+a+b+1) k! (k+a+b)! / ((k+a)! (k+b)!)
            for i in range(1, a + 1):
                r *= (k + b + i) / (k + i)
            v = self._c[(q, a, b)] = math.sqrt(r) * np.cos(self.th) ** a * np.sin(self.th) ** b * p1
        return v

    def polar(self, qp, ap, bp, q, a, b, a3, b3):
        """I3 against every q'' = a'' + b'', a'' + b'' + 2, ... < n2: (the degrees q'', the integrals)."""
        pinned = self._polar.get(pair_key((qp, ap, bp), (q, a, b)) + (a3, b3))
        if pinned is not None:
            return pinned
        st = self._c.get((a3, b3))
        if st is None:
            q3 = np.arange(a3 + b3, self.n2, 2)
            st = self._c[(a3, b3)] = (q3, np.array([self.cbar(int(n3), a3, b3) for n3 in q3]).reshape(len(q3), -1))
        return st[0], st[1] @ (self.w * self.cbar(qp, ap, bp) * self.cbar(q, a, b))

    def all_labels(self, hp, h):
        (qp, m1p, m2p), (q, m1, m2) = self.idx[hp], self.idx[h]
        mu1, mu2 = m1p - m1, m2p - m2
        q3, I3 = self.polar(qp, abs(m1p), abs(m2p), q, abs(m1), abs(m2), abs(mu1), abs(mu2))
        cand = np.array([self.pos2[(int(n3), mu1, mu2)] for n3 in q3], dtype=np.int64)
        return cand, I3 / (2.0 * math.pi)


_YARD = {}


def yard(name, n_end):
    """The tables of one (tree, n_end); bpbpa is bba in permuted axes (`O.tree("bpbpa")`) and shares its coefficients."""
    name = {"bpbpa": "bba"}.get(name, name)
    key = (name, n_end)
    if key not in _YARD:
        if len(_YARD) >= 3:
            _YARD.pop(next(iter(_YARD)))
        _YARD[key] = (Bba if name == "bba" else Caa)(n_end)
    return _YARD[key]


def sign_of(y, hp, h, cand):
    """Re(i^{n + n'' - n'}) over the candidate labels (zero where the power of i is odd)."""
    return np.real(1j ** ((y.idx[h][0] + y.deg2[cand] - y.idx[hp][0]) % 4))


def coefficients(y, hp, h):
    """The Gaunt coefficients of the matrix entry (h', h) over all labels of degree < 2 n_end - 1 (dense, signed; nothing is cut)."""
    cand, g = y.all_labels(hp, h)
    out = np.zeros(y.H2)
    out[cand] = sign_of(y, hp, h, cand) * g
    return out


def table(name, n_end, k, t):
    """T[h''] = C_4 h_{n''}(k |t|) Y_{h''}(t^) over the labels of degree < 2 n_end - 1 of the canonical tree (t in its axes)."""
    y = yard(name, n_end)
    tr = O.tree(y.name)
    t = np.asarray(t, dtype=np.float64)
    r = float(np.linalg.norm(t))
    Cd = (2 * math.pi) ** 2 * math.sqrt(2.0 / math.pi)
    _, hn, _, _ = O.radial_h(y.n2 - 1, 4, k * r)
    return Cd * hn[y.deg2] * tr.harmonics((t / r)[None, :], y.n2)[:, 0]


def polar4_sr(name, n_end, k, t, entries=None):
    """SR[h', h] of bba / caa (bpbpa: t in that tree's own axes): the dense matrix, or the entries listed in `entries` as (h', h)."""
    assert n_end <= SR_N_END_MAX, f"polar4_sr drops coefficients below {G_SKIP}: no reference beyond n_end {SR_N_END_MAX}"
    tr = O.tree(name)
    t = np.asarray(t, dtype=np.float64)
    if tr.base:
        t = t[list(tr.perm)]
    y = yard(name, n_end)
    T = table(name, n_end, k, t)
    def carried(hp, h):
        c = coefficients(y, hp, h)
        return np.where(np.abs(c) >= G_SKIP, c, 0.0)
    if entries is None:
        entries = [(hp, h) for hp in range(y.H) for h in range(y.H)]
        return np.array([carried(hp, h) @ T for hp, h in entries]).reshape(y.H, y.H)
    return np.array([carried(int(hp), int(h)) @ T for hp, h in entries])


def sampled_sr_func(entries_of):
    """`sr_func` for `O.assemble`: only the entries `entries_of(call number)` (a list of (h', h)) are computed, the others are NaN."""
    calls = [0]

    def f(tr, n_end, k, t):
        ent = np.asarray(entries_of(calls[0]))
        calls[0] += 1
        H = tr.n_harm(n_end)
        out = np.full((H, H), np.nan + 0j)
        out[ent[:, 0], ent[:, 1]] = polar4_sr(tr.name, n_end, k, t, entries=ent)
        return out

    return f
