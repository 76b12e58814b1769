"""Closed-form translation yardstick for the standard chain trees "b" * (d - 2) + "a" (helper module, not a test).

In a chain tree the Gaunt integral of three harmonics factorises:

    G(h', h, h'') = int Y_{h'} conj(Y_h) conj(Y_{h''}) dOmega = delta(m'' = m' - m) / sqrt(2 pi) * prod_j I_j ,
    I_j = int_{-1}^{1} (1 - x^2)^{(d-j-3)/2} f'_j f_j f''_j dx ,   f_j = (1 - x^2)^{l_{j+1}/2} Gbar_{l_j - l_{j+1}}^{(l_{j+1} + (d-j-2)/2)}(x)

(one 1-D integral per polar node j = 0 .. d-3, l_{d-2} = |m|), and

    SR[h', h] = C_d sum_{h''} Re(i^{n + n'' - n'}) G(h', h, h'') h_{n''}(k |t|) Y_{h''}(t^) ,   C_d = (2 pi)^{d/2} sqrt(2 / pi).

Every I_j is taken with the 2 n_end-point Gauss-Jacobi rule of its node, exact wherever the integrand is a polynomial times the weight.
NO selection rule is applied: the sum runs over every label of degree < 2 n_end - 1 with m'' = m' - m and the integrals are left to
vanish.  (Where the powers of sqrt(1 - x^2) at a node sum to an odd number the rule is not exact there, but then the degree differences at
some node below sum to an odd number as well - |m'| + |m| + |m' - m| is even - and that node's integrand is odd under x -> -x: the
symmetric rule returns zero to rounding, so the product vanishes all the same.)  That keeps this module independent of the rules by
which the library chooses its terms.  Pure NumPy / SciPy in float64; `Chain` (tests/test_chain_trees_host.py) supplies the labels, the
normalised Gegenbauer polynomials and the harmonics; tests/test_chain_yardstick_host.py ties the result to the oracle's ba / bba tables,
which the reference goldens pin.
"""
import math

import numpy as np
import scipy.special as sp

from oracle import biem_oracle as O

from test_chain_trees_host import Chain, chain

G_SKIP = 1e-13          # terms below this are not carried (rounding of the integrals that vanish)


class _Gaunt:
    """Node tables of one (d, n_end) and a per-entry cache of the term lists."""

    def __init__(self, d, n_end):
        self.d, self.n_end = d, n_end
        self.ch = ch = chain(d)
        n2 = self.n2 = 2 * n_end - 1
        nq = 2 * n_end
        self.idx = ch.index(n_end)
        self.idx2 = ch.index(n2)
        self.H, self.H2 = len(self.idx), len(self.idx2)
        self.deg2 = np.array([t[0] for t in self.idx2])
        lab2 = np.array(self.idx2, dtype=np.int64).reshape(self.H2, d - 1)
        low = np.concatenate([lab2[:, 1:-1], np.abs(lab2[:, -1:])], axis=1)          # l_{j+1}, j = 0 .. d-3
        self.flat2 = lab2[:, :-1] * n2 + low                                        # [H2, d-2]: (l_j, l_{j+1}) of every label
        self.cand = {mu: np.nonzero(lab2[:, -1] == mu)[0] for mu in range(-(n2 - 1), n2)}
        # node factors at the node's rule: F[j][L * n2 + L1, q]; wF = w * F
        self.F, self.w = [], []
        for j in range(d - 2):
            a = (d - j - 3) / 2.0
            x, w = sp.roots_jacobi(nq, a, a)
            s = np.sqrt(1.0 - x * x)
            F = np.zeros((n2 * n2, nq))
            for L in range(n2):
                for L1 in range(L + 1):
                    F[L * n2 + L1] = s ** L1 * Chain._gbar(L - L1, L1 + (d - j - 2) / 2.0, x)
            self.F.append(F)
            self.w.append(w)
        self._node = {}
        self._entry = {}

    def _node_vec(self, j, a0, a1, b0, b1):
        """I_j against every (l''_j, l''_{j+1}) at once."""
        key = (j, a0, a1, b0, b1) if (a0, a1) <= (b0, b1) else (j, b0, b1, a0, a1)
        v = self._node.get(key)
        if v is None:
            n2, F = self.n2, self.F[j]
            v = self._node[key] = F @ (self.w[j] * F[a0 * n2 + a1] * F[b0 * n2 + b1])
        return v

    def all_labels(self, hp, h):
        """(candidate labels h'', G) of the entry (h', h): every label with m'' = m' - m, nothing skipped, no sign."""
        a, b = self.idx[hp], self.idx[h]
        d = self.d
        cand = self.cand[a[-1] - b[-1]]
        la = list(a[:-1]) + [abs(a[-1])]
        lb = list(b[:-1]) + [abs(b[-1])]
        g = np.full(len(cand), 1.0 / math.sqrt(2.0 * math.pi))
        for j in range(d - 2):
            g = g * self._node_vec(j, la[j], la[j + 1], lb[j], lb[j + 1])[self.flat2[cand, j]]
        return cand, g

    def terms(self, hp, h):
        """(labels h'', Re(i^{n + n'' - n'}) G) of the entry (h', h), |G| >= G_SKIP only."""
        out = self._entry.get((hp, h))
        if out is None:
            cand, g = self.all_labels(hp, h)
            keep = np.abs(g) >= G_SKIP
            cand, g = cand[keep], g[keep]
            e = self.idx[h][0] + self.deg2[cand] - self.idx[hp][0]
            assert (e % 2 == 0).all(), ("i^(n + n'' - n') is not real on a term that does not vanish", self.idx[hp], self.idx[h])
            out = self._entry[(hp, h)] = (cand, np.where(e % 4 == 0, 1.0, -1.0) * g)
        return out


_GAUNT = {}


def gaunt(d, n_end):
    key = (d, n_end)
    if key not in _GAUNT:
        if len(_GAUNT) >= 4:
            _GAUNT.pop(next(iter(_GAUNT)))
        _GAUNT[key] = _Gaunt(d, n_end)
    return _GAUNT[key]


def table(d, n_end, k, t):
    """T[h''] = C_d h_{n''}(k |t|) Y_{h''}(t^) over the labels of degree < 2 n_end - 1 (the convention of test_chain_plan_tables)."""
    g = gaunt(d, n_end)
    t = np.asarray(t, dtype=np.float64)
    r = float(np.linalg.norm(t))
    Cd = (2 * math.pi) ** (d / 2.0) * math.sqrt(2.0 / math.pi)
    _, hn, _, _ = O.radial_h(g.n2 - 1, d, k * r)
    return Cd * hn[g.deg2] * g.ch.harmonics((t / r)[None, :], g.n2)[:, 0]


def chain_sr(d, n_end, k, t, entries=None):
    """SR[h', h] = (S|R)_{h' -> h}(t) of the chain tree of dimension d: the dense [H, H] matrix, or with `entries` (a list of (h', h))
    the vector of those entries."""
    g = gaunt(d, n_end)
    T = table(d, n_end, k, t)
    if entries is None:
        out = np.zeros((g.H, g.H), dtype=np.complex128)
        for hp in range(g.H):
            for h in range(g.H):
                lab, cf = g.terms(hp, h)
                out[hp, h] = cf @ T[lab]
        return out
    out = np.zeros(len(entries), dtype=np.complex128)
    for i, (hp, h) in enumerate(entries):
        lab, cf = g.terms(int(hp), int(h))
        out[i] = cf @ T[lab]
    return out


def sr_func(tr, n_end, k, t):
    """The yardstick in the shape `O.assemble` / `O.solve_biem` take as `sr_func` (tr: a chain tree registered in `O._TREES`)."""
    return chain_sr(tr.d, n_end, k, t)


def sampled_sr_func(entries_of):
    """As `sr_func`, but only the entries `entries_of(call number)` (a list of (h', h)) are computed; the others are NaN."""
    calls = [0]

    def f(tr, n_end, k, t):
        ent = entries_of(calls[0])
        calls[0] += 1
        H = tr.n_harm(n_end)
        out = np.full((H, H), np.nan + 0j)
        ent = np.asarray(ent)
        out[ent[:, 0], ent[:, 1]] = chain_sr(tr.d, n_end, k, t, entries=ent)
        return out

    return f
