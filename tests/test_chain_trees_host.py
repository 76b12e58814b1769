"""Standard chain trees "b" * (d - 2) + "a" on the host (no GPU): plan tables against an independent test-local chain tree.

`Chain` restates the chain harmonics with SciPy (Gegenbauer polynomials, Gauss-Jacobi rules).  It equals the oracle's ba / bba
(pinned by the reference goldens), which validates it; at d >= 5 no reference fixture exists and it is the reference the plan tables
are checked against.  The translation term lists at d = 5 .. 10 are checked term by term in test_chain_yardstick_host.py.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.special as sp

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _coords, _lib
from oracle import biem_oracle as O


class Chain(O.Tree):
    """Chain tree of dimension d: Y = prod_j sin^{l_{j+1}} t_j Gbar_{l_j - l_{j+1}}^{(l_{j+1} + (d-j-2)/2)}(cos t_j) e^{i m phi} / sqrt(2 pi)."""

    def index(self, n_end):
        d = self.d
        out = []

        def rec(prefix, j, up):
            if j == d - 2:
                out.extend(tuple(prefix) + (m,) for m in range(-up, up + 1))
                return
            for l in range(up + 1):
                rec(prefix + [l], j + 1, l)

        for n in range(n_end):
            rec([n], 1, n)
        return out

    def degrees(self, n_end):
        return np.array([t[0] for t in self.index(n_end)])

    @staticmethod
    def _gbar(k, lam, x):
        hk = math.pi * 2.0 ** (1 - 2 * lam) * math.exp(math.lgamma(k + 2 * lam) - math.lgamma(k + 1) - 2 * math.lgamma(lam)) / (k + lam)
        return sp.eval_gegenbauer(k, lam, x) / math.sqrt(hk)

    def harmonics(self, u, n_end):
        u = np.asarray(u, dtype=np.float64)
        d = self.d
        tail = np.sqrt(np.cumsum((u * u)[:, ::-1], axis=1)[:, ::-1])            # |u_{j..}|
        c = [np.where(tail[:, j] > 0, u[:, j] / np.where(tail[:, j] > 0, tail[:, j], 1.0), 1.0) for j in range(d - 2)]
        s = [np.where(tail[:, j] > 0, tail[:, j + 1] / np.where(tail[:, j] > 0, tail[:, j], 1.0), 0.0) for j in range(d - 2)]
        phi = np.arctan2(u[:, d - 1], u[:, d - 2])
        idx = self.index(n_end)
        out = np.zeros((len(idx), u.shape[0]), dtype=np.complex128)
        for h, lab in enumerate(idx):
            ls = list(lab[:-1]) + [abs(lab[-1])]
            amp = np.full(u.shape[0], 1.0 / math.sqrt(2 * math.pi))
            for j in range(d - 2):
                amp = amp * s[j] ** ls[j + 1] * self._gbar(ls[j] - ls[j + 1], ls[j + 1] + (d - j - 2) / 2.0, np.clip(c[j], -1, 1))
            out[h] = amp * np.exp(1j * lab[-1] * phi)
        return out

    def quadrature(self, n):
        d = self.d
        rules = [sp.roots_jacobi(n, (d - j - 3) / 2.0, (d - j - 3) / 2.0) for j in range(d - 2)]
        # the Gauss-Chebyshev (a = 1/2) node runs from +1 down, as the bba rule does (oracle, reference goldens)
        rules = [(r[0][::-1], r[1][::-1]) if d - j - 3 == 1 else r for j, r in enumerate(rules)]
        phi = np.arange(2 * n) * (math.pi / n)
        grids = np.meshgrid(*[r[0] for r in rules], phi, indexing="ij")
        wgrid = np.ones(grids[0].shape)
        for j, r in enumerate(rules):
            shape = [1] * (d - 1)
            shape[j] = n
            wgrid = wgrid * r[1].reshape(shape)
        wgrid = wgrid * (math.pi / n)
        comps, sprod = [], np.ones(grids[0].shape)
        for j in range(d - 2):
            comps.append(sprod * grids[j])
            sprod = sprod * np.sqrt(1 - grids[j] ** 2)
        comps += [sprod * np.cos(grids[-1]), sprod * np.sin(grids[-1])]
        return np.stack(comps, -1).reshape(-1, d), wgrid.reshape(-1)


def chain(d):
    return Chain("b" * (d - 2) + "a", d)


def sphere_area(d):
    return 2 * math.pi ** (d / 2) / math.gamma(d / 2)


def _plan(lib, d, n_end):
    p = C.c_void_p()
    _lib.check(lib.biem_plan_create_chain_host(d, n_end, C.byref(p)), "biem_plan_create_chain_host")
    dd, H, Q, H2, nt = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    _lib.check(lib.biem_plan_info(p, C.byref(dd), C.byref(H), C.byref(Q), C.byref(H2), C.byref(nt)))
    return p, dd.value, H.value, Q.value, H2.value, nt.value


def test_chain_harness_equals_oracle_ba_bba():
    rng = np.random.default_rng(0)
    for name, d in (("ba", 3), ("bba", 4)):
        tr, ch = O.tree(name), chain(d)
        assert ch.index(6) == tr.index(6)
        u = rng.normal(size=(20, d))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        assert np.abs(ch.harmonics(u, 6) - tr.harmonics(u, 6)).max() < 5e-14
        (y1, w1), (y2, w2) = ch.quadrature(5), tr.quadrature(5)
        assert np.abs(y1 - y2).max() < 1e-14 and np.abs(w1 - w2).max() < 1e-14


@pytest.mark.parametrize("d,n_end", [(5, 3), (6, 3), (7, 3), (5, 5), (8, 3), (9, 3), (10, 3)])
def test_chain_plan_tables(d, n_end):
    lib = _lib.load()
    ch = chain(d)
    p, dd, H, Q, H2, nt = _plan(lib, d, n_end)
    try:
        name = "b" * (d - 2) + "a"
        assert dd == d and H == _coords.harm_count(name, n_end) == ch.n_harm(n_end)
        assert H2 == _coords.harm_count(name, 2 * n_end - 1)
        lab = np.zeros((H, d - 1), dtype=np.int32)
        deg = np.zeros(H, dtype=np.int32)
        _lib.check(lib.biem_plan_labels_n(p, d - 1, lab.ctypes.data, deg.ctypes.data))
        assert [tuple(r) for r in lab.tolist()] == ch.index(n_end) and (deg == ch.degrees(n_end)).all()
        # the width-3 entry does not truncate: it refuses
        assert lib.biem_plan_labels(p, lab.ctypes.data, deg.ctypes.data) == 3
        y = np.zeros((Q, d))
        w = np.zeros(Q)
        _lib.check(lib.biem_plan_quadrature(p, y.ctypes.data, w.ctypes.data))
        yo, wo = ch.quadrature(n_end)
        assert np.abs(y - yo).max() < 1e-13 and np.abs(w - wo).max() < 1e-13
        assert abs(w.sum() - sphere_area(d)) < 1e-12 * sphere_area(d)
        W = np.zeros((Q, H), dtype=np.complex128)
        _lib.check(lib.biem_plan_projection(p, W.ctypes.data))
        Y = ch.harmonics(yo, n_end)                                       # [H, Q]
        assert np.abs(W - wo[:, None] * np.conj(Y.T)).max() < 1e-13
        # orthonormal under the rule
        assert np.abs(Y @ W - np.eye(H)).max() < 1e-12
        # translation terms: sum_p coef[p] C_d h_{n''}(k|t|) Y_{l''}(t^) == the quadrature closed form with the chain tree
        ptr = np.zeros(H * H + 1, dtype=np.int64)
        coef = np.zeros(nt)
        tidx = np.zeros(nt, dtype=np.int32)
        _lib.check(lib.biem_plan_terms(p, ptr.ctypes.data, coef.ctypes.data, tidx.ctypes.data))
        assert ptr[-1] == nt
        if n_end > 3:
            return
        if d > 7:                            # the tensor rule of the cross-check below is (2 n_end)^(d-2) 4 n_end points: gigabytes of
            return                           # harmonics from d = 8 on; test_chain_yardstick_host.py checks these lists term by term
        O._TREES[ch.name] = ch
        try:
            rng = np.random.default_rng(d)
            k = 1.3
            Cd = (2 * math.pi) ** (d / 2) * math.sqrt(2 / math.pi)
            deg2 = ch.degrees(2 * n_end - 1)
            for _ in range(3):
                t = rng.normal(size=d)
                t *= 2.7 / np.linalg.norm(t)
                _, hn, _, _ = O.radial_h(2 * n_end - 2, d, k * np.linalg.norm(t))
                T = Cd * hn[deg2] * ch.harmonics((t / np.linalg.norm(t))[None, :], 2 * n_end - 1)[:, 0]
                S = np.add.reduceat(coef * T[tidx], ptr[:-1]) if nt else np.zeros(H * H)
                S[ptr[:-1] == ptr[1:]] = 0.0
                SRq = O.translation_SR_quadrature(ch, n_end, k, t)        # [h', h]
                assert np.abs(S.reshape(H, H) - SRq.T).max() < 1e-11 * np.abs(SRq).max()
        finally:
            del O._TREES[ch.name]
            O._sr_tables.cache_clear()
    finally:
        lib.biem_plan_destroy(p)


def test_chain_plans_of_ba_bba_match_their_trees():
    """d = 3, 4 through the chain builder: the labels, rule and projection of ba / bba; the same translation sums."""
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for tree, d in ((1, 3), (2, 4)):
        n_end = 5
        pc, _, H, Q, H2, ntc = _plan(lib, d, n_end)
        po = C.c_void_p()
        _lib.check(lib.biem_plan_create_host(tree, n_end, C.byref(po)))
        try:
            lo = np.zeros((H, 3), dtype=np.int32)
            lc = np.zeros((H, 3), dtype=np.int32)
            _lib.check(lib.biem_plan_labels(po, lo.ctypes.data, None))
            _lib.check(lib.biem_plan_labels_n(pc, 3, lc.ctypes.data, None))
            assert (lo == lc).all()
            Wo, Wc = np.zeros((Q, H), dtype=np.complex128), np.zeros((Q, H), dtype=np.complex128)
            _lib.check(lib.biem_plan_projection(po, Wo.ctypes.data))
            _lib.check(lib.biem_plan_projection(pc, Wc.ctypes.data))
            assert np.abs(Wo - Wc).max() < 1e-14
            sums = []
            T = rng.normal(size=H2) + 1j * rng.normal(size=H2)
            for p in (po, pc):
                nt = C.c_longlong()
                lib.biem_plan_info(p, None, None, None, None, C.byref(nt))
                ptr = np.zeros(H * H + 1, dtype=np.int64)
                coef = np.zeros(nt.value)
                tidx = np.zeros(nt.value, dtype=np.int32)
                _lib.check(lib.biem_plan_terms(p, ptr.ctypes.data, coef.ctypes.data, tidx.ctypes.data))
                sums.append(np.array([np.sum(coef[ptr[e]:ptr[e + 1]] * T[tidx[ptr[e]:ptr[e + 1]]]) for e in range(H * H)]))
            assert np.abs(sums[0] - sums[1]).max() < 1e-13 * np.abs(sums[0]).max()
        finally:
            lib.biem_plan_destroy(po)
            lib.biem_plan_destroy(pc)


def test_chain_over_limit_fails_cleanly():
    lib = _lib.load()
    p = C.c_void_p()
    assert lib.biem_plan_create_chain_host(7, 8, C.byref(p)) == 3            # H2 = 65892 > 65535
    assert b"16-bit" in lib.biem_last_error() and b"65535" in lib.biem_last_error()
    assert lib.biem_plan_create_chain_host(10, 5, C.byref(p)) == 3            # H2 and the node tables fit, Q x H = 3906250 x 935 > 2^31 does not
    assert b"projection matrix" in lib.biem_last_error()
    assert lib.biem_plan_create_chain_host(11, 2, C.byref(p)) == 3
    assert b"unsupported" in lib.biem_last_error()
    assert lib.biem_plan_create_host(7, 3, C.byref(p)) == 3
    assert b"unsupported" in lib.biem_last_error()


def test_unsupported_strings_and_coordinates():
    for bt in ("cba", "bpbpbpa", "bpbbpa", "cab", "caaa", "bbbb", "ba" + "a"):
        with pytest.raises(NotImplementedError, match="not built"):
            amd.create_from_branching_types(bt)
    rng = np.random.default_rng(1)
    for d in (5, 6, 7):
        bt = "b" * (d - 2) + "a"
        c = amd.create_from_branching_types(bt)
        assert c.c_ndim == d and c.s_ndim == d - 1
        x = rng.normal(size=(d, 9))
        sph = c.from_cartesian(x)
        assert np.allclose(c.to_cartesian(sph, as_array=True), x)
        assert np.allclose(sph["r"], np.linalg.norm(x, axis=0))
        assert _coords.n_end_from_harm(bt, _coords.harm_count(bt, 7)) == 7
        assert _coords.harm_count(bt, 4) == chain(d).n_harm(4)
    assert _coords.harm_count("bbba", 7) == 336
