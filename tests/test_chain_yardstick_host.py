"""The factorised closed form of tests/chain_yardstick.py against what is pinned, and the plan's term lists against it (no GPU).

1. On ba / bba the yardstick reproduces `O.translation_SR` (pinned by the reference goldens) at n_end 8 / 6, and at d = 5, 6 the
   independent `O.translation_SR_quadrature` at n_end 3 (its small-order range), to 1e-12 of max |SR|: the oracle's own tables carry
   1e-12 noise cuts.
2. The translation term lists of the chain plans, term by term, at the largest orders the GPU tests run (d = 5 .. 10): every label the
   yardstick carries is listed exactly once with the same coefficient, and nothing else is listed with a coefficient that does not
   vanish.  A contraction with a table would let a missing term cancel a spurious one; this does not.
"""
import ctypes as C
import math

import numpy as np
import pytest

from biem_helmholtz_sphere_amd import _lib
from oracle import biem_oracle as O

import chain_yardstick as CY
from test_chain_trees_host import _plan, chain

SR_TOL = 1e-12          # of max |SR|
COEF_TOL = 1e-13        # a listed coefficient against the yardstick's
G_PRESENT = 1e-12       # a yardstick term at least this large must be listed


def _displacements(d, rng):
    """generic, along +e_0, along -e_{d-1}, in the plane of the last two axes"""
    t = rng.normal(size=d)
    t *= 2.7 / np.linalg.norm(t)
    plane = np.zeros(d)
    plane[d - 2], plane[d - 1] = 1.9, -1.4
    return {"generic": t, "+e0": 2.4 * np.eye(d)[0], "-e_last": -3.1 * np.eye(d)[d - 1], "last plane": plane}


@pytest.mark.parametrize("k", [1.3, 1.3 + 0.2j], ids=["real_k", "complex_k"])
@pytest.mark.parametrize("name,n_end", [("ba", 8), ("bba", 6)])
def test_yardstick_equals_pinned_tables_on_ba_bba(name, n_end, k):
    tr = O.tree(name)
    for what, t in _displacements(tr.d, np.random.default_rng(tr.d)).items():
        want = O.translation_SR(tr, n_end, k, t)
        got = CY.chain_sr(tr.d, n_end, k, t)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name} n_end {n_end} k {k} t {what}: {err:.2e} of max |SR|")
        assert err <= SR_TOL, (name, what, err)
        # the listed-entries form returns the same numbers
        ent = [(0, 0), (len(want) - 1, 0), (3, len(want) - 2)]
        assert np.array_equal(CY.chain_sr(tr.d, n_end, k, t, entries=ent), np.array([got[e] for e in ent]))


@pytest.mark.parametrize("d", [5, 6])
def test_yardstick_equals_quadrature_form_at_small_order(d, monkeypatch):
    ch = chain(d)
    monkeypatch.setitem(O._TREES, ch.name, ch)
    O._sr_tables.cache_clear()
    try:
        for k in (1.3, 1.3 + 0.2j):
            for what, t in _displacements(d, np.random.default_rng(d)).items():
                want = O.translation_SR_quadrature(ch, 3, k, t)
                got = CY.sr_func(ch, 3, k, t)
                err = np.abs(got - want).max() / np.abs(want).max()
                print(f"d {d} k {k} t {what}: {err:.2e} of max |SR|")
                assert err <= SR_TOL, (d, what, err)
    finally:
        O._sr_tables.cache_clear()


def _sample_entries(g, rng, count=150):
    H, n = g.H, g.n_end
    ent = {(H - 1, H - 1), (0, H - 1), (H - 1, 0)}
    top = tuple([n - 1] * (g.d - 2))
    hi, lo = g.idx.index(top + (n - 1,)), g.idx.index(top + (-(n - 1),))
    ent |= {(hi, lo), (lo, hi)}                                          # m' - m = +-(2 n_end - 2)
    flat = rng.choice(H * H, size=count, replace=False)
    return sorted(ent | {(int(e // H), int(e % H)) for e in flat}), (hi, lo)


@pytest.mark.parametrize("d,n_end", [(5, 7), (6, 5), (7, 4), (8, 3), (8, 4), (9, 3), (9, 4), (10, 3)])
def test_plan_term_lists_against_the_yardstick(d, n_end):
    lib = _lib.load()
    g = CY.gaunt(d, n_end)
    p, dd, H, Q, H2, nt = _plan(lib, d, n_end)
    try:
        assert (H, H2) == (g.H, g.H2)
        # (tidx addresses the labels of degree < 2 n_end - 1 in the order of the plan's own labels: test_chain_plan_tables)
        ptr = np.zeros(H * H + 1, dtype=np.int64)
        coef = np.zeros(nt)
        tidx = np.zeros(nt, dtype=np.int32)
        _lib.check(lib.biem_plan_terms(p, ptr.ctypes.data, coef.ctypes.data, tidx.ctypes.data))
        assert ptr[0] == 0 and ptr[-1] == nt and (np.diff(ptr) >= 0).all()
        assert tidx.min() >= 0 and tidx.max() < H2
    finally:
        lib.biem_plan_destroy(p)
    entries, (hi, lo) = _sample_entries(g, np.random.default_rng(100 * d + n_end))
    assert len(entries) >= 150
    worst, n_terms = 0.0, 0
    for hp, h in entries:
        e = h * H + hp                                                  # the plan's entry order: row h, column h'
        li, lc = tidx[ptr[e]:ptr[e + 1]], coef[ptr[e]:ptr[e + 1]]
        assert len(np.unique(li)) == len(li), ("a label is listed twice", g.idx[hp], g.idx[h])
        cand, gv = g.all_labels(hp, h)                                   # every label with m'' = m' - m, no cut, no sign
        sign = np.real(1j ** ((g.idx[h][0] + g.deg2[cand] - g.idx[hp][0]) % 4))
        carried = np.abs(gv) >= CY.G_SKIP
        assert np.all(np.abs(np.imag(1j ** ((g.idx[h][0] + g.deg2[cand[carried]] - g.idx[hp][0]) % 4))) == 0)
        yard = np.zeros(H2)
        yard[cand] = np.where(carried, sign * gv, 0.0)
        raw = np.zeros(H2)
        raw[cand] = np.abs(gv)
        listed = np.zeros(H2)
        listed[li] = lc
        must = np.nonzero(raw >= G_PRESENT)[0]
        assert np.isin(must, li).all(), ("a term is missing", g.idx[hp], g.idx[h], [g.idx2[i] for i in must[~np.isin(must, li)]])
        # every listed label: its coefficient is the yardstick's (carried), or the yardstick's G is below the cut and so is the coefficient
        assert (raw[li][~np.isin(li, cand[carried])] < CY.G_SKIP).all()
        err = np.abs(listed - yard).max() if H2 else 0.0
        worst = max(worst, err)
        n_terms += int(carried.sum())
        assert err <= COEF_TOL, (g.idx[hp], g.idx[h], err)
    # the extreme azimuthal difference holds exactly the labels with |m''| = 2 n_end - 2
    cand, gv = g.all_labels(hi, lo)
    assert len(cand) > 0 and all(g.idx2[i][-1] == 2 * n_end - 2 for i in cand) and (np.abs(gv) >= G_PRESENT).any()
    print(f"d {d} n_end {n_end}: {len(entries)} entries, {n_terms} terms, worst coefficient difference {worst:.2e}")
