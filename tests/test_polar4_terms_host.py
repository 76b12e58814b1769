"""The translation term lists of the 4-D trees, term by term, against tests/polar4_yardstick.py (no GPU).

A bba plan at n_end 22 holds hundreds of millions of terms, so nothing here builds one: `biem_plan_entry_terms` returns the list of one
entry by the code the plan build runs (the last test ties the two together where plans are small).  Per case - bba, bpbpa (bba in
permuted axes: the same lists) and caa at every order of the fixture - 150 entries by the recipe of the chain test (corners, the extreme
azimuthal differences, seeded random entries) and 50 entries with both degrees n_end - 1 whose polar integrals the fixture holds at 40
digits.  The one condition is |listed - exact| <= COEF_TOL over EVERY label of degree < 2 n_end - 1, an unlisted label counting as
zero: it forbids dropping a term that matters and carrying a spurious one alike.  `exact` is the yardstick's coefficient (no selection
rule, no cut; the 40-digit polar integrals where the fixture holds the pair).  COEF_TOL is four times the accuracy the float64
integrals were measured to have (the Gaunt factor of at most one half, and a 2 n_end- against a 3 n_end + 3-node rule), capped at the
chain test's 1e-13.

With the absolute cuts the builder used to have (1e-12 / 1e-14) bba and bpbpa fail at n_end 22 and 24: see the docstring of
test_entry_term_lists_against_the_yardstick.
"""
import ctypes as C

import numpy as np
import pytest

from biem_helmholtz_sphere_amd import _coords, _lib

import polar4_yardstick as PY
from test_polar4_yardstick_host import CASES, POLAR_FP64_ACCURACY, fixture_case

COEF_TOL = min(4.0 * POLAR_FP64_ACCURACY, 1e-13)
CAP = 4096


def _entry(lib, tree, n_end, hp, h, coef, tidx):
    n = C.c_int()
    _lib.check(lib.biem_plan_entry_terms(_lib.TREE_IDS[tree], n_end, hp, h, CAP, C.byref(n), coef.ctypes.data, tidx.ctypes.data), "biem_plan_entry_terms")
    return tidx[:n.value].copy(), coef[:n.value].copy()


def _top(y, sign):
    n = y.n_end
    return y.idx.index((n - 1, n - 1, sign * (n - 1))) if y.name == "bba" else [y.idx.index((n - 1, sign * (n - 1), 0)), y.idx.index((n - 1, 0, sign * (n - 1)))]


def _sample_entries(y, lab, val, pairs, rng, count=150, top=50):
    """(entries by the chain test's recipe, entries with both degrees n_end - 1 drawn from the fixture's pairs: every other one from the
    pairs that hold a non-vanishing integral below 1e-12, where there are any)"""
    H, n = y.H, y.n_end
    ent = {(H - 1, H - 1), (0, H - 1), (H - 1, 0)}
    hi, lo = np.atleast_1d(_top(y, 1)), np.atleast_1d(_top(y, -1))
    ent |= {(int(a), int(b)) for a, b in zip(hi, lo)} | {(int(b), int(a)) for a, b in zip(hi, lo)}     # m' - m = +-(2 n_end - 2)
    flat = rng.choice(H * H, size=count, replace=False)
    ent |= {(int(e // H), int(e % H)) for e in flat}
    w = pairs.shape[1] // 2
    both = [r for r in pairs.tolist() if r[0] == n - 1 and r[w] == n - 1]
    assert both, "the fixture holds no pair with both degrees n_end - 1"
    tiny = {tuple(r[:2 * w]) for r, v in zip(lab.tolist(), val) if 0 < abs(v) < 1e-12}
    small = [r for r in both if tuple(r) in tiny] or both
    tops = set()
    while len(tops) < top:
        src = small if len(tops) % 2 else both
        r = src[rng.integers(len(src))]
        A, B = (r[:w], r[w:]) if rng.integers(2) else (r[w:], r[:w])
        if y.name == "bba":
            lab2 = [(A[0], A[1], int(rng.integers(-A[1], A[1] + 1))), (B[0], B[1], int(rng.integers(-B[1], B[1] + 1)))]
        else:
            lab2 = [(L[0], int(rng.choice([-1, 1])) * L[1], int(rng.choice([-1, 1])) * L[2]) for L in (A, B)]
        tops.add((y.idx.index(lab2[0]), y.idx.index(lab2[1])))
    return sorted(ent), sorted(tops)


def _polar_of(y, hp, h):
    """the polar integral behind every label of degree < 2 n_end - 1 of the entry (bba: A4; caa: I3)"""
    out = np.full(y.H2, np.inf)
    if y.name == "bba":
        (qp, lp, mp), (q, l, m) = y.idx[hp], y.idx[h]
        A4 = y.polar(qp, lp, q, l)
        for i, (q2, l2, m2) in enumerate(y.idx2):
            if m2 == mp - m:
                out[i] = A4[q2, l2]
    else:
        (qp, m1p, m2p), (q, m1, m2) = y.idx[hp], y.idx[h]
        q3, I3 = y.polar(qp, abs(m1p), abs(m2p), q, abs(m1), abs(m2), abs(m1p - m1), abs(m2p - m2))
        for n3, v in zip(q3, I3):
            out[y.pos2[(int(n3), m1p - m1, m2p - m2)]] = v
    return out


@pytest.mark.parametrize("tree,n_end", CASES + [("bpbpa", n) for t, n in CASES if t == "bba"])
def test_entry_term_lists_against_the_yardstick(tree, n_end):
    """With the cuts the builder had before (polar integrals below 1e-12 and products below 1e-14 dropped for bba, below 1e-14 for caa;
    run as this per-entry code with those cuts put back, since the builder before had no per-entry function) this fails for bba and
    bpbpa at n_end 22 and 24 and passes everywhere else: terms are missing whose exact coefficients reach 2.41e-13 at n_end 22 (entry
    (21,21,21) x (21,21,21), label (42,4,0)) and 1.18e-13 (bba) / 1.53e-13 (bpbpa) at n_end 24, against COEF_TOL = 1e-13.  Without the
    cuts the worst |listed - exact| of any case is 3.2e-15."""
    lib = _lib.load()
    lib_tree = _coords.CANONICAL.get(tree, (tree,))[0]
    assert lib_tree in ("bba", "caa")
    y = (PY.Bba if lib_tree == "bba" else PY.Caa)(n_end)
    lab, val, zero, pairs = fixture_case(lib_tree, n_end)
    PY.pin_fixture(y, lab, val, pairs)
    rng = np.random.default_rng(1000 * n_end + len(tree))
    # (bba from n_end 22 on: 150 top-degree entries, not 50 - with 50 the sample at n_end 24 held no coefficient above COEF_TOL on a
    # polar integral below 1e-12, and could not have seen an absolute cut there)
    n_top = 150 if lib_tree == "bba" and n_end >= 22 else 50
    entries, tops = _sample_entries(y, lab, val, pairs, rng, top=n_top)
    assert len(entries) >= 150 and len(tops) == n_top
    coef, tidx = np.zeros(CAP), np.zeros(CAP, dtype=np.int32)
    worst, worst_at, n_terms, small = 0.0, None, 0, 0
    for hp, h in entries + tops:
        li, lc = _entry(lib, lib_tree, n_end, hp, h, coef, tidx)
        assert len(np.unique(li)) == len(li), ("a label is listed twice", y.idx[hp], y.idx[h])
        assert len(li) == 0 or (li.min() >= 0 and li.max() < y.H2)
        exact = PY.coefficients(y, hp, h)
        listed = np.zeros(y.H2)
        listed[li] = lc
        err = np.abs(listed - exact)
        if err.max() > worst:
            worst, worst_at = err.max(), (y.idx[hp], y.idx[h], y.idx2[int(err.argmax())], exact[err.argmax()], listed[err.argmax()])
        n_terms += len(li)
        if (hp, h) in tops:                                             # coefficients that matter on a polar integral below 1e-12
            small += int(((np.abs(exact) > COEF_TOL) & (np.abs(_polar_of(y, hp, h)) < 1e-12)).sum())
    print(f"{tree} n_end {n_end}: {len(entries) + len(tops)} entries, {n_terms} listed terms, worst |listed - exact| {worst:.2e} at {worst_at}; "
          f"{small} exact coefficients above COEF_TOL {COEF_TOL:.1e} on polar integrals below 1e-12 among the top-degree entries")
    if lib_tree == "bba" and n_end >= 22:
        assert small > 0, "the sample holds no coefficient an absolute cut of 1e-12 would drop"
    assert worst <= COEF_TOL, worst_at


@pytest.mark.parametrize("tree,n_end", [(t, n) for t in ("bba", "caa") for n in (1, 2, 3, 5, 6, 8)])
def test_entry_terms_are_the_slices_of_a_built_plan(tree, n_end):
    lib = _lib.load()
    p = C.c_void_p()
    _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS[tree], n_end, C.byref(p)), "biem_plan_create_host")
    try:
        H, nt = C.c_int(), C.c_longlong()
        _lib.check(lib.biem_plan_info(p, None, C.byref(H), None, None, C.byref(nt)))
        H, nt = H.value, nt.value
        ptr, coef, tidx = np.zeros(H * H + 1, dtype=np.int64), np.zeros(nt), np.zeros(nt, dtype=np.int32)
        _lib.check(lib.biem_plan_terms(p, ptr.ctypes.data, coef.ctypes.data, tidx.ctypes.data))
    finally:
        lib.biem_plan_destroy(p)
    c1, t1 = np.zeros(CAP), np.zeros(CAP, dtype=np.int32)
    for h in range(H):
        for hp in range(H):
            e = h * H + hp                                              # the plan's entry order: row h, column h'
            li, lc = _entry(lib, tree, n_end, hp, h, c1, t1)
            assert np.array_equal(li, tidx[ptr[e]:ptr[e + 1]]) and np.array_equal(lc, coef[ptr[e]:ptr[e + 1]]), (tree, n_end, hp, h)


def test_entry_terms_status_codes():
    lib = _lib.load()
    n = C.c_int()
    c1, t1 = np.zeros(4), np.zeros(4, dtype=np.int32)
    assert lib.biem_plan_entry_terms(1, 4, 0, 0, 4, C.byref(n), c1.ctypes.data, t1.ctypes.data) == 3 and b"bba, caa" in lib.biem_last_error()
    assert lib.biem_plan_entry_terms(2, 4, 0, 30, 4, C.byref(n), c1.ctypes.data, t1.ctypes.data) == 1 and b"outside" in lib.biem_last_error()
    H = 30                                                              # bba n_end 4
    assert lib.biem_plan_entry_terms(2, 4, H - 1, H - 1, 4, C.byref(n), c1.ctypes.data, t1.ctypes.data) == 1 and n.value > 4 and b"capacity" in lib.biem_last_error()
    assert (c1 == 0).all()
