"""The plan's coupling table T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega at the orders biem_force() and uscat_hess() reach (no GPU).

tests/test_force_host.py holds the table against a dense d x H x H yardstick up to n_end 5.  Here it is read as SciPy CSR matrices
(never dense) at the ceilings of the field kernels and two orders above them, where the Hessian's ladder runs, and held to

- its structure (order, no repeats, |n - n'| = 1, Hermitian),
- the identities of the coordinate functions: sum_i y_i^2 = 1 and y_i y_j = y_j y_i on the degrees the truncation does not touch,
- the ladder twin of tests/hess_yardstick.py: sum_i D_i D_i c = -k^2 c,
- values that share neither the plan's rule nor its harmonics: closed forms (a, ba), the oracle tree's rule of order n_end + 1
  (the other trees, on a documented sample of rows where the whole table is too large),
- its distance to the plan's keep / refuse cuts (1e-14 / 1e-10).

Tolerances: the 1e-13 of tests/test_force_host.py (measured 2e-15 at n_end <= 5) does not carry over to these orders.  Every figure was measured on the yardstick's own table at an order where the dense one is
affordable and on the plan's table at every case; the asserted bound is 4 x the largest of these per tree family (the margin for
another libm or FMA contraction).  The measured figures are in MEASURED below and in DESIGN.md 5h.
"""
import math
import time

import numpy as np
import pytest
from scipy import sparse

import force_yardstick as FY
import hess_yardstick as HY

CHAINS = ["b" * (d - 2) + "a" for d in (7, 8, 9, 10)]
# the orders k_force and the Hessian's ladder run at: the ceilings of the field kernels (a 320, ba 48, bba 14, caa 12, bbba 8) and the
# plans two orders above them; the chains at the largest order tests/test_chain_trees_host.py builds
CASES = [("a", 320), ("a", 322), ("ba", 48), ("ba", 50), ("bba", 14), ("bba", 16), ("caa", 12), ("caa", 14), ("bbba", 8), ("bbba", 10),
         ("bbbba", 5)] + [(t, 3) for t in CHAINS]
# (tree, density order): the ladder runs in the plan of two orders more
LADDERS = [("a", 320), ("ba", 48), ("bba", 14), ("caa", 12), ("bbba", 8), ("bbbba", 3)] + [(t, 1) for t in CHAINS]
# where the yardstick's own dense table is affordable
AFFORDABLE = [("a", 40), ("ba", 12), ("bba", 8), ("caa", 8), ("bbba", 5), ("bbbba", 4), ("bbbbba", 3)]
FULL_BELOW = 256            # tables of fewer rows are compared whole, larger ones on sample_rows()
KEEP_CUT, REFUSE_CUT = 1e-14, 1e-10          # plan_build_force: kept above KEEP_CUT, the build fails between the two


def family(tree):
    return tree if tree in ("a", "ba", "bba", "caa") else "chain"


# Largest figure measured per family, over the plan's table at every case and the yardstick's own dense table at AFFORDABLE
# (identity: sum_i T^i T^i - I and [T^i, T^j]; value: plan - independent value, and T - T^H; ladder: |sum_i D_i D_i c + k^2 c| / k^2)
MEASURED = {"a": {"identity": 3.7e-15, "value": 3.0e-15, "ladder": 4.5e-15},
            "ba": {"identity": 3.8e-14, "value": 2.6e-14, "ladder": 5.5e-14},
            "bba": {"identity": 4.0e-14, "value": 2.7e-14, "ladder": 5.8e-14},
            "caa": {"identity": 1.3e-13, "value": 4.4e-14, "ladder": 1.4e-13},
            "chain": {"identity": 8.1e-14, "value": 6.4e-14, "ladder": 9.8e-14}}


def tol(tree, what):
    return 4.0 * MEASURED[family(tree)][what]


# ---------------------------------------------------------------------------- independent values
CLOSED = FY.CLOSED          # a, ba: closed forms (tests/force_yardstick.py)


def sample_rows(lab, deg, n_end, seed):
    """The rows h' the yardstick's rule is applied to where the whole table is too large: the first and last row of the top degree and
    16 random ones of it, the first and last row at either end of the range of every label entry (over all rows, and over the top
    degree), and 64 random rows, from a fixed seed.  Small tables are taken whole."""
    H = len(deg)
    if H < FULL_BELOW:
        return np.arange(H)
    rng = np.random.default_rng(seed)
    top = np.flatnonzero(deg == n_end - 1)
    picks = [top[[0, -1]], rng.choice(top, min(16, len(top)), replace=False), rng.choice(H, 64, replace=False)]
    for j in range(lab.shape[1]):
        for sel in (np.arange(H), top):
            for v in (lab[sel, j].min(), lab[sel, j].max()):
                picks.append(sel[lab[sel, j] == v][[0, -1]])
    rows = np.unique(np.concatenate(picks))
    assert len(rows) >= 64
    return rows


def candidates(lab, deg, rows):
    """[len(rows), H] mask of the pairs y_i can couple: |n - n'| = 1 and every label entry at most 1 apart (y_i has degree 1 in every
    sub-sphere of the tree).  Restated here from the labels, not read from the plan."""
    near = (np.abs(lab[rows][:, None, :].astype(np.int64) - lab[None, :, :]) <= 1).all(-1)
    return near & (np.abs(deg[rows][:, None].astype(np.int64) - deg[None, :]) == 1)


def identities(T, deg, n_end):
    """(max |sum_i T^i T^i - I|, max |[T^i, T^j]|) on the rows and columns of degree <= n_end - 2; T a list of CSR matrices."""
    low = np.flatnonzero(deg <= n_end - 2)
    if len(low) == 0:
        return 0.0, 0.0
    block = lambda M: M.tocsr()[low][:, low]
    S = block(sum(Ti @ Ti for Ti in T)) - sparse.identity(len(low), format="csr")
    comp = abs(S).max() if S.nnz else 0.0
    comm = 0.0
    for i in range(len(T)):
        for j in range(i):
            K = block(T[i] @ T[j] - T[j] @ T[i])
            comm = max(comm, abs(K).max() if K.nnz else 0.0)
    return float(comp), float(comm)


def max_abs(M):
    return float(abs(M).max()) if M.nnz else 0.0


def independent(tree, n_end, lab, deg):
    """(rows, ref): ref[i] CSR [H, H] holding the independent value of the rows `rows` on every candidate (a, ba: closed forms, every
    row), and for the rule-built trees off = the largest |yardstick value| outside the candidates of those rows."""
    H = len(deg)
    if tree in CLOSED:
        return np.arange(H), CLOSED[tree](n_end), 0.0
    rows = sample_rows(lab, deg, n_end, seed=1000 * len(tree) + n_end)
    chunk = max(256, (1 << 22) // H)
    dense = FY.coupling_rows(HY.oracle_tree(tree), n_end, rows, chunk)               # [d, R, H]
    cand = candidates(lab, deg, rows)
    off = float(np.abs(dense[:, ~cand]).max()) if (~cand).any() else 0.0
    r, c = np.nonzero(cand)
    return rows, [sparse.csr_matrix((dense[i][r, c], (rows[r], c)), shape=(H, H)) for i in range(dense.shape[0])], off


# ---------------------------------------------------------------------------- the closed forms and the yardstick themselves
@pytest.mark.parametrize("tree,n_end", AFFORDABLE)
def test_yardstick_and_closed_forms_where_the_dense_table_is_affordable(tree, n_end):
    """The identities on the yardstick's own dense table (the figure the tolerances start from), and the closed forms of a and ba
    against it: the closed forms are pinned by the oracle's harmonics before they judge the plan."""
    tr = HY.oracle_tree(tree)
    ref = FY.coupling(tr, n_end)
    deg = tr.degrees(n_end)
    T = [sparse.csr_matrix(np.where(np.abs(M) > KEEP_CUT, M, 0.0)) for M in ref]
    comp, comm = identities(T, deg, n_end)
    herm = np.abs(ref - np.conj(np.swapaxes(ref, 1, 2))).max()
    line = f"{tree} n_end {n_end} (yardstick, dense): completeness {comp:.1e}  commutators {comm:.1e}  Hermitian {herm:.1e}"
    assert comp <= tol(tree, "identity") and comm <= tol(tree, "identity") and herm <= tol(tree, "value"), line
    if tree in CLOSED:
        err = max(np.abs(c.toarray() - M).max() for c, M in zip(CLOSED[tree](n_end), ref))
        line += f"  |closed form - yardstick| {err:.1e}"
        assert err <= tol(tree, "value"), line
    print(line)


# ---------------------------------------------------------------------------- the plan's table
@pytest.mark.parametrize("tree,n_end", CASES)
def test_structure(tree, n_end):
    t0 = time.perf_counter()
    d, lab, deg, ptr, col, comp, val = HY.plan_terms(tree, n_end)
    built = time.perf_counter() - t0
    H = len(deg)
    idx = HY.oracle_tree(tree).index(n_end)
    assert (lab[:, :len(idx[0])] == np.array(idx)).all() and (lab[:, len(idx[0]):] == 0).all()    # the oracle's labels, in its order
    assert ptr[0] == 0 and ptr[-1] == len(col) == len(comp) == len(val) and (np.diff(ptr) >= 0).all()
    rows = np.repeat(np.arange(H), np.diff(ptr))
    assert ((0 <= col) & (col < H)).all() and ((0 <= comp) & (comp < d)).all()
    key = (rows.astype(np.int64) * d + comp) * H + col
    assert (np.diff(key) > 0).all()                                   # ordered by (row, component, column), so no entry twice
    assert (np.abs(deg[rows].astype(np.int64) - deg[col]) == 1).all()                              # nothing off |n - n'| = 1
    assert candidates(lab, deg, np.arange(H))[rows, col].all() if H < 4096 else True
    T = HY.plan_table_sparse(tree, n_end)[3]
    assert sum(Ti.nnz for Ti in T) == len(val)
    herm = max(max_abs(Ti - Ti.conj().T) for Ti in T)
    print(f"{tree} n_end {n_end}: H {H}, {len(val)} entries, Hermitian to {herm:.1e}  (host plan and table built in {built:.1f} s)")
    assert herm <= tol(tree, "value")


@pytest.mark.parametrize("tree,n_end", CASES)
def test_completeness_and_commutators(tree, n_end):
    """sum_i y_i^2 = 1 and y_i y_j = y_j y_i: sum_i T^i T^i = I and [T^i, T^j] = 0 on the degrees <= n_end - 2 (a product of two
    tables passes through one degree more, and the truncation takes only the top one away)."""
    _, _, deg, T = HY.plan_table_sparse(tree, n_end)
    comp, comm = identities(T, deg, n_end)
    print(f"{tree} n_end {n_end}: max |sum_i T^i T^i - I| {comp:.1e}  max |[T^i, T^j]| {comm:.1e}  (bound {tol(tree, 'identity'):.1e})")
    assert comp <= tol(tree, "identity") and comm <= tol(tree, "identity")


@pytest.mark.parametrize("tree,n_end", CASES)
def test_values_and_margin_to_the_cuts(tree, n_end):
    """Every entry of the compared rows against a value that shares neither the plan's rule nor its harmonics, the candidates the plan
    dropped included: those must be exact zeros of the independent value, and the smallest kept entry must stay clear of the band
    (1e-14, 1e-10) in which plan_build_force refuses to build.  The bound on the smallest kept entry: 1e-6, four decades above the
    band - the entries shrink with order and dimension (like 1 / (2.8 n_end) in ba), and one that came within a rounding-sized
    factor of the band would make the absolute cuts the wrong rule before it made them fail."""
    d, lab, deg, ptr, col, comp, val = HY.plan_terms(tree, n_end)
    T = HY.plan_table_sparse(tree, n_end)[3]
    rows, ref, off = independent(tree, n_end, lab, deg)
    pick = sparse.csr_matrix((np.ones(len(rows)), (rows, rows)), shape=(len(deg),) * 2)
    err = max(max_abs(pick @ Ti - Ri) for Ti, Ri in zip(T, ref))
    kept = float(np.abs(val).min()) if len(val) else math.inf
    dropped = 0.0
    for Ti, Ri in zip(T, ref):
        there = sparse.csr_matrix((np.ones(Ti.nnz), Ti.nonzero()), shape=Ti.shape)
        R = Ri.tocoo()
        gone = np.asarray(there[R.row, R.col]).ravel() == 0
        dropped = max(dropped, float(np.abs(R.data[gone]).max()) if gone.any() else 0.0)
    print(f"{tree} n_end {n_end}: {len(rows)} of {len(deg)} rows, |plan - independent| {err:.1e} (bound {tol(tree, 'value'):.1e})  smallest kept "
          f"{kept:.2e}  largest dropped candidate {dropped:.1e}  largest value off the candidates {off:.1e}")
    assert err <= tol(tree, "value")
    assert kept >= 1e4 * REFUSE_CUT
    assert dropped <= KEEP_CUT                                          # exact zeros: the residue of the yardstick's own rounding
    assert off <= tol(tree, "value")                                    # ... and so is everything the labels rule out
    if n_end > 1:
        assert (deg[rows] == n_end - 1).any()


@pytest.mark.parametrize("tree,n_end", LADDERS)
def test_ladder_twin_is_helmholtz(tree, n_end):
    """The NumPy ladder twin on the plan's table of order n_end + 2, with its n_src cuts: sum_i D_i D_i c = -k^2 c for a random
    density of order n_end with |c_h| = 1 in every degree (the expansion solves the Helmholtz equation whatever its coefficients)."""
    k = 1.3 + 0.4j
    H = len(HY.plan_terms(tree, n_end)[2])
    rng = np.random.default_rng(n_end)
    c = np.exp(2j * math.pi * rng.random((2, H)))
    c2, hc = HY.hessian_coefs(tree, n_end, k, c, sparse_table=True)
    err = float(np.abs(sum(hc[i, i] for i in range(hc.shape[0])) + k * k * c2).max() / abs(k * k))
    asym = float(np.abs(hc - np.swapaxes(hc, 0, 1)).max() / abs(k * k))
    print(f"{tree} density order {n_end}: |sum_i D_i D_i c + k^2 c| / |k|^2 {err:.1e}  |D_j D_i c - D_i D_j c| / |k|^2 {asym:.1e}  (bound {tol(tree, 'ladder'):.1e})")
    assert err <= tol(tree, "ladder") and asym <= tol(tree, "ladder")
