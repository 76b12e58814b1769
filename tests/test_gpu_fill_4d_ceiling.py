"""The general fill of the 4-D trees on either side of its pair-table switch, against a reference that shares nothing with it.

`build_entry_chunks` (plan_fill.cpp) keeps the pair table T[h''] of a ball pair in LDS while 16 (H2 + 2 H) bytes leave room for a term
slice, which for the 4-D trees (H = 819 / 1015 / 1240, H2 = 5525 / 6930 / 8432 at n_end 13 / 14 / 15) holds up to n_end 13; from 14 on
the kernel reads the table from global memory.  Cases: bba and bpbpa (bba in permuted axes) at 13, 14, 15, caa at 13, 14.

Reference: `O.assemble` with the translation coefficients of tests/polar4_yardstick.py - float64 with a 3 n_end + 3-node rule, no
selection rule and no cut, pinned by 40-digit integrals (tests/test_polar4_yardstick_host.py).  The oracle's own `_theta4` / `_theta_c`
tables play no part.  Per off-diagonal block 400 entries: the corners, 100 in the rows and 100 in the columns of the top degree, and
seeded random ones; the diagonal blocks whole.

Assertions and their numbers are those of test_matrix_attribute_beyond_the_lds_ceiling (tests/test_gpu_configs.py), on the argument
of its docstring: norm-wise 1e-12 of the block's largest sampled entry; element-wise 1e-9 relative where n + n' <= 20 (beyond that an
entry is an alternating sum of terms far above its value and carries no information in double precision); exact zeros off the diagonal
of a ball's own block.
"""
import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd
from oracle import biem_oracle as O

import polar4_yardstick as PY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [("bba", 13), ("bba", 14), ("bba", 15), ("bpbpa", 13), ("bpbpa", 14), ("bpbpa", 15), ("caa", 13), ("caa", 14)]
KS = np.array([1.3, 1.1 + 0.15j])
ETA = np.array([0.7, 1.0])
ALPHA, BETA = 1.0 + 0.25j, 0.4 - 0.1j
CEN = np.array([[0.0, 1.3, 0.2, -0.4], [0.3, -1.4, -0.1, 0.5]])
RAD = np.array([1.0, 0.8])


def t(a):
    return torch.as_tensor(np.asarray(a), device=DEV)


def _samples(deg, rng, count=400):
    H = len(deg)
    top = np.nonzero(deg == deg.max())[0]
    ent = [(0, 0), (H - 1, H - 1), (0, H - 1), (H - 1, 0)]
    ent += [(int(rng.choice(top)), int(rng.integers(H))) for _ in range(100)]
    ent += [(int(rng.integers(H)), int(rng.choice(top))) for _ in range(100)]
    ent = set(ent)
    while len(ent) < count:
        ent.add((int(rng.integers(H)), int(rng.integers(H))))
    return np.array(sorted(ent))


@pytest.mark.parametrize("tree,n_end", CASES)
def test_general_fill_vs_polar4_yardstick(tree, n_end):
    tr = O.tree(tree)
    deg = tr.degrees(n_end)
    H = len(deg)
    c = amd.create_from_branching_types(tree)
    calc = amd.biem(c, centers=t(CEN)[None].expand(2, 2, 4), radii=t(RAD)[None].expand(2, 2), k=t(KS), eta=t(ETA), n_end=n_end, alpha=ALPHA, beta=BETA)
    M = calc.matrix.cpu().numpy()
    assert M.shape == (2, 2, H, 2, H)
    rng = np.random.default_rng(100 * n_end + len(tree))
    samples = [_samples(deg, rng), _samples(deg, rng)]
    low = (deg[:, None] + deg[None, :]) <= 20
    worst_norm, worst_rel = 0.0, 0.0
    for s in range(2):
        k = KS[s] if KS[s].imag != 0 else float(KS[s].real)
        A, _ = O.assemble(tr, n_end, k, ETA[s], CEN, RAD, np.full(2, ALPHA), np.full(2, BETA), sr_func=PY.sampled_sr_func(lambda i: samples[i % 2]))
        for b in range(2):
            for bp in range(2):
                Mb, Ab = M[s, b, :, bp, :], A[b, :, bp, :]
                have = ~np.isnan(Ab)
                assert have.sum() == (H * H if b == bp else 400)
                Ab = np.where(have, Ab, 0)
                nrm = np.abs(Mb - Ab)[have].max() / np.abs(Ab[have]).max()
                nz = have & (np.abs(Ab) > 1e-200)
                assert (nz & low).any()
                rel = np.max(np.abs(Mb - Ab)[nz & low] / np.abs(Ab)[nz & low])
                worst_norm, worst_rel = max(worst_norm, nrm), max(worst_rel, rel)
                print(f"{tree} n_end {n_end} k {k} block ({b}, {bp}): norm-wise {nrm:.2e}, element-wise (n + n' <= 20, {int((nz & low).sum())} entries) {rel:.2e}")
                assert nrm < 1e-12, (s, b, bp)
                assert rel < 1e-9, (s, b, bp)
                if b == bp:
                    assert np.all(Mb[~nz] == 0)                 # a ball's own block: exactly diagonal
    print(f"{tree} n_end {n_end}: worst norm-wise error {worst_norm:.2e}, worst element-wise error {worst_rel:.2e}")
