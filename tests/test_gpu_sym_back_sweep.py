"""The row-form back substitution as one launch per group of right-hand sides (k_back_sweep) against the per-block launches it
replaces (k_back_row, BIEM_BACK_ROW=blocks): the same arithmetic in the same order, so solutions, info and the growth slots are
compared bit for bit.

Through biem_sym_factor_solve, as tests/test_gpu_sym_left_looking.py calls it, on seeded complex-symmetric matrices with a dominant
diagonal (the generator of test_gpu_dense_regimes.py), under BIEM_BACK_FORM=row.  BIEM_NO_SMALL_PATH is set as well: without it the
one-block case would run in the LDS-resident launch and never reach the back substitution.  (n_pad, n_active, systems, nrhs):

  (64, 64, 3, 1)     one block row: the loop body once, no strip
  (128, 128, 3, 2)   the first hand-over of prefetched entries
  (320, 300, 5, 3)   odd block count, identity padding, the four-wide instantiation with three right-hand sides
  (832, 832, 70, 8)  three groups and a short band; more systems than the column form takes, so the default rule picks the row form too
                     (the case runs without BIEM_BACK_FORM)
  (320, 320, 3, 9)   two passes, 8 + 1
  (320, 320, 3, 0)   the checks alone

The default run against numpy.linalg.solve: 1e-12 relative on the first and the last system, the rule of test_gpu_dense_regimes.py for
complex-symmetric matrices.

Rejections (n_pad = 320, five block rows; the matrices are checked on the CPU first, with a NumPy factorisation, to trip the intended
test and no other): a strip entry beyond the multiplier limit of 100 in block row 1 gives -(64 + 1); such entries in block rows 1 and 3
give the code of block row 3 (the sweep goes bottom up, the first writer wins); strip entries that alone exceed BIEM_LDLT_GROWTH_MAX
give -(n_pad + 1).  The same codes under both settings.
"""
import ctypes as C
import math

import numpy as np
import pytest

try:
    import torch
except ImportError:
    torch = None

gpu = pytest.mark.gpu

NB = 64
CASES = [(64, 64, 3, 1), (128, 128, 3, 2), (320, 300, 5, 3), (832, 832, 70, 8), (320, 320, 3, 9), (320, 320, 3, 0)]
SWITCHES = ("BIEM_SYM_UPDATE", "BIEM_SYM_GROUP", "BIEM_BACK_FORM", "BIEM_DIAG_FORM", "BIEM_NO_SMALL_PATH", "BIEM_BACK_ROW",
            "BIEM_LDLT_PIVOT_REL", "BIEM_LDLT_GROWTH_MAX")
MULT_LIMIT = 100.0          # 1 / NOPIV_REL (ldlt_thresholds)


@pytest.fixture(scope="module")
def lib():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    from biem_helmholtz_sphere_amd import _lib as L

    return L.load(), L


def _gen(seed, N, nrhs, nb):
    """Complex symmetric (1 + 0.2i) I + E + E^T and right-hand sides, on the CPU (test_gpu_dense_regimes._gen's recipe)."""
    rng = np.random.default_rng(seed)
    M = (rng.standard_normal((nb, N, N)) + 1j * rng.standard_normal((nb, N, N))) * (0.12 / math.sqrt(N))
    M = M + M.transpose(0, 2, 1)
    M[:, np.arange(N), np.arange(N)] += 1.0 + 0.2j
    F = rng.standard_normal((nb, N, nrhs)) + 1j * rng.standard_normal((nb, N, nrhs))
    return M, F


def _run(l, L, monkeypatch, env, M, F, n_pad):
    """biem_sym_factor_solve on the systems M (n_active rows, identity padding up to n_pad) under `env`; returns the solutions, info and
    the growth slots as bit patterns."""
    nb, N, nrhs = M.shape[0], M.shape[1], F.shape[2]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    lda = n_pad + ((nrhs + 7) // 8) * 8
    A = torch.zeros((nb, n_pad, lda), dtype=torch.complex128, device="cuda")
    A[:, :N, :N] = torch.as_tensor(M, device="cuda")
    pad = torch.arange(N, n_pad, device="cuda")
    A[:, pad, pad] = 1.0
    if nrhs:
        A[:, :N, n_pad:n_pad + nrhs] = torch.as_tensor(F, device="cuda")
    blk = torch.arange(n_pad, device="cuda") // NB
    A[:, :, :n_pad].masked_fill_(blk[:, None] > blk[None, :], 1e30)         # the tiles the row form promises not to read
    info = torch.ones(nb, dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(nb, n_pad, nrhs)
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    form, where = (C.c_int * 9)(), (C.c_size_t * 11)()
    L.check(l.biem_sym_form(nb, n_pad, n_pad, nrhs, form, where))
    assert form[0] == 0 and form[6] == 0, list(form)                        # the blocked path, back substitution in row form
    L.check(l.biem_sym_factor_solve(nb, n_pad, nrhs, A.data_ptr(), lda, n_pad * lda, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    slots = work[where[3]:where[3] + 16 * nb].clone().view(torch.int64)
    return A[:, :, n_pad:n_pad + nrhs].clone(), info.cpu().tolist(), slots


@gpu
@pytest.mark.parametrize("n_pad,N,nb,nrhs", CASES, ids=[f"n{c[0]}-a{c[1]}-nb{c[2]}-r{c[3]}" for c in CASES])
def test_sweep_equals_the_per_block_launches(lib, monkeypatch, n_pad, N, nb, nrhs):
    l, L = lib
    M, F = _gen(8100 + n_pad + nb + nrhs, N, nrhs, nb)
    base = {"BIEM_NO_SMALL_PATH": "1"} if nb > 64 else {"BIEM_NO_SMALL_PATH": "1", "BIEM_BACK_FORM": "row"}
    X, info, slots = _run(l, L, monkeypatch, base, M, F, n_pad)
    Xb, info_b, slots_b = _run(l, L, monkeypatch, {**base, "BIEM_BACK_ROW": "blocks"}, M, F, n_pad)
    assert info == [0] * nb and info_b == info, (info, info_b)
    assert torch.equal(X, Xb)
    assert torch.equal(slots, slots_b)
    if not nrhs:
        return
    if n_pad > N:
        assert X[:, N:, :].abs().max().item() == 0.0
    for s in (0, nb - 1):
        Xo = np.linalg.solve(M[s], F[s])
        e = np.abs(X[s, :N].cpu().numpy() - Xo).max() / np.abs(Xo).max()
        print(f"system {s} against numpy.linalg.solve: {e:.3e}")
        assert e < 1e-12, (s, e)


# ---------------------------------------------------------------------------- rejections
def _utu(A):
    """U of A = U^T U without interchanges (principal square roots of the pivots), as the row form computes it."""
    S = np.array(A, dtype=np.complex128)
    n = S.shape[0]
    U = np.zeros_like(S)
    for i in range(n):
        U[i, i:] = S[i, i:] / np.sqrt(S[i, i])
        S[i + 1:, i + 1:] -= np.outer(U[i, i + 1:], U[i, i + 1:])
    return U


def _measures(A):
    """Of the factor of A: per block row the largest strip multiplier |u_ic| / |u_ii|; the largest in-block multiplier in the 1-norm
    measure of the diagonal-block kernel; the largest |u_ii u_ic| over the strips and over the diagonal blocks; max |a_ij|."""
    U = _utu(A)
    n = A.shape[0]
    d = np.abs(np.diag(U))
    strip_mult, strip_g, blk_mult, blk_g = [], 0.0, 0.0, 0.0
    cabs1 = lambda z: np.abs(z.real) + np.abs(z.imag)  # noqa: E731
    for b in range(n // NB):
        r0, r1 = b * NB, (b + 1) * NB
        strip = np.abs(U[r0:r1, r1:])
        strip_mult.append(float((strip / d[r0:r1, None]).max()) if strip.size else 0.0)
        if strip.size:
            strip_g = max(strip_g, float((strip * d[r0:r1, None]).max()))
        T = np.triu(U[r0:r1, r0:r1]) * np.diag(U)[r0:r1, None]               # d_i l_ci = u_ii u_ic, the pivot itself on the diagonal
        blk_g = max(blk_g, float(np.abs(T).max()))
        off = np.triu(T, 1)
        blk_mult = max(blk_mult, float((cabs1(off) / cabs1(np.diag(T))[:, None]).max()))
    return strip_mult, blk_mult, strip_g, blk_g, float(np.abs(np.triu(A)).max())


def _with_big_multipliers(M, rows):
    """M with its factor's entry (i, c) raised to 150 u_ii for every (i, c) of `rows`: built from the factor, so nothing else moves."""
    U = _utu(M)
    for i, c in rows:
        U[i, c] = 150.0 * U[i, i]
    return U.T @ U


@gpu
def test_sweep_rejections(lib, monkeypatch):
    l, L = lib
    n_pad, nb = 320, 3
    M, F = _gen(977, n_pad, 1, nb)
    one, two, grow = M.copy(), M.copy(), M.copy()
    one[1] = _with_big_multipliers(M[1], [(84, 200)])                       # block row 1, a column of block row 3
    two[1] = _with_big_multipliers(M[1], [(84, 200), (202, 300)])           # and block row 3, a column of block row 4
    # two strip entries of block row 1 in one column whose squares cancel in that column's pivot: 3 and 3i over a diagonal near 1
    grow[1, 84, 200] = grow[1, 200, 84] = 3.0
    grow[1, 90, 200] = grow[1, 200, 90] = 3.0j
    grow[1, 84, 90] = grow[1, 90, 84] = 0.0
    growth_limit = 0.5
    # on the CPU: each matrix trips the intended test and no other (the untouched systems none)
    for A, bad_rows in ((M[0], []), (M[2], []), (one[1], [1]), (two[1], [1, 3]), (grow[1], [])):
        strip_mult, blk_mult, strip_g, blk_g, amax = _measures(A)
        assert [b for b, m in enumerate(strip_mult) if m > MULT_LIMIT] == bad_rows, strip_mult
        assert all(m > 1.2 * MULT_LIMIT for b, m in enumerate(strip_mult) if b in bad_rows), strip_mult
        assert all(m < 0.5 * MULT_LIMIT for b, m in enumerate(strip_mult) if b not in bad_rows), strip_mult
        assert blk_mult < 0.5 * MULT_LIMIT, blk_mult
        assert max(strip_g, blk_g) < 0.5 * 200.0 * amax                     # far inside the default growth limit
    strip_mult, blk_mult, strip_g, blk_g, amax = _measures(grow[1])
    assert strip_g > 1.5 * growth_limit * amax and blk_g < growth_limit * amax / 1.2, (strip_g, blk_g, amax)
    row = {"BIEM_NO_SMALL_PATH": "1", "BIEM_BACK_FORM": "row"}
    for mats, env, want in ((one, {}, -(64 + 1)), (two, {}, -(192 + 1)), (grow, {"BIEM_LDLT_GROWTH_MAX": str(growth_limit)}, -(n_pad + 1)),
                            (grow, {}, 0)):
        got = {}
        for blocks in (False, True):
            e = {**row, **env, **({"BIEM_BACK_ROW": "blocks"} if blocks else {})}
            X, info, slots = _run(l, L, monkeypatch, e, mats, F, n_pad)
            got[blocks] = (X, info, slots)
            # under the lowered growth limit the neighbours (max |u_ii u_ic| near max |a_ij|) are rejected as well: only system 1 is looked at
            assert info[1] == want, (env, blocks, info)
            if not env:
                assert info[0] == 0 and info[2] == 0, (blocks, info)
        assert got[False][1] == got[True][1]
        assert torch.equal(got[False][2], got[True][2])
        assert torch.equal(got[False][0][[0, 2]], got[True][0][[0, 2]])
