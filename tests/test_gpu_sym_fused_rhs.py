"""The symmetric row form A = U^T U with the strip pass as a pure product (k_gemm3m_strip: U12 = -V^T C, V = -U11^{-T}) that carries the
forward substitution of up to 8 right-hand sides: the compact copy Y[s][q][row] is made first, every diagonal-block kernel solves its
own 64 entries, every strip tile takes its 64 columns' term from the tile in registers, and no second pass reads U.

The generator and the tolerances are those of test_gpu_dense_regimes.py: (1 + 0.2i) I + E + E^T with the unread lower tiles poisoned
with 1e30, max|U^T U - A| < 1e-12, backward residual < 1e-13, 1e-12 against numpy.linalg.solve.  Every case runs under
BIEM_SYM_UPDATE=left and =right.  The shapes are the smallest that take each path of the strip and of the right-hand sides:

  (200, 5, 3)    one group, strips only, keep_w (W = I + V kept beside V for k_back_step), padding to 256
  (320, 20, 2)   column-block back substitution without keep_w: Y is copied back to the augmented columns first
  (320, 130, 2)  two groups, last band one tile row, row-form back substitution
  (600, 3, 8)    eight right-hand sides, one tile per workgroup
  (832, 80, 1)   persistent launches, three full groups and a one-row band
  (1000, 3, 12)  right-hand sides as tile columns, (832, 80, 0) factorisation alone
"""
import math

import numpy as np
import pytest

try:
    import torch
except ImportError:
    torch = None

gpu = pytest.mark.gpu

NB = 64
CHUNK = 8
CASES = [(200, 5, 3), (320, 20, 2), (320, 130, 2), (600, 3, 8), (832, 80, 1), (1000, 3, 12), (832, 80, 0)]
FORMS = ("left", "right")


def npad_of(N):
    return -(-N // NB) * NB


def test_isa_check_reports_the_strip_kernel():
    """CPU: check_isa pins k_gemm3m_strip like the other update kernels - no scratch, no spills, 96 MFMAs in one loop, 24 LDS-DMA (six
    groups of four: no C slice anywhere) - and the exact set of other vector-memory instructions of its epilogue: the tile-map loads,
    5 global_load_dwordx4 (z_j of four rows, Y) and 65 stores (four forms of the 16 result stores, Y), none of them in the chunk
    loop; it still returns the reports of the fixed-K instances."""
    from biem_helmholtz_sphere_amd import _build, _lib

    _lib.load()
    rep = _build.check_isa()
    assert sorted(rep) == [64, 128, 192, 256]
    for kd, r in rep.items():
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["mfma_in_chunk_loop"] == 96, (kd, r)
    r = _build.check_isa_strip()
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["mfma_in_chunk_loop"] == 96 and r["mfma_total"] == 96, r
    assert set(r["vm"]) == {"global_load_lds_dwordx4", "global_load_dword", "global_load_dwordx4", "global_store_dwordx4"}, r
    assert r["vm"]["global_load_lds_dwordx4"] == 24 and r["vm"]["global_store_dwordx4"] == 65 and r["vm"]["global_load_dwordx4"] == 5, r
    assert r["vm"]["global_load_dword"] <= 2, r


@pytest.fixture(scope="module")
def lib():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    from biem_helmholtz_sphere_amd import _lib as L

    return L.load(), L


def _gen(seed, N, nrhs, c0, c1):
    """The clean systems c0 .. c1-1 on the device (test_gpu_dense_regimes._gen, complex symmetric)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 100003 + c0 // CHUNK)
    n = c1 - c0
    M = torch.view_as_complex(torch.randn((n, N, N, 2), dtype=torch.float64, device="cuda", generator=g))
    F = torch.view_as_complex(torch.randn((n, N, nrhs, 2), dtype=torch.float64, device="cuda", generator=g))
    M *= 0.12 / math.sqrt(N)
    M = M + M.transpose(1, 2)
    M.diagonal(dim1=1, dim2=2).add_(1.0 + 0.2j)
    return M, F


def _chunks(nb):
    return [(c0, min(c0 + CHUNK, nb)) for c0 in range(0, nb, CHUNK)]


def _lower_tiles(n_pad):
    blk = torch.arange(n_pad, device="cuda") // NB
    return blk[:, None] > blk[None, :]


def _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed, spoil=None, zero_rhs=False, systems=None):
    """biem_sym_factor_solve under BIEM_SYM_UPDATE=form on the systems of `seed` (all nb of them, or the listed ones); (A, info)."""
    n_pad = npad_of(N)
    lda = n_pad + ((nrhs + 7) // 8) * 8
    A = torch.zeros((nb, n_pad, lda), dtype=torch.complex128, device="cuda")
    pad = torch.arange(N, n_pad, device="cuda")
    poison = _lower_tiles(n_pad)
    for c0, c1 in _chunks(nb):
        M, F = _gen(seed, N, nrhs, c0, c1)
        A[c0:c1, :N, :N] = M
        A[c0:c1, pad, pad] = 1.0
        if nrhs and not zero_rhs:
            A[c0:c1, :N, n_pad:n_pad + nrhs] = F
        A[c0:c1, :, :n_pad].masked_fill_(poison, 1e30)
        del M, F
    if spoil is not None:
        spoil(A)
    if systems is not None:
        A = A[systems].contiguous()
    info = torch.ones(A.shape[0], dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(A.shape[0], n_pad, nrhs)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    monkeypatch.setenv("BIEM_SYM_UPDATE", form)
    L.check(l.biem_sym_factor_solve(A.shape[0], n_pad, nrhs, A.data_ptr(), lda, n_pad * lda, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    return A, info


@gpu
@pytest.mark.parametrize("N,nb,nrhs", CASES, ids=[f"N{c[0]}-nb{c[1]}-r{c[2]}" for c in CASES])
def test_strip_product_factor_solve(lib, monkeypatch, N, nb, nrhs):
    """Both forms on the same data.  Every system under either form: info = 0, max|U^T U - A| < 1e-12, the poisoned lower tiles
    untouched, exact zeros in the solution's padding rows, backward residual < 1e-13, and the same call a second time gives
    torch.equal solutions; the first and last system against numpy.linalg.solve at 1e-12; left against right at 1e-12 relative."""
    l, L = lib
    seed = 5150 + N + nb + nrhs
    n_pad = npad_of(N)
    poison = _lower_tiles(n_pad)
    X = {}
    for form in FORMS:
        A, info = _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed)
        assert (info == 0).all(), (form, torch.nonzero(info).flatten()[:16].tolist())
        assert bool((A[:, :, :n_pad][:, poison] == 1e30).all()), form
        x = A[:, :, n_pad:n_pad + nrhs]
        if nrhs and n_pad > N:
            assert x[:, N:, :].abs().max().item() == 0.0, form
        for c0, c1 in _chunks(nb):
            M, F = _gen(seed, N, nrhs, c0, c1)
            U = torch.triu(A[c0:c1, :N, :N])
            err = (torch.bmm(U.transpose(1, 2), U) - M).abs().amax(dim=(1, 2))
            assert (err < 1e-12).all(), (form, c0, err.max().item())
            if nrhs:
                xs = x[c0:c1, :N, :]
                res = (torch.bmm(M, xs) - F).abs().amax(dim=(1, 2)) / (M.abs().sum(dim=2).amax(dim=1) * xs.abs().amax(dim=(1, 2)))
                assert (res < 1e-13).all(), (form, c0, res.max().item())
            del M, F, U
        X[form] = x.clone()
        U1 = A[:, :, :n_pad].clone()
        del A
        A2, info2 = _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed)
        assert (info2 == 0).all(), form
        assert torch.equal(A2[:, :, n_pad:n_pad + nrhs], X[form]), form
        assert torch.equal(A2[:, :, :n_pad], U1), form
        del A2, U1
    if not nrhs:
        return
    d = (X["left"][:, :N] - X["right"][:, :N]).abs().amax(dim=(1, 2)) / X["right"][:, :N].abs().amax(dim=(1, 2))
    assert (d < 1e-12).all(), (int(d.argmax()), d.max().item())
    for s in (0, nb - 1):
        c0 = s // CHUNK * CHUNK
        M, F = _gen(seed, N, nrhs, c0, min(c0 + CHUNK, nb))
        Xo = np.linalg.solve(M[s - c0].cpu().numpy(), F[s - c0].cpu().numpy())
        for form in FORMS:
            assert np.abs(X[form][s, :N].cpu().numpy() - Xo).max() / np.abs(Xo).max() < 1e-12, (form, s)


@gpu
@pytest.mark.parametrize("N,nb,nrhs", [(200, 5, 3), (832, 80, 1)], ids=["N200-nb5-r3", "N832-nb80-r1"])
def test_zero_right_hand_side_gives_exact_zeros(lib, monkeypatch, N, nb, nrhs):
    """A zero right-hand side comes back as exact zeros under either form (keep_w and row-form back substitution)."""
    l, L = lib
    n_pad = npad_of(N)
    for form in FORMS:
        A, info = _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, 77, zero_rhs=True)
        assert (info == 0).all(), form
        assert A[:, :, n_pad:n_pad + nrhs].abs().max().item() == 0.0, form


@gpu
def test_spoiled_pivot_stays_in_its_system(lib, monkeypatch):
    """One system of six with a pivot far below a hundredth of an entry of its row (test_left_looking_rejections): its info is
    -(first row of the panel + 1) = -257 under either form, and every other system's solution is bit for bit the solution of a run
    without the spoiled system - nothing of a rejected (possibly NaN) system leaves it."""
    l, L = lib
    N, nb, nrhs, seed = 832, 6, 1, 99
    n_pad = npad_of(N)
    others = [0, 2, 3, 4, 5]

    def spoil(A):
        A[1, 300, 300] = 0.001
        A[1, 300, 310] = A[1, 310, 300] = 100.0

    for form in FORMS:
        A, info = _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed, spoil)
        codes = info.cpu().tolist()
        assert codes[1] == -257 and [codes[s] for s in others] == [0] * 5, (form, codes)
        B, info_b = _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed, systems=others)
        assert (info_b == 0).all(), form
        assert torch.equal(A[others][:, :, n_pad:n_pad + nrhs], B[:, :, n_pad:n_pad + nrhs]), form
        assert bool(torch.isfinite(torch.view_as_real(B[:, :N, n_pad])).all()), form
