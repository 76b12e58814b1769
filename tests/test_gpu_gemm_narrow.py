"""The narrow launch of the left-looking bulk update on the GPU: BIEM_GEMM_NARROW=1 against =0 on the same data.

A tile of the last tile column multiplies only the NF column groups that hold active columns (k_gemm3m_narrow<NF>); for every active
entry that is the MFMA sequence of the full tile on the same fragments, and the skipped products are exact zeros.  So X, info and the
active part of U keep their bits; the padding columns may differ in the sign of a zero only.

Cases (nb = 8, BIEM_SYM_UPDATE=left, through biem_sym_factor_solve_n):
  * n_pad = 576: the band at J = 256 is four tile rows by five tile columns (the narrow tiles are its last column of four), the band
    at J = 512 one diagonal tile, which is the narrow launch alone;
  * n_pad = 512: the band at J = 256 is 4 x 4, the last column lies inside its triangular head (six tiles stay in the main launch);
  * padding 0, 15, 16, 32, 48, 63 columns: NF = whole, whole, 3, 2, 1, 1;
  * nrhs = 0 and 1, both group forms (BIEM_SYM_GROUP=twopass|stacked).
Generator and tolerance against numpy.linalg.solve are those of tests/test_gpu_sym_left_looking.py: complex symmetric
(1 + 0.2i) I + E + E^T, unread lower tiles poisoned with 1e30, 1e-12 of the largest entry of the solution.
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
NSYS = 8
PADS = {0: 4, 15: 4, 16: 3, 32: 2, 48: 1, 63: 1}     # padding columns -> NF (4: the launch stays whole)


@pytest.fixture(scope="module")
def lib():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    from biem_helmholtz_sphere_amd import _lib as L

    return L.load(), L


_SYSTEMS = {}


def _systems(N):
    """NSYS seeded systems of order N with one right-hand side each, and their NumPy solutions: made once per N, never changed."""
    if N not in _SYSTEMS:
        g = torch.Generator(device="cuda")
        g.manual_seed(770000 + N)
        M = torch.view_as_complex(torch.randn((NSYS, N, N, 2), dtype=torch.float64, device="cuda", generator=g))
        F = torch.view_as_complex(torch.randn((NSYS, N, 1, 2), dtype=torch.float64, device="cuda", generator=g))
        M *= 0.12 / math.sqrt(N)
        M = M + M.transpose(1, 2)
        M.diagonal(dim1=1, dim2=2).add_(1.0 + 0.2j)
        _SYSTEMS[N] = (M, F, np.linalg.solve(M.cpu().numpy(), F.cpu().numpy()))
    return _SYSTEMS[N]


def _lower_tiles(n_pad):
    blk = torch.arange(n_pad, device="cuda") // NB
    return blk[:, None] > blk[None, :]


def _run(l, L, monkeypatch, narrow, group, n_pad, n_active, nrhs, spoil=None):
    """biem_sym_factor_solve_n under BIEM_GEMM_NARROW=narrow; returns (A, info) on the device."""
    M, F, _ = _systems(n_active)
    lda = n_pad + 8
    A = torch.zeros((NSYS, n_pad, lda), dtype=torch.complex128, device="cuda")
    A[:, :n_active, :n_active] = M
    pad = torch.arange(n_active, n_pad, device="cuda")
    A[:, pad, pad] = 1.0
    if nrhs:
        A[:, :n_active, n_pad:n_pad + 1] = F
    A[:, :, :n_pad].masked_fill_(_lower_tiles(n_pad), 1e30)
    if spoil is not None:
        spoil(A)
    info = torch.ones(NSYS, dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(NSYS, n_pad, nrhs)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    monkeypatch.setenv("BIEM_SYM_UPDATE", "left")
    monkeypatch.setenv("BIEM_SYM_GROUP", group)
    monkeypatch.setenv("BIEM_GEMM_NARROW", narrow)
    L.check(l.biem_sym_factor_solve_n(NSYS, n_pad, n_active, nrhs, A.data_ptr(), lda, n_pad * lda, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    return A, info


def _bits(t):
    return torch.view_as_real(t.contiguous()).view(torch.int64)


@gpu
@pytest.mark.parametrize("pad", sorted(PADS), ids=[f"pad{p}" for p in sorted(PADS)])
@pytest.mark.parametrize("n_pad", (576, 512), ids=("band4x5_then_one_tile", "last_column_in_the_head"))
def test_narrow_launch_keeps_the_bits(lib, monkeypatch, n_pad, pad):
    l, L = lib
    n_active = n_pad - pad
    monkeypatch.setenv("BIEM_GEMM_NARROW", "1")
    assert [l.biem_gemm_narrow_frags(NSYS, n_pad, n_active, J) for J in range(256, n_pad, 256)] == [PADS[pad]] * ((n_pad - 1) // 256)
    monkeypatch.setenv("BIEM_GEMM_NARROW", "0")
    assert l.biem_gemm_narrow_frags(NSYS, n_pad, n_active, 256) == 4
    monkeypatch.delenv("BIEM_GEMM_NARROW")
    assert l.biem_gemm_narrow_frags(NSYS, n_pad, n_active, 256) == 4                         # 32 narrow tiles: the size rule
    assert l.biem_gemm_narrow_frags(NSYS, 576, 576 - pad, 512) == PADS[pad]                  # the whole band: no size rule
    poison = _lower_tiles(n_pad)
    Xo = _systems(n_active)[2]
    for group in ("twopass", "stacked"):
        for nrhs in (0, 1):
            A1, info1 = _run(l, L, monkeypatch, "1", group, n_pad, n_active, nrhs)
            A0, info0 = _run(l, L, monkeypatch, "0", group, n_pad, n_active, nrhs)
            where = (group, nrhs)
            assert info1.tolist() == info0.tolist() == [0] * NSYS, where
            assert torch.equal(_bits(A1[:, :, :n_active]), _bits(A0[:, :, :n_active])), where      # the active part of U (and the poison)
            assert bool((A1[:, :, n_active:n_pad] == A0[:, :, n_active:n_pad]).all()), where       # padding columns: equal, up to the sign of zero
            assert bool((A1[:, :, :n_pad][:, poison] == 1e30).all()), where
            if nrhs:
                assert torch.equal(_bits(A1[:, :, n_pad]), _bits(A0[:, :, n_pad])), where
                X = A1[:, :n_active, n_pad:n_pad + 1].cpu().numpy()
                err = np.abs(X - Xo).max(axis=(1, 2)) / np.abs(Xo).max(axis=(1, 2))
                assert (err < 1e-12).all(), (where, err.max())
                if pad:
                    assert A1[:, n_active:, n_pad].abs().max().item() == 0.0, where


@gpu
def test_narrow_launch_with_a_rejected_system(lib, monkeypatch):
    """System 3 has a zeroed pivot row (and column) in the second group: both settings report the same codes, the other systems are
    solved as if alone - X bit for bit equal between the settings, and to 1e-12 of NumPy."""
    l, L = lib
    n_pad, n_active = 576, 544

    def spoil(A):
        A[3, 300, :n_pad] = 0.0
        A[3, :300, 300] = 0.0

    A1, info1 = _run(l, L, monkeypatch, "1", "stacked", n_pad, n_active, 1, spoil)
    A0, info0 = _run(l, L, monkeypatch, "0", "stacked", n_pad, n_active, 1, spoil)
    codes = info1.tolist()
    assert codes == info0.tolist(), (codes, info0.tolist())
    assert codes[3] < 0 and [c for s, c in enumerate(codes) if s != 3] == [0] * (NSYS - 1), codes
    ok = [s for s in range(NSYS) if s != 3]
    assert torch.equal(_bits(A1[ok][:, :, n_pad]), _bits(A0[ok][:, :, n_pad]))
    Xo = _systems(n_active)[2]
    X = A1[:, :n_active, n_pad:n_pad + 1].cpu().numpy()
    for s in ok:
        assert np.abs(X[s] - Xo[s]).max() / np.abs(Xo[s]).max() < 1e-12, s
