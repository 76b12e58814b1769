"""The stacked pass of the symmetric row form A = U^T U: under the left-looking bulk update the panels b, c, d of a four-panel group
take their pending updates and their solve as ONE pure product, U[p, tx] = -[S_J ; .. ; S_{p-64} ; V_p]^T A[J : p+64, tx]
(k_gemm3m_stack<128 / 192 / 256>, the slab blocks S_r = -U[r, p] V_p from k_sym_slab), instead of a C-streaming pending-update launch
followed by the K = 64 strip.  BIEM_SYM_GROUP=twopass forces the two-pass form under the left-looking update.

The generator and the tolerances are those of test_gpu_sym_fused_rhs.py: (1 + 0.2i) I + E + E^T with the unread lower tiles poisoned
with 1e30, max|U^T U - A| < 1e-12, backward residual < 1e-13, 1e-12 against numpy.linalg.solve.  Every case runs under
BIEM_SYM_UPDATE=left, stacked and forced two-pass:

  (200, 5, 3)    one group (no bulk update, so no stacked pass either: both settings run the same launches), padding, keep_w
  (320, 130, 2)  a group plus one panel
  (448, 20, 1)   a group plus three panels: the stacked pass at K = 128, 192 and 256 over the last columns
  (832, 80, 1)   persistent launches
  (1000, 3, 12)  right-hand sides as tile columns, edge tile column
  (832, 80, 0)   no right-hand side
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
CASES = [(200, 5, 3), (320, 130, 2), (448, 20, 1), (832, 80, 1), (1000, 3, 12), (832, 80, 0)]
GROUP_FORMS = ("stacked", "twopass")


def npad_of(N):
    return -(-N // NB) * NB


def test_isa_check_reports_the_stacked_kernels():
    """CPU: k_gemm3m_stack<128 / 192 / 256> under the pins of the strip kernel - no scratch, no spills, 96 MFMAs in one loop, 24 LDS-DMA,
    65 stores, 5 loads of the right-hand-side epilogue - with no tile-map load and no v_readlane / v_writelane in the chunk loop; the
    reports of the other update kernels are what they were."""
    from biem_helmholtz_sphere_amd import _build, _lib

    _lib.load()
    rep = _build.check_isa_stack()
    slab = rep.pop(_build.SLAB)
    assert slab["scratch_bytes"] == 0 and slab["vgpr_spills"] == 0, slab      # the head kernel of every stacked pass
    assert sorted(rep) == [128, 192, 256]
    for kd, r in rep.items():
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["mfma_in_chunk_loop"] == 96 and r["mfma_total"] == 96, (kd, r)
        assert r["vm"] == {"global_load_lds_dwordx4": 24, "global_store_dwordx4": 65, "global_load_dwordx4": 5}, (kd, r)
        assert r["lane_spill_ops_in_chunk_loop"] == 0, (kd, r)
    assert sorted(_build.check_isa()) == [64, 128, 192, 256]
    r = _build.check_isa_strip()
    assert r["vm"]["global_load_lds_dwordx4"] == 24 and r["vm"]["global_store_dwordx4"] == 65 and r["vm"]["global_load_dwordx4"] == 5, r
    r = _build.check_isa_klong()
    assert set(r["vm"]) == {"global_load_lds_dwordx4", "global_store_dwordx4"} and r["lane_spill_ops_in_chunk_loop"] == 0, r


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


def _factor_solve(l, L, monkeypatch, group, N, nb, nrhs, seed, spoil=None, systems=None):
    """biem_sym_factor_solve under BIEM_SYM_UPDATE=left and BIEM_SYM_GROUP=group on the systems of `seed` (all, or the listed ones)."""
    n_pad = npad_of(N)
    lda = n_pad + ((nrhs + 7) // 8) * 8
    A = torch.zeros((nb, n_pad, lda), dtype=torch.complex128, device="cuda")
    pad = torch.arange(N, n_pad, device="cuda")
    poison = _lower_tiles(n_pad)
    for c0, c1 in _chunks(nb):
        M, F = _gen(seed, N, nrhs, c0, c1)
        A[c0:c1, :N, :N] = M
        A[c0:c1, pad, pad] = 1.0
        if nrhs:
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
    monkeypatch.setenv("BIEM_SYM_UPDATE", "left")
    monkeypatch.setenv("BIEM_SYM_GROUP", group)
    L.check(l.biem_sym_factor_solve(A.shape[0], n_pad, nrhs, A.data_ptr(), lda, n_pad * lda, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    return A, info


@gpu
@pytest.mark.parametrize("N,nb,nrhs", CASES, ids=[f"N{c[0]}-nb{c[1]}-r{c[2]}" for c in CASES])
def test_stacked_group_factor_solve(lib, monkeypatch, N, nb, nrhs):
    """Both group forms on the same data.  Every system under either form: info = 0, max|U^T U - A| < 1e-12, the poisoned lower tiles
    untouched, exact zeros in the solution's padding rows, backward residual < 1e-13, and the same call a second time gives torch.equal
    factors and solutions; the first and last system against numpy.linalg.solve at 1e-12; stacked against two-pass at 1e-12 relative
    (solutions, and the factors entry by entry against each system's largest).  With more than one group the two forms are different
    arithmetic, so their factors are not bit for bit the same: the switch is seen to switch."""
    l, L = lib
    seed = 6100 + N + nb + nrhs
    n_pad = npad_of(N)
    poison = _lower_tiles(n_pad)
    upper = ~poison
    X, Uf = {}, {}
    for group in GROUP_FORMS:
        A, info = _factor_solve(l, L, monkeypatch, group, N, nb, nrhs, seed)
        assert (info == 0).all(), (group, torch.nonzero(info).flatten()[:16].tolist())
        assert bool((A[:, :, :n_pad][:, poison] == 1e30).all()), group
        x = A[:, :, n_pad:n_pad + nrhs]
        if nrhs and n_pad > N:
            assert x[:, N:, :].abs().max().item() == 0.0, group
        for c0, c1 in _chunks(nb):
            M, F = _gen(seed, N, nrhs, c0, c1)
            U = torch.triu(A[c0:c1, :N, :N])
            err = (torch.bmm(U.transpose(1, 2), U) - M).abs().amax(dim=(1, 2))
            print(f"{group} systems {c0}..{c1 - 1}: max|U^T U - A| = {err.max().item():.3e}")
            assert (err < 1e-12).all(), (group, c0, err.max().item())
            if nrhs:
                xs = x[c0:c1, :N, :]
                res = (torch.bmm(M, xs) - F).abs().amax(dim=(1, 2)) / (M.abs().sum(dim=2).amax(dim=1) * xs.abs().amax(dim=(1, 2)))
                print(f"{group} systems {c0}..{c1 - 1}: backward residual = {res.max().item():.3e}")
                assert (res < 1e-13).all(), (group, c0, res.max().item())
            del M, F, U
        X[group] = x.clone()
        Uf[group] = A[:, :, :n_pad].clone()
        del A
        A2, info2 = _factor_solve(l, L, monkeypatch, group, N, nb, nrhs, seed)
        assert (info2 == 0).all(), group
        assert torch.equal(A2[:, :, n_pad:n_pad + nrhs], X[group]), group
        assert torch.equal(A2[:, :, :n_pad], Uf[group]), group
        del A2
    du = torch.where(upper, (Uf["stacked"] - Uf["twopass"]).abs(), torch.zeros((), dtype=torch.float64, device="cuda")).amax(dim=(1, 2))
    du = du / torch.where(upper, Uf["twopass"].abs(), torch.zeros((), dtype=torch.float64, device="cuda")).amax(dim=(1, 2))
    print(f"factors, stacked against two-pass: {du.max().item():.3e}")
    assert (du < 1e-12).all(), (int(du.argmax()), du.max().item())
    if n_pad > 4 * NB:
        assert not torch.equal(Uf["stacked"], Uf["twopass"])
    else:
        assert torch.equal(Uf["stacked"], Uf["twopass"])        # one group: no bulk update, the same launches
    del Uf
    if not nrhs:
        return
    d = (X["stacked"][:, :N] - X["twopass"][:, :N]).abs().amax(dim=(1, 2)) / X["twopass"][:, :N].abs().amax(dim=(1, 2))
    print(f"solutions, stacked against two-pass: {d.max().item():.3e}")
    assert (d < 1e-12).all(), (int(d.argmax()), d.max().item())
    for s in (0, nb - 1):
        c0 = s // CHUNK * CHUNK
        M, F = _gen(seed, N, nrhs, c0, min(c0 + CHUNK, nb))
        Xo = np.linalg.solve(M[s - c0].cpu().numpy(), F[s - c0].cpu().numpy())
        for group in GROUP_FORMS:
            e = np.abs(X[group][s, :N].cpu().numpy() - Xo).max() / np.abs(Xo).max()
            print(f"{group} system {s} against numpy.linalg.solve: {e:.3e}")
            assert e < 1e-12, (group, s, e)


@gpu
@pytest.mark.parametrize("row0", [320, 384, 448], ids=["panel-b", "panel-c", "panel-d"])
def test_spoiled_pivot_in_a_stacked_panel(lib, monkeypatch, row0):
    """One system of six with a pivot far below a hundredth of an entry of its row, inside panel b, c or d of the second group of
    N = 832 (rows 320+, 384+, 448+): its info is -(first row of the panel + 1) under the stacked form as under the two-pass form, and
    every other system comes out bit for bit as in a run without the spoiled system - nothing of a rejected (possibly NaN) system
    leaves it, neither through the slab nor through the right-hand sides."""
    l, L = lib
    N, nb, nrhs, seed = 832, 6, 1, 99
    n_pad = npad_of(N)
    others = [0, 2, 3, 4, 5]
    r = row0 + 44

    def spoil(A):
        A[1, r, r] = 0.001
        A[1, r, r + 10] = A[1, r + 10, r] = 100.0

    for group in GROUP_FORMS:
        A, info = _factor_solve(l, L, monkeypatch, group, N, nb, nrhs, seed, spoil)
        codes = info.cpu().tolist()
        assert codes[1] == -(row0 + 1) and [codes[s] for s in others] == [0] * 5, (group, codes)
        B, info_b = _factor_solve(l, L, monkeypatch, group, N, nb, nrhs, seed, systems=others)
        assert (info_b == 0).all(), group
        assert torch.equal(A[others], B), group
        assert bool(torch.isfinite(torch.view_as_real(B[:, :N, n_pad])).all()), group
