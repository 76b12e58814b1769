"""The left-looking bulk update of the row-form symmetric factorisation A = U^T U (BIEM_SYM_UPDATE=left|right).

Right-looking (tests/test_gpu_dense_regimes.py models it): after every four-panel group a K = 256 update of the whole upper
triangle below.  Left-looking: immediately before group J is factored its (up to) 256 rows take all pending updates in one pass,

    A[J:J+256, J:n_cols] -= U[0:J, J:J+256]^T U[0:J, J:n_cols]          (K = J, tiles with tx >= ty only)

by k_gemm3m_pipe<0> (launch_gemm_left, kernels_gemm3m.hip), whose chunk count is a run-time value; the right-hand sides take the same
terms in k_rhs_update_left (nrhs <= 8, K walked in blocks of 256) or as tile columns of the same launch (nrhs > 8).

This module
  * models the left form's launches (tiles per launch, blk_sh, kd, band height) and the band order of its tiles, and checks on the
    CPU that the GPU case list below reaches every regime of it (two tile grids are worked by hand);
  * checks the selection rule (biem_sym_update_form) on the host;
  * runs the cases under both forms on the same data: U^T U = A, info, untouched poison, exact zeros in padding rows, backward
    residual, NumPy, and left against right.

Generators and tolerances are those of test_gpu_dense_regimes.py: complex symmetric (1 + 0.2i) I + E + E^T, unread lower tiles
poisoned with 1e30, backward residual 1e-13, 1e-12 against numpy.linalg.solve.
"""
import math

import numpy as np
import pytest

try:
    import torch
except ImportError:  # the schedule model needs no torch
    torch = None

gpu = pytest.mark.gpu

NB = 64                 # panel width = tile edge
GRID_CAP = 512          # persistent grid of the update kernels (GEMM_GRID_CAP)


def npad_of(N):
    return -(-N // NB) * NB


# ---------------------------------------------------------------------------- model of the left form (kernels_gemm3m.hip: sym_update_left, launch_gemm_left; kernels_sym.hip: launch_sym_factor_solve)
def band_tiles(h, tx_n):
    """Tiles of a band of h <= 4 tile rows and tx_n >= h tile columns with tx >= ty."""
    return h * (h + 1) // 2 + (tx_n - h) * h if tx_n >= h else tx_n * (tx_n + 1) // 2


def band_decode(r, h):
    """(ty, tx) of tile r of a system in the band order: column-major, column q < h holds the q + 1 tiles on and above the diagonal."""
    head = h * (h + 1) // 2
    if r < head:
        q = 0
        while r >= q + 1:
            r -= q + 1
            q += 1
        return r, q
    rem = r - head
    return rem % h, h + rem // h


def left_schedule(nb, n_pad, nrhs):
    """The K-long launches of launch_sym_factor_solve in the left form, one per group J > 0, and what the right-hand sides do."""
    n_cols = n_pad + nrhs
    rhs_gemv = 0 < nrhs <= 8
    out = []
    for J in range(4 * NB, n_pad, 4 * NB):
        row_end = min(J + 4 * NB, n_pad)
        col_end = n_pad if rhs_gemv else n_cols
        h, tx_n = (row_end - J) // NB, -(-(col_end - J) // NB)
        per_sys = band_tiles(h, tx_n)
        ntiles = per_sys * nb
        out.append(dict(J=J, kd=J, h=h, tx_n=tx_n, per_sys=per_sys, ntiles=ntiles, blk_sh=0 if ntiles <= GRID_CAP else 3 if ntiles < 2048 else 6,
                        grid=min((ntiles + 7) // 8 * 8, GRID_CAP), rhs_edge=col_end > n_pad and nrhs % NB != 0,
                        rhs_blocks=J // (4 * NB) if rhs_gemv else 0))
    return out


def update_form(nb, n_pad, nrhs, env=None):
    """sym_update_left: 1 = left.  Left when the smallest K-long launch (the last group's band) has a tile for every CU: half the
    persistent grid of two workgroups per CU."""
    if n_pad <= 4 * NB:
        return 0
    if env:
        return 1 if env[0] == "l" else 0
    T = n_pad // NB
    h_last = T % 4 or 4
    cols_last = h_last + (-(-nrhs // NB) if nrhs > 8 else 0)
    return 1 if 2 * band_tiles(h_last, cols_last) * nb >= GRID_CAP else 0


# (N, nb, nrhs): what each covers is asserted in test_left_cases_reach_every_regime
LEFT_CASES = [
    (832, 80, 1),        # groups 256 / 256 / 256 / 64: a last band of one tile row; persistent K-long launches
    (1000, 80, 1),       # padding rows
    (1000, 3, 12),       # right-hand sides through the gemm (an edge tile column); launches of at most 512 tiles
    (2048, 8, 2),        # K up to 1792; keep_w back substitution
    (1000, 80, 0),       # checks-only back pass
]


def test_band_order_two_grids_by_hand():
    # a full band, four tile rows and six tile columns: 1 + 2 + 3 + 4 tiles over the diagonal block, then two columns of four
    want = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3),
            (0, 4), (1, 4), (2, 4), (3, 4), (0, 5), (1, 5), (2, 5), (3, 5)]
    assert band_tiles(4, 6) == 18 and [band_decode(r, 4) for r in range(18)] == want
    # the last band of n_pad = 640 with 12 right-hand sides through the gemm: two tile rows, two matrix columns and the edge column
    want = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    assert band_tiles(2, 3) == 5 and [band_decode(r, 2) for r in range(5)] == want
    assert band_tiles(1, 1) == 1 and band_decode(0, 1) == (0, 0)
    assert band_tiles(3, 3) == 6 and [band_decode(r, 3) for r in range(6)] == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]
    # every band: each tile with tx >= ty exactly once; the cfg 3 launches are whole multiples of the 512-workgroup grid
    for h in (1, 2, 3, 4):
        for tx_n in range(h, 12):
            got = [band_decode(r, h) for r in range(band_tiles(h, tx_n))]
            assert sorted(got) == sorted((ty, tx) for tx in range(tx_n) for ty in range(h) if tx >= ty)
    for g in left_schedule(256, 6400, 1):
        assert g["per_sys"] == 4 * g["tx_n"] - 6 and g["ntiles"] % GRID_CAP == 0 and g["blk_sh"] == 6
    # the flop count is that of the right-looking form: sum over groups of tiles x K-256 units = sum over K = 256 launches of tiles
    T = 100
    left_units = sum(g["per_sys"] * g["kd"] // 256 for g in left_schedule(1, 6400, 1))
    right_units = sum((T - 4 * (i + 1)) * (T - 4 * (i + 1) + 1) // 2 for i in range(T // 4 - 1))
    assert left_units == right_units == 39800


def test_left_cases_reach_every_regime():
    got = set()
    for N, nb, nrhs in LEFT_CASES:
        n_pad = npad_of(N)
        for g in left_schedule(nb, n_pad, nrhs):
            got.add("persistent" if g["ntiles"] > GRID_CAP else "one_tile_per_workgroup")
            got.add(("blk_sh", g["blk_sh"]))
            if g["kd"] == 256:
                got.add("kd256")
            if g["kd"] >= 768:
                got.add("kd>=768")
            if g["h"] < 4:
                got.add("short_band")
            if g["rhs_edge"]:
                got.add("rhs_edge_column")
            if g["rhs_blocks"] > 1:
                got.add("rhs_update_several_blocks")
        if n_pad > N:
            got.add("padding")
        if nrhs == 0:
            got.add("checks_only")
        if nb <= 8 and nrhs:
            got.add("keep_w")
    want = {"persistent", "one_tile_per_workgroup", ("blk_sh", 0), ("blk_sh", 3), ("blk_sh", 6), "kd256", "kd>=768", "short_band",
            "rhs_edge_column", "rhs_update_several_blocks", "padding", "checks_only", "keep_w"}
    assert want <= got, want - got
    assert max(g["kd"] for g in left_schedule(8, 2048, 2)) == 1792
    assert [g["h"] for g in left_schedule(80, 832, 1)] == [4, 4, 1]


def test_selection_rule_on_the_host(monkeypatch):
    """biem_sym_update_form against the model: one system per call runs the right-looking form, the headline shape (N = 6400, 256
    systems) the left-looking one; BIEM_SYM_UPDATE forces either; a single group has no bulk update."""
    from biem_helmholtz_sphere_amd import _lib as L

    l = L.load()
    monkeypatch.delenv("BIEM_SYM_UPDATE", raising=False)
    assert l.biem_sym_update_form(1, 6400, 1) == 0
    assert l.biem_sym_update_form(256, 6400, 1) == 1
    assert l.biem_sym_update_form(8, 6400, 1) == 0 and l.biem_sym_update_form(32, 6400, 1) == 1          # as measured
    for nb in (1, 8, 25, 26, 32, 64, 128, 255, 256, 512):
        for n_pad in (256, 320, 576, 832, 1024, 4096, 6400):
            for nrhs in (0, 1, 8, 12, 70):
                assert l.biem_sym_update_form(nb, n_pad, nrhs) == update_form(nb, n_pad, nrhs), (nb, n_pad, nrhs)
    for env in ("left", "right"):
        monkeypatch.setenv("BIEM_SYM_UPDATE", env)
        for nb, n_pad in ((1, 6400), (256, 6400), (80, 832), (3, 256)):
            assert l.biem_sym_update_form(nb, n_pad, 1) == update_form(nb, n_pad, 1, env)


def test_isa_check_covers_the_k_long_kernel():
    """k_gemm3m_pipe<0> under the pins of the fixed-K instances: no scratch, no VGPR spills, 96 MFMAs in the chunk loop, only the
    ring's LDS-DMA and the result stores as vector-memory instructions (it reads no tile map)."""
    from biem_helmholtz_sphere_amd import _build, _lib

    _lib.load()
    r = _build.check_isa_klong()
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["mfma_in_chunk_loop"] == 96 and r["mfma_total"] == 96, r
    assert set(r["vm"]) == {"global_load_lds_dwordx4", "global_store_dwordx4"}, r


# ---------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def lib():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    from biem_helmholtz_sphere_amd import _lib as L

    return L.load(), L


CHUNK = 8


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


def _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed, spoil=None):
    """biem_sym_factor_solve under BIEM_SYM_UPDATE=form on the systems of `seed`; returns (A, info) on the device."""
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
    info = torch.ones(nb, dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(nb, n_pad, nrhs)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    monkeypatch.setenv("BIEM_SYM_UPDATE", form)
    assert l.biem_sym_update_form(nb, n_pad, nrhs) == update_form(nb, n_pad, nrhs, form)
    L.check(l.biem_sym_factor_solve(nb, n_pad, nrhs, A.data_ptr(), lda, n_pad * lda, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    return A, info


@gpu
@pytest.mark.parametrize("N,nb,nrhs", LEFT_CASES, ids=[f"N{c[0]}-nb{c[1]}-r{c[2]}" for c in LEFT_CASES])
def test_left_looking_factor_solve(lib, monkeypatch, N, nb, nrhs):
    """Both forms on the same data.  Every system under either form: info = 0, max|U^T U - A| < 1e-12 on the upper triangle, the
    poisoned lower tiles untouched, exact zeros in the solution's padding rows, backward residual < 1e-13; the first and last system
    against numpy.linalg.solve at 1e-12; the left solutions against the right ones at 1e-12 relative."""
    l, L = lib
    seed = 4242 + N + nb + nrhs
    n_pad = npad_of(N)
    poison = _lower_tiles(n_pad)
    X = {}
    for form in ("left", "right"):
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
        X[form] = x[:, :N, :].clone()
        del A
    if not nrhs:
        return
    d = (X["left"] - X["right"]).abs().amax(dim=(1, 2)) / X["right"].abs().amax(dim=(1, 2))
    assert (d < 1e-12).all(), (int(d.argmax()), d.max().item())
    for s in (0, nb - 1):
        c0 = s // CHUNK * CHUNK
        M, F = _gen(seed, N, nrhs, c0, min(c0 + CHUNK, nb))
        Xo = np.linalg.solve(M[s - c0].cpu().numpy(), F[s - c0].cpu().numpy())
        assert np.abs(X["left"][s].cpu().numpy() - Xo).max() / np.abs(Xo).max() < 1e-12, s


@gpu
def test_left_looking_rejections(lib, monkeypatch):
    """A pivot in row 300 far below a hundredth of an entry of its row (a multiplier above the limit) and a NaN entry in the third group:
    the same info codes under both forms (the multiplier: -(first row of the panel + 1) = -257), the neighbours in the batch
    factored and solved as if alone."""
    l, L = lib
    N, nb, nrhs, seed = 832, 6, 1, 99
    n_pad = npad_of(N)

    def spoil(A):
        # inside the diagonal block of the panel at row 256; the updates of the first group move the pivot by about 0.01 and leave
        # it far below a hundredth of the entry
        A[1, 300, 300] = 0.001
        A[1, 300, 310] = A[1, 310, 300] = 100.0
        A[4, 530, 600] = float("nan")             # rows 512 .. 767: the third group

    out = {}
    for form in ("left", "right"):
        A, info = _factor_solve(l, L, monkeypatch, form, N, nb, nrhs, seed, spoil)
        out[form] = (A[:, :N, n_pad].clone(), info.cpu().tolist())
    assert out["left"][1] == out["right"][1], out
    codes = out["left"][1]
    assert codes[1] == -257 and codes[4] < 0 and [codes[s] for s in (0, 2, 3, 5)] == [0, 0, 0, 0], codes
    M, F = _gen(seed, N, nrhs, 0, nb)
    for s in (0, 2, 3, 5):
        Xo = np.linalg.solve(M[s].cpu().numpy(), F[s].cpu().numpy())[:, 0]
        for form in ("left", "right"):
            assert np.abs(out[form][0][s].cpu().numpy() - Xo).max() / np.abs(Xo).max() < 1e-12, (form, s)


@gpu
def test_left_looking_stored_factor(lib, monkeypatch):
    """biem_sym_factor under the left form, then biem_sym_solve with three right-hand sides, against NumPy (N = 832, 5 systems)."""
    l, L = lib
    N, nb, nrhs = 832, 5, 3
    n_pad = npad_of(N)
    M, F = _gen(7, N, nrhs, 0, nb)
    A = torch.zeros((nb, n_pad, n_pad), dtype=torch.complex128, device="cuda")
    A[:, :N, :N] = M
    A.masked_fill_(_lower_tiles(n_pad), 1e30)
    info = torch.ones(nb, dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(nb, n_pad, 0)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    monkeypatch.setenv("BIEM_SYM_UPDATE", "left")
    L.check(l.biem_sym_factor(nb, n_pad, A.data_ptr(), n_pad, n_pad * n_pad, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    assert (info == 0).all()
    ldb = nrhs + 1
    X = torch.zeros((nb, n_pad, ldb), dtype=torch.complex128, device="cuda")
    X[:, :N, :nrhs] = F
    L.check(l.biem_sym_solve(nb, n_pad, nrhs, A.data_ptr(), n_pad, n_pad * n_pad, X.data_ptr(), ldb, n_pad * ldb, None))
    torch.cuda.synchronize()
    for s in range(nb):
        Xo = np.linalg.solve(M[s].cpu().numpy(), F[s].cpu().numpy())
        assert np.abs(X[s, :N, :nrhs].cpu().numpy() - Xo).max() / np.abs(Xo).max() < 1e-12, s


@gpu
def test_left_looking_end_to_end(monkeypatch):
    """biem() on four balls with n_end = 12 (N = 576: groups 256 / 256 / 64) at 12 wavenumbers with the left form forced, against
    the right form: densities to 1e-12 of each system's largest entry."""
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd
    from oracle import biem_oracle as O

    def dev(a):
        return torch.as_tensor(np.array(a), device="cuda").to(torch.float64).contiguous()

    ks = np.linspace(0.7, 4.0, 12)
    cen = O.grid_centers(1, 3)
    dirs = np.zeros((3, len(ks)))
    dirs[0] = 1.0
    c = amd.create_from_branching_types("ba")
    uin, _ = amd.plane_wave(k=dev(ks), direction=dev(dirs))
    dens = {}
    for form in ("left", "right"):
        monkeypatch.setenv("BIEM_SYM_UPDATE", form)
        calc = amd.biem(c, centers=dev(cen)[None], radii=dev(np.ones(4))[None], k=dev(ks), n_end=12, uin=uin)
        dens[form] = calc.density.clone()
    assert tuple(dens["left"].shape)[0] == 12 and bool(torch.isfinite(dens["left"].abs()).all())
    err = torch.amax(torch.abs(dens["left"] - dens["right"]), dim=(1, 2)) / torch.amax(torch.abs(dens["right"]), dim=(1, 2))
    assert float(err.max()) < 1e-12, (int(err.argmax()), float(err.max()))
