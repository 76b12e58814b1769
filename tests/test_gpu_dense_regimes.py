"""The dense solvers against NumPy in the launch regimes the production shapes run.

The random-matrix tests in test_gpu_parity.py solve small batches: none of their update launches exceeds 512 tiles, so none takes
the persistent path of launch_gemm_stream (a workgroup walking several tiles in blocks of 8 or 64, its LDS-DMA producer running
across tile boundaries), and no call spans 2^31 elements.  The headline step runs almost only there.  This module

  * models the update schedule of the factorisations (which gemm launches, with how many tiles, in which regime) after
    biem_helmholtz_sphere_amd/csrc/kernels_{gemm3m,sym,lu}.hip, and checks on the CPU that the case lists below reach every regime;
  * runs those cases on the GPU with entry-wise checks: backward residual and info of every system, U^T U = A of every system
    (row-form symmetric path), exact zeros in the padding rows of the solution, and numpy.linalg.solve on a few systems;
  * drives the one-launch small-system kernel (k_small_utu) through biem_sym_factor_solve_n with NaN in the padding it promises
    not to touch, against NumPy and against the blocked path on the same systems.

Tolerances are those of test_gpu_parity.py: 1e-13 backward residual, 1e-12 for complex-symmetric and 1e-9 for Gaussian matrices.
"""
import ctypes as C
import math

import numpy as np
import pytest

try:
    import torch
except ImportError:  # the schedule model and its coverage test need no torch
    torch = None

gpu = pytest.mark.gpu

# ---------------------------------------------------------------------------- schedule model (csrc/kernels_gemm3m.hip, kernels_sym.hip, kernels_lu.hip)
NB = 64                  # panel width, tile edge BM3 = BN3 (dense.hpp; kernels_gemm3m.hip)
SMALL_N_MAX, SMALL_RHS_MAX, SMALL_THREADS = 128, 8, 512     # kernels_sym.hip, at k_small_utu


def npad_of(N):
    return -(-N // NB) * NB                                          # lu_npad, kernels_lu.hip


def gemm_launch(kind, nb, row_begin, row_end, col_begin, col_end, kd, tri=0):
    """One launch_gemm_stream call (kernels_gemm3m.hip, with finish_tile_grid): its tile grid and persistent-block regime, or None if empty."""
    rrows, rcols = row_end - row_begin, col_end - col_begin
    if rrows <= 0 or rcols <= 0:
        return None
    ty_n, tx_n = -(-rrows // NB), -(-rcols // NB)
    per_sys = ty_n * (ty_n + 1) // 2 if tri else ty_n * tx_n
    ntiles = per_sys * nb
    blk_sh = 0 if ntiles <= 512 else 3 if ntiles < 2048 else 6      # finish_tile_grid
    return dict(kind=kind, kd=kd, tri=tri, ty_n=ty_n, tx_n=tx_n, per_sys=per_sys, ntiles=ntiles, blk_sh=blk_sh,
                full_bands=ty_n // 8, grid=min((ntiles + 7) // 8 * 8, 512), col_end=col_end, rcols=rcols)   # finish_tile_grid


def sym_small_path(n_active, nrhs, no_small=False):
    """sym_small_path, kernels_sym.hip (BIEM_NO_SMALL_PATH switches it off)."""
    lds = (n_active * (n_active + 1) // 2 + n_active * nrhs + 4 * n_active) * 16          # small_utu_lds
    return (0 < n_active <= SMALL_N_MAX and nrhs <= SMALL_RHS_MAX and n_active + nrhs <= 128 and lds <= 160 * 1024 - 2048
            and not no_small)


def small_instance(n_active, nrhs):
    """The k_small_utu<KR, TWO> instantiation launch_sym_factor_solve picks (kernels_sym.hip, at BIEM_SMALL)."""
    two = n_active + nrhs > 64
    kr = -(-n_active // (SMALL_THREADS // 64))
    if not two:
        return (4, False) if kr <= 4 else (8, False)
    for k in (8, 9, 12):
        if kr <= k:
            return (k, True)
    return (16, True)


def sym_schedule(nb, n_pad, nrhs, n_active=None, no_small=False, back_form=None):
    """launch_sym_factor_solve (row form A = U^T U, kernels_sym.hip; the form: sym_form there) with the right-looking bulk update.
    no_small: BIEM_NO_SMALL_PATH is set; back_form: the value of BIEM_BACK_FORM (row, col or step), None: not set."""
    n_active = n_pad if n_active is None else n_active
    if sym_small_path(n_active, nrhs, no_small):
        return dict(small=small_instance(n_active, nrhs), launches=[], back=None)
    n_cols = n_pad + nrhs
    rhs_gemv = 0 < nrhs <= 8
    col_form = nb <= 64 if back_form is None else back_form[0] in "cs"
    keep_w = col_form and 0 < nrhs <= 3 * NB and (nb <= 8 if back_form is None else back_form[0] == "s")
    back = "keep_w" if keep_w else "col" if (nrhs > 4 * NB or (col_form and nrhs > 0)) else "row"
    out = []

    def add(*a, **k):
        g = gemm_launch(*a, **k)
        if g:
            out.append(g)

    def panel(j):                                                                  # its `panel` lambda
        if n_cols > j + NB:
            add("panel", nb, j, j + NB, j + NB, n_cols, NB)

    for J in range(0, n_pad, 4 * NB):
        panel(J)
        for q in range(1, 4):
            jq = J + q * NB
            if jq >= n_pad:
                break
            add("in_group", nb, jq, jq + NB, jq, n_cols, q * NB)
            panel(jq)
        if J + 4 * NB >= n_pad:
            break
        add("k256", nb, J + 4 * NB, n_pad, J + 4 * NB, n_pad, 4 * NB, tri=2)       # (upper triangle of tiles)
        if not rhs_gemv and nrhs > 0:
            add("rhs", nb, J + 4 * NB, n_pad, n_pad, n_cols, 4 * NB)
    return dict(small=None, launches=out, back=back, rhs_gemv=rhs_gemv, keep_w=keep_w)


def lu_schedule(nb, n_pad, nrhs, symmetric=False):
    """launch_lu_factor_solve (kernels_lu.hip): the pivoted LU, or its column form L D L^T (symmetric=True)."""
    n_cols = n_pad + nrhs
    out = []

    def add(*a, **k):
        g = gemm_launch(*a, **k)
        if g:
            out.append(g)

    def trsm(j, col_begin=None):                                                   # its `trsm` lambda
        col_begin = j + NB if col_begin is None else col_begin
        add("trsm", nb, j, j + NB, col_begin, n_cols, NB)

    if symmetric:
        rhs_gemv = 0 < nrhs <= 8

        def u_rows_sym(j, pc):                                                     # its `u_rows_sym` lambda
            if not rhs_gemv and nrhs > 0:
                if pc > 0:
                    add("rhs", nb, j, j + NB, n_pad, n_cols, pc)
                trsm(j, n_pad)

        for J in range(0, n_pad, 4 * NB):
            u_rows_sym(J, 0)
            for q in range(1, 4):
                jq = J + q * NB
                if jq >= n_pad:
                    break
                add("in_group", nb, jq, n_pad, jq, jq + NB, q * NB)
                u_rows_sym(jq, q * NB)
            if J + 4 * NB >= n_pad:
                break
            add("k256", nb, J + 4 * NB, n_pad, J + 4 * NB, n_pad, 4 * NB, tri=1)   # lower triangle of tiles
            if not rhs_gemv and nrhs > 0:
                add("rhs", nb, J + 4 * NB, n_pad, n_pad, n_cols, 4 * NB)
        return dict(small=None, launches=out, back="col" if nrhs > 0 else None)

    for J in range(0, n_pad, 4 * NB):
        trsm(J)
        if J + NB >= n_pad:
            break
        add("in_group", nb, J + NB, n_pad, J + NB, J + 2 * NB, NB)
        add("in_group", nb, J + NB, J + 2 * NB, J + 2 * NB, n_cols, NB)
        trsm(J + NB)
        if J + 2 * NB >= n_pad:
            break
        c_end = min(J + 3 * NB, n_pad)
        add("in_group", nb, J + 2 * NB, n_pad, J + 2 * NB, c_end, 2 * NB)
        add("in_group", nb, J + 2 * NB, c_end, c_end, n_cols, 2 * NB)
        trsm(J + 2 * NB)
        if J + 3 * NB >= n_pad:
            break
        add("in_group", nb, J + 3 * NB, n_pad, J + 3 * NB, J + 4 * NB, 3 * NB)
        add("in_group", nb, J + 3 * NB, J + 4 * NB, J + 4 * NB, n_cols, 3 * NB)
        trsm(J + 3 * NB)
        add("k256", nb, J + 4 * NB, n_pad, J + 4 * NB, n_cols, 4 * NB)
    return dict(small=None, launches=out, back="col" if nrhs > 0 else None)


# ---------------------------------------------------------------------------- the cases
# entry: sym = biem_sym_factor_solve, lu = biem_lu_factor_solve (stored factors), lu_discard = the same with
# BIEM_LU_DISCARD_FACTORS=1 (the fused path's form), ldlt = biem_ldlt_factor_solve, lu_factor / ldlt_factor = the factor-only
# entries followed by biem_lu_solve with nrhs right-hand sides
DENSE_CASES = [
    # A: K = 256 in all three blk_sh regimes across its groups, partial last bands; keep_w back substitution
    *[("A", e, 2048, 8, 1) for e in ("sym", "lu", "lu_discard", "ldlt")],
    # B: persistent panel and in-group launches; row-form back substitution (nb > 64); identity padding rows
    *[("B", e, 1000, 80, 1) for e in ("sym", "lu", "lu_discard", "ldlt")],
    # C: right-hand sides through the gemm, 12-column edge tiles in persistent launches; column-block back substitution
    *[("C", e, 1000, 64, 12) for e in ("sym", "lu", "lu_discard", "ldlt")],
    # D: more than 2^31 complex elements in one call
    ("D", "sym", 2000, 520, 1), ("D", "lu_discard", 2000, 520, 1),
    # E: factor-only launches (nrhs = 0 in the factorisation) at the A and B shapes, then biem_lu_solve; the symmetric
    # row form with nrhs = 0 (back-substitution pass for the checks alone)
    *[("E", e, N, nb, 2) for (N, nb) in ((2048, 8), (1000, 80)) for e in ("lu_factor", "ldlt_factor")],
    ("E", "sym", 1000, 80, 0),
]

SYM_ENTRIES = ("sym",)
GAUSS_ENTRIES = ("lu", "lu_discard", "lu_factor")
FACTOR_ENTRIES = ("lu_factor", "ldlt_factor")


def case_layout(entry, N, nb, nrhs):
    """(n_pad, lda, factorisation nrhs) of a dense case; the matrix is [nb][n_pad][lda] complex, system s at s * n_pad * lda."""
    n_pad = npad_of(N)
    if entry in FACTOR_ENTRIES:
        return n_pad, n_pad, 0
    return n_pad, n_pad + ((nrhs + 7) // 8) * 8, nrhs


def case_schedule(entry, N, nb, nrhs):
    n_pad, lda, fnrhs = case_layout(entry, N, nb, nrhs)
    if entry == "sym":
        sch = sym_schedule(nb, n_pad, fnrhs)
    else:
        sch = lu_schedule(nb, n_pad, fnrhs, symmetric=entry in ("ldlt", "ldlt_factor"))
    sch["max_offset"] = (nb - 1) * n_pad * lda + (n_pad - 1) * lda + (n_pad + fnrhs - 1)     # largest element offset of the call
    return sch


# small systems through biem_sym_factor_solve_n: n_pad = lu_npad(n_active + 1) keeps at least one padding row and column
SMALL_CASES = [(n, r) for n in (1, 30, 50, 60, 64, 70, 90, 100, 121, 128) for r in (0, 1, 2, 8) if n + r <= 128]
SMALL_BATCH = (90, 2, 2000)        # (n_active, nrhs, nb): one large batch at a single shape


def small_npad(n):
    return npad_of(n + 1)


def reached(dense_cases=DENSE_CASES, small_cases=SMALL_CASES):
    """What the case lists reach, derived from the schedule model."""
    got = set()
    for shape, entry, N, nb, nrhs in dense_cases:
        n_pad, lda, fnrhs = case_layout(entry, N, nb, nrhs)
        sch = case_schedule(entry, N, nb, nrhs)
        for g in sch["launches"]:
            if g["ntiles"] > 512:
                got.add(("persistent_kd", g["kd"]))
                if g["col_end"] > n_pad and fnrhs % NB:
                    got.add(("rhs_edge_persistent",))
            if g["kind"] == "k256" and g["tri"] and g["ty_n"] > 8 and g["ty_n"] % 8:
                got.add(("tri_partial_band_blk_sh", g["blk_sh"]))
            if g["kind"] == "k256" and g["blk_sh"] == 6:
                got.add(("entry_k256_blk_sh6", entry))
        if entry == "sym" and sch["back"]:
            got.add(("sym_back", sch["back"]))
        if N < n_pad:       # identity padding rows, by the number of right-hand sides the factorisation carries
            got.add(("entry_padded", entry, "none" if fnrhs == 0 else "few" if fnrhs <= 8 else "many"))
        if sch["max_offset"] >= 2 ** 31:
            got.add(("offset_2_31",))
    for n, r in small_cases:
        got.add(("small",) + small_instance(n, r) if sym_small_path(n, r) else ("small_case_not_small", n, r))
    return got


REQUIRED = ({("persistent_kd", kd) for kd in (64, 128, 192, 256)}
            | {("tri_partial_band_blk_sh", 3), ("tri_partial_band_blk_sh", 6), ("rhs_edge_persistent",), ("offset_2_31",)}
            | {("sym_back", f) for f in ("keep_w", "col", "row")}
            | {("small", 4, False), ("small", 8, False), ("small", 8, True), ("small", 9, True), ("small", 12, True), ("small", 16, True)}
            | {("entry_k256_blk_sh6", e) for e in ("sym", "lu", "lu_discard", "ldlt", "lu_factor", "ldlt_factor")}
            | {("entry_padded", e, r) for e in ("sym", "lu", "lu_discard", "ldlt") for r in ("few", "many")}
            | {("entry_padded", e, "none") for e in ("sym", "lu_factor", "ldlt_factor")})


def test_case_lists_reach_every_launch_regime():
    """CPU: the schedule model says the case lists below reach every regime of the update and back-substitution launches and
    every instantiation of k_small_utu; and no shape of the dense list is redundant (each one reaches something no other does)."""
    got = reached()
    assert REQUIRED <= got, sorted(REQUIRED - got)
    assert not [g for g in got if g[0] == "small_case_not_small"], "a small case the model sends down the blocked path"
    shapes = sorted({c[0] for c in DENSE_CASES})
    for s in shapes:
        rest = reached([c for c in DENSE_CASES if c[0] != s])
        assert not REQUIRED <= rest, f"shape {s} reaches nothing the other shapes do not"


def test_schedule_model_spot_values():
    """CPU: a few tile grids of the model worked by hand from launch_gemm_stream, so the model cannot drift into agreeing with
    itself: the first K = 256 update of shape A (28 tile rows, upper triangle: 406 tiles per system, 8 systems, blocks of 64) and
    the in-group K = 192 launch of shape B (one tile row, columns 192 .. 1025: 13 full tiles + the edge tile holding the right-hand
    side, 80 systems)."""
    a = [g for g in sym_schedule(8, 2048, 1)["launches"] if g["kind"] == "k256"]
    assert [(g["ty_n"], g["ntiles"], g["blk_sh"]) for g in a[:3]] == [(28, 3248, 6), (24, 2400, 6), (20, 1680, 3)]
    assert a[0]["full_bands"] == 3 and a[0]["grid"] == 512
    b = [g for g in sym_schedule(80, 1024, 1)["launches"] if g["kind"] == "in_group" and g["kd"] == 192]
    assert (b[0]["ty_n"], b[0]["tx_n"], b[0]["ntiles"], b[0]["blk_sh"]) == (1, 14, 1120, 3)
    assert small_instance(64, 0) == (8, False) and small_instance(64, 1) == (8, True) and small_instance(72, 0) == (9, True)
    assert not sym_small_path(120, 9) and not sym_small_path(121, 8) and sym_small_path(120, 8)


# ---------------------------------------------------------------------------- GPU fixtures and helpers
@pytest.fixture(scope="module")
def lib():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    from biem_helmholtz_sphere_amd import _lib as L

    return L.load(), L


CHUNK = 8                  # systems per generated chunk (the seed of a chunk is fixed by its index, so any chunk can be rebuilt)


def _gen(entry, seed, N, nrhs, c0, c1):
    """The clean systems c0 .. c1-1 (one aligned chunk) on the device: matrices [c][N][N] and right-hand sides [c][N][nrhs]."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 100003 + c0 // CHUNK)
    n = c1 - c0
    M = torch.view_as_complex(torch.randn((n, N, N, 2), dtype=torch.float64, device="cuda", generator=g))
    F = torch.view_as_complex(torch.randn((n, N, nrhs, 2), dtype=torch.float64, device="cuda", generator=g))
    if entry not in GAUSS_ENTRIES:       # complex symmetric (1 + 0.2i) I + E + E^T
        M *= 0.12 / math.sqrt(N)
        M = M + M.transpose(1, 2)
        M.diagonal(dim1=1, dim2=2).add_(1.0 + 0.2j)
    return M, F


def _chunks(nb):
    return [(c0, min(c0 + CHUNK, nb)) for c0 in range(0, nb, CHUNK)]


def _tile_mask(n_pad, lower, device="cuda"):
    blk = torch.arange(n_pad, device=device) // NB
    return blk[:, None] > blk[None, :] if lower else blk[:, None] < blk[None, :]


def _dense_run(l, L, case, monkeypatch):
    shape, entry, N, nb, nrhs = case
    seed = sum(map(ord, shape + entry)) + N + nb + nrhs
    n_pad, lda, fnrhs = case_layout(entry, N, nb, nrhs)
    wb = l.biem_lu_workspace_bytes(nb, n_pad, fnrhs)
    a_bytes = nb * n_pad * lda * 16
    if a_bytes > 8 << 30:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        need = a_bytes + wb + (4 << 30)
        if free < need:
            pytest.skip(f"shape {shape} needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free")
    A = torch.zeros((nb, n_pad, lda), dtype=torch.complex128, device="cuda")
    # poison: the part of A the entry promises not to read (row form: strict lower triangle outside the diagonal tiles; column
    # forms: the upper one)
    poison = _tile_mask(n_pad, lower=True) if entry == "sym" else _tile_mask(n_pad, lower=False) if entry in ("ldlt", "ldlt_factor") else None
    pad = torch.arange(N, n_pad, device="cuda")
    for c0, c1 in _chunks(nb):
        M, F = _gen(entry, seed, N, nrhs, c0, c1)
        A[c0:c1, :N, :N] = M
        A[c0:c1, pad, pad] = 1.0
        if fnrhs:
            A[c0:c1, :N, n_pad:n_pad + nrhs] = F
        if poison is not None:
            A[c0:c1, :, :n_pad].masked_fill_(poison, 1e30)
        del M, F
    info = torch.ones(nb, dtype=torch.int32, device="cuda")
    ipiv = torch.zeros((nb, n_pad), dtype=torch.int32, device="cuda")
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    sst = n_pad * lda
    if entry == "lu_discard":
        monkeypatch.setenv("BIEM_LU_DISCARD_FACTORS", "1")
    if entry == "sym":
        L.check(l.biem_sym_factor_solve(nb, n_pad, nrhs, A.data_ptr(), lda, sst, info.data_ptr(), work.data_ptr(), wb, None))
    elif entry in ("lu", "lu_discard"):
        L.check(l.biem_lu_factor_solve(nb, n_pad, nrhs, A.data_ptr(), lda, sst, ipiv.data_ptr(), info.data_ptr(), work.data_ptr(), wb, None))
    elif entry == "ldlt":
        L.check(l.biem_ldlt_factor_solve(nb, n_pad, nrhs, A.data_ptr(), lda, sst, ipiv.data_ptr(), info.data_ptr(), work.data_ptr(), wb, None))
    else:
        factor = l.biem_lu_factor if entry == "lu_factor" else l.biem_ldlt_factor
        L.check(factor(nb, n_pad, A.data_ptr(), lda, sst, ipiv.data_ptr(), info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    del work
    assert (info == 0).all(), torch.nonzero(info).flatten()[:16].tolist()
    if entry in FACTOR_ENTRIES:
        ldb = nrhs + 1
        X = torch.zeros((nb, n_pad, ldb), dtype=torch.complex128, device="cuda")
        for c0, c1 in _chunks(nb):
            X[c0:c1, :N, :nrhs] = _gen(entry, seed, N, nrhs, c0, c1)[1]
        L.check(l.biem_lu_solve(nb, n_pad, nrhs, A.data_ptr(), lda, sst, ipiv.data_ptr(), X.data_ptr(), ldb, n_pad * ldb, None))
        torch.cuda.synchronize()
        X = X[:, :, :nrhs]
    else:
        X = A[:, :, n_pad:n_pad + nrhs]
    return A, X, seed, n_pad


@gpu
@pytest.mark.parametrize("case", DENSE_CASES, ids=[f"{c[0]}-{c[1]}-N{c[2]}-nb{c[3]}-r{c[4]}" for c in DENSE_CASES])
def test_dense_factor_solve_in_production_regimes(lib, case, monkeypatch):
    """Every system: info = 0, backward residual max|A x - f| / (max row sum |A| max|x|) < 1e-13 (complex128 on the device),
    exact zeros in the solution's padding rows, and for the row-form symmetric path max|U^T U - A| < 1e-12.  The first and last
    system (and, at shape D, the first one past 2^31 elements) against numpy.linalg.solve: 1e-12 relative (complex-symmetric),
    1e-9 (Gaussian, pivoted)."""
    l, L = lib
    shape, entry, N, nb, nrhs = case
    A, X, seed, n_pad = _dense_run(l, L, case, monkeypatch)
    sst = A.shape[1] * A.shape[2]
    if nrhs and n_pad > N:
        assert X[:, N:, :].abs().max().item() == 0.0
    for c0, c1 in _chunks(nb):
        M, F = _gen(entry, seed, N, nrhs, c0, c1)
        if nrhs:
            x = X[c0:c1, :N, :]
            res = (torch.bmm(M, x) - F).abs().amax(dim=(1, 2)) / (M.abs().sum(dim=2).amax(dim=1) * x.abs().amax(dim=(1, 2)))
            assert (res < 1e-13).all(), (c0, res.max().item(), torch.nonzero(res >= 1e-13).flatten()[:8].tolist())
        if entry == "sym":
            U = torch.triu(A[c0:c1, :N, :N])
            err = (torch.bmm(U.transpose(1, 2), U) - M).abs().amax(dim=(1, 2))
            assert (err < 1e-12).all(), (c0, err.max().item())
        del M, F
    if not nrhs:
        return
    spots = {0, nb - 1}
    if shape == "D":
        s31 = -(-2 ** 31 // sst)
        assert s31 < nb
        spots.add(s31)
    tol = 1e-9 if entry in GAUSS_ENTRIES else 1e-12
    for s in sorted(spots):
        c0 = s // CHUNK * CHUNK
        M, F = _gen(entry, seed, N, nrhs, c0, min(c0 + CHUNK, nb))
        Ms, Fs = M[s - c0].cpu().numpy(), F[s - c0].cpu().numpy()
        Xo = np.linalg.solve(Ms, Fs)
        xs = X[s, :N, :].cpu().numpy()
        assert np.abs(xs - Xo).max() / np.abs(Xo).max() < tol, (shape, entry, s)


# ---------------------------------------------------------------------------- the one-launch small-system kernel
def _small_problem(n, nrhs, nb, rng):
    E = (rng.normal(size=(nb, n, n)) + 1j * rng.normal(size=(nb, n, n))) * (0.12 / np.sqrt(n))
    As = np.eye(n)[None] * (1.0 + 0.2j) + E + np.swapaxes(E, 1, 2)
    Fs = rng.normal(size=(nb, n, nrhs)) + 1j * rng.normal(size=(nb, n, nrhs))
    return As, Fs


def _small_run(l, L, n, nrhs, nb, no_small, seed):
    """biem_sym_factor_solve_n on nb systems of n unknowns in n_pad = lu_npad(n + 1) rows.  Where the model says the one-launch
    path runs, the padding rows and columns (and the right-hand sides' padding rows) are NaN and must stay NaN; on the blocked path
    they are identity padding (zero right-hand sides), whose solution rows must come back exactly zero."""
    rng = np.random.default_rng(seed)
    n_pad = small_npad(n)
    lda = n_pad + ((nrhs + 7) // 8) * 8
    As, Fs = _small_problem(n, nrhs, nb, rng)
    small = sym_small_path(n, nrhs, no_small)
    A = np.zeros((nb, n_pad, lda), dtype=np.complex128)
    A[:, :n, :n] = As
    A[:, :n, n_pad:n_pad + nrhs] = Fs
    if small:
        A[:, n:, :] = np.nan
        A[:, :, n:n_pad] = np.nan
    else:
        A[:, np.arange(n, n_pad), np.arange(n, n_pad)] = 1.0
    blk = np.arange(n) // NB
    A[:, :n, :n][:, blk[:, None] > blk[None, :]] = 1e30          # must never be read
    dA = torch.as_tensor(A, device="cuda")
    info = torch.ones(nb, dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(nb, n_pad, nrhs)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    L.check(l.biem_sym_factor_solve_n(nb, n_pad, n, nrhs, dA.data_ptr(), lda, n_pad * lda, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    assert (info.cpu().numpy() == 0).all(), info.cpu().numpy()
    out = dA.cpu().numpy()
    if small:
        assert np.isnan(out[:, n:, :n_pad + nrhs]).all() and np.isnan(out[:, :, n:n_pad]).all(), "padding was written"
    elif nrhs:
        assert np.abs(out[:, n:, n_pad:n_pad + nrhs]).max() == 0
    X = out[:, :n, n_pad:n_pad + nrhs]
    assert np.isfinite(X).all()
    if nrhs:
        Xo = np.linalg.solve(As, Fs)
        err = np.abs(X - Xo).max(axis=(1, 2)) / np.abs(Xo).max(axis=(1, 2))
        assert (err < 1e-12).all(), (n, nrhs, err.max())
    U = np.triu(out[:, :n, :n])
    err = np.abs(np.swapaxes(U, 1, 2) @ U - As).max(axis=(1, 2))
    assert (err < 1e-12).all(), (n, nrhs, err.max())
    return X


@gpu
@pytest.mark.parametrize("n,nrhs", SMALL_CASES)
def test_sym_factor_solve_n_small_systems(lib, n, nrhs, monkeypatch):
    """biem_sym_factor_solve_n with n_active < n_pad: the one-launch path (every k_small_utu<KR, TWO> across the list) against
    numpy.linalg.solve and U^T U = A at 1e-12, untouched NaN padding; then BIEM_NO_SMALL_PATH=1 - the blocked path on the same
    systems with identity padding - agrees with it."""
    l, L = lib
    X1 = _small_run(l, L, n, nrhs, 3, False, 1000 + 10 * n + nrhs)
    monkeypatch.setenv("BIEM_NO_SMALL_PATH", "1")
    X2 = _small_run(l, L, n, nrhs, 3, True, 1000 + 10 * n + nrhs)
    if nrhs:
        assert np.abs(X1 - X2).max() / np.abs(X2).max() < 1e-12


@gpu
def test_sym_factor_solve_n_large_batch(lib, monkeypatch):
    """One launch of 2000 small systems (k_small_utu<12, true>) and the blocked path on the same systems."""
    l, L = lib
    n, nrhs, nb = SMALL_BATCH
    assert small_instance(n, nrhs) == (12, True)
    X1 = _small_run(l, L, n, nrhs, nb, False, 77)
    monkeypatch.setenv("BIEM_NO_SMALL_PATH", "1")
    X2 = _small_run(l, L, n, nrhs, nb, True, 77)
    assert np.abs(X1 - X2).max() / np.abs(X2).max() < 1e-12


def test_sym_factor_solve_n_rejects_n_active_out_of_range():
    """CPU: the argument check of the new entry runs before any device work."""
    from biem_helmholtz_sphere_amd import _lib as L

    l = L.load()
    buf = (C.c_double * 2)()
    for n_active in (0, -1, 65):
        rc = l.biem_sym_factor_solve_n(1, 64, n_active, 1, C.addressof(buf), 72, 64 * 72, C.addressof(buf), C.addressof(buf), 1, None)
        assert rc != L.BIEM_OK and b"n_active" in l.biem_last_error()
