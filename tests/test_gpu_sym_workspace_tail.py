"""biem_sym_factor_solve_n stays inside its workspace in every form of a call.

The smallest shape with two four-panel groups (n_pad = 320, so a bulk update runs; 300 active rows, 2 systems), with 0, 1, 9, 200 and
257 right-hand sides - none, in the compact copy, as matrix columns, more than the kept inverses leave room for, more than the compact
copy holds - under the default rules and under every forced form the rules allow.  The workspace is allocated with a 4 KiB tail behind
the biem_lu_workspace_bytes the call is told about; the tail holds a fixed bit pattern, which must still be there afterwards.

Generator and tolerance are those of test_gpu_dense_regimes.py: complex symmetric (1 + 0.2i) I + E + E^T, backward residual 1e-13.
"""
import ctypes as C

import pytest

import test_gpu_dense_regimes as R
from test_gpu_dense_regimes import lib, torch  # noqa: F401  (the module's fixture)

gpu = pytest.mark.gpu

N_PAD, N_ACTIVE, NB_SYS = 320, 300, 2
NRHS = (0, 1, 9, 200, 257)
TAIL = 4096
SWITCHES = ("BIEM_SYM_UPDATE", "BIEM_SYM_GROUP", "BIEM_BACK_FORM", "BIEM_DIAG_FORM", "BIEM_NO_SMALL_PATH")
LEFT, STACKED = {"BIEM_SYM_UPDATE": "left"}, {"BIEM_SYM_UPDATE": "left", "BIEM_SYM_GROUP": "stacked"}
SETTINGS = [{}, LEFT, STACKED] + [{**base, "BIEM_BACK_FORM": b} for base in ({}, STACKED) for b in ("row", "col", "step")]


@gpu
def test_every_form_stays_inside_its_workspace(lib, monkeypatch):  # noqa: F811
    l, L = lib
    M, F = R._gen("sym", 4242, N_ACTIVE, max(NRHS), 0, NB_SYS)
    norm = M.abs().sum(dim=2).amax(dim=1)
    lower = R._tile_mask(N_PAD, lower=True)
    pad = torch.arange(N_ACTIVE, N_PAD, device="cuda")
    seen = set()
    for env in SETTINGS:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        for nrhs in NRHS:
            if env.get("BIEM_BACK_FORM") == "step" and nrhs > 192:
                continue
            form = (C.c_int * 9)()
            L.check(l.biem_sym_form(NB_SYS, N_PAD, N_ACTIVE, nrhs, form, None))
            seen |= {("left", form[3]), ("stacked", form[4]), ("rhs_gemv", form[5]), ("back", form[6])}
            lda = N_PAD + (nrhs + 7) // 8 * 8
            A = torch.zeros((NB_SYS, N_PAD, lda), dtype=torch.complex128, device="cuda")
            A[:, :N_ACTIVE, :N_ACTIVE] = M
            A[:, pad, pad] = 1.0
            A[:, :N_ACTIVE, N_PAD:N_PAD + nrhs] = F[:, :, :nrhs]
            A[:, :, :N_PAD].masked_fill_(lower, 1e30)              # the tiles the row form promises not to read
            wb = l.biem_lu_workspace_bytes(NB_SYS, N_PAD, nrhs)
            work = torch.full((wb + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
            info = torch.ones(NB_SYS, dtype=torch.int32, device="cuda")
            L.check(l.biem_sym_factor_solve_n(NB_SYS, N_PAD, N_ACTIVE, nrhs, A.data_ptr(), lda, N_PAD * lda, info.data_ptr(), work.data_ptr(), wb, None))
            torch.cuda.synchronize()
            where = (sorted(env.items()), nrhs)
            assert (info == 0).all(), (where, info.tolist())
            assert (work[wb:] == 0x5A).all(), (where, "the tail behind the workspace was written")
            if nrhs:
                X = A[:, :, N_PAD:N_PAD + nrhs]
                assert X[:, N_ACTIVE:, :].abs().max().item() == 0.0, where
                x = X[:, :N_ACTIVE, :]
                res = (torch.bmm(M, x) - F[:, :, :nrhs]).abs().amax(dim=(1, 2)) / (norm * x.abs().amax(dim=(1, 2)))
                print(where, "backward residual", res.max().item())
                assert (res < 1e-13).all(), (where, res.tolist())
    want = {("left", 0), ("left", 1), ("stacked", 0), ("stacked", 1), ("rhs_gemv", 0), ("rhs_gemv", 1), ("back", 0), ("back", 1), ("back", 2)}
    assert seen == want, want ^ seen
