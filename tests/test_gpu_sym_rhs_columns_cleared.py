"""The right-hand-side columns of the augmented matrices are cleared by the solve itself (k_clear_cols), whatever the workspace held.

A flat `ba` layout (four balls in a plane, n_end 13: E = 364 -> 384, O = 312 -> 320) under BIEM_SYM_SPLIT=1, where E's right-hand-side
columns lie inside the O rows' matrix columns and are cleared before the fill writes O, and the columns behind n_pad after it.  The
solve workspace is filled with a fixed nonzero bit pattern before the call, the way tests/test_gpu_sym_workspace_tail.py fills its
workspace; the densities equal those of BIEM_SYM_SPLIT=0 inside the bound of tests/test_gpu_sym_split.py (1e-10 of the largest entry),
and are bit for bit the same under another pattern (0xFF: every stale double a NaN).
"""
import numpy as np
import pytest

import test_gpu_sym_split as S
from test_gpu_sym_split import amd, torch  # noqa: F401  (the module's fixture)

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("nrhs", [1, 9])
def test_stale_workspace_does_not_reach_the_densities(amd, monkeypatch, nrhs):  # noqa: F811
    from biem_helmholtz_sphere_amd import _biem as impl

    plain_ws = impl._workspace

    def patterned(byte):
        def ws(dev, key, wbytes=None):
            work = plain_ws(dev, key, wbytes)
            if work is not None:
                work.fill_(byte)
            return work
        return ws

    args = ("ba", S.SQUARE, np.ones(4), 13, 3, nrhs)
    dens = {}
    for byte in (0x5A, 0xFF):
        monkeypatch.setattr(impl, "_workspace", patterned(byte))
        dens[byte], how, _ = S._solve(amd, monkeypatch, {"BIEM_SYM_SPLIT": "1"}, *args)
        assert how == (384, 320), how
    plain, how0, _ = S._solve(amd, monkeypatch, {"BIEM_SYM_SPLIT": "0"}, *args)
    assert how0 == (0, 0), how0
    e = np.abs(dens[0x5A] - plain).max() / np.abs(plain).max()
    print(f"nrhs {nrhs}: split on a patterned workspace against unsplit {e:.2e}")
    assert e <= S.TOL, e
    assert np.array_equal(dens[0x5A], dens[0xFF])
