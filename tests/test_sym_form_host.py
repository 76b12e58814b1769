"""CPU tests of the two things launch_sym_factor_solve decides on the host before it launches anything (csrc/dense.hpp, kernels_sym.hip):

  * DenseWork, the layout of the one workspace of the dense factorisations, against the formulas it replaced, written out here;
  * SymForm, the form of a call, against the Python model the GPU tests of the dense solvers select their cases with
    (test_gpu_dense_regimes.py: sym_small_path, small_instance, sym_schedule; test_gpu_sym_left_looking.py: update_form), under the
    default environment and under every switch those tests force a form with.

Both come from biem_sym_form, which needs no GPU.
"""
import ctypes as C
import itertools

import pytest

import test_gpu_dense_regimes as R
import test_gpu_sym_left_looking as LL
from biem_helmholtz_sphere_amd import _lib

NB_GRID = (1, 2, 8, 9, 64, 65, 191, 192, 256)
NPAD_GRID = (64, 128, 256, 320, 1024, 4096, 6400)
NRHS_GRID = (0, 1, 8, 9, 192, 193, 256, 257)
FORM_LEN, WORK_LEN = 9, 11                       # BIEM_SYM_FORM_LEN, BIEM_SYM_WORK_LEN
SWITCHES = ("BIEM_SYM_UPDATE", "BIEM_SYM_GROUP", "BIEM_BACK_FORM", "BIEM_DIAG_FORM", "BIEM_NO_SMALL_PATH")
# every setting the GPU tests force a form with, and the default environment
SETTINGS = [{}, {"BIEM_SYM_UPDATE": "left"}, {"BIEM_SYM_UPDATE": "right"}, {"BIEM_SYM_GROUP": "twopass"}, {"BIEM_SYM_GROUP": "stacked"},
            {"BIEM_SYM_UPDATE": "left", "BIEM_SYM_GROUP": "twopass"}, {"BIEM_SYM_UPDATE": "left", "BIEM_SYM_GROUP": "stacked"},
            {"BIEM_BACK_FORM": "row"}, {"BIEM_BACK_FORM": "col"}, {"BIEM_BACK_FORM": "step"}, {"BIEM_DIAG_FORM": "step"},
            {"BIEM_DIAG_FORM": "step", "BIEM_BACK_FORM": "row"}, {"BIEM_NO_SMALL_PATH": "1"}]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _set(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _query(lib, nb, n_pad, n_active, nrhs):
    form, work = (C.c_int * FORM_LEN)(), (C.c_size_t * WORK_LEN)()
    _lib.check(lib.biem_sym_form(nb, n_pad, n_active, nrhs, form, work))
    return list(form), list(work)


def test_workspace_layout_is_the_one_it_replaced(lib, monkeypatch):
    """work[] of biem_sym_form: every region where the hand-written pointer arithmetic of the launchers had it, the regions pairwise
    disjoint, inside the total and aligned for their element types; and for every back-substitution form what the row form keeps in
    the panel region lies inside it."""
    for back in (None, "row", "col", "step"):
        _set(monkeypatch, {} if back is None else {"BIEM_BACK_FORM": back})
        for nb, n_pad, nrhs in itertools.product(NB_GRID, NPAD_GRID, NRHS_GRID):
            form, work = _query(lib, nb, n_pad, n_pad, nrhs)
            panels, block, tri_map, growth, spare, slab, total = work[:7]
            T = n_pad // 64
            assert total == lib.biem_lu_workspace_bytes(nb, n_pad, nrhs)
            assert total == nb * (4 * 64 * n_pad + 64 * 64) * 16 + (T * (T + 1) // 2 + 63) // 64 * 64 * 4 + nb * 2 * 8 + nb * 64 * 16 + nb * 4 * 64 * 64 * 16
            assert panels == 0
            assert block == nb * 4 * 64 * n_pad * 16
            assert tri_map == block + nb * 64 * 64 * 16
            assert growth == tri_map + (T * (T + 1) // 2 + 63) // 64 * 64 * 4
            assert spare == growth + nb * 2 * 8
            assert slab == total - nb * 4 * 64 * 64 * 16 == spare + nb * 64 * 16
            starts = [panels, block, tri_map, growth, spare, slab, total]
            assert all(a < b for a, b in zip(starts, starts[1:])), starts       # in order and none empty: disjoint, inside the total
            for off, align in ((panels, 16), (block, 16), (tri_map, 4), (growth, 8), (spare, 16), (slab, 16)):
                assert off % align == 0, (nb, n_pad, nrhs, off, align)
            # the row form's aliases of the panel region
            wall_off, wall_bytes, y_off, y_bytes = work[7:]
            small, keep_w, rhs_gemv, back_form = form[0], form[7], form[5], form[6]
            assert wall_bytes == (nb * n_pad * 64 * 16 if keep_w and not small else 0)
            uses_copy = not small and (rhs_gemv or keep_w or (back_form == 0 and nrhs > 0))
            assert y_bytes == (nb * nrhs * n_pad * 16 if uses_copy else 0)
            assert wall_off == panels and y_off == wall_off + wall_bytes and y_off % 16 == 0        # disjoint: the copy stands behind the inverses
            assert y_off + y_bytes <= block, (nb, n_pad, nrhs, back, form, work)


def _model(nb, n_pad, n_active, nrhs, env):
    no_small = "BIEM_NO_SMALL_PATH" in env
    small = R.sym_small_path(n_active, nrhs, no_small)
    kr, two = R.small_instance(n_active, nrhs) if small else (0, False)
    left = LL.update_form(nb, n_pad, nrhs, env.get("BIEM_SYM_UPDATE"))
    group = env.get("BIEM_SYM_GROUP")
    stacked = bool(left) and (nb >= 192 if group is None else group[0] == "s")
    sch = R.sym_schedule(nb, n_pad, nrhs, no_small=True, back_form=env.get("BIEM_BACK_FORM"))     # (the blocked path's fields at any n_active)
    back = {"row": 0, "col": 1, "keep_w": 2}[sch["back"]]
    diag_blk = env.get("BIEM_DIAG_FORM", "four")[0] != "s"
    return [int(small), kr, int(two), int(left), int(stacked), int(sch["rhs_gemv"]), back, int(sch["keep_w"]), int(diag_blk)]


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()) or "default")
def test_form_is_the_models(lib, monkeypatch, env):
    """form[] of biem_sym_form equals the model at every point of the grid, with n_active = n_pad, n_pad - 1 and 1; and the single
    decisions the library also hands out on their own agree with it."""
    _set(monkeypatch, env)
    for nb, n_pad, nrhs in itertools.product(NB_GRID, NPAD_GRID, NRHS_GRID):
        for n_active in (n_pad, n_pad - 1, 1):
            form, _ = _query(lib, nb, n_pad, n_active, nrhs)
            assert form == _model(nb, n_pad, n_active, nrhs, env), (nb, n_pad, n_active, nrhs)
        assert lib.biem_sym_update_form(nb, n_pad, nrhs) == form[3]


def test_form_query_rejects_bad_shapes(lib):
    form, work = (C.c_int * FORM_LEN)(), (C.c_size_t * WORK_LEN)()
    for nb, n_pad, n_active, nrhs in ((0, 64, 64, 1), (1, 100, 100, 1), (1, 64, 0, 1), (1, 64, 65, 1), (1, 64, 64, -1)):
        assert lib.biem_sym_form(nb, n_pad, n_active, nrhs, form, work) != 0
    assert lib.biem_sym_form(1, 64, 64, 1, None, None) == 0
