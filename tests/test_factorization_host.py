"""CPU tests of the factor-once-solve-many surface: symbols, signatures and the argument checks that run before device work."""
import ctypes as C

import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _lib

NEW = ["biem_sym_factor", "biem_sym_solve", "biem_factor_workspace_bytes", "biem_factor_ldlt", "biem_solve_factored_workspace_bytes",
       "biem_solve_factored"]


def test_new_symbols_are_exported_with_their_signatures():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_biem_factorize_is_exported():
    assert "biem_factorize" in amd.__all__ and callable(amd.biem_factorize)
    assert "BIEMFactorization" in amd.__all__


def _fails(rc, text):
    assert rc != _lib.BIEM_OK
    msg = _lib.load().biem_last_error()
    assert text in msg, msg


@pytest.fixture()
def buf():
    b = (C.c_double * 2)()
    return C.addressof(b), b


def test_sym_solve_rejects_bad_arguments(buf):
    lib, (p, _keep) = _lib.load(), buf
    _fails(lib.biem_sym_solve(1, 100, 1, p, 100, 100 * 100, p, 1, 100, None), b"multiple of 64")
    _fails(lib.biem_sym_solve(1, 0, 1, p, 64, 64 * 64, p, 1, 64, None), b"multiple of 64")
    _fails(lib.biem_sym_solve(1, 64, 1, p, 63, 64 * 64, p, 1, 64, None), b"lda < n_pad")
    _fails(lib.biem_sym_solve(1, 64, 4, p, 64, 64 * 64, p, 3, 64, None), b"ldb < nrhs")
    _fails(lib.biem_sym_solve(65536, 64, 1, p, 64, 64 * 64, p, 1, 64, None), b"65535")
    _fails(lib.biem_sym_solve(1, 64, 65536, p, 64, 64 * 64, p, 65536, 64 * 65536, None), b"65535")
    _fails(lib.biem_sym_solve(1, 64, 1, None, 64, 64 * 64, p, 1, 64, None), b"d_U")
    _fails(lib.biem_sym_solve(1, 64, 1, p, 64, 64 * 64, None, 1, 64, None), b"d_B")


def test_sym_factor_rejects_bad_arguments(buf):
    lib, (p, _keep) = _lib.load(), buf
    wb = lib.biem_lu_workspace_bytes(1, 64, 0)
    _fails(lib.biem_sym_factor(1, 100, p, 100, 100 * 100, p, p, 1 << 30, None), b"multiple of 64")
    _fails(lib.biem_sym_factor(1, 64, p, 63, 64 * 64, p, p, wb, None), b"lda")
    _fails(lib.biem_sym_factor(65536, 64, p, 64, 64 * 64, p, p, 1 << 40, None), b"65535")
    _fails(lib.biem_sym_factor(1, 64, p, 64, 64 * 64, p, p, wb - 1, None), b"workspace")
    _fails(lib.biem_sym_factor(1, 64, None, 64, 64 * 64, p, p, wb, None), b"d_A")
    _fails(lib.biem_sym_factor(1, 64, p, 64, 64 * 64, None, p, wb, None), b"d_info")
    _fails(lib.biem_sym_factor(1, 64, p, 64, 64 * 64, p, None, wb, None), b"d_work")


def test_factor_and_solve_entries_need_a_device_plan(buf):
    lib, (p, _keep) = _lib.load(), buf
    _fails(lib.biem_factor_ldlt(None, 1, 2, p, p, p, p, 0, p, p, 0, p, 64, 64 * 64, p, p, 0, p, 1 << 30, None), b"plan")
    _fails(lib.biem_solve_factored(None, 1, 2, 1, p, 64, 64 * 64, p, p, p, p, 1 << 30, None), b"plan")
    plan = C.c_void_p()
    _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS["ba"], 4, C.byref(plan)))
    try:
        _fails(lib.biem_factor_ldlt(plan, 1, 2, p, p, p, p, 0, p, p, 0, p, 64, 64 * 64, p, p, 0, p, 1 << 30, None), b"not uploaded")
        _fails(lib.biem_solve_factored(plan, 1, 2, 1, p, 64, 64 * 64, p, p, p, p, 1 << 30, None), b"not uploaded")
        # workspace sizes are host arithmetic: H = 16 for ba at n_end 4, two balls -> n_pad 64; right-hand sides padded to 8
        assert lib.biem_solve_factored_workspace_bytes(plan, 3, 2, 5) == 3 * 64 * 8 * 16
        assert lib.biem_factor_workspace_bytes(plan, 3, 2, 0) >= lib.biem_lu_workspace_bytes(3, 64, 0)
        assert lib.biem_factor_workspace_bytes(None, 3, 2, 0) == 0
    finally:
        lib.biem_plan_destroy(plan)


# biem_solve_workspace_bytes at (nb, chunk) = (5, 5), (5, 0), (40000, 0), (40000, 40000); biem_factor_workspace_bytes at (5, 5), (5, 0),
# (65535, 0); biem_solve_factored_workspace_bytes at nb = 5 - for the six plans of tests/test_sym_split_host.py's
# test_workspace_size_covers_both_forms, as the library returned them before the whole-path driver got a file of its own.  40000 systems
# are cut by the 24 GiB budget when no chunk is asked for and by the limit of 32768 systems per chunk when 40000 are; 65535 systems by the
# 4 GiB budget of the factor layout, which has no such limit.
PINNED_SIZES = {
    ("ba", 13, 4, 1): ([57021184, 57021184, 25878614528, 373703930624], [16894464, 16894464, 4290955008], 450560),
    ("ba", 13, 4, 9): ([57471744, 57471744, 25887000576, 376656720640], [16894464, 16894464, 4290955008], 901120),
    ("ba", 20, 16, 1): ([3513005568, 3513005568, 25907340032, 23022789024512], [164687360, 164687360, 4281297408], 4096000),
    ("bba", 7, 2, 3): ([16896000, 16896000, 25847410944, 110727801344], [8488960, 8488960, 4293433344], 204800),
    ("ba", 11, 2, 1): ([16754432, 16754432, 25827862016, 109803637248], [7034880, 7034880, 4293749504], 163840),
    ("a", 6, 3, 2): ([5689856, 5689856, 25852375808, 37290072576], [2979328, 2979328, 4291855616], 40960),
}


@pytest.mark.parametrize("tree,n_end,B,nrhs", list(PINNED_SIZES))
def test_workspace_sizes_are_pinned(tree, n_end, B, nrhs):
    """The layout arithmetic of the whole path (chunk size from a budget, caps, padded right-hand-side columns) as numbers."""
    lib = _lib.load()
    plan = C.c_void_p()
    _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS[tree], n_end, C.byref(plan)))
    try:
        solve = [lib.biem_solve_workspace_bytes(plan, nb, B, nrhs, chunk) for nb, chunk in ((5, 5), (5, 0), (40000, 0), (40000, 40000))]
        factor = [lib.biem_factor_workspace_bytes(plan, nb, B, chunk) for nb, chunk in ((5, 5), (5, 0), (65535, 0))]
        assert (solve, factor, lib.biem_solve_factored_workspace_bytes(plan, 5, B, nrhs)) == PINNED_SIZES[tree, n_end, B, nrhs]
    finally:
        lib.biem_plan_destroy(plan)


def _whole_path_calls(lib, plan, p):
    """{entry: call with `plan` and the address p for every pointer} - the entries that share the bodies of the whole path"""
    solve = lambda fn: fn(plan, 1, 2, 1, p, p, p, p, 0, p, p, 0, p, p, p, 0, p, 1 << 30, None)
    solve_n = lambda fn: fn(plan, 1, 2, 1, p, p, p, p, 0, p, p, 0, p, p, p, p, 0, p, 1 << 30, None)
    factor = lambda fn: fn(plan, 1, 2, p, p, p, p, 0, p, p, 0, p, 64, 64 * 64, p, p, 0, p, 1 << 30, None)
    return {"biem_solve": lambda: solve(lib.biem_solve), "biem_solve_ldlt": lambda: solve(lib.biem_solve_ldlt),
            "biem_solve_n": lambda: solve_n(lib.biem_solve_n), "biem_solve_ldlt_n": lambda: solve_n(lib.biem_solve_ldlt_n),
            "biem_factor_ldlt": lambda: factor(lib.biem_factor_ldlt), "biem_factor_ldlt_n": lambda: factor(lib.biem_factor_ldlt_n),
            "biem_solve_factored": lambda: lib.biem_solve_factored(plan, 1, 2, 1, p, 64, 64 * 64, p, p, p, p, 1 << 30, None),
            "biem_solve_factored_n": lambda: lib.biem_solve_factored_n(plan, 1, 2, 1, p, 64, 64 * 64, p, p, p, 0, p, p, p, p, 1 << 30, None)}


def test_shared_bodies_report_under_the_entry_that_was_called(buf):
    """A plan that was never uploaded, and no plan at all: BIEM_ERR_ARG before any device work, the text opens with the entry's own name."""
    lib, (p, _keep) = _lib.load(), buf
    plan = C.c_void_p()
    _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS["ba"], 4, C.byref(plan)))
    try:
        for name, call in _whole_path_calls(lib, plan, p).items():
            assert call() == 1, name                                       # BIEM_ERR_ARG
            assert lib.biem_last_error() == name.encode() + b": plan not uploaded to a device (biem_plan_upload)", name
        for name, call in _whole_path_calls(lib, None, p).items():
            assert call() == 1, name
            assert lib.biem_last_error() == name.encode() + b": null plan", name
    finally:
        lib.biem_plan_destroy(plan)
