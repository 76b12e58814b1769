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
