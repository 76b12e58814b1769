#!/usr/bin/env python3
"""Host-side comparison of two builds of the library (no GPU): python tools/compare_dense_host.py OLD.so NEW.so

The public sizes (biem_lu_workspace_bytes on a grid; biem_solve_workspace_bytes, biem_factor_workspace_bytes and
biem_solve_factored_workspace_bytes for a few plans, among them batches that meet the caps of the chunk size) and the bulk-update decision biem_sym_update_form under the default environment and the switches that force a form must be the same in
both.  Prints one line per check and exits 1 on a difference.
"""
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from biem_helmholtz_sphere_amd import _lib  # noqa: E402  (signatures and tree ids only: the libraries are loaded by path)

NB = (1, 2, 8, 9, 64, 65, 191, 192, 256)
NPAD = (64, 128, 256, 320, 1024, 4096, 6400)
NRHS = (0, 1, 8, 9, 192, 193, 256, 257)
PLANS = [("ba", 13, 4, 1), ("ba", 13, 4, 9), ("ba", 20, 16, 1), ("bba", 7, 2, 3), ("ba", 11, 2, 1), ("a", 6, 3, 2)]      # tests/test_sym_split_host.py
# (nb, chunk); 40000 systems meet the solve layout's cap of 32768 per chunk (asked for or not), 65535 the factor layout's own limit
CHUNKS = ((5, 5), (5, 0), (256, 0), (256, 32), (40000, 0), (40000, 40000), (65535, 0))
SETTINGS = [{}, {"BIEM_SYM_UPDATE": "left"}, {"BIEM_SYM_UPDATE": "right"}, {"BIEM_SYM_GROUP": "twopass"}, {"BIEM_SYM_GROUP": "stacked"},
            {"BIEM_BACK_FORM": "row"}, {"BIEM_BACK_FORM": "col"}, {"BIEM_BACK_FORM": "step"}, {"BIEM_DIAG_FORM": "step"}, {"BIEM_NO_SMALL_PATH": "1"}]
SWITCHES = ("BIEM_SYM_UPDATE", "BIEM_SYM_GROUP", "BIEM_BACK_FORM", "BIEM_DIAG_FORM", "BIEM_NO_SMALL_PATH")


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    bad = 0

    def report(what, a, b):
        nonlocal bad
        same = a == b
        bad += not same
        print(f"{what}: {len(a)} values, {'identical' if same else 'DIFFERENT: ' + str([i for i, (x, y) in enumerate(zip(a, b)) if x != y][:8])}")

    grid = list(itertools.product(NB, NPAD, NRHS))
    report("biem_lu_workspace_bytes, nb x n_pad x nrhs grid", *[[lib.biem_lu_workspace_bytes(*g) for g in grid] for lib in (old, new)])
    sizes = []
    for lib in (old, new):
        vals = []
        for tree, n_end, B, nrhs in PLANS:
            plan = C.c_void_p()
            assert lib.biem_plan_create_host(_lib.TREE_IDS[tree], n_end, C.byref(plan)) == 0
            for nb, chunk in CHUNKS:
                vals += [lib.biem_solve_workspace_bytes(plan, nb, B, nrhs, chunk), lib.biem_factor_workspace_bytes(plan, nb, B, chunk),
                         lib.biem_solve_factored_workspace_bytes(plan, nb, B, nrhs)]
            lib.biem_plan_destroy(plan)
        sizes.append(vals)
    report(f"biem_solve_ / biem_factor_ / biem_solve_factored_workspace_bytes, {len(PLANS)} plans x {len(CHUNKS)} (nb, chunk)", *sizes)
    for env in SETTINGS:
        for name in SWITCHES:
            os.environ.pop(name, None)
        os.environ.update(env)
        report(f"biem_sym_update_form, grid, {env or 'default environment'}", *[[lib.biem_sym_update_form(*g) for g in grid] for lib in (old, new)])
    print("all identical" if not bad else f"{bad} check(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
