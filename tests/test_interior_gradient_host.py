"""CPU tests of uinterior_grad() / utotal_grad(): the public surface, the argument checks that run before any device work, the C
declaration and the code object of the interior gradient kernels (cross-compiled for gfx950: spills, private segment)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _biem, _build, _lib
from test_interior_field_host import FLUID, ROOT, _decl, _result

UIN_GRAD = lambda x: np.zeros_like(x, dtype=np.complex128)      # noqa: E731  (never reached by the checks below)


def _call(fn, res, x, **kw):
    if fn is amd.biem_u_total_grad:
        kw.setdefault("uin_grad", UIN_GRAD)
    return fn(res, x, **kw)


def test_exported_and_methods_of_the_calculator():
    for name in ("biem_u_interior_grad", "biem_u_total_grad"):
        assert name in amd.__all__ and name in _biem.__all__ and callable(getattr(amd, name))
    assert callable(amd.BIEMResultCalculator.uinterior_grad) and callable(amd.BIEMResultCalculator.utotal_grad)
    # methods only: the record's fields stay as they are (no uin_grad is stored)
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")


def test_value_errors_come_before_any_device_work():
    x = np.zeros((3, 2))
    for fn in (amd.biem_u_interior_grad, amd.biem_u_total_grad):
        with pytest.raises(ValueError) as e:
            _call(fn, _result("ba", 3, density=None), x, **FLUID)
        assert str(e.value) == "The BIEMResult does not have density."
        for kind in ("inner", "middle"):
            with pytest.raises(ValueError, match=f"Invalid kind: {kind}"):
                _call(fn, _result("ba", 3, kind=kind), x, **FLUID)
        with pytest.raises(ValueError, match="k_interior \\* radii must not be zero"):
            _call(fn, _result("ba", 3), x, k_interior=np.array([0.0]), density_ratio=np.array([0.5]))
        with pytest.raises(ValueError, match="not broadcastable"):
            _call(fn, _result("ba", 3), x, k_interior=np.ones(3), density_ratio=np.array([0.5]))              # B = 1
        with pytest.raises(ValueError, match="not broadcastable"):
            _call(fn, _result("ba", 3), x, k_interior=np.ones((2, 2, 1)), density_ratio=np.array([0.5]))      # more axes than k has
    with pytest.raises(TypeError, match="uin_grad"):
        amd.biem_u_total_grad(_result("ba", 3), x, **FLUID)                                                  # a required keyword
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types("ba"), centers=np.zeros((3, 1)), radii=np.ones(1), k=1.0, n_end=3,
                                    eta=1.0, kind="outer")
    with pytest.raises(ValueError, match="does not have density"):
        calc.uinterior_grad(x, **FLUID)
    with pytest.raises(ValueError, match="does not have density"):
        calc.utotal_grad(x, uin_grad=UIN_GRAD, **FLUID)
    with pytest.raises(TypeError, match="uin_grad"):
        calc.utotal_grad(x, **FLUID)
    with pytest.raises(TypeError):
        amd.biem_u_interior_grad(_result("ba", 3), x, np.array([2.0]), np.array([0.5]))     # the fluid is keyword-only


@pytest.mark.parametrize("fn", ["biem_u_interior_grad", "biem_u_total_grad"])
@pytest.mark.parametrize("bt,n_end", [("bbba", 3), ("bbbbba", 2), ("ba", 49), ("bpa", 49), ("bba", 15), ("bpbpa", 15), ("caa", 13), ("a", 321)])
def test_not_built_raises_naming_the_covered_set(bt, n_end, fn):
    d = amd.create_from_branching_types(bt).c_ndim
    with pytest.raises(NotImplementedError) as e:
        _call(getattr(amd, fn), _result(bt, n_end), np.zeros((d, 2)), **FLUID)
    msg = str(e.value)
    assert repr(bt) in msg and f"n_end={n_end}" in msg
    assert "a (n_end <= 320), ba (n_end <= 48), bba (n_end <= 14), caa (n_end <= 12)" in msg and "chain" in msg


def test_header_declares_the_entry_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ret, params = _decl(hdr, "biem_uinterior_grad")
    res, args = _lib.SIGNATURES["biem_uinterior_grad"]
    assert len(params) == len(args) == 19
    assert ret == "int" and res is C.c_int
    for p, a in zip(params, args):
        ctype = C.c_void_p if "*" in "".join(p) else C.c_size_t if p[0] == "size_t" else C.c_int
        assert a is ctype, p
    assert "biem_uinterior_grad" in doc
    names = lambda n: [p[-1].lstrip("*") for p in _decl(hdr, n)[1]]
    assert names("biem_uinterior_grad") == names("biem_uinterior")
    assert _lib.SIGNATURES["biem_uinterior_grad"] == _lib.SIGNATURES["biem_uinterior"]


def test_library_cross_compiles_and_exports_the_entry():
    _build.build(force=False)                       # every translation unit for gfx950 (a no-op when the library matches the sources)
    assert not _build.is_stale()
    lib = _lib.load()
    rc = lib.biem_uinterior_grad(None, 1, 1, 1, None, None, None, None, 0, None, None, 0, None, None, 0, None, None, 0, None)
    assert rc != _lib.BIEM_OK and b"plan" in lib.biem_last_error()      # no plan: an argument error, no device touched


def test_interior_gradient_kernels_do_not_spill():
    """Four instantiations of the gradient kernel (one per tree) in the gfx950 code object: no VGPR spills, and no more private
    segment than the kind-inner gradient kernel of the same tree (radial_jh's start values)."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    assert objdump and readelf
    _lib.load()
    with tempfile.TemporaryDirectory(prefix="biem_interior_grad_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        metas = {}
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            metas.update(_build._kernel_meta(readelf, os.path.join(tmp, o)))
    grad = {n: m for n, m in metas.items() if "k_uinterior_grad_fast" in n}
    assert len(grad) == 4, sorted(grad)
    for name, m in grad.items():
        assert not any(s in name for s in ("k_uinterior_fast", "k_interior_coef", "k_uscat_grad_fast"))    # names other tests count by
        tree = re.search(r"k_uinterior_grad_fastILi(\d)E", name).group(1)
        inner = [v for n, v in metas.items() if re.search(r"k_uscat_grad_fastILi%sELb1E" % tree, n)]
        assert len(inner) == 1
        print(name[:45], m, "uscat gradient kernel (inner):", inner[0])
        assert int(m["vgpr_spill_count"]) == 0, (name, m)
        assert int(m["private_segment_fixed_size"]) <= int(inner[0]["private_segment_fixed_size"]), (name, m, inner[0])
