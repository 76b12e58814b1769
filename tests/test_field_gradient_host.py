"""CPU tests of uscat_grad(): the public surface, the argument checks that run before any device work, the C declaration and
the code object of the gradient kernels (cross-compiled for gfx950: registers, spills, private segment)."""
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _biem, _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(bt, n_end, **kw):
    c = amd.create_from_branching_types(bt)
    from biem_helmholtz_sphere_amd._coords import harm_count

    H = harm_count(bt, n_end)
    d = c.c_ndim
    base = dict(c=c, centers=np.zeros((d, 1)), radii=np.ones(1), k=np.float64(1.0), eta=np.float64(1.0), kind="outer",
                density=np.ones((1, H), dtype=np.complex128))
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_exported_and_a_method_of_the_calculator():
    assert "biem_u_grad" in amd.__all__ and callable(amd.biem_u_grad)
    assert callable(amd.BIEMResultCalculator.uscat_grad)
    assert "uscat_grad" not in amd.BIEMResultCalculator.__slots__            # a method only: the record's fields stay as they are
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")
    assert callable(amd.BIEMResultCalculatorProtocol.uscat_grad)


def test_argument_errors_come_before_any_device_work():
    x = np.zeros((3, 2))
    for fn in (amd.biem_u, amd.biem_u_grad):
        with pytest.raises(ValueError) as e:
            fn(_result("ba", 3, density=None), x)
        assert str(e.value) == "The BIEMResult does not have density."
        with pytest.raises(ValueError, match="Invalid kind: middle"):
            fn(_result("ba", 3, kind="middle"), x)
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types("ba"), centers=np.zeros((3, 1)), radii=np.ones(1), k=1.0, n_end=3,
                                    eta=1.0, kind="outer")
    with pytest.raises(ValueError, match="does not have density"):
        calc.uscat_grad(x)
    with pytest.raises(TypeError):
        amd.biem_u_grad(_result("ba", 3), x, far_field=True)               # no far-field gradient: not an argument


@pytest.mark.parametrize("bt,n_end", [("bbba", 3), ("bbbbba", 2), ("ba", 49), ("bpa", 49), ("bba", 15), ("bpbpa", 15), ("caa", 13), ("a", 321)])
def test_not_built_raises_naming_the_covered_set(bt, n_end):
    d = amd.create_from_branching_types(bt).c_ndim
    with pytest.raises(NotImplementedError) as e:
        amd.biem_u_grad(_result(bt, n_end), np.zeros((d, 2)))
    msg = str(e.value)
    assert repr(bt) in msg and f"n_end={n_end}" in msg
    assert "a (n_end <= 320), ba (n_end <= 48), bba (n_end <= 14), caa (n_end <= 12)" in msg and "chain" in msg


def test_python_ceilings_are_the_kernels():
    src = open(os.path.join(ROOT, "biem_helmholtz_sphere_amd", "csrc", "kernels_uscat.hip")).read()
    val = {m.group(1): m.group(2) for m in re.finditer(r"constexpr int (k\w+) = (\w+);", src)}
    num = lambda name: int(val[name]) if val[name].isdigit() else num(val[name])
    assert _biem.USCAT_GRAD_N_END_MAX == {"a": num("kFastNendMax2"), "ba": num("kFastNendMax3"), "bba": num("kFastNendMax4"),
                                         "caa": num("kFastNendMaxCaa")}


def _params(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split() for p in m.group(1).split(",")]


def test_header_declares_the_entry_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    grad, val = _params(hdr, "biem_uscat_grad"), _params(hdr, "biem_uscat")
    res, args = _lib.SIGNATURES["biem_uscat_grad"]
    assert len(grad) == len(args) == 16
    assert [p[:-1] for p in grad] == [p[:-1] for p in val] and [p[-1] for p in grad] == [p[-1] for p in val]   # types and names as biem_uscat
    assert _lib.SIGNATURES["biem_uscat_grad"] == _lib.SIGNATURES["biem_uscat"]
    assert "biem_uscat_grad" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_library_cross_compiles_and_exports_the_entry():
    _build.build(force=False)                       # every translation unit for gfx950 (a no-op when the library matches the sources)
    assert not _build.is_stale()
    lib = _lib.load()
    fn = lib.biem_uscat_grad
    assert fn.restype is _lib.SIGNATURES["biem_uscat_grad"][0] and len(fn.argtypes) == 16
    rc = fn(None, 1, 1, 1, None, None, None, None, 0, None, None, 0, None, None, 0, None)      # no plan: an argument error, no device touched
    assert rc != _lib.BIEM_OK and b"plan" in lib.biem_last_error()


def test_gradient_kernels_do_not_spill():
    """Eight instantiations (4 trees x 2 kinds) in the gfx950 code object, none with VGPR spills, each with the private segment of its
    value kernel (the start values of the radial recurrence, outside the harmonic loops) and no more."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    assert objdump and readelf
    _lib.load()
    with tempfile.TemporaryDirectory(prefix="biem_grad_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        metas = {}
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            metas.update(_build._kernel_meta(readelf, os.path.join(tmp, o)))
    grad = {n: m for n, m in metas.items() if "k_uscat_grad_fast" in n}
    assert len(grad) == 8, sorted(grad)
    for name, m in grad.items():
        tree, inner = re.search(r"k_uscat_grad_fastILi(\d)ELb(\d)E", name).groups()
        value = [v for n, v in metas.items() if re.search(r"k_uscat_fastILi%sELb0ELb%sE" % (tree, inner), n)]
        assert len(value) == 1
        print(name[:40], m, "value kernel:", value[0])
        assert int(m["vgpr_spill_count"]) == 0, (name, m)
        assert int(m["vgpr_count"]) <= 512, (name, m)                  # the unified VGPR + AGPR file of a lane at one wave per SIMD
        assert int(m["private_segment_fixed_size"]) <= int(value[0]["private_segment_fixed_size"]), (name, m, value[0])
