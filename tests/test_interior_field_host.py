"""CPU tests of uinterior() / utotal(): the public surface, the argument checks that run before any device work, the C declarations
and the code object of the interior-field kernels (cross-compiled for gfx950: spills, private segment)."""
import ctypes as C
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
ENTRIES = ("biem_interior_coef", "biem_uinterior_workspace_bytes", "biem_uinterior")


def _result(bt, n_end, **kw):
    from biem_helmholtz_sphere_amd._coords import harm_count

    c = amd.create_from_branching_types(bt)
    d = c.c_ndim
    base = dict(c=c, centers=np.zeros((d, 1)), radii=np.ones(1), k=np.float64(1.0), eta=np.float64(1.0), kind="outer", uin=None,
                density=np.ones((1, harm_count(bt, n_end)), dtype=np.complex128))
    base.update(kw)
    return types.SimpleNamespace(**base)


FLUID = dict(k_interior=np.array([2.0]), density_ratio=np.array([0.5]))


def test_exported_and_methods_of_the_calculator():
    for name in ("biem_u_interior", "biem_u_total"):
        assert name in amd.__all__ and name in _biem.__all__ and callable(getattr(amd, name))
    assert callable(amd.BIEMResultCalculator.uinterior) and callable(amd.BIEMResultCalculator.utotal)
    # methods only: the record's fields stay as they are
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")


def test_value_errors_come_before_any_device_work():
    x = np.zeros((3, 2))
    for fn in (amd.biem_u_interior, amd.biem_u_total):
        uin = (lambda x, expand_x=True: x[0]) if fn is amd.biem_u_total else None
        with pytest.raises(ValueError) as e:
            fn(_result("ba", 3, density=None, uin=uin), x, **FLUID)
        assert str(e.value) == "The BIEMResult does not have density."
        for kind in ("inner", "middle"):
            with pytest.raises(ValueError, match=f"Invalid kind: {kind}"):
                fn(_result("ba", 3, kind=kind, uin=uin), x, **FLUID)
        with pytest.raises(ValueError, match="k_interior \\* radii must not be zero"):
            fn(_result("ba", 3, uin=uin), x, k_interior=np.array([0.0]), density_ratio=np.array([0.5]))
        with pytest.raises(ValueError, match="not broadcastable"):
            fn(_result("ba", 3, uin=uin), x, k_interior=np.ones(3), density_ratio=np.array([0.5]))              # B = 1
        with pytest.raises(ValueError, match="not broadcastable"):
            fn(_result("ba", 3, uin=uin), x, k_interior=np.ones((2, 2, 1)), density_ratio=np.array([0.5]))      # more axes than k has
    with pytest.raises(ValueError) as e:
        amd.biem_u_total(_result("ba", 3), x, **FLUID)
    assert str(e.value) == "The BIEMResult does not have uin."
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types("ba"), centers=np.zeros((3, 1)), radii=np.ones(1), k=1.0, n_end=3,
                                    eta=1.0, kind="outer")
    with pytest.raises(ValueError, match="does not have density"):
        calc.uinterior(x, **FLUID)
    with pytest.raises(ValueError, match="does not have uin"):
        calc.utotal(x, **FLUID)
    with pytest.raises(TypeError):
        amd.biem_u_interior(_result("ba", 3), x, np.array([2.0]), np.array([0.5]))          # the fluid is keyword-only


@pytest.mark.parametrize("bt,n_end", [("bbba", 3), ("bbbbba", 2), ("ba", 49), ("bpa", 49), ("bba", 15), ("bpbpa", 15), ("caa", 13), ("a", 321)])
def test_not_built_raises_naming_the_covered_set(bt, n_end):
    d = amd.create_from_branching_types(bt).c_ndim
    with pytest.raises(NotImplementedError) as e:
        amd.biem_u_interior(_result(bt, n_end), np.zeros((d, 2)), **FLUID)
    msg = str(e.value)
    assert repr(bt) in msg and f"n_end={n_end}" in msg
    assert "a (n_end <= 320), ba (n_end <= 48), bba (n_end <= 14), caa (n_end <= 12)" in msg and "chain" in msg


def _decl(text, name):
    m = re.search(r"\b(int|size_t) %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return m.group(1), [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split() for p in m.group(2).split(",")]


def test_header_declares_the_entries_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    want = {"biem_interior_coef": 13, "biem_uinterior_workspace_bytes": 3, "biem_uinterior": 19}
    for name in ENTRIES:
        ret, params = _decl(hdr, name)
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args) == want[name], name
        assert res is (C.c_size_t if ret == "size_t" else C.c_int)
        for p, a in zip(params, args):
            ctype = C.c_void_p if "*" in "".join(p) else C.c_size_t if p[0] == "size_t" else C.c_int
            assert a is ctype, (name, p)
        assert name in doc
    # the field entry takes biem_uscat's arguments with the fluid (d_kint, d_delta, fluid_batched) in front of the density
    names = lambda n: [p[-1].lstrip("*") for p in _decl(hdr, n)[1]]
    us, ui = names("biem_uscat"), names("biem_uinterior")
    i = us.index("d_density")
    assert ui == us[:i] + ["d_kint", "d_delta", "fluid_batched"] + us[i:]


def test_library_cross_compiles_and_exports_the_entries():
    _build.build(force=False)                       # every translation unit for gfx950 (a no-op when the library matches the sources)
    assert not _build.is_stale()
    assert "kernels_uinterior.hip" in _build.SOURCES and "fast_layout.hpp" in _build.HEADERS
    lib = _lib.load()
    rc = lib.biem_uinterior(None, 1, 1, 1, None, None, None, None, 0, None, None, 0, None, None, 0, None, None, 0, None)
    assert rc != _lib.BIEM_OK and b"plan" in lib.biem_last_error()      # no plan: an argument error, no device touched
    rc = lib.biem_interior_coef(None, 1, 1, None, None, None, 0, None, None, 0, None, None, None)
    assert rc != _lib.BIEM_OK and b"plan" in lib.biem_last_error()
    assert lib.biem_uinterior_workspace_bytes(None, 1, 1) == 0


def test_interior_kernels_do_not_spill():
    """Four instantiations of the field kernel (one per tree) and the coefficient kernel in the gfx950 code object: no VGPR spills, and
    no more private segment than the kind-inner value kernel of the same tree (radial_jh's start values)."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    assert objdump and readelf
    _lib.load()
    with tempfile.TemporaryDirectory(prefix="biem_interior_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        metas = {}
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            metas.update(_build._kernel_meta(readelf, os.path.join(tmp, o)))
    field = {n: m for n, m in metas.items() if "k_uinterior_fast" in n}
    assert len(field) == 4, sorted(field)
    assert len([n for n in metas if "k_interior_coef" in n]) == 1
    for name, m in field.items():
        tree = re.search(r"k_uinterior_fastILi(\d)E", name).group(1)
        value = [v for n, v in metas.items() if re.search(r"k_uscat_fastILi%sELb0ELb1E" % tree, n)]
        assert len(value) == 1
        print(name[:40], m, "value kernel (inner):", value[0])
        assert int(m["vgpr_spill_count"]) == 0, (name, m)
        assert int(m["private_segment_fixed_size"]) <= int(value[0]["private_segment_fixed_size"]), (name, m, value[0])
