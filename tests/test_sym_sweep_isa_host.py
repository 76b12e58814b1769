"""The code objects of the row-form back-substitution sweep and of the slab kernel (CPU: llvm-readelf on the built library)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from biem_helmholtz_sphere_amd import _build, _lib


def test_sweep_and_slab_kernels_use_no_scratch():
    """k_back_sweep<1 / 2 / 4 / 8> (one 1024-thread workgroup per system: 128 VGPRs per lane) and k_sym_slab (two 256-thread workgroups
    per CU: 256 VGPRs per lane): no scratch, no spills, inside the register budget of their launch bounds."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    if not objdump or not readelf:
        pytest.skip("llvm-objdump / llvm-readelf not found")
    _lib.load()
    metas = {}
    with tempfile.TemporaryDirectory(prefix="biem_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        for f in os.listdir(tmp):
            if "gfx950" in f:
                metas.update(_build._kernel_meta(readelf, os.path.join(tmp, f)))
    seen = set()
    for n, m in metas.items():
        sweep = re.search(r"k_back_sweepILi(\d+)E", n)
        if sweep or "k_sym_slab" in n:
            seen.add(int(sweep.group(1)) if sweep else "slab")
            assert int(m["private_segment_fixed_size"]) == 0 and int(m["vgpr_spill_count"]) == 0, (n, m)
            assert int(m["vgpr_count"]) <= (128 if sweep else 256), (n, m)
    assert seen == {1, 2, 4, 8, "slab"}, seen
    # the same pins inside the build's own check
    rep = _build.check_isa_sweep()
    assert sorted(rep) == [1, 2, 4, 8] and all(r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 for r in rep.values()), rep
    slab = _build.check_isa_stack()[_build.SLAB]
    assert slab["scratch_bytes"] == 0 and slab["vgpr_spills"] == 0, slab
