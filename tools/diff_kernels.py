#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, kernel by kernel.

    python tools/diff_kernels.py OLD.so NEW.so

The code objects are extracted by `_build._code_objects`, as for `_build.check_isa` (llvm-objdump --offloading).  Compared per kernel: that both builds
have it, its disassembly with addresses and encodings stripped and cut at the symbol's size (what follows is alignment padding), and
its metadata (VGPRs, SGPRs, static LDS, scratch, spills ...).  Which translation unit a kernel sits in does not matter.  Prints the kernels that differ; exit status 1 if any.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from biem_helmholtz_sphere_amd._build import IsaCheckError, _code_objects, _llvm_tool  # noqa: E402

META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
             "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size", "uses_dynamic_stack")


def _metadata(readelf: str, obj: str) -> dict:
    """{kernel symbol: {key: value}} from the code object's notes (one record per kernel, opened by its argument list)."""
    out = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True, text=True).stdout
    metas, cur = {}, None
    for line in out.splitlines():
        if re.match(r"  - \.\w+:", line):                          # a list item at the top level: the next kernel's record
            cur = {}
        m = re.match(r"\s+-?\s*\.(\w+):\s+(\S+)\s*$", line)
        if not m or cur is None:
            continue
        if m.group(1) == "symbol":
            metas[m.group(2).strip("'\"")[:-len(".kd")]] = cur
        elif m.group(1) in META_KEYS:
            cur[m.group(1)] = m.group(2)
    return metas


def _disassembly(objdump: str, readelf: str, obj: str) -> dict:
    """{function symbol: [instruction text]}: no addresses, no encodings, nothing past the symbol's size"""
    end = {}
    for line in subprocess.run([readelf, "--symbols", "--wide", obj], check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            end[f[7]] = int(f[1], 16) + int(f[2])
    out = subprocess.run([objdump, "-d", obj], check=True, capture_output=True, text=True).stdout
    funcs, name = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            continue
        m = re.match(r"\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and name is not None and int(m.group(2), 16) < end.get(name, 0):
            funcs[name].append(re.sub(r"\s+", " ", m.group(1)))
    return funcs


def kernels_of(lib: str) -> dict:
    """{kernel symbol: (metadata, instruction text)} over every gfx950 code object of the library"""
    objdump, readelf = _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    if not objdump or not readelf:
        raise SystemExit("llvm-objdump / llvm-readelf not found")
    kernels = {}
    with tempfile.TemporaryDirectory(prefix="biem_diffk_") as tmp:
        try:
            objs = _code_objects(lib, tmp)
        except IsaCheckError as e:
            raise SystemExit(str(e))
        for obj in objs:
            metas, dis = _metadata(readelf, obj), _disassembly(objdump, readelf, obj)
            for sym, meta in metas.items():
                if sym in kernels:
                    raise SystemExit(f"{lib}: kernel {sym} is defined in two code objects")
                if not dis.get(sym):
                    raise SystemExit(f"{lib}: kernel {sym} has metadata but no code")
                kernels[sym] = (meta, dis[sym])
    return kernels


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__)
        return 2
    old, new = kernels_of(argv[1]), kernels_of(argv[2])
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            print(f"ONLY IN {'OLD' if sym in old else 'NEW'}: {sym}")
            bad += 1
            continue
        (m0, d0), (m1, d1) = old[sym], new[sym]
        what = []
        if m0 != m1:
            what.append("metadata " + ", ".join(f"{k}: {m0.get(k)} -> {m1.get(k)}" for k in META_KEYS if m0.get(k) != m1.get(k)))
        if d0 != d1:
            first = next((i for i, (a, b) in enumerate(zip(d0, d1)) if a != b), min(len(d0), len(d1)))
            what.append(f"code ({len(d0)} -> {len(d1)} instructions, first difference at #{first}: "
                        f"{d0[first] if first < len(d0) else '<end>'!r} / {d1[first] if first < len(d1) else '<end>'!r})")
        if what:
            print(f"DIFFERS: {sym}: " + "; ".join(what))
            bad += 1
    n_ins = sum(len(d) for _, d in new.values())
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {n_ins} instructions compared: {bad} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
