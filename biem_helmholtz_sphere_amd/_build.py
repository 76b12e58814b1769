"""Build libbiem_mi355.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

The library carries a hash of the sources it was built from (`biem_build_id`); `is_stale()` compares it with the checkout's,
so an edited `csrc/` is never run against an old binary (file times do not survive a copy to another machine, the hash does).
After the link the gfx950 code object is disassembled and the trailing-update kernels are checked (`check_isa`): their LDS-DMA
ring counts vector-memory instructions by hand (`s_waitcnt vmcnt(N)`), which is only right while the compiler adds none.
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
import tempfile
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbiem_mi355.so")
SOURCES = ["abi.cpp", "solve_path.cpp", "plan.cpp", "plan_tree.cpp", "plan_fill.cpp", "kernels_tables.hip", "kernels_fill.hip", "kernels_fill_sym.hip", "kernels_rhs.hip", "kernels_rhs_pw.hip", "kernels_degree_bc.hip", "kernels_uscat.hip", "kernels_uinterior.hip", "kernels_power.hip", "kernels_force.hip", "kernels_ladder.hip",
           "kernels_gemm3m.hip", "kernels_lu.hip", "kernels_sym.hip", "kernels_trisolve.hip"]
HEADERS = ["common.hpp", "plan.hpp", "plan_build.hpp", "special.hpp", "fast_layout.hpp", "fill.hpp", "dense.hpp", os.path.join("..", "..", "include", "biem_mi355.h")]
_MARK = b"BIEM_SRC_HASH="


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built")


def _llvm_tool(name: str) -> str | None:
    for cand in (shutil.which(name), os.path.join("/opt/rocm/lib/llvm/bin", name), os.path.join("/opt/rocm/llvm/bin", name)):
        if cand and os.path.exists(cand):
            return cand
    return None


def source_hash() -> str:
    """sha256 over the translation units, the headers and the extra compiler flags (first 16 hex digits)."""
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read() + b"\0")
    h.update(os.environ.get("BIEM_HIPCC_FLAGS", "").encode())
    return h.hexdigest()[:16]


def built_hash(path: str = LIB) -> str | None:
    """The source hash stored in a built library (read from the file, without loading it)."""
    try:
        with open(path, "rb") as fh:
            blob = fh.read()
    except OSError:
        return None
    i = blob.find(_MARK)
    if i < 0:
        return None
    j = blob.find(b";", i)
    return blob[i + len(_MARK):j].decode(errors="replace") if j > 0 else None


def is_stale() -> bool:
    return built_hash() != source_hash()


# ------------------------------------------------------------------------------------------------
# ISA check of the trailing-update kernels (CPU side: llvm-objdump / llvm-readelf on the built library)
# ------------------------------------------------------------------------------------------------
# What the check pins for every k_gemm3m_pipe<KD> (whole kernel; the compiler places cold paths of the chunk loop outside its
# address range, so per-loop counts are not stable):
#   * no scratch, no VGPR spills (either would add vector-memory instructions the vmcnt waits do not count);
#   * exactly 96 MFMAs, all inside one loop (3 real products x 2 k4-steps x 16 accumulators per chunk);
#   * the only vector-memory instructions are global_load_lds_dwordx4 (the ring), global_store_dwordx4 (48 = three epilogue
#     forms x 16 result stores, outside the chunk loop) and at most 2 global_load_dword (the triangular tile map, read when the
#     producer moves to its next tile; hipcc waits vmcnt(0) for it, which only drains the ring early);
#   * the static number of LDS-DMA instructions equals the count of the reviewed build (prologue + fused groups with / without a
#     C unit + the clamped edge-tile group).  A different count means the compiler restructured the groups: re-derive the
#     vmcnt(N) constants of kernels_gemm3m.hip against the new disassembly before changing the numbers here.
EXPECTED_LDS_DMA = {64: 34, 128: 28, 192: 32, 256: 32}
# k_gemm3m_pipe<0>, the K-long instance of the left-looking update (run-time chunk count, no tile map): the same pins, reported by
# check_isa_klong(); check_isa() checks it too and returns the reports of the fixed-K instances
KLONG = 0
EXPECTED_LDS_DMA_KLONG = 32
# The reviewed K-long build keeps every scalar of its chunk loop in SGPRs: no v_readlane / v_writelane (scalars spilled to VGPR lanes and
# read back in front of the MFMA block) inside the loop.  The build before it had 15 and ran the bulk update measurably slower
# (DESIGN.md section 5), so a compiler that brings them back is reported, not taken silently.
MAX_LANE_SPILL_OPS_KLONG = 0
# k_gemm3m_narrow<NF>, the K-long instance for the last tile column of a left-looking band (NF of the tile's four 16-column groups are
# multiplied, the rest is identity padding): the text of the K-long kernel with shorter MFMA nests, so its pins hold - no scratch, no
# spills, 32 LDS-DMA, 48 stores, no lane spills in the chunk loop - with 24 NF MFMAs per chunk, all in one loop, and no tile-map load.
# Keys (NARROW, NF), handed out by check_isa_narrow().
NARROW = "narrow"
NARROW_NF = (1, 2, 3)
MFMA_PER_FRAG = 24
# k_gemm3m_strip, the product form of the K = 64 kernel (symmetric strip pass: no C slots, four DMAs per group): the same pins, under
# the key STRIP, handed out by check_isa_strip().  In its chunk loop the vector-memory instructions are the ring's LDS-DMA alone: the
# product form adds none.  24 = six groups of four (prologue, fused, unfused interior and clamped edge
# forms), every wait is vmcnt(4), vmcnt(4 + 16) behind a full tile's stores, or vmcnt(0).
# The epilogue that carries the right-hand sides adds, outside the chunk loop, exactly 5 global_load_dwordx4 (z_j of the lane's four
# rows, the 64 entries of Y) and 17 stores (a fourth form of the 16 result stores, Y); tiles that run it end with vmcnt(0).
STRIP = "strip"
EXPECTED_LDS_DMA_STRIP = 24
EXPECTED_STORES_STRIP = 65
EXPECTED_LOADS_STRIP = 5
# k_gemm3m_stack<KD>, the product form at K = 128 / 192 / 256 (the stacked pass of the panels b, c, d of a group): the text of the strip
# kernel with a longer chunk loop and the tile decode of a single tile row, so the strip's pins hold for every instance - 24 LDS-DMA,
# 65 stores, 5 loads of the right-hand-side epilogue outside the chunk loop - with no tile-map load at all and, as for the K-long
# kernel, no v_readlane / v_writelane in the chunk loop (the strip kernel has 5, on the path that decodes the producer's next tile).
# Keys (STACK, KD), handed out by check_isa_stack().
STACK = "stack"
SLAB = "slab"
# k_back_sweep<NQ>, the row-form back substitution in one launch per group of right-hand sides: one 1024-thread workgroup per system,
# so 128 VGPRs per lane is all there is - a spill puts scratch traffic into the stream over U.  No scratch and no VGPR spills are pinned
# for every instance.  Keys (SWEEP, NQ), handed out by check_isa_sweep().
SWEEP = "sweep"
SWEEP_NQ = (1, 2, 4, 8)
STACK_KD = (128, 192, 256)
EXPECTED_LDS_DMA_STACK = 24
EXPECTED_STORES_STACK = 65
EXPECTED_LOADS_STACK = 5
MAX_LANE_SPILL_OPS_STACK = 0
EXPECTED_STORES = 48
MFMA_PER_CHUNK = 96
MAX_TILE_MAP_LOADS = 2


class IsaCheckError(RuntimeError):
    pass


def _kernel_meta(readelf: str, obj: str) -> dict:
    out = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True, text=True).stdout
    metas, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r"\s+-?\s*\.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key in cur:           # a new kernel record starts when a key repeats
            if "name" in cur:
                metas[cur["name"]] = cur
            cur = {}
        cur[key] = val
    if "name" in cur:
        metas[cur["name"]] = cur
    return metas


def _disassemble(objdump: str, obj: str) -> dict:
    out = subprocess.run([objdump, "-d", obj], check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            kernels[name] = []
            continue
        m = re.match(r"\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and name is not None:
            kernels[name].append((int(m.group(3), 16), m.group(1), m.group(2)))
    return kernels


def _chunk_loop(ins):
    """Instructions of the smallest backward-branch loop that holds every MFMA of the kernel."""
    n_mfma = sum(1 for _, op, _ in ins if op.startswith("v_mfma"))
    best = None
    for a, op, args in ins:
        if not (op.startswith("s_cbranch") or op == "s_branch"):
            continue
        if not re.fullmatch(r"-?\d+", args.strip()):
            continue
        off = int(args)
        if off >= 32768:
            off -= 65536
        tgt = a + 4 + 4 * off
        if tgt >= a:
            continue
        body = [x for x in ins if tgt <= x[0] <= a]
        if sum(1 for _, o, _ in body if o.startswith("v_mfma")) == n_mfma and (best is None or len(body) < len(best)):
            best = body
    return best, n_mfma


def _vregs(tok: str) -> set:
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def _prefetch_hazards(ins) -> list:
    """Instructions that touch the destination of a global_load_dwordx4 before the next `s_waitcnt vmcnt(0)`.  k_fill_red issues its table
    prefetch from inline asm and waits for it much later (BIEM_TN_CLAIM), so the compiler does not know the registers are in flight: under
    register pressure it has spilled them right behind the load and reused them as an address (k_fill_red<8, 2, false>), which stores
    stale data and lets the load land in a live pointer."""
    pending, bad = set(), []
    for a, op, args in ins:
        if op == "s_waitcnt" and "vmcnt(0)" in args:
            pending = set()
            continue
        toks = [t.strip() for t in args.split(",")]
        used = set().union(*[_vregs(t) for t in toks]) if toks else set()
        if used & pending:
            bad.append(f"{a:#x}: {op} {args}")
        if op == "global_load_dwordx4":
            pending |= _vregs(toks[0])
    return bad


def _label(kd) -> str:
    if isinstance(kd, tuple):
        return f"k_back_sweep<{kd[1]}>" if kd[0] == SWEEP else f"k_gemm3m_narrow<{kd[1]}>" if kd[0] == NARROW else f"k_gemm3m_stack<{kd[1]}>"
    return "k_gemm3m_strip" if kd == STRIP else "k_sym_slab" if kd == SLAB else f"k_gemm3m_pipe<{kd}>"


def check_isa(lib_path: str = LIB, verbose: bool = False, _all_kernels: bool = False) -> dict:
    """Disassemble the gfx950 code objects of `lib_path`; raise IsaCheckError unless every k_gemm3m_pipe<*> has no scratch,
    no VGPR spills, 96 MFMAs in its chunk loop and only the expected vector-memory instructions there.  Returns the report."""
    objdump, readelf = _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    if not objdump or not readelf:
        raise IsaCheckError("llvm-objdump / llvm-readelf not found: cannot check the code object")
    report = {}
    with tempfile.TemporaryDirectory(prefix="biem_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        objs = sorted(f for f in os.listdir(tmp) if "gfx950" in f)
        if not objs:
            raise IsaCheckError("no gfx950 code object found in " + lib_path)
        for o in objs:
            path = os.path.join(tmp, o)
            metas = _kernel_meta(readelf, path)
            for n in metas:
                # k_sym_slab, the small VALU kernel in front of every stacked pass: a build of it with its loops unrolled spilled 1164
                # registers to scratch and cost the stage a third of its time, so no scratch and no spills are pinned for it too
                if "k_sym_slab" in n:
                    rep = {"scratch_bytes": int(metas[n].get("private_segment_fixed_size", -1)), "vgpr_spills": int(metas[n].get("vgpr_spill_count", -1)),
                           "vgprs": int(metas[n].get("vgpr_count", -1))}
                    report[SLAB] = rep
                    if rep["scratch_bytes"] != 0 or rep["vgpr_spills"] != 0:
                        raise IsaCheckError(f"k_sym_slab: scratch {rep['scratch_bytes']} B, {rep['vgpr_spills']} VGPR spills")
                m = re.search(r"k_back_sweepILi(\d+)E", n)
                if m:
                    rep = {"scratch_bytes": int(metas[n].get("private_segment_fixed_size", -1)), "vgpr_spills": int(metas[n].get("vgpr_spill_count", -1)),
                           "vgprs": int(metas[n].get("vgpr_count", -1))}
                    report[(SWEEP, int(m.group(1)))] = rep
                    if rep["scratch_bytes"] != 0 or rep["vgpr_spills"] != 0:
                        raise IsaCheckError(f"k_back_sweep<{m.group(1)}>: scratch {rep['scratch_bytes']} B, {rep['vgpr_spills']} VGPR spills")
            gemm = [n for n in metas if "k_gemm3m_pipe" in n or "k_gemm3m_strip" in n or "k_gemm3m_stack" in n or "k_gemm3m_narrow" in n]
            red = [n for n in metas if "k_fill_red" in n]
            if not gemm and not red:
                continue
            dis = _disassemble(objdump, path)
            # k_fill_red<KT, NC, SPLIT>: no prefetch register may be read, moved or spilled while its load is in flight
            for name in red:
                bad = _prefetch_hazards(dis[name])
                if bad:
                    raise IsaCheckError(f"{name}: {len(bad)} instructions touch a prefetch register before its wait, first {bad[0]}")
            for name in gemm:
                stack, narrow = "k_gemm3m_stack" in name, "k_gemm3m_narrow" in name
                kd = STRIP if "k_gemm3m_strip" in name else (STACK, int(re.search(r"k_gemm3m_stackILi(\d+)E", name).group(1))) if stack else \
                    (NARROW, int(re.search(r"k_gemm3m_narrowILi(\d+)E", name).group(1))) if narrow else \
                    int(re.search(r"k_gemm3m_pipeILi(\d+)E", name).group(1))
                want_mfma = MFMA_PER_FRAG * kd[1] if narrow else MFMA_PER_CHUNK
                label = _label(kd)
                meta, ins = metas[name], dis[name]
                loop, n_mfma = _chunk_loop(ins)
                if loop is None:
                    raise IsaCheckError(f"{label}: no loop holds the kernel's MFMAs")
                ops = Counter(op for _, op, _ in ins)
                lops = Counter(op for _, op, _ in loop)
                vm = {op: c for op, c in ops.items() if op.startswith(("global_", "buffer_", "flat_", "scratch_"))}
                rep = {"scratch_bytes": int(meta.get("private_segment_fixed_size", -1)), "vgpr_spills": int(meta.get("vgpr_spill_count", -1)),
                       "sgpr_spills": int(meta.get("sgpr_spill_count", -1)), "vgprs": int(meta.get("vgpr_count", -1)),
                       "mfma_in_chunk_loop": sum(c for op, c in lops.items() if op.startswith("v_mfma")), "mfma_total": n_mfma,
                       "vm": vm, "lane_spill_ops_in_chunk_loop": lops.get("v_readlane_b32", 0) + lops.get("v_writelane_b32", 0)}
                report[kd] = rep
                bad = []
                if rep["scratch_bytes"] != 0:
                    bad.append(f"scratch {rep['scratch_bytes']} B")
                if rep["vgpr_spills"] != 0:
                    bad.append(f"{rep['vgpr_spills']} VGPR spills")
                if rep["mfma_in_chunk_loop"] != want_mfma or n_mfma != want_mfma:
                    bad.append(f"{rep['mfma_in_chunk_loop']} MFMAs in the chunk loop, {n_mfma} in the kernel (expected {want_mfma})")
                extra = {op: c for op, c in vm.items() if op not in ("global_load_lds_dwordx4", "global_load_dword", "global_store_dwordx4")}
                if (kd == STRIP or stack) and extra.get("global_load_dwordx4") == (EXPECTED_LOADS_STACK if stack else EXPECTED_LOADS_STRIP) and \
                        not any(op == "global_load_dwordx4" for _, op, _ in loop):
                    del extra["global_load_dwordx4"]
                if extra:
                    bad.append(f"unexpected vector-memory instructions: {extra}")
                want_dma = EXPECTED_LDS_DMA_STACK if stack else EXPECTED_LDS_DMA_STRIP if kd == STRIP else EXPECTED_LDS_DMA_KLONG if kd == KLONG or narrow else \
                    EXPECTED_LDS_DMA.get(kd)
                if vm.get("global_load_lds_dwordx4", 0) != want_dma:
                    bad.append(f"{vm.get('global_load_lds_dwordx4', 0)} LDS-DMA instructions (reviewed build: {want_dma})")
                want_stores = EXPECTED_STORES_STACK if stack else EXPECTED_STORES_STRIP if kd == STRIP else EXPECTED_STORES
                if vm.get("global_store_dwordx4", 0) != want_stores:
                    bad.append(f"{vm.get('global_store_dwordx4', 0)} result stores (reviewed build: {want_stores})")
                if (kd == KLONG or narrow) and rep["lane_spill_ops_in_chunk_loop"] > MAX_LANE_SPILL_OPS_KLONG:
                    bad.append(f"{rep['lane_spill_ops_in_chunk_loop']} lane-spill instructions in the chunk loop (reviewed build: {MAX_LANE_SPILL_OPS_KLONG})")
                if stack and rep["lane_spill_ops_in_chunk_loop"] > MAX_LANE_SPILL_OPS_STACK:
                    bad.append(f"{rep['lane_spill_ops_in_chunk_loop']} lane-spill instructions in the chunk loop (reviewed build: {MAX_LANE_SPILL_OPS_STACK})")
                if (stack or narrow) and vm.get("global_load_dword", 0) != 0:
                    bad.append(f"{vm.get('global_load_dword', 0)} global_load_dword (this launch reads no tile map)")
                if vm.get("global_load_dword", 0) > MAX_TILE_MAP_LOADS:
                    bad.append(f"{vm.get('global_load_dword', 0)} global_load_dword (expected <= {MAX_TILE_MAP_LOADS})")
                if bad:
                    raise IsaCheckError(f"{label}: the hand-counted vmcnt scheme is not safe with this code object: " + "; ".join(bad))
    want = set(EXPECTED_LDS_DMA) | {KLONG, STRIP, SLAB} | {(STACK, k) for k in STACK_KD} | {(SWEEP, q) for q in SWEEP_NQ} | \
        {(NARROW, f) for f in NARROW_NF}
    if set(report) != want:
        raise IsaCheckError(f"update kernels found: {sorted(report, key=str)}, expected {sorted(want, key=str)}")
    if verbose:
        for kd in sorted(report, key=str):
            print(f"isa check {_label(kd)}: {report[kd]}")
    # (tests/test_host_logic.py pins the key set of this report to the fixed-K instances [64, 128, 192, 256]: the K-long instance and the
    # strip kernel are checked above like the others and handed out by check_isa_klong / check_isa_strip)
    return report if _all_kernels else {kd: r for kd, r in report.items() if kd in EXPECTED_LDS_DMA}


def check_isa_klong(lib_path: str = LIB) -> dict:
    """The report of k_gemm3m_pipe<0> (same checks as check_isa, which raises for it as well)."""
    return check_isa(lib_path, _all_kernels=True)[KLONG]


def check_isa_strip(lib_path: str = LIB) -> dict:
    """The report of k_gemm3m_strip (same checks as check_isa, which raises for it as well)."""
    return check_isa(lib_path, _all_kernels=True)[STRIP]


def check_isa_stack(lib_path: str = LIB) -> dict:
    """The reports of k_gemm3m_stack<KD>, keyed by KD, and of k_sym_slab under SLAB (same checks as check_isa, which raises for them as well)."""
    rep = check_isa(lib_path, _all_kernels=True)
    return {**{k: rep[(STACK, k)] for k in STACK_KD}, SLAB: rep[SLAB]}


def check_isa_narrow(lib_path: str = LIB) -> dict:
    """The reports of k_gemm3m_narrow<NF>, keyed by NF (same checks as check_isa, which raises for them as well)."""
    rep = check_isa(lib_path, _all_kernels=True)
    return {f: rep[(NARROW, f)] for f in NARROW_NF}


def check_isa_sweep(lib_path: str = LIB) -> dict:
    """The reports of k_back_sweep<NQ>, keyed by NQ (same checks as check_isa, which raises for them as well)."""
    rep = check_isa(lib_path, _all_kernels=True)
    return {q: rep[(SWEEP, q)] for q in SWEEP_NQ}


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP translation unit into one shared library (written next to it, then renamed over it); returns its path."""
    if not force and not is_stale():
        return LIB
    tmp = LIB + f".tmp{os.getpid()}"
    cmd = [_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", f'-DBIEM_SRC_HASH="{source_hash()}"', "-o", tmp]
    cmd += os.environ.get("BIEM_HIPCC_FLAGS", "").split()      # experiments only
    cmd += [os.path.join(CSRC, f) for f in SOURCES]
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.run(cmd, check=True, cwd=CSRC)
        if os.environ.get("BIEM_SKIP_ISA_CHECK") != "1":       # (timing-ablation builds change the instruction counts on purpose)
            check_isa(tmp, verbose=verbose)
        os.replace(tmp, LIB)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
