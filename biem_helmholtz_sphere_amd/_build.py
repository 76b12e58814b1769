"""Build libbiem_mi355.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

The library carries a hash of the sources it was built from (`biem_build_id`); `is_stale()` compares it with the checkout's,
so an edited `csrc/` is never run against an old binary (file times do not survive a copy to another machine, the hash does).
After the link the gfx950 code object is disassembled and the trailing-update kernels are checked (`check_isa`): their LDS-DMA
ring counts vector-memory instructions by hand (`s_waitcnt vmcnt(N)`), which is only right while the compiler adds none.
"""
from __future__ import annotations

import copy
import hashlib
import os
import re
import shutil
import subprocess
import tempfile
from collections import Counter
from dataclasses import dataclass

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbiem_mi355.so")
SOURCES = ["abi.cpp", "solve_path.cpp", "plan.cpp", "plan_tree.cpp", "plan_fill.cpp", "kernels_tables.hip", "kernels_fill.hip", "kernels_fill_sym.hip", "kernels_rhs.hip", "kernels_rhs_pw.hip", "kernels_rhs_ps.hip", "kernels_rhs_ms.hip", "kernels_rhs_ex.hip", "kernels_cluster.hip", "kernels_uscat.hip", "kernels_uinterior.hip", "kernels_power.hip", "kernels_force.hip", "kernels_ladder.hip",
           "kernels_gemm3m.hip", "kernels_lu.hip", "kernels_sym.hip", "kernels_trisolve.hip"]
HEADERS = ["common.hpp", "plan.hpp", "plan_build.hpp", "special.hpp", "fast_layout.hpp", "fill.hpp", "dense.hpp", "rhs_translate.hpp", os.path.join("..", "..", "include", "biem_mi355.h")]
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
# Three steps: _isa_facts() reads what the library holds (once per file), _violations() compares one kernel's facts with its record in
# PINS and nothing else, check_isa() raises on the first kernel with violations.
#
# Keys of PINS and of the report: KD (64 / 128 / 192 / 256) for k_gemm3m_pipe<KD> and KLONG for k_gemm3m_pipe<0>, (NARROW, NF), STRIP,
# (STACK, KD), SLAB, (SWEEP, NQ).
KLONG = 0
PIPE_KD = (64, 128, 192, 256)
NARROW = "narrow"
NARROW_NF = (1, 2, 3)
STRIP = "strip"
STACK = "stack"
STACK_KD = (128, 192, 256)
SLAB = "slab"
SWEEP = "sweep"
SWEEP_NQ = (1, 2, 4, 8)


@dataclass(frozen=True)
class Pins:
    """What is pinned for one kernel.  Every kernel: no scratch and no VGPR spills (either would add vector-memory instructions the vmcnt
    waits do not count).  With `mfma` set, the kernel is an update kernel and the counts below hold for the whole kernel (the compiler
    places cold paths of the chunk loop outside its address range, so per-loop counts are not stable); its only vector-memory instructions
    are then global_load_lds_dwordx4 (the ring), global_store_dwordx4, global_load_dword and the `loads` global_load_dwordx4."""
    scratch_bytes: int = 0
    vgpr_spills: int = 0
    mfma: int | None = None            # MFMAs of the kernel, all inside one loop, the chunk loop (None: not an update kernel, no count below applies)
    lds_dma: int | None = None         # static global_load_lds_dwordx4 count of the reviewed build
    stores: int | None = None          # global_store_dwordx4, all outside the chunk loop
    loads: int = 0                     # global_load_dwordx4: exactly this many, none of them in the chunk loop (0: none allowed anywhere)
    tile_map_loads: int = 0            # global_load_dword at most (the triangular tile map; 0: this launch reads no tile map)
    lane_spill_ops: int | None = None  # v_readlane / v_writelane in the chunk loop at most (None: not pinned)


PINS = {
    # k_gemm3m_pipe<KD>: 96 MFMAs, all inside one loop (3 real products x 2 k4-steps x 16 accumulators per chunk); 48 stores = three epilogue
    # forms x 16 result stores, outside the chunk loop; at most 2 global_load_dword (the triangular tile map, read when the producer
    # moves to its next tile; hipcc waits vmcnt(0) for it, which only drains the ring early).  The static number of LDS-DMA instructions
    # equals the count of the reviewed build (prologue + fused groups with / without a C unit + the clamped edge-tile group).  A
    # different count means the compiler restructured the groups: re-derive the vmcnt(N) constants of kernels_gemm3m.hip against the
    # new disassembly before changing the numbers here.
    **{kd: Pins(mfma=96, lds_dma=dma, stores=48, tile_map_loads=2) for kd, dma in zip(PIPE_KD, (34, 28, 32, 32))},
    # k_gemm3m_pipe<0>, the K-long instance of the left-looking update (run-time chunk count, no tile map): the same pins, reported by
    # check_isa_klong(); check_isa() checks it too and returns the reports of the fixed-K instances.
    # The reviewed K-long build keeps every scalar of its chunk loop in SGPRs: no v_readlane / v_writelane (scalars spilled to VGPR lanes
    # and read back in front of the MFMA block) inside the loop.  The build before it had 15 and ran the bulk update measurably slower
    # (DESIGN.md section 5), so a compiler that brings them back is reported, not taken silently.
    KLONG: Pins(mfma=96, lds_dma=32, stores=48, tile_map_loads=2, lane_spill_ops=0),
    # k_gemm3m_narrow<NF>, the K-long instance for the last tile column of a left-looking band (NF of the tile's four 16-column groups
    # are multiplied, the rest is identity padding): the text of the K-long kernel with shorter MFMA nests, so its pins hold - no
    # scratch, no spills, 32 LDS-DMA, 48 stores, no lane spills in the chunk loop - with 24 NF MFMAs per chunk, all in one loop, and no
    # tile-map load.  Handed out by check_isa_narrow().
    **{(NARROW, nf): Pins(mfma=24 * nf, lds_dma=32, stores=48, tile_map_loads=0, lane_spill_ops=0) for nf in NARROW_NF},
    # k_gemm3m_strip, the product form of the K = 64 kernel (symmetric strip pass: no C slots, four DMAs per group): the same pins,
    # handed out by check_isa_strip().  In its chunk loop the vector-memory instructions are the ring's LDS-DMA alone: the product form
    # adds none.  24 = six groups of four (prologue, fused, unfused interior and clamped edge forms), every wait is vmcnt(4),
    # vmcnt(4 + 16) behind a full tile's stores, or vmcnt(0).  The epilogue that carries the right-hand sides adds, outside the chunk
    # loop, exactly 5 global_load_dwordx4 (z_j of the lane's four rows, the 64 entries of Y) and 17 stores (a fourth form of the 16
    # result stores, Y): 65 in all; tiles that run it end with vmcnt(0).
    STRIP: Pins(mfma=96, lds_dma=24, stores=65, loads=5, tile_map_loads=2),
    # k_gemm3m_stack<KD>, the product form at K = 128 / 192 / 256 (the stacked pass of the panels b, c, d of a group): the text of the
    # strip kernel with a longer chunk loop and the tile decode of a single tile row, so the strip's pins hold for every instance - 24
    # LDS-DMA, 65 stores, 5 loads of the right-hand-side epilogue outside the chunk loop - with no tile-map load at all and, as for the
    # K-long kernel, no v_readlane / v_writelane in the chunk loop (the strip kernel has 5, on the path that decodes the producer's
    # next tile).  Handed out by check_isa_stack().
    **{(STACK, kd): Pins(mfma=96, lds_dma=24, stores=65, loads=5, tile_map_loads=0, lane_spill_ops=0) for kd in STACK_KD},
    # k_sym_slab, the small VALU kernel in front of every stacked pass: a build of it with its loops unrolled spilled 1164 registers to
    # scratch and cost the stage a third of its time, so no scratch and no spills are pinned for it too (check_isa_stack()[SLAB])
    SLAB: Pins(),
    # k_back_sweep<NQ>, the row-form back substitution in one launch per group of right-hand sides: one 1024-thread workgroup per
    # system, so 128 VGPRs per lane is all there is - a spill puts scratch traffic into the stream over U.  No scratch and no VGPR
    # spills are pinned for every instance.  Handed out by check_isa_sweep().
    **{(SWEEP, nq): Pins() for nq in SWEEP_NQ},
}
# the names tests read: aliases into the table
EXPECTED_LDS_DMA = {kd: PINS[kd].lds_dma for kd in PIPE_KD}
EXPECTED_LDS_DMA_KLONG = PINS[KLONG].lds_dma
EXPECTED_STORES = PINS[KLONG].stores
MAX_LANE_SPILL_OPS_KLONG = PINS[KLONG].lane_spill_ops


class IsaCheckError(RuntimeError):
    pass


def _code_objects(lib_path: str, tmp: str) -> list:
    """Unpack the gfx950 code objects of `lib_path` into the directory `tmp`; their paths."""
    objdump = _llvm_tool("llvm-objdump")
    if not objdump:
        raise IsaCheckError("llvm-objdump not found: cannot unpack the code object")
    local = os.path.join(tmp, "lib.so")
    shutil.copy(lib_path, local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f)
    if not objs:
        raise IsaCheckError("no gfx950 code object found in " + lib_path)
    return objs


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


def _key_of(name: str):
    """The key of a checked kernel from its mangled name, or None"""
    if "k_sym_slab" in name:
        return SLAB
    if "k_gemm3m_strip" in name:
        return STRIP
    for stem, family in (("k_back_sweep", SWEEP), ("k_gemm3m_stack", STACK), ("k_gemm3m_narrow", NARROW), ("k_gemm3m_pipe", None)):
        m = re.search(stem + r"ILi(\d+)E", name)
        if m:
            return int(m.group(1)) if family is None else (family, int(m.group(1)))
    return None


_FACTS = {}     # (path, size, mtime) -> what _isa_facts read from that file


def _isa_facts(lib_path: str = LIB) -> dict:
    """What the checks need to know of the library, read once per file (keyed on path, size and modification time; callers do not change
    the result): {"kernels": {key: facts}, "prefetch_hazards": {k_fill_red instance: [instructions]}}.  The facts of a kernel are its
    report as check_isa returns it - metadata, instruction counts of the kernel and of its chunk loop - plus, under names that start
    with an underscore, what only the check reads."""
    st = os.stat(lib_path)
    cache_key = (os.path.abspath(lib_path), st.st_size, st.st_mtime_ns)
    if cache_key in _FACTS:
        return _FACTS[cache_key]
    objdump, readelf = _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    if not objdump or not readelf:
        raise IsaCheckError("llvm-objdump / llvm-readelf not found: cannot check the code object")
    kernels, hazards = {}, {}
    with tempfile.TemporaryDirectory(prefix="biem_isa_") as tmp:
        for path in _code_objects(lib_path, tmp):
            metas = _kernel_meta(readelf, path)
            keys = {n: _key_of(n) for n in metas}
            red = [n for n in metas if "k_fill_red" in n]
            dis = _disassemble(objdump, path) if red or any(k is not None and PINS[k].mfma is not None for k in keys.values()) else {}
            for name in red:
                hazards[name] = _prefetch_hazards(dis[name])
            for name, key in keys.items():
                if key is None:
                    continue
                meta = metas[name]
                facts = {"scratch_bytes": int(meta.get("private_segment_fixed_size", -1)), "vgpr_spills": int(meta.get("vgpr_spill_count", -1)),
                         "vgprs": int(meta.get("vgpr_count", -1))}
                if PINS[key].mfma is not None:
                    ins = dis[name]
                    loop, n_mfma = _chunk_loop(ins)
                    ops = Counter(op for _, op, _ in ins)
                    lops = Counter(op for _, op, _ in loop or [])
                    facts.update({"sgpr_spills": int(meta.get("sgpr_spill_count", -1)),
                                  "mfma_in_chunk_loop": sum(c for op, c in lops.items() if op.startswith("v_mfma")), "mfma_total": n_mfma,
                                  "vm": {op: c for op, c in ops.items() if op.startswith(("global_", "buffer_", "flat_", "scratch_"))},
                                  "lane_spill_ops_in_chunk_loop": lops.get("v_readlane_b32", 0) + lops.get("v_writelane_b32", 0),
                                  "_has_chunk_loop": loop is not None, "_loads_in_chunk_loop": lops.get("global_load_dwordx4", 0)})
                kernels[key] = facts
    _FACTS[cache_key] = {"kernels": kernels, "prefetch_hazards": hazards}
    return _FACTS[cache_key]


def _violations(key, facts: dict) -> list:
    """What the facts of kernel `key` break of its record PINS[key]: one phrase per pin, none if the kernel is as reviewed"""
    pins, bad = PINS[key], []
    if pins.mfma is None:
        if facts["scratch_bytes"] != pins.scratch_bytes or facts["vgpr_spills"] != pins.vgpr_spills:
            bad.append(f"scratch {facts['scratch_bytes']} B, {facts['vgpr_spills']} VGPR spills")
        return bad
    if not facts["_has_chunk_loop"]:
        return ["no loop holds the kernel's MFMAs"]
    vm = facts["vm"]
    if facts["scratch_bytes"] != pins.scratch_bytes:
        bad.append(f"scratch {facts['scratch_bytes']} B")
    if facts["vgpr_spills"] != pins.vgpr_spills:
        bad.append(f"{facts['vgpr_spills']} VGPR spills")
    if facts["mfma_in_chunk_loop"] != pins.mfma or facts["mfma_total"] != pins.mfma:
        bad.append(f"{facts['mfma_in_chunk_loop']} MFMAs in the chunk loop, {facts['mfma_total']} in the kernel (expected {pins.mfma})")
    extra = {op: c for op, c in vm.items() if op not in ("global_load_lds_dwordx4", "global_load_dword", "global_store_dwordx4")}
    if pins.loads and extra.get("global_load_dwordx4") == pins.loads and facts["_loads_in_chunk_loop"] == 0:
        del extra["global_load_dwordx4"]
    if extra:
        bad.append(f"unexpected vector-memory instructions: {extra}")
    if vm.get("global_load_lds_dwordx4", 0) != pins.lds_dma:
        bad.append(f"{vm.get('global_load_lds_dwordx4', 0)} LDS-DMA instructions (reviewed build: {pins.lds_dma})")
    if vm.get("global_store_dwordx4", 0) != pins.stores:
        bad.append(f"{vm.get('global_store_dwordx4', 0)} result stores (reviewed build: {pins.stores})")
    if pins.lane_spill_ops is not None and facts["lane_spill_ops_in_chunk_loop"] > pins.lane_spill_ops:
        bad.append(f"{facts['lane_spill_ops_in_chunk_loop']} lane-spill instructions in the chunk loop (reviewed build: {pins.lane_spill_ops})")
    if vm.get("global_load_dword", 0) > pins.tile_map_loads:
        bad.append(f"{vm.get('global_load_dword', 0)} global_load_dword " +
                   (f"(expected <= {pins.tile_map_loads})" if pins.tile_map_loads else "(this launch reads no tile map)"))
    return bad


def _complaint(key, bad: list) -> str:
    """The message of IsaCheckError for the violations `bad` of kernel `key`"""
    counted = PINS[key].mfma is not None and bad != ["no loop holds the kernel's MFMAs"]
    return f"{_label(key)}: " + ("the hand-counted vmcnt scheme is not safe with this code object: " if counted else "") + "; ".join(bad)


def _check_facts(facts: dict) -> None:
    """Raise IsaCheckError for the first kernel of `facts` (as _isa_facts returns them) that breaks a pin, or if a kernel of PINS is missing"""
    for name, bad in facts["prefetch_hazards"].items():
        # k_fill_red<KT, NC, SPLIT>: no prefetch register may be read, moved or spilled while its load is in flight
        if bad:
            raise IsaCheckError(f"{name}: {len(bad)} instructions touch a prefetch register before its wait, first {bad[0]}")
    for key, f in facts["kernels"].items():
        bad = _violations(key, f)
        if bad:
            raise IsaCheckError(_complaint(key, bad))
    if set(facts["kernels"]) != set(PINS):
        raise IsaCheckError(f"update kernels found: {sorted(facts['kernels'], key=str)}, expected {sorted(PINS, key=str)}")


def check_isa(lib_path: str = LIB, verbose: bool = False, _all_kernels: bool = False) -> dict:
    """Disassemble the gfx950 code objects of `lib_path` (once per file); raise IsaCheckError unless every kernel of PINS is there and keeps
    its pins: for every k_gemm3m_* no scratch, no VGPR spills, its MFMAs in its chunk loop and only the expected vector-memory
    instructions.  Returns the report of the fixed-K instances k_gemm3m_pipe<64 / 128 / 192 / 256>."""
    facts = _isa_facts(lib_path)
    _check_facts(facts)
    report = {key: copy.deepcopy({k: v for k, v in f.items() if not k.startswith("_")}) for key, f in facts["kernels"].items()}
    if verbose:
        for kd in sorted(report, key=str):
            print(f"isa check {_label(kd)}: {report[kd]}")
    # (tests/test_host_logic.py pins the key set of this report to the fixed-K instances [64, 128, 192, 256]: the other kernels are
    # checked above like them and handed out by the accessors below)
    return report if _all_kernels else {kd: r for kd, r in report.items() if kd in PIPE_KD}


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
