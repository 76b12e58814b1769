"""The pin table of the ISA check (_build.PINS), host side (no GPU): every pin, once violated, is reported.

_build.check_isa is three steps: _isa_facts reads the built library (one disassembly per file), _violations compares one kernel's facts
with its record in PINS, _check_facts raises for the first kernel with violations or for a missing kernel.  This module takes the real
facts of one member of every kernel family and checks that

  * they break nothing;
  * a copy with ONE value moved off its pin - an LDS-DMA more or fewer, a store more, an MFMA fewer in the chunk loop, 16 bytes of scratch,
    one VGPR spill, one lane-spill instruction or one tile-map load above the maximum, one more vector load - makes _check_facts raise
    an IsaCheckError that names the kernel and the pin;
  * a library without that kernel is refused;
  * check_isa and its five accessors share one disassembly and hand out copies.
"""
import copy

import pytest

from biem_helmholtz_sphere_amd import _build, _lib

# one member of every family, with the name the message must carry
MEMBERS = {128: "k_gemm3m_pipe<128>", _build.KLONG: "k_gemm3m_pipe<0>", (_build.NARROW, 2): "k_gemm3m_narrow<2>", _build.STRIP: "k_gemm3m_strip",
           (_build.STACK, 192): "k_gemm3m_stack<192>", _build.SLAB: "k_sym_slab", (_build.SWEEP, 4): "k_back_sweep<4>"}


@pytest.fixture(scope="module")
def facts():
    _lib.load()                       # (builds the library if the checkout has none that matches its sources)
    return _build._isa_facts()


def perturbations(key):
    """(what, change of the kernel's facts, phrase of the violation) for every pin of PINS[key]"""
    pins = _build.PINS[key]
    out = [("scratch", lambda f: f.update(scratch_bytes=pins.scratch_bytes + 16), "scratch 16 B"),
           ("spill", lambda f: f.update(vgpr_spills=pins.vgpr_spills + 1), "1 VGPR spills")]
    if pins.mfma is None:
        return out

    def vm(op, d):
        return lambda f: f["vm"].update({op: f["vm"].get(op, 0) + d})
    out += [("mfma", lambda f: f.update(mfma_in_chunk_loop=pins.mfma - 1), f"{pins.mfma - 1} MFMAs in the chunk loop, {pins.mfma} in the kernel"),
            ("mfma outside", lambda f: f.update(mfma_total=pins.mfma + 1), f"{pins.mfma + 1} in the kernel"),
            ("dma +1", vm("global_load_lds_dwordx4", 1), f"{pins.lds_dma + 1} LDS-DMA instructions"),
            ("dma -1", vm("global_load_lds_dwordx4", -1), f"{pins.lds_dma - 1} LDS-DMA instructions"),
            ("store", vm("global_store_dwordx4", 1), f"{pins.stores + 1} result stores"),
            ("x4 load", vm("global_load_dwordx4", 1), f"unexpected vector-memory instructions: {{'global_load_dwordx4': {pins.loads + 1}}}"),
            ("scratch op", vm("scratch_store_dwordx4", 1), "unexpected vector-memory instructions: {'scratch_store_dwordx4': 1}"),
            ("tile map", lambda f: f["vm"].update(global_load_dword=pins.tile_map_loads + 1), f"{pins.tile_map_loads + 1} global_load_dword")]
    if pins.loads:
        out.append(("x4 load in loop", lambda f: f.update(_loads_in_chunk_loop=1), "unexpected vector-memory instructions: {'global_load_dwordx4'"))
    if pins.lane_spill_ops is not None:
        out.append(("lane spill", lambda f: f.update(lane_spill_ops_in_chunk_loop=pins.lane_spill_ops + 1),
                    f"{pins.lane_spill_ops + 1} lane-spill instructions in the chunk loop"))
    return out


def test_every_family_has_a_member_here():
    def fam(k):
        return k[0] if isinstance(k, tuple) else k if isinstance(k, str) else ("klong" if k == _build.KLONG else "pipe")
    assert {fam(k) for k in _build.PINS} == {fam(k) for k in MEMBERS} and set(MEMBERS) <= set(_build.PINS)
    assert set(_build.PINS) == set(_build.PIPE_KD) | {_build.KLONG, _build.STRIP, _build.SLAB} | {(_build.NARROW, f) for f in _build.NARROW_NF} | \
        {(_build.STACK, k) for k in _build.STACK_KD} | {(_build.SWEEP, q) for q in _build.SWEEP_NQ}


def test_the_built_library_breaks_no_pin(facts):
    assert set(facts["kernels"]) == set(_build.PINS)
    for key, f in facts["kernels"].items():
        assert _build._violations(key, f) == [], key
    _build._check_facts(facts)


@pytest.mark.parametrize("key", list(MEMBERS), ids=str)
def test_each_violated_pin_raises_and_names_kernel_and_pin(facts, key):
    pins = _build.PINS[key]
    cases = perturbations(key)
    # every field of the record is covered by a case
    want = {"scratch", "spill"} if pins.mfma is None else {"scratch", "spill", "mfma", "dma +1", "store", "x4 load", "tile map"} | \
        ({"lane spill"} if pins.lane_spill_ops is not None else set())
    assert want <= {c[0] for c in cases}
    for what, change, phrase in cases:
        f = copy.deepcopy(facts["kernels"][key])
        change(f)
        bad = _build._violations(key, f)
        assert len(bad) == 1 and phrase in bad[0], (key, what, bad)
        broken = {"kernels": {**facts["kernels"], key: f}, "prefetch_hazards": facts["prefetch_hazards"]}
        with pytest.raises(_build.IsaCheckError) as e:
            _build._check_facts(broken)
        assert str(e.value).startswith(MEMBERS[key] + ": ") and phrase in str(e.value), (key, what, str(e.value))
    # a pin that is not set is not checked: the strip kernel keeps its 5 lane-spill instructions
    if pins.mfma is not None and pins.lane_spill_ops is None:
        f = copy.deepcopy(facts["kernels"][key])
        f["lane_spill_ops_in_chunk_loop"] += 1
        assert _build._violations(key, f) == []


def test_a_kernel_without_its_chunk_loop_is_refused(facts):
    f = copy.deepcopy(facts["kernels"][128])
    f["_has_chunk_loop"] = False
    assert _build._violations(128, f) == ["no loop holds the kernel's MFMAs"]
    assert _build._complaint(128, _build._violations(128, f)) == "k_gemm3m_pipe<128>: no loop holds the kernel's MFMAs"


@pytest.mark.parametrize("key", list(MEMBERS), ids=str)
def test_a_missing_kernel_is_refused(facts, key):
    less = {"kernels": {k: f for k, f in facts["kernels"].items() if k != key}, "prefetch_hazards": facts["prefetch_hazards"]}
    with pytest.raises(_build.IsaCheckError, match="update kernels found"):
        _build._check_facts(less)


def test_a_prefetch_hazard_is_refused(facts):
    assert facts["prefetch_hazards"] and not any(facts["prefetch_hazards"].values())       # the k_fill_red instances are there and clean
    name = next(iter(facts["prefetch_hazards"]))
    bad = {"kernels": facts["kernels"], "prefetch_hazards": {**facts["prefetch_hazards"], name: ["0x40: v_mov_b32 v1, v2"]}}
    with pytest.raises(_build.IsaCheckError, match="1 instructions touch a prefetch register"):
        _build._check_facts(bad)


def test_one_disassembly_serves_check_isa_and_the_accessors(facts, monkeypatch):
    def never(*a, **k):
        raise AssertionError("the library was disassembled again")
    monkeypatch.setattr(_build, "_disassemble", never)
    monkeypatch.setattr(_build, "_code_objects", never)
    assert _build._isa_facts() is facts
    rep = _build.check_isa()
    assert sorted(rep) == [64, 128, 192, 256]
    assert _build.check_isa_klong() == _build.check_isa(_all_kernels=True)[_build.KLONG]
    assert set(_build.check_isa_stack()) == set(_build.STACK_KD) | {_build.SLAB}
    assert sorted(_build.check_isa_narrow()) == list(_build.NARROW_NF) and sorted(_build.check_isa_sweep()) == list(_build.SWEEP_NQ)
    assert _build.check_isa_strip()["vm"]["global_load_dwordx4"] == _build.PINS[_build.STRIP].loads
    # reports are copies without the check's private entries: changing one does not reach the cache
    assert not any(k.startswith("_") for r in _build.check_isa(_all_kernels=True).values() for k in r)
    rep[128]["vm"]["global_load_lds_dwordx4"] += 1
    assert _build.check_isa()[128]["vm"]["global_load_lds_dwordx4"] == _build.EXPECTED_LDS_DMA[128]
