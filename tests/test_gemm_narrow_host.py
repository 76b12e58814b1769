"""The narrow launch of the left-looking bulk update, host side (no GPU).

The last tile column of an n_pad system holds n_pad - n_active columns of identity padding, where U is zero off the diagonal.  Under the
left-looking update the band at row J may split that tile column off into a launch of k_gemm3m_narrow<NF>, which multiplies NF of the
tile's four 16-column groups (launch_gemm_left, gemm_narrow_frags in kernels_gemm3m.hip).  This module checks

  * the rule, biem_gemm_narrow_frags(nb, n_pad, n_active, J), against a model: the NF formula, the 512-tile rule, the whole-band
    exception and the switch BIEM_GEMM_NARROW;
  * its declaration in include/biem_mi355.h against _lib.SIGNATURES;
  * the pins of the three instances in the built library (check_isa_narrow), and that check_isa's default report keeps its keys.
"""
import os
import re

import pytest

from biem_helmholtz_sphere_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 64
GRID_CAP = 512          # persistent grid of the update kernels (GEMM_GRID_CAP)


def narrow_frags(nb, n_pad, n_active, J, mode=None):
    """Model of gemm_narrow_frags.  mode: BIEM_GEMM_NARROW ("0" off, "1" no size rule, None the rule)."""
    pad = n_pad - n_active
    if mode == "0" or not 0 < J < n_pad or pad < 0 or pad >= NB:
        return 4
    nf = -(-(NB - pad) // 16)
    if nf >= 4:
        return 4
    w = (n_pad - J) // NB                  # tile columns from the band's diagonal on
    h = min(4, w)                          # tile rows of the band = tiles of its last tile column
    if mode != "1" and w != 1 and h * nb < GRID_CAP:
        return 4
    return nf


@pytest.fixture()
def lib(monkeypatch):
    monkeypatch.delenv("BIEM_GEMM_NARROW", raising=False)
    return _lib.load()


def test_nf_formula(lib):
    """NF = ceil((64 - padding) / 16), 4 (whole launch) below 16 padding columns; 256 systems pass the size rule at every band."""
    n_pad = 3392
    for pad, nf in ((0, 4), (1, 4), (15, 4), (16, 3), (17, 3), (31, 3), (32, 2), (47, 2), (48, 1), (63, 1)):
        for J in (256, 1024, 3072):
            assert lib.biem_gemm_narrow_frags(256, n_pad, n_pad - pad, J) == nf == narrow_frags(256, n_pad, n_pad - pad, J), (pad, J)
    # no band at J = 0 (the first group takes no bulk update) or outside the matrix
    assert lib.biem_gemm_narrow_frags(256, n_pad, n_pad - 32, 0) == 4
    assert lib.biem_gemm_narrow_frags(256, n_pad, n_pad - 32, n_pad) == 4


def test_size_rule_and_whole_band(lib):
    """The headline shape (cfg 3: 3360 -> 3392 and 3040 -> 3072 rows, 32 padding columns) splits at 256 and 128 systems - 4 nb >= 512
    narrow tiles - and stays whole at 64; the one-tile last band of the 53-tile block is narrow at any batch size."""
    for n_pad, n_active in ((3392, 3360), (3072, 3040)):
        T = n_pad // NB
        for J in range(256, n_pad, 256):
            w = T - J // NB
            for nb, on in ((256, True), (128, True), (127, False), (64, False), (1, False)):
                want = 2 if on or w == 1 else 4
                assert lib.biem_gemm_narrow_frags(nb, n_pad, n_active, J) == want, (n_pad, J, nb)
    assert lib.biem_gemm_narrow_frags(1, 3392, 3360, 3328) == 2            # T = 53: the last band is one diagonal tile
    assert lib.biem_gemm_narrow_frags(64, 3072, 3040, 2816) == 4           # T = 48: the last band is 4 x 4, 256 narrow tiles
    # cfg 4 (4064 -> 4096, 64 systems): whole.  cfg 5 (28 and 21 tile columns, 32 and 24 padding columns) at 256 systems: NF 2 and 3
    assert all(lib.biem_gemm_narrow_frags(64, 4096, 4064, J) == 4 for J in range(256, 4096, 256))
    assert all(lib.biem_gemm_narrow_frags(256, 1792, 1760, J) == 2 for J in range(256, 1792, 256))
    assert all(lib.biem_gemm_narrow_frags(256, 1344, 1320, J) == 3 for J in range(256, 1344, 256))
    # short last bands: h = w = 2 tiles per system need 256 systems, h = w = 3 need 171
    assert lib.biem_gemm_narrow_frags(256, 640, 600, 512) == 2 and lib.biem_gemm_narrow_frags(255, 640, 600, 512) == 4
    assert lib.biem_gemm_narrow_frags(171, 704, 660, 512) == 2 and lib.biem_gemm_narrow_frags(170, 704, 660, 512) == 4


def test_rule_against_the_model_on_a_grid(lib, monkeypatch):
    for mode in (None, "0", "1", "rule"):
        if mode is None:
            monkeypatch.delenv("BIEM_GEMM_NARROW", raising=False)
        else:
            monkeypatch.setenv("BIEM_GEMM_NARROW", mode)
        m = mode if mode in ("0", "1") else None          # any other value leaves the rule in place
        for nb in (1, 8, 127, 128, 170, 171, 255, 256, 512, 1024):
            for n_pad in (320, 512, 576, 640, 704, 768, 1344, 3072, 3392):
                for pad in (0, 15, 16, 24, 32, 48, 63):
                    for J in range(0, n_pad + 256, 256):
                        got = lib.biem_gemm_narrow_frags(nb, n_pad, n_pad - pad, J)
                        assert got == narrow_frags(nb, n_pad, n_pad - pad, J, m), (mode, nb, n_pad, pad, J, got)


def test_header_declares_the_query():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    decl = re.search(r"\bint biem_gemm_narrow_frags\(([^;]*)\);", hdr)
    assert decl, "biem_gemm_narrow_frags is not declared in include/biem_mi355.h"
    params = [p.split() for p in decl.group(1).split(",")]
    assert [p[-1] for p in params] == ["nb", "n_pad", "n_active", "J"] and all(p[:-1] == ["int"] for p in params)
    ret, args = _lib.SIGNATURES["biem_gemm_narrow_frags"]
    assert len(args) == 4 and all(a is args[0] for a in args) and ret is args[0]


def test_isa_check_covers_the_narrow_kernels():
    """k_gemm3m_narrow<NF> under the pins of the K-long instance: no scratch, no spills, 24 NF MFMAs per chunk in one loop, the K-long
    kernel's 32 LDS-DMA and 48 stores as the only vector-memory instructions, no lane spills in the chunk loop.  The default report of
    check_isa keeps its keys."""
    _lib.load()
    rep = _build.check_isa_narrow()
    klong = _build.check_isa_klong()
    assert sorted(rep) == [1, 2, 3] == sorted(_build.NARROW_NF)
    for nf, r in rep.items():
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (nf, r)
        assert r["mfma_in_chunk_loop"] == r["mfma_total"] == 24 * nf, (nf, r)
        assert r["vm"] == klong["vm"] == {"global_load_lds_dwordx4": _build.EXPECTED_LDS_DMA_KLONG, "global_store_dwordx4": _build.EXPECTED_STORES}, (nf, r)
        assert r["lane_spill_ops_in_chunk_loop"] <= _build.MAX_LANE_SPILL_OPS_KLONG, (nf, r)
    assert sorted(_build.check_isa()) == [64, 128, 192, 256]
