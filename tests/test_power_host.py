"""CPU tests of biem_power() / biem_far_pattern(): the identities that pin the yardstick (tests/power_yardstick.py) on the oracle, the
public surface, the argument checks that run before any device work, and the C declarations.

The identities are limited by the truncation at n_end = 8, not by rounding, hence 1e-9 and not the parity contract: energy balance
P_ext - sum P_abs = int |F|^2, the optical theorem, and the flux of the oracle's near field through a large sphere (measured when
the feature was written: at most 2.8e-11, 2.3e-10 and 3e-9 - the last is the error of the central difference, see _flux_bound).
"""
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _build, _lib
from oracle import biem_oracle as O

import power_yardstick as PY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N_END = 1.3, 8
COEFFICIENTS = {
    "soft": (1.0, 0.0),
    "robin": (1.0 + 0.5j, 0.3 - 0.2j),
    "per_ball": (np.array([0.4 + 0.1j, 1.0]), np.array([1.0, 0.0])),
}


def geometry(d):
    """Two balls, radii 1.0 / 0.7, centres 0.1 arange(d) and (2.5, 0.5, 0, ...); plane wave along (0.6, 0.8, 0, ...)."""
    cen = np.zeros((2, d))
    cen[0] = 0.1 * np.arange(d)
    cen[1, :2] = (2.5, 0.5)
    p = np.zeros(d)
    p[:2] = (0.6, 0.8)
    return cen, np.array([1.0, 0.7]), p


_SOLVED = {}


def solved(tree, case):
    """The oracle's solution of the test geometry (computed once per (tree, coefficients), never modified)."""
    key = (tree, case)
    if key not in _SOLVED:
        cen, rad, p = geometry(O.tree(tree).d)
        uin, ugr = O.plane_wave(K, p)
        a, b = COEFFICIENTS[case] if isinstance(case, str) else case
        res = O.solve_biem(tree, centers=cen, radii=rad, k=K, n_end=N_END, alpha=a, beta=b, uin=uin, uin_grad=ugr)
        _SOLVED[key] = (res, uin, ugr, p, PY.power(res, uin, ugr, a, b))
    return _SOLVED[key]


@pytest.mark.parametrize("case", sorted(COEFFICIENTS))
@pytest.mark.parametrize("tree", ["a", "ba", "bba"])
def test_energy_balance_and_optical_theorem(tree, case):
    res, _, _, p, (ext, ab, sca) = solved(tree, case)
    pattern = PY.pattern_power(res, 24)
    assert abs(pattern - PY.pattern_power(res, 32)) <= 1e-13 * pattern            # the rule resolves |F|^2
    balance = abs(ext.sum() - ab.sum() - pattern) / ext.sum()
    optical = abs(PY.optical_theorem(res, p) - ext.sum()) / ext.sum()
    print(f"{tree} {case}: P_ext {ext} P_abs {ab} P_sca {sca:.10f}  balance {balance:.1e}  optical theorem {optical:.1e}")
    assert ext.sum() > 0 and sca > 0 and (ab >= 0).all()
    if case == "soft":
        assert (ab == 0.0).all()
    assert balance <= 1e-9
    assert optical <= 1e-9


def _flux_bound(sca, ext, step):
    """Central difference of a field ~ e^{ikr}: relative error (k step)^2 / 6 of d_r u and so of the flux; twice that for the part of
    the field that is not yet asymptotic at the radius used, plus the energy-balance bound itself."""
    return (K * step) ** 2 / 3.0 * sca + 1e-9 * ext


@pytest.mark.parametrize("case", sorted(COEFFICIENTS))
@pytest.mark.parametrize("tree,nq", [("a", 40), ("ba", 24), ("bba", 12)])
def test_scattered_power_is_the_flux_of_the_near_field(tree, nq, case):
    res, _, _, _, (ext, _, sca) = solved(tree, case)
    step = 1e-4
    flux = PY.oracle_flux(res, 40.0, nq, step)
    print(f"{tree} {case}: P_sca {sca:.10f}  flux {flux:.10f}  difference / P_ext {abs(flux - sca) / ext.sum():.1e}")
    assert abs(flux - sca) <= _flux_bound(sca, ext.sum(), step)


def test_active_boundary_absorbs_negative_power():
    _, _, _, _, (ext, ab, sca) = solved("ba", (0.4 - 0.1j, 1.0))
    print(ext, ab, sca)
    assert (ab < 0).all()
    assert np.abs(ab - np.array([-2.06, -0.87])).max() < 0.01                     # the figures of the derivation


def test_true_pattern_differs_from_the_reference_formula_off_the_origin():
    """What far_pattern is for: the oracle's far field (the reference's formula) is no pattern for a ball off the origin - its |F|^2
    does not integrate to the scattered power - while for one ball at the origin both agree."""
    res, _, _, _, (_, _, sca) = solved("ba", "soft")
    y, w = res.tree.quadrature(24)
    reference = float(np.sum(w * np.abs(O.uscat(res, y, far_field=True)) ** 2))
    assert abs(reference - sca) > 0.1 * sca
    uin, ugr = O.plane_wave(K, [0.6, 0.8, 0.0])
    one = O.solve_biem("ba", centers=np.zeros((1, 3)), radii=[1.0], k=K, n_end=N_END, uin=uin, uin_grad=ugr)
    assert np.abs(PY.far_pattern(one, y) - O.uscat(one, y, far_field=True)).max() <= 1e-14


# ---------------------------------------------------------------------------- public surface and argument checks
def _result(bt="ba", n_end=3, **kw):
    from biem_helmholtz_sphere_amd._coords import harm_count

    c = amd.create_from_branching_types(bt)
    d = c.c_ndim
    base = dict(c=c, centers=np.zeros((d, 1)), radii=np.ones(1), k=np.array(1.0), eta=np.array(1.0), kind="outer", n_end=n_end,
                density=np.ones((1, harm_count(bt, n_end)), dtype=np.complex128), uin=lambda x, expand_x=True: np.ones(x.shape[1:]))
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_exported_and_methods_of_the_calculator():
    for name in ("biem_power", "biem_far_pattern", "BIEMPower"):
        assert name in amd.__all__ and hasattr(amd, name)
    assert callable(amd.BIEMResultCalculator.power) and callable(amd.BIEMResultCalculator.far_pattern)
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")
    rec = amd.BIEMPower(extinction=np.ones(2), absorption=np.zeros(2), scattering=np.float64(2.0))
    with pytest.raises(AttributeError):
        rec.scattering = 0.0                                                       # frozen
    assert "far_field=True" in amd.biem_far_pattern.__doc__                        # says how it differs from uscat(far_field=True)


def test_argument_errors_come_before_any_device_work():
    grad = lambda x: np.zeros(x.shape)
    with pytest.raises(ValueError, match="Invalid kind: inner"):
        amd.biem_power(_result(kind="inner"), uin_grad=grad)
    with pytest.raises(ValueError, match="Im k must be zero"):
        amd.biem_power(_result(k=np.array(1.0 + 0.1j)), uin_grad=grad)
    with pytest.raises(ValueError, match="Im k must be zero"):
        amd.biem_power(_result(k=np.array([1.0, 1.0 + 1e-300j])), uin_grad=grad)  # any system
    with pytest.raises(ValueError) as e:
        amd.biem_power(_result(density=None), uin_grad=grad)
    assert str(e.value) == "The BIEMResult does not have density."
    with pytest.raises(ValueError, match="uin must be provided"):
        amd.biem_power(_result(uin=None), uin_grad=grad)
    with pytest.raises(ValueError, match="uin_grad must be provided"):
        amd.biem_power(_result(), uin_grad=None)                                   # needed also for beta = 0
    with pytest.raises(TypeError):
        amd.biem_power(_result())                                                  # uin_grad is a required keyword
    with pytest.raises(ValueError, match="does not have density"):
        amd.biem_far_pattern(_result(density=None), np.ones((3, 2)))
    calc = amd.BIEMResultCalculator(c=amd.create_from_branching_types("ba"), centers=np.zeros((3, 1)), radii=np.ones(1), k=np.array(1.0),
                                    n_end=3, eta=np.array(1.0), kind="outer")
    with pytest.raises(ValueError, match="does not have density"):
        calc.power(uin_grad=grad)
    with pytest.raises(ValueError, match="does not have density"):
        calc.far_pattern(np.ones((3, 2)))


# ---------------------------------------------------------------------------- the C ABI
def _params(text, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split() for p in m.group(1).split(",")]


def test_header_declares_both_entries_with_the_signature_table_s_arguments():
    hdr = open(os.path.join(ROOT, "include", "biem_mi355.h")).read()
    plain, per_degree = _params(hdr, "biem_power"), _params(hdr, "biem_power_n")
    assert len(plain) == len(per_degree) == len(_lib.SIGNATURES["biem_power"][1]) == 17
    assert _lib.SIGNATURES["biem_power"] == _lib.SIGNATURES["biem_power_n"]
    assert [p[:-1] for p in plain] == [p[:-1] for p in per_degree]                 # the same types
    names = [p[-1].lstrip("*") for p in plain]
    assert names == ["plan", "nb", "B", "nrhs", "d_k", "d_eta", "d_radii", "geom_batched", "d_alpha", "d_beta", "ab_batched", "d_tab",
                     "d_density", "d_pu", "d_pv", "d_out", "stream"]
    assert [p[-1].lstrip("*") for p in per_degree] == [n + "_n" if n in ("d_alpha", "d_beta") else n for n in names]
    for (types_, name), ctype in zip(((p[:-1], p[-1]) for p in plain), _lib.SIGNATURES["biem_power"][1]):
        assert (ctype is _lib._i) == (types_ == ["int"]), (name, types_)         # ints are ints, everything else a pointer
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "biem_power" in text and "biem_power_n" in text


def test_library_cross_compiles_and_exports_the_entries():
    _build.build(force=False)                       # every translation unit for gfx950 (a no-op when the library matches the sources)
    assert not _build.is_stale()
    assert "kernels_power.hip" in _build.SOURCES
    lib = _lib.load()
    for name in ("biem_power", "biem_power_n"):
        fn = getattr(lib, name)
        rc = fn(*([None, 1, 1, 1] + [None] * 3 + [0] + [None] * 2 + [0] + [None] * 6))        # no plan: an argument error, no device touched
        assert rc == 1 and b"plan" in lib.biem_last_error() and name.encode() in lib.biem_last_error()


def test_power_kernel_uses_no_scratch():
    """k_power in the gfx950 code object: no private segment (the radial recurrences run in LDS), no spills."""
    objdump, readelf = _build._llvm_tool("llvm-objdump"), _build._llvm_tool("llvm-readelf")
    assert objdump and readelf
    _lib.load()
    with tempfile.TemporaryDirectory(prefix="biem_power_isa_") as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(_build.LIB, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        metas = {}
        for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            metas.update(_build._kernel_meta(readelf, os.path.join(tmp, o)))
    power = [m for n, m in metas.items() if "k_power" in n]
    assert len(power) == 1, sorted(metas)
    print(power[0])
    assert int(power[0]["private_segment_fixed_size"]) == 0 and int(power[0]["vgpr_spill_count"]) == 0 and int(power[0]["sgpr_spill_count"]) == 0
