"""Host tests of incidence by expansion coefficients (no GPU): the argument checks of the coefficient pairs, the order inferred from the
length of the coefficient axis for every tree and the exports.  tests/test_gpu_expansion.py runs the kernels."""
import numpy as np
import pytest

import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd import _build, _lib
from biem_helmholtz_sphere_amd._biem import _closed_form_request
from biem_helmholtz_sphere_amd._coords import harm_count
from biem_helmholtz_sphere_amd._incident import _harmonic_order

ENTRIES = ["biem_rhs_expansion", "biem_solve_ex", "biem_solve_ldlt_ex", "biem_solve_factored_ex", "biem_expansion_field"]


def request(c, k, n_end, **kw):
    names = ["uin", "uin_grad", "plane_wave_direction", "point_source_position", "multipole_source_position", "multipole_source_index",
             "regular_wave_origin", "regular_wave_index", "regular_wave_coefficients", "multipole_source_coefficients"]
    assert set(kw) <= set(names)
    return _closed_form_request(c, k, n_end, *(kw.get(n) for n in names))


@pytest.mark.parametrize("pos,coef,idx", [("regular_wave_origin", "regular_wave_coefficients", "regular_wave_index"),
                                         ("multipole_source_position", "multipole_source_coefficients", "multipole_source_index")])
def test_argument_errors_need_no_device(pos, coef, idx):
    c = amd.create_from_branching_types("ba")
    k, o, P = np.array(1.1), np.array([0.1, 0.2, 3.0]), np.ones(9, dtype=np.complex128)
    with pytest.raises(ValueError, match=f"{pos} and {coef} must be given together"):
        request(c, k, 4, **{coef: P})
    with pytest.raises(ValueError, match=f"{coef} replaces {idx}"):
        request(c, k, 4, **{pos: o, coef: P, idx: 1})
    others = [dict(plane_wave_direction=o), dict(point_source_position=o), dict(uin=lambda x: x), dict(uin_grad=lambda x: x)]
    others.append(dict(multipole_source_position=o, multipole_source_index=0) if pos.startswith("regular") else
                  dict(regular_wave_origin=o, regular_wave_index=0))
    for other in others:
        with pytest.raises(ValueError, match=f"{coef} replaces uin / uin_grad"):
            request(c, k, 4, **{pos: o, coef: P}, **other)
    with pytest.raises(ValueError, match="replaces"):
        request(c, k, 4, regular_wave_origin=o, regular_wave_coefficients=P, multipole_source_position=o, multipole_source_coefficients=P)
    with pytest.raises(ValueError, match=r"length 10, which is no harmonic count of the tree: the nearest valid lengths are 9 \(n_in=3\) and 16 \(n_in=4\)"):
        request(c, k, 4, **{pos: o, coef: np.ones(10)})
    with pytest.raises(ValueError, match="got a scalar"):
        request(c, k, 4, **{pos: o, coef: 1.0})
    with pytest.raises(ValueError, match="must be a complex"):
        request(c, k, 4, **{pos: o, coef: np.array(["a"] * 9)})
    with pytest.raises(ValueError, match=f"first dimension of {pos}"):
        request(c, k, 4, **{pos: np.zeros(2), coef: P})
    with pytest.raises(ValueError, match="not broadcastable"):
        request(c, np.ones(4), 4, **{pos: np.zeros((3, 4)), coef: np.ones((5, 9))})
    with pytest.raises(ValueError, match="not broadcastable"):                         # (more axes than the positions have)
        request(c, k, 4, **{pos: o, coef: np.ones((2, 9))})
    name, (S, Pc, n_in), given = request(c, np.ones(1), 4, **{pos: np.zeros((3, 5)), coef: np.ones((5, 25))})
    assert name == coef and S.shape == (3, 5) and S.dtype == np.float64 and n_in == 5 and Pc.shape == (5, 25)
    # the index pair is untouched
    name, (S, I), _ = request(c, np.ones(1), 4, **{pos: np.zeros((3, 5)), idx: np.arange(5)})
    assert name == pos and I.tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "bpbpa", "caa", "bbba", "bbbba"])
def test_the_order_is_inferred_from_the_length_for_every_tree(tree):
    c = amd.create_from_branching_types(tree)
    counts = [harm_count(tree, n) for n in range(1, 9)]
    assert counts == sorted(set(counts))
    for n, H in enumerate(counts, start=1):
        assert _harmonic_order(c, H, "P") == n
        if n > 1 and H - 1 != counts[n - 2]:
            with pytest.raises(ValueError, match=rf"nearest valid lengths are {counts[n - 2]} \(n_in={n - 1}\) and {H} \(n_in={n}\)"):
                _harmonic_order(c, H - 1, "P")
    with pytest.raises(ValueError, match=r"nearest valid lengths are 1 \(n_in=1\)"):
        _harmonic_order(c, 0, "P")
    # the field functions infer it the same way, before any device is touched
    for make, key in ((amd.regular_expansion, "origin"), (amd.multipole_expansion, "source")):
        with pytest.raises(ValueError, match="no harmonic count of the tree"):
            make(c, k=np.array(1.0), coefficients=np.ones(counts[2] + 1), **{key: np.zeros(c.c_ndim)})
        with pytest.raises(ValueError, match=f"first dimension of {key}"):
            make(c, k=np.array(1.0), coefficients=np.ones(counts[2]), **{key: np.zeros(c.c_ndim + 1)})
        with pytest.raises(ValueError, match="not broadcastable"):
            make(c, k=np.ones(4), coefficients=np.ones((5, counts[2])), **{key: np.zeros((c.c_ndim, 4))})


def test_plane_wave_coefficients_checks_its_order_first():
    c = amd.create_from_branching_types("ba")
    with pytest.raises(ValueError, match="n_in must be positive"):
        amd.plane_wave_coefficients(c, k=np.array(1.0), direction=np.array([0.0, 0.0, 1.0]), origin=np.zeros(3), n_in=0)


def test_exports_and_signatures():
    for name in ("regular_expansion", "multipole_expansion", "plane_wave_coefficients"):
        assert name in amd._biem.__all__ and callable(getattr(amd, name))
    import inspect

    for fn in (amd.biem, amd._biem.BIEMFactorization.solve):
        assert {"regular_wave_coefficients", "multipole_source_coefficients"} <= set(inspect.signature(fn).parameters)
    for name in ENTRIES + ["biem_rhs_expansion_workspace_bytes"]:
        assert name in _lib.SIGNATURES, name


def test_library_cross_compiles_and_refuses_bad_arguments_before_any_device_call():
    _build.build(force=False)
    assert not _build.is_stale()
    assert "kernels_rhs_ex.hip" in _build.SOURCES and "rhs_translate.hpp" in _build.HEADERS
    lib = _lib.load()
    assert lib.biem_rhs_expansion_workspace_bytes(None, 4, 3, 1) == 0
    for name in ENTRIES:
        args = [0 if t is _lib._i or t is _lib._ll or t is _lib._sz else None for t in _lib.SIGNATURES[name][1]]
        rc = getattr(lib, name)(*args)                                   # no plan: an argument error, no device touched
        assert rc == 1 and name.encode() in lib.biem_last_error(), (name, lib.biem_last_error())
