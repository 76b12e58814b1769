"""CPU tests of the degree-dependent boundary coefficients (``biem(alpha_n=, beta_n=)``, ``fluid_inclusion_bc``): the public
surface, the argument checks that run before any device work, and the C declarations of the new entry points."""
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import biem_helmholtz_sphere_amd as amd  # noqa: E402
from biem_helmholtz_sphere_amd import _build, _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N_END = 2, 4


def _kw(**over):
    kw = dict(centers=np.array([[0.0, 0.0, 2.0], [0.0, 0.0, -2.0]]), radii=np.ones(B), k=np.asarray(1.3), n_end=N_END)
    kw.update(over)
    return kw


def _c():
    return amd.create_from_branching_types("ba")


@pytest.mark.parametrize("fn", [amd.biem, amd.biem_factorize])
def test_pair_is_given_together(fn):
    one = np.ones((B, N_END))
    for kw in (dict(alpha_n=one), dict(beta_n=one)):
        with pytest.raises(ValueError, match="alpha_n and beta_n must be given together"):
            fn(_c(), **_kw(**kw))


@pytest.mark.parametrize("fn", [amd.biem, amd.biem_factorize])
def test_shape_errors(fn):
    one = np.ones((B, N_END))
    with pytest.raises(ValueError, match=f"The last dimension of alpha_n must be n_end={N_END}, but got {N_END + 1}"):
        fn(_c(), **_kw(alpha_n=np.ones((B, N_END + 1)), beta_n=one))
    with pytest.raises(ValueError, match=f"The last dimension of beta_n must be n_end={N_END}, but got 1"):
        fn(_c(), **_kw(alpha_n=one, beta_n=np.ones((B, 1))))
    with pytest.raises(ValueError, match=r"alpha_n must be an array of shape \(\.\.\., B, n_end\) with 2 axes"):
        fn(_c(), **_kw(alpha_n=np.ones(N_END), beta_n=one))                       # the ball axis is missing
    with pytest.raises(ValueError, match="are not broadcastable"):
        fn(_c(), **_kw(alpha_n=np.ones((B + 1, N_END)), beta_n=one))              # three rows for two balls
    # a batch axis of 3 wavenumbers against a batch axis of 2 sets of coefficients
    kb = _kw(k=np.array([1.0, 1.1, 1.2]), centers=_kw()["centers"][None], radii=np.ones((1, B)))
    with pytest.raises(ValueError, match="are not broadcastable"):
        fn(_c(), **dict(kb, alpha_n=np.ones((2, B, N_END)), beta_n=np.ones((1, B, N_END))))


@pytest.mark.parametrize("fn", [amd.biem, amd.biem_factorize])
@pytest.mark.parametrize("ab", [dict(alpha=2.0), dict(beta=1.0), dict(alpha=np.ones(B)), dict(beta=np.zeros(B))])
def test_not_combined_with_alpha_or_beta(fn, ab):
    one = np.ones((B, N_END))
    with pytest.raises(ValueError, match="leave alpha and beta at their defaults"):
        fn(_c(), **_kw(alpha_n=one, beta_n=one, **ab))


def test_messages_of_the_scalar_pair_are_unchanged():
    with pytest.raises(ValueError, match=r"alpha and beta must be scalars or arrays of shape \(\.\.\., B\) with 1 axes"):
        amd.biem(_c(), **_kw(alpha=np.ones((1, B))))


def test_defaults_and_record_are_unchanged():
    for fn in (amd.biem, amd.biem_factorize):
        p = inspect.signature(fn).parameters
        assert p["alpha"].default == 1.0 and p["beta"].default == 0.0
        for nm in ("alpha_n", "beta_n"):
            assert p[nm].default is None and p[nm].kind is inspect.Parameter.KEYWORD_ONLY
    assert amd.BIEMResultCalculator.__slots__ == ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")
    assert "fluid_inclusion_bc" in amd.__all__ and callable(amd.fluid_inclusion_bc)
    assert [p.kind for p in inspect.signature(amd.fluid_inclusion_bc).parameters.values()] == [inspect.Parameter.KEYWORD_ONLY] * 6
    assert inspect.signature(amd.fluid_inclusion_bc).parameters["k"].default is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the helper computes (tests/test_gpu_degree_bc.py)")
def test_without_a_device_the_library_says_so():
    with pytest.raises(_lib.BiemLibraryError, match="no HIP device visible"):
        amd.fluid_inclusion_bc(c_ndim=3, n_end=N_END, radii=np.ones(B), k_interior=2.0, density_ratio=0.5)
    one = np.ones((B, N_END))
    with pytest.raises(_lib.BiemLibraryError, match="no HIP device visible"):     # valid arguments get as far as the device
        amd.biem(_c(), **_kw(alpha_n=one, beta_n=0 * one))


def test_new_entries_are_declared_bound_and_built():
    names = ["biem_ball_tables_n", "biem_rhs_project_n", "biem_solve_n", "biem_solve_ldlt_n", "biem_factor_ldlt_n", "biem_solve_factored_n",
             "biem_flag_unscalable"]
    with open(os.path.join(ROOT, "include", "biem_mi355.h")) as fh:
        header = fh.read()
    for nm in names:
        decl = re.search(r"\bint " + nm + r"\(([^;]*)\);", header)
        assert decl, nm
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[nm][1]), nm          # one ctypes type per declared argument
    # the per-degree kernels are instantiations of the scalar ones' templates: no translation unit of their own
    assert "kernels_tables.hip" in _build.SOURCES and "kernels_rhs.hip" in _build.SOURCES
    # the scalar entries keep their declarations: the per-degree ones are additions
    for nm in ("biem_ball_tables", "biem_rhs_project", "biem_solve", "biem_solve_ldlt", "biem_factor_ldlt", "biem_solve_factored"):
        assert re.search(r"\bint " + nm + r"\(", header), nm
