"""GPU tests of the split form of the symmetric path: flat sphere layouts (every centre at the same last canonical coordinate) are
filled as A~ = diag(E, O) - cosine block, sine block - and factored as two blocks by the existing factorisation on two views of one
allocation (tests/test_sym_split_host.py has the structure itself on the oracle).

Every case solves the same inputs three times - BIEM_SYM_SPLIT=1 (the size rule dropped, so that small shapes take the path), =0
(unsplit) and BIEM_SOLVER=lu - asserts through biem_last_solve_split which form ran, and compares the densities: 1e-10 of the largest
density entry, the parity contract of BASELINE.md (ldlt against lu measures 1e-14 to 3e-13 elsewhere in the suite).  The measured
values are printed.

Shapes: `ba`, 4 balls, n_end 13: E = 364 -> 384 (6 tiles: two groups, last band of two tile rows), O = 312 -> 320 (5 tiles, last band
of one row); `ba`, 2 balls, n_end 11: E = 132 on the general path, O = 110 in the one-launch small path; n_end 10: both blocks small.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch
except ImportError:
    torch = None

gpu = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def amd():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), device="cuda").to(dtype or torch.float64).contiguous()


def _last_split():
    from biem_helmholtz_sphere_amd import _lib as L

    a, b = C.c_int(-1), C.c_int(-1)
    L.check(L.load().biem_last_solve_split(C.byref(a), C.byref(b)))
    return a.value, b.value


# square lattice of equal spheres in the plane x2 = 0.3 (pairs with equal displacement: the fill's pair classes are not trivial)
SQUARE = np.array([[0.0, 0.0, 0.3], [2.5, 0.0, 0.3], [0.0, 2.5, 0.3], [2.5, 2.5, 0.3]])
PAIR = np.array([[0.0, 1.3, -0.2], [0.4, -1.2, -0.2]])


def _solve(amd, monkeypatch, env, tree, cen, rad, n_end, nb, nrhs, geom_per_system=False, **kw):
    """density [nrhs, nb, B, H] (NumPy), (npE, npO) of the run (None under BIEM_SOLVER=lu), the solve statistics."""
    from biem_helmholtz_sphere_amd import _biem as impl

    cen, rad = np.asarray(cen, float), np.asarray(rad, float)
    d = cen.shape[-1]
    ks = np.linspace(0.8, 2.4, nb)[None, :]                                     # (1, K)
    ang = 0.4 + 0.9 * np.arange(nrhs)
    dirs = np.zeros((d, nrhs, 1))
    dirs[0, :, 0], dirs[1, :, 0] = np.cos(ang) * 0.8, np.sin(ang) * 0.8
    dirs[d - 1, :, 0] += 0.6 if d > 2 else 0.0                                  # (not in the plane of the centres: no symmetry of the field)
    dirs /= np.linalg.norm(dirs, axis=0, keepdims=True)
    c = amd.create_from_branching_types(tree)
    if geom_per_system:
        cen_t, rad_t = _dev(np.broadcast_to(cen, (1, nb) + cen.shape)), _dev(np.broadcast_to(rad, (1, nb) + rad.shape))
    else:
        cen_t, rad_t = _dev(cen)[None, None], _dev(rad)[None, None]
    with monkeypatch.context() as mp:
        for name in ("BIEM_SYM_SPLIT", "BIEM_SOLVER"):
            mp.delenv(name, raising=False)
        for name, val in env.items():
            mp.setenv(name, val)
        uin, ugr = amd.plane_wave(k=_dev(ks), direction=_dev(dirs))
        calc = amd.biem(c, centers=cen_t, radii=rad_t, k=_dev(ks), n_end=n_end, uin=uin, uin_grad=ugr, **kw)
        dens = calc.density.cpu().numpy()
        how = None if env.get("BIEM_SOLVER") == "lu" else _last_split()
        stats = dict(impl._last_solve_stats)
    assert dens.shape[:2] == (nrhs, nb) and np.all(np.isfinite(dens))
    return dens, how, stats


def _three_ways(amd, monkeypatch, expect, *args, env=None, **kw):
    """The split, the unsplit and the LU run of one case; `expect`: (npE, npO) the BIEM_SYM_SPLIT=1 run must report."""
    env = dict(env or {})
    got, how, st = _solve(amd, monkeypatch, {**env, "BIEM_SYM_SPLIT": "1"}, *args, **kw)
    assert how == expect, (how, expect)
    assert (st["ldlt_systems"], st["lu_systems"]) == (got.shape[1], 0), st
    plain, how0, _ = _solve(amd, monkeypatch, {**env, "BIEM_SYM_SPLIT": "0"}, *args, **kw)
    assert how0 == (0, 0), how0
    lu, _, _ = _solve(amd, monkeypatch, {**env, "BIEM_SOLVER": "lu"}, *args, **kw)
    scale = np.abs(lu).max()
    e0, e1 = np.abs(got - plain).max() / scale, np.abs(got - lu).max() / scale
    print(f"split {expect}: against unsplit {e0:.2e}, against lu {e1:.2e} (unsplit against lu {np.abs(plain - lu).max() / scale:.2e})")
    assert e0 <= TOL and e1 <= TOL, (e0, e1)
    return got


@gpu
@pytest.mark.parametrize("nb", [3, 12])
@pytest.mark.parametrize("nrhs", [1, 8, 9])
def test_four_balls_two_groups(amd, monkeypatch, nb, nrhs):
    """3 systems: the stored-inverse back substitution (keep_w); 12: the column form.  1 and 8 right-hand sides leave the matrix, 9 ride as
    tile columns - in E they land in the unused E x O rectangle."""
    _three_ways(amd, monkeypatch, (384, 320), "ba", SQUARE, np.ones(4), 13, nb, nrhs)


@gpu
@pytest.mark.parametrize("nrhs", [1, 9])
def test_production_launch_forms_on_the_views(amd, monkeypatch, nrhs):
    """Left-looking bulk update and stacked group passes on views whose n_pad (384, 320) is no multiple of 256."""
    _three_ways(amd, monkeypatch, (384, 320), "ba", SQUARE, np.ones(4), 13, 12, nrhs, env={"BIEM_SYM_UPDATE": "left", "BIEM_SYM_GROUP": "stacked"})


@gpu
@pytest.mark.parametrize("n_end,expect", [(11, (192, 128)), (10, (128, 128))])
def test_small_blocks(amd, monkeypatch, n_end, expect):
    """n_end 11: E = 132 on the general path, O = 110 in one LDS-resident launch; n_end 10: E = 110 and O = 90, both in one launch each."""
    _three_ways(amd, monkeypatch, expect, "ba", PAIR, [1.0, 0.8], n_end, 3, 1)


@gpu
def test_bba_flat_in_x3(amd, monkeypatch):
    cen = [[0.0, 1.6, 0.2, 0.25], [0.3, -1.5, 0.0, 0.25]]
    _three_ways(amd, monkeypatch, (192, 128), "bba", cen, [1.0, 0.8], 7, 3, 2)        # H = 140: 84 cosine, 56 sine slots per ball


@gpu
def test_bpa_flat_in_x0(amd, monkeypatch):
    """bpa runs as ba in the axes (x2, x1, x0): its last canonical coordinate is the caller's x0."""
    cen = [[-0.1, 1.6, 0.2], [-0.1, -1.5, 0.0], [-0.1, 0.1, 2.9]]
    _three_ways(amd, monkeypatch, (128, 128), "bpa", cen, [1.0, 0.8, 0.6], 8, 3, 1)   # H = 64: 36 + 28; E = 108, O = 84


@gpu
def test_minus_zero_is_in_the_plane_of_zero(amd, monkeypatch):
    cen = PAIR.copy()
    cen[:, 2] = [0.0, -0.0]
    _three_ways(amd, monkeypatch, (128, 128), "ba", cen, [1.0, 0.8], 10, 3, 1)


@gpu
@pytest.mark.parametrize("case", ["one ulp off the plane", "flat in x1 only", "geometry per system", "caa", "collinear in 2-D"])
def test_layouts_that_run_unsplit(amd, monkeypatch, case):
    """The override drops the size rule only: none of these takes the split form, and the results agree as before."""
    kw = {}
    if case == "one ulp off the plane":
        cen = PAIR.copy()
        cen[1, 2] = np.nextafter(cen[1, 2], 1.0)
        args = ("ba", cen, [1.0, 0.8], 10, 3, 1)
    elif case == "flat in x1 only":
        args = ("ba", [[0.0, 0.5, 1.3], [0.4, 0.5, -1.2]], [1.0, 0.8], 10, 3, 1)
    elif case == "geometry per system":
        args, kw = ("ba", PAIR, [1.0, 0.8], 10, 3, 1), {"geom_per_system": True}
    elif case == "caa":
        args = ("caa", [[0.0, 1.6, 0.2, 0.25], [0.3, -1.5, 0.0, 0.25]], [1.0, 0.8], 6, 3, 1)
    else:
        args = ("a", [[0.0, 0.2], [2.4, 0.2], [-2.2, 0.2]], [1.0, 0.8, 0.6], 40, 3, 1)         # N = 237 by the list-free 2-D fill
    _three_ways(amd, monkeypatch, (0, 0), *args, **kw)


@gpu
def test_size_rule(amd, monkeypatch):
    """Without the override a flat call below 1024 unknowns runs unsplit, one of 1024 (ba, 4 balls, n_end 16: E = 544 -> 576,
    O = 480 -> 512) runs split - and agrees with the unsplit run and the LU."""
    _, how, _ = _solve(amd, monkeypatch, {}, "ba", SQUARE, np.ones(4), 13, 3, 1)
    assert how == (0, 0), how
    got, how, _ = _solve(amd, monkeypatch, {}, "ba", SQUARE, np.ones(4), 16, 2, 1)
    assert how == (576, 512), how
    plain, how0, _ = _solve(amd, monkeypatch, {"BIEM_SYM_SPLIT": "0"}, "ba", SQUARE, np.ones(4), 16, 2, 1)
    lu, _, _ = _solve(amd, monkeypatch, {"BIEM_SOLVER": "lu"}, "ba", SQUARE, np.ones(4), 16, 2, 1)
    scale = np.abs(lu).max()
    e0, e1 = np.abs(got - plain).max() / scale, np.abs(got - lu).max() / scale
    print(f"default rule at N = 1024: against unsplit {e0:.2e}, against lu {e1:.2e}")
    assert how0 == (0, 0) and e0 <= TOL and e1 <= TOL, (how0, e0, e1)


@gpu
def test_robin_coefficients(amd, monkeypatch):
    _three_ways(amd, monkeypatch, (384, 320), "ba", SQUARE, np.ones(4), 13, 3, 2, alpha=1.0, beta=0.3)


@gpu
def test_degree_dependent_coefficients(amd, monkeypatch):
    """The *_n entry: coefficients per (ball, degree), every pair its own class."""
    n_end = 13
    n = np.arange(n_end)
    an = np.stack([1.0 + 0.05 * n + 0.02j * (b + 1) for b in range(4)])
    bn = np.stack([0.3 / (1.0 + 0.1 * n) + 0.01j * b for b in range(4)])
    _three_ways(amd, monkeypatch, (384, 320), "ba", SQUARE, np.ones(4), n_end, 3, 2,
                alpha_n=_dev(an, torch.complex128)[None, None], beta_n=_dev(bn, torch.complex128)[None, None])


@gpu
@pytest.mark.parametrize("env", [{"BIEM_FILL_DEDUPE_MIN": "1"}, {"BIEM_FILL_NO_DEDUPE": "1"}])
def test_pair_classes_on_and_off(amd, monkeypatch, env):
    """Classes for 3 systems (off by default below 8), none for 12 (on by default): the square lattice has 4 classes among its 6 pairs."""
    nb = 3 if "BIEM_FILL_DEDUPE_MIN" in env else 12
    _three_ways(amd, monkeypatch, (384, 320), "ba", SQUARE, np.ones(4), 13, nb, 1, env=env)


@gpu
def test_two_identical_calls_agree_bit_for_bit(amd, monkeypatch):
    a, how, _ = _solve(amd, monkeypatch, {"BIEM_SYM_SPLIT": "1"}, "ba", SQUARE, np.ones(4), 13, 12, 2)
    b, _, _ = _solve(amd, monkeypatch, {"BIEM_SYM_SPLIT": "1"}, "ba", SQUARE, np.ones(4), 13, 12, 2)
    assert how == (384, 320) and np.array_equal(a, b)


@gpu
def test_every_system_rejected_goes_to_the_pivoted_lu(amd, monkeypatch):
    """BIEM_LDLT_PIVOT_REL=1e30 rejects every pivot: the merged codes are negative for every system, all are solved by the LU."""
    got, how, st = _solve(amd, monkeypatch, {"BIEM_SYM_SPLIT": "1", "BIEM_LDLT_PIVOT_REL": "1e30"}, "ba", SQUARE, np.ones(4), 13, 3, 2)
    assert how == (384, 320) and (st["ldlt_systems"], st["lu_systems"]) == (3, 3), (how, st)
    assert all(c < 0 for c in st["rejected_info"]), st
    lu, _, _ = _solve(amd, monkeypatch, {"BIEM_SOLVER": "lu"}, "ba", SQUARE, np.ones(4), 13, 3, 2)
    err = np.abs(got - lu).max() / np.abs(lu).max()
    print(f"all systems rejected: against lu {err:.2e}")
    assert err <= TOL
