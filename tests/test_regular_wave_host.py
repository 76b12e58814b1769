"""Host tests of tests/regular_wave_yardstick.py (no GPU): the (R|R) matrix the GPU tests of regular-wave incidence and of the cluster
coefficients are held against is pinned here to the addition theorem sampled at points and to (R|R)(0) = identity, and the public
argument checks that need no device are exercised."""
import numpy as np
import pytest

from oracle import biem_oracle as O

import regular_wave_yardstick as RW
from test_chain_trees_host import chain

CASES = [("a", 9), ("ba", 7), ("bpa", 6), ("bba", 5), ("bpbpa", 4), ("caa", 5), ("bbba", 4)]


def _tree(name):
    return O.tree(name) if name in O._TREES else chain(len(name) + 1)


def _points(d, rmax, n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, d))
    return rng.uniform(0.2, 1.0, (n, 1)) * rmax * v / np.linalg.norm(v, axis=-1, keepdims=True)


@pytest.mark.parametrize("k", [0.9, 0.7 + 0.25j, 0.7 - 0.25j], ids=["real", "im_plus", "im_minus"])
@pytest.mark.parametrize("name,n_end", CASES, ids=[c[0] for c in CASES])
def test_the_yardstick_satisfies_the_addition_theorem(name, n_end, k):
    """j_n'(k |c + r - o|) Y_h'(..) = sum_h RR[h', h] j_n(k |r|) Y_h(r^) at 12 points with |r| <= 0.3 |t|, t = c - o, |t| = 0.45, for every
    h'.  The series is cut at degree n_end - 1.  Its remainder is measured, not guessed: the entries of RR do not depend on the order, so
    the yardstick at order n_end + 1 supplies the first dropped degree, and with |k r| <= 0.13 successive degrees fall by more than a
    factor 4 (the ratio j_{n+1} / j_n < |k r| / 2 times the growth of the harmonics' count and size, below 8 here), so the whole tail is
    below twice its first term.  Bound: 2 x (first dropped degree) + 1e-13 sum_h |j_n Y_h|: the quadrature forms every entry of RR from
    terms of size one, so an entry carries an absolute error of a few 2^-53 however small it is itself (measured: 5e-17 on entries of
    1e-4), and for a high degree n' the field is far smaller than that scale."""
    tr = _tree(name)
    d = tr.d
    t = 0.45 * np.array([0.48, -0.6, 0.36, 0.52, -0.1][:d]) / np.linalg.norm([0.48, -0.6, 0.36, 0.52, -0.1][:d])
    o = np.array([0.3, -0.2, 0.5, 0.1, 0.7][:d])
    c = o + t
    r = _points(d, 0.3 * 0.45, 12, seed=n_end)
    RR = RW.translation_rr(tr, n_end, k, t)
    RR1 = RW.translation_rr(tr, n_end + 1, k, t)
    deg, deg1 = RW.degrees(tr, n_end), RW.degrees(tr, n_end + 1)
    up = RW.raised_index(tr, n_end, n_end + 1)
    assert np.abs(RR1[np.ix_(up, up)] - RR).max() <= 1e-13 * np.abs(RR).max()          # the entries do not depend on the order
    rn = np.linalg.norm(r, axis=-1)
    Y, Y1 = tr.harmonics(r / rn[:, None], n_end), tr.harmonics(r / rn[:, None], n_end + 1)
    J = np.stack([RW.regular_radial(n_end, d, k * ri) for ri in rn], axis=1)            # [n_end + 1, P]
    basis, basis1 = J[deg] * Y, J[deg1] * Y1
    top = deg1 == n_end
    worst = 0.0
    for hp in range(len(deg)):
        want = RW.regular_samples(tr, n_end, k, o, hp, c[None] + r)
        got = RR[hp] @ basis
        tail = np.abs(RR1[up[hp], top] @ basis1[top])
        scale = np.abs(want).max()
        err = np.abs(got - want)
        worst = max(worst, (err / scale).max())
        terms = np.abs(basis).sum(axis=0)
        assert (err <= 2 * tail + 1e-13 * terms).all(), (name, hp, (err / terms).max(), (tail / terms).max())
    print(f"{name} n_end {n_end} k {k}: addition theorem, worst error / max |u_in| {worst:.1e}")


@pytest.mark.parametrize("k", [1.3, 0.9 + 0.3j])
@pytest.mark.parametrize("name,n_end", CASES, ids=[c[0] for c in CASES])
def test_the_yardstick_at_zero_displacement_is_the_identity(name, n_end, k):
    """RR(0) = I: only l = 0 survives j_l(0), and C_d j_0(0) Y_0 int Y_h' conj(Y_h) = delta.  1e-13: the rounding of the quadrature."""
    tr = _tree(name)
    RR = RW.translation_rr(tr, n_end, k, np.zeros(tr.d))
    assert np.abs(RR - np.eye(len(RR))).max() <= 1e-13


def test_regular_radial_at_zero_and_against_the_oracle():
    for d in (2, 3, 4, 5):
        for z in (0.7, 1.9 + 0.4j, 1.9 - 0.4j):
            assert np.abs(RW.regular_radial(6, d, z) - O.radial_h(6, d, z)[0]).max() <= 1e-15
        small = RW.regular_radial(3, d, 1e-9)
        assert abs(small[0] - RW.regular_radial(3, d, 0.0)[0]) <= 1e-15 and np.abs(small[1:]).max() <= 1e-9


def test_the_cluster_sum_of_one_ball_at_the_origin_is_its_own_coefficients():
    """o = c_0, one ball: A = density x blc placed by label on the longer axis, zeros elsewhere."""
    tr = O.tree("ba")
    n_end, n_out, k = 3, 5, 1.1
    rng = np.random.default_rng(0)
    dens = rng.normal(size=(1, tr.n_harm(n_end))) + 1j * rng.normal(size=(1, tr.n_harm(n_end)))
    cen = np.array([[0.3, 0.1, -0.2]])
    A = RW.cluster_coefficients(tr, n_end, n_out, k, 1.0, cen, np.array([0.8]), cen[0], dens)
    idx = RW.raised_index(tr, n_end, n_out)
    want = np.zeros(tr.n_harm(n_out), dtype=np.complex128)
    want[idx] = dens[0] * RW.blc(tr, n_end, k, 1.0, 0.8)[tr.degrees(n_end)]
    assert np.abs(A - want).max() <= 1e-13 * np.abs(want).max()


def test_the_header_declares_the_new_entries():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "biem_mi355.h")).read()
    for name in ("biem_rhs_regular_wave_workspace_bytes", "biem_rhs_regular_wave", "biem_solve_rw", "biem_solve_ldlt_rw",
                 "biem_solve_factored_rw", "biem_cluster_coefficients_workspace_bytes", "biem_cluster_coefficients"):
        assert f" {name}(" in text, name
    from biem_helmholtz_sphere_amd import _lib

    assert all(name in _lib.SIGNATURES for name in ("biem_rhs_regular_wave", "biem_solve_factored_rw", "biem_cluster_coefficients"))


def test_argument_errors_need_no_device():
    """The pair is given together, excludes every other incidence argument, and its index is checked like the multipole one."""
    import biem_helmholtz_sphere_amd as amd
    from biem_helmholtz_sphere_amd._biem import _closed_form_request

    c = amd.create_from_branching_types("ba")
    k, o = np.array([1.3]), np.zeros((3, 1))
    with pytest.raises(ValueError, match="regular_wave_origin and regular_wave_index must be given together"):
        _closed_form_request(c, k, 4, None, None, None, None, None, None, o, None)
    with pytest.raises(ValueError, match="regular_wave_origin and regular_wave_index must be given together"):
        _closed_form_request(c, k, 4, None, None, None, None, None, None, None, 1)
    for other in (dict(plane_wave_direction=o), dict(point_source_position=o), dict(multipole_source_position=o, multipole_source_index=0),
                  dict(uin=lambda x: x)):
        args = dict(uin=None, uin_grad=None, plane_wave_direction=None, point_source_position=None, multipole_source_position=None,
                    multipole_source_index=None)
        args.update(other)
        with pytest.raises(ValueError, match="regular_wave_origin replaces"):
            _closed_form_request(c, k, 4, args["uin"], args["uin_grad"], args["plane_wave_direction"], args["point_source_position"],
                                 args["multipole_source_position"], args["multipole_source_index"], o, 1)
    with pytest.raises(ValueError, match=r"regular_wave_index must lie in \[0, H\) with H=16"):
        _closed_form_request(c, k, 4, None, None, None, None, None, None, o, 16)
    with pytest.raises(ValueError, match="regular_wave_index must be an integer"):
        _closed_form_request(c, k, 4, None, None, None, None, None, None, o, 1.5)
    with pytest.raises(ValueError, match="first dimension of regular_wave_origin"):
        _closed_form_request(c, k, 4, None, None, None, None, None, None, np.zeros((2, 1)), 1)
    name, (S, I), _ = _closed_form_request(c, k, 4, None, None, None, None, None, None, np.zeros((3, 5)), np.arange(5))
    assert name == "regular_wave_origin" and S.shape == (3, 5) and I.dtype == np.int32 and I.tolist() == [0, 1, 2, 3, 4]
