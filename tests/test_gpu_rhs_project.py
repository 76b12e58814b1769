"""GPU tests of the projection of boundary samples on their own: ``biem_rhs_project`` and ``biem_rhs_project_n`` against NumPy.

    one set:   f = g @ W
    two sets:  f = -(alpha_n[deg] * (gu @ W) + beta_n[deg] * (gdn @ W))       (a null set is zero)

W [Q][H] comes from ``biem_plan_projection`` and deg from ``biem_plan_labels``; rows of g are (system, right-hand side, ball),
f goes to ``d_f[s sys_stride + (b H + h) elem_stride + r rhs_stride]``.

The bound is componentwise and derived.  With S = sum_q |g_q| |W_q| = (|g| @ |W|) and the unit roundoff u = eps / 2: each component of
a sum of Q complex products is a chain of 2 Q real multiply-adds (fused on the device: one rounding each; the few-rows form cuts the
chain in 16 and adds the pieces, which is shorter), whose terms sum to at most S in modulus, so a component is off by at most
gamma_{2Q} S = Q eps S (1 + O(Q eps)) and the complex value by sqrt2 times that.  NumPy's own product, in whatever order, with
separate multiplications, stays inside sqrt2 (Q + 1) eps S.  Together 2 sqrt2 (Q + 1/2) eps S < 4 (Q + 2) eps S.  The two-set epilogue
multiplies each sum by a coefficient and adds (under 2 eps per sum, relative to |coefficient| S, on either side), which the margin
4 (Q + 2) - 2 sqrt2 (Q + 1/2) > 7 covers once |alpha_n| and |beta_n| are applied to the two bounds.  Nothing here is tuned to what
the kernels give.

Shapes: the smallest that reach each branch.  Tree ``ba`` has Q = 2 n_end^2 and H = n_end^2: n_end = 12 is the smallest order with
Q = 288 > 256 (two chunks of quadrature points, the second ragged), but its H = 144 is nine whole blocks of 16 harmonics, so n_end = 13
(H = 169, Q = 338) runs beside it for the ragged last block of the few-rows form.  H <= 256 either way: one block of harmonics in the
full form, ragged.  105 rows take the few-rows form, 1050 rows the full form for one set (from 1017 rows on) and for two (from 509
on); both counts leave the last row block ragged at 8 and at 4 rows per block.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SENTINEL = complex(-7.5, 1234.0)
FORMS = {"few": (5, 7, 3), "full": (35, 6, 5)}            # nb, nrhs, B
ORDERS = [12, 13]                                         # n_end of the plan


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from biem_helmholtz_sphere_amd import _lib as L

    return L


def _cdev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(torch.complex128).contiguous()


@lru_cache(maxsize=None)
def _plan(tree, n_end):
    """(handle, H, Q, W [Q][H], deg [H]) of a plan on the current device, from the C entries"""
    from biem_helmholtz_sphere_amd import _biem, _lib as L

    lib = L.load()
    plan = _biem._plan(tree, n_end, torch.device("cuda", torch.cuda.current_device()))
    H, Q = C.c_int(), C.c_int()
    L.check(lib.biem_plan_info(plan.handle, None, C.byref(H), C.byref(Q), None, None))
    H, Q = H.value, Q.value
    W = np.zeros((Q, H), dtype=np.complex128)
    L.check(lib.biem_plan_projection(plan.handle, W.ctypes.data))
    lab, deg = np.zeros((H, 3), dtype=np.int32), np.zeros(H, dtype=np.int32)
    L.check(lib.biem_plan_labels(plan.handle, lab.ctypes.data, deg.ctypes.data))
    return plan.handle, H, Q, W, deg


@lru_cache(maxsize=None)
def _case(form, n_end):
    """Inputs of a form and their NumPy projections, computed once: samples, coefficients, P = g @ W and |g| @ |W| per set"""
    nb, nrhs, B = FORMS[form]
    handle, H, Q, W, deg = _plan("ba", n_end)
    assert 256 < Q < 512 and H <= 256 and (H % 16 != 0 or n_end == 12)
    rng = np.random.default_rng(17 + nb + n_end)
    cplx = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    g = [cplx(nb, nrhs, B, Q), cplx(nb, nrhs, B, Q)]
    coef = {ab: (cplx(nb if ab else 1, B, n_end), cplx(nb if ab else 1, B, n_end)) for ab in (0, 1)}
    P = [x @ W for x in g]
    bound = [np.abs(x) @ np.abs(W) for x in g]
    dev = {"g": [_cdev(x) for x in g], "coef": {ab: tuple(_cdev(c) for c in coef[ab]) for ab in (0, 1)}}
    return handle, H, Q, deg, g, coef, P, bound, dev


def _layout(nb, nrhs, B, H, strided):
    """strides (in complex numbers) and the flat index of every (s, r, b, h)"""
    rhs_stride = 2 if strided else 1
    elem_stride = 2 * nrhs + 3 if strided else nrhs
    sys_stride = B * H * elem_stride + (5 if strided else 0)
    s, r, b, h = np.meshgrid(np.arange(nb), np.arange(nrhs), np.arange(B), np.arange(H), indexing="ij")
    return sys_stride, elem_stride, rhs_stride, s * sys_stride + (b * H + h) * elem_stride + r * rhs_stride


def _compare(out, idx, want, bound, Q, what):
    got = out[idx]
    err = np.abs(got - want)
    lim = 4 * (Q + 2) * EPS * bound
    print(f"{what}: largest error / bound {np.max(err / lim):.3f}")
    assert np.all(err <= lim), f"{what}: {int((err > lim).sum())} entries outside 4 (Q + 2) eps (|g| @ |W|), worst ratio {np.max(err / lim):.3g}"
    gaps = np.ones(out.shape, dtype=bool)
    gaps[idx.ravel()] = False
    assert np.all(out[gaps] == SENTINEL), f"{what}: wrote between the entries of f"


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("n_end", ORDERS)
@pytest.mark.parametrize("form", list(FORMS))
def test_one_set_is_g_times_w(L, form, n_end, strided):
    nb, nrhs, B = FORMS[form]
    handle, H, Q, deg, g, coef, P, bound, dev = _case(form, n_end)
    sys_stride, elem_stride, rhs_stride, idx = _layout(nb, nrhs, B, H, strided)
    f = torch.full((nb * sys_stride,), SENTINEL, dtype=torch.complex128, device="cuda")
    L.check(L.load().biem_rhs_project(handle, nb, B, nrhs, dev["g"][0].data_ptr(), f.data_ptr(), sys_stride, elem_stride, rhs_stride, None))
    torch.cuda.synchronize()
    _compare(f.cpu().numpy(), idx, P[0], bound[0], Q, f"one set, {form}, n_end={n_end}")


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("ab_batched", [0, 1])
@pytest.mark.parametrize("sets", ["both", "gu_null", "gdn_null"])
@pytest.mark.parametrize("n_end", ORDERS)
@pytest.mark.parametrize("form", list(FORMS))
def test_two_sets_are_mixed_per_degree(L, form, n_end, sets, ab_batched, strided):
    nb, nrhs, B = FORMS[form]
    handle, H, Q, deg, g, coef, P, bound, dev = _case(form, n_end)
    sys_stride, elem_stride, rhs_stride, idx = _layout(nb, nrhs, B, H, strided)
    use = (sets != "gu_null", sets != "gdn_null")
    # coefficients [nb or 1][B][n_end] -> [nb or 1][1][B][H] of the rows' balls and the harmonics' degrees
    al, be = (c[:, None, :, :][..., deg] for c in coef[ab_batched])
    want = -(al * P[0] * use[0] + be * P[1] * use[1])
    lim = np.abs(al) * bound[0] * use[0] + np.abs(be) * bound[1] * use[1]
    al_d, be_d = dev["coef"][ab_batched]
    f = torch.full((nb * sys_stride,), SENTINEL, dtype=torch.complex128, device="cuda")
    L.check(L.load().biem_rhs_project_n(handle, nb, B, nrhs, dev["g"][0].data_ptr() if use[0] else None,
                                        dev["g"][1].data_ptr() if use[1] else None, al_d.data_ptr(), be_d.data_ptr(), ab_batched,
                                        f.data_ptr(), sys_stride, elem_stride, rhs_stride, None))
    torch.cuda.synchronize()
    _compare(f.cpu().numpy(), idx, want, lim, Q, f"two sets ({sets}), {form}, n_end={n_end}, ab_batched={ab_batched}")


def test_more_row_blocks_than_a_grid_dimension_of_65535(L):
    """524296 rows, 65537 row blocks of 8, at H = 1 (tree a, n_end = 1): the full form of one set on a flat grid."""
    nb, nrhs, B = 1, 8, 65537
    handle, H, Q, W, deg = _plan("a", 1)
    assert H == 1 and nb * nrhs * B == 8 * 65535 + 16 and nb * nrhs * B * Q * 16 < 64 << 20
    rng = np.random.default_rng(5)
    g = rng.normal(size=(nb, nrhs, B, Q)) + 1j * rng.normal(size=(nb, nrhs, B, Q))
    sys_stride, elem_stride, rhs_stride, idx = _layout(nb, nrhs, B, H, False)
    g_d = _cdev(g)
    f = torch.full((nb * sys_stride,), SENTINEL, dtype=torch.complex128, device="cuda")
    L.check(L.load().biem_rhs_project(handle, nb, B, nrhs, g_d.data_ptr(), f.data_ptr(), sys_stride, elem_stride, rhs_stride, None))
    torch.cuda.synchronize()
    _compare(f.cpu().numpy(), idx, g @ W, np.abs(g) @ np.abs(W), Q, "one set, 524296 rows")
