"""GPU tests of the gradient inside penetrable fluid balls: ``uinterior_grad`` / ``utotal_grad`` (``biem_u_interior_grad``,
``biem_u_total_grad``) and the C entry ``biem_uinterior_grad``.  Shapes, fluids and helpers are those of
``tests/test_gpu_interior_field.py``.

Yardsticks, each with its own tolerance:

* the 8th-order central difference of the NumPy interior sum ``_u_from_coef`` on the algebraic coefficients,
      f' ~ [4/5 (f1 - f-1) - 1/5 (f2 - f-2) + 4/105 (f3 - f-3) - 1/280 (f4 - f-4)] / h,
  at h = 5e-3, first held against h = 1e-2 within STENCIL_TOL = 1e-11 of max |grad u| (that guards the yardstick; the sum is analytic
  beyond the surface, so a stencil around the point at 0.999 rho may leave the ball); then |GPU - stencil| <= PARITY_TOL = 1e-10 of
  max |grad u|.  Both numbers are those of ``tests/test_gpu_field_gradient.py``;
* the radial derivative of the analytic one-sphere series from SciPy's Bessel functions: 1e-11 of max |grad u|;
* the transmission conditions at the surface of one sphere: 1e-10.

Every test prints the error it measured.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_interior_field as F  # noqa: E402  (geometry, fluids, yardstick, series, point sets)
from test_gpu_interior_field import amd  # noqa: E402,F401  (the module's fixture)
from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

_dev, _cdev, K, ETA = F._dev, F._cdev, F.K, F.ETA
C8 = (4.0 / 5.0, -1.0 / 5.0, 4.0 / 105.0, -1.0 / 280.0)
STENCIL_TOL, PARITY_TOL = 1e-11, 1e-10


def _central8(f, x, h):
    """8th-order central difference of f (x [P, d] -> [P]) along every axis: [d, P]."""
    P, d = x.shape
    g = np.zeros((d, P), dtype=np.complex128)
    for i in range(d):
        for j, c in enumerate(C8, start=1):
            step = np.zeros(d)
            step[i] = j * h
            g[i] += c * (f(x + step) - f(x - step))
    return g / h


def _case_points(cen, rad):
    """_interior_points (the centre and 0.999 rho among them) and, per ball, offsets along every coordinate axis through the centre
    (+0.6 rho, -0.45 rho): the poles of every node of every tree."""
    x, ball = F._interior_points(cen, rad)
    d = cen.shape[1]
    ax = [cen[b] + f * rad[b] * np.eye(d)[i] for b in range(len(rad)) for i in range(d) for f in (0.6, -0.45)]
    return np.concatenate([x, np.array(ax)]), np.concatenate([ball, np.repeat(np.arange(len(rad)), 2 * d)])


_YARDSTICK = {}


def _stencil_yardstick(tree, B, n_end, fluid, spread=1.0):
    """(x, ball, grad u [d, P], max |grad u|) of the interior sum on the yardstick's density: computed once per case, read-only."""
    key = (tree, B, n_end, fluid, spread)
    if key not in _YARDSTICK:
        tr, cen, rad = F._dn_systems(tree, B, n_end, spread)[:3]
        _, s = F._yardstick(tree, B, n_end, fluid, spread)
        kb, delta = F._fluid(fluid, B)
        a = F._alg_coef(tr, n_end, rad, s, kb, delta)
        x, ball = _case_points(cen, rad)
        f = lambda y: F._u_from_coef(tr, n_end, a, kb, cen, y, ball)
        g1, g2 = _central8(f, x, 1e-2), _central8(f, x, 5e-3)
        scale = np.abs(g2).max()
        dev = np.abs(g1 - g2).max() / scale
        print(f"yardstick {tree} B={B} n_end={n_end} {fluid}: stencils h=1e-2 / 5e-3 agree to {dev:.2e} of max |grad u| = {scale:.4f}")
        assert dev <= STENCIL_TOL, dev
        for v in (x, ball, g2):
            v.setflags(write=False)
        _YARDSTICK[key] = (x, ball, g2, scale)
    return _YARDSTICK[key]


# ---------------------------------------------------------------------------- 1. kernel arithmetic, the same density on both sides
@pytest.mark.parametrize("fluid", sorted(F.FLUIDS))
@pytest.mark.parametrize("tree,B,n_end", F.SHAPES)
def test_kernels_against_the_stencil_same_density(amd, tree, B, n_end, fluid):
    """The yardstick's density on both sides (no solve): only function evaluation and the sums differ.  bpa / bpbpa pin the axis
    permutation of the components; the axis offsets are poles of every node of every tree."""
    tr, cen, rad = F._dn_systems(tree, B, n_end)[:3]
    dens, _ = F._yardstick(tree, B, n_end, fluid)
    kb, delta = F._fluid(fluid, B)
    x, ball, ref, scale = _stencil_yardstick(tree, B, n_end, fluid)
    calc = F._calculator(amd, tree, n_end, cen, rad, dens)
    g = calc.uinterior_grad(_dev(x.T), k_interior=_cdev(kb), density_ratio=_dev(delta)).cpu().numpy()
    assert g.shape == ref.shape == (tr.d, len(x))
    err = np.abs(g - ref).max() / scale
    print(f"{tree} B={B} n_end={n_end} {fluid}: {err:.2e} of max |grad u| = {scale:.4f}")
    assert err <= PARITY_TOL


# ---------------------------------------------------------------------------- 2. one sphere against SciPy
def _series_grad(kb, delta, x):
    """Full gradient of the analytic one-sphere series (analytic beyond the surface): only for scales and first-order corrections."""
    return _central8(lambda y: F._series_3d(kb, delta, F._C0[:3], 1.0, y), x, 5e-3)


@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("tree", ["ba", "bpa"])
def test_radial_derivative_of_one_sphere_against_the_analytic_series(amd, tree, case):
    """e . uinterior_grad against d/dr of the SciPy series (independent of oracle and tree), at the points of the value test but the
    centre, where e is undefined."""
    kb, delta = F.SINGLE[case]
    calc = F._solve(amd, tree, 1, 16, kb, delta)
    c = F._C0[:3]
    x = F._single_points(3)
    x = x[np.linalg.norm(x - c, axis=1) > 0]
    assert len(x) == 15
    e = (x - c) / np.linalg.norm(x - c, axis=1, keepdims=True)
    ref = F._series_3d(kb, delta, c, 1.0, x, radial_derivative=True)
    scale = np.linalg.norm(_series_grad(kb, delta, x), axis=0).max()
    g = calc.uinterior_grad(_dev(x.T), k_interior=_cdev([kb]), density_ratio=_dev([delta])).cpu().numpy()
    err = np.abs(np.sum(e.T * g, axis=0) - ref).max() / scale
    print(f"{tree} k_b={kb} delta={delta}: {err:.2e} of max |grad u| = {scale:.4f}")
    assert err <= 1e-11


# ---------------------------------------------------------------------------- 3. transmission across the surface
@pytest.mark.parametrize("case", range(3))
def test_transmission_across_the_surface(amd, case):
    """At rho (1 -+ eps) n, eps = 1e-13 (each point about 450 ulps from the surface: both masks are decided safely), 8 directions:

        |n . grad u_int - delta n . (grad u_in + grad u_scat)| <= 1e-10 max |d_r u_int|          (the normal component jumps by delta)
        |tangential part of grad u_int - tangential part of the exterior gradient| <= 1e-10 max |grad u_ext|

    Both scales come from the SciPy series at the surface, not from the device (d_r u_ext = d_r u_int / delta, the tangential parts
    agree).  The analytic solution itself varies over 2 eps rho: to first order the normal residual is -eps rho (d_rr u_int +
    delta d_rr u_ext), with d_rr u_int by differencing the series' radial derivative and d_rr u_ext from it through the Helmholtz
    equation on both sides (the surface Laplacian of u is continuous):
        d_rr u_ext = -k^2 u - (2 / rho) d_r u_int / delta + (k_b^2 u + d_rr u_int + (2 / rho) d_r u_int).
    Where that first-order value is not below a tenth of the tolerance it is subtracted (as test_continuity_across_the_surface
    does); the bound stays.  The tangential parts change by about eps rho |k_b| |grad u| <= 1e-12 of their size: far below a tenth.
    Also: utotal_grad is the exterior sum at the outer points and uinterior_grad at the inner ones, bit for bit."""
    kb, delta = F.SINGLE[case]
    calc = F._solve(amd, "ba", 1, 16, kb, delta)
    _, ugr = amd.plane_wave(k=_dev(K), direction=_dev(F._DIRECTION[:3]))
    rng = np.random.default_rng(13)
    n = rng.normal(size=(8, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    eps, rho, c = 1e-13, 1.0, F._C0[:3]
    kw = dict(k_interior=_cdev([kb]), density_ratio=_dev([delta]))
    xi, xo = _dev((c + rho * (1 - eps) * n).T), _dev((c + rho * (1 + eps) * n).T)
    gi = calc.uinterior_grad(xi, **kw).cpu().numpy()
    go = (ugr(xo) + calc.uscat_grad(xo)).cpu().numpy()
    assert np.isfinite(gi).all() and np.isfinite(go).all()            # neither side is masked
    assert np.array_equal(calc.utotal_grad(xo, uin_grad=ugr, **kw).cpu().numpy(), go)
    assert np.array_equal(calc.utotal_grad(xi, uin_grad=ugr, **kw).cpu().numpy(), gi)
    # the series at the surface: scales and the first-order variation
    xs = c + rho * n
    u = F._series_3d(kb, delta, c, rho, xs)
    dr = F._series_3d(kb, delta, c, rho, xs, radial_derivative=True)
    hh = 1e-4
    drr = (F._series_3d(kb, delta, c, rho, c + rho * (1 + hh) * n, radial_derivative=True)
           - F._series_3d(kb, delta, c, rho, c + rho * (1 - hh) * n, radial_derivative=True)) / (2 * hh * rho)
    drr_ext = -K ** 2 * u - (2 / rho) * dr / delta + (kb ** 2 * u + drr + (2 / rho) * dr)
    first = -eps * rho * (drr + delta * drr_ext)
    gs = _series_grad(kb, delta, xs)
    tan_s = gs - n.T * np.sum(n.T * gs, axis=0)
    scale_n = np.abs(dr).max()
    scale_ext = np.sqrt(np.abs(dr / delta) ** 2 + np.sum(np.abs(tan_s) ** 2, axis=0)).max()
    ni, no = np.sum(n.T * gi, axis=0), np.sum(n.T * go, axis=0)
    res = ni - delta * no
    tol_n = 1e-10 * scale_n
    subtract = np.abs(first).max() > 0.1 * tol_n
    err_n = np.abs(res - (first if subtract else 0.0)).max()
    err_t = np.abs((gi - n.T * ni) - (go - n.T * no)).max()
    print(f"k_b={kb} delta={delta}: normal {err_n / scale_n:.2e} of max |d_r u_int| = {scale_n:.4f} (first-order variation "
          f"{np.abs(first).max() / scale_n:.2e}, {'subtracted' if subtract else 'below a tenth of the bound, not subtracted'}); "
          f"tangential {err_t / scale_ext:.2e} of max |grad u_ext| = {scale_ext:.4f}")
    assert err_n <= tol_n
    assert err_t <= 1e-10 * scale_ext


# ---------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("fluid", sorted(F.FLUIDS))
@pytest.mark.parametrize("tree,B,n_end,spread", [("ba", 3, 7, 1.3), ("a", 3, 8, 1.0)])
def test_end_to_end_against_the_stencil(amd, tree, B, n_end, spread, fluid):
    """biem(alpha_n=, beta_n=) then uinterior_grad, against the stencil on the yardstick's density."""
    kb, delta = F._fluid(fluid, B)
    x, ball, ref, scale = _stencil_yardstick(tree, B, n_end, fluid, spread)
    calc = F._solve(amd, tree, B, n_end, kb, delta, spread)
    g = calc.uinterior_grad(_dev(x.T), k_interior=_cdev(kb), density_ratio=_dev(delta)).cpu().numpy()
    err = np.abs(g - ref).max() / scale
    print(f"{tree} B={B} n_end={n_end} {fluid}: {err:.2e} of max |grad u| = {scale:.4f}")
    assert err <= 1e-10


# ---------------------------------------------------------------------------- 5. semantics
def test_semantics_of_the_mask_and_of_utotal_grad(amd):
    tree, B, n_end = "ba", 2, 6
    cen, rad = F._geometry(3, B)
    kb, delta = F._fluid("two_fluids", B)
    calc = F._solve(amd, tree, B, n_end, kb, delta)
    _, ugr = amd.plane_wave(k=_dev(K), direction=_dev(F._DIRECTION[:3]))
    x, ball = F._semantic_points(cen, rad)
    xd = _dev(x.T)
    kw = dict(k_interior=_cdev(kb), density_ratio=_dev(delta))
    ui = calc.uinterior(xd, **kw).cpu().numpy()
    gi = calc.uinterior_grad(xd, **kw).cpu().numpy()
    assert gi.shape == (3, 300)
    assert (np.isnan(gi) == np.isnan(ui)[None]).all() and (np.isnan(ui) == (ball < 0)).all()      # NaN in all components exactly there
    assert np.isfinite(gi[:, ball >= 0]).all()
    perm = np.random.default_rng(1).permutation(300)              # the same values in any point order
    gp = calc.uinterior_grad(_dev(x[perm].T), **kw).cpu().numpy()
    assert np.array_equal(gp, gi[:, perm], equal_nan=True)
    gt = calc.utotal_grad(xd, uin_grad=ugr, **kw).cpu().numpy()
    ge = (ugr(xd) + calc.uscat_grad(xd)).cpu().numpy()
    assert np.isfinite(gt).all()
    assert np.array_equal(gt[:, ball < 0], ge[:, ball < 0]) and np.array_equal(gt[:, ball >= 0], gi[:, ball >= 0])
    # an impenetrable ball: NaN inside it, the other ball bit-identical
    kn = kb.copy()
    kn[1] = np.nan
    gn = calc.uinterior_grad(xd, k_interior=_cdev(kn), density_ratio=_dev(delta)).cpu().numpy()
    assert np.isnan(gn[:, ball == 1]).all() and np.array_equal(gn[:, ball == 0], gi[:, ball == 0]) and np.isnan(gn[:, ball < 0]).all()
    gtn = calc.utotal_grad(xd, k_interior=_cdev(kn), density_ratio=_dev(delta), uin_grad=ugr).cpu().numpy()
    assert np.isnan(gtn).sum() == (ball == 1).sum() * 3
    # the sound-soft limit
    g0 = calc.uinterior_grad(xd, k_interior=_cdev(kb), density_ratio=_dev([0.0, 0.0])).cpu().numpy()
    assert (g0[:, ball >= 0] == 0).all() and np.isnan(g0[:, ball < 0]).all()
    print(f"300 points: {int((ball == 0).sum())} in ball 0, {int((ball == 1).sum())} in ball 1, {int((ball < 0).sum())} outside; "
          f"max |grad u_interior| {np.nanmax(np.abs(gi)):.3f}")


def test_transparent_pair_is_nan_inside_and_no_error(amd):
    tree, B, n_end = "ba", 2, 6
    cen, rad = F._geometry(3, B)
    calc = F._solve(amd, tree, B, n_end, K, 1.0)
    x, ball = F._interior_points(cen, rad)
    g = calc.uinterior_grad(_dev(x.T), k_interior=_cdev([K, K]), density_ratio=_dev([1.0, 1.0])).cpu().numpy()
    print(f"transparent pair: {int(np.isnan(g).sum())} of {g.size} components NaN")
    assert np.isnan(g).all()


# ---------------------------------------------------------------------------- 6. batches and namespaces
def test_batches_and_numpy_namespace(amd):
    """3 wavenumbers, k_interior of shape (3, B), per-system points with expand_x=False, NumPy in and out: each slice equals the
    unbatched call on the same density to 1e-13."""
    tree, B, n_end = "ba", 2, 6
    c = amd.create_from_branching_types(tree)
    cen, rad = F._geometry(3, B)
    ks = np.array([0.9, 1.3, 2.2])
    kb = np.array([[2.1, 0.9 + 0.1j], [1.5, 2.4], [3.0 + 0.2j, 0.7]])
    delta = np.array([0.5, 3.0])
    rng = np.random.default_rng(2)
    P = 9
    u = rng.normal(size=(3, P, 3))
    u /= np.linalg.norm(u, axis=0, keepdims=True)
    bsel = rng.integers(0, B, P)
    x = cen[bsel].T[:, :, None] + (rad[bsel][:, None] * rng.uniform(0.05, 0.95, (P, 3)))[None] * u      # (d, P, 3): other points per system
    an, bn = amd.fluid_inclusion_bc(c_ndim=3, n_end=n_end, radii=rad, k_interior=kb, density_ratio=delta)
    dirs = np.repeat(F._DIRECTION[:3, None], 3, 1)
    uin, ugr = amd.plane_wave(k=ks, direction=dirs)
    calc = amd.biem(c, centers=cen[None], radii=rad[None], k=ks, eta=np.full(3, ETA), n_end=n_end, alpha_n=an, beta_n=bn, uin=uin, uin_grad=ugr)
    got = calc.uinterior_grad(x, k_interior=kb, density_ratio=delta, expand_x=False)
    tot = calc.utotal_grad(x, k_interior=kb, density_ratio=delta, uin_grad=ugr, expand_x=False)
    assert isinstance(got, np.ndarray) and got.shape == (3, P, 3) and got.dtype == np.complex128
    assert np.isfinite(got).all() and np.array_equal(tot, got)
    for s in range(3):
        one = amd.BIEMResultCalculator(c=c, centers=calc.centers[:, 0], radii=calc.radii[0], k=np.asarray(calc.k[s]), n_end=n_end,
                                       eta=np.asarray(calc.eta[s]), kind="outer", density=calc.density[s])
        ref = one.uinterior_grad(x[:, :, s], k_interior=kb[s], density_ratio=delta)
        assert ref.shape == (3, P)
        err = np.max(np.abs(got[:, :, s] - ref)) / np.max(np.abs(ref))
        print(f"system {s}: {err:.2e}")
        assert err <= 1e-13


# ---------------------------------------------------------------------------- 7. the C entry's argument checks
def test_c_entry_rejects_other_flags_and_uncovered_plans(amd):
    from biem_helmholtz_sphere_amd import _biem, _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())

    def operands(d, H, P):
        ops = dict(k=_cdev([K]), eta=_dev([ETA]), cen=_dev(np.zeros((1, d))), rad=_dev([1.0]), kb=_cdev([2.1]), dl=_cdev([0.5]),
                   dens=_cdev(np.ones((1, H))), pts=_dev(np.zeros((d, P))),
                   out=torch.full((d, P, 1), 7.0, dtype=torch.complex128, device="cuda"),
                   val=torch.zeros((P, 1), dtype=torch.complex128, device="cuda"),
                   work=torch.zeros(H * 16, dtype=torch.uint8, device="cuda"))
        return ops, {n: t.data_ptr() for n, t in ops.items()}

    B, H, P = 1, 16, 3
    ops, p = operands(3, H, P)

    def call(fn, handle, flags, p, H, out="out"):
        return fn(handle, 1, B, P, p["k"], p["eta"], p["cen"], p["rad"], 0, p["kb"], p["dl"], 0, p["dens"], p["pts"], flags,
                  p[out], p["work"], B * H * 16, None)
    plan = _biem._plan("ba", 4, dev)
    for flags in (L.USCAT_FAR_FIELD, L.USCAT_PER_BALL, L.USCAT_KIND_INNER, L.USCAT_PER_BALL | L.USCAT_POINTS_BATCHED, 16):
        assert call(lib.biem_uinterior_grad, plan.handle, flags, p, H) == 1                           # BIEM_ERR_ARG
        msg = lib.biem_last_error()
        assert b"BIEM_USCAT_POINTS_BATCHED" in msg and b"biem_uinterior_grad" in msg
    assert call(lib.biem_uinterior_grad, plan.handle, 0, p, H) == L.BIEM_OK
    torch.cuda.synchronize()
    assert np.isfinite(ops["out"].cpu().numpy()).all()                                  # (three times the centre of the ball)
    chain = _biem._plan("bbba", 2, dev)
    assert call(lib.biem_uinterior_grad, chain.handle, 0, p, H) == L.BIEM_ERR_UNSUPPORTED and b"chain" in lib.biem_last_error()
    wide = _biem._plan("a", 200, dev)                                                   # below the order ceiling, above the LDS of 64 rows
    assert call(lib.biem_uinterior_grad, wide.handle, 0, p, H) == L.BIEM_ERR_UNSUPPORTED and b"LDS" in lib.biem_last_error()
    # the last order whose 64 rows of n_end + 3 radial values fit: accepted, every component written, NaN exactly where the value is
    H = 2 * 152 - 1
    ops, p = operands(2, H, P)
    edge = _biem._plan("a", 152, dev)
    assert call(lib.biem_uinterior_grad, edge.handle, 0, p, H) == L.BIEM_OK
    assert call(lib.biem_uinterior, edge.handle, 0, p, H, out="val") == L.BIEM_OK
    torch.cuda.synchronize()
    g, v = ops["out"].cpu().numpy()[:, :, 0], ops["val"].cpu().numpy()[:, 0]
    print(f"tree a, n_end 152, centre: grad u = {g[:, 0]}, u = {v[0]}")
    assert not (g == 7.0).any() and (np.isnan(g) == np.isnan(v)[None]).all()
    assert np.array_equal(g[:, 0], g[:, 1], equal_nan=True) and np.array_equal(g[:, 0], g[:, 2], equal_nan=True)
    over = _biem._plan("a", 153, dev)
    assert call(lib.biem_uinterior_grad, over.handle, 0, p, H) == L.BIEM_ERR_UNSUPPORTED and b"LDS" in lib.biem_last_error()
