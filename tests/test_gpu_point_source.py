"""GPU tests of point-source incidence in closed form: ``biem_rhs_point_source`` against tests/point_source_yardstick.py, sources on the
tree's axes, the chain tree bbba against the projection of the sampled field at a higher order, ``biem(point_source_position=)`` /
``BIEMFactorization.solve(point_source_position=)`` end to end on every solve path against ``numpy.linalg.solve`` of the oracle's matrix
with the yardstick's right-hand side, reciprocity of the device's solutions, and the result record.  tests/test_point_source_host.py
pins the yardstick.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

import point_source_yardstick as PS  # noqa: E402
from test_point_source_host import CHAIN_TOLERANCE  # noqa: E402

ETA = 1.0
ROBIN = (1.0 + 0.5j, 0.3 - 0.2j)
FLUID = ((2.1, 0.9 + 0.1j, 1.4), (0.5, 3.0, 1.5))     # k_interior, density ratio per ball
KS = (1.3, 0.9 + 0.3j)
RADII = np.array([1.0, 0.7, 0.85])


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), device="cuda").to(dtype).contiguous()


def tc(a):
    return t(a, torch.complex128)


def ptr(x):
    return int(x.data_ptr())


def geometry(B, d, flat=False):
    """B separated balls off every axis (flat: all in the plane of zero last coordinate)."""
    cen = np.zeros((B, d))
    i = np.arange(B)
    cen[:, 0] = 2.6 * i + 0.1
    cen[:, 1] = 0.3 * i * i - 0.2
    for j in range(2, d):
        cen[:, j] = 0.0 if (flat and j == d - 1) else 0.15 * (j + i % 2)
    return cen, np.resize(RADII, B)


def sources(geometries, n, seed=0):
    """[n, d]: source i lies 0.4 .. 1.5 radii off the surface of ball i % B along a direction with every component non-zero, and at
    least 0.4 radii off every other surface - in every one of `geometries`, a list of (centers, radii)."""
    rng = np.random.default_rng(seed)
    cen0, rad0 = geometries[0]
    B, d = cen0.shape
    out = []
    while len(out) < n:
        b = len(out) % B
        v = rng.normal(size=d)
        v = v + 0.3 * np.sign(v)
        s = cen0[b] + rad0[b] * (1.0 + rng.uniform(0.4, 1.5)) * v / np.linalg.norm(v)
        if all((np.linalg.norm(s[None] - cen, axis=-1) >= 1.4 * rad).all() for cen, rad in geometries):
            out.append(s)
    return np.stack(out)


def fluid_pair(amd, d, n_end, rad, ks):
    """fluid_inclusion_bc per system: [len(ks), B, n_end] NumPy arrays."""
    B = len(rad)
    an, bn = amd.fluid_inclusion_bc(c_ndim=d, n_end=n_end, radii=t(rad), k_interior=tc(FLUID[0][:B]), density_ratio=t(FLUID[1][:B]),
                                    k=tc(np.asarray(ks)))
    return an.cpu().numpy(), bn.cpu().numpy()


# ---------------------------------------------------------------------------- 1. the kernel against the yardstick
def _tables(amd, plan, nb, B, k, rad, alpha, beta, per_degree):
    lib = amd._biem.L.load()
    tab = torch.empty((nb, B, 3, plan.n_end), dtype=torch.complex128, device="cuda")
    fn = lib.biem_ball_tables_n if per_degree else lib.biem_ball_tables
    amd._biem.L.check(fn(plan.handle, nb, B, ptr(k), ptr(t(np.ones(nb))), ptr(rad), 0, ptr(alpha), ptr(beta), int(alpha.shape[0] == nb and nb > 1),
                         ptr(tab), 0), "biem_ball_tables")
    return tab


def _rhs_point_source(amd, plan, nb, B, nrhs, k, cen, tab, src, batched, layout):
    """biem_rhs_point_source into the natural layout [nb, nrhs, B H] or the solve layout [nb, B H, ld] (ld: nrhs rounded up to 8); returns
    f[nb, nrhs, B H].  The solve layout is preset with a sentinel: the columns nrhs .. ld - 1 must keep it."""
    lib, H = amd._biem.L.load(), plan.H
    wb = int(lib.biem_rhs_point_source_workspace_bytes(plan.handle, nb, B, nrhs, batched, 0))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    if layout == "natural":
        f = torch.full((nb, nrhs, B * H), 7.0, dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)
    else:
        ld = (nrhs + 7) // 8 * 8
        f = torch.full((nb, B * H, ld), 7.0, dtype=torch.complex128, device="cuda")
        strides = (B * H * ld, ld, 1)
    amd._biem.L.check(lib.biem_rhs_point_source(plan.handle, nb, B, nrhs, ptr(k), ptr(cen), 0, ptr(tab), ptr(src), batched, ptr(f), *strides,
                                                ptr(work), wb, 0), "biem_rhs_point_source")
    torch.cuda.synchronize()
    f = f.cpu().numpy()
    if layout == "natural":
        return f
    assert (f[:, :, nrhs:] == 7.0).all()
    return f[:, :, :nrhs].transpose(0, 2, 1)


def _kernel_case(amd, tree, coef, batched, nrhs_list=(1, 5), n_end=None):
    from biem_helmholtz_sphere_amd._coords import canonical_tree

    n_end = n_end or {"a": 8, "ba": 6, "bpa": 6, "bba": 4, "caa": 4}[tree]
    tr = O.tree(tree)
    d, B, nb = tr.d, 2, 2
    canon, perm = canonical_tree(tree)
    perm = list(perm)
    plan = amd._biem._plan(canon, n_end, torch.device("cuda", torch.cuda.current_device()))
    cen, rad = geometry(B, d)
    if coef == "fluid":
        an, bn = fluid_pair(amd, d, n_end, rad, KS)                  # [nb, B, n_end]
        pairs = [(an[s], bn[s]) for s in range(nb)]
        al, be = tc(an), tc(bn)
    else:
        pairs = [ROBIN] * nb
        al, be = tc(np.full((1, B), ROBIN[0])), tc(np.full((1, B), ROBIN[1]))
    k = tc(KS)
    tab = _tables(amd, plan, nb, B, k, t(rad), al, be, coef == "fluid")
    worst = 0.0
    for nrhs in nrhs_list:
        S = (sources([(cen, rad)], nb * nrhs, seed=nrhs).reshape(nb, nrhs, d) if batched
             else np.broadcast_to(sources([(cen, rad)], nrhs, seed=nrhs), (nb, nrhs, d)))
        src = t(S[..., perm] if batched else S[0][:, perm])
        want = np.stack([np.stack([PS.rhs(tr, n_end, KS[s], cen, rad, *pairs[s], S[s, r]).reshape(-1) for r in range(nrhs)]) for s in range(nb)])
        for layout in ("natural", "solve"):
            got = _rhs_point_source(amd, plan, nb, B, nrhs, k, t(cen[:, perm]), tab, src, int(batched), layout)
            err = max(np.abs(got[s] - want[s]).max() / np.abs(want[s]).max() for s in range(nb))
            worst = max(worst, err)
            assert err <= 1e-12, (tree, coef, batched, nrhs, layout, err)
    print(f"{tree} {coef} {'batched' if batched else 'shared'} sources: worst error / max |f| {worst:.1e}")


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("coef", ["robin", "fluid"])
@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "caa"])
def test_rhs_point_source_against_the_yardstick(amd, tree, coef, batched):
    """Two systems (k = 1.3 and 0.9 + 0.3i), two balls, nrhs = 1 and 5, both write layouts: 1e-12 of max |f| per system."""
    _kernel_case(amd, tree, coef, batched)


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
def test_rhs_point_source_with_the_right_hand_sides_along_the_lanes(amd, batched):
    """nrhs = 70 in the solve layout (more than a wave of contiguous right-hand sides: the form with r along the lanes) and in the natural one."""
    _kernel_case(amd, "ba", "robin", batched, nrhs_list=(70,), n_end=9)


# ---------------------------------------------------------------------------- 2. sources on the tree's axes
@pytest.mark.parametrize("tree", ["ba", "bba"])
def test_sources_on_the_tree_s_axes(amd, tree):
    """t = s - c parallel to the first and to the last coordinate axis and in the plane of zero last coordinate, where the angles of the
    tree are degenerate.  One ball, alpha = 1, beta = 0, rho / |t| = 0.05, n_end 12: -sum_h f_h Y_h(y_q) at the plan's quadrature points is
    h_0(k |c + rho y_q - s|) to 1e-11 of its maximum (the truncation is 0.05^12); where the oracle's harmonics are finite at t^ the
    yardstick is compared too, to 1e-12 of max |f|."""
    n_end, rho, dist = 12, 0.1, 2.0
    tr = O.tree(tree)
    d = tr.d
    plan = amd._biem._plan(tree, n_end, torch.device("cuda", torch.cuda.current_device()))
    cen = (0.3 + 0.25 * np.arange(d))[None]
    rad = np.array([rho])
    first, last, flat = np.zeros(d), np.zeros(d), np.zeros(d)
    first[0], last[-1], flat[:-1] = 1.0, 1.0, np.array([0.6, -0.5, 0.4])[:d - 1]
    units = np.stack([first, -first, last, -last, flat / np.linalg.norm(flat)])
    S = cen + dist * units
    nb, nrhs = len(KS), len(S)
    k = tc(KS)
    tab = _tables(amd, plan, nb, 1, k, t(rad), tc([[1.0]]), tc([[0.0]]), False)
    y = plan.quad_y.cpu().numpy()                                          # [Q, d]
    Y = tr.harmonics(y, n_end)                                             # [H, Q]
    assert np.isfinite(Y).all()
    for layout in ("natural", "solve"):
        f = _rhs_point_source(amd, plan, nb, 1, nrhs, k, t(cen), tab, t(S), 0, layout)       # [nb, nrhs, H]
        assert np.isfinite(f).all()
        for s in range(nb):
            for r in range(nrhs):
                want = O.point_source(KS[s], S[r], 0)[0](cen + rho * y)
                err = np.abs(-f[s, r] @ Y - want).max() / np.abs(want).max()
                note = ""
                with np.errstate(all="ignore"):
                    ref = PS.rhs(tr, n_end, KS[s], cen, rad, 1.0, 0.0, S[r]).reshape(-1)
                if np.isfinite(ref).all():
                    e2 = np.abs(f[s, r] - ref).max() / np.abs(ref).max()
                    note = f", against the yardstick {e2:.1e}"
                    assert e2 <= 1e-12, (tree, layout, s, r, e2)
                print(f"{tree} {layout} k {KS[s]} t^ {units[r]}: resynthesised field {err:.1e}{note}")
                assert err <= 1e-11, (tree, layout, s, r, err)


# ---------------------------------------------------------------------------- 3. a chain tree
def _h0_and_derivative_in_five_dimensions(z):
    """h_0 of d = 5 and its derivative in elementary functions: h_0^(5)(z) = h_1(z) / z and d/dz = -h_2(z) / z with the spherical Hankel
    functions h_1 = -e^{iz} (z + i) / z^2, h_2 = i e^{iz} (z^2 + 3 i z - 3) / z^3.  (SciPy's jv / yv of order 3/2, which the oracle's
    radial_h uses for real arguments, are off by up to 2.3e-14 at z = 8 .. 10.4 against 40-digit values; the library's own radial
    functions by 1e-15.  The sampled field here must be better than the tolerance it is held to.)"""
    e = np.exp(1j * z)
    return -e * (z + 1j) / z ** 3, -1j * e * (z * z + 3j * z - 3.0) / z ** 4


def test_chain_tree_against_the_projection_of_the_sampled_field(amd):
    """bbba (d = 5), n_end 3: the closed form against biem_rhs_project of the sampled monopole at the plan of n_end 6, labels matched as the
    Hessian's layout does; rho / |t| <= 0.025 and k rho <= 0.2, so that the rule of order 6 resolves the field to rounding in the degrees
    < 3 (tests/test_point_source_host.py, whose tolerance this is)."""
    lib, L = amd._biem.L.load(), amd._biem.L
    dev = torch.device("cuda", torch.cuda.current_device())
    small, big = amd._biem._plan("bbba", 3, dev), amd._biem._plan("bbba", 6, dev)
    where = {tuple(lab) + (int(n),): i for i, (lab, n) in enumerate(zip(big.labels.tolist(), big.degrees.tolist()))}
    idx = [where[tuple(lab) + (int(n),)] for lab, n in zip(small.labels.tolist(), small.degrees.tolist())]
    d, B, nb, nrhs = 5, 2, 2, 3
    ks = np.array([0.8, 0.6 + 0.2j])
    cen, _ = geometry(B, d)
    rad = np.array([0.25, 0.2])
    v = np.random.default_rng(5).normal(size=(nrhs, d))
    v = v + 0.3 * np.sign(v)
    S = cen.mean(axis=0)[None] + 12.0 * v / np.linalg.norm(v, axis=-1, keepdims=True)
    assert (np.linalg.norm(S[:, None] - cen[None], axis=-1) >= 10.0).all()
    y = big.quad_y.cpu().numpy()                                            # [Q, d]
    x = cen[:, None, :] + rad[:, None, None] * y[None]                      # [B, Q, d]
    rel = x[None] - S[:, None, None, :]                                     # [nrhs, B, Q, d]
    r = np.linalg.norm(rel, axis=-1)
    z = ks[:, None, None, None] * r[None]                                   # [nb, nrhs, B, Q]
    u, du = _h0_and_derivative_in_five_dimensions(z)
    g = -ROBIN[0] * u - ROBIN[1] * ks[:, None, None, None] * du * (np.einsum("rbqd,qd->rbq", rel, y) / r)[None]
    fs = torch.zeros((nb, nrhs, B * big.H), dtype=torch.complex128, device="cuda")
    L.check(lib.biem_rhs_project(big.handle, nb, B, nrhs, ptr(tc(g)), ptr(fs), nrhs * B * big.H, 1, B * big.H, 0), "biem_rhs_project")
    want = fs.cpu().numpy().reshape(nb, nrhs, B, big.H)[..., idx].reshape(nb, nrhs, -1)
    al, be = tc(np.full((1, B), ROBIN[0])), tc(np.full((1, B), ROBIN[1]))
    tab = _tables(amd, small, nb, B, tc(ks), t(rad), al, be, False)
    for layout in ("natural", "solve"):
        got = _rhs_point_source(amd, small, nb, B, nrhs, tc(ks), t(cen), tab, t(S), 0, layout)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"bbba {layout}: closed form vs sampled projection at n_end 6: {err:.2e} of max |f|")
        assert err <= CHAIN_TOLERANCE


# ---------------------------------------------------------------------------- 4. end to end
def _oracle_densities(tree, n_end, k, cen, rad, alpha, beta, srcs):
    """(closed[nrhs, B, H], sampled[nrhs, B, H]): numpy.linalg.solve of the oracle's matrix with the yardstick's right-hand sides, and
    the oracle's own densities of the sampled monopoles.  alpha / beta scalars (through O.solve_biem) or [B, n_end] (through O.assemble,
    whose ball tables take a coefficient per degree; the sampled right-hand side from the projections under the oracle's n_end-point rule)."""
    tr = O.tree(tree)
    B = len(rad)
    closed, sampled = [], []
    A = None
    for s in srcs:
        if np.ndim(alpha) == 2:
            if A is None:
                A = O.assemble(tr, n_end, k, ETA, cen, rad, alpha, beta)[0]
            deg = tr.degrees(n_end)
            f = np.stack([-(alpha[b][deg] * U + beta[b][deg] * V) for b in range(B)
                          for U, V in [PS.quadrature_projections(tr, n_end, k, cen[b], rad[b], s, n_end)]])
            dens = np.linalg.solve(A.reshape(f.size, f.size), f.reshape(-1)).reshape(f.shape)
        else:
            uin, ugr = O.point_source(k, s, 0)
            res = O.solve_biem(tree, centers=cen, radii=rad, k=k, n_end=n_end, eta=ETA, alpha=alpha, beta=beta, uin=uin, uin_grad=ugr,
                               force_matrix=True)
            A, dens = res.matrix, res.density
        f = PS.rhs(tr, n_end, k, cen, rad, alpha, beta, s, ETA)
        closed.append(np.linalg.solve(A.reshape(f.size, f.size), f.reshape(-1)).reshape(f.shape))
        sampled.append(dens)
    return np.stack(closed), np.stack(sampled)


#        id              tree  B  n_end  ks                     coef     kind     flat   geom_b  nrhs  env
E2E = [
    ("small",           "a",   3, 8,     (1.3, 2.2),            "robin", "outer", False, False,  2,    {}),
    ("blocked",         "ba",  6, 7,     (1.1,),                "robin", "outer", False, False,  2,    {}),
    ("split",           "ba",  4, 6,     (1.2,),                "robin", "outer", True,  False,  2,    {"BIEM_SYM_SPLIT": "1"}),
    ("lu",              "ba",  3, 6,     (1.4, 0.9 + 0.3j),     "robin", "outer", False, False,  2,    {"BIEM_SOLVER": "lu"}),
    ("one_ball",        "ba",  1, 7,     (1.3, 2.0),            "robin", "outer", False, False,  2,    {}),
    ("geometry_batched", "ba", 3, 6,     (1.4, 0.9),            "robin", "outer", False, True,   1,    {}),
    ("fluid",           "ba",  3, 6,     (1.4, 0.9),            "fluid", "outer", False, False,  2,    {}),
    ("inner",           "ba",  3, 6,     (1.4, 0.9),            "soft",  "inner", False, False,  2,    {}),
    ("nrhs70",          "ba",  2, 6,     (1.3,),                "robin", "outer", False, False,  70,   {}),
    ("bpa",             "bpa", 2, 6,     (1.3,),                "robin", "outer", False, False,  2,    {}),
]


@pytest.mark.parametrize("cid,tree,B,n_end,ks,coef,kind,flat,geom_b,nrhs,env", E2E, ids=[e[0] for e in E2E])
def test_end_to_end_against_the_oracle_s_matrix(amd, monkeypatch, cid, tree, B, n_end, ks, coef, kind, flat, geom_b, nrhs, env):
    """biem(point_source_position=) and biem_factorize().solve(point_source_position=) against numpy.linalg.solve of the oracle's matrix
    with the yardstick's right-hand side, relative to max |density| per system: at most max(2 e0, 1e-12), e0 the error of the unchanged
    sampled call against the oracle's own density measured here (one more rounding in the right-hand side; the floor is the project's
    density contract).  k has shape (K, 1), the sources (d, 1, nrhs): right-hand sides of one factorisation per system, each 0.4 .. 1.5
    radii off the nearest surface."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = amd.create_from_branching_types(tree)
    d, K = c.c_ndim, len(ks)
    cen, rad = geometry(B, d, flat)
    cens = np.stack([cen + 0.1 * i for i in range(K)]) if geom_b else np.broadcast_to(cen, (K, B, d))
    rads = np.stack([rad * (1.0 - 0.05 * i) for i in range(K)]) if geom_b else np.broadcast_to(rad, (K, B))
    S = sources([(cens[i], rads[i]) for i in range(K)], nrhs, seed=B + n_end)     # [nrhs, d]
    kt = (tc if any(isinstance(v, complex) for v in ks) else t)(np.asarray(ks)[:, None])
    if coef == "fluid":
        an, bn = fluid_pair(amd, d, n_end, rad, ks)
        kw = dict(alpha_n=tc(an[:, None]), beta_n=tc(bn[:, None]))
        pairs = [(an[i], bn[i]) for i in range(K)]
    else:
        a, b = ROBIN if coef == "robin" else (1.0, 0.0)
        kw = dict(alpha=a, beta=b)
        pairs = [(a, b)] * K
    op = dict(centers=t(cens[:, None] if geom_b else cen[None, None]), radii=t(rads[:, None] if geom_b else rad[None, None]), k=kt,
              eta=t(np.ones((K, 1))), n_end=n_end, kind=kind, **kw)
    St = t(S.T[:, None, :])                                                       # (d, 1, nrhs)
    uin, ugr = amd.point_source(k=kt, source=St, n=0)
    sampled = amd.biem(c, uin=uin, uin_grad=ugr, **op).density.cpu().numpy()
    direct = amd.biem(c, point_source_position=St, **op)
    if cid == "split":
        npE, npO = C.c_int(), C.c_int()
        amd._biem.L.load().biem_last_solve_split(C.byref(npE), C.byref(npO))
        assert npE.value > 0 and npO.value > 0                                     # the flat layout did take the split form
    fac = amd.biem_factorize(c, **op)
    assert (fac.n_lu > 0) == (cid == "lu")
    factored = fac.solve(point_source_position=St)
    assert tuple(direct.density.shape) == tuple(factored.density.shape) == sampled.shape == (K, nrhs, B, direct.density.shape[-1])
    for i in range(K):
        closed, ref = _oracle_densities(tree, n_end, ks[i], cens[i], rads[i], *pairs[i], S)
        scale = np.abs(ref).max()
        e0 = np.abs(sampled[i] - ref).max() / scale
        bound = max(2 * e0, 1e-12)
        for what, got in (("biem", direct.density), ("fac.solve", factored.density)):
            err = np.abs(got[i].cpu().numpy() - closed).max() / np.abs(closed).max()
            print(f"{cid} k={ks[i]} {what}: error {err:.1e}  (sampled call vs the oracle's density e0 = {e0:.1e}; closed vs sampled "
                  f"density {np.abs(closed - ref).max() / scale:.1e})")
            assert err <= bound, (cid, i, what, err, e0)


# ---------------------------------------------------------------------------- 5. reciprocity
@pytest.mark.parametrize("tree", ["ba", "a"])
def test_reciprocity_of_the_device_s_solutions(amd, tree):
    """Three balls, two sources x1, x2 as two right-hand sides of one factorisation; u_scat of each solution at the other source.  The
    defect |u12 - u21| / |u| is at most 2 max(e12, e21, 1e-12), e12 / e21 the errors of the two device values against O.uscat of the
    oracle-matrix solution with the yardstick's right-hand side.  The defect of the sampled call at the same shape is printed."""
    c = amd.create_from_branching_types(tree)
    tr = O.tree(tree)
    d, n_end, k = tr.d, 6, 1.3
    cen, rad = geometry(3, d)
    X = sources([(cen, rad)], 2, seed=11)                                          # [2, d]
    op = dict(centers=t(cen[None]), radii=t(rad[None]), k=t([k]), eta=t([ETA]), n_end=n_end, alpha=ROBIN[0], beta=ROBIN[1])
    Xt = t(X.T)                                                                    # (d, 2): two right-hand sides of the one system
    res = amd.biem_factorize(c, **op).solve(point_source_position=Xt)
    u = res.uscat(Xt).cpu().numpy()                                                # [point, right-hand side]
    u12, u21 = u[1, 0], u[0, 1]
    ref = O.solve_biem(tree, centers=cen, radii=rad, k=k, n_end=n_end, eta=ETA, alpha=ROBIN[0], beta=ROBIN[1])
    A = ref.matrix.reshape(ref.matrix.shape[0] * ref.matrix.shape[1], -1)
    want = []
    for i in (0, 1):
        f = PS.rhs(tr, n_end, k, cen, rad, *ROBIN, X[i], ETA)
        dens = np.linalg.solve(A, f.reshape(-1)).reshape(f.shape)
        want.append(O.uscat(dataclasses.replace(ref, density=dens), X[1 - i][None])[0])
    e12, e21 = abs(u12 - want[0]) / abs(want[0]), abs(u21 - want[1]) / abs(want[1])
    defect = abs(u12 - u21) / abs(u12)
    uin, ugr = amd.point_source(k=t([k]), source=Xt, n=0)
    us = amd.biem(c, uin=uin, uin_grad=ugr, **op).uscat(Xt).cpu().numpy()
    print(f"{tree}: reciprocity defect {defect:.1e} of |u| (errors against the oracle {e12:.1e}, {e21:.1e}); sampled call: "
          f"{abs(us[1, 0] - us[0, 1]) / abs(us[1, 0]):.1e}")
    assert defect <= 2 * max(e12, e21, 1e-12)


# ---------------------------------------------------------------------------- 6. the record
@pytest.mark.parametrize("shape", ["vector", "per_system", "rhs_axis"])
def test_record_matches_the_sampled_call(amd, shape):
    """S of shape (d,) against a scalar k, (d, K) against batch (K,), (d, M, 1) against batch (1, K): the density's shape and namespace
    are the sampled call's, .uin is point_source's callable, NumPy operands give NumPy results."""
    c = amd.create_from_branching_types("ba")
    cen, rad = geometry(2, 3)
    K, M = 3, 4
    if shape == "vector":
        k, S, lead = t(1.3), t(sources([(cen, rad)], 1)[0]), ()
    elif shape == "per_system":
        k, S, lead = t([1.3, 0.9, 1.7]), t(sources([(cen, rad)], K).T), (K,)
    else:
        k, S, lead = t([[1.3, 0.9, 1.7]]), t(sources([(cen, rad)], M).T[:, :, None]), (M, K)
    nd = k.ndim
    op = dict(centers=t(cen[(None,) * nd]), radii=t(rad[(None,) * nd]), k=k, eta=torch.ones_like(k), n_end=6, alpha=ROBIN[0], beta=ROBIN[1])
    uin, ugr = amd.point_source(k=k, source=S, n=0)
    old = amd.biem(c, uin=uin, uin_grad=ugr, **op)
    new = amd.biem(c, point_source_position=S, **op)
    assert new.density.is_cuda and new.density.dtype == old.density.dtype and tuple(new.density.shape) == tuple(old.density.shape) == lead + (2, 36)
    # the same problem, up to the aliasing of the samples: a few percent for sources 0.4 radii off a surface at n_end 6 (measured here:
    # 1.9e-2 .. 3.3e-2), where another problem would differ by O(1)
    diff = float((new.density - old.density).abs().max() / old.density.abs().max())
    print(f"{shape}: closed-form vs sampled density {diff:.1e} of max |density|")
    assert diff <= 0.2
    x = t(np.random.default_rng(1).normal(size=(3, 5)) * 3)
    assert torch.equal(new.uin(x), uin(x[(...,) + (None,) * nd])) and tuple(new.uin(x).shape) == (5,) + lead
    factored = amd.biem_factorize(c, **op).solve(point_source_position=S)
    assert tuple(factored.density.shape) == tuple(new.density.shape) and torch.equal(factored.uin(x), new.uin(x))
    assert (factored.density - new.density).abs().max() <= 1e-12 * new.density.abs().max()
    as_numpy = amd.biem(c, point_source_position=S.cpu().numpy(), **{n: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for n, v in op.items()})
    assert isinstance(as_numpy.density, np.ndarray) and np.array_equal(as_numpy.density, new.density.cpu().numpy())


def test_two_calls_give_the_same_bits(amd):
    c = amd.create_from_branching_types("ba")
    cen, rad = geometry(3, 3)
    k = t([[1.3], [0.9]])
    S = t(sources([(cen, rad)], 70).T[:, None, :])
    op = dict(centers=t(cen[None, None]), radii=t(rad[None, None]), k=k, eta=torch.ones_like(k), n_end=6)
    first, again = amd.biem(c, point_source_position=S, **op).density, amd.biem(c, point_source_position=S, **op).density
    assert torch.isfinite(first.real).all() and torch.equal(first, again)
    fac = amd.biem_factorize(c, **op)
    assert torch.equal(fac.solve(point_source_position=S).density, fac.solve(point_source_position=S).density)
    one = amd.biem(c, point_source_position=S[:, :, :3], **op).density
    assert torch.equal(one, amd.biem(c, point_source_position=S[:, :, :3], **op).density)


def test_a_source_inside_or_on_a_ball_is_a_value_error(amd):
    """Tested on the device before any library call; the message names the source and the ball."""
    c = amd.create_from_branching_types("ba")
    cen, rad = np.array([[0.5, 0.25, 0.0], [4.0, 0.25, 0.0]]), np.array([1.0, 0.5])
    op = dict(centers=t(cen[None]), radii=t(rad[None]), k=t([1.3]), n_end=4)
    outside = np.array([0.5, 3.0, 0.0])
    inside, on = np.array([4.0, 0.5, 0.1]), np.array([1.5, 0.25, 0.0])            # inside ball 1; exactly on the surface of ball 0
    assert np.linalg.norm(on - cen[0]) == rad[0]
    for bad, ball in ((inside, 1), (on, 0)):
        with pytest.raises(ValueError, match=f"source 1 .* ball {ball}"):
            amd.biem(c, point_source_position=t(np.stack([outside, bad]).T), **op)
    fac = amd.biem_factorize(c, **op)
    with pytest.raises(ValueError, match="source 0 .* ball 1"):
        fac.solve(point_source_position=t(inside[:, None]))
    assert torch.isfinite(fac.solve(point_source_position=t(outside[:, None])).density.real).all()


def test_the_order_limit_in_two_dimensions_is_not_implemented(amd):
    """n_end 321 in 2-D: beyond the radial table of a (source, ball) pair, NotImplementedError naming the limit."""
    c = amd.create_from_branching_types("a")
    with pytest.raises(NotImplementedError, match="320"):
        amd.biem(c, centers=t([[0.0, 0.0]]), radii=t([1.0]), k=t(1.3), n_end=321, point_source_position=t([3.0, 0.5]))
