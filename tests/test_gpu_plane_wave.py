"""GPU tests of plane-wave incidence in closed form: ``biem_rhs_plane_wave`` against tests/plane_wave_yardstick.py, the chain tree bbba
against the projection of the sampled wave at a higher order, and ``biem(plane_wave_direction=)`` /
``BIEMFactorization.solve(plane_wave_direction=)`` end to end on every solve path against ``numpy.linalg.solve`` of the oracle's matrix
with the yardstick's right-hand side.  tests/test_plane_wave_host.py pins the yardstick.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

import plane_wave_yardstick as PW  # noqa: E402
from test_plane_wave_host import CHAIN_TOLERANCE  # noqa: E402

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


def directions(d, n, seed=0):
    """[n, d], every component non-zero, not normalised."""
    v = np.random.default_rng(seed).normal(size=(n, d))
    return v + 0.3 * np.sign(v)


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


def _rhs_plane_wave(amd, plan, nb, B, nrhs, k, cen, tab, dirs, batched, layout):
    """biem_rhs_plane_wave into the natural layout [nb, nrhs, B H] or the solve layout [nb, B H, ld] (ld: nrhs rounded up to 8); returns
    f[nb, nrhs, B H].  The solve layout is preset with a sentinel: the columns nrhs .. ld - 1 must keep it."""
    lib, H = amd._biem.L.load(), plan.H
    wb = int(lib.biem_rhs_plane_wave_workspace_bytes(plan.handle, nb, nrhs, batched))
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    if layout == "natural":
        f = torch.full((nb, nrhs, B * H), 7.0, dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)
    else:
        ld = (nrhs + 7) // 8 * 8
        f = torch.full((nb, B * H, ld), 7.0, dtype=torch.complex128, device="cuda")
        strides = (B * H * ld, ld, 1)
    amd._biem.L.check(lib.biem_rhs_plane_wave(plan.handle, nb, B, nrhs, ptr(k), ptr(cen), 0, ptr(tab), ptr(dirs), batched, ptr(f), *strides,
                                              ptr(work), wb, 0), "biem_rhs_plane_wave")
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
        D = directions(d, nb * nrhs, seed=nrhs).reshape(nb, nrhs, d) if batched else np.broadcast_to(directions(d, nrhs, seed=nrhs), (nb, nrhs, d))
        unit = D / np.linalg.norm(D, axis=-1, keepdims=True)
        dirs = t(unit[..., perm] if batched else unit[0][:, perm])
        want = np.stack([np.stack([PW.rhs(tr, n_end, KS[s], cen, rad, *pairs[s], D[s, r]).reshape(-1) for r in range(nrhs)]) for s in range(nb)])
        for layout in ("natural", "solve"):
            got = _rhs_plane_wave(amd, plan, nb, B, nrhs, k, t(cen[:, perm]), tab, dirs, int(batched), layout)
            err = max(np.abs(got[s] - want[s]).max() / np.abs(want[s]).max() for s in range(nb))
            worst = max(worst, err)
            assert err <= 1e-12, (tree, coef, batched, nrhs, layout, err)
    print(f"{tree} {coef} {'batched' if batched else 'shared'} directions: worst error / max |f| {worst:.1e}")


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("coef", ["robin", "fluid"])
@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "caa"])
def test_rhs_plane_wave_against_the_yardstick(amd, tree, coef, batched):
    """Two systems (k = 1.3 and 0.9 + 0.3i), two balls, nrhs = 1 and 5, both write layouts: 1e-12 of max |f| per system."""
    _kernel_case(amd, tree, coef, batched)


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
def test_rhs_plane_wave_with_the_right_hand_sides_along_the_lanes(amd, batched):
    """nrhs = 70 in the solve layout (more than a wave of contiguous right-hand sides: the form with r along the lanes) and in the natural one."""
    _kernel_case(amd, "ba", "robin", batched, nrhs_list=(70,), n_end=9)


# ---------------------------------------------------------------------------- 2. a chain tree
def test_chain_tree_against_the_projection_of_the_sampled_wave(amd):
    """bbba (d = 5), n_end 3: the closed form against biem_rhs_project of the sampled wave at the plan of n_end 6, labels matched as the
    Hessian's layout does, k rho <= 0.4 (the rule of order 6 resolves the wave to rounding in the degrees < 3).  Tolerance: the one
    measured for the CPU chain test (tests/test_plane_wave_host.py)."""
    lib, L = amd._biem.L.load(), amd._biem.L
    dev = torch.device("cuda", torch.cuda.current_device())
    small, big = amd._biem._plan("bbba", 3, dev), amd._biem._plan("bbba", 6, dev)
    where = {tuple(lab) + (int(n),): i for i, (lab, n) in enumerate(zip(big.labels.tolist(), big.degrees.tolist()))}
    idx = [where[tuple(lab) + (int(n),)] for lab, n in zip(small.labels.tolist(), small.degrees.tolist())]
    d, B, nb, nrhs = 5, 2, 2, 3
    ks = np.array([0.8, 0.6 + 0.2j])
    cen, rad = geometry(B, d)
    # k rho <= 0.2: the rule of order 6 is exact to degree 11, so a harmonic of degree <= 2 aliases with the wave's degrees >= 10, whose
    # size against degree 0 is (k rho)^10 / 21!! - 8e-15 at k rho = 0.4, as large as the tolerance; 1e-17 at 0.2
    rad = np.array([0.25, 0.2])
    D = directions(d, nrhs, seed=5)
    unit = D / np.linalg.norm(D, axis=-1, keepdims=True)
    y = big.quad_y.cpu().numpy()                                            # [Q, d]
    x = cen[None, :, None, :] + rad[None, :, None, None] * y[None, None]    # [1, B, Q, d]
    phase = np.exp(1j * ks[:, None, None, None] * np.einsum("sbqd,rd->rbq", x, unit)[None])          # [nb, nrhs, B, Q]
    dn = 1j * ks[:, None, None, None] * (y @ unit.T).T[None, :, None, :] * phase
    g = tc(-ROBIN[0] * phase - ROBIN[1] * dn)
    fs = torch.zeros((nb, nrhs, B * big.H), dtype=torch.complex128, device="cuda")
    L.check(lib.biem_rhs_project(big.handle, nb, B, nrhs, ptr(g), ptr(fs), nrhs * B * big.H, 1, B * big.H, 0), "biem_rhs_project")
    want = fs.cpu().numpy().reshape(nb, nrhs, B, big.H)[..., idx].reshape(nb, nrhs, -1)
    al, be = tc(np.full((1, B), ROBIN[0])), tc(np.full((1, B), ROBIN[1]))
    tab = _tables(amd, small, nb, B, tc(ks), t(rad), al, be, False)
    for layout in ("natural", "solve"):
        got = _rhs_plane_wave(amd, small, nb, B, nrhs, tc(ks), t(cen), tab, t(unit), 0, layout)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"bbba {layout}: closed form vs sampled projection at n_end 6: {err:.2e} of max |f|")
        assert err <= CHAIN_TOLERANCE


# ---------------------------------------------------------------------------- 3. end to end
def _oracle_densities(tree, n_end, k, cen, rad, alpha, beta, dirs):
    """(closed[nrhs, B, H], sampled[nrhs, B, H]): numpy.linalg.solve of the oracle's matrix with the yardstick's right-hand sides, and
    the oracle's own densities of the sampled waves.  alpha / beta scalars (through O.solve_biem) or [B, n_end] (through O.assemble, whose
    ball tables take a coefficient per degree; the sampled right-hand side from the projections under the oracle's n_end-point rule)."""
    tr = O.tree(tree)
    B = len(rad)
    closed, sampled = [], []
    A = None
    for p in dirs:
        if np.ndim(alpha) == 2:
            if A is None:
                A = O.assemble(tr, n_end, k, ETA, cen, rad, alpha, beta)[0]
            deg = tr.degrees(n_end)
            f = np.stack([-(alpha[b][deg] * U + beta[b][deg] * V) for b in range(B)
                          for U, V in [PW.quadrature_projections(tr, n_end, k, cen[b], rad[b], p, n_end)]])
            dens = np.linalg.solve(A.reshape(f.size, f.size), f.reshape(-1)).reshape(f.shape)
        else:
            uin, ugr = O.plane_wave(k, p)
            res = O.solve_biem(tree, centers=cen, radii=rad, k=k, n_end=n_end, eta=ETA, alpha=alpha, beta=beta, uin=uin, uin_grad=ugr,
                               force_matrix=True)
            A, dens = res.matrix, res.density
        f = PW.rhs(tr, n_end, k, cen, rad, alpha, beta, p, ETA)
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
    """biem(plane_wave_direction=) and biem_factorize().solve(plane_wave_direction=) against numpy.linalg.solve of the oracle's matrix
    with the yardstick's right-hand side, relative to max |density| per system: at most max(2 e0, 1e-12), e0 the error of the unchanged
    sampled call against the oracle's own density measured here (one more rounding in the right-hand side; the floor is the project's
    density contract).  k has shape (K, 1), the directions (d, 1, nrhs): right-hand sides of one factorisation per system."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = amd.create_from_branching_types(tree)
    d, K = c.c_ndim, len(ks)
    cen, rad = geometry(B, d, flat)
    cens = np.stack([cen + 0.1 * i for i in range(K)]) if geom_b else np.broadcast_to(cen, (K, B, d))
    rads = np.stack([rad * (1.0 - 0.05 * i) for i in range(K)]) if geom_b else np.broadcast_to(rad, (K, B))
    D = directions(d, nrhs, seed=B + n_end)                                       # [nrhs, d]
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
    Dt = t(D.T[:, None, :])                                                       # (d, 1, nrhs)
    uin, ugr = amd.plane_wave(k=kt, direction=Dt)
    sampled = amd.biem(c, uin=uin, uin_grad=ugr, **op).density.cpu().numpy()
    direct = amd.biem(c, plane_wave_direction=Dt, **op)
    if cid == "split":
        npE, npO = C.c_int(), C.c_int()
        amd._biem.L.load().biem_last_solve_split(C.byref(npE), C.byref(npO))
        assert npE.value > 0 and npO.value > 0                                     # the flat layout did take the split form
    fac = amd.biem_factorize(c, **op)
    assert (fac.n_lu > 0) == (cid == "lu")
    factored = fac.solve(plane_wave_direction=Dt)
    assert tuple(direct.density.shape) == tuple(factored.density.shape) == sampled.shape == (K, nrhs, B, direct.density.shape[-1])
    for i in range(K):
        closed, ref = _oracle_densities(tree, n_end, ks[i], cens[i], rads[i], *pairs[i], D)
        scale = np.abs(ref).max()
        e0 = np.abs(sampled[i] - ref).max() / scale
        bound = max(2 * e0, 1e-12)
        for what, got in (("biem", direct.density), ("fac.solve", factored.density)):
            err = np.abs(got[i].cpu().numpy() - closed).max() / np.abs(closed).max()
            print(f"{cid} k={ks[i]} {what}: error {err:.1e}  (sampled call vs the oracle's density e0 = {e0:.1e}; closed vs sampled "
                  f"density {np.abs(closed - ref).max() / scale:.1e})")
            assert err <= bound, (cid, i, what, err, e0)


# ---------------------------------------------------------------------------- 4. the record
@pytest.mark.parametrize("shape", ["vector", "per_system", "rhs_axis"])
def test_record_matches_the_sampled_call(amd, shape):
    """D of shape (d,) against a scalar k, (d, K) against batch (K,), (d, M, 1) against batch (1, K): the density's shape and namespace
    are the sampled call's, .uin is plane_wave's callable, and the length of D does not matter, not even in the last bit."""
    c = amd.create_from_branching_types("ba")
    cen, rad = geometry(2, 3)
    K, M = 3, 4
    if shape == "vector":
        k, D, lead = t(1.3), t(directions(3, 1)[0]), ()
    elif shape == "per_system":
        k, D, lead = t([1.3, 0.9, 1.7]), t(directions(3, K).T), (K,)
    else:
        k, D, lead = t([[1.3, 0.9, 1.7]]), t(directions(3, M).T[:, :, None]), (M, K)
    nd = k.ndim
    op = dict(centers=t(cen[(None,) * nd]), radii=t(rad[(None,) * nd]), k=k, eta=torch.ones_like(k), n_end=6, alpha=ROBIN[0], beta=ROBIN[1])
    uin, ugr = amd.plane_wave(k=k, direction=D)
    old = amd.biem(c, uin=uin, uin_grad=ugr, **op)
    new = amd.biem(c, plane_wave_direction=D, **op)
    assert new.density.is_cuda and new.density.dtype == old.density.dtype and tuple(new.density.shape) == tuple(old.density.shape) == lead + (2, 36)
    assert (new.density - old.density).abs().max() <= 1e-3 * old.density.abs().max()       # the same problem, up to the aliasing of the samples
    x = t(np.random.default_rng(1).normal(size=(3, 5)) * 3)
    assert torch.equal(new.uin(x), uin(x[(...,) + (None,) * nd])) and tuple(new.uin(x).shape) == (5,) + lead
    assert torch.equal(amd.biem(c, plane_wave_direction=2 * D, **op).density, new.density)
    factored = amd.biem_factorize(c, **op).solve(plane_wave_direction=D)
    assert tuple(factored.density.shape) == tuple(new.density.shape) and torch.equal(factored.uin(x), new.uin(x))
    assert (factored.density - new.density).abs().max() <= 1e-12 * new.density.abs().max()
    as_numpy = amd.biem(c, plane_wave_direction=D.cpu().numpy(), **{n: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for n, v in op.items()})
    assert isinstance(as_numpy.density, np.ndarray) and np.array_equal(as_numpy.density, new.density.cpu().numpy())


def test_integer_directions_are_accepted(amd):
    c = amd.create_from_branching_types("ba")
    cen, rad = geometry(2, 3)
    op = dict(centers=cen, radii=rad, k=np.array(1.3), n_end=5)
    a = amd.biem(c, plane_wave_direction=np.array([2, -1, 2]), **op).density
    b = amd.biem(c, plane_wave_direction=np.array([2.0, -1.0, 2.0]) / 3.0, **op).density
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------- 5. determinism
def test_two_calls_give_the_same_bits(amd):
    c = amd.create_from_branching_types("ba")
    cen, rad = geometry(3, 3)
    k = t([[1.3], [0.9]])
    D = t(directions(3, 70).T[:, None, :])
    op = dict(centers=t(cen[None, None]), radii=t(rad[None, None]), k=k, eta=torch.ones_like(k), n_end=6)
    first, again = amd.biem(c, plane_wave_direction=D, **op).density, amd.biem(c, plane_wave_direction=D, **op).density
    assert torch.isfinite(first.real).all() and torch.equal(first, again)
    fac = amd.biem_factorize(c, **op)
    assert torch.equal(fac.solve(plane_wave_direction=D).density, fac.solve(plane_wave_direction=D).density)
    one = amd.biem(c, plane_wave_direction=D[:, :, :3], **op).density
    assert torch.equal(one, amd.biem(c, plane_wave_direction=D[:, :, :3], **op).density)
