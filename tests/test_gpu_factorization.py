"""GPU tests of factor once, solve many: biem_factorize(...).solve(...) against biem(), the oracle and numpy.linalg.solve."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


@pytest.fixture(scope="module")
def lib(amd):
    from biem_helmholtz_sphere_amd import _lib as L

    return L.load(), L


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), device="cuda").to(dtype).contiguous()


def _geometry(rng, B, d, gap=1.15):
    cen, rad = [], []
    while len(cen) < B:
        c = rng.uniform(-4, 4, size=d)
        r = rng.uniform(0.4, 1.0)
        if all(np.linalg.norm(c - c2) > gap * (r + r2) for c2, r2 in zip(cen, rad)):
            cen.append(c)
            rad.append(r)
    return np.array(cen), np.array(rad)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _factor_bits(fac):
    return None if fac._factors is None else fac._factors.view(torch.int64).clone()


# tree, B, n_end, k (per system), alpha, beta, kind, geometry batched
PARITY = [
    ("a", 3, 8, [1.3, 2.2], 1.0, 0.0, "outer", False),                 # N = 45: one-launch path
    ("ba", 3, 6, [1.4, 0.9], 1.0, 1.0, "outer", False),                # N = 108, Robin
    ("ba", 6, 7, [1.1, 1.7], 1.0, 0.0, "outer", False),                # N = 294, n_pad = 320: blocked path, a full four-panel group
    ("ba", 3, 6, [1.2 + 0.3j, 0.8 + 0.1j], 1.0, 0.0, "outer", False),  # complex k
    ("ba", 3, 6, [1.4, 0.9], 1.0, 0.0, "inner", False),
    ("ba", 3, 6, [1.4, 0.9], 1.0, 1.0, "outer", True),                 # geometry per system
    ("bpa", 3, 6, [1.4, 0.9], 1.0, 0.0, "outer", False),               # primed tree: perm
    ("bba", 2, 4, [1.2, 1.9], 1.0, 1.0, "outer", False),
    ("caa", 3, 4, [1.2, 1.9], 1.0, 0.0, "outer", False),
    ("ba", 1, 7, [1.3, 2.0], 1.0, 1.0, "outer", False),                # B = 1: the tables-only shortcut
]


@pytest.mark.parametrize("tree,B,n_end,ks,alpha,beta,kind,geom_b", PARITY)
def test_factorized_solve_matches_biem(amd, tree, B, n_end, ks, alpha, beta, kind, geom_b):
    rng = np.random.default_rng(sum(map(ord, tree)) + B + n_end)
    c = amd.create_from_branching_types(tree)
    d = c.c_ndim
    K = len(ks)
    cen, rad = _geometry(rng, B, d)
    if geom_b:
        cen = np.stack([cen + 0.1 * i for i in range(K)])
        rad = np.stack([rad * (1.0 - 0.05 * i) for i in range(K)])
    else:
        cen, rad = cen[None], rad[None]
    kt = _dev(ks, torch.complex128 if any(isinstance(v, complex) for v in ks) else torch.float64)
    dirs = rng.normal(size=(d, K))
    uin, ugr = amd.plane_wave(k=kt, direction=_dev(dirs))
    kw = dict(centers=_dev(cen), radii=_dev(rad), k=kt, eta=_dev(np.full(K, 1.2)), n_end=n_end, alpha=alpha, beta=beta, kind=kind)
    ref = amd.biem(c, uin=uin, uin_grad=ugr, **kw)
    fac = amd.biem_factorize(c, **kw)
    assert fac.n_symmetric + fac.n_lu == (K if B > 1 else 0) and fac.nbytes > 0
    res = fac.solve(uin=uin, uin_grad=ugr)
    assert tuple(res.density.shape) == tuple(ref.density.shape)
    assert _rel(res.density.cpu().numpy(), ref.density.cpu().numpy()) <= 1e-12
    if kind == "outer":
        x = rng.normal(size=(d, 5)) * 2.0 + 9.0
    else:
        x = (cen[0, 0] + 0.3 * rad[0, 0] * rng.uniform(-1, 1, size=(5, d)) / math.sqrt(d)).T
    u, uref = res.uscat(_dev(x)).cpu().numpy(), ref.uscat(_dev(x)).cpu().numpy()
    fin = np.isfinite(uref)                                   # (the field's own NaN mask, e.g. points outside an inner domain)
    assert np.array_equal(np.isfinite(u), fin) and (fin.any() or kind == "inner")
    if fin.any():
        assert _rel(u[fin], uref[fin]) <= 1e-12
    if B > 1:
        assert torch.equal(torch.as_tensor(res.matrix), torch.as_tensor(ref.matrix))


def test_factorized_solve_against_oracle(amd):
    rng = np.random.default_rng(3)
    cen, rad = _geometry(rng, 3, 3)
    k, eta, n_end, alpha, beta = 1.4, 1.3, 6, 1.0, 0.5
    direction = rng.normal(size=3)
    x = np.array([[6.0, 0.5, 0.2], [-5.0, 2.0, 1.0], [0.5, 7.0, -2.0]])
    uo, go = O.plane_wave(k, direction)
    ores = O.solve_biem("ba", centers=cen, radii=rad, k=k, n_end=n_end, eta=eta, alpha=alpha, beta=beta, uin=uo, uin_grad=go)
    c = amd.create_from_branching_types("ba")
    fac = amd.biem_factorize(c, centers=_dev(cen), radii=_dev(rad), k=_dev(k), eta=_dev(eta), n_end=n_end, alpha=alpha, beta=beta)
    uin, ugr = amd.plane_wave(k=_dev(k), direction=_dev(direction))
    res = fac.solve(uin=uin, uin_grad=ugr)
    dens = res.density.cpu().numpy()
    assert np.max(np.abs(dens - ores.density) / (np.abs(ores.density) + 1e-12 * np.abs(ores.density).max())) < 1e-8
    ref = O.uscat(ores, x)
    assert np.max(np.abs(res.uscat(_dev(x.T)).cpu().numpy() - ref) / np.abs(ref)) < 1e-10


def test_many_incidences_later(amd):
    """One factorisation; 64 plane-wave directions in one call, the same in 8 calls, and a point source: each equals biem()."""
    c = amd.create_from_branching_types("ba")
    rng = np.random.default_rng(8)
    cen, rad = _geometry(rng, 4, 3)
    ks = np.array([1.3])
    kw = dict(centers=_dev(cen)[None], radii=_dev(rad)[None], k=_dev(ks), n_end=7, alpha=1.0, beta=0.4)
    fac = amd.biem_factorize(c, **kw)
    before = _factor_bits(fac)
    ang = rng.uniform(0, 2 * np.pi, size=64)
    dirs = np.stack([np.cos(ang), np.sin(ang), 0.3 * np.ones(64)])[:, None, :]    # (d, 1, 64): k axis, then the incidences
    k2 = _dev(ks)[:, None]
    kw2 = dict(kw, k=k2, centers=kw["centers"][None], radii=kw["radii"][None])
    fac2 = amd.biem_factorize(c, **kw2)
    uin, ugr = amd.plane_wave(k=k2, direction=_dev(dirs))
    ref = amd.biem(c, uin=uin, uin_grad=ugr, **kw2)
    res = fac2.solve(uin=uin, uin_grad=ugr)
    assert tuple(res.density.shape) == (1, 64, 4, 49)
    assert _rel(res.density.cpu().numpy(), ref.density.cpu().numpy()) <= 1e-12
    again = fac2.solve(uin=uin, uin_grad=ugr)
    assert torch.equal(again.density, res.density)                                 # bit for bit
    for p in range(8):
        u8, g8 = amd.plane_wave(k=k2, direction=_dev(dirs[:, :, 8 * p:8 * p + 8]))
        part = fac2.solve(uin=u8, uin_grad=g8).density
        assert _rel(part.cpu().numpy(), ref.density[:, 8 * p:8 * p + 8].cpu().numpy()) <= 1e-12
    us, gs = amd.point_source(k=_dev(ks), source=_dev([[0.5], [7.0], [-1.0]]), n=0)
    refp = amd.biem(c, uin=us, uin_grad=gs, **kw)
    resp = fac.solve(uin=us, uin_grad=gs)
    assert _rel(resp.density.cpu().numpy(), refp.density.cpu().numpy()) <= 1e-12
    assert torch.equal(_factor_bits(fac), before)                                 # the stored factors are never written


def test_numpy_in_numpy_out_and_alpha_beta_rules(amd):
    c = amd.create_from_branching_types("ba")
    cen = np.array([[0.0, 1.7, 0.1], [0.2, -1.6, 0.0]])
    fac = amd.biem_factorize(c, centers=cen, radii=np.ones(2), k=np.asarray(1.2), n_end=5, alpha=1.0, beta=0.5)
    uin, ugr = amd.plane_wave(k=np.asarray(1.2), direction=np.array([1.0, 0.0, 0.0]))
    res = fac.solve(uin=uin, uin_grad=ugr)
    ref = amd.biem(c, centers=cen, radii=np.ones(2), k=np.asarray(1.2), n_end=5, alpha=1.0, beta=0.5, uin=uin, uin_grad=ugr)
    assert isinstance(res.density, np.ndarray) and _rel(res.density, ref.density) <= 1e-12
    with pytest.raises(ValueError, match="uin_grad must be provided"):
        fac.solve(uin=uin)
    with pytest.raises(ValueError, match="uin must be provided"):
        fac.solve(uin_grad=ugr)
    fac.close()
    assert fac.nbytes == 0
    with pytest.raises(ValueError, match="closed"):
        fac.solve(uin=uin, uin_grad=ugr)


def test_rejected_systems_are_kept_in_lu_form(amd, monkeypatch):
    """Systems the symmetric factorisation rejects are factored by the pivoted LU into the same slot; their densities match
    biem() with BIEM_SOLVER=lu."""
    c = amd.create_from_branching_types("ba")
    cen = np.zeros((2, 3))
    cen[0, 1], cen[1, 1] = 1.02, -1.02
    ks = np.array([1.0, 2.5, 3.3])
    dirs = np.zeros((3, 3))
    dirs[0] = 1.0
    uin, _ = amd.plane_wave(k=_dev(ks), direction=_dev(dirs))
    kw = dict(centers=_dev(cen)[None], radii=_dev(np.ones(2))[None], k=_dev(ks), n_end=12)
    monkeypatch.setenv("BIEM_LDLT_PIVOT_REL", "1e30")
    fac = amd.biem_factorize(c, **kw)
    monkeypatch.delenv("BIEM_LDLT_PIVOT_REL")
    assert fac.n_lu == 3 and fac.n_symmetric == 0
    monkeypatch.setenv("BIEM_SOLVER", "lu")
    ref = amd.biem(c, uin=uin, **kw)
    monkeypatch.delenv("BIEM_SOLVER")
    res = fac.solve(uin=uin)
    assert _rel(res.density.cpu().numpy(), ref.density.cpu().numpy()) <= 1e-12


def test_factor_does_not_fit_states_the_bytes(amd):
    c = amd.create_from_branching_types("ba")
    free, _ = torch.cuda.mem_get_info()
    avail = free + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()    # (what torch's allocator holds counts as available)
    nb = int(avail // (1024 * 1024 * 16)) + 64                     # factors of nb systems of 1024 unknowns exceed it
    cen = torch.as_tensor(np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 6.0, 0.0], [3.0, 0.0, 0.0]]), device="cuda")
    k = torch.linspace(1.0, 2.0, nb, dtype=torch.float64, device="cuda")
    with pytest.raises(torch.OutOfMemoryError, match="bytes"):
        amd.biem_factorize(c, centers=cen[None].expand(nb, 4, 3), radii=torch.ones((nb, 4), dtype=torch.float64, device="cuda"), k=k,
                           n_end=16)                                               # N = 4 * 256 = 1024


# ---------------------------------------------------------------------------- the kernels alone, through the ABI
def _sym_case(nb, n_pad, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    M = torch.view_as_complex(torch.randn((nb, n_pad, n_pad, 2), dtype=torch.float64, device="cuda", generator=g))
    M *= 0.12 / math.sqrt(n_pad)
    M = M + M.transpose(1, 2)
    M.diagonal(dim1=1, dim2=2).add_(1.0 + 0.2j)
    return M


@pytest.mark.parametrize("n_pad", [64, 128, 512, 4096])
@pytest.mark.parametrize("nb", [1, 3, 64])
def test_sym_factor_then_solve_vs_numpy(lib, n_pad, nb):
    l, L = lib
    if n_pad == 4096 and nb == 64:
        nb_check = [0, 63]
    else:
        nb_check = list(range(nb))
    M = _sym_case(nb, n_pad, n_pad + nb)
    A = M.clone()
    blk = torch.arange(n_pad, device="cuda") // 64
    A.masked_fill_(blk[:, None] > blk[None, :], 1e30)       # the strict lower triangle of tiles is never read
    info = torch.ones(nb, dtype=torch.int32, device="cuda")
    wb = l.biem_lu_workspace_bytes(nb, n_pad, 0)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    L.check(l.biem_sym_factor(nb, n_pad, A.data_ptr(), n_pad, n_pad * n_pad, info.data_ptr(), work.data_ptr(), wb, None))
    torch.cuda.synchronize()
    del work
    assert (info == 0).all()
    U = torch.triu(A)
    for s in nb_check[:3]:
        assert torch.max(torch.abs(U[s].T @ U[s] - M[s])) < 1e-12 * torch.max(torch.abs(M[s]))
    Ucopy = A.view(torch.int64).clone()
    Mh = {s: M[s].cpu().numpy() for s in nb_check}
    del M
    for nrhs in (1, 7, 8, 64, 200):
        ldb = nrhs + 3
        Bm = torch.view_as_complex(torch.randn((nb, n_pad, ldb, 2), dtype=torch.float64, device="cuda"))
        X = Bm.clone()
        L.check(l.biem_sym_solve(nb, n_pad, nrhs, A.data_ptr(), n_pad, n_pad * n_pad, X.data_ptr(), ldb, n_pad * ldb, None))
        torch.cuda.synchronize()
        assert torch.equal(X[:, :, nrhs:], Bm[:, :, nrhs:])           # columns past nrhs untouched
        for s in nb_check:
            ref = np.linalg.solve(Mh[s], Bm[s, :, :nrhs].cpu().numpy())
            assert _rel(X[s, :, :nrhs].cpu().numpy(), ref) < 1e-12, (s, nrhs)
    assert torch.equal(A.view(torch.int64), Ucopy)


def test_factor_and_solve_entries_check_their_arguments(amd, lib):
    l, L = lib
    from biem_helmholtz_sphere_amd import _biem as impl

    dev = torch.device("cuda", torch.cuda.current_device())
    plan = impl._plan("ba", 5, dev)
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    n_pad = l.biem_lu_npad(2 * plan.H)
    need = l.biem_factor_workspace_bytes(plan.handle, 1, 2, 0)
    rc = l.biem_factor_ldlt(plan.handle, 1, 2, p, p, p, p, 0, p, p, 0, p, n_pad - 1, n_pad * n_pad, p, p, 0, p, need, None)
    assert rc != L.BIEM_OK and b"lda" in l.biem_last_error()
    rc = l.biem_factor_ldlt(plan.handle, 1, 2, p, p, p, p, 0, p, p, 0, p, n_pad, n_pad * n_pad, p, p, 0, p, need - 1, None)
    assert rc != L.BIEM_OK and b"workspace" in l.biem_last_error()
    rc = l.biem_factor_ldlt(plan.handle, 65536, 2, p, p, p, p, 0, p, p, 0, p, n_pad, n_pad * n_pad, p, p, 0, p, need, None)
    assert rc != L.BIEM_OK and b"65535" in l.biem_last_error()
    sneed = l.biem_solve_factored_workspace_bytes(plan.handle, 1, 2, 3)
    assert sneed == n_pad * 8 * 16
    rc = l.biem_solve_factored(plan.handle, 1, 2, 3, p, n_pad, n_pad * n_pad, p, p, p, p, sneed - 1, None)
    assert rc != L.BIEM_OK and b"workspace" in l.biem_last_error()
    rc = l.biem_solve_factored(plan.handle, 1, 2, 3, p, n_pad - 1, n_pad * n_pad, p, p, p, p, sneed, None)
    assert rc != L.BIEM_OK and b"lda" in l.biem_last_error()
    rc = l.biem_solve_factored(plan.handle, 1, 2, 65536, p, n_pad, n_pad * n_pad, p, p, p, p, sneed, None)
    assert rc != L.BIEM_OK and b"65535" in l.biem_last_error()
