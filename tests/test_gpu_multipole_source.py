"""GPU tests of multipole incidence in closed form: ``biem_rhs_multipole`` against tests/multipole_source_yardstick.py, against a column of
the library's own matrix with a probe ball at the source, sliced against unsliced, ``biem(multipole_source_position=,
multipole_source_index=)`` / ``BIEMFactorization.solve`` end to end on every solve path against ``numpy.linalg.solve`` of the oracle's
matrix with the yardstick's right-hand side, the record's ``.uin`` / ``multipole_source`` against NumPy twins, and the errors.
tests/test_multipole_source_host.py pins the yardstick.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import biem_oracle as O  # noqa: E402  (test infrastructure: the checker)

import chain_yardstick as CY  # noqa: E402
import multipole_source_yardstick as MS  # noqa: E402
import point_source_yardstick as PS  # noqa: E402
from test_gpu_point_source import E2E, ETA, FLUID, KS, ROBIN, _oracle_densities, _tables, fluid_pair, geometry, ptr, sources, t, tc  # noqa: E402
from test_multipole_source_host import _outgoing  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def ti(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")


def index_set(tr, n_end):
    """Five positions on the harmonic axis: degree 0, the first of degree 1, a conjugate pair of degree 1, the top degree."""
    h0, one, partner, top = MS.source_indices(tr, n_end)
    return [h0, int(np.nonzero(tr.degrees(n_end) == 1)[0][0]), one, partner, top]


# ---------------------------------------------------------------------------- 1. the kernel against the yardstick
def _rhs_multipole(amd, plan, nb, B, nrhs, k, cen, tab, src, idx, batched, layout):
    """biem_rhs_multipole into the natural layout [nb, nrhs, B H] or the solve layout [nb, B H, ld] (ld: nrhs rounded up to 8); returns
    f[nb, nrhs, B H].  The solve layout is preset with a sentinel: the columns nrhs .. ld - 1 must keep it."""
    lib, H = amd._biem.L.load(), plan.H
    wb = int(lib.biem_rhs_multipole_workspace_bytes(plan.handle, nb, B, nrhs, batched, 0))
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    if layout == "natural":
        f = torch.full((nb, nrhs, B * H), 7.0, dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)
    else:
        ld = (nrhs + 7) // 8 * 8
        f = torch.full((nb, B * H, ld), 7.0, dtype=torch.complex128, device="cuda")
        strides = (B * H * ld, ld, 1)
    amd._biem.L.check(lib.biem_rhs_multipole(plan.handle, nb, B, nrhs, ptr(k), ptr(cen), 0, ptr(tab), ptr(src), batched, ptr(idx), ptr(f),
                                             *strides, ptr(work), wb, 0), "biem_rhs_multipole")
    torch.cuda.synchronize()
    f = f.cpu().numpy()
    if layout == "natural":
        return f
    assert (f[:, :, nrhs:] == 7.0).all()
    return f[:, :, :nrhs].transpose(0, 2, 1)


def _kernel_case(amd, tree, coef, batched, n_end, nrhs_list=(1, 5), indices=None):
    from biem_helmholtz_sphere_amd._coords import canonical_tree

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
    pool = indices or index_set(tr, n_end)
    worst = 0.0
    for nrhs in nrhs_list:
        S = (sources([(cen, rad)], nb * nrhs, seed=nrhs).reshape(nb, nrhs, d) if batched
             else np.broadcast_to(sources([(cen, rad)], nrhs, seed=nrhs), (nb, nrhs, d)))
        first = [pool[(len(pool) - 1 + r) % len(pool)] for r in range(nrhs)]          # nrhs 1: the top degree; nrhs 5: all five
        I = np.stack([first, first[::-1]]) if batched else np.broadcast_to(first, (nb, nrhs))
        src = t(S[..., perm] if batched else S[0][:, perm])
        idx = ti(I if batched else I[0])
        want = np.stack([np.stack([MS.rhs(tr, n_end, KS[s], cen, rad, *pairs[s], S[s, r], int(I[s, r]), ETA).reshape(-1) for r in range(nrhs)])
                         for s in range(nb)])
        for layout in ("natural", "solve"):
            got = _rhs_multipole(amd, plan, nb, B, nrhs, k, t(cen[:, perm]), tab, src, idx, int(batched), layout)
            err = max(np.abs(got[s, r] - want[s, r]).max() / np.abs(want[s, r]).max() for s in range(nb) for r in range(nrhs))
            worst = max(worst, err)
            assert err <= 1e-12, (tree, coef, batched, nrhs, layout, err)
    print(f"{tree} n_end {n_end} {coef} {'batched' if batched else 'shared'} sources: worst error / max |f| per right-hand side {worst:.1e}")


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("coef", ["robin", "fluid"])
@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba", "caa"])
def test_rhs_multipole_against_the_yardstick(amd, tree, coef, batched):
    """Two systems (k = 1.3 and 0.9 + 0.3i), two balls, nrhs = 1 and 5, sources of degree 0, 1 (a conjugate pair among them) and
    n_end - 1, both write layouts: 1e-12 of max |f| per (system, right-hand side) - a source of a high degree dwarfs a monopole."""
    _kernel_case(amd, tree, coef, batched, {"a": 6, "ba": 5, "bpa": 5, "bba": 4, "caa": 3}[tree])


def test_rhs_multipole_at_a_middle_order(amd):
    """ba at n_end 12, sources of degree 0, 1 and 11."""
    tr = O.tree("ba")
    h0, one, _, top = MS.source_indices(tr, 12)
    _kernel_case(amd, "ba", "robin", False, 12, nrhs_list=(3,), indices=[one, top, h0])


def test_rhs_multipole_on_a_chain_tree_against_the_plan_s_tables(amd):
    """bbba (d = 5), n_end 3: f = -gj_n sum_p coef[p] T[tidx[p]] with the plan's own term lists (biem_plan_terms) and the table
    T = C_d h_n''(k |t|) Y_l(t^) of tests/chain_yardstick's harmonics, as tests/test_multipole_source_host.py builds it."""
    lib, L = amd._biem.L.load(), amd._biem.L
    d, n_end, B, nb = 5, 3, 2, 2
    plan = amd._biem._plan("bbba", n_end, torch.device("cuda", torch.cuda.current_device()))
    H = plan.H
    ptr_, coef, tidx = np.zeros(H * H + 1, dtype=np.int64), np.zeros(plan.n_terms), np.zeros(plan.n_terms, dtype=np.int32)
    L.check(lib.biem_plan_terms(plan.handle, ptr_.ctypes.data, coef.ctypes.data, tidx.ctypes.data), "biem_plan_terms")
    ch, g = CY.chain(d), CY.gaunt(d, n_end)
    assert [tuple(v) for v in plan.labels.tolist()] == [tuple(v) for v in ch.index(n_end)]
    ks = np.array([0.8, 0.6 + 0.2j])
    cen, rad = geometry(B, d)
    idx = [0, int(np.nonzero(plan.degrees == 1)[0][-1]), int(np.nonzero(plan.degrees == 1)[0][0]), H - 1]
    nrhs = len(idx)
    S = sources([(cen, rad)], nrhs, seed=5)
    al, be = tc(np.full((1, B), ROBIN[0])), tc(np.full((1, B), ROBIN[1]))
    tab = _tables(amd, plan, nb, B, tc(ks), t(rad), al, be, False)
    gj = tab.cpu().numpy()[:, :, 0, :]                                       # [nb, B, n_end]
    want = np.zeros((nb, nrhs, B, H), dtype=np.complex128)
    for s in range(nb):
        for r in range(nrhs):
            for b in range(B):
                tv = cen[b] - S[r]
                dist = np.linalg.norm(tv)
                T = PS.c_d(d) * _outgoing(g.n2 - 1, d, ks[s] * dist)[g.deg2] * ch.harmonics((tv / dist)[None, :], g.n2)[:, 0]
                row = np.array([coef[ptr_[h * H + idx[r]]:ptr_[h * H + idx[r] + 1]] @ T[tidx[ptr_[h * H + idx[r]]:ptr_[h * H + idx[r] + 1]]]
                                for h in range(H)])
                want[s, r, b] = -gj[s, b][plan.degrees] * row
    want = want.reshape(nb, nrhs, B * H)
    for layout in ("natural", "solve"):
        got = _rhs_multipole(amd, plan, nb, B, nrhs, tc(ks), t(cen), tab, t(S), ti(idx), 0, layout)
        err = max(np.abs(got[s, r] - want[s, r]).max() / np.abs(want[s, r]).max() for s in range(nb) for r in range(nrhs))
        print(f"bbba {layout}: closed form vs the plan-table yardstick {err:.2e} of max |f| per right-hand side")
        assert err <= 1e-12


# ---------------------------------------------------------------------------- 2. a column of the library's own matrix
@pytest.mark.parametrize("tree", ["ba", "bba"])
def test_the_right_hand_side_is_a_column_of_the_library_s_own_matrix(amd, tree):
    """B balls plus one probe ball at s (radius 0.1): with calc.matrix in the reference's scaling, A[b, h, probe, h'] =
    gj_n(b) (S|R)_{h'->h}(c_b - s) blc_n'(probe), so f(b, h) = -A[b, h, probe, h'] / blc_n'(probe): the new contraction against the fill,
    no oracle in between.  1e-12 of max |f| per (system, right-hand side)."""
    tr = O.tree(tree)
    c = amd.create_from_branching_types(tree)
    d, B, nb, n_end = tr.d, 2, 2, {"ba": 5, "bba": 4}[tree]
    plan = amd._biem._plan(tree, n_end, torch.device("cuda", torch.cuda.current_device()))
    cen, rad = geometry(B, d)
    idx = index_set(tr, n_end)
    S = sources([(cen, rad)], len(idx), seed=3)
    k = tc(KS)
    deg = plan.degrees
    al1, be1 = tc(np.full((1, B + 1), ROBIN[0])), tc(np.full((1, B + 1), ROBIN[1]))
    for r, hp in enumerate(idx):
        cen1, rad1 = np.concatenate([cen, S[r][None]]), np.concatenate([rad, [0.1]])
        assert (np.linalg.norm(cen - S[r][None], axis=-1) > rad + 0.1).all()
        A = amd.biem(c, centers=t(cen1[None]), radii=t(rad1[None]), k=k, eta=t(np.ones(nb)), n_end=n_end, alpha=ROBIN[0], beta=ROBIN[1]).matrix
        A = A.cpu().numpy()                                                    # [nb, B + 1, H, B + 1, H]
        tab1 = _tables(amd, plan, nb, B + 1, k, t(rad1), al1, be1, False)
        blc = tab1.cpu().numpy()[:, B, 2, deg[hp]]                             # [nb]
        want = -A[:, :B, :, B, hp] / blc[:, None, None]                        # [nb, B, H]
        tab = tab1[:, :B].contiguous()
        got = _rhs_multipole(amd, plan, nb, B, 1, k, t(cen), tab, t(S[r][None]), ti([hp]), 0, "natural")[:, 0].reshape(nb, B, -1)
        for s in range(nb):
            err = np.abs(got[s] - want[s]).max() / np.abs(want[s]).max()
            print(f"{tree} k {KS[s]} h' {hp} (degree {deg[hp]}): rhs vs the matrix column {err:.1e}")
            assert err <= 1e-12, (tree, s, hp, err)


# ---------------------------------------------------------------------------- 3. slices
def test_slices_do_not_change_a_bit(amd, monkeypatch):
    """BIEM_RHS_TABLE_BYTES set so that the walk over (systems x right-hand sides) takes four slices: the result is bit for bit the
    unsliced one, and two plain calls give the same bits."""
    lib = amd._biem.L.load()
    tr, n_end, B, nb, nrhs = O.tree("ba"), 5, 2, 2, 5
    plan = amd._biem._plan("ba", n_end, torch.device("cuda", torch.cuda.current_device()))
    cen, rad = geometry(B, 3)
    S = sources([(cen, rad)], nb * nrhs, seed=9).reshape(nb, nrhs, 3)
    pool = index_set(tr, n_end)
    I = np.stack([pool, pool[::-1]])
    k = tc(KS)
    tab = _tables(amd, plan, nb, B, k, t(rad), tc(np.full((1, B), ROBIN[0])), tc(np.full((1, B), ROBIN[1])), False)
    run = lambda layout: _rhs_multipole(amd, plan, nb, B, nrhs, k, t(cen), tab, t(S), ti(I), 1, layout)
    per_pair = B * plan.H2 * 16
    whole = int(lib.biem_rhs_multipole_workspace_bytes(plan.handle, nb, B, nrhs, 1, 0))
    assert whole >= nb * nrhs * per_pair
    plain = {layout: run(layout) for layout in ("natural", "solve")}
    for layout in plain:
        assert np.isfinite(plain[layout]).all() and np.array_equal(plain[layout], run(layout))
    monkeypatch.setenv("BIEM_RHS_TABLE_BYTES", str(3 * per_pair))                  # 10 pairs in slices of 3, 3, 3, 1
    sliced = int(lib.biem_rhs_multipole_workspace_bytes(plan.handle, nb, B, nrhs, 1, 0))
    assert 3 * per_pair <= sliced < 4 * per_pair
    for layout in plain:
        assert np.array_equal(plain[layout], run(layout))
    monkeypatch.setenv("BIEM_RHS_TABLE_BYTES", "1")                                # below one pair: one pair per slice
    assert per_pair <= int(lib.biem_rhs_multipole_workspace_bytes(plan.handle, nb, B, nrhs, 1, 0)) < 2 * per_pair
    assert np.array_equal(plain["solve"], run("solve"))


# ---------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("cid,tree,B,n_end,ks,coef,kind,flat,geom_b,nrhs,env", E2E, ids=[e[0] for e in E2E])
def test_end_to_end_against_the_oracle_s_matrix(amd, monkeypatch, cid, tree, B, n_end, ks, coef, kind, flat, geom_b, nrhs, env):
    """biem(multipole_source_position=, multipole_source_index=) and biem_factorize().solve(...) against numpy.linalg.solve of the
    oracle's matrix with the yardstick's right-hand side, sources of degree 0, 1 and 2 in turn, relative to max |density| per (system,
    right-hand side): at most max(2 e0, 1e-12), e0 the error of the unchanged sampled point_source(n=0) call on the same geometry against
    the oracle's own density, measured here - the method of tests/test_gpu_point_source.py, on the rows of its table."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = amd.create_from_branching_types(tree)
    tr = O.tree(tree)
    d, K = c.c_ndim, len(ks)
    cen, rad = geometry(B, d, flat)
    cens = np.stack([cen + 0.1 * i for i in range(K)]) if geom_b else np.broadcast_to(cen, (K, B, d))
    rads = np.stack([rad * (1.0 - 0.05 * i) for i in range(K)]) if geom_b else np.broadcast_to(rad, (K, B))
    S = sources([(cens[i], rads[i]) for i in range(K)], nrhs, seed=B + n_end)     # [nrhs, d]
    deg = tr.degrees(n_end)
    by_degree = [int(np.nonzero(deg == n)[0][-1]) for n in (0, 1, 2)]
    I = np.array([by_degree[r % 3] for r in range(nrhs)])
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
    direct = amd.biem(c, multipole_source_position=St, multipole_source_index=I[None, :], **op)
    if cid == "split":
        npE, npO = C.c_int(), C.c_int()
        amd._biem.L.load().biem_last_solve_split(C.byref(npE), C.byref(npO))
        assert npE.value > 0 and npO.value > 0                                     # the flat layout did take the split form
    fac = amd.biem_factorize(c, **op)
    assert (fac.n_lu > 0) == (cid == "lu")
    factored = fac.solve(multipole_source_position=St, multipole_source_index=ti(I))
    assert tuple(direct.density.shape) == tuple(factored.density.shape) == sampled.shape == (K, nrhs, B, direct.density.shape[-1])
    for i in range(K):
        _, ref = _oracle_densities(tree, n_end, ks[i], cens[i], rads[i], *pairs[i], S)
        e0 = np.abs(sampled[i] - ref).max() / np.abs(ref).max()
        bound = max(2 * e0, 1e-12)
        if np.ndim(pairs[i][0]) == 2:
            A = O.assemble(tr, n_end, ks[i], ETA, cens[i], rads[i], *pairs[i])[0]
        else:
            A = O.solve_biem(tree, centers=cens[i], radii=rads[i], k=ks[i], n_end=n_end, eta=ETA, alpha=pairs[i][0], beta=pairs[i][1]).matrix
        N = B * len(deg)
        F = np.stack([MS.rhs(tr, n_end, ks[i], cens[i], rads[i], *pairs[i], S[r], int(I[r]), ETA).reshape(-1) for r in range(nrhs)], axis=1)
        closed = np.linalg.solve(A.reshape(N, N), F).T.reshape(nrhs, B, -1)
        for what, got in (("biem", direct.density), ("fac.solve", factored.density)):
            g = got[i].cpu().numpy()
            err = max(np.abs(g[r] - closed[r]).max() / np.abs(closed[r]).max() for r in range(nrhs))
            print(f"{cid} k={ks[i]} {what}: error {err:.1e} per right-hand side  (sampled point-source call vs the oracle's density e0 = {e0:.1e})")
            assert err <= bound, (cid, i, what, err, e0)


# ---------------------------------------------------------------------------- 5. the record
def _central_difference(f, x, h):
    """Gradient [d, P] of f at x [P, d] by the 6th-order central difference of step h."""
    w = np.array([-1.0, 9.0, -45.0, 0.0, 45.0, -9.0, 1.0]) / 60.0
    out = []
    for i in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[i] = h
        out.append(sum(w[j + 3] * f(x + j * e[None]) for j in range(-3, 4) if j) / h)
    return np.stack(out)


@pytest.mark.parametrize("tree", ["a", "ba", "bpa", "bba"])
def test_record_uin_and_multipole_source_against_numpy_twins(amd, tree):
    """.uin of a closed-form call is multipole_source's callable; uin at 50 points against O.radial_h-type radial function times the
    tree's harmonic (1e-12 of its maximum: one radial recurrence and one harmonic), uin_grad against the 6th-order central difference of
    that twin, within 4 times the difference's own truncation error, estimated by halving the step.  Both figures are printed."""
    c = amd.create_from_branching_types(tree)
    tr = O.tree(tree)
    d, n_end, nd = tr.d, 5, 1
    cen, rad = geometry(2, d)
    ks = np.array([1.3, 0.9 + 0.3j])
    S = sources([(cen, rad)], 1, seed=2)[0]
    rng = np.random.default_rng(4)
    v = rng.normal(size=(50, d))
    x = S[None] + rng.uniform(0.5, 3.0, (50, 1)) * v / np.linalg.norm(v, axis=-1, keepdims=True)
    for hp in index_set(tr, n_end)[1:]:
        k = tc(ks)
        res = amd.biem(c, centers=t(cen[None]), radii=t(rad[None]), k=k, n_end=n_end, alpha=ROBIN[0], beta=ROBIN[1],
                       multipole_source_position=t(S[:, None]), multipole_source_index=hp)
        uin, ugr = amd.multipole_source(c, k=k, source=t(S[:, None]), index=hp, n_end=n_end)
        xt = t(x.T)
        got = res.uin(xt)
        assert tuple(got.shape) == (50, 2) and torch.equal(got, uin(xt[..., None]))
        got, grad = got.cpu().numpy(), ugr(xt[..., None]).cpu().numpy()
        assert grad.shape == (d, 50, 2)
        for s in range(2):
            twin = lambda y: MS.multipole_samples(tr, n_end, ks[s], S, hp, y)
            want = twin(x)
            err = np.abs(got[:, s] - want).max() / np.abs(want).max()
            coarse, fine = _central_difference(twin, x, 0.02), _central_difference(twin, x, 0.01)
            trunc = np.abs(coarse - fine).max() / np.abs(fine).max()
            gerr = np.abs(grad[:, :, s] - fine).max() / np.abs(fine).max()
            print(f"{tree} k {ks[s]} h' {hp}: uin {err:.1e}; uin_grad vs the central difference {gerr:.1e}, its truncation error {trunc:.1e}")
            assert err <= 1e-12 and gerr <= 4 * trunc, (tree, s, hp, err, gerr, trunc)
    as_numpy = amd.multipole_source(c, k=ks, source=S[:, None], index=hp, n_end=n_end)[0](x.T[..., None])
    assert isinstance(as_numpy, np.ndarray) and np.array_equal(as_numpy, got)


def test_utotal_of_a_dipole_has_no_nan_outside_the_balls(amd):
    c = amd.create_from_branching_types("ba")
    n_end, B = 5, 2
    cen, rad = geometry(B, 3)
    ks = np.array([1.3])
    an, bn = fluid_pair(amd, 3, n_end, rad, ks)
    S = sources([(cen, rad)], 1, seed=6)[0]
    one = MS.source_indices(O.tree("ba"), n_end)[1]
    res = amd.biem(c, centers=t(cen[None]), radii=t(rad[None]), k=t(ks), n_end=n_end, alpha_n=tc(an), beta_n=tc(bn),
                   multipole_source_position=t(S[:, None]), multipole_source_index=one)
    rng = np.random.default_rng(8)
    x = rng.uniform(-3.0, 6.0, (400, 3))
    keep = (np.linalg.norm(x[:, None] - cen[None], axis=-1) > rad[None]).all(axis=1) & (np.linalg.norm(x - S[None], axis=-1) > 0.3)
    x = x[keep]
    assert len(x) >= 100
    ut = res.utotal(t(x.T), k_interior=tc(FLUID[0][:B]), density_ratio=t(FLUID[1][:B])).cpu().numpy()
    assert ut.shape == (len(x), 1) and np.isfinite(ut).all()
    assert np.array_equal(ut, (res.uin(t(x.T)) + res.uscat(t(x.T))).cpu().numpy())


# ---------------------------------------------------------------------------- 6. errors
def test_a_source_inside_or_on_a_ball_is_a_value_error(amd):
    """Tested on the device before any library call; the message names the argument, the source and the ball."""
    c = amd.create_from_branching_types("ba")
    cen, rad = np.array([[0.5, 0.25, 0.0], [4.0, 0.25, 0.0]]), np.array([1.0, 0.5])
    op = dict(centers=t(cen[None]), radii=t(rad[None]), k=t([1.3]), n_end=4)
    outside = np.array([0.5, 3.0, 0.0])
    inside, on = np.array([4.0, 0.5, 0.1]), np.array([1.5, 0.25, 0.0])            # inside ball 1; exactly on the surface of ball 0
    assert np.linalg.norm(on - cen[0]) == rad[0]
    for bad, ball in ((inside, 1), (on, 0)):
        with pytest.raises(ValueError, match=f"multipole_source_position: source 1 .* ball {ball}"):
            amd.biem(c, multipole_source_position=t(np.stack([outside, bad]).T), multipole_source_index=np.array([1, 2]), **op)
    fac = amd.biem_factorize(c, **op)
    with pytest.raises(ValueError, match="source 0 .* ball 1"):
        fac.solve(multipole_source_position=t(inside[:, None]), multipole_source_index=1)
    assert torch.isfinite(fac.solve(multipole_source_position=t(outside[:, None]), multipole_source_index=1).density.real).all()


def test_the_order_limit_in_two_dimensions_is_not_implemented(amd):
    """n_end 321 in 2-D: beyond the radial row of a (source, ball) pair, NotImplementedError naming the limit."""
    c = amd.create_from_branching_types("a")
    with pytest.raises(NotImplementedError, match="320"):
        amd.biem(c, centers=t([[0.0, 0.0]]), radii=t([1.0]), k=t(1.3), n_end=321, multipole_source_position=t([3.0, 0.5]),
                 multipole_source_index=2)
