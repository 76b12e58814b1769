"""GPU tests of the layer below the field kernels at the orders and arguments production reaches: the radial functions of
``biem_radial`` / ``biem_radial_complex`` to nmax = 320 and |z| = 16384, the per-ball tables of ``biem_ball_tables`` /
``biem_ball_tables_n`` on every plan, and the 2-D matrix fill at n_end = 152, 200 (pair table in the LDS) and 400 (global scratch),
against the 40-digit values of tests/golden/radial_full_order.npz (tools/make_radial_fixtures.py, oracle/mp_radial.py).

This file reads only the fixture and NumPy: every expected value comes with the scale its error is measured against and with the
weight max(n + 1, |z|) of the bound

    |got - expected| <= min(C * 2^-52 * weight, 1e-11) * scale

(a relative perturbation delta of the argument changes these functions by about weight * delta; 1e-11 is what the
small-argument tests of tests/test_gpu_parity.py already hold the kernels to).  One C per group, 8 x the largest ratio measured on an
MI355X rounded up to a power of two; the measured ratios are in DESIGN.md 5f and each test prints its own before it asserts.
"""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radial_full_order.npz")
EPS = 2.0 ** -52
CAP = 1e-11
# largest ratios measured on an MI355X: real 1.6, complex 6.53, tables 32.9, matrix 8.85
C = {"real": 16.0, "complex": 64.0, "tables": 512.0, "matrix": 128.0}


@pytest.fixture(scope="module")
def fx():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {name: z[name] for name in z.files}


@pytest.fixture(scope="module")
def meta(fx):
    return json.loads(str(fx["meta"]))


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), device="cuda").to(dtype).contiguous()


def _check(group, what, got, want, scale, weight, where):
    """Print the largest ratio error / (2^-52 weight scale) with its place, then assert the bound on every value."""
    assert np.isfinite(got).all(), what
    rel = np.abs(got - want) / scale
    ratio = rel / (EPS * weight)
    i = int(np.argmax(ratio))
    print(f"  {what}: largest ratio {ratio[i]:.3g} (error {rel[i]:.2e} of the scale) at {where(i)}; {len(ratio)} values")
    bad = np.flatnonzero(~(rel <= np.minimum(C[group] * EPS * weight, CAP)))
    assert bad.size == 0, f"{what}: {bad.size} of {rel.size} values miss the bound, the first at {where(int(bad[0]))}: {rel[bad[0]]:.2e}"
    return float(ratio[i])


# ---------------------------------------------------------------------------- radial functions
@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 9, 10])
@pytest.mark.parametrize("entry", ["real", "complex"])
def test_radial_functions_at_full_order(amd, fx, meta, entry, d):
    from biem_helmholtz_sphere_amd import _lib as L
    nmax = meta["dims"][str(d)]
    p = f"rad/{entry}/d{d}/"
    arg, a, n = fx[p + "arg"], fx[p + "a"].astype(np.int64), fx[p + "n"].astype(np.int64)
    cplx = entry == "complex"
    dt = torch.complex128 if cplx else torch.float64
    out = torch.zeros((len(arg), 2, nmax + 1), dtype=dt, device="cuda")
    x = _dev(arg, dt)
    L.check((L.load().biem_radial_complex if cplx else L.load().biem_radial)(d, nmax, len(arg), x.data_ptr(), out.data_ptr(), None))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    z_want = fx[p + "z"]
    h_want = fx[p + "h"] if cplx else z_want + 1j * fx[p + "y"]
    z_got = out[a, 0, n]
    h_got = out[a, 1, n] if cplx else out[a, 0, n] + 1j * out[a, 1, n]
    w = fx[p + "weight"].astype(np.float64)

    def where(i):
        return f"z = {arg[a[i]]}, n = {n[i]}"
    _check(entry, f"{entry} d = {d}: z_n", z_got, z_want, np.abs(z_want) * fx[p + "z_ratio"].astype(np.float64), w, where)
    _check(entry, f"{entry} d = {d}: h_n", h_got, h_want, np.abs(h_want), w, where)


# ---------------------------------------------------------------------------- per-ball tables
@pytest.mark.parametrize("pid", ["a", "ba", "bba", "caa", "chain5"])
def test_ball_tables_of_every_plan(amd, fx, meta, pid):
    from biem_helmholtz_sphere_amd import _biem, _lib as L
    plan_meta = next(q for q in meta["plans"] if q["id"] == pid)
    n_end = plan_meta["n_end"]
    p = f"tab/{pid}/"
    lib = L.load()
    plan = _biem._plan(plan_meta["tree"], n_end, torch.device("cuda", torch.cuda.current_device()))
    assert plan.d == plan_meta["d"]
    ks = fx[p + "k"]
    nb, B = len(ks), len(fx[p + "radii"])
    k_d, eta_d, rad_d = _dev(ks, torch.complex128), _dev(fx[p + "eta"]), _dev(fx[p + "radii"])
    got = {}
    for entry, al, be in ((lib.biem_ball_tables, fx[p + "alpha"], fx[p + "beta"]), (lib.biem_ball_tables_n, fx[p + "alpha_n"], fx[p + "beta_n"])):
        al_d, be_d = _dev(al, torch.complex128), _dev(be, torch.complex128)
        tab = torch.zeros((nb, B, 3, n_end), dtype=torch.complex128, device="cuda")
        L.check(entry(plan.handle, nb, B, k_d.data_ptr(), eta_d.data_ptr(), rad_d.data_ptr(), 0, al_d.data_ptr(), be_d.data_ptr(), 0, tab.data_ptr(), None))
        torch.cuda.synchronize()
        got[al.ndim] = tab.cpu().numpy()
    s, b, n = (fx[p + nm].astype(np.int64) for nm in ("s", "b", "n"))
    w = fx[p + "weight"].astype(np.float64)

    def where(i):
        return f"k = {ks[s[i]]}, ball {b[i]}, n = {n[i]}"
    for name, ndim, slot in (("gj", 1, 0), ("gh", 1, 1), ("blc", 1, 2), ("gj_n", 2, 0), ("gh_n", 2, 1), ("blc", 2, 2)):
        want = fx[p + name]
        _check("tables", f"{pid} {name}" + (" (degree-dependent entry)" if ndim == 2 else ""), got[ndim][s, b, slot, n], want,
               np.abs(want) * fx[p + name + "_ratio"].astype(np.float64), w, where)


# ---------------------------------------------------------------------------- the 2-D matrix at high order
def _matrix_cases():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return [c["id"] for c in json.loads(str(z["meta"]))["matrix"]]


def _labels(n_end):
    """m of the 2-D harmonics in the library's order, |m|, and |mu| = |m' - m| [m, m']."""
    ms = np.concatenate([np.arange(n_end), np.arange(-(n_end - 1), 0)])
    return ms, np.abs(ms), np.abs(ms[None, :] - ms[:, None])


def off_diagonal_block(n_end, Hk, E, gj, blc, flipped):
    """A[b, m, b', m'] from the factors: Hk[mu] = H_mu(k |t|), E[mu] = e^{i mu phi} of t (flipped: the block of -t, phi + pi),
    gj [n_end] of the row ball, blc [n_end] of the column ball."""
    ms, deg, amu = _labels(n_end)
    mu = ms[None, :] - ms[:, None]
    sign = np.array([1.0, 1.0j, -1.0, -1.0j])[(deg[:, None] + amu - deg[None, :]) % 4]
    ph = np.where(mu >= 0, E[amu], np.conj(E[amu]))
    if flipped:
        ph = ph * np.where(amu % 2 == 0, 1.0, -1.0)
    return sign * Hk[amu] * ph * gj[deg][:, None] * blc[deg][None, :]


@pytest.mark.parametrize("cid", _matrix_cases())
def test_matrix_2d_at_high_order(amd, fx, meta, cid):
    """calc.matrix of two discs (radii 1.0, 0.8; soft, eta = 1) element-wise against the product of the stored 40-digit factors,
    A[b, m, b', m'] = i^{|m| + |mu| - |m'|} H_{|mu|}(k |t|) e^{i mu phi} gj_b[|m|] blc_b'[|m'|],  mu = m' - m,  t = c_b - c_b'
    (four fp64 products: a 3-ulp reference), relative to the entry; the diagonal blocks exactly diagonal with gh blc."""
    c = next(q for q in meta["matrix"] if q["id"] == cid)
    n_end, k = c["n_end"], c["k"]
    cen, rad = np.array(c["centers"]), np.array(c["radii"])
    calc = amd.biem(amd.create_from_branching_types("a"), centers=_dev(cen), radii=_dev(rad), k=_dev(k), eta=_dev(1.0), n_end=n_end, alpha=1.0, beta=0.0)
    M = calc.matrix.cpu().numpy()
    Hn = 2 * n_end - 1
    assert M.shape == (2, Hn, 2, Hn) and np.isfinite(M).all()
    ms, deg, amu = _labels(n_end)
    Hk, E = fx[c["H"]][:Hn], fx[c["E"]][:Hn]
    gj, gh, blc = (fx[c["tab"] + "/" + nm][:, :n_end] for nm in ("gj", "gh", "blc"))
    kt = k * float(np.hypot(*(cen[0] - cen[1])))
    for b in range(2):
        bp = 1 - b
        want = off_diagonal_block(n_end, Hk, E, gj[b], blc[bp], flipped=b == 1)
        w = np.maximum(amu + 1.0, kt) + np.maximum(deg + 1.0, k * rad[b])[:, None] + np.maximum(deg + 1.0, k * rad[bp])[None, :]

        def where(i, b=b):
            r, q = divmod(i, Hn)
            return f"block ({b}, {1 - b}), m = {ms[r]}, m' = {ms[q]}"
        _check("matrix", f"{cid} block ({b}, {bp})", M[b, :, bp, :].ravel(), want.ravel(), np.abs(want).ravel(), w.ravel(), where)
        D = M[b, :, b, :]
        assert np.count_nonzero(D - np.diag(np.diag(D))) == 0
        dw = gh[b][deg] * blc[b][deg]
        _check("matrix", f"{cid} diagonal of ball {b}", np.diag(D).copy(), dw, np.abs(dw), 2.0 * np.maximum(deg + 1.0, k * rad[b]), lambda i: f"m = {ms[i]}")
