"""CPU tests of the yardstick behind tests/test_gpu_radial_full_order.py: the evaluator ``oracle/mp_radial.py`` and the fixture
``tests/golden/radial_full_order.npz`` that ``tools/make_radial_fixtures.py`` writes with it.

1. At low order (nmax <= 40, |z| <= 30) the evaluator equals the golden-pinned fp64 oracle to 1e-12 of the scale each quantity is
   measured against: ``O.radial``, ``O.radial_h``, ``O.ball_tables``, and ``translation_SR_2d_graf`` at n_end = 9.  The way the GPU
   test multiplies the stored factors into matrix blocks equals ``O.assemble`` there.
2. The fixture is what the generator makes: one stored value per case recomputed bit for bit (mpmath on Python integers is
   deterministic), within the size limit, with every value inside the fp64 range it promises.
"""
import json
import os

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import test_gpu_radial_full_order as G  # noqa: E402  (its block assembly; nothing in it runs at import)
from oracle import biem_oracle as O  # noqa: E402
from oracle import mp_radial as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with np.load(G.FIXTURE, allow_pickle=False) as _z:
    FX = {name: _z[name] for name in _z.files}
META = json.loads(str(FX["meta"]))
DIMS = sorted(int(d) for d in META["dims"])


def _c(v):
    return np.array([complex(t) for t in v])


# ---------------------------------------------------------------------------- 1. low order against the oracle
@pytest.mark.parametrize("d", DIMS)
def test_radial_equals_the_oracle_at_low_order(d):
    nmax = 40
    for z in (0.05, 1.0, 2.404825557695773, 7.3, 29.5, 1.3 + 0.25j, 5 + 3j, 20 + 8j, 3 - 0.4j, 12 - 2j, 0.05 + 0.02j, 8 + 15j):
        j, h = R.radial(nmax, d, z)
        sj, sh, _ = R.radial_scales(nmax, d, z, j, h)
        if isinstance(z, float):
            jo, yo, _, _ = O.radial(nmax, d, z)
            ho = jo + 1j * yo
        else:
            jo, ho, _, _ = O.radial_h(nmax, d, z)
        ok = np.isfinite(ho) & (np.abs(ho) < 1e290)
        ej = np.max((np.abs(jo - _c(j)) / np.array(sj))[ok])
        eh = np.max((np.abs(ho - _c(h)) / np.array(sh))[ok])
        print(f"  d = {d} z = {z}: z_n {ej:.1e}, h_n {eh:.1e}")
        assert ej <= 1e-12 and eh <= 1e-12, (d, z)


def test_scale_of_the_regular_function():
    """Relative from the turning point on and for |z| <= 1; below it the envelope, which at a zero of z_n is the singular function."""
    z = 2.404825557695773
    j, h = R.radial(4, 2, z)
    sj, sh, w = R.radial_scales(4, 2, z, j, h)
    assert abs(complex(j[0])) < 1e-15 and sj[0] == pytest.approx(abs(complex(h[0])), rel=1e-12)      # J_0 at its first zero
    assert sj[3] == abs(j[3]) and sh[2] == abs(h[2]) and w == [z, z, 3.0, 4.0, 5.0]
    j, h = R.radial(2, 2, 1e-3)
    assert R.radial_scales(2, 2, 1e-3, j, h)[0][0] == abs(j[0])
    assert R.digits(300 + 40j) == 40 + 35 and R.digits(300 - 40j) == 75 and R.digits(7.0) == 40


@pytest.mark.parametrize("tree,n_end", [("a", 40), ("ba", 24), ("bba", 12), ("caa", 12)])
def test_ball_tables_equal_the_oracle_at_low_order(tree, n_end):
    tr = O.tree(tree)
    for k, eta, rho, al, be in ((0.5, 1.0, 1.0, 1.0, 0.0), (8.0, 0.6, 0.8, 0.0, 1.0), (30.0, 1.0, 0.37, 1 + 0.25j, 0.4 - 0.1j), (3 + 0.4j, 0.6, 0.8, 1 + 0.25j, 0.4 - 0.1j)):
        t = R.ball_tables(tr.d, n_end, k, eta, rho, al, be)
        for name, want in zip(("gj", "gh", "blc"), O.ball_tables(tr, n_end, k, eta, rho, al, be)):
            ok = np.isfinite(want) & (np.abs(want) < 1e290)
            err = np.max((np.abs(want - _c(t[name])) / np.array(t[name + "_scale"]))[ok])
            print(f"  {tree} k = {k}: {name} {err:.1e}")
            assert err <= 1e-12, (tree, k, name)
    # one pair per degree: each degree is the scalar table of its own pair
    an, bn = np.linspace(0.5, 2.0, n_end) * (1 + 0.25j), np.linspace(1.0, -1.0, n_end) * (0.4 - 0.1j)
    tn = R.ball_tables(tr.d, n_end, 8.0, 0.6, 0.8, an, bn)
    for n in (0, 3, n_end - 1):
        t1 = R.ball_tables(tr.d, n_end, 8.0, 0.6, 0.8, complex(an[n]), complex(bn[n]))
        assert all(tn[name][n] == t1[name][n] for name in ("gj", "gh", "blc", "gj_scale", "gh_scale", "blc_scale"))


def test_translation_2d_equals_the_oracle():
    n_end, k = 9, 1.7
    for t in (np.array([4.0, 0.0]), np.array([-4.0, 0.0]), np.array([0.0, 4.0]), np.array([3.1, -2.7]), np.array([-3.1, 2.7])):
        want = O.translation_SR_2d_graf(n_end, k, t)
        got = R.translation_2d(n_end, k, t)
        err = np.max(np.abs(got - want) / np.abs(want))
        print(f"  t = {t}: {err:.1e}")
        assert err <= 1e-12


def test_block_assembly_of_the_gpu_test_equals_the_oracle():
    """``off_diagonal_block`` with factors from mp_radial against ``O.assemble`` (both blocks, so t and -t; its diagonal is gh blc)."""
    n_end, k, eta = 9, 1.7, 1.0
    tr = O.tree("a")
    cen, rad = np.array([[0.0, 0.0], [3.1, -2.7]]), np.array([1.0, 0.8])
    A, _ = O.assemble(tr, n_end, k, eta, cen, rad, np.ones(2), np.zeros(2))
    Hk, E = (_c(v) for v in R.translation_2d_factors(n_end, k, cen[0] - cen[1]))
    tabs = [R.ball_tables(2, n_end, k, eta, rho, 1.0, 0.0) for rho in rad]
    deg = tr.degrees(n_end)
    assert np.array_equal(deg, G._labels(n_end)[1])
    for b in range(2):
        got = G.off_diagonal_block(n_end, Hk, E, _c(tabs[b]["gj"]), _c(tabs[1 - b]["blc"]), flipped=b == 1)
        assert np.max(np.abs(got - A[b, :, 1 - b, :]) / np.abs(got)) <= 1e-12
        assert np.max(np.abs(np.diag(A[b, :, b, :]) - (_c(tabs[b]["gh"]) * _c(tabs[b]["blc"]))[deg]) / np.abs(np.diag(A[b, :, b, :]))) <= 1e-12


# ---------------------------------------------------------------------------- 2. the fixture
def test_fixture_size_and_range():
    assert os.path.getsize(G.FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "full_order_fields.npz"))
    assert os.path.getsize(G.FIXTURE) <= 1 << 20
    for name, a in FX.items():
        if name == "meta" or a.dtype.kind not in "fc" or name.endswith(("_ratio", "weight", "/arg", "/eta", "/radii", "/alpha", "/beta", "/alpha_n", "/beta_n", "/k")):
            continue
        m = np.abs(a)
        assert ((m >= 1e-280) & (m <= 1e280)).all(), name
    for entry in ("real", "complex"):
        for d in DIMS:
            p = f"rad/{entry}/d{d}/"
            r = FX[p + "z_ratio"]
            assert np.isfinite(r).all() and (r >= 1.0 - 1e-6).all(), p
            nmax = META["dims"][str(d)]
            arg, a, n = FX[p + "arg"], FX[p + "a"], FX[p + "n"]
            assert n.max() == nmax and len(arg) <= 24 and set(a) == set(range(len(arg)))       # every argument reaches the test
            if d in (2, 3):                                                                      # ... and the top order where it matters
                full = (318.7, 320.0) if entry == "real" else (20 - 8j, 300 - 40j)
                for zf in full:
                    i = int(np.flatnonzero(arg == zf)[0])
                    stored = n[a == i]                                   # (z_n(20 - 8i) leaves the fp64 range near n = 283)
                    assert np.array_equal(stored, np.arange(len(stored))) and len(stored) >= (250 if zf == 20 - 8j else nmax + 1), (p, zf)
    neg = FX["rad/complex/d3/arg"].imag < 0
    assert neg.sum() >= 4
    for c in META["matrix"]:
        assert len(FX[c["H"]]) >= 2 * c["n_end"] - 1 and len(FX[c["E"]]) >= 2 * c["n_end"] - 1 and FX[c["tab"] + "/gj"].shape[1] >= c["n_end"]
    assert sorted(c["n_end"] for c in META["matrix"]) == [152, 152, 152, 200, 400]


@pytest.mark.parametrize("entry", ["real", "complex"])
@pytest.mark.parametrize("d", DIMS)
def test_stored_radial_value_is_what_the_generator_makes(entry, d):
    """One record per argument, recomputed from the stored argument: bit-equal fp64, scale and weight included.  (The three arguments
    of |Im z| >= 150 run at 170 to 560 digits, half a minute in the even dimensions: they are left to the generator's --check.)"""
    p = f"rad/{entry}/d{d}/"
    nmax = META["dims"][str(d)]
    arg, a, n = FX[p + "arg"], FX[p + "a"], FX[p + "n"]
    for ai in range(len(arg)):
        rec = np.flatnonzero(a == ai)
        i = int(rec[(7 * ai + d) % len(rec)])
        z = float(arg[ai]) if entry == "real" else complex(arg[ai])
        if R.digits(z) > 120:
            continue
        j, h = R.radial(nmax, d, z)
        sj, _, w = R.radial_scales(nmax, d, z, j, h)
        zj, zh = complex(j[n[i]]), complex(h[n[i]])
        if entry == "real":
            assert (FX[p + "z"][i], FX[p + "y"][i]) == (zj.real, zh.imag), (d, z, n[i])
        else:
            assert (FX[p + "z"][i], FX[p + "h"][i]) == (zj, zh), (d, z, n[i])
        assert FX[p + "z_ratio"][i] == np.float32(sj[n[i]] / abs(zj)) and FX[p + "weight"][i] == np.float32(w[n[i]])


@pytest.mark.parametrize("pid", [q["id"] for q in META["plans"]])
def test_stored_table_value_is_what_the_generator_makes(pid):
    q = next(q for q in META["plans"] if q["id"] == pid)
    p = f"tab/{pid}/"
    s, b, n = FX[p + "s"], FX[p + "b"], FX[p + "n"]
    assert set(zip(s.tolist(), b.tolist())) == {(i, j) for i in range(4) for j in range(3)}
    assert n.max() == q["n_end"] - 1
    for i in (0, len(s) // 2, len(s) - 1):
        k, eta, rho = complex(FX[p + "k"][s[i]]), float(FX[p + "eta"][s[i]]), float(FX[p + "radii"][b[i]])
        k = k.real if k.imag == 0 else k
        t = R.ball_tables(q["d"], q["n_end"], k, eta, rho, complex(FX[p + "alpha"][b[i]]), complex(FX[p + "beta"][b[i]]))
        tn = R.ball_tables(q["d"], q["n_end"], k, eta, rho, FX[p + "alpha_n"][b[i]], FX[p + "beta_n"][b[i]])
        for name, tt in (("gj", t), ("gh", t), ("blc", t), ("gj_n", tn), ("gh_n", tn)):
            v = complex(tt[name[:3].rstrip("_")][n[i]])
            assert FX[p + name][i] == v, (pid, name, i)
            assert FX[p + name + "_ratio"][i] == np.float32(tt[name[:3].rstrip("_") + "_scale"][n[i]] / abs(v))


@pytest.mark.parametrize("cid", [c["id"] for c in META["matrix"]])
def test_stored_matrix_factors_are_what_the_generator_makes(cid):
    c = next(q for q in META["matrix"] if q["id"] == cid)
    cen = np.array(c["centers"])
    n_end = c["n_end"]
    hk, e = R.translation_2d_factors(n_end, c["k"], cen[0] - cen[1])
    for mu in (0, 1, n_end, 2 * n_end - 2):
        assert FX[c["H"]][mu] == complex(hk[mu]) and FX[c["E"]][mu] == complex(e[mu]), (cid, mu)
    t = R.ball_tables(2, n_end, c["k"], 1.0, c["radii"][1], 1.0, 0.0)
    for nm in ("gj", "gh", "blc"):
        assert FX[c["tab"] + "/" + nm][1, n_end - 1] == complex(t[nm][n_end - 1]) and FX[c["tab"] + "/" + nm][1, 0] == complex(t[nm][0])
