"""Reader and checker of ``tests/golden/full_order_rhs*.npz``  --  TEST INFRASTRUCTURE ONLY (NumPy; no mpmath, no GPU).

The fixtures pin ``biem_harmonics``, ``biem_rhs_point_source``, ``biem_rhs_plane_wave`` and ``biem_power`` at the order ceilings against
values computed at 40 digits by ``oracle.mp_rhs`` (written by ``tools/make_full_order_rhs_fixtures.py``, read by
``tests/test_gpu_full_order_rhs.py`` and ``tests/test_full_order_rhs_host.py``).

A right-hand side of ba 48 has 2304 entries per (system, source, ball), so FACTORS are stored, each rounded from 40 digits, and
multiplied here:  Y_h = amp[sign-free label of h] e1[|m|]^(+-) (e2[|m2|]^(+-)),  f = G_n conj(Y_h)  (point source),
f = pf i^n gj_n conj(Y_h)  (plane wave).  The products run in extended precision where NumPy has it, so the assembled value is within
4 * 2^-52 of the rounded 40-digit one (at most four stored factors, half an ulp each, and the final rounding); the bound adds that.

The power inputs (density, pu, pv) are rebuilt exactly from integers: (p + i q) / 16 with p, q in 1 .. 15 from a modular formula, times
a stored power of two and a stored power of i per ball and degree.
"""
from __future__ import annotations

import json
import math
import os
import types

import numpy as np

from . import biem_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
PATHS = (os.path.join(GOLDEN, "full_order_rhs_a.npz"), os.path.join(GOLDEN, "full_order_rhs.npz"))
EPS = 2.0 ** -52
CAP = 1e-10                 # the parity contract of BASELINE.md: a cap, not a measurement
ASSEMBLY = 4.0 * EPS        # the assembled expectation against the rounded 40-digit value
CANONICAL = ("a", "ba", "bba", "caa")
CHAIN_CEILINGS = {"bbba": 8, "bbbba": 5, "bbbbbbbba": 3}      # tests/test_force_table_full_order_host.py
WIDE_GROUPS, WIDE_AZIMUTHS, WIDE_NRHS = 7, 10, 70
ROT = np.array([1.0, 1.0j, -1.0, -1.0j])
# One constant per group of tests/test_gpu_full_order_rhs.py: 8 x the largest ratio error / (2^-52 weight scale) measured on an MI355X,
# rounded up to a power of two.  The planted-fault test of tests/test_full_order_rhs_host.py judges with the same.
MEASURED = {"harmonics": 8.99, "point_source": 6.90, "plane_wave": 5.84, "power": 2.90}
C = {"harmonics": 128.0, "point_source": 64.0, "plane_wave": 64.0, "power": 32.0}


# --------------------------------------------------------------------------------------
# labels
# --------------------------------------------------------------------------------------
def chain_dim(tree: str) -> int:
    """d of a standard chain "b" * (d - 2) + "a" (d >= 3), else 0."""
    return len(tree) + 1 if len(tree) >= 2 and tree == "b" * (len(tree) - 1) + "a" else 0


def tree_dim(tree: str) -> int:
    return {"a": 2, "ba": 3, "bba": 4, "caa": 4}.get(tree) or chain_dim(tree)


def chain_index(d: int, n_end: int):
    """Labels (l_0 = n, l_1, ..., l_{d-3}, m) of the chain of dimension d, l_0 >= l_1 >= ... >= |m|, in the order of ``Tree.index``."""
    out = []

    def rec(prefix, j, up):
        if j == d - 2:
            out.extend(tuple(prefix) + (m,) for m in range(-up, up + 1))
            return
        for l in range(up + 1):
            rec(prefix + [l], j + 1, l)

    for n in range(n_end):
        rec([n], 1, n)
    return out


def labels(tree: str, n_end: int):
    """Label tuples of a canonical tree (a, ba, bba, caa) or a standard chain d >= 5, in the plan's order."""
    if tree in CANONICAL:
        return [tuple(int(v) for v in lab) for lab in O.tree(tree).index(n_end)]
    d = chain_dim(tree)
    if d < 5:
        raise NotImplementedError(tree)
    return chain_index(d, n_end)


def structure(tree: str, n_end: int):
    """How a harmonic is put together from the stored factors: labels [H, w], deg [H], aidx [H] (index of the sign-free label among the
    ``keys``), m [H, A] the signed azimuthal entries (A = 2 for caa, else 1), ynorm [n_end] = sqrt(N(d, n) / |S^{d-1}|)."""
    lab = labels(tree, n_end)
    d = tree_dim(tree)
    naz = 2 if tree == "caa" else 1
    deg = np.array([abs(l[0]) for l in lab], dtype=np.int64)        # (tree a: the label is m and the degree |m|)
    keys, aidx = {}, []
    for l in lab:
        key = () if tree == "a" else tuple(l[:len(l) - naz]) + tuple(abs(v) for v in l[len(l) - naz:])   # (a: one amplitude, 1 / sqrt(2 pi))
        aidx.append(keys.setdefault(key, len(keys)))
    m = np.array([l[len(l) - naz:] for l in lab], dtype=np.int64).reshape(len(lab), naz)
    count = np.bincount(deg, minlength=n_end).astype(np.float64)
    area = 2.0 * math.pi ** (d / 2.0) / math.gamma(d / 2.0)
    return types.SimpleNamespace(tree=tree, n_end=n_end, d=d, labels=np.array(lab, dtype=np.int64).reshape(len(lab), -1), deg=deg,
                                 aidx=np.array(aidx), m=m, keys=list(keys), H=len(lab), ynorm=np.sqrt(count / area))


WORK = np.clongdouble if np.finfo(np.longdouble).nmant >= 63 else np.complex128


def harmonics_from_factors(st, amp, es):
    """Y [P, H] in the working precision from amp [P, U] (real) and the unit phases es = [e1 [P, n_end] (, e2)]."""
    Y = amp[:, st.aidx].astype(WORK)
    for a, e in enumerate(es):
        m = st.m[:, a]
        ph = e[:, np.abs(m)].astype(WORK)
        Y = Y * np.where(m[None, :] >= 0, ph, np.conj(ph))
    return Y


def i_pow(n):
    return ROT[np.asarray(n) & 3]


# --------------------------------------------------------------------------------------
# inputs rebuilt from integers
# --------------------------------------------------------------------------------------
def dyadic(H: int, seed: int) -> np.ndarray:
    """(p + i q) / 16, p, q in 1 .. 15: [H] complex128 in the open first quadrant, exact."""
    h = np.arange(H, dtype=np.int64)
    p = (h * 7919 + seed * 104729 + 12345) % 15 + 1
    q = (h * 6271 + seed * 15485863 + 777) % 15 + 1
    return (p + 1j * q) / 16.0


def scaled(z: np.ndarray, exp2: np.ndarray, rot: np.ndarray) -> np.ndarray:
    """z 2^exp2 i^rot, exactly: ldexp on either part, then a swap and a negation."""
    z = np.ldexp(z.real, exp2) + 1j * np.ldexp(z.imag, exp2)
    r = np.asarray(rot) & 3
    re = np.where(r == 0, z.real, np.where(r == 1, -z.imag, np.where(r == 2, -z.real, z.imag)))
    im = np.where(r == 0, z.imag, np.where(r == 1, z.real, np.where(r == 2, -z.imag, -z.real)))
    return re + 1j * im


POWER_NRHS = 2


def power_inputs(deg: np.ndarray, exps: np.ndarray):
    """(density, pu, pv) [POWER_NRHS, B, H] from exps [B, 4, n_end] int: rows (exponent of the density, its power of i, exponent of pv,
    its power of i); pu is the plain dyadic table."""
    B, H = exps.shape[0], len(deg)
    out = [np.zeros((POWER_NRHS, B, H), dtype=np.complex128) for _ in range(3)]
    for r in range(POWER_NRHS):
        for b in range(B):
            s = 3 * (r * B + b)
            out[0][r, b] = scaled(dyadic(H, s), exps[b, 0][deg], exps[b, 1][deg])
            out[1][r, b] = dyadic(H, s + 1)
            out[2][r, b] = scaled(dyadic(H, s + 2), exps[b, 2][deg], exps[b, 3][deg])
    return out


def degree_pair(alpha, beta, n_end: int):
    """The per-degree pair of the biem_power_n cases, [B, n_end] each: alpha_n = alpha (1 + (n % 5) / 8), beta_n = beta (1 - (n % 3) / 4)
    (real factors: a lossless ball stays lossless in every degree)."""
    n = np.arange(n_end)
    a = np.asarray(alpha, dtype=np.complex128)[:, None] * (1.0 + (n % 5) / 8.0)[None, :]
    b = np.asarray(beta, dtype=np.complex128)[:, None] * (1.0 - (n % 3) / 4.0)[None, :]
    return a, b


# --------------------------------------------------------------------------------------
# the reader
# --------------------------------------------------------------------------------------
def load(paths=PATHS) -> dict:
    """{case id: record}.  Kinds of record (``rec.kind``):

    "main"  tree, n_end, d, B, nb; k [nb]; centers [B, d]; radii [2] (the first B are the case's balls, both are the power's); src [5, d];
            dirs [5, d]; gj [nb, B, n_end]; hdirs [P, d] (the t = src - center, index r B + b, then dirs); amp [P, U], es [1 or 2][P, n_end];
            G [nb, 5, B, n_end]; pf [nb, 5, B]; the power case: palpha, pbeta [2], ptab [2, 3, n_end], pexps [2, 4, n_end], pwant,
            pscale [POWER_NRHS, 2, 2], pcond [POWER_NRHS, 2] and, on a and ba, ptab_n, pwant_n, pscale_n, pcond_n of ``degree_pair``;
    "wide"  70 sources around ball 0 of the main case of the tree, system 0: src [70, d]; G [7, n_end], amp [7, U] by group r % 7;
            es [1][10, n_end] by azimuth r % 10;
    "edge"  tree a, n_end 150, k rho = 1.3: k [1], centers [1, 2], radii [1], src [3, 2], gj [1, 1, n_end], G [1, 3, 1, n_end], hdirs, amp, es.
    Every record has ``st`` (``structure``)."""
    out = {}
    for path in paths:
        with np.load(path, allow_pickle=False) as z:
            for cid in json.loads(str(z["cases"])):
                rec = types.SimpleNamespace(id=cid, **json.loads(str(z[cid + "/meta"])))
                for key in z.files:
                    if key.startswith(cid + "/") and key != cid + "/meta":
                        setattr(rec, key[len(cid) + 1:], z[key])
                rec.es = [rec.e1] + ([rec.e2] if hasattr(rec, "e2") else [])
                rec.st = structure(rec.tree, rec.n_end)
                out[cid] = rec
    return out


# --------------------------------------------------------------------------------------
# expectations from the stored factors
# --------------------------------------------------------------------------------------
def expected_harmonics(rec):
    """(Y [P, H], scale [P, H], weight [P, H]) at rec.hdirs."""
    st = rec.st
    Y = harmonics_from_factors(st, rec.amp, rec.es).astype(np.complex128)
    return Y, np.broadcast_to(st.ynorm[st.deg], Y.shape), np.broadcast_to(st.deg + 1.0, Y.shape)


def _dist(rec):
    """|t| [nrhs, B] in fp64 (a weight only)."""
    return np.linalg.norm(rec.src[:, None, :] - rec.centers[None, :rec.B, :], axis=-1)


def expected_point_source(rec):
    """(f, scale, weight) [nb, nrhs, B, H] of a main or edge record: f = G_n conj(Y_h(t^)), scale = |G_n| sqrt(N(d, n) / |S^{d-1}|),
    weight = max(n + 1, |k| |t|)."""
    st, B, nrhs = rec.st, rec.B, len(rec.src)
    Y = harmonics_from_factors(st, rec.amp[:nrhs * B], [e[:nrhs * B] for e in rec.es]).reshape(nrhs, B, st.H)
    f = (rec.G[..., st.deg].astype(WORK) * np.conj(Y)[None]).astype(np.complex128)
    scale = np.abs(rec.G)[..., st.deg] * st.ynorm[st.deg]
    weight = np.maximum(st.deg + 1.0, (np.abs(rec.k)[:, None, None] * _dist(rec)[None])[..., None])
    return f, scale, np.broadcast_to(weight, f.shape)


def expected_wide(rec, main):
    """(f, scale, weight) [1, 70, 1, H] of a wide record: source r has the radial row and the amplitudes of group r % 7 and the phases of
    azimuth r % 10."""
    st = rec.st
    r = np.arange(WIDE_NRHS)
    g, a = r % WIDE_GROUPS, r % WIDE_AZIMUTHS
    Y = harmonics_from_factors(st, rec.amp[g], [e[a] for e in rec.es])
    G = rec.G[g]
    f = (G[:, st.deg].astype(WORK) * np.conj(Y)).astype(np.complex128)
    scale = np.abs(G)[:, st.deg] * st.ynorm[st.deg]
    dist = np.linalg.norm(rec.src - main.centers[0], axis=-1)
    weight = np.maximum(st.deg + 1.0, abs(main.k[0]) * dist[:, None])
    return f[None, :, None, :], scale[None, :, None, :], weight[None, :, None, :]


def expected_plane_wave(rec):
    """(f, scale, weight) [nb, 5, B, H]: f = pf i^n gj_n conj(Y_h(p^)), scale = |pf| |gj_n| sqrt(N / |S|), weight = max(n + 1, |k| |c|)."""
    st, B = rec.st, rec.B
    nd = len(rec.dirs)
    Y = harmonics_from_factors(st, rec.amp[-nd:], [e[-nd:] for e in rec.es])                     # [5, H]
    rad = (rec.gj[..., st.deg] * i_pow(st.deg)).astype(WORK)                                     # [nb, B, H]  (i^n: exact)
    f = (rec.pf.astype(WORK)[..., None] * rad[:, None] * np.conj(Y)[None, :, None, :]).astype(np.complex128)
    scale = np.abs(rec.pf)[..., None] * (np.abs(rec.gj)[..., st.deg] * st.ynorm[st.deg])[:, None]
    kc = np.abs(rec.k)[:, None] * np.linalg.norm(rec.centers[:B], axis=-1)[None, :]              # [nb, B]
    weight = np.maximum(st.deg + 1.0, kc[:, None, :, None])
    return f, scale, np.broadcast_to(weight, f.shape)


# --------------------------------------------------------------------------------------
# the checker
# --------------------------------------------------------------------------------------
def ratios(got, want, scale, weight):
    """|got - want| / (2^-52 weight scale); inf where got is not finite."""
    got = np.asarray(got)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / (EPS * weight * scale))
    return np.where(np.isfinite(got), r, np.inf)


def within(got, want, scale, weight, C):
    """|got - want| <= (min(C 2^-52 weight, 1e-10) + 4 2^-52) scale, entry by entry; a non-finite entry fails."""
    got = np.asarray(got)
    ok = np.abs(got - want) <= (np.minimum(C * EPS * weight, CAP) + ASSEMBLY) * scale
    return ok & np.isfinite(got)


def worst(got, want, scale, weight):
    """(largest ratio, its index)."""
    r = ratios(got, want, scale, weight)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i)
