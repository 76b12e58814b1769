"""NumPy yardstick of regular-wave incidence and of the cluster's outgoing coefficients (helper module, not a test).

The regular wave u_in(x) = j_n'(k |x - o|) Y_h'((x - o)^) about an origin o, expanded about a centre c with t = c - o, is row h' of

    u_in(c + r) = sum_h RR[h', h] j_n(k |r|) Y_h(r^),      RR = (R|R)(t),

and RR is the expression of `translation_SR_quadrature` in oracle/biem_oracle.py with the regular radial function in place of the
outgoing one - written here, the oracle is not patched, and none of the library's term lists is used:

    RR[h', h] = C_d conj(i^n') i^n sum_q w_q Y_h'(y_q) conj(Y_h(y_q)) F(y_q),   F(y) = sum_l i^n(l) j_n(l)(k |t|) Y_l(t^) conj(Y_l(y))

over the labels l of degree < 2 n_end - 1, at the oracle's 2 n_end-point rule.  Unlike its h form the sum is well conditioned: the
j_n'' decay with the degree, nothing cancels.  At t = 0 only l = 0 is left, j_0(0) = sqrt(pi/2) 2^{1-d/2} / Gamma(d/2), and the direction
is immaterial.  The chain trees take the closed-form Gaunt lists of tests/chain_yardstick.py with the same regular table.

The same matrix carries the scattered field of a cluster to one outgoing expansion about o: (S|S) = (R|R),
    A_h'' = sum_b sum_h RR(o - c_b)[h, h''] c_{b,h}.
"""
import math

import numpy as np
import scipy.special as sp

from oracle import biem_oracle as O


def regular_radial(nmax, d, z):
    """j_n(z), n = 0 .. nmax, of the project's normalisation sqrt(pi/2) J_{n+d/2-1}(z) / z^{d/2-1}; z real or complex, z = 0 included."""
    n = np.arange(nmax + 1)
    if z == 0:
        out = np.zeros(nmax + 1, dtype=np.complex128)
        out[0] = math.sqrt(math.pi / 2.0) * 2.0 ** (1.0 - d / 2.0) / math.gamma(d / 2.0)
        return out
    if d == 3 and complex(z).imag == 0.0:
        return sp.spherical_jn(n, float(np.real(z))).astype(np.complex128)
    z = complex(z) if complex(z).imag != 0.0 else float(np.real(z))
    return (math.sqrt(math.pi / 2.0) / z ** (d / 2.0 - 1.0) * sp.jv(n + d / 2.0 - 1.0, z)).astype(np.complex128)


def outgoing_radial(nmax, d, z):
    """h_n(z), n = 0 .. nmax (O.radial_h)."""
    return O.radial_h(nmax, d, z)[1]


def _direction(t):
    t = np.asarray(t, dtype=np.float64)
    r = float(np.linalg.norm(t))
    if r == 0.0:
        u = np.zeros_like(t)
        u[0] = 1.0
        return r, u
    return r, t / r


def is_chain(tr):
    return not hasattr(tr, "base") or tr.name not in ("a", "ba", "bba", "caa", "bpa", "bpbpa")


_RR = {}


def translation_rr(tr, n_end, k, t):
    """RR[h', h] = (R|R)_{h'->h}(t) of an oracle tree (a, ba, bpa, bba, bpbpa, caa) or a chain of tests/test_chain_trees_host.py."""
    key = (tr.name, n_end, complex(k), np.asarray(t, dtype=np.float64).tobytes())
    if key in _RR:
        return _RR[key]
    if len(_RR) >= 512:
        _RR.clear()
    r, u = _direction(t)
    d = tr.d
    Cd = (2 * math.pi) ** (d / 2.0) * math.sqrt(2.0 / math.pi)
    jn = regular_radial(2 * n_end - 2, d, k * r)
    if is_chain(tr):
        import chain_yardstick as CY

        g = CY.gaunt(d, n_end)
        T = Cd * jn[g.deg2] * g.ch.harmonics(u[None, :], g.n2)[:, 0]
        out = np.zeros((g.H, g.H), dtype=np.complex128)
        for hp in range(g.H):
            for h in range(g.H):
                lab, cf = g.terms(hp, h)
                out[hp, h] = cf @ T[lab]
    else:
        yq, wq, Yq, Yq2, deg, deg2 = O._sr_tables(tr.name, n_end)
        Yt = tr.harmonics(u[None, :], 2 * n_end - 1)[:, 0]
        F = ((1j ** deg2) * jn[deg2] * Yt) @ np.conj(Yq2)
        ph = 1j ** deg
        A = (Yq * (wq * F)[None, :]) @ np.conj(Yq).T
        out = Cd * (np.conj(ph)[:, None] * A * ph[None, :])
    _RR[key] = out
    return out


def degrees(tr, n_end):
    return np.asarray(tr.degrees(n_end)) if hasattr(tr, "degrees") else np.array([lab[0] for lab in tr.index(n_end)])


def regular_samples(tr, n_end, k, o, hp, x):
    """u_in at the points x [P, d]; a point on the origin is an ordinary one."""
    rel = np.asarray(x, dtype=np.float64) - np.asarray(o, dtype=np.float64)[None, :]
    r = np.linalg.norm(rel, axis=-1)
    n = int(degrees(tr, n_end)[hp])
    u = rel / np.where(r > 0, r, 1.0)[:, None]
    u[r == 0] = np.eye(tr.d)[0]
    rad = np.array([regular_radial(n, tr.d, k * ri)[n] for ri in r])
    return rad * tr.harmonics(u, n_end)[hp]


def outgoing_samples(tr, n_out, k, o, A, x):
    """sum_h'' A_h'' h_n''(k |x - o|) Y_h''((x - o)^) at the points x [P, d]."""
    rel = np.asarray(x, dtype=np.float64) - np.asarray(o, dtype=np.float64)[None, :]
    r = np.linalg.norm(rel, axis=-1)
    deg = degrees(tr, n_out)
    Y = tr.harmonics(rel / r[:, None], n_out)
    rad = np.stack([outgoing_radial(n_out - 1, tr.d, k * ri)[deg] for ri in r], axis=1)      # [H, P]
    return np.einsum("h,hp,hp->p", np.asarray(A), rad, Y)


def _full(v, B, n_end):
    v = np.asarray(v, dtype=np.complex128)
    return np.broadcast_to(v.reshape(v.shape + (1,) * (2 - v.ndim)) if v.ndim else v, (B, n_end))


def rhs(tr, n_end, k, centers, radii, alpha, beta, o, hp, eta=1.0, table_tree=None):
    """f[B, H] = -gj_n RR(c_b - o)[h', h] of one system; alpha / beta scalars, [B] or [B, n_end] (gj of the oracle's ball_tables;
    table_tree: the oracle tree of the same dimension the ball tables are asked of, for a chain)."""
    B = len(radii)
    deg = degrees(tr, n_end)
    an, bn = _full(alpha, B, n_end), _full(beta, B, n_end)
    out = np.zeros((B, len(deg)), dtype=np.complex128)
    for b in range(B):
        gj = ball_gj(tr, n_end, k, radii[b], an[b], bn[b])
        t = np.asarray(centers[b], dtype=np.float64) - np.asarray(o, dtype=np.float64)
        out[b] = -gj[deg] * translation_rr(tr, n_end, k, t)[hp]
    return out


def ball_gj(tr, n_end, k, rho, alpha_n, beta_n):
    """gj_n = alpha_n j_n(k rho) + beta_n k j_n'(k rho), n < n_end."""
    j, _, jp, _ = O.radial_h(n_end - 1, tr.d, k * rho)
    return np.asarray(alpha_n) * j + np.asarray(beta_n) * k * jp


def blc(tr, n_end, k, eta, rho):
    """blc_n = k^{d-2} rho^{d-1} (eta j_n + i k j_n')(k rho): density -> outgoing coefficient of a ball (kernels_uscat.hip)."""
    j, _, jp, _ = O.radial_h(n_end - 1, tr.d, k * rho)
    return k ** (tr.d - 2) * rho ** (tr.d - 1) * (eta * j + 1j * k * jp)


def raised_index(tr, n_end, n_out):
    """Per harmonic of order n_end its position on the axis of order n_out, by label."""
    where = {tuple(lab): i for i, lab in enumerate(tr.index(n_out))}
    return np.array([where[tuple(lab)] for lab in tr.index(n_end)])


def cluster_coefficients(tr, n_end, n_out, k, eta, centers, radii, o, density):
    """A[H_out] of one system and one right-hand side from its density [B, H]."""
    deg = degrees(tr, n_end)
    idx = raised_index(tr, n_end, n_out)
    A = np.zeros(len(tr.index(n_out)), dtype=np.complex128)
    for b in range(len(radii)):
        c = np.asarray(density[b]) * blc(tr, n_end, k, eta, radii[b])[deg]
        t = np.asarray(o, dtype=np.float64) - np.asarray(centers[b], dtype=np.float64)
        A += c @ translation_rr(tr, n_out, k, t)[idx, :]
    return A
