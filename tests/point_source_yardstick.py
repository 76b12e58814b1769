"""NumPy twin of the closed-form right-hand side of point-source incidence (helper module, not a test).

Written against the CPU oracle (`oracle.biem_oracle`: `ball_tables`, `radial_h`, a tree's `harmonics` / `degrees`).  With the project's
radial functions z_n = sqrt(pi/2) Z_{n+d/2-1}(x) / x^{d/2-1} and orthonormal harmonics, the monopole u_in(x) = h_0(k |x - s|) has on the
surface of a ball of centre c and radius rho, with t = s - c and |t| > rho, the projections

    U_h = C_d j_n(k rho) h_n(k |t|) conj(Y_h(t^)),    V_h = C_d k j_n'(k rho) h_n(k |t|) conj(Y_h(t^))

of u_in and d_n u_in, C_d = 2^{(d+1)/2} pi^{(d-1)/2}, and the right-hand side is f = -(alpha U + beta V) = -C_d gj_n h_n(k |t|) conj(Y_h(t^)).
"""
import math

import numpy as np
import scipy.special as sp

from oracle import biem_oracle as O


def c_d(d):
    return 2.0 ** ((d + 1) / 2.0) * np.pi ** ((d - 1) / 2.0)


def outgoing(tr, n_end, k, center, s):
    """C_d h_n(k |t|) conj(Y_h(t^)) [H], t = s - center: everything of U, V and f but the ball's radial factor."""
    t = np.asarray(s, dtype=np.float64) - np.asarray(center, dtype=np.float64)
    r = np.linalg.norm(t)
    deg = tr.degrees(n_end)
    Y = tr.harmonics((t / r)[None, :], n_end)[:, 0]
    h = O.radial_h(n_end - 1, tr.d, k * r)[1]
    return c_d(tr.d) * h[deg] * np.conj(Y)


def projections(tr, n_end, k, center, rho, s):
    """(U[H], V[H]) of one ball in closed form."""
    deg = tr.degrees(n_end)
    j, _, jp, _ = O.radial_h(n_end - 1, tr.d, k * rho)
    a = outgoing(tr, n_end, k, center, s)
    return a * j[deg], a * (k * jp)[deg]


def monopole_samples(k, s, x, y):
    """(u_in, d_n u_in) of O.point_source(k, s, 0) at the points x [P, d] with normals y [P, d], by the SciPy functions O.radial_h calls
    but on whole arrays: the oracle's callables loop over the points in Python, 40 us each, which a fine rule in 4-D has 10^5 of.
    tests/test_point_source_host.py holds the two samplers together."""
    s = np.asarray(s, dtype=np.float64)
    d = s.shape[0]
    rel = x - s
    r = np.linalg.norm(rel, axis=-1)
    z = k * r
    if d == 3 and not np.iscomplexobj(z):
        h0, h1 = (sp.spherical_jn(n, z) + 1j * sp.spherical_yn(n, z) for n in (0, 1))
    elif not np.iscomplexobj(z):
        pref = math.sqrt(math.pi / 2.0) / z ** (d / 2.0 - 1.0)
        h0, h1 = (pref * (sp.jv(n + d / 2.0 - 1.0, z) + 1j * sp.yv(n + d / 2.0 - 1.0, z)) for n in (0, 1))
    else:
        pref = math.sqrt(math.pi / 2.0) / z ** (d / 2.0 - 1.0)
        h0, h1 = (pref * sp.hankel1(n + d / 2.0 - 1.0, z) for n in (0, 1))
    return h0, -k * h1 * np.sum(rel * y, axis=-1) / r             # h_0' = -h_1


def quadrature_projections(tr, n_end, k, center, rho, s, nq, vectorised=False):
    """(U[H], V[H]) by the tree's nq-rule: what the sampled path computes with nq = n_end.  The samples are those of the oracle's
    O.point_source(k, s, 0); vectorised: of monopole_samples, the same functions on whole arrays."""
    y, w = tr.quadrature(nq)
    Yc = np.conj(tr.harmonics(y, n_end))
    x = np.asarray(center)[None, :] + rho * y
    if vectorised:
        u, dn = monopole_samples(k, s, x, y)
    else:
        uin, ugr = O.point_source(k, s, 0)
        u, dn = uin(x), np.sum(ugr(x) * y, axis=-1)
    return Yc @ (w * u), Yc @ (w * dn)


def rhs(tr, n_end, k, centers, radii, alpha, beta, s, eta=1.0):
    """f[B, H] of one system; alpha / beta scalars, per ball [B] or per ball and degree [B, n_end] (gj of the oracle's ball_tables)."""
    B = len(radii)
    deg = tr.degrees(n_end)
    def full(v):                                    # scalar, [B] or [B, n_end] -> [B, n_end]
        v = np.asarray(v, dtype=np.complex128)
        return np.broadcast_to(v.reshape(v.shape + (1,) * (2 - v.ndim)) if v.ndim else v, (B, n_end))

    an, bn = full(alpha), full(beta)
    out = np.zeros((B, len(deg)), dtype=np.complex128)
    for b in range(B):
        gj = O.ball_tables(tr, n_end, k, eta, radii[b], an[b], bn[b])[0]
        out[b] = -gj[deg] * outgoing(tr, n_end, k, centers[b], s)
    return out
