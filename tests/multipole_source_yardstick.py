"""NumPy twin of the closed-form right-hand side of multipole incidence (helper module, not a test).

Written against the CPU oracle (`oracle.biem_oracle`: `translation_SR`, `ball_tables`, `radial_h`, a tree's `harmonics` / `degrees` /
`quadrature`).  The outgoing multipole u_in(x) = h_n'(k |x - s|) Y_h'((x - s)^) at s, expanded about the centre c of a ball with
t = c - s and |t| > rho, is row h' of the translation operator,

    u_in(c + r) = sum_h SR[h', h] j_n(k |r|) Y_h(r^),      SR = O.translation_SR(tr, n_end, k, c - s),

so its projections on the sphere are U_h = SR[h', h] j_n(k rho), V_h = SR[h', h] k j_n'(k rho) and the right-hand side is
f = -(alpha U + beta V) = -gj_n SR[h', h].  h' is a position on the harmonic axis of the canonical tree.
"""
import math

import numpy as np
import scipy.special as sp

from oracle import biem_oracle as O


_SR = {}


def translation(tr, n_end, k, t):
    """O.translation_SR(tr, n_end, k, t), kept: a test asks for the same (tree, order, k, displacement) once per coefficient set and layout."""
    key = (tr.name, n_end, complex(k), np.asarray(t, dtype=np.float64).tobytes())
    if key not in _SR:
        if len(_SR) >= 256:
            _SR.clear()
        _SR[key] = O.translation_SR(tr, n_end, k, np.asarray(t, dtype=np.float64))
    return _SR[key]


def outgoing_radial(n, d, z):
    """h_n(z) of O.radial_h on a whole array z, by the SciPy functions it calls point by point (tests/test_multipole_source_host.py
    holds the two together)."""
    z = np.asarray(z)
    if d == 3 and not np.iscomplexobj(z):
        return sp.spherical_jn(n, z) + 1j * sp.spherical_yn(n, z)
    nu = n + d / 2.0 - 1.0
    pref = math.sqrt(math.pi / 2.0) / z ** (d / 2.0 - 1.0)
    if not np.iscomplexobj(z):
        return pref * (sp.jv(nu, z) + 1j * sp.yv(nu, z))
    return pref * sp.hankel1(nu, z)


def multipole_samples(tr, n_end, k, s, hp, x):
    """u_in at the points x [P, d]: the radial function of the degree of h' times the tree's harmonic h'."""
    rel = x - np.asarray(s, dtype=np.float64)[None, :]
    r = np.linalg.norm(rel, axis=-1)
    n = int(tr.degrees(n_end)[hp])
    return outgoing_radial(n, tr.d, k * r) * tr.harmonics(rel / r[:, None], n_end)[hp]


def quadrature_projections(tr, n_end, k, center, rho, s, hp, nq):
    """U[H] of one ball by the tree's nq-point rule applied to the sampled multipole: what the sampled path computes with nq = n_end."""
    y, w = tr.quadrature(nq)
    Yc = np.conj(tr.harmonics(y, n_end))
    x = np.asarray(center)[None, :] + rho * y
    return Yc @ (w * multipole_samples(tr, n_end, k, s, hp, x))


def projections(tr, n_end, k, center, rho, s, hp):
    """(U[H], V[H]) of one ball in closed form."""
    deg = tr.degrees(n_end)
    j, _, jp, _ = O.radial_h(n_end - 1, tr.d, k * rho)
    row = translation(tr, n_end, k, np.asarray(center, dtype=np.float64) - np.asarray(s, dtype=np.float64))[hp]
    return row * j[deg], row * (k * jp)[deg]


def rhs(tr, n_end, k, centers, radii, alpha, beta, s, hp, eta=1.0):
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
        t = np.asarray(centers[b], dtype=np.float64) - np.asarray(s, dtype=np.float64)
        out[b] = -gj[deg] * translation(tr, n_end, k, t)[hp]
    return out


def source_indices(tr, n_end):
    """Positions on the harmonic axis the tests use: (degree 0, degree 1, its conjugate partner or another of degree 1, the top degree)."""
    deg = tr.degrees(n_end)
    u = np.array([[0.36, -0.48, 0.64, 0.48][:tr.d]])
    Y = tr.harmonics(u / np.linalg.norm(u), n_end)[:, 0]
    one = int(np.nonzero(deg == 1)[0][-1])                       # the last of degree 1: a complex harmonic in every tree
    partner = int(np.argmin(np.abs(Y - np.conj(Y[one]))))
    return int(np.nonzero(deg == 0)[0][0]), one, partner, int(np.nonzero(deg == n_end - 1)[0][-1])
