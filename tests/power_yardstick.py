"""NumPy restatement of the integrated quantities of a solved scattering problem (helper module, not a test).

Written against the CPU oracle (`oracle.biem_oracle`: `radial_h`, a tree's `quadrature` / `harmonics` / `degrees`, `res.coef`), for real k
and the reference's far-field normalisation u_scat ~ F(x^) e^{ikr} / r^{(d-1)/2}; "power" is (1/k) Im oint conj(u) d_n u dS, the
cross section of a unit plane wave.  With c = res.coef (outgoing coefficients), U, V the projections of u_in and d_n u_in on the
surface of ball b onto Y_h, and the Wronskian j y' - y j' = x^{1-d} of the project's radial functions:

    P_ext,b = -(rho^{d-1} / k) sum_h Im[ conj(U_h) k c_h h_n'(k rho) + conj(c_h h_n(k rho)) V_h ]
    P_abs,b = rho^{d-1} k (k rho)^{2-2d} sum_h Im(alpha_n conj beta_n) |c_h|^2 / |gj_n|^2 ,   gj_n = alpha_n j_n + beta_n k j_n'
    F(x^)   = (ik)^{-(d-1)/2} sum_b e^{-ik x^.c_b} sum_h c_{b,h} (-i)^n Y_h(x^)

`flux` is the route that shares none of this: the quadrature of (1/k) Im[conj(u) d_r u] over a large sphere from field values alone.
"""
import numpy as np

from oracle import biem_oracle as O


def degree_pair(alpha, beta, B, n_end):
    """alpha / beta (scalars, per ball [B], or per ball and degree [B, n_end]) as [B, n_end] complex arrays."""
    def full(v):
        v = np.asarray(v, dtype=np.complex128)
        if v.ndim <= 1:
            v = np.broadcast_to(v, (B,))[:, None]
        return np.broadcast_to(v, (B, n_end))
    return full(alpha), full(beta)


def projections(res, uin, uin_grad):
    """U[b, h], V[b, h]: sum_q w_q f(c_b + rho_b y_q) conj(Y_h(y_q)) of f = u_in and f = y . grad u_in (the oracle's plane_wave /
    point_source callables, x[..., d])."""
    tr, n_end = res.tree, res.n_end
    yq, wq = tr.quadrature(n_end)
    Yc = np.conj(tr.harmonics(yq, n_end))
    U = np.zeros((len(res.radii), Yc.shape[0]), dtype=np.complex128)
    V = np.zeros_like(U)
    for b, (cb, rho) in enumerate(zip(res.centers, res.radii)):
        x = cb[None, :] + rho * yq
        U[b] = Yc @ (wq * uin(x))
        V[b] = Yc @ (wq * np.sum(uin_grad(x) * yq, axis=-1))
    return U, V


def power(res, uin, uin_grad, alpha=1.0, beta=0.0):
    """(P_ext[B], P_abs[B], P_sca) of an OracleResult solved with the boundary coefficients alpha, beta (see degree_pair)."""
    tr, n_end, k = res.tree, res.n_end, float(res.k)
    d, deg, B = tr.d, tr.degrees(n_end), len(res.radii)
    an, bn = degree_pair(alpha, beta, B, n_end)
    U, V = projections(res, uin, uin_grad)
    ext, ab = np.zeros(B), np.zeros(B)
    for b, rho in enumerate(res.radii):
        j, h, jp, hp = O.radial_h(n_end - 1, d, k * rho)
        c = res.coef[b]
        ext[b] = -(rho ** (d - 1) / k) * np.sum(np.imag(np.conj(U[b]) * k * c * hp[deg] + np.conj(c * h[deg]) * V[b]))
        w = np.imag(an[b] * np.conj(bn[b]))
        lossy = w != 0
        gj = an[b] * j + bn[b] * k * jp
        per_degree = np.zeros(n_end)
        per_degree[lossy] = w[lossy] / np.abs(gj[lossy]) ** 2
        ab[b] = rho ** (d - 1) * k * (k * rho) ** (2 - 2 * d) * np.sum(per_degree[deg] * np.abs(c) ** 2)
    return ext, ab, float(ext.sum() - ab.sum())


def far_pattern(res, directions, per_ball=False):
    """F at unit vectors directions[P, d]: [P], or [P, B] per ball."""
    tr, n_end, k = res.tree, res.n_end, res.k
    d, deg = tr.d, tr.degrees(n_end)
    xh = np.asarray(directions, dtype=np.float64)
    Y = tr.harmonics(xh, n_end)
    out = np.stack([np.exp(-1j * k * (xh @ cb)) * ((res.coef[b] * (-1j) ** deg) @ Y) for b, cb in enumerate(res.centers)], axis=-1)
    out = out / (1j * k) ** ((d - 1) / 2.0)
    return out if per_ball else out.sum(axis=-1)


def pattern_power(res, nq):
    """int |F|^2 dOmega with the tree's nq-rule."""
    y, w = res.tree.quadrature(nq)
    return float(np.sum(w * np.abs(far_pattern(res, y)) ** 2))


def optical_theorem(res, direction):
    """2 (2 pi / k)^{(d-1)/2} Im[ e^{i pi (d-3)/4} F(p^) ]: the extinction of a unit plane wave along p^."""
    d, k = res.tree.d, float(res.k)
    p = np.asarray(direction, dtype=np.float64)
    F = far_pattern(res, (p / np.linalg.norm(p))[None, :])[0]
    return float(2.0 * (2.0 * np.pi / k) ** ((d - 1) / 2.0) * np.imag(np.exp(1j * np.pi * (d - 3) / 4.0) * F))


def flux(k, R, y, w, u, du_r):
    """(1/k) sum_q w_q R^{d-1} Im[conj(u_q) (d_r u)_q] over the sphere of radius R sampled at R y_q (y[Q, d] unit vectors)."""
    d = y.shape[1]
    return float(np.sum(w * R ** (d - 1) * np.imag(np.conj(u) * du_r)) / k)


def oracle_flux(res, R, nq, step=1e-4):
    """flux of the oracle's near field through |x| = R, the radial derivative by a central difference of step `step`."""
    y, w = res.tree.quadrature(nq)
    u = O.uscat(res, R * y)
    du = (O.uscat(res, (R + step) * y) - O.uscat(res, (R - step) * y)) / (2 * step)
    return flux(float(res.k), R, y, w, u, du)
