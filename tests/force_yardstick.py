"""NumPy restatement of the time-averaged radiation force on each ball of a solved scattering problem (helper module, not a test).

Written against the CPU oracle like tests/power_yardstick.py, for real k and kind="outer".  In the normalisation of the powers (for a
unit plane wave an area, the radiation-pressure cross section as a vector), with u the total exterior field, S_b any closed surface in
the fluid around ball b alone and n its outward normal:

    Phi_b = -(1 / (2 k^2)) oint_{S_b} [ (k^2 |u|^2 - |grad u|^2) n + 2 Re( grad u conj(d_n u) ) ] dS

On the ball's own surface the traces follow from the outgoing coefficients c = res.coef and the boundary condition alone
(gj_n = alpha_n j_n + beta_n k j_n', Wronskian Wr = i (k rho)^{1-d}):

    s_h = c_h k Wr / gj_n ,   u_h = -beta_n s_h  (u on r = rho) ,   v_h = alpha_n s_h  (d_n u)

and with T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega and lambda_n = n (n + d - 2)

    Phi_{b,i} = -(rho^{d-1} / (2 k^2)) Re sum_{h',h} T^i_{h'h} [ conj(u_h') u_h (k^2 - (lambda_n + lambda_n' - (d-1)) / (2 rho^2))
                                                              + conj(v_h') v_h + (1/rho) (lambda_n - lambda_n' + d - 1) conj(v_h') u_h ]

`surface_force` is the route that shares none of this (the stress tensor from field values alone), `momentum_balance` the third:
sum_b Phi_b = P_ext p^ - int |F(x^)|^2 x^ dOmega for a unit plane wave along p^.
"""
import numpy as np

from oracle import biem_oracle as O

import power_yardstick as PY


def coupling(tree, n_end):
    """T[i, h', h] = int y_i Y_h conj(Y_h') dOmega with the tree's rule of order n_end + 1 (exact: the integrand has degree <= 2 n_end - 1)."""
    y, w = tree.quadrature(n_end + 1)
    Y = tree.harmonics(y, n_end)
    return np.stack([(np.conj(Y) * (w * y[:, i])) @ Y.T for i in range(y.shape[1])])


def surface_traces(res, alpha=1.0, beta=0.0):
    """(u[b, h], v[b, h]): coefficients of u and d_n u on the surface of every ball."""
    tr, n_end, k = res.tree, res.n_end, float(res.k)
    d, deg, B = tr.d, tr.degrees(n_end), len(res.radii)
    an, bn = PY.degree_pair(alpha, beta, B, n_end)
    u = np.zeros((B, len(deg)), dtype=np.complex128)
    v = np.zeros_like(u)
    for b, rho in enumerate(res.radii):
        j, _, jp, _ = O.radial_h(n_end - 1, d, k * rho)
        gj = an[b] * j + bn[b] * k * jp
        s = res.coef[b] * k * 1j * (k * rho) ** (1 - d) / gj[deg]
        u[b], v[b] = -bn[b][deg] * s, an[b][deg] * s
    return u, v


def force(res, alpha=1.0, beta=0.0, T=None):
    """Phi[B, d] of an OracleResult solved with the boundary coefficients alpha, beta (see power_yardstick.degree_pair)."""
    tr, n_end, k = res.tree, res.n_end, float(res.k)
    d, deg = tr.d, tr.degrees(n_end)
    T = coupling(tr, n_end) if T is None else T
    lam = (deg * (deg + d - 2)).astype(np.float64)
    u, v = surface_traces(res, alpha, beta)
    out = np.zeros((len(res.radii), d))
    for b, rho in enumerate(res.radii):
        uu = np.conj(u[b])[:, None] * u[b][None, :] * (k * k - (lam[None, :] + lam[:, None] - (d - 1)) / (2 * rho * rho))
        vv = np.conj(v[b])[:, None] * v[b][None, :]
        vu = np.conj(v[b])[:, None] * u[b][None, :] * (lam[None, :] - lam[:, None] + d - 1) / rho
        out[b] = -(rho ** (d - 1) / (2 * k * k)) * np.real(np.einsum("igh,gh->i", T, uu + vv + vu))
    return out


def surface_force(res, uin, R_factor=1.02, nq=16, step=1e-4, with_scale=False):
    """Phi[B, d] by quadrature of the stress tensor over the spheres of radius R_factor * rho_b with the tree's nq-rule; the gradient
    of the total field uin + uscat by central differences of step `step` along every axis.  with_scale: also S[B] =
    (1 / (2 k^2)) oint (|grad u|^2 + 2 |grad u| |d_n u|) dS, the size of the terms that carry the error of the differences."""
    tr, k = res.tree, float(res.k)
    d = tr.d
    y, w = tr.quadrature(nq)
    total = lambda x: uin(x) + O.uscat(res, x)
    out, scale = np.zeros((len(res.radii), d)), np.zeros(len(res.radii))
    for b, (cb, rho) in enumerate(zip(res.centers, res.radii)):
        R = R_factor * rho
        x = cb[None, :] + R * y
        u = total(x)
        g = np.stack([(total(x + step * e) - total(x - step * e)) / (2 * step) for e in np.eye(d)], axis=-1)       # [Q, d]
        dn = np.sum(g * y, axis=-1)
        dens = (k * k * np.abs(u) ** 2 - np.sum(np.abs(g) ** 2, axis=-1))[:, None] * y + 2 * np.real(g * np.conj(dn)[:, None])
        out[b] = -(R ** (d - 1) / (2 * k * k)) * np.sum(w[:, None] * dens, axis=0)
        g2 = np.sum(np.abs(g) ** 2, axis=-1)
        scale[b] = (R ** (d - 1) / (2 * k * k)) * np.sum(w * (g2 + 2 * np.sqrt(g2) * np.abs(dn)))
    return (out, scale) if with_scale else out


def momentum_balance(res, uin, uin_grad, p, alpha=1.0, beta=0.0, nq=24):
    """P_ext p^ - int |F|^2 x^ dOmega [d]: what sum_b Phi_b is for a unit plane wave along p."""
    ext, _, _ = PY.power(res, uin, uin_grad, alpha, beta)
    y, w = res.tree.quadrature(nq)
    p = np.asarray(p, dtype=np.float64)
    return ext.sum() * p / np.linalg.norm(p) - np.sum((w * np.abs(PY.far_pattern(res, y)) ** 2)[:, None] * y, axis=0)
