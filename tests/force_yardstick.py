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
import math

import numpy as np
from scipy import sparse

from oracle import biem_oracle as O

import power_yardstick as PY


def coupling(tree, n_end):
    """T[i, h', h] = int y_i Y_h conj(Y_h') dOmega with the tree's rule of order n_end + 1 (exact: the integrand has degree <= 2 n_end - 1)."""
    y, w = tree.quadrature(n_end + 1)
    Y = tree.harmonics(y, n_end)
    return np.stack([(np.conj(Y) * (w * y[:, i])) @ Y.T for i in range(y.shape[1])])


def coupling_rows(tree, n_end, rows, chunk=4096):
    """Rows h' in `rows` of `coupling`, T[i, r, h] dense over every column h, by the same rule of order n_end + 1 taken `chunk` points at a
    time: what the orders need at which neither the [H, Q] harmonics nor the [d, H, H] table fits."""
    y, w = tree.quadrature(n_end + 1)
    rows = np.asarray(rows)
    out = np.zeros((y.shape[1], len(rows), tree.n_harm(n_end)), dtype=np.complex128)
    for q in range(0, len(w), chunk):
        Y = tree.harmonics(y[q:q + chunk], n_end)
        for i in range(y.shape[1]):
            out[i] += (np.conj(Y[rows]) * (w[q:q + chunk] * y[q:q + chunk, i])) @ Y.T
    return out


def closed_form_a(n_end):
    """Tree a as CSR [T^0, T^1]: Y_m = e^{i m phi} / sqrt(2 pi), y = (cos phi, sin phi), so T^0_{m +- 1, m} = 1/2, T^1_{m + 1, m} = -i/2,
    T^1_{m - 1, m} = +i/2.  Shares nothing with a rule or with evaluated harmonics."""
    idx = [t[0] for t in O.tree("a").index(n_end)]
    pos = {m: h for h, m in enumerate(idx)}
    r, c, v0, v1 = [], [], [], []
    for m, h in pos.items():
        for s in (1, -1):
            if m + s in pos:
                r.append(pos[m + s]), c.append(h), v0.append(0.5), v1.append(-0.5j * s)
    H = len(idx)
    return [sparse.csr_matrix((np.array(v, dtype=np.complex128), (r, c)), shape=(H, H)) for v in (v0, v1)]


def closed_form_ba(n_end):
    """Tree ba as CSR [T^0, T^1, T^2]: Y_lm = Pbar_l^|m|(y_0) e^{i m phi} / sqrt(2 pi) without the Condon-Shortley phase (every Pbar has
    a positive leading coefficient), phi the angle of (y_1, y_2).  The textbook recurrences, A = sqrt(((l+1)^2 - m^2) / ((2l+1)(2l+3))):

        y_0 Y_lm                   = A(l, m) Y_{l+1,m} + A(l-1, m) Y_{l-1,m}
        sin(t) e^{+i phi} Y_lm     = s [ sqrt((l+m+1)(l+m+2) / ((2l+1)(2l+3))) Y_{l+1,m+1} - sqrt((l-m)(l-m-1) / ((2l-1)(2l+1))) Y_{l-1,m+1} ]
        sin(t) e^{-i phi} Y_lm     = s'[ sqrt((l-m+1)(l-m+2) / ((2l+1)(2l+3))) Y_{l+1,m-1} - sqrt((l+m)(l+m-1) / ((2l-1)(2l+1))) Y_{l-1,m-1} ]

    s = +1 for m >= 0 and -1 below, s' = -1 for m >= 1 and +1 below: the signs the phase (-1)^m of the m >= 0 harmonics, which these
    harmonics do not carry, leaves behind.  y_1 = sin(t) cos(phi), y_2 = sin(t) sin(phi)."""
    pos = {lm: h for h, lm in enumerate(O.tree("ba").index(n_end))}
    ent = [{}, {}, {}]

    def put(i, to, frm, v):
        if to in pos and v != 0:
            ent[i][pos[to], pos[frm]] = v

    for (l, m) in pos:
        put(0, (l + 1, m), (l, m), math.sqrt(((l + 1) ** 2 - m * m) / ((2 * l + 1) * (2 * l + 3))))
        if l:
            put(0, (l - 1, m), (l, m), math.sqrt((l * l - m * m) / ((2 * l - 1) * (2 * l + 1))))
        s = 1.0 if m >= 0 else -1.0
        s_ = -1.0 if m >= 1 else 1.0
        up, dn = (2 * l + 1) * (2 * l + 3), (2 * l - 1) * (2 * l + 1)
        plus = (((l + 1, m + 1), s * math.sqrt((l + m + 1) * (l + m + 2) / up)), ((l - 1, m + 1), -s * math.sqrt((l - m) * (l - m - 1) / dn) if l else 0.0))
        minus = (((l + 1, m - 1), s_ * math.sqrt((l - m + 1) * (l - m + 2) / up)), ((l - 1, m - 1), -s_ * math.sqrt((l + m) * (l + m - 1) / dn) if l else 0.0))
        for to, e in plus:                                 # y_1 = (e+ + e-) / 2, y_2 = (e+ - e-) / (2 i)
            put(1, to, (l, m), 0.5 * e), put(2, to, (l, m), -0.5j * e)
        for to, e in minus:
            put(1, to, (l, m), 0.5 * e), put(2, to, (l, m), 0.5j * e)
    H = len(pos)
    return [sparse.csr_matrix((np.array(list(e.values()), dtype=np.complex128), tuple(np.array(list(e.keys())).T)), shape=(H, H)) for e in ent]


CLOSED = {"a": closed_form_a, "ba": closed_form_ba}


def independent_table(name, n_end, cut=1e-12):
    """[T^i as CSR [H, H]] in the caller's axes of tree `name`, from nothing the plan computes: the closed forms (a, ba), otherwise
    `coupling` with its rounding residue removed (measured at most 7.2e-15, the smallest entry of these orders 3e-4: `cut` is far
    from both).  bpa / bpbpa: the base tree's table with the components in the caller's order (canonical y_i = x_{perm[i]})."""
    tr = O.tree(name)
    base = tr.base or name
    T = CLOSED[base](n_end) if base in CLOSED else [sparse.csr_matrix(np.where(np.abs(M) > cut, M, 0.0)) for M in coupling(O.tree(base), n_end)]
    if not tr.base:
        return T
    out = [None] * tr.d
    for i, pi in enumerate(tr.perm):
        out[pi] = T[i]
    return out


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
    if not isinstance(T, np.ndarray):                    # a list of sparse [H, H] matrices: the same sum over the stored entries alone
        for b, rho in enumerate(res.radii):
            for i, Ti in enumerate(T):
                M = Ti.tocoo()
                g, h = M.row, M.col
                br = (np.conj(u[b][g]) * u[b][h] * (k * k - (lam[h] + lam[g] - (d - 1)) / (2 * rho * rho)) + np.conj(v[b][g]) * v[b][h]
                      + np.conj(v[b][g]) * u[b][h] * (lam[h] - lam[g] + d - 1) / rho)
                out[b, i] = -(rho ** (d - 1) / (2 * k * k)) * np.real(np.sum(M.data * br))
        return out
    for b, rho in enumerate(res.radii):
        uu =np.conj(u[b])[:, None] * u[b][None, :] * (k * k - (lam[None, :] + lam[:, None] - (d - 1)) / (2 * rho * rho))
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
