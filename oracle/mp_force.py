"""High-precision evaluation of the radiation force  --  TEST INFRASTRUCTURE ONLY, CPU only (mpmath).

A restatement at ``mp_field.DPS`` digits of the sum ``k_force`` evaluates (tests/force_yardstick.py states it in fp64): with
c_h = density_h blc_n(rho), gj_n = alpha_n j_n(k rho) + beta_n k j_n'(k rho) and Wr = i (k rho)^{1-d},

    u_h = -beta_n c_h k Wr / gj_n ,   v_h = alpha_n c_h k Wr / gj_n ,   lambda_n = n (n + d - 2)
    Phi_i = -(rho^{d-1} / (2 k^2)) Re sum_{h',h} T^i_{h'h} [ conj(u_h') u_h (k^2 - (lambda_n + lambda_n' - (d-1)) / (2 rho^2))
                                                             + conj(v_h') v_h + (1/rho) (lambda_n - lambda_n' + d - 1) conj(v_h') u_h ]

The radial functions are those of ``mp_field``; the table T is handed in (sparse, per component, in the caller's axes) and is never
the plan's: ``tests/force_yardstick.py::independent_table``.  Wavenumber, radii, boundary pairs and densities enter as the exact
values of their fp64 numbers.  ``tools/make_full_order_hess_force_fixtures.py`` uses this at the order ceilings;
``tests/test_full_order_hess_force_host.py`` ties it to the fp64 yardstick at low order.  No GPU test imports it.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

from . import biem_oracle as O
from . import mp_field as M


def factors(tree: str, n_end: int, k: float, eta: float, radii, alpha_n, beta_n):
    """Per ball (sU[n], sV[n]) = (-beta_n, alpha_n) blc_n k Wr / gj_n for n < n_end; alpha_n, beta_n [B, n_end] complex128."""
    tr = O.tree(tree)
    d, B = tr.d, len(radii)
    F = M.MPField(tree, n_end, k, eta, np.zeros((B, d)), radii, np.zeros((B, tr.n_harm(n_end))), "outer")
    out = []
    with mp.workdps(M.DPS):
        for b in range(B):
            x = F.k * F.rho[b]
            j, jp = M._with_derivative(M.radial_j(n_end, d, x), x)
            blc = F.blc(b, False)
            kwr = F.k * mp.mpc(0, 1) * x ** (1 - d)
            sU, sV = [], []
            for n in range(n_end):
                a, be = M._mp(alpha_n[b, n]), M._mp(beta_n[b, n])
                f = blc[n] * kwr / (a * j[n] + be * F.k * jp[n])
                sU.append(-be * f), sV.append(a * f)
            out.append((sU, sV))
    return out


def force(tree: str, n_end: int, k: float, radii, fac, density, table, skip=(), components=None):
    """(Phi[B, d], cond[B]): the double sum over the stored entries of `table` (one sparse [H, H] matrix per component), and
    cond = |sum |terms||_2 / |Phi_b|_2 with every product of the bracket a term of its own.  Balls in `skip` and components outside
    `components` stay NaN (cond then covers the computed components)."""
    tr = O.tree(tree)
    d = tr.d
    deg = [int(n) for n in tr.degrees(n_end)]
    lam = [n * (n + d - 2) for n in deg]
    B = len(radii)
    phi, cond = np.full((B, d), np.nan), np.full(B, np.nan)
    comps = list(range(d)) if components is None else list(components)
    coo = {i: table[i].tocoo() for i in comps}
    with mp.workdps(M.DPS):
        kk = mp.mpf(float(k))
        for b in range(B):
            if b in skip:
                continue
            rho = mp.mpf(float(radii[b]))
            sU, sV = fac[b]
            dn = [mp.mpc(float(z.real), float(z.imag)) for z in density[b]]
            u = [dn[h] * sU[deg[h]] for h in range(len(deg))]
            v = [dn[h] * sV[deg[h]] for h in range(len(deg))]
            pref = rho ** (d - 1) / (2 * kk * kk)
            tot, tabs = [], []
            for i in comps:
                Ti = coo[i]
                s, a = mp.mpf(0), mp.mpf(0)
                for g, h, t in zip(Ti.row.tolist(), Ti.col.tolist(), Ti.data.tolist()):
                    tm = mp.mpc(t.real, t.imag)
                    ug, vg = mp.conj(u[g]), mp.conj(v[g])
                    p1 = ug * u[h] * (kk * kk - (lam[h] + lam[g] - (d - 1)) / (2 * rho * rho))
                    p2 = vg * v[h]
                    p3 = vg * u[h] * (lam[h] - lam[g] + d - 1) / rho
                    s += mp.re(tm * (p1 + p2 + p3))
                    a += abs(tm) * (abs(p1) + abs(p2) + abs(p3))
                tot.append(-pref * s), tabs.append(pref * a)
            phi[b, comps] = [float(t) for t in tot]
            cond[b] = float(mp.sqrt(mp.fsum(t * t for t in tabs)) / mp.sqrt(mp.fsum(t * t for t in tot)))
    return phi, cond
