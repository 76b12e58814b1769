"""High-precision closed-form right-hand sides, chain harmonics and power sums  --  TEST INFRASTRUCTURE ONLY, CPU only (mpmath).

What ``biem_harmonics`` (chains included), ``biem_rhs_point_source``, ``biem_rhs_plane_wave`` and ``biem_power`` compute, restated in
mpmath on top of ``oracle/mp_field.py`` (harmonics of a, ba, bba, caa; radial functions) - DESIGN.md 5k, 5l, 5g, 5m:

* chain harmonics    Y = prod_j sin^{l_{j+1}} t_j Gbar_{l_j - l_{j+1}}^{(l_{j+1} + (d-j-2)/2)}(cos t_j) e^{i m phi} / sqrt(2 pi), the standard
                     chains "b" * (d - 2) + "a" in the label order of ``Tree.index`` (d = 3, 4: the oracle's ba, bba);
* point source       G_n = -C_d gj_n h_n(k |t|),  f_h = G_{n(h)} conj(Y_h(t^)),  C_d = 2^{(d+1)/2} pi^{(d-1)/2};
* plane wave         f_h = -C_d e^{i k p.c} i^n gj_n conj(Y_h(p^));
* power              P_ext = -(rho^{d-1} / k) sum_h Im[conj(U_h) k c_h h_n'(k rho) + conj(c_h h_n(k rho)) V_h],  c_h = density_h blc_n,
                     P_abs = rho^{d-1} k (k rho)^{2-2d} sum_h Im(alpha_n conj beta_n) |c_h|^2 / |gj_n|^2  (the header of kernels_power.hip).

Inputs enter as the exact values of their fp64 numbers (the gj / blc rows are the fp64 tables the kernels are fed).  Everything runs
at ``mp_radial.digits`` of the radial argument.  ``tests/test_full_order_rhs_host.py`` ties every function to the fp64 yardsticks at
low order; ``tools/make_full_order_rhs_fixtures.py`` uses them at the order ceilings.  No GPU test imports this module.
"""
from __future__ import annotations

from functools import lru_cache

import mpmath as mp

from .full_order_rhs_fixture import CANONICAL, chain_dim, chain_index, labels  # noqa: F401  (one label order for fixture and yardstick)
from .mp_field import _mp, _phase, _powers, harmonics, radial_h
from .mp_radial import digits

def c_d(d: int):
    return mp.mpf(2) ** (mp.mpf(d + 1) / 2) * mp.pi ** (mp.mpf(d - 1) / 2)


def sphere_area(d: int):
    return 2 * mp.pi ** (mp.mpf(d) / 2) / mp.gamma(mp.mpf(d) / 2)


# --------------------------------------------------------------------------------------
# chain harmonics
# --------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _gbar_lam_tables(kmax: int, lam2: int, dps: int):
    """lam = lam2 / 2 (integer or half-integer): p_0 = 1 / sqrt(h_0), h_0 = sqrt(pi) Gamma(lam + 1/2) / Gamma(lam + 1), and a_q of
    x p_{q-1} = a_q p_q + a_{q-1} p_{q-2}."""
    with mp.workdps(dps):
        lam = mp.mpf(lam2) / 2
        h0 = mp.sqrt(mp.pi) * mp.gamma(lam + mp.mpf(1) / 2) / mp.gamma(lam + 1)
        a = [None] + [mp.sqrt(q * (q + 2 * lam - 1) / ((q + lam - 1) * (q + lam))) / 2 for q in range(1, kmax + 1)]
        return 1 / mp.sqrt(h0), a


def _gbar_lam(kmax: int, lam2: int, x):
    """[p_0 .. p_kmax] of the orthonormal Gegenbauer polynomials of parameter lam2 / 2 at x."""
    p0, a = _gbar_lam_tables(kmax, lam2, mp.mp.dps)
    p = [p0]
    if kmax >= 1:
        p.append(x * p0 / a[1])
    for q in range(2, kmax + 1):
        p.append((x * p[q - 1] - a[q - 1] * p[q - 2]) / a[q])
    return p


def chain_angles(d: int, u):
    """(c[d-2], s[d-2], e^{i phi}) of the direction u (mpf list, any length): cos t_j = u_j / |u_{j..}|, sin t_j = |u_{j+1..}| / |u_{j..}|,
    (1, 0) where |u_{j..}| vanishes, and the azimuth of (u_{d-2}, u_{d-1}) with e^{i phi} = 1 where both vanish (atan2(0, 0) = 0)."""
    tail = [mp.mpf(0)] * (d + 1)
    for j in range(d - 1, -1, -1):
        tail[j] = tail[j + 1] + u[j] * u[j]
    c, s = [], []
    for j in range(d - 2):
        rho, rho1 = mp.sqrt(tail[j]), mp.sqrt(tail[j + 1])
        c.append(u[j] / rho if rho != 0 else mp.mpf(1))
        s.append(rho1 / rho if rho != 0 else mp.mpf(0))
    return c, s, _phase(u[d - 2], u[d - 1])


def chain_amplitudes(d: int, n_end: int, u):
    """{(l_0, ..., l_{d-3}, |m|): prod_j node factor / sqrt(2 pi)} (real) and the powers e^{i m phi}, m = 0 .. n_end - 1."""
    c, s, w = chain_angles(d, u)
    nm = max(n_end - 1, 0)
    isq = 1 / mp.sqrt(2 * mp.pi)
    # node j: F[j][L1][L - L1] = sin^{L1} Gbar_{L - L1}^{(L1 + (d-j-2)/2)}(cos)
    F = []
    for j in range(d - 2):
        Fj = []
        for L1 in range(nm + 1):
            g = _gbar_lam(nm - L1, 2 * L1 + (d - j - 2), c[j])
            sl = s[j] ** L1
            Fj.append([sl * v for v in g])
        F.append(Fj)
    amp = {}
    for lab in chain_index(d, n_end):
        key = lab[:-1] + (abs(lab[-1]),)
        if key not in amp:
            v = isq
            for j in range(d - 2):
                v = v * F[j][key[j + 1]][key[j] - key[j + 1]]
            amp[key] = v
    return amp, _powers(w, nm)


def chain_harmonics(d: int, n_end: int, u):
    """Y_h(u) of the standard chain of dimension d >= 3 at the direction u (mpf list, need not be normalised), in the order of
    ``chain_index`` (d = 3, 4: the order of the oracle's ba, bba)."""
    amp, wp = chain_amplitudes(d, n_end, u)
    out = []
    for lab in chain_index(d, n_end):
        m = lab[-1]
        out.append(amp[lab[:-1] + (abs(m),)] * (wp[m] if m >= 0 else mp.conj(wp[-m])))
    return out


def tree_harmonics(tree: str, n_end: int, u):
    """Y_h at the direction u (mpf list, any length) of a canonical tree or a chain d >= 5."""
    if tree in CANONICAL:
        r = mp.sqrt(mp.fsum(v * v for v in u))
        return harmonics(tree, n_end, [v / r for v in u])
    return chain_harmonics(chain_dim(tree), n_end, u)


def azimuth_powers(tree: str, n_end: int, u):
    """The unit phases the labels' signed entries multiply: [e^{i m phi}] (m < n_end) per azimuth of the tree - one list, or two for caa."""
    nm = max(n_end - 1, 0)
    if tree == "caa":
        return [_powers(_phase(u[0], u[1]), nm), _powers(_phase(u[2], u[3]), nm)]
    d = len(u)
    return [_powers(_phase(u[d - 2], u[d - 1]), nm)]


# --------------------------------------------------------------------------------------
# closed-form right-hand sides
# --------------------------------------------------------------------------------------
def point_source_G(d: int, n_end: int, k, tab_gj, dist):
    """[-C_d gj_n h_n(k dist)], n < n_end: k an fp64 number (real or complex), tab_gj the fp64 row the kernel is fed, dist = |t| an mpf
    (the exact distance of the fp64 coordinates).  Also returns [h_n]."""
    with mp.workdps(max(mp.mp.dps, digits(complex(k) * float(dist)))):
        h = radial_h(n_end - 1, d, _mp(k) * dist)
        cd = c_d(d)
        return [-cd * _mp(tab_gj[n]) * h[n] for n in range(n_end)], h


def plane_wave_factor(d: int, k, p, c):
    """-C_d e^{i k p.c}: k, p[d], c[d] fp64 numbers, the product p.c exact."""
    t = mp.fsum(mp.mpf(float(a)) * mp.mpf(float(b)) for a, b in zip(p, c))
    return -c_d(d) * mp.exp(1j * _mp(k) * t)


def power(d: int, n_end: int, k, rho, alpha_n, beta_n, tab, density, pu, pv, deg):
    """(P_ext, P_abs, sum |terms of P_ext| / |P_ext|, sum |terms of P_ext|, sum |terms of P_abs|) of one ball and right-hand side: the
    two sums of the header of kernels_power.hip term by term.  k, rho real fp64; alpha_n, beta_n [n_end] complex fp64; tab [3][n_end]
    the fp64 ball tables (rows gj, gh, blc: 0 and 2 enter); density, pu, pv [H] complex fp64; deg [H].  A degree with
    Im(alpha_n conj beta_n) == 0 contributes an exact 0 to P_abs."""
    with mp.workdps(max(mp.mp.dps, digits(float(k) * float(rho)))):
        kk, rh = mp.mpf(float(k)), mp.mpf(float(rho))
        x = kk * rh
        h = radial_h(n_end, d, x)
        khp = [kk * (n / x * h[n] - h[n + 1]) for n in range(n_end)]
        w = []
        for n in range(n_end):
            a, b = _mp(alpha_n[n]), _mp(beta_n[n])
            wn = mp.im(a * mp.conj(b))
            w.append(wn / abs(_mp(tab[0][n])) ** 2 if wn != 0 else mp.mpf(0))
        te, ta = [], []
        for hh, n in enumerate(deg):
            n = int(n)
            c = _mp(density[hh]) * _mp(tab[2][n])
            te.append(mp.im(mp.conj(_mp(pu[hh])) * c * khp[n]))
            te.append(mp.im(mp.conj(c * h[n]) * _mp(pv[hh])))
            if w[n] != 0:
                ta.append(w[n] * abs(c) ** 2)
        fe, fa = -(rh ** (d - 1) / kk), rh ** (d - 1) * kk * x ** (2 - 2 * d)
        pe, pa = fe * mp.fsum(te), fa * mp.fsum(ta)
        se, sa = abs(fe) * mp.fsum(abs(v) for v in te), abs(fa) * mp.fsum(abs(v) for v in ta)
        return pe, pa, (se / abs(pe) if pe != 0 else mp.inf), se, sa
