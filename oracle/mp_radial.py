"""High-precision radial functions, per-ball tables and the 2-D translation entry  --  TEST INFRASTRUCTURE ONLY, CPU only (mpmath).

The layer below ``oracle/mp_field.py``: what ``radial_jh`` (csrc/special.hpp), ``k_ball_tables`` (csrc/kernels_tables.hip, scalar and per-degree coefficients) and the 2-D pair
tables compute, restated in mpmath.  Inputs enter as the exact values of their fp64 numbers.

* radial functions  z_n^{(d)}(z) = sqrt(pi/2) J_{n+d/2-1}(z) / z^{d/2-1}  and  h_n^{(d)}  likewise with hankel1, d = 2 .. 10;
* ball tables       gj = alpha_n z_n + beta_n k z_n',  gh = alpha_n h_n + beta_n k h_n',  blc = k^{d-2} rho^{d-1} (eta z_n + i k z_n')
                    as ``biem_oracle.ball_tables`` states them (alpha, beta scalars or one value per degree);
* 2-D translation   SR[m', m] = i^{|m| + |mu| - |m'|} H_{|mu|}(k |t|) e^{i mu phi},  mu = m' - m  (``translation_SR_2d_graf``), with
                    e^{i phi} = (t_x + i t_y) / |t| from the exact coordinates.

PRECISION.  ``mpmath.hankel1`` is j + i y, which cancels by e^{2 Im z} for Im z > 0, and the upward recurrence of h loses the same
factor for Im z < 0 (|h_n| falls with n up to the turning point).  Everything here therefore runs at ``digits(z)`` =
40 + ceil(2 |Im z| / ln 10) digits, and ``tools/make_radial_fixtures.py`` recomputes every stored value at 20 more digits and requires
agreement to 1e-30 relative.

ERROR SCALES (what an fp64 result is measured against):
  h_n                relative;
  z_n, n + d/2 - 1 >= |z| or |z| <= 1      relative (the small regular functions scale matrix rows);
  z_n otherwise      the envelope E_n = max(|z_n|, min(|h^(1)_n|, |h^(2)_n|)), h^(2) = 2 z - h^(1): near a zero of z_n the relative
                     error says nothing;
  gj, gh             |alpha z| + |beta k z'|  (Robin coefficients may cancel);
  blc                |k^{d-2} rho^{d-1}| (|eta z| + |k z'|);
and the weight max(n + 1, |z|): a relative perturbation delta of the argument changes these functions by about that times delta.

``tests/test_radial_yardstick_host.py`` ties this module to the golden-pinned fp64 oracle at low order.  No GPU test imports it.
"""
from __future__ import annotations

import math

import mpmath as mp

from .mp_field import _mp, radial_h, radial_j

BASE_DPS = 40


def digits(z, extra: int = 0) -> int:
    """Working digits for the argument z: 40 + ceil(2 |Im z| / ln 10) (+ extra)."""
    return BASE_DPS + int(math.ceil(2.0 * abs(complex(z).imag) / math.log(10.0))) + extra


def radial(nmax: int, d: int, z, extra: int = 0):
    """(z_n, h_n), n = 0 .. nmax, at the fp64 number z (real or complex), as mpmath numbers computed at digits(z) + extra digits."""
    with mp.workdps(digits(z, extra)):
        zz = _mp(z)
        return radial_j(nmax, d, zz), radial_h(nmax, d, zz)


def radial_scales(nmax: int, d: int, z, j, h):
    """(scale of z_n, scale of h_n, weight) per order, as floats, for the values of ``radial``.

    z_n is measured relative to itself from the turning point of its Bessel order on, n + d/2 - 1 >= |z| (for d > 2 earlier than
    n >= |z|: the stricter reading), and for |z| <= 1, where nothing oscillates and the envelope would be the singular function."""
    az = abs(complex(z))
    sj, sh, w = [], [], []
    for n in range(nmax + 1):
        aj, ah = abs(j[n]), abs(h[n])
        sj.append(float(aj if (n + 0.5 * d - 1 >= az or az <= 1.0) else max(aj, min(ah, abs(2 * j[n] - h[n])))))
        sh.append(float(ah))
        w.append(max(n + 1.0, az))
    return sj, sh, w


def ball_tables(d: int, n_end: int, k, eta, rho, alpha, beta, extra: int = 0):
    """gj, gh, blc (n = 0 .. n_end - 1) of one ball with their scales and the weight: dict of lists (values mpmath, the rest floats).

    alpha, beta: one fp64 number each, or a sequence of n_end of them (the degree-dependent tables).
    """
    x64 = complex(k) * float(rho)
    with mp.workdps(digits(x64, extra)):
        kk, et, rh = _mp(k), mp.mpf(float(eta)), mp.mpf(float(rho))
        x = kk * rh                                      # the exact product; the kernels round it (one ulp of the argument)
        j, h = radial_j(n_end, d, x), radial_h(n_end, d, x)
        per_degree = hasattr(alpha, "__len__")
        out = dict(gj=[], gh=[], blc=[], gj_scale=[], gh_scale=[], blc_scale=[], weight=[])
        pref = kk ** (d - 2) * rh ** (d - 1)
        for n in range(n_end):
            al, be = (_mp(alpha[n]), _mp(beta[n])) if per_degree else (_mp(alpha), _mp(beta))
            jp, hp = n / x * j[n] - j[n + 1], n / x * h[n] - h[n + 1]
            out["gj"].append(al * j[n] + be * kk * jp)
            out["gh"].append(al * h[n] + be * kk * hp)
            out["blc"].append(pref * (et * j[n] + 1j * kk * jp))
            out["gj_scale"].append(float(abs(al * j[n]) + abs(be * kk * jp)))
            out["gh_scale"].append(float(abs(al * h[n]) + abs(be * kk * hp)))
            out["blc_scale"].append(float(abs(pref) * (abs(et * j[n]) + abs(kk * jp))))
            out["weight"].append(max(n + 1.0, abs(complex(x))))
        return out


def translation_2d_factors(n_end: int, k, t, extra: int = 0):
    """H_mu(k |t|) and e^{i mu phi}, mu = 0 .. 2 n_end - 2, of the displacement t = (t_x, t_y) (fp64 numbers): two lists (mpmath)."""
    with mp.workdps(digits(complex(k) * math.hypot(float(t[0]), float(t[1])), extra)):
        tx, ty = mp.mpf(float(t[0])), mp.mpf(float(t[1]))
        r = mp.sqrt(tx * tx + ty * ty)
        hank = [v / mp.sqrt(mp.pi / 2) for v in radial_h(2 * n_end - 2, 2, _mp(k) * r)]
        w = mp.mpc(tx, ty) / r
        e = [mp.mpc(1)]
        for _ in range(2 * n_end - 2):
            e.append(e[-1] * w)
        return hank, e


def translation_2d(n_end: int, k, t):
    """The matrix of ``biem_oracle.translation_SR_2d_graf`` (rows m', columns m in the order of Tree("a").index), rounded to fp64."""
    import numpy as np

    from . import biem_oracle as O

    hank, e = translation_2d_factors(n_end, k, t)
    ms = [m for (m,) in O.tree("a").index(n_end)]
    out = np.zeros((len(ms), len(ms)), dtype=np.complex128)
    with mp.workdps(digits(complex(k) * math.hypot(float(t[0]), float(t[1])))):
        for a, mp_ in enumerate(ms):
            for b, m in enumerate(ms):
                mu = mp_ - m
                ph = e[mu] if mu >= 0 else mp.conj(e[-mu])
                out[a, b] = complex(mp.mpc(0, 1) ** (abs(m) + abs(mu) - abs(mp_)) * hank[abs(mu)] * ph)
    return out
