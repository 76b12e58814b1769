"""High-precision evaluation of the field series  --  TEST INFRASTRUCTURE ONLY, CPU only (mpmath).

An independent restatement, in mpmath arithmetic at ``DPS`` digits, of the three sums the per-lane field kernels evaluate:

* the exterior near field   sum_b sum_h dens[b,h] blc_n(rho_b) h_n(k r) Y_h          (``biem_oracle.uscat``, kind "outer")
* the kind-inner field      the same with j_n(k r) and blc built from h_n(k rho), h_n'(k rho)
* the far-field pattern     sum_b e^{-i k x.c_b} / (i k)^{(d-1)/2} sum_h dens blc_n (-i)^n Y_h
* the interior field        sum_h a_{b,h} j_n(k_b r) Y_h,  a = -s delta k W / gj_n,  s = dens blc_n,  W = i / (k rho)^{d-1},
                            gj_n = -k_b j_n'(k_b rho) j_n(k rho) + delta j_n(k_b rho) k j_n'(k rho)

and of their Cartesian gradients, taken by central differences of the high-precision field itself (step ``GRAD_STEP``: the
truncation error (n step / rho)^2 / 6 and the rounding 10^-DPS / step are both far below fp64), so no formula here divides by a
sine and points on the axes of a coordinate tree need no special case.

The harmonics follow the definitions of ``biem_oracle.Tree.harmonics`` (``_pbar``, ``_gbar``, ``_cbar``) with every constant in
mpmath; the radial functions start from ``mpmath.hankel1`` / ``mpmath.besselj`` at two orders and run the three-term recurrence
upwards (h) or downwards (j).  Densities, points, centres, radii and wavenumbers enter as the exact values of their fp64 numbers.

``tests/test_full_order_yardstick_host.py`` ties this module to the golden-pinned fp64 oracle at low order; the generator
``tools/make_full_order_fixtures.py`` uses it at the order ceilings of the kernels.  No GPU test imports it.
"""
from __future__ import annotations

from functools import lru_cache

import mpmath as mp
import numpy as np

from . import biem_oracle as O

DPS = 40
GRAD_STEP = "1e-12"


# --------------------------------------------------------------------------------------
# constants of the harmonics (cached per order, computed at DPS digits)
# --------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _pbar_tables(nmax: int):
    with mp.workdps(DPS):
        diag = [None] + [mp.sqrt(mp.mpf(2 * m + 1) / (2 * m)) for m in range(1, nmax + 1)]
        first = [mp.sqrt(mp.mpf(2 * m + 3)) for m in range(nmax + 1)]
        a = {(n, m): mp.sqrt(mp.mpf(4 * n * n - 1) / (n * n - m * m)) for m in range(nmax) for n in range(m + 2, nmax + 1)}
        b = {(n, m): mp.sqrt(mp.mpf((n - 1) ** 2 - m * m) / (4 * (n - 1) ** 2 - 1)) for m in range(nmax) for n in range(m + 2, nmax + 1)}
        return diag, first, a, b, mp.sqrt(mp.mpf(1) / 2)


def _pbar(nmax: int, x, s):
    """P[n][m], 0 <= m <= n <= nmax: orthonormal associated Legendre at x with s = sqrt(1 - x^2) (no Condon-Shortley phase)."""
    diag, first, a, b, p00 = _pbar_tables(nmax)
    P = [[mp.mpf(0)] * (nmax + 1) for _ in range(nmax + 1)]
    P[0][0] = p00
    for m in range(1, nmax + 1):
        P[m][m] = diag[m] * s * P[m - 1][m - 1]
    for m in range(nmax):
        P[m + 1][m] = first[m] * x * P[m][m]
        for n in range(m + 2, nmax + 1):
            P[n][m] = a[n, m] * (x * P[n - 1][m] - b[n, m] * P[n - 2][m])
    return P


@lru_cache(maxsize=None)
def _gbar_tables(kmax: int, l: int):
    """lam = l + 1: p_0 = 1 / sqrt(h_0) and a_k of  x p_{k-1} = a_k p_k + a_{k-1} p_{k-2}."""
    with mp.workdps(DPS):
        lam = mp.mpf(l + 1)
        h0 = mp.sqrt(mp.pi) * mp.gamma(lam + mp.mpf(1) / 2) / mp.gamma(lam + 1)
        a = [None] + [mp.sqrt(k * (k + 2 * lam - 1) / ((k + lam - 1) * (k + lam))) / 2 for k in range(1, kmax + 1)]
        return 1 / mp.sqrt(h0), a


def _gbar(kmax: int, l: int, x):
    p0, a = _gbar_tables(kmax, l)
    p = [p0]
    if kmax >= 1:
        p.append(x * p0 / a[1])
    for k in range(2, kmax + 1):
        p.append((x * p[k - 1] - a[k - 1] * p[k - 2]) / a[k])
    return p


@lru_cache(maxsize=None)
def _cbar_tables(n: int, a: int, b: int):
    """norm and the integer coefficients of P_k^{(b, a)}(x) = sum_s C(k+b, k-s) C(k+a, s) ((x-1)/2)^s ((x+1)/2)^{k-s}, k = (n-a-b)/2."""
    with mp.workdps(DPS):
        k = (n - a - b) // 2
        f = mp.factorial
        norm = mp.sqrt(2 * mp.mpf(2 * k + a + b + 1) * f(k) * f(k + a + b) / (f(k + a) * f(k + b)))
        return k, norm, [mp.binomial(k + b, k - s) * mp.binomial(k + a, s) for s in range(k + 1)]


def _cbar(n: int, a: int, b: int, c, s):
    """cos^a sin^b Pbar_k^{(b,a)}(cos 2 theta) with c = cos theta, s = sin theta, normalised over sin cos dtheta."""
    k, norm, co = _cbar_tables(n, a, b)
    x = c * c - s * s
    um, up = (x - 1) / 2, (x + 1) / 2
    jac = mp.fsum(co[q] * um ** q * up ** (k - q) for q in range(k + 1))
    return norm * c ** a * s ** b * jac


def _phase(re, im):
    """(re + i im) / |re + i im|, or 1 where both vanish (atan2(0, 0) = 0)."""
    r = mp.hypot(re, im)
    return mp.mpc(re, im) / r if r != 0 else mp.mpc(1)


def _powers(w, nmax: int):
    out = [mp.mpc(1)]
    for _ in range(nmax):
        out.append(out[-1] * w)
    return out


def harmonics(name: str, n_end: int, u):
    """Y_h(u) of a canonical tree (a, ba, bba, caa) at the unit vector u (mpf list), in the order of ``Tree.index``."""
    idx = O.tree(name).index(n_end)
    isq = 1 / mp.sqrt(2 * mp.pi)
    nm = max(n_end - 1, 0)
    if name == "a":
        wp = _powers(_phase(u[0], u[1]), nm)
        return [(wp[m] if m >= 0 else mp.conj(wp[-m])) * isq for (m,) in idx]
    if name == "ba":
        Pb = _pbar(nm, u[0], mp.hypot(u[1], u[2]))
        wp = _powers(_phase(u[1], u[2]), nm)
        return [Pb[n][abs(m)] * (wp[m] if m >= 0 else mp.conj(wp[-m])) * isq for (n, m) in idx]
    if name == "bba":
        c0, s0 = u[0], mp.sqrt(u[1] ** 2 + u[2] ** 2 + u[3] ** 2)
        c1 = u[1] / s0 if s0 != 0 else mp.mpf(1)
        s1 = mp.hypot(u[2], u[3]) / s0 if s0 != 0 else mp.mpf(0)
        Pb = _pbar(nm, c1, s1)
        wp = _powers(_phase(u[2], u[3]), nm)
        G = [_gbar(n_end - 1 - l, l, c0) for l in range(n_end)]
        sl = [s0 ** l for l in range(n_end)]
        return [sl[l] * G[l][n - l] * Pb[l][abs(m)] * (wp[m] if m >= 0 else mp.conj(wp[-m])) * isq for (n, l, m) in idx]
    if name == "caa":
        c, s = mp.hypot(u[0], u[1]), mp.hypot(u[2], u[3])
        w1, w2 = _powers(_phase(u[0], u[1]), nm), _powers(_phase(u[2], u[3]), nm)
        cb = {}
        out = []
        for (n, m1, m2) in idx:
            key = (n, abs(m1), abs(m2))
            if key not in cb:
                cb[key] = _cbar(n, abs(m1), abs(m2), c, s)
            e1 = w1[m1] if m1 >= 0 else mp.conj(w1[-m1])
            e2 = w2[m2] if m2 >= 0 else mp.conj(w2[-m2])
            out.append(cb[key] * e1 * e2 * isq * isq)
        return out
    raise NotImplementedError(name)


# --------------------------------------------------------------------------------------
# radial functions  z_n^{(d)}(z) = sqrt(pi/2) Z_{n + d/2 - 1}(z) / z^{d/2 - 1},  n = 0 .. nmax
# --------------------------------------------------------------------------------------
def radial_h(nmax: int, d: int, z):
    """Outgoing h_n^{(d)}(z): hankel1 at the two lowest orders, then upwards (the dominant direction for n > |z|)."""
    nu0 = mp.mpf(d) / 2 - 1
    pref = mp.sqrt(mp.pi / 2) / z ** nu0
    f = [pref * mp.hankel1(nu0, z), pref * mp.hankel1(nu0 + 1, z)]
    for n in range(1, nmax):
        f.append(2 * (n + nu0) / z * f[n] - f[n - 1])
    return f[:nmax + 1]


def radial_j(nmax: int, d: int, z):
    """Regular j_n^{(d)}(z): besselj at the two highest orders, then downwards; z = 0 is the closed form delta_{n0} sqrt(pi/2) 2^{1-d/2} / Gamma(d/2)."""
    nu0 = mp.mpf(d) / 2 - 1
    if z == 0:
        return [mp.sqrt(mp.pi / 2) * mp.mpf(2) ** (1 - mp.mpf(d) / 2) / mp.gamma(mp.mpf(d) / 2)] + [mp.mpf(0)] * nmax
    pref = mp.sqrt(mp.pi / 2) / z ** nu0
    f = [None] * (nmax + 2)
    f[nmax + 1] = pref * mp.besselj(nu0 + nmax + 1, z)
    f[nmax] = pref * mp.besselj(nu0 + nmax, z)
    for n in range(nmax, 0, -1):
        f[n - 1] = 2 * (n + nu0) / z * f[n] - f[n + 1]
    return f[:nmax + 1]


def _with_derivative(f, z):
    """(z_n, z_n') for n = 0 .. len(f) - 2 from z_n' = (n / z) z_n - z_{n+1}."""
    return f[:-1], [n / z * f[n] - f[n + 1] for n in range(len(f) - 1)]


def _mp(v):
    """The exact value of an fp64 real or complex number."""
    v = complex(v)
    return mp.mpf(v.real) if v.imag == 0.0 else mp.mpc(v.real, v.imag)


HESS_STEPS = ("1e-10", "2e-10")
STEP_AGREE = 1e-14


def hessian_by_differences(F, x, step, mode: str = "near"):
    """[d][d] mpc at one point (mpf list): second central differences of the sum over the balls of the 40-digit series of F."""
    d = F.d
    h = mp.mpf(step)
    balls = F.balls(mode, x)

    def f(shift):
        y = [x[i] + shift.get(i, 0) * h for i in range(d)]
        return mp.fsum(F.ball_sum(mode, b, y) for b in balls)

    f0 = f({})
    H = [[None] * d for _ in range(d)]
    for i in range(d):
        H[i][i] = (f({i: 1}) - 2 * f0 + f({i: -1})) / (h * h)
        for j in range(i + 1, d):
            H[i][j] = H[j][i] = (f({i: 1, j: 1}) - f({i: 1, j: -1}) - f({i: -1, j: 1}) + f({i: -1, j: -1})) / (4 * h * h)
    return H


# --------------------------------------------------------------------------------------
# the evaluator
# --------------------------------------------------------------------------------------
class MPField:
    """The series of one result record (one k, one eta): density [B, H] as ``biem_oracle.OracleResult`` holds it.

    ``k_interior`` / ``density_ratio`` [B] switch on the interior field.  Points are rows x[d] in the caller's axes.
    Every public method works at ``DPS`` digits whatever the caller's mpmath precision.
    """

    def __init__(self, tree: str, n_end: int, k, eta, centers, radii, density, kind: str = "outer", k_interior=None, density_ratio=None):
        self.tr = O.tree(tree)
        self.canon = self.tr.base or self.tr.name
        self.perm = list(self.tr.perm) if self.tr.base else list(range(self.tr.d))
        self.d, self.n_end, self.kind = self.tr.d, int(n_end), kind
        self.deg = [int(n) for n in self.tr.degrees(n_end)]
        self.H = len(self.deg)
        self.centers = np.asarray(centers, dtype=np.float64).reshape(-1, self.d)
        self.radii = np.asarray(radii, dtype=np.float64).reshape(-1)
        self.B = len(self.radii)
        self.density = np.asarray(density, dtype=np.complex128).reshape(self.B, self.H)
        with mp.workdps(DPS):
            self.k, self.eta = _mp(k), _mp(eta)
            self.cen = [[mp.mpf(float(v)) for v in c] for c in self.centers]
            self.rho = [mp.mpf(float(r)) for r in self.radii]
            self.kb = None if k_interior is None else [_mp(v) for v in np.broadcast_to(np.asarray(k_interior, dtype=np.complex128), (self.B,))]
            self.delta = None if density_ratio is None else [_mp(v) for v in np.broadcast_to(np.asarray(density_ratio, dtype=np.complex128), (self.B,))]
        self._coef = {}

    # ---- per-degree factors ---------------------------------------------------------------
    def blc(self, b: int, inner: bool):
        """blc_n(rho_b), n < n_end: dlc - i eta slc with j (outer, far field) or h (kind inner) at k rho."""
        d, k, rho = self.d, self.k, self.rho[b]
        z, zp = _with_derivative((radial_h if inner else radial_j)(self.n_end, d, k * rho), k * rho)
        return [1j * k ** (d - 1) * rho ** (d - 1) * zp[n] - 1j * self.eta * (1j * k ** (d - 2) * rho ** (d - 1) * z[n]) for n in range(self.n_end)]

    def interior_factor(self, b: int):
        """a_{b,h} / dens[b,h] per degree: -blc_n delta k W / gj_n."""
        d, k, rho, kb, dl = self.d, self.k, self.rho[b], self.kb[b], self.delta[b]
        x = k * rho
        j, jp = _with_derivative(radial_j(self.n_end, d, x), x)
        jz, jpz = _with_derivative(radial_j(self.n_end, d, kb * rho), kb * rho)
        blc = self.blc(b, False)
        W = 1j / x ** (d - 1)
        return [-blc[n] * dl * k * W / (-kb * jpz[n] * j[n] + dl * jz[n] * k * jp[n]) for n in range(self.n_end)]

    def coef(self, mode: str, b: int):
        """The coefficient of z_n Y_h in ball b's sum: mode "near" (by kind), "far" ((-i)^n included) or "interior"."""
        if (mode, b) not in self._coef:
            if mode == "near":
                fac = self.blc(b, self.kind == "inner")
            elif mode == "far":
                blc = self.blc(b, False)
                fac = [blc[n] * mp.mpc(0, -1) ** n for n in range(self.n_end)]
            elif mode == "interior":
                fac = self.interior_factor(b)
            else:
                raise ValueError(mode)
            dn = self.density[b]
            self._coef[mode, b] = [mp.mpc(float(dn[h].real), float(dn[h].imag)) * fac[self.deg[h]] for h in range(self.H)]
        return self._coef[mode, b]

    # ---- one ball's sum ----------------------------------------------------------------------
    def _x(self, x):
        return [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in x]

    def ball_sum(self, mode: str, b: int, x, with_abs: bool = False):
        """sum_h of ball b at x (mpf list, caller's axes); with_abs: also sum_h |term|."""
        rel = [x[i] - self.cen[b][i] for i in range(self.d)]
        r = mp.sqrt(mp.fsum(v * v for v in rel))
        u = [rel[p] / r for p in self.perm] if r != 0 else [mp.mpf(1)] + [mp.mpf(0)] * (self.d - 1)
        Y = harmonics(self.canon, self.n_end, u)
        c = self.coef(mode, b)
        nm = self.n_end - 1
        if mode == "far":
            rad = [mp.mpf(1)] * self.n_end
            common = mp.exp(-1j * self.k * mp.fsum(x[i] * self.cen[b][i] for i in range(self.d))) / (1j * self.k) ** (mp.mpf(self.d - 1) / 2)
        else:
            common = mp.mpf(1)
            if mode == "interior":
                rad = radial_j(nm, self.d, self.kb[b] * r)
            elif self.kind == "inner":
                rad = radial_j(nm, self.d, self.k * r)
            else:
                rad = radial_h(nm, self.d, self.k * r)
        byn = [mp.mpc(0)] * self.n_end
        absn = [mp.mpf(0)] * self.n_end
        for h, n in enumerate(self.deg):
            t = c[h] * Y[h]
            byn[n] += t
            if with_abs:
                absn[n] += abs(t)
        total = common * mp.fsum(byn[n] * rad[n] for n in range(self.n_end))
        if with_abs:
            return total, abs(common) * mp.fsum(absn[n] * abs(rad[n]) for n in range(self.n_end))
        return total

    def ball_of(self, x):
        """The ball whose interior holds x (the first, as the kernels scan), or -1."""
        for b in range(self.B):
            if mp.fsum((x[i] - self.cen[b][i]) ** 2 for i in range(self.d)) < self.rho[b] ** 2:
                return b
        return -1

    def valid(self, mode: str, x):
        """The mask of ``biem_oracle.uscat`` / of the interior field, from the exact distances."""
        if mode == "far":
            return True
        if mode == "interior":
            return self.ball_of(x) >= 0
        r2 = [mp.fsum((x[i] - self.cen[b][i]) ** 2 for i in range(self.d)) for b in range(self.B)]
        if self.kind == "outer":
            return all(r2[b] >= self.rho[b] ** 2 for b in range(self.B))
        return all(r2[b] <= self.rho[b] ** 2 for b in range(self.B))

    def balls(self, mode: str, x):
        return [self.ball_of(x)] if mode == "interior" else list(range(self.B))

    # ---- public: values, condition numbers, gradients --------------------------------------------
    def value(self, mode: str, x, with_cond: bool = False):
        """Per-ball sums [B'] at one point (B' = 1 for the interior field: the ball that holds x), unmasked.
        with_cond: also sum |terms| per ball."""
        with mp.workdps(DPS):
            x = self._x(x)
            res = [self.ball_sum(mode, b, x, with_cond) for b in self.balls(mode, x)]
            return ([v for v, _ in res], [a for _, a in res]) if with_cond else res

    def gradient(self, mode: str, x, components=None):
        """Cartesian gradient [d] (or the listed components) of the sum over balls at one point, by central differences of the
        high-precision field."""
        with mp.workdps(DPS):
            x = self._x(x)
            balls = self.balls(mode, x)
            step = mp.mpf(GRAD_STEP)
            g = []
            for i in (range(self.d) if components is None else components):
                xp, xm = list(x), list(x)
                xp[i] += step
                xm[i] -= step
                g.append(mp.fsum(self.ball_sum(mode, b, xp) - self.ball_sum(mode, b, xm) for b in balls) / (2 * step))
            return g

    def hessian(self, mode: str, x):
        """Cartesian Hessian [d][d] of the sum over balls at one point: second central differences (diagonal) and four-point cross
        differences of the high-precision field with the step HESS_STEPS[0], accepted only if the step HESS_STEPS[1] agrees within
        STEP_AGREE of the largest component (truncation (step^2 / 12) f'''' and rounding 10^-DPS / step^2 are both near 1e-20)."""
        with mp.workdps(DPS):
            x = self._x(x)
            one, two = (hessian_by_differences(self, x, s, mode) for s in HESS_STEPS)
            scale = max(abs(v) for row in one for v in row)
            worst = max(abs(one[i][j] - two[i][j]) for i in range(self.d) for j in range(self.d))
            if worst > STEP_AGREE * scale:
                raise ArithmeticError(f"second differences of steps {HESS_STEPS} differ by {float(worst / scale):.1e} of max |H|")
            return one

    # ---- NumPy faces with the oracle's conventions -----------------------------------------------
    def _mode(self, far_field: bool, interior: bool) -> str:
        return "interior" if interior else "far" if far_field else "near"

    def uscat(self, x, far_field: bool = False, per_ball: bool = False, interior: bool = False) -> np.ndarray:
        """As ``biem_oracle.uscat`` (x[P, d] -> [P] or [P, B], NaN where masked), rounded to fp64; interior=True: the interior field."""
        mode = self._mode(far_field, interior)
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.d)
        out = np.full((len(x), self.B), np.nan + 0j)
        with mp.workdps(DPS):
            for p, xp in enumerate(x):
                xm = self._x(xp)
                if self.valid(mode, xm):
                    v = self.value(mode, xm)
                    out[p, :len(v)] = [complex(t) for t in v]
                    if not per_ball:
                        out[p, 0] = complex(mp.fsum(v))
        return out if per_ball and not interior else out[:, 0]

    def uscat_grad(self, x, interior: bool = False) -> np.ndarray:
        """Gradient [d, P] in the caller's axes, NaN where the value is masked."""
        mode = self._mode(False, interior)
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.d)
        out = np.full((self.d, len(x)), np.nan + 0j)
        with mp.workdps(DPS):
            for p, xp in enumerate(x):
                xm = self._x(xp)
                if self.valid(mode, xm):
                    out[:, p] = [complex(t) for t in self.gradient(mode, xm)]
        return out
