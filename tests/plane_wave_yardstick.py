"""NumPy twin of the closed-form right-hand side of plane-wave incidence (helper module, not a test).

Written against the CPU oracle (`oracle.biem_oracle`: `ball_tables`, `radial_h`, a tree's `harmonics` / `degrees`).  With the project's
radial functions z_n = sqrt(pi/2) Z_{n+d/2-1}(x) / x^{d/2-1} and orthonormal harmonics, u_in = e^{i k p^.x} has on the surface of a ball
of centre c and radius rho the projections

    U_h = C_d i^n j_n(k rho) conj(Y_h(p^)) e^{i k p^.c},    V_h = C_d i^n k j_n'(k rho) conj(Y_h(p^)) e^{i k p^.c}

of u_in and d_n u_in, C_d = 2^{(d+1)/2} pi^{(d-1)/2}, and the right-hand side is f = -(alpha U + beta V) = -C_d i^n gj_n conj(Y_h) e^{i k p^.c}.
"""
import numpy as np

from oracle import biem_oracle as O


def c_d(d):
    return 2.0 ** ((d + 1) / 2.0) * np.pi ** ((d - 1) / 2.0)


def angular(tr, n_end, k, center, p):
    """C_d i^n conj(Y_h(p^)) e^{i k p^.c} [H]: everything of U, V and f but the radial factor."""
    p = np.asarray(p, dtype=np.float64)
    p = p / np.linalg.norm(p)
    deg = tr.degrees(n_end)
    Y = tr.harmonics(p[None, :], n_end)[:, 0]
    return c_d(tr.d) * 1j ** deg * np.conj(Y) * np.exp(1j * k * (p @ np.asarray(center, dtype=np.float64)))


def projections(tr, n_end, k, center, rho, p):
    """(U[H], V[H]) of one ball in closed form."""
    deg = tr.degrees(n_end)
    j, _, jp, _ = O.radial_h(n_end - 1, tr.d, k * rho)
    a = angular(tr, n_end, k, center, p)
    return a * j[deg], a * (k * jp)[deg]


def quadrature_projections(tr, n_end, k, center, rho, p, nq):
    """(U[H], V[H]) by the tree's nq-rule: what the sampled path computes with nq = n_end."""
    uin, ugr = O.plane_wave(k, p)
    y, w = tr.quadrature(nq)
    Yc = np.conj(tr.harmonics(y, n_end))
    x = np.asarray(center)[None, :] + rho * y
    return Yc @ (w * uin(x)), Yc @ (w * np.sum(ugr(x) * y, axis=-1))


def rhs(tr, n_end, k, centers, radii, alpha, beta, p, eta=1.0):
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
        out[b] = -gj[deg] * angular(tr, n_end, k, centers[b], p)
    return out
