"""Reader of ``tests/golden/full_order_fields.npz``  --  TEST INFRASTRUCTURE ONLY (NumPy; no mpmath, no GPU).

The fixture pins the per-lane field kernels at their order ceilings against values computed at 40 digits by ``oracle.mp_field``
(written by ``tools/make_full_order_fixtures.py``, read by ``tests/test_gpu_full_order.py`` and
``tests/test_full_order_yardstick_host.py``).

A density of 2 x 2304 complex numbers per case would make the file several MB, so it is stored in two factors whose product is
an exactly reproducible fp64 number:  density[b, h] = w[b, h] * t[b, n(h)]  with one complex table ``w`` per (tree family, order)
shared by all its cases (|w| in [0.5, 1.5], phases over the circle) and one REAL per-degree scale ``t`` per case and ball.
A real times a complex is two independent fp64 products, so generator, host test and GPU test hold bit-identical densities;
the expected values were computed from exactly those numbers.
"""
from __future__ import annotations

import json
import os
import types

import numpy as np

from . import biem_oracle as O

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "full_order_fields.npz")
LDS_BYTES = 160 * 1024      # the launchers' limit per workgroup
LANES = 64                  # T of the kernels that keep a per-lane j_n row (kind inner, interior)


def lds_row_ceiling(grad: bool) -> int:
    """Largest 2-D order whose per-lane rows fit the LDS: the launchers' formula
    shm = 16 (2 n_end - 1 + T js),  js = (n_end + 2) | 1 (value) or (n_end + 3) | 1 (gradient),  T = 64,  shm <= 160 KiB.
    (A kernel whose code object holds LDS of its own fits less; its launcher adds that.)"""
    n = 1
    while 16 * (2 * (n + 1) - 1 + LANES * (((n + 1) + (3 if grad else 2)) | 1)) <= LDS_BYTES:
        n += 1
    return n


def density(w: np.ndarray, t: np.ndarray, deg: np.ndarray) -> np.ndarray:
    """w[B, H] complex times the real per-degree scale t[B, n_end]: real and imaginary parts multiplied separately."""
    s = t[:, deg]
    return (w.real * s) + 1j * (w.imag * s)


HESS_FORCE_PATH = os.path.join(os.path.dirname(PATH), "full_order_hess_force.npz")


def load_hess_force(path: str = HESS_FORCE_PATH) -> dict:
    """{case id: record} of ``tests/golden/full_order_hess_force.npz`` (``tools/make_full_order_hess_force_fixtures.py``).

    A force record has tree, n_end, regime, bc ("robin": the scalar pair alpha, beta; "fluid" / "transparent-top": alpha_n, beta_n
    [B, n_end]), k, eta, radii [B], density [B, H], phi [B, d] (NaN for a ball whose expected output is NaN), cond [B], oracle_err [B].
    A Hessian record (family "hess") has tree, kind, regime, n_end, k, eta, centers [B, d], radii [B], density [B, H], x [P, d],
    valid [P], hess [d, d, P] (stored as its upper triangle), cond [P] (of the value series) and oracle_err [P] (the fp64 twin).
    The launch-shape record (regime "batch") has k [S], radii [S, B], density [S, R, B, H] (right-hand side r is the table w rolled by
    r harmonics) and phi [S, R, B, d], cond and oracle_err [S, R, B]."""
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for cid in json.loads(str(z["cases"])):
            meta = json.loads(str(z[cid + "/meta"]))
            rec = types.SimpleNamespace(id=cid, **meta)
            for key in z.files:
                if key.startswith(cid + "/") and key != cid + "/meta":
                    setattr(rec, key[len(cid) + 1:], z[key])
            rec.radii = np.array(meta["radii"])
            rec.cond, rec.oracle_err = rec.caps.astype(np.float64)          # (the two admission figures, in single precision)
            if "centers" in meta:
                rec.centers = np.array(meta["centers"])
            if "k_interior" in meta:
                rec.density_ratio = np.array(meta["density_ratio"])
                rec.k_interior = np.array([[complex(*v) for v in row] for row in meta["k_interior"]])
                rec.k_interior = rec.k_interior[0] if rec.radii.ndim == 1 else rec.k_interior
            deg = O.tree(rec.tree).degrees(rec.n_end)
            w = z["w/" + rec.w].astype(np.complex128)          # (stored in single precision: exact fp64 numbers at half the size)
            if rec.family == "hess":
                rec.k = complex(*meta["k"]) if meta["k"][1] != 0.0 else float(meta["k"][0])
                d = rec.x.shape[1]
                iu = np.triu_indices(d)
                rec.hess = np.empty((d, d, len(rec.x)), dtype=np.complex128)
                rec.hess[iu] = rec.hess_upper
                rec.hess[(iu[1], iu[0])] = rec.hess_upper
                rec.density = density(w[:len(rec.radii)], rec.t, deg)
                out[cid] = rec
                continue
            rec.alpha, rec.beta = complex(*meta["alpha"]), complex(*meta["beta"])
            if rec.regime == "batch":
                rec.k = np.array(meta["k"])
                rec.density = np.stack([np.stack([density(np.roll(w, r, axis=1), t, deg) for r in range(rec.phi.shape[1])]) for t in rec.t])
            else:
                rec.density = density(w[:len(rec.radii)], rec.t, deg)
            out[cid] = rec
    return out


def load(path: str = PATH) -> dict:
    """{case id: record}.  A record has tree, kind ("outer", "inner", "interior"), regime, n_end, k, eta, centers [B, d], radii [B],
    density [B, H], x [P, d], valid [P], value [P], cond [P], oracle_err [P] and, where the case has them, grad [d, P],
    per_ball [P, B] (+ cond_ball, oracle_err_ball), density_far / far [P] (+ cond_far, oracle_err_far), k_interior / density_ratio [B]."""
    out = {}
    with np.load(path, allow_pickle=False) as z:
        ids = json.loads(str(z["cases"]))
        for cid in ids:
            meta = json.loads(str(z[cid + "/meta"]))
            rec = types.SimpleNamespace(id=cid, **meta)
            rec.k = complex(*meta["k"]) if meta["k"][1] != 0.0 else float(meta["k"][0])
            for key in z.files:
                if key.startswith(cid + "/") and key != cid + "/meta":
                    setattr(rec, key[len(cid) + 1:], z[key])
            deg = O.tree(rec.tree).degrees(rec.n_end)
            w = z["w/" + rec.w][:len(rec.radii)]
            rec.density = density(w, rec.t, deg)
            rec.density_far = density(w, rec.t_far, deg) if hasattr(rec, "t_far") else None
            rec.grad = getattr(rec, "grad", None)
            out[cid] = rec
    return out
