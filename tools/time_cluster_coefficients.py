"""Times regular-wave incidence, the cluster's outgoing coefficients and the T-matrix, in one process: one JSON line per measurement.

python tools/time_cluster_coefficients.py [systems] [right-hand sides ...]   default: 256 systems of cfg 3 (ba, 16 balls, n_end 20), 1 and 64

Per number of right-hand sides (regular waves about the middle of the cluster, the last harmonic of degree 1), median and spread
(min, max) in ms of
  (a) rhs_regular_wave:  biem_rhs_regular_wave alone, into the natural layout, beside
      rhs_multipole:     biem_rhs_multipole for as many dipoles on a circle around the cluster (tools/time_multipole_rhs.py);
  (b) cluster:           calc.cluster_coefficients(origin=middle) of the solved densities, its two stages alone (table rows of every
                         (system, ball); contraction, with the coefficient pass), beside
      far_pattern:       calc.far_pattern at H directions (as many numbers per right-hand side);
and once
  (c) tmatrix:           fac.tmatrix(origin=middle) beside solve_all: the fac.solve of all H regular waves it contains, in one call,
                         and cluster_all: cluster_coefficients of those densities.
Every step runs once before it is timed; times are wall-clock around a device synchronisation.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import biem_helmholtz_sphere_amd as amd  # noqa: E402
from biem_helmholtz_sphere_amd import _biem, _fields, _operator  # noqa: E402
from bench import workload  # noqa: E402  (the configurations of the benchmark)

REPS = 5


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def run(nb, counts, with_tmatrix=True):
    w = workload(3, nb, 0, nb)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    c = amd.create_from_branching_types(w["tree"])
    B, n_end = w["B"], w["n_end"]
    cen = np.asarray(w["centers"], dtype=np.float64)
    kw = dict(centers=t(cen)[None, None], radii=t(np.ones(B))[None, None], k=t(w["ks"])[:, None], eta=t(w["etas"])[:, None],
              n_end=n_end, alpha=w["alpha"], beta=w["beta"])
    fac = amd.biem_factorize(c, **kw)
    op, lib, L = fac._op, _biem.L.load(), _biem.L
    H, sp, fl = op.plan.H, _biem._stream_ptr(op.dev), op.fl
    _, degrees = amd.harmonic_labels(c, n_end)
    dipole = int(np.nonzero(degrees == 1)[0][-1])
    mid = cen.mean(axis=0)
    ring = np.linalg.norm(cen - mid, axis=-1).max() + 1.5
    base = dict(systems=nb, balls=B, n_end=n_end, H=H)
    for nrhs in counts:
        ang = np.linspace(0.0, 2.0 * np.pi, nrhs, endpoint=False) + 0.1
        pos = np.tile(mid[:, None, None], (1, 1, nrhs))
        org = t(pos)
        pos = pos.copy()
        pos[0, 0] += ring * np.cos(ang)
        pos[1, 0] += ring * np.sin(ang)
        S = t(pos)
        f = torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)
        ms, _ = _operator._multipole_source_source(op, _operator._check_multipole_source(c, kw["k"], n_end, S, dipole, None, None, None, None))
        rw, _ = _operator._regular_wave_source(op, _operator._check_multipole_source(c, kw["k"], n_end, org, dipole, None, None, None, None,
                                                                                    "regular_wave_origin", "regular_wave_index"))
        wb = max(ms.workspace_bytes(op, nb), rw.workspace_bytes(op, nb))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")

        def rhs(entry, g):
            return lambda: L.check(getattr(lib, entry)(op.plan.handle, nb, B, nrhs, _biem._ptr(fl.k), _biem._ptr(fl.centers), fl.geom_batched,
                                                       _biem._ptr(fac._tab), _biem._ptr(g.pts), g.batched, _biem._ptr(g.index), _biem._ptr(f), *strides,
                                                       _biem._ptr(work), wb, sp), entry)

        rec = dict(base, right_hand_sides=nrhs)
        rec["rhs_regular_wave_ms"] = timed(rhs("biem_rhs_regular_wave", rw))
        rec["rhs_multipole_ms"] = timed(rhs("biem_rhs_multipole", ms))
        del work, f
        calc = fac.solve(regular_wave_origin=org, regular_wave_index=dipole)
        o = t(mid)
        rec["cluster_ms"] = timed(lambda: calc.cluster_coefficients(origin=o))
        rec["cluster_tables_ms"] = timed(lambda: _fields.biem_cluster_coefficients(calc, origin=o, _stage=1))
        rec["cluster_contraction_ms"] = timed(lambda: _fields.biem_cluster_coefficients(calc, origin=o, _stage=2))
        rng = np.random.default_rng(0)
        dirs = t(rng.normal(size=(3, H)))
        rec["far_pattern_H_directions_ms"] = timed(lambda: calc.far_pattern(dirs))
        del calc
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
    if with_tmatrix:
        o = t(mid)
        rec = dict(base)
        rec["tmatrix_ms"] = timed(lambda: fac.tmatrix(origin=o), reps=3)
        allw = t(np.tile(mid[:, None, None], (1, 1, H)))
        idx = np.arange(H)[None, :]
        rec["solve_all_ms"] = timed(lambda: fac.solve(regular_wave_origin=allw, regular_wave_index=idx), reps=3)
        calc = fac.solve(regular_wave_origin=allw, regular_wave_index=idx)
        rec["cluster_all_ms"] = timed(lambda: calc.cluster_coefficients(origin=o), reps=3)
        rec["cluster_share_of_tmatrix"] = round(rec["cluster_all_ms"]["median"] / rec["tmatrix_ms"]["median"], 4)
        print(json.dumps(rec), flush=True)
    fac.close()


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    run(args[0] if args else 256, args[1:] or [1, 64])
