"""Times multipole incidence in closed form beside point-source incidence, in one process: one JSON line per number of sources.

python tools/time_multipole_rhs.py [systems] [sources ...]      default: 256 systems of cfg 3 (ba, 16 balls, n_end 20), 1 and 64 sources

Per number of dipole sources (the last harmonic of degree 1), median and spread (min, max) in ms of
  (a) rhs_multipole:      biem_rhs_multipole alone, into the natural layout,
  (b) rhs_point_source:   biem_rhs_point_source alone for the same positions, into the same layout,
  (c) solve_multipole:    fac.solve(multipole_source_position=, multipole_source_index=),
  (d) solve_point_source: fac.solve(point_source_position=),
the workspace of either right-hand side, the slices the multipole launcher walks, and - from torch's profiler, where it records the
library's kernels - the device time of one biem_rhs_multipole call by stage (table rows, contraction).  The sources stand on a circle
around the cluster, half a radius off the nearest surface.  Every step runs once before it is timed; times are wall-clock around a
device synchronisation.
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
from biem_helmholtz_sphere_amd import _biem, _operator  # noqa: E402
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


def stages(fn):
    """Device ms of one call of fn by kernel (table rows, contraction), or None where the profiler does not see the library's kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name, key in (("k_ms_tables", "tables_ms"), ("k_rhs_ms_2d", "rhs_2d_ms"), ("k_rhs_ms", "contraction_ms")):
                if name in ev.key:
                    total = getattr(ev, "device_time_total", None)
                    total = getattr(ev, "cuda_time_total", 0.0) if total is None else total
                    out[key] = round(out.get(key, 0.0) + total / 1e3, 4)
                    break
        return out or None
    except Exception as e:                        # (a measurement aid: the times above do not depend on it)
        return dict(error=repr(e))


def run(nb, counts):
    w = workload(3, nb, 0, nb)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    c = amd.create_from_branching_types(w["tree"])
    B = w["B"]
    cen = np.asarray(w["centers"], dtype=np.float64)
    kw = dict(centers=t(cen)[None, None], radii=t(np.ones(B))[None, None], k=t(w["ks"])[:, None], eta=t(w["etas"])[:, None],
              n_end=w["n_end"], alpha=w["alpha"], beta=w["beta"])
    fac = amd.biem_factorize(c, **kw)
    op, lib, L = fac._op, _biem.L.load(), _biem.L
    H, sp = op.plan.H, _biem._stream_ptr(op.dev)
    _, degrees = amd.harmonic_labels(c, w["n_end"])
    dipole = int(np.nonzero(degrees == 1)[0][-1])
    mid = cen.mean(axis=0)
    ring = np.linalg.norm(cen - mid, axis=-1).max() + 1.5               # 1.5 from the outermost centres: 0.5 off their unit spheres
    for nrhs in counts:
        ang = np.linspace(0.0, 2.0 * np.pi, nrhs, endpoint=False) + 0.1
        pos = np.tile(mid[:, None, None], (1, 1, nrhs))
        pos[0, 0] += ring * np.cos(ang)
        pos[1, 0] += ring * np.sin(ang)
        S = t(pos)
        f = torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)
        fl = op.fl
        ms, _ = _operator._multipole_source_source(op, _operator._check_multipole_source(c, kw["k"], w["n_end"], S, dipole, None, None, None, None))
        ps, _ = _operator._point_source_source(op, _operator._check_point_source_position(c, kw["k"], S, None, None, None))
        wb_ms, wb_ps = ms.workspace_bytes(op, nb), ps.workspace_bytes(op, nb)
        work = torch.empty(max(wb_ms, wb_ps, 16), dtype=torch.uint8, device="cuda")

        def rhs_multipole():
            L.check(lib.biem_rhs_multipole(op.plan.handle, nb, B, nrhs, _biem._ptr(fl.k), _biem._ptr(fl.centers), fl.geom_batched,
                                           _biem._ptr(fac._tab), _biem._ptr(ms.pts), ms.batched, _biem._ptr(ms.index), _biem._ptr(f), *strides,
                                           _biem._ptr(work), wb_ms, sp), "biem_rhs_multipole")

        def rhs_point_source():
            L.check(lib.biem_rhs_point_source(op.plan.handle, nb, B, nrhs, _biem._ptr(fl.k), _biem._ptr(fl.centers), fl.geom_batched,
                                              _biem._ptr(fac._tab), _biem._ptr(ps.pts), ps.batched, _biem._ptr(f), *strides,
                                              _biem._ptr(work), wb_ps, sp), "biem_rhs_point_source")

        per_pair = B * op.plan.H2 * 16
        rec = dict(systems=nb, balls=B, n_end=w["n_end"], sources=nrhs, dipole_index=dipole, workspace_bytes_multipole=wb_ms,
                   workspace_bytes_point_source=wb_ps, table_bytes_unsliced=nb * nrhs * per_pair,
                   slices=-(-nb * nrhs // max(1, wb_ms // per_pair)))
        rec["rhs_multipole_ms"] = timed(rhs_multipole)
        rec["rhs_point_source_ms"] = timed(rhs_point_source)
        rec["solve_multipole_ms"] = timed(lambda: fac.solve(multipole_source_position=S, multipole_source_index=dipole))
        rec["solve_point_source_ms"] = timed(lambda: fac.solve(point_source_position=S))
        rec["rhs_multipole_stages"] = stages(rhs_multipole)
        rec["rhs_share_of_solve"] = round(rec["rhs_multipole_ms"]["median"] / rec["solve_multipole_ms"]["median"], 3)
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
    fac.close()


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    run(args[0] if args else 256, args[1:] or [1, 64])
