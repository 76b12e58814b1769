"""Times point-source incidence in closed form against the sampled path, in one process: one JSON line per number of sources.

python tools/time_point_source_rhs.py [systems] [sources ...]      default: 256 systems of cfg 3 (ba, 16 balls, n_end 20), 1 and 64 sources

Per number of sources, median and spread (min, max) in ms of
  (a) sample_project:    _boundary_samples (the callables of point_source, n = 0, at the quadrature points) plus biem_rhs_project,
  (b) rhs_point_source:  biem_rhs_point_source alone, into the same natural layout,
  (c) solve_sampled:     fac.solve(uin=, uin_grad=),
  (d) solve_direct:      fac.solve(point_source_position=),
  (e) containment_check: the test |s - c_b| > rho_b on the device with its one synchronisation (part of (d)),
the bytes of the samples against the bytes of the sources, and the largest difference of the two densities relative to their largest
entry (the aliasing of the sampled right-hand side).  The sources stand on a circle around the cluster, half a radius off the nearest
surface.  Every step runs once before it is timed; times are wall-clock around a device synchronisation.
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


def run(nb, counts):
    w = workload(3, nb, 0, nb)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    c = amd.create_from_branching_types(w["tree"])
    d, B = w["d"], w["B"]
    cen = np.asarray(w["centers"], dtype=np.float64)
    kw = dict(centers=t(cen)[None, None], radii=t(np.ones(B))[None, None], k=t(w["ks"])[:, None], eta=t(w["etas"])[:, None],
              n_end=w["n_end"], alpha=w["alpha"], beta=w["beta"])
    fac = amd.biem_factorize(c, **kw)
    op, lib, L = fac._op, _biem.L.load(), _biem.L
    H, sp = op.plan.H, _biem._stream_ptr(op.dev)
    mid = cen.mean(axis=0)
    ring = np.linalg.norm(cen - mid, axis=-1).max() + 1.5               # 1.5 from the outermost centres: 0.5 off their unit spheres
    for nrhs in counts:
        ang = np.linspace(0.0, 2.0 * np.pi, nrhs, endpoint=False) + 0.1
        pos = np.tile(mid[:, None, None], (1, 1, nrhs))
        pos[0, 0] += ring * np.cos(ang)
        pos[1, 0] += ring * np.sin(ang)
        S = t(pos)
        uin, ugr = amd.point_source(k=kw["k"], source=S, n=0)
        ugr = ugr if w["beta"] != 0 else None
        f = torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device="cuda")
        strides = (nrhs * B * H, 1, B * H)

        def sample_project():
            g, _ = _operator._boundary_samples(op, uin, ugr)
            _operator._rhs_project(op, nb, g, 0, f, *strides, sp)
            return g

        src, _ = _operator._point_source_source(op, _operator._check_point_source_position(c, kw["k"], S, None, None, None))
        wb = src.workspace_bytes(op, nb)
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
        fl = op.fl

        def rhs_point_source():
            L.check(lib.biem_rhs_point_source(op.plan.handle, nb, B, nrhs, _biem._ptr(fl.k), _biem._ptr(fl.centers), fl.geom_batched,
                                              _biem._ptr(fac._tab), _biem._ptr(src.pts), src.batched, _biem._ptr(f), *strides,
                                              _biem._ptr(work), wb, sp), "biem_rhs_point_source")

        g = sample_project()
        sample_bytes = int(sum(x.numel() * 16 for x in (g if isinstance(g, tuple) else (g,)) if x is not None))
        del g
        rec = dict(systems=nb, balls=B, n_end=w["n_end"], sources=nrhs, sample_bytes=sample_bytes,
                   source_bytes=int(src.pts.numel() * 8), workspace_bytes=wb)
        rec["sample_project_ms"] = timed(sample_project)
        rec["rhs_point_source_ms"] = timed(rhs_point_source)
        rec["solve_sampled_ms"] = timed(lambda: fac.solve(uin=uin, uin_grad=ugr))
        rec["solve_direct_ms"] = timed(lambda: fac.solve(point_source_position=S))
        rec["containment_check_ms"] = timed(lambda: _operator._check_sources_outside(op, src.pts))
        old, new = fac.solve(uin=uin, uin_grad=ugr).density, fac.solve(point_source_position=S).density
        rec["max_rel_density_diff"] = float((old - new).abs().max() / old.abs().max())
        rec["rhs_speedup"] = round(rec["sample_project_ms"]["median"] / rec["rhs_point_source_ms"]["median"], 2)
        rec["solve_speedup"] = round(rec["solve_sampled_ms"]["median"] / rec["solve_direct_ms"]["median"], 2)
        del old, new
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
    fac.close()


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    run(args[0] if args else 256, args[1:] or [1, 64])
