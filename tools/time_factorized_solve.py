"""Times factor once, solve many against biem(): one JSON line per case.

python tools/time_factorized_solve.py [case ...]      cases: cfg3_batch (256 systems), cfg3_one, cfg2_one, cfg4_one (default: all)

Per case: biem_ms (the whole biem() call, one incidence per system), factorize_ms (biem_factorize), solve_ms for 1, 8 and 64
incidences per system (fac.solve), solve_bytes (the factor's upper triangle read twice, forward and back, plus the right-hand
sides read and written once each), solve_hbm_fraction (solve_bytes / solve time against 8 TB/s) and the largest difference of
the one-incidence densities from biem()'s, relative to their largest entry.  Every shape runs once before it is timed; times
are wall-clock around a device synchronisation, the minimum of `REPS` runs.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import biem_helmholtz_sphere_amd as amd  # noqa: E402
from bench import workload  # noqa: E402  (the configurations of the benchmark)

HBM = 8.0e12
REPS = 3
CASES = {"cfg3_batch": (3, 256), "cfg3_one": (3, 1), "cfg2_one": (2, 1), "cfg4_one": (4, 1)}


def timed(fn, reps=REPS):
    fn()                                           # warm-up of this shape
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def run(name, cfg, nb):
    w = workload(cfg, nb, 0, nb)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    c = amd.create_from_branching_types(w["tree"])
    d, B = w["d"], w["B"]
    kw = dict(centers=t(w["centers"])[None, None], radii=t(np.ones(B))[None, None], k=t(w["ks"])[:, None], eta=t(w["etas"])[:, None],
              n_end=w["n_end"], alpha=w["alpha"], beta=w["beta"])

    def field(nrhs):
        ang = np.linspace(0.0, np.pi, nrhs, endpoint=False)
        dirs = np.zeros((d, 1, nrhs))
        dirs[0, 0], dirs[1, 0] = np.cos(ang), np.sin(ang)
        u, g = amd.plane_wave(k=kw["k"], direction=t(dirs))
        return dict(uin=u, uin_grad=g if w["beta"] != 0 else None)

    reps_big = 1 if nb > 1 else REPS
    biem_ms, ref = timed(lambda: amd.biem(c, **kw, **field(1)).density, reps_big)
    torch.cuda.empty_cache()                       # biem()'s workspace and the kept factors do not fit side by side at cfg 3's batch
    fac = None

    def factorize():
        nonlocal fac
        if fac is not None:
            fac.close()
            fac = None
            torch.cuda.empty_cache()
        fac = amd.biem_factorize(c, **kw)
        return fac

    factorize_ms, _ = timed(factorize, reps_big)
    n_pad = int(fac._factors.shape[-1])
    rec = dict(case=name, systems=nb, N=B * fac._plan.H, n_pad=n_pad, n_symmetric=fac.n_symmetric, n_lu=fac.n_lu, factor_bytes=fac.nbytes,
               biem_ms=round(biem_ms, 3), factorize_ms=round(factorize_ms, 3), solve_ms={}, solve_bytes={}, solve_hbm_fraction={})
    for nrhs in (1, 8, 64):
        f = field(nrhs)
        ms, dens = timed(lambda: fac.solve(**f).density)
        byt = nb * (2 * (n_pad * n_pad / 2) * 16 + 2 * n_pad * nrhs * 16)
        rec["solve_ms"][nrhs] = round(ms, 4)
        rec["solve_bytes"][nrhs] = int(byt)
        rec["solve_hbm_fraction"][nrhs] = round(byt / (ms * 1e-3) / HBM, 4)
        if nrhs == 1:
            rec["max_rel_density_diff"] = float((dens - ref).abs().max() / ref.abs().max())
    rec["biem_over_solve_1"] = round(biem_ms / rec["solve_ms"][1], 2)
    fac.close()
    del ref
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    for name in sys.argv[1:] or list(CASES):
        run(name, *CASES[name])
