"""Times incidence by expansion coefficients against the route it replaces, in one process: one JSON line per measurement.

python tools/time_expansion_rhs.py [systems] [coefficient vectors ...]   default: 256 systems of cfg 3 (ba, 16 balls, n_end 20), 1 and 64

Per order n_in of the coefficients (n_end and n_end + 6), number of coefficient vectors and form (one origin, the middle of the
cluster, shared by all vectors of a system / every vector about its own origin), median and spread (min, max) in ms of
  rhs_expansion:   biem_rhs_expansion alone, into the natural layout, and its two stages alone (table rows; contraction);
  solve:           fac.solve(regular_wave_origin=, regular_wave_coefficients=) end to end;
and once
  rhs_regular_wave_one_index / solve_one_index: biem_rhs_regular_wave and fac.solve of ONE harmonic, the unit both are measured in;
  solve_all_and_combine: the only route without the coefficients - fac.solve of all H regular waves about the middle plus the
                   combination of their densities with one coefficient vector per system.
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


def run(nb, counts, with_all=True):
    w = workload(3, nb, 0, nb)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    c = amd.create_from_branching_types(w["tree"])
    B, n_end = w["B"], w["n_end"]
    cen = np.asarray(w["centers"], dtype=np.float64)
    kw = dict(centers=t(cen)[None, None], radii=t(np.ones(B))[None, None], k=t(w["ks"])[:, None], eta=t(w["etas"])[:, None],
              n_end=n_end, alpha=w["alpha"], beta=w["beta"])
    fac = amd.biem_factorize(c, **kw)
    op, lib, L = fac._op, _biem.L.load(), _biem.L
    H, sp, fl, ptr = op.plan.H, _biem._stream_ptr(op.dev), op.fl, _biem._ptr
    mid = cen.mean(axis=0)
    base = dict(systems=nb, balls=B, n_end=n_end, H=H)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for n_in in (n_end, n_end + 6):
        H_in = n_in * n_in
        for nrhs in counts:
            P = torch.randn((nb, nrhs, H_in), dtype=torch.complex128, device="cuda", generator=gen)
            f = torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device="cuda")
            strides = (nrhs * B * H, 1, B * H)
            for form in ("shared", "own") if nrhs > 1 else ("shared",):
                pos = np.tile(mid[:, None, None], (1, 1, nrhs if form == "own" else 1))
                if form == "own":
                    pos[0, 0] += 0.05 * np.arange(nrhs)
                org = t(pos)
                g, _ = _operator._expansion_source(op, _operator._check_expansion(c, kw["k"], org, P, None, (), "regular_wave_origin",
                                                                                  "regular_wave_coefficients", "regular_wave_index"), True)
                wb = g.workspace_bytes(op, nb)
                work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")

                def rhs(stage):
                    return lambda: L.check(lib.biem_rhs_expansion(op.plan.handle, nb, B, nrhs, ptr(fl.k), ptr(fl.centers), fl.geom_batched,
                                                                  ptr(fac._tab), *g.source_args(), ptr(f), *strides, stage, ptr(work), wb, sp),
                                           "biem_rhs_expansion")

                rec = dict(base, n_in=n_in, coefficient_vectors=nrhs, origins=form, table_slices=-(-nb * int(g.pts.shape[1]) * B * g.lists.H2 * 16 // max(wb, 1)))
                rec["rhs_expansion_ms"] = timed(rhs(0))
                rec["tables_ms"] = timed(rhs(1))
                rec["contraction_ms"] = timed(rhs(2))
                del work
                rec["solve_ms"] = timed(lambda: fac.solve(regular_wave_origin=org, regular_wave_coefficients=P))
                rec["rhs_share_of_solve"] = round(rec["rhs_expansion_ms"]["median"] / rec["solve_ms"]["median"], 4)
                torch.cuda.empty_cache()
                print(json.dumps(rec), flush=True)
            del f, P
    # the unit: one harmonic by its index
    org1 = t(mid[:, None, None])
    rw, _ = _operator._regular_wave_source(op, _operator._check_multipole_source(c, kw["k"], n_end, org1, 1, None, None, None, None,
                                                                                "regular_wave_origin", "regular_wave_index"))
    wb = rw.workspace_bytes(op, nb)
    work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    f = torch.empty((nb, 1, B * H), dtype=torch.complex128, device="cuda")
    rec = dict(base)
    rec["rhs_regular_wave_one_index_ms"] = timed(lambda: L.check(lib.biem_rhs_regular_wave(
        op.plan.handle, nb, B, 1, ptr(fl.k), ptr(fl.centers), fl.geom_batched, ptr(fac._tab), ptr(rw.pts), rw.batched, ptr(rw.index), ptr(f),
        B * H, 1, B * H, ptr(work), wb, sp), "biem_rhs_regular_wave"))
    rec["solve_one_index_ms"] = timed(lambda: fac.solve(regular_wave_origin=org1, regular_wave_index=1))
    del work, f
    if with_all:
        allw = t(np.tile(mid[:, None, None], (1, 1, H)))
        idx = np.arange(H)[None, :]
        p1 = torch.randn((nb, H), dtype=torch.complex128, device="cuda", generator=gen)
        rec["solve_all_and_combine_ms"] = timed(
            lambda: torch.einsum("sh,shbn->sbn", p1, fac.solve(regular_wave_origin=allw, regular_wave_index=idx).density), reps=2)
        one = timed(lambda: fac.solve(regular_wave_origin=org1, regular_wave_coefficients=p1[:, None, :]))
        rec["solve_one_vector_ms"] = one
        rec["all_and_combine_over_one_vector"] = round(rec["solve_all_and_combine_ms"]["median"] / one["median"], 1)
    print(json.dumps(rec), flush=True)
    fac.close()


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    run(args[0] if args else 256, args[1:] or [1, 64])
