"""Times biem() with degree-dependent boundary coefficients against the scalar call, here and at another checkout.

python tools/time_degree_bc.py [--other-root DIR] [--rounds R] [--systems NB]

The shape is the benchmark's configuration 3 (16 balls, n_end 20, NB = 256 wavenumbers, one plane wave per system).  Three cases:
  scalar@other  biem(alpha=1, beta=0) of the package under DIR (a checkout of the parent commit with its library built)
  scalar        the same call of this checkout
  fluid         biem(alpha_n=, beta_n=) of this checkout, every ball a fluid inclusion (k_b = 1.5 k, density ratio 0.5)
Every measurement is a process of its own (python tools/time_degree_bc.py --case NAME --root DIR), started in turn, R rounds of
other / scalar / fluid / ..., so that drift of the device (clocks, temperature) falls on all cases alike.  A process runs its
call once to warm up, then times it `REPS` times around a device synchronisation and, with the library's event profiler on, once
more for the stage times.  The last line is a JSON summary: per case the median over the rounds of the per-process minimum, the
ratios fluid / scalar and scalar / scalar@other, and the stage times (ms) tables / fill / rhs / rest of the last round.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 2
STAGES = ["tables", "fill", "rhs", "panel", "swap", "trsm", "gemm", "back", "other"]


def measure(case: str, root: str, nb: int) -> dict:
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import biem_helmholtz_sphere_amd as amd
    from biem_helmholtz_sphere_amd import _lib as L
    from bench import workload

    w = workload(3, nb, 0, nb)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    c = amd.create_from_branching_types(w["tree"])
    B, n_end = w["B"], w["n_end"]
    kw = dict(centers=t(w["centers"])[None], radii=t(np.ones(B))[None], k=t(w["ks"]), eta=t(w["etas"]), n_end=n_end)
    dirs = np.zeros((w["d"], nb))
    dirs[0] = 1.0
    uin, ugr = amd.plane_wave(k=kw["k"], direction=t(dirs))
    if case == "fluid":
        an, bn = amd.fluid_inclusion_bc(c_ndim=w["d"], n_end=n_end, radii=kw["radii"], k_interior=1.5 * kw["k"][:, None], density_ratio=0.5)
        kw.update(alpha_n=an, beta_n=bn, uin=uin, uin_grad=ugr)
    else:
        kw.update(alpha=1.0, beta=0.0, uin=uin)

    def call():
        d = amd.biem(c, **kw).density
        torch.cuda.synchronize()
        return d

    dens = call()
    finite = bool(torch.isfinite(dens.real).all() and torch.isfinite(dens.imag).all())
    del dens
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    lib = L.load()
    ms = (C.c_double * 9)()
    lib.biem_profile_begin()
    call()
    lib.biem_profile_end(ms, None, None)
    from biem_helmholtz_sphere_amd import _biem
    return dict(case=case, root=os.path.relpath(root, ROOT), systems=nb, ms=round(min(times), 2), all_ms=[round(x, 2) for x in times], finite=finite,
                lu_systems=_biem._last_solve_stats.get("lu_systems"), stages_ms={n: round(v, 2) for n, v in zip(STAGES, ms)})


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--other-root", default=None, help="a checkout of the commit to compare with, its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--case", default=None, help="(one measurement in this process) scalar or fluid")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(measure(a.case, os.path.abspath(a.root), a.systems)), flush=True)
        return
    order = ([("scalar@other", "scalar", os.path.abspath(a.other_root))] if a.other_root else []) + [("scalar", "scalar", ROOT), ("fluid", "fluid", ROOT)]
    runs = {name: [] for name, _, _ in order}
    for _ in range(a.rounds):
        for name, case, root in order:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--root", root, "--systems", str(a.systems)],
                                 check=True, capture_output=True, text=True, cwd=root, timeout=600).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            rec["case"] = name
            print(json.dumps(rec), flush=True)
            runs[name].append(rec)
    med = {name: statistics.median(r["ms"] for r in rs) for name, rs in runs.items()}
    summary = dict(summary=True, systems=a.systems, rounds=a.rounds, median_ms={n: round(v, 2) for n, v in med.items()},
                   fluid_over_scalar=round(med["fluid"] / med["scalar"], 4),
                   stages_ms={n: rs[-1]["stages_ms"] for n, rs in runs.items()})
    if a.other_root:
        summary["scalar_over_other"] = round(med["scalar"] / med["scalar@other"], 4)
        summary["fluid_over_other"] = round(med["fluid"] / med["scalar@other"], 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
