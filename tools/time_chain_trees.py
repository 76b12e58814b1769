"""Times the standard chain trees "b" * (d - 2) + "a" beside cfg 3 (ba, 16 balls, n_end 20): one JSON line per case with the plan-build
seconds, the term count, the stage times of the library's profiler (pair tables, fill, factorisation; ms per call), systems/s of
biem(), and the field evaluation (point-systems/s, and harmonic terms per second = point-systems x balls x H).
python tools/time_chain_trees.py [systems]      (default 256)"""
import ctypes as C
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import biem_helmholtz_sphere_amd as amd  # noqa: E402
from biem_helmholtz_sphere_amd import _lib  # noqa: E402

nsys = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dev = "cuda"
t = lambda a: torch.as_tensor(np.array(a), dtype=torch.float64, device=dev)  # noqa: E731
CLASSES = ["tables", "fill", "rhs", "panel", "swap", "trsm", "gemm", "back", "other"]


def grid16(d):
    ax = np.arange(-2, 2) * 4.0 + 2.0
    x0, x1 = np.meshgrid(ax, ax, indexing="ij")
    return np.stack([x0.ravel(), x1.ravel()] + [np.zeros(16)] * (d - 2), -1)


def case(label, bt, d, n_end, cen, ns):
    lib = _lib.load()
    B = len(cen)
    t0 = time.time()
    p = C.c_void_p()
    if d >= 5:
        _lib.check(lib.biem_plan_create_chain_host(d, n_end, C.byref(p)))
    else:
        _lib.check(lib.biem_plan_create_host(1, n_end, C.byref(p)))
    build_s = time.time() - t0
    H, nt = C.c_int(), C.c_longlong()
    lib.biem_plan_info(p, None, C.byref(H), None, None, C.byref(nt))
    lib.biem_plan_destroy(p)
    ks = np.linspace(0.5, 2.0, ns)
    dirs = np.zeros((d, ns))
    dirs[0] = 1
    uin, ugr = amd.plane_wave(k=t(ks), direction=t(dirs))
    c = amd.create_from_branching_types(bt)
    kw = dict(centers=t(cen)[None], radii=t(np.ones(B))[None], k=t(ks), n_end=n_end, uin=uin, uin_grad=ugr)
    calc = amd.biem(c, **kw)                                       # warm-up (plan, workspace)
    torch.cuda.synchronize()
    lib.biem_profile_begin()
    t0 = time.time()
    calc = amd.biem(c, **kw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    ms, work, launches = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_longlong * 9)()
    lib.biem_profile_end(ms, work, launches)
    g = np.linspace(-12, 12, 32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    pts = t(np.stack([X, Y] + [0.3 * np.ones_like(X)] * (d - 2)))
    calc.uscat(pts)
    torch.cuda.synchronize()
    t0 = time.time()
    calc.uscat(pts)
    torch.cuda.synchronize()
    du = time.time() - t0
    ps = pts[0].numel() * ns / du
    print(json.dumps(dict(case=label, tree=bt, d=d, n_end=n_end, balls=B, N=B * H.value, systems=ns, plan_build_s=round(build_s, 3),
                          terms=nt.value, stage_ms={CLASSES[i]: round(ms[i], 3) for i in range(9) if ms[i] > 0},
                          fill_ms_per_system=round((ms[0] + ms[1]) / ns, 4), systems_per_s=round(ns / dt, 2),
                          uscat_point_systems_per_s=float("%.3e" % ps), uscat_terms_per_s=float("%.3e" % (ps * B * H.value)))),
          flush=True)


case("cfg3", "ba", 3, 20, grid16(3), nsys)
case("d5", "bbba", 5, 7, grid16(5), nsys)
case("d6", "bbbba", 6, 5, grid16(6)[:8], 64)
case("d7", "bbbbba", 7, 4, grid16(7)[:8], 64)
