"""Times the library entry biem_force beside biem_power at the same shape: the benchmark's configuration 3 (tree ba, 16 unit balls,
n_end 20: H = 400), 256 systems, with 1 and with 64 right-hand sides per system.
python tools/time_force.py [systems] [repetitions]
biem_force reads the density, one [nb][nrhs][B][H] complex array, once from memory (and again through the cache for the neighbour
degrees of every row) and the plan's coupling table (3610 entries at this order, shared by every wave); biem_power reads the density
and two projections.  Operands are random (the time does not depend on the values; the tables are those of biem_ball_tables for Robin
coefficients).  The first biem_force call builds and uploads the coupling table and is timed on its own.  Per shape: the median of the
repetitions (default 9, the two calls alternating, after two warm-up calls of each) in ms, the spread and the ratio of the times.  A
call is timed from the host around a device synchronisation, so each entry's own wait for the wavenumbers is included."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import biem_helmholtz_sphere_amd as amd  # noqa: E402,F401
from biem_helmholtz_sphere_amd import _biem, _lib as L  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
B, n_end = 16, 20
dev = torch.device("cuda", torch.cuda.current_device())
lib = L.load()
plan = _biem._plan("ba", n_end, dev)
H, d = plan.H, plan.d
ptr, sp = _biem._ptr, _biem._stream_ptr(dev)
gen = torch.Generator(device=dev).manual_seed(0)
rand = lambda *shape: torch.randn(*shape, dtype=torch.complex128, device=dev, generator=gen)
k = torch.linspace(0.5, 8.0, nb, dtype=torch.float64, device=dev).to(torch.complex128)
eta = torch.ones(nb, dtype=torch.float64, device=dev)
radii = torch.ones((1, B), dtype=torch.float64, device=dev)
alpha = torch.full((1, B), 1.0 + 0.5j, dtype=torch.complex128, device=dev)
beta = torch.full((1, B), 0.3 - 0.2j, dtype=torch.complex128, device=dev)
tab = torch.empty((nb, B, 3, n_end), dtype=torch.complex128, device=dev)
L.check(lib.biem_ball_tables(plan.handle, nb, B, ptr(k), ptr(eta), ptr(radii), 0, ptr(alpha), ptr(beta), 0, ptr(tab), sp), "biem_ball_tables")


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


first = True
for nrhs in (1, 64):
    dens, pu, pv = rand(nb, nrhs, B, H), rand(nb, nrhs, B, H), rand(nb, nrhs, B, H)
    out_f = torch.empty((nb, nrhs, B, d), dtype=torch.float64, device=dev)
    out_p = torch.empty((nb, nrhs, B, 2), dtype=torch.float64, device=dev)
    fns = {
        "biem_force": lambda: L.check(lib.biem_force(plan.handle, nb, B, nrhs, ptr(k), ptr(eta), ptr(radii), 0, ptr(alpha), ptr(beta), 0, ptr(tab),
                                                     ptr(dens), ptr(out_f), sp), "biem_force"),
        "biem_power": lambda: L.check(lib.biem_power(plan.handle, nb, B, nrhs, ptr(k), ptr(eta), ptr(radii), 0, ptr(alpha), ptr(beta), 0, ptr(tab),
                                                     ptr(dens), ptr(pu), ptr(pv), ptr(out_p), sp), "biem_power"),
    }
    if first:
        print("first biem_force call (builds and uploads the coupling table): %.1f ms" % once(fns["biem_force"]), flush=True)
        first = False
    for _ in range(2):
        for fn in fns.values():
            once(fn)
    ts = {nm: [] for nm in fns}
    for _ in range(reps):
        for nm, fn in fns.items():
            ts[nm].append(once(fn))
    assert bool(torch.isfinite(out_f).all()) and bool(torch.isfinite(out_p).all())
    med = {nm: float(np.median(v)) for nm, v in ts.items()}
    print("%d systems x %d right-hand sides x %d balls x n_end %d: " % (nb, nrhs, B, n_end) + "  ".join(
        "%s %.3f ms (spread %.0f %%)" % (nm, med[nm], 100 * (max(v) - min(v)) / med[nm]) for nm, v in ts.items())
        + "  biem_force / biem_power %.3f" % (med["biem_force"] / med["biem_power"]), flush=True)
    del dens, pu, pv, out_f, out_p
