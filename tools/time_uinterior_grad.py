"""Times uinterior_grad() beside uinterior() at the same shape: the cfg-3 geometry (16 unit balls on a 4 x 4 lattice, n_end 20) with a
fluid in every ball (k_b = 1.5 k, density ratio 0.5), 100 x 100 points in the plane of the centres.
python tools/time_uinterior_grad.py [systems] [case] [repetitions]     case: mixed (a grid over the whole lattice: a fifth of the
points inside a ball) | inside (a grid lying entirely inside one ball) | all (default).  Per case: point-systems/s of the two calls
(median of the repetitions, default 7, after two warm-up calls of each, the two alternating), the spread, and the ratio of the times.
The yardstick for the ratio is d + 1 = 4: the calls of uinterior a one-sided difference scheme would need for the same d components
(and such a scheme reads NaN wherever its stencil crosses a surface)."""
import numpy as np, torch, time, sys
sys.path.insert(0, __file__.rsplit("/", 2)[0])
import biem_helmholtz_sphere_amd as amd
nsys = int(sys.argv[1]) if len(sys.argv) > 1 else 8
case = sys.argv[2] if len(sys.argv) > 2 else "all"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
t = lambda a: torch.as_tensor(np.array(a), dtype=torch.float64, device="cuda")
ks = np.linspace(0.5, 8.0, nsys)
ax = np.arange(-2, 2) * 4.0 + 2.0
x0, x1 = np.meshgrid(ax, ax, indexing="ij")
cen = np.stack([x0.ravel(), x1.ravel(), np.zeros(16)], -1)
dirs = np.zeros((3, nsys)); dirs[0] = 1
c = amd.create_from_branching_types("ba")
kb = torch.as_tensor(1.5 * ks[:, None] * np.ones(16), dtype=torch.complex128, device="cuda")
delta = t(0.5 * np.ones(16))
an, bn = amd.fluid_inclusion_bc(c_ndim=3, n_end=20, radii=t(np.ones(16)), k_interior=kb, density_ratio=delta, k=t(ks))
uin, ugr = amd.plane_wave(k=t(ks), direction=t(dirs))
calc = amd.biem(c, centers=t(cen)[None], radii=t(np.ones(16))[None], k=t(ks), n_end=20, alpha_n=an, beta_n=bn, uin=uin, uin_grad=ugr)


def once(fn, pts):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn(pts)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def timed(name, pts):
    fns = [("uinterior", lambda p: calc.uinterior(p, k_interior=kb, density_ratio=delta)),
           ("uinterior_grad", lambda p: calc.uinterior_grad(p, k_interior=kb, density_ratio=delta))]
    for _ in range(2):
        for _, fn in fns:
            once(fn, pts)
    ts, outs = {nm: [] for nm, _ in fns}, {}
    for _ in range(reps):
        for nm, fn in fns:
            dt, outs[nm] = once(fn, pts)
            ts[nm].append(dt)
    med = {nm: float(np.median(v)) for nm, v in ts.items()}
    n = pts[0].numel() * nsys
    nan = torch.isnan(outs["uinterior"].real)
    assert bool((torch.isnan(outs["uinterior_grad"].real) == nan[None]).all())      # NaN in every component exactly where the value is
    print("%-6s %d points x %d systems, %.3f of them inside a ball: " % (name, pts[0].numel(), nsys, float((~nan).float().mean())) + "  ".join(
        "%s %.4f s (%.2e point-systems/s, spread %.0f %%)" % (nm, med[nm], n / med[nm], 100 * (max(ts[nm]) - min(ts[nm])) / med[nm]) for nm, _ in fns)
        + "  uinterior_grad / uinterior %.2f (a difference scheme: d + 1 = 4)" % (med["uinterior_grad"] / med["uinterior"]), flush=True)


if case in ("mixed", "all"):
    g = np.linspace(-8, 8, 100)
    X, Y = np.meshgrid(g, g, indexing="ij")
    timed("mixed", t(np.stack([X, Y, np.zeros_like(X)])))
if case in ("inside", "all"):
    g = np.linspace(-0.7, 0.7, 100)
    X, Y = np.meshgrid(g, g, indexing="ij")
    timed("inside", t(np.stack([cen[5, 0] + X, cen[5, 1] + Y, np.zeros_like(X)])))
