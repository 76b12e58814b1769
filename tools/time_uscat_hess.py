"""Times uscat_hess() beside uscat() and uscat_grad() on the cases and the 100 x 100 grid of tools/time_uscat_grad.py.
python tools/time_uscat_hess.py [systems] [case] [repetitions]     case: ba (cfg 3 densities: 16 balls, n_end 20) | caa (4-D, 8 balls, n_end 8) |
all (default).  Per case: the build time of the plan of order n_end + 2 (the first uscat_hess call of a tree and order builds it, fill
lists included, and caches it), then the median time of the three (default 9 repetitions after two warm-up calls of each, the three
alternating) with spreads, and the ratios hess / uscat and hess / ((d + 1) uscat_grad) - the cheapest difference scheme of the Hessian
there was before costs d + 1 gradient calls."""
import numpy as np, torch, time, sys
sys.path.insert(0, __file__.rsplit("/", 2)[0])
import biem_helmholtz_sphere_amd as amd
from biem_helmholtz_sphere_amd._plans import _plan
nsys = int(sys.argv[1]) if len(sys.argv) > 1 else 8
case = sys.argv[2] if len(sys.argv) > 2 else "all"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
t = lambda a: torch.as_tensor(np.array(a), dtype=torch.float64, device="cuda")
ks = np.linspace(0.5, 8.0, nsys)
g = np.linspace(-12, 12, 100)
X, Y = np.meshgrid(g, g, indexing="ij")


def once(fn, pts):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn(pts)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def timed(name, tree, n_end, calc, pts):
    d = pts.shape[0]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    _plan(tree, n_end + 2, pts.device)
    torch.cuda.synchronize()
    print("%-6s plan of order %d built in %.2f s" % (name, n_end + 2, time.perf_counter() - t0), flush=True)
    fns = (calc.uscat, calc.uscat_grad, calc.uscat_hess)
    dt, _ = once(calc.uscat_hess, pts)
    print("%-6s first uscat_hess call (label map, force coupling table of the plan) %.2f s" % (name, dt), flush=True)
    for _ in range(2):
        for fn in fns:
            once(fn, pts)
    times, outs = [[], [], []], [None] * 3
    for _ in range(reps):
        for i, fn in enumerate(fns):
            dt, outs[i] = once(fn, pts); times[i].append(dt)
    med = [float(np.median(x)) for x in times]
    spread = [100 * (max(x) - min(x)) / m for x, m in zip(times, med)]
    n = pts[0].numel() * nsys
    u, gr, H = outs
    assert bool((torch.isnan(H.real) == torch.isnan(u.real)[None, None]).all())
    v = ~torch.isnan(u.real)
    res = (sum(H[i, i] for i in range(d)) + torch.as_tensor(ks, device=u.device) ** 2 * u)[v].abs().max() / H[:, :, v].abs().max()
    print("%-6s %d points x %d systems: uscat %.4f s (%.2e point-systems/s, spread %.0f %%)  uscat_grad %.4f s (spread %.0f %%)  uscat_hess %.4f s "
          "(%.2e point-systems/s, spread %.0f %%)\n       hess / uscat %.2f (d (d + 1) / 2 = %d field evaluations at order n_end + 2), "
          "hess / ((d + 1) uscat_grad) %.2f, |tr H + k^2 u| %.1e of max|H|, nan fraction %.2f" % (
              name, pts[0].numel(), nsys, med[0], n / med[0], spread[0], med[1], spread[1], med[2], n / med[2], spread[2], med[2] / med[0],
              d * (d + 1) // 2, med[2] / ((d + 1) * med[1]), float(res), float(torch.isnan(u.real).float().mean())), flush=True)


if case in ("ba", "all"):
    ax = np.arange(-2, 2) * 4.0 + 2.0
    x0, x1 = np.meshgrid(ax, ax, indexing="ij")
    cen = np.stack([x0.ravel(), x1.ravel(), np.zeros(16)], -1)
    dirs = np.zeros((3, nsys)); dirs[0] = 1
    uin, _ = amd.plane_wave(k=t(ks), direction=t(dirs))
    calc = amd.biem(amd.create_from_branching_types("ba"), centers=t(cen)[None], radii=t(np.ones(16))[None], k=t(ks), n_end=20, uin=uin)
    timed("ba", "ba", 20, calc, t(np.stack([X, Y, 0.3 * np.ones_like(X)])))
if case in ("caa", "all"):
    cen = np.zeros((8, 4)); cen[:, 0] = 3.0 * (np.arange(8) % 4) - 4.5; cen[:, 2] = 3.0 * (np.arange(8) // 4) - 1.5
    dirs = np.zeros((4, nsys)); dirs[0] = 1
    uin, _ = amd.plane_wave(k=t(ks), direction=t(dirs))
    calc = amd.biem(amd.create_from_branching_types("caa"), centers=t(cen)[None], radii=t(np.ones(8))[None], k=t(ks), n_end=8, uin=uin)
    timed("caa", "caa", 8, calc, t(np.stack([X, 0.2 * np.ones_like(X), Y, 0.3 * np.ones_like(X)])))
