"""Times uscat_grad() beside uscat() on the cases and the 100 x 100 grid of tools/time_uscat.py.
python tools/time_uscat_grad.py [systems] [case] [repetitions]     case: ba (cfg 3 densities) | caa (4-D, 8 balls, n_end 8) | inner (one ball, ba,
n_end 20, points inside) | all (default).  Per case: point-systems/s of both (median of the repetitions, default 7, after two warm-up
calls of each, the two alternating) and the ratio of the times - what a gradient costs in units of one field evaluation; the cheapest
difference scheme of uscat() costs d + 1."""
import numpy as np, torch, time, sys
sys.path.insert(0, __file__.rsplit("/", 2)[0])
import biem_helmholtz_sphere_amd as amd
nsys = int(sys.argv[1]) if len(sys.argv) > 1 else 8
case = sys.argv[2] if len(sys.argv) > 2 else "all"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
t = lambda a: torch.as_tensor(np.array(a), dtype=torch.float64, device="cuda")
ks = np.linspace(0.5, 8.0, nsys)
g = np.linspace(-12, 12, 100)
X, Y = np.meshgrid(g, g, indexing="ij")


def once(fn, pts):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn(pts)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def timed(name, calc, pts):
    d = pts.shape[0]
    for _ in range(2):
        once(calc.uscat, pts); once(calc.uscat_grad, pts)
    tu, tg = [], []
    for _ in range(reps):
        dt, u = once(calc.uscat, pts); tu.append(dt)
        dt, gr = once(calc.uscat_grad, pts); tg.append(dt)
    mu, mg = float(np.median(tu)), float(np.median(tg))
    n = pts[0].numel() * nsys
    assert bool((torch.isnan(gr.real) == torch.isnan(u.real)[None]).all())
    print("%-6s %d points x %d systems: uscat %.4f s (%.2e point-systems/s, spread %.0f %%)  uscat_grad %.4f s (%.2e point-systems/s, spread %.0f %%)"
          "  ratio %.2f (d + 1 = %d), nan fraction %.2f" % (
              name, pts[0].numel(), nsys, mu, n / mu, 100 * (max(tu) - min(tu)) / mu, mg, n / mg, 100 * (max(tg) - min(tg)) / mg, mg / mu, d + 1,
              float(torch.isnan(u.real).float().mean())), flush=True)


if case in ("ba", "all"):
    ax = np.arange(-2, 2) * 4.0 + 2.0
    x0, x1 = np.meshgrid(ax, ax, indexing="ij")
    cen = np.stack([x0.ravel(), x1.ravel(), np.zeros(16)], -1)
    dirs = np.zeros((3, nsys)); dirs[0] = 1
    uin, _ = amd.plane_wave(k=t(ks), direction=t(dirs))
    calc = amd.biem(amd.create_from_branching_types("ba"), centers=t(cen)[None], radii=t(np.ones(16))[None], k=t(ks), n_end=20, uin=uin)
    timed("ba", calc, t(np.stack([X, Y, 0.3 * np.ones_like(X)])))
if case in ("caa", "all"):
    cen = np.zeros((8, 4)); cen[:, 0] = 3.0 * (np.arange(8) % 4) - 4.5; cen[:, 2] = 3.0 * (np.arange(8) // 4) - 1.5
    dirs = np.zeros((4, nsys)); dirs[0] = 1
    uin, _ = amd.plane_wave(k=t(ks), direction=t(dirs))
    calc = amd.biem(amd.create_from_branching_types("caa"), centers=t(cen)[None], radii=t(np.ones(8))[None], k=t(ks), n_end=8, uin=uin)
    timed("caa", calc, t(np.stack([X, 0.2 * np.ones_like(X), Y, 0.3 * np.ones_like(X)])))
if case in ("inner", "all"):
    dirs = np.zeros((3, nsys)); dirs[0] = 1
    uin, _ = amd.plane_wave(k=t(ks), direction=t(dirs))
    calc = amd.biem(amd.create_from_branching_types("ba"), centers=t(np.zeros((1, 3)))[None], radii=t([12.0 * 1.5])[None], k=t(ks), n_end=20,
                    uin=uin, kind="inner")
    timed("inner", calc, t(np.stack([X, Y, 0.3 * np.ones_like(X)])))
