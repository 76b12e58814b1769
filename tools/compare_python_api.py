#!/usr/bin/env python3
"""The public Python API on a fixed list of small seeded cases, as text that two checkouts can be compared by (needs a GPU).

    python tools/compare_python_api.py run > OUT        one line per case, from the checkout this file lies in
    python tools/compare_python_api.py diff OLD NEW      "identical" / "DIFFERENT" per case, exit 1 on a difference

A line holds, for one case: the sha256 of every array the case returned (density, fields, powers, forces, matrix), the solve
statistics, n_symmetric / n_lu of a factorisation, and the launches and work per class between biem_profile_begin and
biem_profile_end.  The tool does not run another checkout's code itself: run it once from each, each in a process of its own.
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

CLASSES = ["tables", "fill", "rhs", "panel", "swap", "trsm", "gemm", "back", "other"]


def run():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import numpy as np
    import torch

    import biem_helmholtz_sphere_amd as amd
    from biem_helmholtz_sphere_amd import _biem, _lib as L

    lib = L.load()
    rng = np.random.default_rng(11)
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.asarray(a), dtype=dt, device="cuda")

    def sha(a):
        kind = f"{type(a).__name__}@{a.device}" if isinstance(a, torch.Tensor) else type(a).__name__
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return f"{kind} {a.dtype}{list(a.shape)}:" + hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]

    @contextlib.contextmanager
    def env(**kw):
        old = {k: os.environ.get(k) for k in kw}
        os.environ.update(kw)
        try:
            yield
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def case(name, fn):
        _biem._last_solve_stats.clear()
        torch.cuda.synchronize()
        L.check(lib.biem_profile_begin())
        try:
            out = fn()
        except Exception as e:  # noqa: BLE001  (an exception is a result like any other: both checkouts must raise the same)
            out = {"raised": f"{type(e).__name__}: {e}"}
        torch.cuda.synchronize()
        ms, work, launches = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_longlong * 9)()
        L.check(lib.biem_profile_end(ms, work, launches))
        prof = {c: [int(launches[i]), float(work[i])] for i, c in enumerate(CLASSES) if launches[i]}
        rec = {k: (v if isinstance(v, (int, str)) else sha(v)) for k, v in out.items()}
        print(json.dumps({"case": name, "out": rec, "stats": dict(_biem._last_solve_stats), "profile": prof}, sort_keys=True), flush=True)

    # geometry: B balls on the y axis (tree ba / bpa, d = 3) or in the plane (tree a), radii 1, gaps 0.4
    def geom(B, d=3):
        cen = np.zeros((B, d))
        cen[:, 1] = 2.4 * np.arange(B) - 1.2 * (B - 1)
        cen[:, 0] = 0.1 * rng.standard_normal(B)
        return cen, 1.0 + 0.1 * rng.random(B)

    ba, bpa, a2 = (amd.create_from_branching_types(t) for t in ("ba", "bpa", "a"))
    cen3, rad3 = geom(3)
    cen2, rad2 = geom(2)
    ks = np.array([1.0, 1.7, 2.3])
    dirs = np.array([[1.0, 0.3, -0.2]] * 3).T                         # (3, 3): one direction per system
    uin3, ugr3 = amd.plane_wave(k=dev(ks), direction=dev(dirs))
    kw3 = dict(centers=dev(cen3)[None], radii=dev(rad3)[None], k=dev(ks), eta=dev(np.ones(3)), n_end=6)
    dens = lambda calc: {"density": calc.density}

    case("biem default", lambda: dens(amd.biem(ba, uin=uin3, **kw3)))
    case("biem default, with matrix", lambda: (lambda r: {"density": r.density, "matrix": r.matrix})(amd.biem(ba, uin=uin3, **kw3)))
    with env(BIEM_SOLVER="lu"):
        case("biem BIEM_SOLVER=lu", lambda: dens(amd.biem(ba, uin=uin3, **kw3)))
    with env(BIEM_LDLT_PIVOT_REL="1e30"):
        case("biem every system rejected", lambda: dens(amd.biem(ba, uin=uin3, **kw3)))
    kw1 = dict(centers=dev(cen3[:1])[None], radii=dev(rad3[:1])[None], k=dev(ks), eta=dev(np.ones(3)), n_end=6)
    case("biem single ball", lambda: dens(amd.biem(ba, uin=uin3, **kw1)))
    case("biem single ball, force_matrix", lambda: dens(amd.biem(ba, uin=uin3, force_matrix=True, **kw1)))
    case("biem no incident field", lambda: (lambda r: {"density": str(r.density), "matrix": r.matrix})(amd.biem(ba, **kw3)))
    uin0, _ = amd.plane_wave(k=dev(np.zeros(0)), direction=dev(np.zeros((3, 0))))
    case("biem empty batch axis", lambda: dens(amd.biem(ba, uin=uin0, centers=dev(cen2)[None], radii=dev(rad2)[None], k=dev(np.zeros(0)),
                                                        eta=dev(np.zeros(0)), n_end=5)))
    case("biem chunk=1, 3 systems", lambda: dens(amd.biem(ba, uin=uin3, chunk=1, **kw3)))
    with env(BIEM_MAX_RESIDENT_BYTES="3000000"):
        case("biem BIEM_MAX_RESIDENT_BYTES", lambda: dens(amd.biem(ba, uin=uin3, **kw3)))
    fluid = dict(k_interior=dev(np.array([1.3, 0.8 + 0.1j, 2.0]), torch.complex128), density_ratio=dev([0.7, 1.4, 2.0]))
    a_n, b_n = amd.fluid_inclusion_bc(c_ndim=3, n_end=6, radii=dev(rad3), k=dev(ks), **{k: v[None] for k, v in fluid.items()})
    case("fluid_inclusion_bc", lambda: {"alpha_n": a_n, "beta_n": b_n})
    case("biem alpha_n / beta_n", lambda: dens(amd.biem(ba, uin=uin3, uin_grad=ugr3, alpha_n=a_n, beta_n=b_n, **kw3)))
    with env(BIEM_LDLT_PIVOT_REL="1e30"):
        case("biem alpha_n / beta_n, every system rejected", lambda: dens(amd.biem(ba, uin=uin3, uin_grad=ugr3, alpha_n=a_n, beta_n=b_n, **kw3)))
    # the incident field varies along a batch axis on which the operator has size 1: 4 directions, 2 wavenumbers, one geometry
    k21 = dev(np.array([[1.1], [1.9]]))
    d4 = rng.standard_normal((3, 1, 4))
    uin_r, ugr_r = amd.plane_wave(k=k21, direction=dev(d4))
    kwr = dict(centers=dev(cen2)[None, None], radii=dev(rad2)[None, None], k=k21, eta=dev(np.ones((1, 1))), n_end=7)
    case("biem right-hand-side axis", lambda: dens(amd.biem(ba, uin=uin_r, uin_grad=ugr_r, alpha=1.0, beta=0.3, **kwr)))
    kwp = dict(kw3, centers=dev(cen3[:, [1, 0, 2]])[None])
    case("biem primed tree bpa", lambda: dens(amd.biem(bpa, uin=uin3, **kwp)))
    uin_np, ugr_np = amd.plane_wave(k=ks, direction=dirs)
    kwn = dict(centers=cen3[None], radii=rad3[None], k=ks, eta=np.ones(3), n_end=6)
    case("biem NumPy inputs", lambda: dens(amd.biem(ba, uin=uin_np, **kwn)))
    case("biem tree a, 4 balls", lambda: dens(amd.biem(a2, uin=amd.plane_wave(k=dev(ks), direction=dev(dirs[:2]))[0], centers=dev(geom(4, 2)[0])[None],
                                                       radii=dev(np.ones(4))[None], k=dev(ks), eta=dev(np.ones(3)), n_end=8)))
    case("biem same shape again (memo)", lambda: dens(amd.biem(ba, uin=uin3, **kw3)))
    case("biem same shape a third time (memo)", lambda: dens(amd.biem(ba, uin=uin3, **kw3)))

    def factored(c, kw, solve, **pre):
        with env(**pre):
            fac = amd.biem_factorize(c, **kw)
        res = fac.solve(**solve)
        return {"density": res.density, "n_symmetric": fac.n_symmetric, "n_lu": fac.n_lu, "nbytes": fac.nbytes}

    case("factorize symmetric", lambda: factored(ba, kw3, dict(uin=uin3)))
    case("factorize rhs axis", lambda: factored(ba, dict(kwr, alpha=1.0, beta=0.3), dict(uin=uin_r, uin_grad=ugr_r)))
    case("factorize LU form", lambda: factored(ba, kw3, dict(uin=uin3), BIEM_LDLT_PIVOT_REL="1e30"))
    case("factorize BIEM_SOLVER=lu", lambda: factored(ba, kw3, dict(uin=uin3), BIEM_SOLVER="lu"))
    case("factorize degree-dependent", lambda: factored(ba, dict(kw3, alpha_n=a_n, beta_n=b_n), dict(uin=uin3, uin_grad=ugr3)))
    case("factorize degree-dependent, LU form", lambda: factored(ba, dict(kw3, alpha_n=a_n, beta_n=b_n), dict(uin=uin3, uin_grad=ugr3),
                                                                 BIEM_LDLT_PIVOT_REL="1e30"))
    case("factorize single ball", lambda: factored(ba, kw1, dict(uin=uin3)))
    case("factorize NumPy", lambda: factored(ba, kwn, dict(uin=uin_np)))

    # fields
    calc = amd.biem(ba, uin=uin3, **kw3)
    calc_n = amd.biem(ba, uin=uin3, uin_grad=ugr3, alpha_n=a_n, beta_n=b_n, **kw3)
    calc_p = amd.biem(bpa, uin=uin3, **kwp)
    calc_r = amd.biem(ba, uin=uin_r, uin_grad=ugr_r, alpha=1.0, beta=0.3, **kwr)
    calc_np = amd.biem(ba, uin=uin_np, **kwn)
    calc_in = amd.biem(ba, uin=uin3, kind="inner", **kw1)
    x = dev(np.concatenate([4.0 * rng.standard_normal((3, 13)), cen3.T + 0.3, 40.0 * rng.standard_normal((3, 5))], axis=1))   # outside, inside, far
    xb = x[:, :, None].expand(3, x.shape[1], 3)
    case("uscat near and far points", lambda: {"u": calc.uscat(x)})
    case("uscat far_field", lambda: {"u": calc.uscat(x, far_field=True)})
    case("uscat per_ball", lambda: {"u": calc.uscat(x, per_ball=True)})
    case("uscat expand_x=False", lambda: {"u": calc.uscat(xb, expand_x=False)})
    case("uscat kind=inner", lambda: {"u": calc_in.uscat(0.3 * x)})
    case("uscat NumPy", lambda: {"u": calc_np.uscat(x.cpu().numpy())})
    case("uscat bpa", lambda: {"u": calc_p.uscat(x)})
    case("uscat_grad", lambda: {"g": calc.uscat_grad(x), "gb": calc.uscat_grad(x, per_ball=True)})
    case("uscat_grad bpa", lambda: {"g": calc_p.uscat_grad(x)})
    case("uinterior", lambda: {"u": calc_n.uinterior(x, **fluid)})
    case("uinterior_grad", lambda: {"g": calc_n.uinterior_grad(x, **fluid)})
    case("utotal", lambda: {"u": calc_n.utotal(x, **fluid)})
    case("utotal_grad", lambda: {"g": calc_n.utotal_grad(x, uin_grad=ugr3, **fluid)})
    case("far_pattern", lambda: {"f": calc.far_pattern(x), "fb": calc.far_pattern(x, per_ball=True), "fr": calc_r.far_pattern(x[:, :4])})

    def power(p):
        return {"extinction": p.extinction, "absorption": p.absorption, "scattering": p.scattering}

    case("power", lambda: power(calc.power(uin_grad=ugr3)))
    case("power rhs axis", lambda: power(calc_r.power(uin_grad=ugr_r, alpha=1.0, beta=0.3)))
    case("power degree-dependent", lambda: power(calc_n.power(uin_grad=ugr3, alpha_n=a_n, beta_n=b_n)))
    case("power NumPy", lambda: power(calc_np.power(uin_grad=ugr_np)))
    case("force", lambda: {"f": calc.force()})
    case("force rhs axis", lambda: {"f": calc_r.force(alpha=1.0, beta=0.3)})
    case("force degree-dependent", lambda: {"f": calc_n.force(alpha_n=a_n, beta_n=b_n)})
    case("force bpa", lambda: {"f": calc_p.force()})


def diff(old, new):
    a, b = ([json.loads(line) for line in open(p) if line.startswith("{")] for p in (old, new))
    names = [r["case"] for r in a]
    bad = int(names != [r["case"] for r in b])
    if bad:
        print("DIFFERENT: the two outputs do not hold the same cases")
    for ra, rb in zip(a, b):
        same = ra == rb
        bad += not same
        what = "" if same else " " + ", ".join(k for k in ("out", "stats", "profile") if ra[k] != rb[k])
        print(f"{'identical' if same else 'DIFFERENT' + what}: {ra['case']}: {len(ra['out'])} results, stats {ra['stats']}, launches/work per class {ra['profile']}")
    print(f"{len(a)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
