#!/usr/bin/env python3
"""Write tests/golden/hess_fields.npz: the Cartesian Hessian of the scattered field of small solved problems, by second differences
of the 40-digit field series of oracle/mp_field.py.  CPU only (mpmath); no GPU test imports mpmath.

    python tools/make_hess_fixtures.py            # write the fixture (about a minute on 8 cores)
    python tools/make_hess_fixtures.py --check    # recompute and compare with the committed file, array by array

Cases: the trees a, ba, bpa, bba, bpbpa, caa at n_end 8 / 6 / 6 / 5 / 5 / 5 with the two-ball geometry, the plane-wave direction and the
point set of tests/test_gpu_field_gradient.py (a far point, the origin, both poles of the root axis, the coordinate axes and planes of
the tree, a point at 1.05 rho) and one point inside a ball for the mask; k = 1.3 on every tree and one complex k on a and on bpbpa.
Kind inner: one ball per tree family (a, ba, bba, caa) with its centre among the points and one point outside for the mask.  The
densities come from oracle.biem_oracle.solve_biem and are stored, so a test needs no solve.

The Hessian is the second central difference (diagonal) and the four-point cross difference (off the diagonal) of
MPField.ball_sum summed over the balls, with step 1e-10 at 40 digits: truncation (step^2 / 12) f'''' and rounding 1e-40 / step^2 are
both near 1e-20.  Before anything is stored the steps 1e-10 and 2e-10 must agree within 1e-14 of max |H| of the case.
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import biem_oracle as O  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "hess_fields.npz")
N_END = {"a": 8, "ba": 6, "bpa": 6, "bba": 5, "bpbpa": 5, "caa": 5}
DIM = {"a": 2, "ba": 3, "bpa": 3, "bba": 4, "bpbpa": 4, "caa": 4}
ROOT_AXIS = {"a": 0, "ba": 0, "bba": 0, "caa": 0, "bpa": 2, "bpbpa": 3}      # canonical axis 0 in the caller's axes
STEPS = ("1e-10", "2e-10")
STEP_AGREE = 1e-14


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def two_balls(d):
    return np.array([[1.7, 0.9, -0.6, 0.5], [-1.4, -1.1, 0.8, -0.7]])[:, :d].copy(), np.array([1.0, 0.7])


def one_ball(d):
    return np.array([[0.4, -0.3, 0.2, 0.1]])[:, :d].copy(), np.array([1.3])


def direction(d):
    return _unit(np.array([0.9, -0.5, 0.7, 0.3])[:d])


def outer_points(bt, cen, rad):
    """The points of tests/test_gpu_field_gradient.py::_points, then one inside ball 0 (masked)."""
    d = DIM[bt]
    e = np.eye(d)
    pts = [3.5 * _unit(np.array([0.3, -0.8, 0.45, 0.6])[:d]), np.zeros(d)]
    pts.append(cen[1] + 1.2 * rad[1] * e[ROOT_AXIS[bt]])
    pts.append(cen[0] - 1.3 * rad[0] * e[ROOT_AXIS[bt]])
    pts.append(cen[1] + 1.2 * rad[1] * e[0])
    if d == 4:
        pts.append(cen[0] + 1.25 * rad[0] * _unit([0.6, -0.8, 0.0, 0.0]))
        pts.append(cen[1] + 1.25 * rad[1] * _unit([0.0, 0.0, 0.7, 0.5]))
        pts.append(cen[0] + 1.25 * rad[0] * _unit([0.0, 0.6, -0.8, 0.0]))
        pts.append(cen[1] + 1.25 * rad[1] * _unit([0.7, 0.0, 0.0, -0.5]))
    pts.append(cen[0] + 1.05 * rad[0] * _unit(np.array([-0.5, 0.4, 0.6, -0.3])[:d]))
    pts.append(cen[0] + 0.5 * rad[0] * _unit(np.ones(d)))
    return np.array(pts)


def inner_points(bt, cen, rad):
    """Inside the one ball: a generic point, the centre, both poles of the root axis, x0, the tree's planes, a point at 0.95 rho; then
    one outside (masked)."""
    d = DIM[bt]
    e = np.eye(d)
    c, rho = cen[0], rad[0]
    pts = [c + 0.5 * rho * _unit(np.array([0.3, -0.8, 0.45, 0.6])[:d]), c.copy()]
    pts.append(c + 0.6 * rho * e[ROOT_AXIS[bt]])
    pts.append(c - 0.7 * rho * e[ROOT_AXIS[bt]])
    pts.append(c + 0.4 * rho * e[d - 1])
    if d == 4:
        pts.append(c + 0.45 * rho * _unit([0.6, -0.8, 0.0, 0.0]))
        pts.append(c + 0.45 * rho * _unit([0.0, 0.0, 0.7, 0.5]))
        pts.append(c + 0.45 * rho * _unit([0.0, 0.6, -0.8, 0.0]))
        pts.append(c + 0.45 * rho * _unit([0.7, 0.0, 0.0, -0.5]))
    pts.append(c + 0.95 * rho * _unit(np.array([-0.5, 0.4, 0.6, -0.3])[:d]))
    pts.append(c + 1.1 * rho * _unit(np.ones(d)))
    return np.array(pts)


def case_list():
    cases = [dict(tree=bt, kind="outer", k=1.3) for bt in ("a", "ba", "bpa", "bba", "bpbpa", "caa")]
    cases += [dict(tree="a", kind="outer", k=1.3 + 0.2j), dict(tree="bpbpa", kind="outer", k=1.2 + 0.15j)]
    cases += [dict(tree=bt, kind="inner", k=1.3) for bt in ("a", "ba", "bba", "caa")]
    for c in cases:
        kc = complex(c["k"])
        c["id"] = f"{c['kind']}-{c['tree']}-k{kc.real:g}" + (f"+{kc.imag:g}i" if kc.imag else "")
    return cases


def mp_hessian(F, x, step):
    """[d, d] mpc at one point: the rule of oracle.mp_field (MPField.hessian applies it with both steps and the same acceptance)."""
    from oracle import mp_field as M

    return M.hessian_by_differences(F, x, step)


def build_case(case):
    import mpmath as mp
    from oracle import mp_field as M

    t0 = time.time()
    bt, kind, k = case["tree"], case["kind"], case["k"]
    d, n_end = DIM[bt], N_END[bt]
    cen, rad = two_balls(d) if kind == "outer" else one_ball(d)
    uo, go = O.plane_wave(k, direction(d))
    res = O.solve_biem(bt, centers=cen, radii=rad, k=k, n_end=n_end, eta=1.0, alpha=1.0, beta=0.0, uin=uo, uin_grad=go, kind=kind)
    x = outer_points(bt, cen, rad) if kind == "outer" else inner_points(bt, cen, rad)
    F = M.MPField(bt, n_end, k, 1.0, cen, rad, res.density, kind)
    P = len(x)
    hess = np.full((d, d, P), complex(np.nan, 0.0))
    valid = np.zeros(P, dtype=bool)
    worst = 0.0
    with mp.workdps(M.DPS):
        both = []
        for p in range(P):
            xm = F._x(x[p])
            valid[p] = bool(F.valid("near", xm))
            both.append([mp_hessian(F, xm, s) for s in STEPS] if valid[p] else None)
        scale = max(abs(v) for hs in both if hs for row in hs[0] for v in row)
        for p, hs in enumerate(both):
            if hs is None:
                continue
            for i in range(d):
                for j in range(d):
                    worst = max(worst, float(abs(hs[0][i][j] - hs[1][i][j]) / scale))
                    hess[i, j, p] = complex(hs[0][i][j])
    assert worst <= STEP_AGREE, (case["id"], worst)
    assert valid[:-1].all() and not valid[-1]
    u = O.uscat(res, x)
    assert np.array_equal(np.isnan(u), ~valid)
    trace = np.abs(sum(hess[i, i] for i in range(d)) + complex(k) ** 2 * u)[valid].max() / float(scale)
    print(f"{case['id']:22s} P={P:2d} max|H| {float(scale):.3e}  steps agree within {worst:.1e}  |tr H + k^2 u(fp64 oracle)| {trace:.1e} of max|H|  "
          f"{time.time() - t0:5.1f}s", flush=True)
    kc = complex(k)
    meta = dict(tree=bt, kind=kind, n_end=n_end, k=[kc.real, kc.imag], eta=1.0)
    arrays = dict(centers=cen, radii=rad, density=np.asarray(res.density, dtype=np.complex128), x=x, valid=valid, hess=hess)
    return case["id"], meta, arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=PATH)
    ap.add_argument("--check", action="store_true", help="recompute and compare with the file instead of writing it")
    ap.add_argument("--jobs", type=int, default=min(8, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    cases = case_list()
    with multiprocessing.get_context("fork").Pool(args.jobs) as pool:
        done = pool.map(build_case, sorted(cases, key=lambda c: -DIM[c["tree"]]), chunksize=1)
    by_id = {cid: (meta, arrays) for cid, meta, arrays in done}
    order = [c["id"] for c in cases]
    store = {"cases": np.array(json.dumps(order))}
    for cid in order:
        meta, arrays = by_id[cid]
        store[cid + "/meta"] = np.array(json.dumps(meta))
        store.update({f"{cid}/{name}": a for name, a in arrays.items()})
    if args.check:
        bad = 0
        with np.load(args.out, allow_pickle=False) as z:
            for name, a in store.items():
                if name not in z.files or not np.array_equal(z[name], a, equal_nan=a.dtype.kind in "fc"):
                    print("differs:", name)
                    bad += 1
            for name in sorted(set(z.files) - set(store)):
                print("only in the file:", name)
                bad += 1
        print(f"{len(store)} arrays compared, {bad} differ")
        return 1 if bad else 0
    np.savez_compressed(args.out, **store)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(order)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
