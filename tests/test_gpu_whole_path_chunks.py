"""GPU tests of the whole-path driver through the raw C entries: one batch of 3 systems with 2 right-hand sides, cut into chunks of 1, 2
and 3 systems (a last partial chunk; the offsets of wavenumbers, centres - shared and per system -, tables, samples, densities and codes
of the chunks behind the first), solved by

    biem_solve_ldlt,  biem_solve_ldlt_n (the plain coefficients repeated over the degrees),  biem_solve (pivoted LU),
    biem_factor_ldlt + biem_solve_factored,  biem_factor_ldlt_n + biem_solve_factored_n.

Every entry at every chunk size gives the density of biem() under BIEM_SOLVER=lu to 1e-10 of its largest entry (the tolerance between
forms of tests/test_gpu_sym_split.py; no bit equality across chunk sizes: the bulk update may depend on the systems per launch) and the
same codes.  Then the last system is made unscalable (alpha_n = beta_n = 0 in one degree of one ball, so gj_n = 0 exactly): its code is
-(n_pad + 2) from biem_solve_ldlt_n and from biem_factor_ldlt_n at every chunk size, and the systems in front of it are solved as before.

Shapes: `ba`, 2 balls, n_end 4 (N = 32: one LDS-resident launch per chunk); `ba`, 4 coplanar balls, n_end 13 (N = 676) - with
BIEM_SYM_SPLIT=1, in a child process started with it, the split form (E 384, O 320 rows), else the unsplit general path.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import torch
except ImportError:
    torch = None

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
NB, NRHS, CHUNKS = 3, 2, (1, 2, 3)
ALPHA, BETA = 1.0, 0.3
SQUARE = np.array([[0.0, 0.0, 0.3], [2.5, 0.0, 0.3], [0.0, 2.5, 0.3], [2.5, 2.5, 0.3]])      # (tests/test_gpu_sym_split.py)
PAIR = np.array([[0.0, 1.3, -0.2], [0.4, -1.2, -0.2]])
SHAPES = {"small": (PAIR, [1.0, 0.8], 4), "four balls": (SQUARE, np.ones(4), 13)}


@pytest.fixture(scope="module")
def amd():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    import biem_helmholtz_sphere_amd as amd

    return amd


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), device="cuda").to(dtype or torch.float64).contiguous()


class _Case:
    """The operands of one batch as the C entries take them (the package's own flattening and boundary samples) and its reference density."""

    def __init__(self, amd, cen, rad, n_end, geom_per_system, spoil_last=False):
        from biem_helmholtz_sphere_amd import _lib, _operator as op

        self.lib, self.L = _lib.load(), _lib
        cen, rad = np.asarray(cen, float), np.asarray(rad, float)
        B, d = cen.shape
        ks = np.linspace(0.8, 2.4, NB)[None, :]
        ang = 0.4 + 0.9 * np.arange(NRHS)
        dirs = np.zeros((d, NRHS, 1))
        dirs[0, :, 0], dirs[1, :, 0], dirs[2, :, 0] = np.cos(ang) * 0.8, np.sin(ang) * 0.8, 0.6
        dirs /= np.linalg.norm(dirs, axis=0, keepdims=True)
        c = amd.create_from_branching_types("ba")
        if geom_per_system:
            cen_t, rad_t = _dev(np.broadcast_to(cen, (1, NB) + cen.shape)), _dev(np.broadcast_to(rad, (1, NB) + rad.shape))
        else:
            cen_t, rad_t = _dev(cen)[None, None], _dev(rad)[None, None]
        uin, ugr = amd.plane_wave(k=_dev(ks), direction=_dev(dirs))
        geom = dict(centers=cen_t, radii=rad_t, k=_dev(ks), n_end=n_end)
        # the plain coefficients, and the same repeated over the degrees: shared by the systems, or one set per system (spoil_last: with
        # both coefficients of degree 2 of the last ball of the last system zero)
        an, bn = np.full((1, NB if spoil_last else 1, B, n_end), ALPHA, complex), np.full((1, NB if spoil_last else 1, B, n_end), BETA, complex)
        if spoil_last:
            an[0, -1, -1, 2] = bn[0, -1, -1, 2] = 0.0
        self.plain = op._operator(c, cen_t, rad_t, _dev(ks), n_end, ALPHA, BETA, None, "outer")
        self.per_degree = op._operator(c, cen_t, rad_t, _dev(ks), n_end, 1.0, 0.0, None, "outer", _dev(an, torch.complex128), _dev(bn, torch.complex128))
        self.g = {id(o): op._boundary_samples(o, uin, ugr)[0] for o in (self.plain, self.per_degree)}
        self.sample_ptrs = op._sample_ptrs
        self.B, self.H, self.n_end = B, self.plain.plan.H, n_end
        self.n_pad = int(self.lib.biem_lu_npad(B * self.H))
        old = os.environ.get("BIEM_SOLVER")
        os.environ["BIEM_SOLVER"] = "lu"
        try:
            ref = amd.biem(c, uin=uin, uin_grad=ugr, alpha=ALPHA, beta=BETA, **geom).density.cpu().numpy()          # [nrhs, nb, B, H]
        finally:
            os.environ.pop("BIEM_SOLVER") if old is None else os.environ.__setitem__("BIEM_SOLVER", old)
        self.ref = np.moveaxis(ref, 0, 1)
        assert self.ref.shape == (NB, NRHS, B, self.H) and np.all(np.isfinite(self.ref))

    def _operands(self, o):
        fl, p = o.fl, lambda t: t.data_ptr()
        return (o.plan.handle, NB, self.B), (p(fl.k), p(fl.eta), p(fl.centers), p(fl.radii), fl.geom_batched, p(fl.alpha), p(fl.beta), fl.ab_batched)

    def solve(self, name, chunk):
        """density [nb, nrhs, B, H] and codes [nb] of one fused entry"""
        o = self.per_degree if name.endswith("_n") else self.plain
        head, operands = self._operands(o)
        wb = int(self.lib.biem_solve_workspace_bytes(o.plan.handle, NB, self.B, NRHS, chunk))
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        dens = torch.zeros((NB, NRHS, self.B, self.H), dtype=torch.complex128, device="cuda")
        info = torch.full((NB,), 77, dtype=torch.int32, device="cuda")
        self.L.check(getattr(self.lib, name)(*head, NRHS, *operands, *self.sample_ptrs(self.g[id(o)]), dens.data_ptr(), info.data_ptr(), chunk,
                                             work.data_ptr(), wb, None), name)
        torch.cuda.synchronize()
        return dens.cpu().numpy(), info.cpu().numpy()

    def factor(self, suffix, chunk):
        """factors, tables and codes of biem_factor_ldlt / biem_factor_ldlt_n"""
        o = self.per_degree if suffix else self.plain
        head, operands = self._operands(o)
        n_pad = self.n_pad
        wb = int(self.lib.biem_factor_workspace_bytes(o.plan.handle, NB, self.B, chunk))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
        F = torch.zeros((NB, n_pad, n_pad), dtype=torch.complex128, device="cuda")
        tab = torch.zeros((NB, self.B, 3, self.n_end), dtype=torch.complex128, device="cuda")
        info = torch.full((NB,), 77, dtype=torch.int32, device="cuda")
        self.L.check(getattr(self.lib, "biem_factor_ldlt" + suffix)(*head, *operands, F.data_ptr(), n_pad, n_pad * n_pad, tab.data_ptr(), info.data_ptr(),
                                                                    chunk, work.data_ptr(), wb, None), "biem_factor_ldlt" + suffix)
        torch.cuda.synchronize()
        return F, tab, info.cpu().numpy()

    def factor_and_solve(self, suffix, chunk):
        o = self.per_degree if suffix else self.plain
        F, tab, info = self.factor(suffix, chunk)
        fl, n_pad = o.fl, self.n_pad
        wb = int(self.lib.biem_solve_factored_workspace_bytes(o.plan.handle, NB, self.B, NRHS))
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        dens = torch.zeros((NB, NRHS, self.B, self.H), dtype=torch.complex128, device="cuda")
        coef = (fl.alpha.data_ptr(), fl.beta.data_ptr(), fl.ab_batched) if suffix else ()
        self.L.check(getattr(self.lib, "biem_solve_factored" + suffix)(o.plan.handle, NB, self.B, NRHS, F.data_ptr(), n_pad, n_pad * n_pad, tab.data_ptr(), *coef,
                                                                       *self.sample_ptrs(self.g[id(o)]), dens.data_ptr(), work.data_ptr(), wb, None),
                     "biem_solve_factored" + suffix)
        torch.cuda.synchronize()
        return dens.cpu().numpy(), info

    def last_split(self):
        a, b = C.c_int(-1), C.c_int(-1)
        self.L.check(self.lib.biem_last_solve_split(C.byref(a), C.byref(b)))
        return a.value, b.value


def _all_entries_all_chunkings(amd, shape, geom_per_system, expect_split):
    cen, rad, n_end = SHAPES[shape]
    case = _Case(amd, cen, rad, n_end, geom_per_system)
    scale = np.abs(case.ref).max()
    seen = []
    for chunk in CHUNKS:
        runs = {name: case.solve(name, chunk) for name in ("biem_solve_ldlt", "biem_solve_ldlt_n")}
        assert case.last_split() == expect_split, (chunk, case.last_split())
        runs["biem_solve"] = case.solve("biem_solve", chunk)
        runs["biem_factor_ldlt + biem_solve_factored"] = case.factor_and_solve("", chunk)
        runs["biem_factor_ldlt_n + biem_solve_factored_n"] = case.factor_and_solve("_n", chunk)
        for name, (dens, info) in runs.items():
            err = np.abs(dens - case.ref).max() / scale
            print(f"{shape}, chunk {chunk}, {name}: {err:.2e} of the largest density from the reference, codes {info.tolist()}")
            assert np.array_equal(info, np.zeros(NB, np.int32)), (name, chunk, info)
            assert err <= TOL, (name, chunk, err)
            seen.append(dens)
    spread = max(np.abs(a - b).max() for i, a in enumerate(seen) for b in seen[:i]) / scale
    print(f"{shape}: largest distance between two of the {len(seen)} runs {spread:.2e}")
    assert spread <= TOL, spread


def _unscalable_last_system(amd, shape, geom_per_system, expect_split):
    cen, rad, n_end = SHAPES[shape]
    case = _Case(amd, cen, rad, n_end, geom_per_system, spoil_last=True)
    scale = np.abs(case.ref).max()
    for chunk in CHUNKS:
        dens, info = case.solve("biem_solve_ldlt_n", chunk)
        split = case.last_split()
        assert split == expect_split, (chunk, split)
        n_pad = sum(split) if split != (0, 0) else case.n_pad
        _, _, info_f = case.factor("_n", chunk)
        print(f"{shape}, chunk {chunk}: codes {info.tolist()} (fused), {info_f.tolist()} (factor)")
        assert info.tolist() == [0] * (NB - 1) + [-(n_pad + 2)], (chunk, info)
        assert info_f.tolist() == [0] * (NB - 1) + [-(case.n_pad + 2)], (chunk, info_f)
        err = np.abs(dens[:-1] - case.ref[:-1]).max() / scale
        assert err <= TOL, (chunk, err)


def _run(amd, shape, geom_per_system, expect_split):
    _all_entries_all_chunkings(amd, shape, geom_per_system, expect_split)
    _unscalable_last_system(amd, shape, geom_per_system, expect_split)


@gpu
@pytest.mark.parametrize("shape,geom_per_system", [("small", False), ("small", True), ("four balls", True)])
def test_chunks_and_entries_agree(amd, monkeypatch, shape, geom_per_system):
    """The one-launch small path with shared and with per-system centres, and the unsplit general path with per-system centres."""
    monkeypatch.delenv("BIEM_SYM_SPLIT", raising=False)
    monkeypatch.delenv("BIEM_SOLVER", raising=False)
    _run(amd, shape, geom_per_system, (0, 0))


@gpu
def test_chunks_and_entries_agree_in_the_split_form(amd):
    """The four coplanar balls with shared centres under BIEM_SYM_SPLIT=1, set before the child process starts; the child asserts through
    biem_last_solve_split that every fused symmetric call ran in the split form (E 384, O 320)."""
    env = {k: v for k, v in os.environ.items() if k != "BIEM_SOLVER"}
    env["BIEM_SYM_SPLIT"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "split form ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import biem_helmholtz_sphere_amd

    assert os.environ.get("BIEM_SYM_SPLIT") == "1"
    _run(biem_helmholtz_sphere_amd, "four balls", False, (384, 320))
    print("split form ok")
