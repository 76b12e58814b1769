"""The per-lane field kernels AT their order ceilings (n_end 320 / 48 / 14 / 12 on the trees a / ba / bba / caa; the 2-D orders 153 / 152
at which the per-lane j_n rows of kind inner and of the interior field fill the LDS) against 40-digit values.

The suite otherwise checks ``uscat_grad``, ``uinterior`` and ``uinterior_grad`` at n_end <= 8 and ``uscat`` at high order only against the
other GPU kernel, while the kernels' LDS layout, coefficient staging, recurrence tables and per-lane rows are all indexed by n_end.
Here every case comes from ``tests/golden/full_order_fields.npz`` (``tools/make_full_order_fixtures.py``): synthetic densities that give
EVERY degree a term of modulus in [0.5, 1.5] at a reference radius - a solved density decays with the degree and hides the top
ones below any tolerance - and the value and gradient of the series evaluated by ``oracle/mp_field.py`` in 40-digit arithmetic,
rounded to fp64.  Nothing high-precision runs here: a case is one or two kernel calls on stored inputs.

Assertions, per point (not per case: the fields span many decades between r = 1.02 rho and r = 1.5 rho):
* the NaN mask is exactly the stored one;
* |got - want| <= 1e-10 |want| for values, the same with the Euclidean norm over the components for gradients.
1e-10 is the parity contract.  The pointwise scale is sound because the generator admits a point only if its condition
number sum |terms| / |sum| is at most 100 in every VALUE checked (value, per-ball value, far field) and the fp64 oracle itself meets
1e-11 there (both stored per point; gradients carry no cap of their own: they are sums of the same terms weighted by factors of
order n / r, and no fp64 yardstick reaches 1e-11 for them at these orders; ``tests/test_full_order_yardstick_host.py`` checks the caps and ties the 40-digit evaluator to the oracle at low order).
Every test prints the largest error it measured.
"""
import numpy as np
import pytest
import torch

import biem_helmholtz_sphere_amd as amd
from oracle import full_order_fixture as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY_TOL = 1e-10
CASES = FX.load()
EXT = [c for c in CASES if c.startswith("ext-")]
INNER = [c for c in CASES if c.startswith("inner-")]
INTERIOR = [c for c in CASES if c.startswith("interior-")]
KERNELS = ["per_lane", "generic"]


def t(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device=DEV, dtype=dtype)


def _calculator(rec, density):
    """A result record built directly around a stored density (no solve)."""
    return amd.BIEMResultCalculator(c=amd.create_from_branching_types(rec.tree), centers=t(rec.centers.T), radii=t(rec.radii), k=t(rec.k),
                                    n_end=rec.n_end, eta=t(float(rec.eta)), kind="outer" if rec.kind == "interior" else rec.kind,
                                    density=t(density, torch.complex128))


def _fluid(rec):
    return dict(k_interior=t(rec.k_interior, torch.complex128), density_ratio=t(rec.density_ratio, torch.float64))


def _check_value(what, got, want, valid, masked=True):
    """got, want [P] or [P, B]; valid [P].  Returns the largest pointwise relative error."""
    assert got.shape == want.shape, (got.shape, want.shape)
    v = valid if masked else np.ones_like(valid)
    bad = np.isnan(got.real) | np.isnan(got.imag)
    assert np.array_equal(bad, np.broadcast_to(~v.reshape(v.shape + (1,) * (got.ndim - 1)), got.shape)), f"{what}: NaN mask {bad}"
    err = np.abs(got[v] - want[v]) / np.abs(want[v])
    print(f"  {what}: max |got - want| / |want| = {err.max():.2e} over {int(v.sum())} points (|want| {np.abs(want[v]).min():.1e} .. {np.abs(want[v]).max():.1e})")
    assert (err <= PARITY_TOL).all(), f"{what}: {err}"
    return err.max()


def _check_grad(what, got, want, valid):
    """got, want [d, P]."""
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.isnan(got.real) | np.isnan(got.imag)
    assert np.array_equal(bad, np.broadcast_to(~valid, got.shape)), f"{what}: NaN mask {bad}"
    err = np.linalg.norm(got[:, valid] - want[:, valid], axis=0) / np.linalg.norm(want[:, valid], axis=0)
    print(f"  {what}: max |got - want| / |want| = {err.max():.2e} over {int(valid.sum())} points (Euclidean norm over the components)")
    assert (err <= PARITY_TOL).all(), f"{what}: {err}"
    return err.max()


def _select(monkeypatch, kernel):
    if kernel == "generic":
        monkeypatch.setenv("BIEM_USCAT_GENERIC", "1")
    else:
        monkeypatch.delenv("BIEM_USCAT_GENERIC", raising=False)


def test_the_fixture_holds_the_ceilings_of_this_build():
    """The cases sit at the orders the library reports as its ceilings and at the LDS limits of the launchers' formulas."""
    assert amd._biem.USCAT_GRAD_N_END_MAX == {"a": 320, "ba": 48, "bba": 14, "caa": 12}
    top = {}
    for rec in CASES.values():
        fam = {"bpa": "ba", "bpbpa": "bba"}.get(rec.tree, rec.tree)
        top[fam] = max(top.get(fam, 0), rec.n_end)
        assert len(rec.x) % 64 != 0
    assert top == amd._biem.USCAT_GRAD_N_END_MAX
    v_max, g_max = FX.lds_row_ceiling(False), FX.lds_row_ceiling(True)
    for kind in ("inner", "interior"):
        assert any(r.kind == kind and r.tree == "a" and r.n_end == g_max and r.grad is not None for r in CASES.values())
        assert any(r.kind == kind and r.tree == "a" and r.n_end == v_max for r in CASES.values())      # (interior: one above its ceiling)
    assert any(r.kind == "inner" and r.tree == "a" and r.n_end == v_max + 1 for r in CASES.values())


# ---------------------------------------------------------------------------- exterior: two balls
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cid", EXT)
def test_exterior_value_per_ball_and_far_field(cid, kernel, monkeypatch):
    """uscat, uscat(per_ball=True), uscat(far_field=True) through the per-lane kernel and through the harmonic-by-harmonic one
    (BIEM_USCAT_GENERIC=1): both are pinned to the same independent numbers."""
    rec = CASES[cid]
    _select(monkeypatch, kernel)
    x = t(rec.x.T)
    calc = _calculator(rec, rec.density)
    print(f"{cid} [{kernel}]: condition <= {np.nanmax(rec.cond):.0f} / {np.nanmax(rec.cond_ball):.0f} / {np.nanmax(rec.cond_far):.0f}, fp64 oracle "
          f"{np.nanmax(rec.oracle_err):.1e} / {np.nanmax(rec.oracle_err_ball):.1e} / {np.nanmax(rec.oracle_err_far):.1e} (value / per ball / far field)")
    _check_value("value", calc.uscat(x).cpu().numpy(), rec.value, rec.valid)
    _check_value("per ball", calc.uscat(x, per_ball=True).cpu().numpy(), rec.per_ball, rec.valid)
    far = _calculator(rec, rec.density_far).uscat(x, far_field=True).cpu().numpy()
    _check_value("far field", far, rec.far, rec.valid, masked=False)


@pytest.mark.parametrize("cid", EXT)
def test_exterior_gradient(cid):
    rec = CASES[cid]
    got = _calculator(rec, rec.density).uscat_grad(t(rec.x.T)).cpu().numpy()
    print(cid)
    _check_grad("gradient", got, rec.grad, rec.valid)


# ---------------------------------------------------------------------------- kind = "inner": one ball
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cid", INNER)
def test_inner_value(cid, kernel, monkeypatch):
    """Orders whose per-lane rows do not fit the LDS (2-D above 153) take the harmonic-by-harmonic kernel in both settings."""
    rec = CASES[cid]
    _select(monkeypatch, kernel)
    print(f"{cid} [{kernel}]: condition <= {np.nanmax(rec.cond):.0f}, fp64 oracle {np.nanmax(rec.oracle_err):.1e}")
    _check_value("value", _calculator(rec, rec.density).uscat(t(rec.x.T)).cpu().numpy(), rec.value, rec.valid)


@pytest.mark.parametrize("cid", [c for c in INNER if CASES[c].grad is not None])
def test_inner_gradient(cid):
    rec = CASES[cid]
    print(cid)
    _check_grad("gradient", _calculator(rec, rec.density).uscat_grad(t(rec.x.T)).cpu().numpy(), rec.grad, rec.valid)


def test_orders_above_the_lds_rows_of_kind_inner():
    """2-D, kind inner, one order above what the per-lane rows hold: the value is still right (through the other kernel), the gradient,
    which has no other kernel, raises NotImplementedError naming the LDS."""
    v_max, g_max = FX.lds_row_ceiling(False), FX.lds_row_ceiling(True)
    above = [r for r in CASES.values() if r.kind == "inner" and r.tree == "a" and r.n_end == v_max + 1]
    assert above
    for rec in above:
        print(rec.id)
        _check_value("value", _calculator(rec, rec.density).uscat(t(rec.x.T)).cpu().numpy(), rec.value, rec.valid)
    over = [r for r in CASES.values() if r.kind == "inner" and r.tree == "a" and r.n_end == g_max + 1]
    assert over
    for rec in over:
        with pytest.raises(NotImplementedError, match="LDS"):
            _calculator(rec, rec.density).uscat_grad(t(rec.x.T))


# ---------------------------------------------------------------------------- the interior field: two balls, two fluids
@pytest.mark.parametrize("cid", INTERIOR)
def test_interior_value(cid):
    rec = CASES[cid]
    print(f"{cid}: condition <= {np.nanmax(rec.cond):.0f}, fp64 formula {np.nanmax(rec.oracle_err):.1e}")
    if rec.tree == "a" and rec.n_end > FX.lds_row_ceiling(True):
        # One order above the gradient's: the value rows alone fit the LDS (163600 of 163840 bytes), but a kernel's code object may hold LDS
        # of its own beside them.  Whether it then fits is the launcher's to say, from the code object it launches: it computes the
        # stored values or refuses naming the LDS, and never fails otherwise (this case found it failing inside the launch).
        try:
            got = _calculator(rec, rec.density).uinterior(t(rec.x.T), **_fluid(rec)).cpu().numpy()
        except NotImplementedError as e:
            print(f"  refused: {e}")
            assert "LDS" in str(e) and f"n_end={rec.n_end}" in str(e)
            return
        _check_value("value", got, rec.value, rec.valid)
        return
    got = _calculator(rec, rec.density).uinterior(t(rec.x.T), **_fluid(rec)).cpu().numpy()
    _check_value("value", got, rec.value, rec.valid)


@pytest.mark.parametrize("cid", [c for c in INTERIOR if CASES[c].grad is not None])
def test_interior_gradient(cid):
    rec = CASES[cid]
    print(cid)
    got = _calculator(rec, rec.density).uinterior_grad(t(rec.x.T), **_fluid(rec)).cpu().numpy()
    _check_grad("gradient", got, rec.grad, rec.valid)


def test_orders_above_the_lds_rows_of_the_interior_field():
    """2-D: at the first order whose gradient rows do not fit the LDS, uinterior_grad raises naming the LDS (152 itself is computed above)."""
    rec = next(r for r in CASES.values() if r.kind == "interior" and r.tree == "a" and r.n_end == FX.lds_row_ceiling(True) + 1)
    with pytest.raises(NotImplementedError, match="LDS"):
        _calculator(rec, rec.density).uinterior_grad(t(rec.x.T), **_fluid(rec))
