"""Observables of a solved problem (extensions): cross sections and the radiation force on each ball.  Algebra
on what the solve left behind, in one small kernel each; every function only reads the record's attributes."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Any, Callable

import torch

from . import _lib as L
from ._arrays import Array, _inverse_perm, _ptr, _stream_ptr, _to_dev
from ._fields import _check_built
from ._operator import _RhsAxes, _ball_tables, _boundary_samples, _entry, _result_operator, _rhs_project


@dataclass(frozen=True)
class BIEMPower:
    """What :func:`biem_power` returns: real float64 arrays in the caller's array type, batch axes (right-hand-side axes included)
    in the caller's order."""

    extinction: Array    # (...(first), B): power each ball removes from the incident field
    absorption: Array    # (...(first), B): power each ball absorbs
    scattering: Array    # (...(first)):    sum of the extinction minus sum of the absorption


def biem_power(res: Any, /, *, uin_grad: Callable[[Array], Array], uin: Callable[[Array], Array] | None = None,
               alpha: Array | complex = 1.0, beta: Array | complex = 0.0, alpha_n: Array | None = None,
               beta_n: Array | None = None) -> BIEMPower:
    r"""Power the cluster removes from the incident field (extinction), absorbs per ball, and re-radiates (scattering).

    For real ``k``, in the far-field normalisation :math:`u_{scat} \sim F(\hat x) e^{ikr} / r^{(d-1)/2}`: "power" is
    :math:`(1/k)\,\mathrm{Im} \oint \bar u\, \partial_n u\, dS`, for a unit plane wave the cross section.  Algebra on what the solve
    left behind - the density, the projections of ``uin`` and ``uin_grad`` on every sphere and the per-ball tables - in one small
    kernel: no second solve, no matrix, every coordinate tree :func:`biem` solves.  The extinction formula holds for any incident field.

    ``uin_grad`` and the coefficients ``alpha`` / ``beta`` (or ``alpha_n`` / ``beta_n``) are the ones :func:`biem` took: the record
    stores neither (the rule of ``utotal_grad``).  ``uin`` defaults to the one the record stores; both callables are always needed,
    also for ``beta = 0``.  A ball whose coefficients have ``Im(alpha_n conj(beta_n)) == 0`` (sound-soft, sound-hard, real impedance,
    a lossless fluid) absorbs exactly ``0.0``; ``Im(alpha_n conj(beta_n)) < 0`` is an active boundary and absorbs a negative power.
    A lossy degree the ball does not scatter (``gj_n`` zero or not finite) makes that ball's absorption NaN, as in ``uinterior``.
    ``scattering`` is a difference: where absorption dominates it carries the absolute error of the extinction, not its own size.

    ``ValueError`` for ``kind="inner"``, any ``Im k != 0``, a result without density and a missing ``uin`` or ``uin_grad``.
    """
    if uin is None and res.uin is not None:
        stored = res.uin
        uin = lambda x: stored(x, expand_x=False)     # (the record's wrapper; _boundary_samples hands over the batch axes itself)
    op = _result_operator(res, "powers", alpha, beta, alpha_n, beta_n, require=(
        (uin, "uin is None and the BIEMResult does not have uin. uin must be provided to compute the extinction."),
        (uin_grad, "uin_grad is None. uin_grad must be provided to compute the extinction.")))
    plan, fl, dev = op.plan, op.fl, op.dev
    nb, B, H = fl.nb, fl.B, plan.H
    # the unweighted samples of the per-degree path, whatever the coefficients: U and V are projections of u_in and d_n u_in alone
    (gu, gdn), axes = _boundary_samples(replace(op, per_degree=True), uin, uin_grad)
    nrhs = axes.nrhs
    dens_t = _to_dev(res.density, dev, torch.complex128)
    if tuple(dens_t.shape) != axes.full + (B, H):
        raise ValueError(f"density has shape {tuple(dens_t.shape)}, but uin / uin_grad and the operator give {axes.full + (B, H)}")
    dens_t = axes.lay_out(dens_t)
    out = torch.empty((nb, nrhs, B, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        if out.numel() > 0:
            plain = replace(op, per_degree=False)     # (biem_rhs_project of one set: no coefficient enters)
            pu, pv = (torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device=dev) for _ in range(2))
            _rhs_project(plain, nb, gu, 0, pu, nrhs * B * H, 1, B * H, sp)
            _rhs_project(plain, nb, gdn, 0, pv, nrhs * B * H, 1, B * H, sp)
            tab = _ball_tables(op, sp)
            lib = L.load()
            entry, what = _entry("biem_power", op.per_degree)
            _check_built(lib, entry(plan.handle, nb, B, nrhs, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.radii), fl.geom_batched, _ptr(fl.alpha),
                                    _ptr(fl.beta), fl.ab_batched, _ptr(tab), _ptr(dens_t), _ptr(pu), _ptr(pv), _ptr(out), sp), what)
    out = axes.restore(out)
    ext, ab = out[..., 0], out[..., 1]
    give = lambda t: op.origin.give(t.contiguous(), complex_out=False)
    return BIEMPower(extinction=give(ext), absorption=give(ab), scattering=give(ext.sum(-1) - ab.sum(-1)))


def biem_force(res: Any, /, *, alpha: Array | complex = 1.0, beta: Array | complex = 0.0, alpha_n: Array | None = None,
               beta_n: Array | None = None) -> Array:
    r"""Time-averaged acoustic radiation force on each ball, real float64 of shape ``(c_ndim, ...(first), B)``: the component axis
    first, in the caller's axis order like ``uscat_grad``, batch axes (right-hand-side axes included) as in ``BIEMPower.extinction``.

    For real ``k`` and ``kind="outer"``, in the normalisation of :func:`biem_power` (for a unit plane wave an area, the
    radiation-pressure cross section as a vector): with ``u`` the total exterior field (time factor :math:`e^{-i\omega t}`),
    :math:`S_b` any closed surface in the fluid around ball ``b`` alone and ``n`` its outward normal,

        Phi_b = -(1 / (2 k^2)) oint_{S_b} [ (k^2 |u|^2 - |grad u|^2) n + 2 Re( grad u conj(d_n u) ) ] dS.

    The physical force on a ball in a fluid of density :math:`\rho_0` at angular frequency :math:`\omega` is
    ``Phi k^2 / (2 rho_0 omega^2)`` for pressure amplitude ``u``.  Algebra on the density alone, in one small kernel: on the ball's own
    surface the boundary condition fixes both traces of ``u``, so neither ``uin`` nor ``uin_grad`` is needed, nor a second solve, a
    matrix or a field evaluation; every coordinate tree :func:`biem` solves.  For a plane wave along ``p^`` the forces obey the
    momentum balance ``sum_b Phi_b = P_ext p^ - int |F(x^)|^2 x^ dOmega`` with :func:`biem_power` and :func:`biem_far_pattern`.

    The coefficients ``alpha`` / ``beta`` (or ``alpha_n`` / ``beta_n``) are the ones :func:`biem` took: the record stores none.  A ball
    with a degree it does not scatter (``gj_n`` zero or not finite, e.g. the transparent sphere ``k_b = k, delta = 1``) and a nonzero
    coefficient there gets NaN in every component, as in ``uinterior``; the other balls are not affected.

    ``ValueError`` for ``kind="inner"``, any ``Im k != 0`` and a result without density.
    """
    op = _result_operator(res, "force", alpha, beta, alpha_n, beta_n)
    plan, fl, dev = op.plan, op.fl, op.dev
    nb, B, H, d = fl.nb, fl.B, plan.H, plan.d
    dens_t = _to_dev(res.density, dev, torch.complex128)
    # batch axes of the density on which the operator has size 1 are right-hand sides (the layout of _boundary_samples)
    full, nbt = tuple(dens_t.shape[:-2]), len(op.batch)
    if len(full) != nbt or tuple(dens_t.shape[-2:]) != (B, H) or any(op.batch[i] not in (1, full[i]) for i in range(nbt)):
        raise ValueError(f"density has shape {tuple(dens_t.shape)}, but the operator gives {tuple(op.batch) + (B, H)}")
    axes = _RhsAxes.of(op.batch, full)
    nrhs = axes.nrhs
    dens_t = axes.lay_out(dens_t)
    out = torch.empty((nb, nrhs, B, d), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        if out.numel() > 0:
            tab = _ball_tables(op, sp)
            lib = L.load()
            entry, what = _entry("biem_force", op.per_degree)
            _check_built(lib, entry(plan.handle, nb, B, nrhs, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.radii), fl.geom_batched, _ptr(fl.alpha),
                                    _ptr(fl.beta), fl.ab_batched, _ptr(tab), _ptr(dens_t), _ptr(out), sp), what)
    out = torch.movedim(axes.restore(out), -1, 0)     # (d, ...(first), B), the plan's axes
    if list(op.perm) != list(range(d)):
        out = out[_inverse_perm(op.perm)]
    return op.origin.give(out.contiguous(), complex_out=False)
