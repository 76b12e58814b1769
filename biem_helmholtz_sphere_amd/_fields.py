"""Field evaluation from a result record (reference ``biem_u``, ``_biem.py:822-977``) and its extensions: the gradient, the field
inside penetrable fluid balls, the total field and the far-field pattern about the origin.  Every function only reads the
record's attributes."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Callable, Tuple

import numpy as np
import torch

from . import _lib as L
from ._arrays import Array, _Origin, _host_array, _inverse_perm, _is_complex, _ptr, _result_origin, _shape, _stacked, _stream_ptr, _to_dev
from ._coords import canonical_tree, n_end_from_harm
from ._operator import _Flat, _RhsAxes, _flatten
from ._plans import _Plan, _label_positions, _plan


# --------------------------------------------------------------------------------------
# field evaluation (reference biem_u :822-977)
# --------------------------------------------------------------------------------------
def biem_u(res: Any, x: Array, /, far_field: bool = False, per_ball: bool = False, expand_x: bool = True) -> Array:
    """Scattered field at cartesian x of shape (c_ndim, ...(x)) [expand_x] or (c_ndim, ...(x), ...(first)).

    The near field is NaN (for every ball of ``per_ball=True``) where its series is not valid: ``kind="outer"`` inside any ball,
    ``kind="inner"`` outside any ball.  So ``kind="inner"`` with B >= 2 marks every point NaN unless it lies inside ALL balls -
    for disjoint balls, every point; the oracle's mask and the kernels' alike.  The far field has no mask.
    """
    return _field(res, x, far_field=far_field, per_ball=per_ball, expand_x=expand_x, grad=False)


# orders the per-lane gradient kernels cover (csrc/kernels_uscat.hip: kFastNendMax*), by canonical tree
USCAT_GRAD_N_END_MAX = {"a": 320, "ba": 48, "bba": 14, "caa": 12}


def biem_u_grad(res: Any, x: Array, /, per_ball: bool = False, expand_x: bool = True) -> Array:
    """Cartesian gradient of the scattered field at x (as :func:`biem_u` takes it), component axis first.

    Shape ``(c_ndim, ...(x), ...(first))``, with a trailing ``B`` for ``per_ball=True`` - the convention of ``uin_grad``, so
    ``uscat_grad(x) + uin_grad(x)`` is the gradient of the total field.  Components are in the caller's axis order for every
    tree.  NaN in every component where :func:`biem_u` gives NaN; a point on an axis of the coordinate tree is an ordinary point.
    Built for the trees a, ba, bpa, bba, bpbpa, caa up to n_end 320 / 48 / 14 / 12 (2-D / 3-D / bba / caa);
    ``NotImplementedError`` beyond that and for the chain trees d >= 5.
    """
    return _field(res, x, far_field=False, per_ball=per_ball, expand_x=expand_x, grad=True)


# order of the radial tables the plan build and the field kernels share (csrc/common.hpp: kMaxRad)
RADIAL_TABLE_ORDER = 320
_HESS_LAYOUTS: dict = {}


def _hess_layout(tree: str, n_end: int, dev: torch.device) -> Tuple[_Plan, torch.Tensor]:
    """The plan of order n_end + 2 and, per harmonic of the order-n_end plan, its place in that plan's layout (matched by label: the
    shorter list is no prefix of the longer one - tree a lists m = 0 .. n_end - 1 and then the negative m).  Cached like the plans."""
    big = _plan(tree, n_end + 2, dev)
    key = (tree, int(n_end), big.dev.index, big.chain)
    hit = _HESS_LAYOUTS.get(key)
    if hit is None:
        small = _plan(tree, n_end, dev)
        where = {tuple(lab) + (int(n),): i for i, (lab, n) in enumerate(zip(big.labels.tolist(), big.degrees.tolist()))}
        idx = [where[tuple(lab) + (int(n),)] for lab, n in zip(small.labels.tolist(), small.degrees.tolist())]
        if len(set(idx)) != small.H:
            raise RuntimeError(f"the labels of tree {tree!r} at n_end={n_end} do not embed one to one into those at n_end={n_end + 2}")
        hit = _HESS_LAYOUTS[key] = (big, torch.as_tensor(idx, dtype=torch.long, device=big.dev))
    return hit


def biem_u_hess(res: Any, x: Array, /, per_ball: bool = False, expand_x: bool = True) -> Array:
    r"""Cartesian Hessian of the scattered field at x (as :func:`biem_u` takes it), both component axes first.

    Shape ``(c_ndim, c_ndim, ...(x), ...(first))``, with a trailing ``B`` for ``per_ball=True``, complex128, in the namespace of
    :func:`biem_u_grad`.  Both component axes are in the caller's axis order for every tree; the result is exactly symmetric (the
    lower triangle is a copy of the upper) and NaN in all components exactly where :func:`biem_u` is NaN.  Both kinds.

    Nothing is differenced: a derivative of a multipole expansion is a multipole expansion about the same centre, one degree longer,
    :math:`(D_i c)_{h'} = k\,\mathrm{sgn}(n_h - n_{h'}) \sum_h T^i_{h'h} c_h` with the coupling table of :func:`biem_force`, so the
    Hessian is the value kernels of :func:`biem_u` applied to :math:`D_j D_i c` at order ``n_end + 2``.  Every tree
    and order :func:`biem_u` covers at ``n_end + 2`` is covered - the chain trees d >= 5 and orders above the ceilings of
    :func:`biem_u_grad` included; ``NotImplementedError`` beyond that.  The first call of a (tree, n_end, device) builds the plan of
    order ``n_end + 2``.
    """
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    if res.kind not in ("outer", "inner"):
        raise ValueError(f"Invalid kind: {res.kind}")
    c = res.c
    tree, perm = canonical_tree(c.branching_types_expression_str)
    d = c.c_ndim
    n_end = n_end_from_harm(tree, int(res.density.shape[-1]))
    if d >= 3 and 2 * (n_end + 2) > RADIAL_TABLE_ORDER:
        raise NotImplementedError(
            f"uscat_hess evaluates the field at order n_end + 2 = {n_end + 2}; for tree {c.branching_types_expression_str!r} the plan of "
            f"that order needs radial tables of order {2 * (n_end + 2)}, above the built {RADIAL_TABLE_ORDER}")
    lib = L.load()                                         # (a library that is missing is reported before a device that is)
    f = _field_operands(res, x, tree, perm, expand_x)
    plan, idx = _hess_layout(tree, n_end, f.dev)
    fl, dev = f.fl, f.dev
    nb, B, P = fl.nb, fl.B, int(f.pts.shape[1])
    dens = torch.zeros((nb, B, plan.H), dtype=torch.complex128, device=dev)
    dens[:, :, idx] = f.density
    flags = f.flags | (L.USCAT_PER_BALL if per_ball else 0) | (L.USCAT_KIND_INNER if res.kind == "inner" else 0)
    balls = (B,) if per_ball else ()
    pairs = [(i, j) for i in range(d) for j in range(i, d)]
    upper = torch.empty((len(pairs), P, nb) + balls, dtype=torch.complex128, device=dev)
    with torch.cuda.device(dev):
        wb = int(lib.biem_uscat_hess_workspace_bytes(plan.handle, nb, B))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
        if P > 0 and nb > 0:
            rc = lib.biem_uscat_hess(plan.handle, nb, B, P, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                                     _ptr(dens), _ptr(f.pts), flags, _ptr(upper), _ptr(work), wb, _stream_ptr(dev))
            _check_built(lib, rc, "biem_uscat_hess")
    inv = _inverse_perm(perm)                              # canonical component of each of the caller's axes
    at = {p: q for q, p in enumerate(pairs)}
    out = torch.empty((d, d, P, nb) + balls, dtype=torch.complex128, device=dev)
    for i in range(d):
        for j in range(d):
            a, b = inv[i], inv[j]
            out[i, j] = upper[at[(min(a, b), max(a, b))]]
    return f.origin.give(out.reshape((d, d) + f.xshape + f.batch + balls))


def _check_built(lib, rc: int, entry: str) -> None:
    """L.check, with BIEM_ERR_UNSUPPORTED (a limit only the library knows: the LDS of the per-lane rows in 2-D) as NotImplementedError."""
    if rc == L.BIEM_ERR_UNSUPPORTED:
        msg = lib.biem_last_error()
        raise NotImplementedError(msg.decode() if msg else f"{entry}: not built for this size")
    L.check(rc, entry)


def _check_covered(what: str, c: Any, tree: str, n_end: int, beyond: str) -> None:
    """NotImplementedError unless the per-lane kernels cover (tree, n_end); `beyond`: what the trees and orders outside them are left with."""
    if n_end > USCAT_GRAD_N_END_MAX.get(tree, 0):
        cov = ", ".join(f"{t} (n_end <= {n})" for t, n in USCAT_GRAD_N_END_MAX.items())
        raise NotImplementedError(
            f"{what} is not built for tree {c.branching_types_expression_str!r} at n_end={n_end}; covered: {cov}, "
            f"bpa and bpbpa as ba and bba; the chain trees d >= 5 and larger orders have {beyond}")


@dataclass
class _FieldOperands:
    """The flattened device operands of one field evaluation (biem_u, biem_u_grad, biem_u_interior, biem_u_interior_grad)."""

    origin: _Origin
    dev: torch.device
    fl: _Flat
    plan: _Plan
    pts: torch.Tensor         # [d, P] or [d, P, nb] (flags: USCAT_POINTS_BATCHED), canonical axes
    density: torch.Tensor     # [nb, B, H]
    flags: int
    xshape: Tuple[int, ...]
    batch: Tuple[int, ...]


def _field_operands(res: Any, x: Array, tree: str, perm, expand_x: bool, extra_batch=()) -> _FieldOperands:
    """extra_batch: leading shapes of further per-system operands, broadcast into the batch shape."""
    c = res.c
    origin, dev = _result_origin(res, x)
    f64 = torch.float64
    k_t = _to_dev(res.k, dev, torch.complex128)
    eta_t = _to_dev(res.eta, dev, f64)
    cen_t = _to_dev(res.centers, dev, f64)[list(perm)]   # [d, ...(first), B], canonical axes
    rad_t = _to_dev(res.radii, dev, f64)            # [...(first), B]
    dens_t = _to_dev(res.density, dev, torch.complex128)
    d = c.c_ndim
    H = int(dens_t.shape[-1])
    n_end = n_end_from_harm(tree, H)
    ndim_first = k_t.ndim
    batch = tuple(np.broadcast_shapes(tuple(k_t.shape), tuple(eta_t.shape), tuple(cen_t.shape[1:-1]), tuple(rad_t.shape[:-1]),
                                      tuple(dens_t.shape[:-2]), *extra_batch))
    fl = _flatten(batch, torch.movedim(cen_t, 0, -1), rad_t, k_t, eta_t)
    nb, B = fl.nb, fl.B
    plan = _plan(tree, n_end, dev)

    x_t = _to_dev(_stacked(x), dev, f64)
    if x_t.shape[0] != d:
        raise ValueError(f"x must have shape ({d}, ...), got {tuple(x_t.shape)}")
    x_t = x_t[list(perm)]
    if expand_x:
        xshape = tuple(x_t.shape[1:])
        pts = x_t.reshape(d, -1).contiguous()
        flags = 0
    else:
        nx = x_t.ndim - 1 - ndim_first
        if nx < 0:
            raise ValueError("expand_x=False needs x of shape (c_ndim, ...(x), ...(first))")
        xshape = tuple(x_t.shape[1:1 + nx])
        pts = x_t.expand((d,) + xshape + batch).reshape(d, -1, nb).contiguous()
        flags = L.USCAT_POINTS_BATCHED
    df = dens_t.expand(batch + (B, H)).reshape(nb, B, H).contiguous()
    return _FieldOperands(origin, dev, fl, plan, pts, df, flags, xshape, batch)


def _launch(f: _FieldOperands, perm, base: str, extra: tuple, flags: int, *, grad: bool, per_ball: bool = False) -> Array:
    """What the field evaluations share around their one library call: the output ([d,] P, nb [, B]), the workspace of
    `base`_workspace_bytes, the entry `base` (gradient: `base`_grad) with its `extra` arguments after the geometry, the gradient's
    components back along the caller's axes, and the result in the caller's shape and namespace."""
    lib, fl, plan, dev = L.load(), f.fl, f.plan, f.dev
    nb, B, d, P = fl.nb, fl.B, int(f.pts.shape[0]), int(f.pts.shape[1])
    comp, balls = ((d,) if grad else ()), ((B,) if per_ball else ())
    out = torch.empty(comp + (P, nb) + balls, dtype=torch.complex128, device=dev)
    what = base + "_grad" if grad else base
    with torch.cuda.device(dev):
        wb = int(getattr(lib, base + "_workspace_bytes")(plan.handle, nb, B))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
        if P > 0 and nb > 0:
            rc = getattr(lib, what)(plan.handle, nb, B, P, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                                    *extra, _ptr(f.density), _ptr(f.pts), flags, _ptr(out), _ptr(work), wb, _stream_ptr(dev))
            if what == "biem_uscat":
                L.check(rc, what)
            else:
                _check_built(lib, rc, what)
    if grad and list(perm) != list(range(d)):
        out = out[_inverse_perm(perm)]
    return f.origin.give(out.reshape(comp + f.xshape + f.batch + balls))


def _field(res: Any, x: Array, *, far_field: bool, per_ball: bool, expand_x: bool, grad: bool) -> Array:
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    if res.kind not in ("outer", "inner"):
        raise ValueError(f"Invalid kind: {res.kind}")
    c = res.c
    tree, perm = canonical_tree(c.branching_types_expression_str)
    if grad:
        _check_covered("uscat_grad", c, tree, n_end_from_harm(tree, int(res.density.shape[-1])), "uscat() only")
    L.load()                                               # (a library that is missing is reported before a device that is)
    f = _field_operands(res, x, tree, perm, expand_x)
    flags = (f.flags | (L.USCAT_FAR_FIELD if far_field else 0) | (L.USCAT_PER_BALL if per_ball else 0)
             | (L.USCAT_KIND_INNER if res.kind == "inner" else 0))
    return _launch(f, perm, "biem_uscat", (), flags, grad=grad, per_ball=per_ball)


# --------------------------------------------------------------------------------------
# the total field inside penetrable fluid balls (an extension)
# --------------------------------------------------------------------------------------
def biem_u_interior(res: Any, x: Array, /, *, k_interior: Array, density_ratio: Array, expand_x: bool = True) -> Array:
    r"""Total field inside the penetrable fluid balls of a :func:`biem` result solved with :func:`fluid_inclusion_bc`.

    ``x`` as :func:`biem_u` takes it; ``k_interior`` and ``density_ratio`` as :func:`fluid_inclusion_bc` takes them (they broadcast
    to ``(..., B)``, real or complex).  The result has the shape and namespace of ``biem_u(res, x, expand_x=expand_x)``.  A point with
    ``|x - c_b| < rho_b`` gets :math:`u_b(x) = \sum_h a_{b,h} j_n(k_b |x - c_b|) Y_h`, every other point NaN: exactly the complement of
    where :func:`biem_u` is valid (a point at ``r == rho`` belongs to the exterior).  The coefficients follow algebraically from the
    density, :math:`a = -s\,\delta_b k W / gj_n` with :math:`s` = density x blc_n and :math:`W = i / (k\rho_b)^{d-1}`: no second solve.

    A ball whose ``k_interior`` is NaN is impenetrable: NaN inside it.  ``density_ratio = 0`` (the sound-soft limit) gives 0 inside.
    A degree the ball does not scatter (``gj_n = 0``: the transparent sphere ``k_b = k, delta = 1``) leaves no trace in the density, so
    the field inside that ball cannot be recovered from it: NaN inside, no error.

    ``ValueError`` for ``kind != "outer"``, a result without density, ``k_interior * radii == 0`` and shapes that do not broadcast.
    Built for the trees a, ba, bpa, bba, bpbpa, caa up to n_end 320 / 48 / 14 / 12 (2-D / 3-D / bba / caa) while the per-lane
    rows fit the LDS (2-D: n_end <= 152); ``NotImplementedError`` beyond that and for the chain trees d >= 5.
    """
    return _interior(res, x, k_interior, density_ratio, expand_x, grad=False)


def _interior(res: Any, x: Array, k_interior: Array, density_ratio: Array, expand_x: bool, *, grad: bool) -> Array:
    """biem_u_interior (grad=False) and biem_u_interior_grad (grad=True): one set of checks and operands, two library entries."""
    what = "uinterior_grad" if grad else "uinterior"
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    if res.kind != "outer":
        raise ValueError(f"Invalid kind: {res.kind} (the interior field belongs to an exterior problem, kind='outer')")
    c = res.c
    tree, perm = canonical_tree(c.branching_types_expression_str)
    _check_covered(what, c, tree, n_end_from_harm(tree, int(res.density.shape[-1])), "no interior field")
    rs, ks, kis, dls = _shape(res.radii), _shape(res.k), _shape(k_interior), _shape(density_ratio)
    B = rs[-1]
    try:
        full = np.broadcast_shapes(kis, dls, rs)
        if full[-1] != B or len(kis) > len(ks) + 1 or len(dls) > len(ks) + 1:
            raise ValueError
        np.broadcast_shapes(full[:-1], ks)
    except ValueError as e:
        raise ValueError(
            "Shapes of k_interior, density_ratio and the batch shape + (B,) are not broadcastable\n"
            f"tuple(k_interior.shape)={kis}\ntuple(density_ratio.shape)={dls}\ntuple(radii.shape)={rs}\ntuple(k.shape)={ks}") from e
    if np.any(_host_array(k_interior) * _host_array(res.radii) == 0):
        raise ValueError("k_interior * radii must not be zero")

    L.load()                                               # (a library that is missing is reported before a device that is)
    f = _field_operands(res, x, tree, perm, expand_x, extra_batch=(kis[:-1], dls[:-1]))
    nb, batch = f.fl.nb, f.batch
    kb_t, dl_t = (_to_dev(a, f.dev, torch.complex128) for a in (k_interior, density_ratio))
    fluid_b = any(s != 1 for s in tuple(kb_t.shape[:-1]) + tuple(dl_t.shape[:-1]))

    def per_ball(t):                                       # [nb, B], or [1, B] shared by all systems
        t = t.expand(tuple(torch.broadcast_shapes(tuple(t.shape), (B,))))
        return (t.expand(batch + (B,)).reshape(nb, B) if fluid_b else t.reshape(1, B)).contiguous()

    kb_f, dl_f = per_ball(kb_t), per_ball(dl_t)
    return _launch(f, perm, "biem_uinterior", (_ptr(kb_f), _ptr(dl_f), int(fluid_b)), f.flags, grad=grad)


def biem_u_interior_grad(res: Any, x: Array, /, *, k_interior: Array, density_ratio: Array, expand_x: bool = True) -> Array:
    r"""Cartesian gradient of the field inside the penetrable fluid balls, component axis first.

    Arguments, checks, broadcasting and namespace as :func:`biem_u_interior`; shape ``(c_ndim, ...(x), ...(first))`` like
    :func:`biem_u_grad`, components in the caller's axis order for every tree.  Inside ball ``b`` it is the term-by-term gradient of
    the series of :func:`biem_u_interior`, :math:`\nabla (j_n Y_h) = -k_b j_{n+1}(k_b r) Y_h e + (j_n(k_b r) / r) (\nabla S_h)(e)`
    with the solid harmonic :math:`S_h`, a form that never divides by a sine: the centre of a ball and points on the axes of the
    coordinate tree are ordinary points.  NaN in every component exactly where :func:`biem_u_interior` is NaN (a point in no ball,
    an impenetrable ball, a ball whose interior field the density does not determine); ``density_ratio = 0`` gives exactly 0.

    Built for the trees a, ba, bpa, bba, bpbpa, caa up to n_end 320 / 48 / 14 / 12 (2-D / 3-D / bba / caa) while the per-lane
    rows fit the LDS (2-D: n_end <= 152); ``NotImplementedError`` beyond that and for the chain trees d >= 5.
    """
    return _interior(res, x, k_interior, density_ratio, expand_x, grad=True)


def _inside_or(inside: Array, outside: Array, uin: Array) -> Array:
    """`inside` where it has a value, `uin + outside` where it is NaN, in the namespace, dtype and on the device of `inside`."""
    if isinstance(inside, torch.Tensor):
        uin = uin.to(inside.device) if isinstance(uin, torch.Tensor) else torch.as_tensor(np.asarray(uin), device=inside.device)
        return torch.where(torch.isnan(inside.real), (uin + outside).to(inside.dtype), inside)
    uin = uin.detach().cpu().numpy() if isinstance(uin, torch.Tensor) else np.asarray(uin)
    return np.where(np.isnan(inside.real), (uin + outside).astype(inside.dtype), inside)


def biem_u_total(res: Any, x: Array, /, *, k_interior: Array, density_ratio: Array, expand_x: bool = True) -> Array:
    """Total field everywhere: ``res.uin(x) + uscat(x)`` outside all balls, :func:`biem_u_interior` inside them.

    Arguments, shape and namespace as :func:`biem_u_interior`.  NaN remains only inside an impenetrable ball (``k_interior`` NaN) or
    one whose interior field cannot be recovered from the density.  ``ValueError`` if the result carries no ``uin``.
    """
    if res.uin is None:
        raise ValueError("The BIEMResult does not have uin.")
    inside = biem_u_interior(res, x, k_interior=k_interior, density_ratio=density_ratio, expand_x=expand_x)
    outside = biem_u(res, x, expand_x=expand_x)
    uin = res.uin(x, expand_x=expand_x)
    return _inside_or(inside, outside, uin)


def biem_u_total_grad(res: Any, x: Array, /, *, k_interior: Array, density_ratio: Array, uin_grad: Callable[[Array], Array],
                      expand_x: bool = True) -> Array:
    """Gradient of the total field everywhere: ``uin_grad(x) + uscat_grad(x)`` outside all balls, :func:`biem_u_interior_grad` inside.

    Arguments, shape and namespace as :func:`biem_u_interior_grad`.  The result record keeps no gradient of the incident field, so
    ``uin_grad`` - the callable :func:`biem` took - is a required keyword; for ``expand_x=True`` it is called with ``x`` extended by
    the trailing singleton batch axes that ``res.uin`` adds.  NaN remains only inside an impenetrable ball (``k_interior`` NaN) or
    one whose interior field cannot be recovered from the density.

    Across a surface the tangential components are continuous, while the normal component jumps by the factor ``density_ratio``:
    the transmission condition is continuity of ``(1 / density) d_n u``, so ``d_n u_interior = density_ratio * d_n u_exterior``.
    That is physics, not an error of the evaluation.
    """
    inside = biem_u_interior_grad(res, x, k_interior=k_interior, density_ratio=density_ratio, expand_x=expand_x)
    outside = biem_u_grad(res, x, expand_x=expand_x)
    if expand_x:
        x = _stacked(x)[(...,) + (None,) * len(_shape(res.k))]
    uin = uin_grad(x)
    return _inside_or(inside, outside, uin)


def _raised_layout(tree: str, n_end: int, n_out: int, dev: torch.device) -> Tuple[_Plan, torch.Tensor]:
    """The plan of order n_out >= n_end and, per harmonic of the order-n_end plan, its place on that plan's axis, matched by label (the
    axis of a larger order does not begin with the smaller one, as _hess_layout)."""
    big = _plan(tree, n_out, dev)
    return big, torch.as_tensor(_label_positions(tree, n_end, n_out, dev), dtype=torch.long, device=big.dev)


def biem_cluster_coefficients(res: Any, /, *, origin: Array | None = None, n_out: int | None = None, _stage: int = 0) -> Array:
    r"""Outgoing coefficients of the scattered field of the whole cluster about ``origin``: ``A`` of shape ``(...(first), H_out)``,
    complex128, the right-hand-side axes of the density included, with

        u_scat(x) = sum_h'' A_h'' h_n''(k |x - o|) Y_h''((x - o)^)    for |x - o| > max_b (|c_b - o| + rho_b),
        A_h'' = sum_b sum_h (R|R)_{h->h''}(o - c_b) c_{b,h},            c = density x blc (the coefficients of :func:`biem_u`),

    ``h''`` along ``harmonic_labels(c, n_out)``.  ``origin`` has shape ``(c_ndim,)`` or ``(c_ndim, ...)`` broadcastable to the axes of
    the systems (default: the zero vector) and may lie anywhere; ``n_out`` (default ``n_end``, at least ``n_end``) is the order the
    expansion is truncated at - the translation of a ball off the origin feeds every degree, so a cluster of radius R about o wants
    ``n_out`` well above ``k R``.  Axes of the density on which k, eta, the geometry and the origin have size 1 are right-hand sides of
    one translation table.  ``kind="outer"`` only.  Real and complex k, every tree :func:`biem_u` covers; ``NotImplementedError``
    above the order of the translation term lists (n_out > 320 in 2-D, > 160 elsewhere).  The result is bit-reproducible."""
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    if res.kind != "outer":
        raise ValueError(f"Invalid kind: {res.kind} (kind='inner' has no outgoing expansion: cluster_coefficients needs kind='outer')")
    c = res.c
    tree, perm = canonical_tree(c.branching_types_expression_str)
    d = c.c_ndim
    o_origin, dev = _result_origin(res, res.density if origin is None else origin)
    f64 = torch.float64
    dens_t = _to_dev(res.density, dev, torch.complex128)
    H = int(dens_t.shape[-1])
    n_end = n_end_from_harm(tree, H)
    n_out = n_end if n_out is None else int(n_out)
    if n_out < n_end:
        raise ValueError(f"n_out={n_out} must be at least n_end={n_end}")
    k_t = _to_dev(res.k, dev, torch.complex128)
    eta_t = _to_dev(res.eta, dev, f64)
    cen_t = _to_dev(res.centers, dev, f64)[list(perm)]     # [d, ...(first), B], canonical axes
    rad_t = _to_dev(res.radii, dev, f64)
    nd = dens_t.ndim - 2
    o_t = torch.zeros((d,) + (1,) * nd, dtype=f64, device=dev) if origin is None else _to_dev(_stacked(origin), dev, f64)
    if o_t.ndim < 1 or o_t.shape[0] != d:
        raise ValueError(f"origin must have shape ({d},) or ({d}, ...), got {tuple(o_t.shape)}")
    if o_t.ndim == 1:
        o_t = o_t.reshape((d,) + (1,) * nd)
    o_t = o_t[list(perm)]
    try:
        batch = tuple(np.broadcast_shapes(tuple(k_t.shape), tuple(eta_t.shape), tuple(cen_t.shape[1:-1]), tuple(rad_t.shape[:-1]),
                                          tuple(o_t.shape[1:])))
        batch = (1,) * (nd - len(batch)) + batch
        full = tuple(np.broadcast_shapes(batch, tuple(dens_t.shape[:-2])))
        if len(full) != nd:
            raise ValueError
    except ValueError as e:
        raise ValueError("Shapes of origin[1:], the batch and the density are not broadcastable\n"
                         f"tuple(origin.shape)={tuple(o_t.shape)}\ntuple(density.shape)={tuple(dens_t.shape)}\ntuple(k.shape)={tuple(k_t.shape)}") from e
    axes = _RhsAxes.of(batch, full)
    fl = _flatten(batch, torch.movedim(cen_t, 0, -1), rad_t, k_t, eta_t)
    nb, B, nrhs = fl.nb, fl.B, axes.nrhs
    obatched = int(any(s != 1 for s in o_t.shape[1:]))
    of = (torch.movedim(o_t, 0, -1).expand(batch + (d,)).reshape(nb, d) if obatched else o_t.reshape(1, d)).contiguous()
    out = _cluster_flat(tree, n_end, n_out, fl, of, obatched, axes.lay_out(dens_t.expand(full + (B, H))), dev, int(_stage))
    return o_origin.give(axes.restore(out).contiguous())


def _cluster_flat(tree: str, n_end: int, n_out: int, fl: _Flat, of: torch.Tensor, obatched: int, dens: torch.Tensor, dev: torch.device,
                  stage: int = 0) -> torch.Tensor:
    """biem_cluster_coefficients on flattened operands: the densities dens [nb, nrhs, B, H] of order n_end, the origins of [nb or 1, d] in
    canonical axes; returns [nb, nrhs, H_out].  For n_out > n_end the density goes onto the axis of the larger plan by label."""
    nb, B, nrhs = fl.nb, fl.B, int(dens.shape[1])
    if n_out == n_end:
        plan = _plan(tree, n_end, dev)
        dens = dens.contiguous()
    else:
        plan, idx = _raised_layout(tree, n_end, n_out, dev)
        small = dens
        dens = torch.zeros((nb, nrhs, B, plan.H), dtype=torch.complex128, device=dev)
        dens[..., idx] = small
    out = torch.empty((nb, nrhs, plan.H), dtype=torch.complex128, device=dev)
    lib = L.load()
    with torch.cuda.device(dev):
        wb = int(lib.biem_cluster_coefficients_workspace_bytes(plan.handle, nb, B, nrhs))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
        if nb > 0 and nrhs > 0:
            rc = lib.biem_cluster_coefficients(plan.handle, nb, B, nrhs, n_end, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii),
                                               fl.geom_batched, _ptr(of), obatched, _ptr(dens), _ptr(out), stage, _ptr(work), wb,
                                               _stream_ptr(dev))
            _check_built(lib, rc, "biem_cluster_coefficients")
    return out


def biem_far_pattern(res: Any, directions: Array, /, per_ball: bool = False) -> Array:
    r"""Far-field pattern of the cluster about the origin: :math:`u_{scat}(r \hat x) \to F(\hat x)\, e^{ikr} / r^{(d-1)/2}`,

        F(x^) = (ik)^{-(d-1)/2} sum_b e^{-ik x^.c_b} sum_h c_{b,h} (-i)^n Y_h(x^).

    ``directions`` has shape ``(c_ndim, ...)`` and is normalised here (a zero vector gives NaN); the result has shape
    ``(..., ...(first))``, with a trailing ``B`` for ``per_ball=True``, in the namespace of :func:`biem_u`.  Real and complex ``k``.
    Unlike ``uscat(x, far_field=True)``, which keeps the reference's formula - harmonics at the direction of ``x - c_b`` and the phase
    of ``x`` itself, the pattern of a ball at the origin only - this is the pattern of the whole cluster for balls anywhere.
    """
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    origin, dev = _result_origin(res, directions)
    f64 = torch.float64
    x_t = _to_dev(_stacked(directions), dev, f64)
    d = res.c.c_ndim
    if x_t.shape[0] != d:
        raise ValueError(f"directions must have shape ({d}, ...), got {tuple(x_t.shape)}")
    xh = x_t / torch.linalg.vector_norm(x_t, dim=0, keepdim=True)
    ok = torch.isfinite(xh).all(dim=0, keepdim=True)
    e0 = torch.zeros((d,) + (1,) * (x_t.ndim - 1), dtype=f64, device=dev)
    e0[0] = 1.0
    cen_t = _to_dev(res.centers, dev, f64)             # [d, ...(first), B]
    k_t = _to_dev(res.k, dev, torch.complex128 if _is_complex(res.k) else f64)
    # every ball moved to the origin: there the reference's far-field formula IS the pattern of that ball
    at_origin = SimpleNamespace(c=res.c, centers=torch.zeros_like(cen_t), radii=_to_dev(res.radii, dev, f64), k=k_t, n_end=res.n_end,
                                eta=_to_dev(res.eta, dev, f64), kind=res.kind, density=_to_dev(res.density, dev, torch.complex128))
    pb = biem_u(at_origin, torch.where(ok, xh, e0), far_field=True, per_ball=True)         # (..., ...(first), B)
    nd, nfirst = x_t.ndim - 1, cen_t.ndim - 2
    dot = torch.sum(xh[(...,) + (None,) * (nfirst + 1)] * cen_t[(slice(None),) + (None,) * nd], dim=0)
    out = pb * torch.exp(-1j * k_t[..., None] * dot)   # (a direction that was zero: NaN through the phase)
    return origin.give(out if per_ball else out.sum(-1))
