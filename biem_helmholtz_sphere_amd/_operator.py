"""The operator of one call: input checks (reference ``_biem.py:240-326``), the operands on the device, the plan, the boundary
samples of an incident field and the small library calls that biem(), biem_factorize() and the observables share."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._arrays import _Origin, _host_array, _inverse_perm, _is_complex, _origin_of, _ptr, _shape, _to_dev
from ._coords import canonical_tree
from ._incident import _harm_n_ndim_le, _harmonic_order
from ._plans import _Plan, _label_positions, _plan


# --------------------------------------------------------------------------------------
# input checking (reference :240-326; error and warning texts are part of the API)
# --------------------------------------------------------------------------------------
def _validate_biem_inputs(c, centers, radii, k, eta, alpha, beta) -> Tuple[int, ...]:
    """Shape / dtype checks of reference :240-326 on metadata only (no device needed); returns the batch shape."""
    for nm, a in (("centers", centers), ("radii", radii), ("k", k)):
        if not isinstance(a, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{nm} must be an array (torch.Tensor or numpy.ndarray), got {type(a).__name__}")
    if eta is not None and _is_complex(eta):
        raise ValueError("The decoupling parameter must be real.")
    ks, cs, rs = _shape(k), _shape(centers), _shape(radii)
    es = (1,) * len(ks) if eta is None else _shape(eta)
    als = _shape(alpha) or (1,) * (len(ks) + 1)
    bes = _shape(beta) or (1,) * (len(ks) + 1)
    if len({len(ks), len(es), len(cs) - 2, len(rs) - 1}) != 1:
        raise ValueError(f"k.ndim={len(ks)}, eta.ndim={len(es)}, centers.ndim - 2={len(cs) - 2}, radii.ndim -1={len(rs) - 1}are not the same.")
    if len(als) != len(ks) + 1 or len(bes) != len(ks) + 1:
        raise ValueError(f"alpha and beta must be scalars or arrays of shape (..., B) with {len(ks) + 1} axes")
    try:
        batch = np.broadcast_shapes(ks, es, cs[:-2], rs[:-1], als[:-1], bes[:-1])
    except ValueError as e:
        raise ValueError(
            "Shapes of k, eta and " "centers.shape[:-2], radii.shape[:-1] " "are not broadcastable\n"
            f"tuple(k.shape)={ks}\ntuple(eta.shape)={es}\ntuple(centers.shape)={cs}\ntuple(radii.shape)={rs}\n"
            f"tuple(alpha.shape)={als}\ntuple(beta.shape)={bes}"
        ) from e
    try:
        np.broadcast_shapes(cs[:-1], rs, als, bes)
    except ValueError as e:
        raise ValueError(
            "centers.shape[:-1] and radii.shape " "are not broadcastable\n"
            f"tuple(centers.shape)={cs}\ntuple(radii.shape)={rs}\ntuple(alpha.shape)={als}\ntuple(beta.shape)={bes}"
        ) from e
    if cs[-1] != c.c_ndim:
        raise ValueError(f"The last dimension of centers must be c.c_ndim={c.c_ndim}, but got {cs[-1]}")
    return tuple(batch)


def _is_default(v: Any, default: float) -> bool:
    return isinstance(v, (int, float, complex)) and not isinstance(v, bool) and v == default


def _validate_degree_bc(batch, ks, B: int, n_end: int, alpha, beta, alpha_n, beta_n) -> Tuple[int, ...]:
    """Checks of the degree-dependent pair alpha_n / beta_n of shape (..., B, n_end) on metadata only; returns the batch shape
    with their leading axes broadcast in."""
    if (alpha_n is None) != (beta_n is None):
        raise ValueError("alpha_n and beta_n must be given together")
    if not (_is_default(alpha, 1.0) and _is_default(beta, 0.0)):
        raise ValueError("alpha_n / beta_n replace alpha / beta: leave alpha and beta at their defaults when alpha_n and beta_n are given")
    ans, bns = _shape(alpha_n), _shape(beta_n)
    for nm, sh in (("alpha_n", ans), ("beta_n", bns)):
        if len(sh) != len(ks) + 2:
            raise ValueError(f"{nm} must be an array of shape (..., B, n_end) with {len(ks) + 2} axes, got shape {sh}")
        if sh[-1] != n_end:
            raise ValueError(f"The last dimension of {nm} must be n_end={n_end}, but got {sh[-1]}")
    try:
        np.broadcast_shapes(ans[-2:-1], bns[-2:-1], (B,))
        if np.broadcast_shapes(ans[-2:-1], (B,)) != (B,) or np.broadcast_shapes(bns[-2:-1], (B,)) != (B,):
            raise ValueError
        return tuple(np.broadcast_shapes(tuple(batch), ans[:-2], bns[:-2]))
    except ValueError as e:
        raise ValueError(
            "Shapes of alpha_n, beta_n and the batch shape + (B, n_end) " "are not broadcastable\n"
            f"tuple(alpha_n.shape)={ans}\ntuple(beta_n.shape)={bns}\nbatch shape={tuple(batch)}, B={B}, n_end={n_end}"
        ) from e


def _warn_biem_inputs(k: Any, eta: Any) -> None:
    """The two UserWarnings of reference :269-285 (texts verbatim, missing blanks included): eta == 0 somewhere; Im k < 0 or
    eta Re k < 0 somewhere.  Like the reference, which warns after ``xp.asarray(eta)``, the test runs on CONVERTED arrays, so
    k and eta may mix torch tensors (any device), NumPy arrays, lists and scalars.  (The reference's own test of the second
    one, :278-280, guards the Im k term with "eta is not castable to float64", which is never true once the complex-eta check
    above it has passed, so there only eta Re k < 0 can fire; here the condition the message states is checked.)"""
    if isinstance(k, torch.Tensor) and isinstance(eta, torch.Tensor) and k.is_cuda and eta.is_cuda and k.device == eta.device:
        # both on one GPU: ONE device -> host copy (each copy is a synchronisation; a call with one small system pays for every one)
        nk = k.numel()
        buf = torch.cat([k.detach().reshape(-1).to(torch.complex128), eta.detach().reshape(-1).to(torch.complex128)]).cpu().numpy()
        k_h = buf[:nk].reshape(tuple(k.shape))
        if not k.is_complex():
            k_h = k_h.real
        eta_h = buf[nk:].real.reshape(tuple(eta.shape))
    else:
        k_h = _host_array(k)
        eta_h = None if eta is None else _host_array(eta)
    if eta_h is not None and bool(np.any(eta_h == 0)):
        warnings.warn("The solution may be incorrect" "if k is an eigenvalue for laplacian" "on the interior region with"
                      "Neumann boundary condition.", UserWarning, stacklevel=4)
    k_re = k_h.real
    bad = (np.iscomplexobj(k_h) and bool(np.any(k_h.imag < 0))) or bool(np.any((k_re if eta_h is None else eta_h * k_re) < 0))
    if bad:
        warnings.warn("The solution may be incorrectif not (Im k >= 0 and eta Re k >= 0).", UserWarning, stacklevel=4)


@dataclass
class _Flat:
    """Flattened, contiguous device operands of one biem() call (biem_u: the geometry only, alpha / beta None)."""

    nb: int
    B: int
    k: torch.Tensor          # [nb]
    eta: torch.Tensor        # [nb]
    centers: torch.Tensor    # [nb or 1, B, d]
    radii: torch.Tensor      # [nb or 1, B]
    geom_batched: int
    alpha: Optional[torch.Tensor] = None     # [nb or 1, B] complex128; degree-dependent: [nb or 1, B, n_end]
    beta: Optional[torch.Tensor] = None
    ab_batched: int = 0


def _flatten(batch, centers_t, radii_t, k_t, eta_t, alpha_t=None, beta_t=None, degree_axis: int = 0) -> _Flat:
    nb = int(np.prod(batch)) if len(batch) else 1
    B, d = int(radii_t.shape[-1]), centers_t.shape[-1]
    kf = k_t.expand(batch).reshape(nb).contiguous()
    ef = eta_t.expand(batch).reshape(nb).contiguous()
    geom_b = any(s != 1 for s in tuple(centers_t.shape[:-2]) + tuple(radii_t.shape[:-1]))
    if geom_b:
        cf = centers_t.expand(tuple(batch) + (B, d)).reshape(nb, B, d).contiguous()
        rf = radii_t.expand(tuple(batch) + (B,)).reshape(nb, B).contiguous()
    else:
        cf = centers_t.reshape(1, B, d).contiguous()
        rf = radii_t.reshape(1, B).contiguous()
    if alpha_t is None:
        return _Flat(nb, B, kf, ef, cf, rf, int(geom_b))
    if degree_axis:
        ab_b = any(s != 1 for s in tuple(alpha_t.shape[:-2]) + tuple(beta_t.shape[:-2]))
        lead = (tuple(batch), nb) if ab_b else ((1,) * len(batch), 1)
        af, bf = (t.expand(lead[0] + (B, degree_axis)).reshape(lead[1], B, degree_axis).contiguous() for t in (alpha_t, beta_t))
        return _Flat(nb, B, kf, ef, cf, rf, int(geom_b), af, bf, int(ab_b))
    ab_b = any(s != 1 for s in tuple(alpha_t.shape[:-1]) + tuple(beta_t.shape[:-1]))
    if ab_b:
        af, bf = (t.expand(tuple(batch) + (B,)).reshape(nb, B).contiguous() for t in (alpha_t, beta_t))
    else:
        af, bf = (t.reshape(-1)[-t.shape[-1]:].expand(B).reshape(1, B).contiguous() for t in (alpha_t, beta_t))
    return _Flat(nb, B, kf, ef, cf, rf, int(geom_b), af, bf, int(ab_b))


@dataclass
class _Operator:
    """Everything of one biem() / biem_factorize() call that does not depend on the incident field."""

    c: Any
    n_end: int
    kind: str
    origin: _Origin
    dev: torch.device
    batch: Tuple[int, ...]
    perm: Tuple[int, ...]    # canonical axis i = the caller's axis perm[i]
    plan: _Plan
    fl: _Flat                # in canonical axes
    centers_t: torch.Tensor  # the caller's arrays on the device, caller's axes
    radii_t: torch.Tensor
    k_t: torch.Tensor
    eta_t: torch.Tensor
    k_complex: bool
    alpha: Any               # alpha / beta as given (Python scalars are tested for zero on the host) and on the device
    beta: Any
    alpha_t: torch.Tensor
    beta_t: torch.Tensor
    per_degree: bool = False # alpha / beta are the degree-dependent alpha_n / beta_n of shape (..., B, n_end); fl.alpha / fl.beta likewise
    k_given: Any = None      # k as the caller gave it (the wavenumber of a plane_wave_direction's callable)


def _operator(c, centers, radii, k, n_end, alpha, beta, eta, kind, alpha_n=None, beta_n=None) -> _Operator:
    """Input checks of reference :240-326, the operands on the device and the plan."""
    batch = _validate_biem_inputs(c, centers, radii, k, eta, alpha, beta)
    per_degree = alpha_n is not None or beta_n is not None
    if per_degree:
        batch = _validate_degree_bc(batch, _shape(k), _shape(radii)[-1], int(n_end), alpha, beta, alpha_n, beta_n)
        alpha, beta = alpha_n, beta_n                  # from here on the pair is (alpha_n, beta_n), one more trailing axis
    _warn_biem_inputs(k, eta)
    origin, dev = _origin_of(centers, radii, k, eta, alpha, beta)
    f64 = torch.float64
    centers_t = _to_dev(centers, dev, f64)
    radii_t = _to_dev(radii, dev, f64)
    k_t = _to_dev(k, dev, torch.complex128)     # the kernels take complex wavenumbers (Im k = 0: real special functions)
    if eta is None:
        eta_t = torch.ones((1,) * k_t.ndim, dtype=f64, device=dev)
    else:
        eta_t = _to_dev(eta, dev, f64)
    alpha_t, beta_t = (_to_dev(a, dev, torch.complex128) for a in (alpha, beta))
    alpha_t, beta_t = (t[(None,) * (k_t.ndim + 1)] if t.ndim == 0 else t for t in (alpha_t, beta_t))
    # trees with primed nodes run as their canonical tree in permuted axes (canonical component i = original perm[i])
    tree, perm = canonical_tree(c.branching_types_expression_str)
    plan = _plan(tree, n_end, dev)
    fl = _flatten(batch, centers_t if list(perm) == list(range(len(perm))) else centers_t[..., list(perm)], radii_t, k_t, eta_t,
                  alpha_t, beta_t, int(n_end) if per_degree else 0)
    return _Operator(c, n_end, kind, origin, dev, tuple(batch), perm, plan, fl, centers_t, radii_t, k_t, eta_t, _is_complex(k),
                     alpha, beta, alpha_t, beta_t, per_degree, k)


def _result_operator(res: Any, what: str, alpha, beta, alpha_n, beta_n, require=()) -> _Operator:
    """The operator of a result record and the coefficients biem() took (the record stores none), for an observable named `what`
    ("powers", "force").  ValueError for kind != "outer", any Im k != 0 and a record without density, then for the first None among
    the caller's own operands `require`, (value, message) pairs - all before any device work."""
    plural = what.endswith("s")
    if res.kind != "outer":
        raise ValueError(f"Invalid kind: {res.kind} (the {what} belong{'' if plural else 's'} to an exterior problem, kind='outer')")
    k_h = _host_array(res.k)
    if np.iscomplexobj(k_h) and bool(np.any(k_h.imag != 0)):
        raise ValueError(f"The {what} {'are' if plural else 'is'} defined for a real wavenumber: Im k must be zero for every system.")
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    for value, message in require:
        if value is None:
            raise ValueError(message)
    as_array = lambda a: a if isinstance(a, (torch.Tensor, np.ndarray)) else np.asarray(a)
    centers = as_array(res.centers)
    centers = torch.movedim(centers, 0, -1) if isinstance(centers, torch.Tensor) else np.moveaxis(centers, 0, -1)
    with warnings.catch_warnings():                   # (biem() has given the warnings of these operands already)
        warnings.simplefilter("ignore", UserWarning)
        return _operator(res.c, centers, as_array(res.radii), as_array(res.k), int(res.n_end), alpha, beta, as_array(res.eta), res.kind,
                         alpha_n, beta_n)


def _check_incident(op: _Operator, uin, uin_grad) -> None:
    """The boundary condition needs uin where alpha != 0 and uin_grad where beta != 0.  The zero tests run only when the matching
    callable is missing; Python scalars are decided on the host (a device tensor costs a synchronisation)."""
    def all_zero(v, v_t):
        return (v == 0) if isinstance(v, (int, float, complex)) else bool(torch.all(v_t == 0))
    if uin is None and not all_zero(op.alpha, op.alpha_t):
        raise ValueError("alpha is not zero, but uin is None. uin must be provided to compute the boundary condition.")
    if uin_grad is None and not all_zero(op.beta, op.beta_t):
        raise ValueError("beta is not zero, but uin_grad is None. uin_grad must be provided to compute the boundary condition.")


@dataclass(frozen=True)
class _RhsAxes:
    """Batch axes of the right-hand sides.  The incident field (or a density), of batch shape `full`, may vary along batch axes on
    which the operator (k, eta, geometry, alpha, beta) has size 1 (e.g. many incidence directions for one wavenumber): those axes
    become right-hand sides of ONE factorisation.  The reference broadcasts the matrix over them in btensorsolve (_biem.py:797),
    i.e. factors it again per incidence."""

    full: Tuple[int, ...]
    op_axes: Tuple[int, ...]
    rhs_axes: Tuple[int, ...]
    nrhs: int

    @classmethod
    def of(cls, batch, full) -> "_RhsAxes":     # batch: the operator's batch shape; full: as many axes
        op_axes = tuple(i for i in range(len(batch)) if batch[i] == full[i])
        rhs_axes = tuple(i for i in range(len(batch)) if batch[i] != full[i])
        return cls(tuple(full), op_axes, rhs_axes, int(np.prod([full[i] for i in rhs_axes])) if rhs_axes else 1)

    def lay_out(self, t: torch.Tensor) -> torch.Tensor:
        """(*full, *tail) in the caller's axis order -> contiguous [nb, nrhs, *tail] in (op axes, rhs axes) order."""
        nf = len(self.full)
        tail = tuple(t.shape[nf:])
        nb = math.prod(self.full[i] for i in self.op_axes)
        t = t.permute(list(self.op_axes) + list(self.rhs_axes) + [nf + j for j in range(len(tail))])
        return t.reshape((nb, self.nrhs) + tail).contiguous()

    def restore(self, t: torch.Tensor) -> torch.Tensor:
        """[nb, nrhs, ...] in (op axes, rhs axes) order -> (*full, ...) in the caller's axis order."""
        full = self.full
        tail = tuple(t.shape[2:])
        t = t.reshape(tuple(full[i] for i in self.op_axes) + tuple(full[i] for i in self.rhs_axes) + tail)
        order = self.op_axes + self.rhs_axes
        inv = [order.index(i) for i in range(len(full))]
        return t.permute(inv + [len(full) + j for j in range(len(tail))])


def _boundary_samples(op: _Operator, uin, uin_grad):
    """g[nb, nrhs, B, Q] = (-alpha u_in - beta d_n u_in)(c_b + rho_b y_q): the closure `f` of reference :611-624.  With degree-dependent
    coefficients the two parts stay apart and unweighted, g = (gu, gdn) = (u_in, d_n u_in) at those points (a missing callable: None):
    the degree is known only after the projection (biem_rhs_project_n).  Returns g and the _RhsAxes of its layout.

    fl.centers are in the plan's canonical axes; the user's callables see ORIGINAL axes (x_orig[perm[i]] = x_canon[i])."""
    plan, origin, fl, batch, perm = op.plan, op.origin, op.fl, op.batch, op.perm
    dev, d, Q, B, nb = plan.dev, plan.d, plan.Q, fl.B, fl.nb
    qshape = plan.quad_shape()
    nbt = len(batch)
    inv = _inverse_perm(perm)
    ident = inv == list(range(d))                                      # (no primed nodes: no gather kernels for the axis order)
    ykey = tuple(inv)
    y = plan.y_by_axes.get(ykey)
    if y is None:
        y = plan.y_by_axes[ykey] = (plan.quad_y.T if ident else plan.quad_y.T[inv]).reshape((d,) + qshape).contiguous()   # (d, ...(f)), original axes
    x_rel = y[(...,) + (None,) * (nbt + 1)]                            # (d, ...(f), 1.., 1)
    gbatch = tuple(batch) if fl.geom_batched else (1,) * nbt
    cen = (fl.centers if ident else fl.centers[..., inv]).reshape(gbatch + (B, d))
    rad = fl.radii.reshape(gbatch + (B,))
    # (d, ...(f), ...batch, B)
    cen_m = torch.movedim(cen, -1, 0)[(slice(None),) + (None,) * len(qshape)]
    x = rad[(None,) * (1 + len(qshape))] * x_rel + cen_m
    # (d, ...(f), B, ...batch): the layout the reference hands to uin (:620-621)
    x = torch.movedim(x, -1, 1 + len(qshape))
    x = x.expand((d,) + qshape + (B,) + tuple(batch))
    xu = origin.user_array(x)
    # alpha/beta along (B, ...batch)
    def ab(t):
        t = t.reshape((tuple(batch) if fl.ab_batched else (1,) * nbt) + (B,))
        return torch.movedim(t, -1, 0)[(None,) * len(qshape)]       # (1.., B, ...batch)
    g = None
    lead = qshape + (B,) + tuple(batch)
    if op.per_degree:
        parts = [None if uin is None else _to_dev(uin(xu), dev, torch.complex128),
                 None if uin_grad is None else torch.sum(_to_dev(uin_grad(xu), dev, torch.complex128) * x_rel.to(torch.complex128), dim=0)]
        tgt = tuple(torch.broadcast_shapes(lead, *(tuple(t.shape) for t in parts if t is not None)))
        parts = [None if t is None else t.expand(tgt) for t in parts]
        g = next(t for t in parts if t is not None)
    else:
        if uin is not None:
            u = _to_dev(uin(xu), dev, torch.complex128)
            g = (ab(fl.alpha) * u).neg_()                                  # (a fresh tensor: negated in place)
        if uin_grad is not None:
            gu = _to_dev(uin_grad(xu), dev, torch.complex128)
            t = ab(fl.beta) * torch.sum(gu * x_rel.to(torch.complex128), dim=0)
            g = t.neg_() if g is None else g - t
        if g is None:
            g = torch.zeros(lead, dtype=torch.complex128, device=dev)
        else:
            tgt = tuple(torch.broadcast_shapes(tuple(g.shape), lead))       # (a callable that returned fewer / shorter axes than it was given)
            if tuple(g.shape) != tgt:
                g = g.expand(tgt)
        parts = [g]
    nq = len(qshape)
    full = tuple(g.shape[nq + 1:])
    if len(full) != nbt:
        raise ValueError(f"uin/uin_grad returned an array with batch shape {full}, expected {nbt} batch axes like k")
    axes = _RhsAxes.of(batch, full)
    def laid_out(t):
        t = t.reshape((Q, B) + full)
        return axes.lay_out(t.permute([2 + i for i in range(nbt)] + [1, 0]))      # (*full, B, Q) -> (*op, *rhs, B, Q) as [nb, nrhs, B, Q]
    parts = [None if t is None else laid_out(t) for t in parts]
    return (tuple(parts) if op.per_degree else parts[0]), axes


@dataclass(frozen=True)
class _PlaneWaves:
    """Plane waves as the source of the right-hand sides, in closed form (biem_rhs_plane_wave): unit directions in the plan's canonical
    axes, [nb, nrhs, d] when they differ between the systems of the operator (batched), else [1, nrhs, d].  Stands where the samples of
    _boundary_samples stand; _nrhs, _sample_ptrs, _pick_systems, _source_entry, _source_workspace_bytes and _rhs_project tell them apart."""

    dirs: torch.Tensor
    batched: int
    per_degree: bool         # of the operator: the `_pw` entries take it as an argument, not as a second set of entries
    suffix = "_pw"           # of the whole-path entries
    rhs_entry = "biem_rhs_plane_wave"

    @property
    def vectors(self) -> torch.Tensor:
        return self.dirs

    def workspace_bytes(self, op: "_Operator", n: int) -> int:
        return int(L.load().biem_rhs_plane_wave_workspace_bytes(op.plan.handle, n, int(self.dirs.shape[1]), self.batched))


@dataclass(frozen=True)
class _PointSources:
    """Point sources h_0(k |x - s|) as the source of the right-hand sides, in closed form (biem_rhs_point_source): positions in the plan's
    canonical axes, [nb, nrhs, d] when they differ between the systems of the operator (batched), else [1, nrhs, d].  Stands where
    _PlaneWaves stands, with the same fields."""

    pts: torch.Tensor
    batched: int
    per_degree: bool
    suffix = "_ps"
    rhs_entry = "biem_rhs_point_source"

    @property
    def vectors(self) -> torch.Tensor:
        return self.pts

    def workspace_bytes(self, op: "_Operator", n: int) -> int:
        return int(L.load().biem_rhs_point_source_workspace_bytes(op.plan.handle, n, op.fl.B, int(self.pts.shape[1]), self.batched,
                                                                  op.fl.geom_batched))


@dataclass(frozen=True)
class _MultipoleSources:
    """Outgoing multipoles h_n'(k |x - s|) Y_h'((x - s)^) as the source of the right-hand sides, in closed form (biem_rhs_multipole):
    positions as _PointSources', and the harmonic h' of every source, an index into the plan's harmonic axis, int32 [nb, nrhs] or
    [1, nrhs] with the positions."""

    pts: torch.Tensor
    batched: int
    per_degree: bool
    index: torch.Tensor
    suffix = "_ms"
    rhs_entry = "biem_rhs_multipole"

    @property
    def vectors(self) -> torch.Tensor:
        return self.pts

    def workspace_bytes(self, op: "_Operator", n: int) -> int:
        return int(L.load().biem_rhs_multipole_workspace_bytes(op.plan.handle, n, op.fl.B, int(self.pts.shape[1]), self.batched,
                                                               op.fl.geom_batched))


@dataclass(frozen=True)
class _RegularWaves(_MultipoleSources):
    """Regular waves j_n'(k |x - o|) Y_h'((x - o)^) about the origins `pts` as the source of the right-hand sides, in closed form
    (biem_rhs_regular_wave): the fields and layouts of _MultipoleSources, whose every use they share; the origins are unrestricted."""

    suffix = "_rw"
    rhs_entry = "biem_rhs_regular_wave"

    def workspace_bytes(self, op: "_Operator", n: int) -> int:
        return int(L.load().biem_rhs_regular_wave_workspace_bytes(op.plan.handle, n, op.fl.B, int(self.pts.shape[1]), self.batched,
                                                                  op.fl.geom_batched))


@dataclass(frozen=True)
class _Expansion:
    """A whole expansion sum_h' p_h' z_n' Y_h' about the origins `pts` (z = j: regular, any origin; z = h: outgoing, origins outside the
    balls) as the source of the right-hand sides, in closed form (biem_rhs_expansion).  pts [nb or 1, n_origin, d] in canonical axes,
    n_origin 1 (one origin for all right-hand sides of a system) or nrhs; coef [nb or 1, nrhs, H_list] complex128 along the axis of the
    list plan `lists`, of order max(n_in, n_end); index_map int32 [H]: where the operator's harmonics lie on that axis."""

    pts: torch.Tensor
    batched: int
    per_degree: bool
    coef: torch.Tensor
    coef_batched: int
    lists: Any
    index_map: torch.Tensor
    n_in: int
    regular: bool
    suffix = "_ex"
    rhs_entry = "biem_rhs_expansion"

    @property
    def vectors(self) -> torch.Tensor:
        return self.pts

    def workspace_bytes(self, op: "_Operator", n: int) -> int:
        return int(L.load().biem_rhs_expansion_workspace_bytes(self.lists.handle, n, op.fl.B, int(self.pts.shape[1])))

    def source_args(self, s0: int = 0) -> tuple:
        """What the `_ex` entries take after per_degree, from system s0 on."""
        return (_ptr(self.pts[s0:] if self.batched else self.pts), self.batched, int(self.pts.shape[1]),
                _ptr(self.coef[s0:] if self.coef_batched else self.coef), self.coef_batched, self.lists.handle, _ptr(self.index_map),
                self.n_in, int(self.regular))


_CLOSED_FORM = (_PlaneWaves, _PointSources, _MultipoleSources, _Expansion)          # (_RegularWaves: a _MultipoleSources)


def _check_closed_form(g, rc: int, what: str) -> None:
    """L.check; for point and multipole sources BIEM_ERR_UNSUPPORTED (the order limits of their tables) as NotImplementedError."""
    if isinstance(g, (_PointSources, _MultipoleSources, _Expansion)) and rc == L.BIEM_ERR_UNSUPPORTED:
        msg = L.load().biem_last_error()
        raise NotImplementedError(msg.decode() if msg else f"{what}: not built for this order")
    L.check(rc, what)


def _check_plane_wave_direction(c, k, direction, uin, uin_grad) -> np.ndarray:
    """The checks of biem(plane_wave_direction=) that need no device; returns the directions on the host as float64, not yet normalised."""
    if uin is not None or uin_grad is not None:
        raise ValueError("plane_wave_direction replaces uin / uin_grad: give either the direction or the callables, not both")
    D = _host_array(direction)
    if D.dtype.kind not in "iuf":
        raise ValueError(f"plane_wave_direction must be a real array, got dtype {D.dtype}")
    D = D.astype(np.float64)
    if D.ndim < 1 or D.shape[0] != c.c_ndim:
        raise ValueError(f"The first dimension of plane_wave_direction must be c.c_ndim={c.c_ndim}, but got shape {tuple(D.shape)}")
    if D.ndim != len(_shape(k)) + 1:
        raise ValueError(f"plane_wave_direction.ndim={D.ndim} is not k.ndim + 1={len(_shape(k)) + 1}")
    if not bool(np.all(np.isfinite(D))):
        raise ValueError("plane_wave_direction has a non-finite entry")
    if D.size and not bool(np.all(np.any(D != 0, axis=0))):
        raise ValueError("plane_wave_direction has a zero vector: a plane wave needs a direction")
    return D


def _plane_wave_source(op: _Operator, D: np.ndarray):
    """The source of the checked directions D (c_ndim, ...) and the _RhsAxes of its layout: the trailing axes of D broadcast against
    the batch as the direction of plane_wave() does, and those on which the operator has size 1 become right-hand sides."""
    batch = op.batch
    try:
        full = tuple(np.broadcast_shapes(batch, D.shape[1:]))
    except ValueError as e:
        raise ValueError("Shapes of the batch and plane_wave_direction[1:] are not broadcastable\n"
                         f"batch shape={batch}\ntuple(plane_wave_direction.shape)={tuple(D.shape)}") from e
    axes = _RhsAxes.of(batch, full)
    D = D / np.linalg.norm(D, axis=0, keepdims=True)
    D = D[list(op.perm)]                                              # canonical component i = the caller's perm[i], as the centres
    batched = int(any(D.shape[1 + i] != 1 for i in axes.op_axes))
    t = torch.as_tensor(np.moveaxis(np.broadcast_to(D, (D.shape[0],) + full), 0, -1).copy(), device=op.dev)
    dirs = axes.lay_out(t)                                            # [nb, nrhs, d]
    return _PlaneWaves(dirs if batched else dirs[:1].contiguous(), batched, op.per_degree), axes


def _check_point_source_position(c, k, position, uin, uin_grad, plane_wave_direction) -> np.ndarray:
    """The checks of biem(point_source_position=) that need no device; returns the positions on the host as float64."""
    if uin is not None or uin_grad is not None or plane_wave_direction is not None:
        raise ValueError("point_source_position replaces uin / uin_grad / plane_wave_direction: give one source of the incident field, not several")
    return _check_source_position("point_source_position", c, k, position)


def _check_source_position(name: str, c, k, position) -> np.ndarray:
    """The checks of the positions of point or multipole sources (the argument `name`) that need no device; returns them as float64."""
    S = _host_array(position)
    if S.dtype.kind not in "iuf":
        raise ValueError(f"{name} must be a real array, got dtype {S.dtype}")
    S = S.astype(np.float64)
    if S.ndim < 1 or S.shape[0] != c.c_ndim:
        raise ValueError(f"The first dimension of {name} must be c.c_ndim={c.c_ndim}, but got shape {tuple(S.shape)}")
    if S.ndim != len(_shape(k)) + 1:
        raise ValueError(f"{name}.ndim={S.ndim} is not k.ndim + 1={len(_shape(k)) + 1}")
    if not bool(np.all(np.isfinite(S))):
        raise ValueError(f"{name} has a non-finite entry")
    return S


def _check_sources_outside(op: _Operator, pts: torch.Tensor, name: str = "point_source_position") -> None:
    """ValueError unless |s - c_b| > rho_b for every (system, source, ball) of pts [nb or 1, nrhs, d] (canonical axes), naming the first
    that fails.  On the device; the test of the result is one synchronisation."""
    fl = op.fl
    if not pts.numel() or not fl.B:
        return
    dist = torch.linalg.vector_norm(pts[:, :, None, :] - fl.centers[:, None, :, :], dim=-1)      # [nb or 1, nrhs, B]
    bad = ~(dist > fl.radii[:, None, :])
    if bool(bad.any()):
        s, r, b = (int(v) for v in torch.nonzero(bad)[0])
        what = "a point source" if name == "point_source_position" else "a multipole source"
        raise ValueError(f"{name}: source {r} (system {s}) lies on or inside ball {b}: |s - c| = {float(dist[s, r, b]):.17g} "
                         f"<= radius {float(fl.radii[s if fl.geom_batched else 0, b]):.17g}; {what} must lie strictly outside every ball")


def _source_positions(op: _Operator, S: np.ndarray, name: str = "point_source_position", outside: bool = True):
    """The checked positions S (c_ndim, ...) of the argument `name` laid out as [nb or 1, nrhs, d] in canonical axes, whether they differ
    between the systems, the _RhsAxes of the layout and the full batch shape, as _plane_wave_source.  Every source must lie strictly
    outside every ball (the expansion about a ball's centre converges only there, for kind "inner" and "outer" alike):
    _check_sources_outside, before any library call - unless `outside` is False (the origins of regular waves lie anywhere: no check, no
    synchronisation)."""
    batch = op.batch
    try:
        full = tuple(np.broadcast_shapes(batch, S.shape[1:]))
    except ValueError as e:
        raise ValueError(f"Shapes of the batch and {name}[1:] are not broadcastable\n"
                         f"batch shape={batch}\ntuple({name}.shape)={tuple(S.shape)}") from e
    axes = _RhsAxes.of(batch, full)
    S = S[list(op.perm)]                                              # canonical component i = the caller's perm[i], as the centres
    batched = int(any(S.shape[1 + i] != 1 for i in axes.op_axes))
    t = torch.as_tensor(np.moveaxis(np.broadcast_to(S, (S.shape[0],) + full), 0, -1).copy(), device=op.dev)
    pts = axes.lay_out(t)                                             # [nb, nrhs, d]
    pts = pts if batched else pts[:1].contiguous()
    if outside:
        _check_sources_outside(op, pts, name)
    return pts, batched, axes, full


def _point_source_source(op: _Operator, S: np.ndarray):
    """The source of the checked positions S and the _RhsAxes of its layout."""
    pts, batched, axes, _ = _source_positions(op, S)
    return _PointSources(pts, batched, op.per_degree), axes


def _check_multipole_source(c, k, n_end, position, index, uin, uin_grad, plane_wave_direction, point_source_position,
                            pname: str = "multipole_source_position", iname: str = "multipole_source_index", others=()):
    """The checks of biem(multipole_source_position=, multipole_source_index=) that need no device; returns the positions (float64) and
    the indices (int32, broadcast to the positions' trailing axes) on the host.  The pair (regular_wave_origin, regular_wave_index)
    under its names `pname` / `iname` alike, `others` the further incidence arguments it excludes."""
    if position is None or index is None:
        raise ValueError(f"{pname} and {iname} must be given together")
    if (uin is not None or uin_grad is not None or plane_wave_direction is not None or point_source_position is not None
            or any(o is not None for o in others)):
        rest = "" if pname == "multipole_source_position" else " / multipole_source_position"
        raise ValueError(f"{pname} replaces uin / uin_grad / plane_wave_direction / point_source_position{rest}: give one source "
                         "of the incident field, not several")
    S = _check_source_position(pname, c, k, position)
    I = np.asarray(index) if isinstance(index, (int, np.integer)) and not isinstance(index, bool) else _host_array(index)
    if I.dtype.kind not in "iu":
        raise ValueError(f"{iname} must be an integer or an integer array, got dtype {I.dtype}")
    H = _harm_n_ndim_le(int(n_end), c.c_ndim)
    if I.size and (int(I.min()) < 0 or int(I.max()) >= H):
        raise ValueError(f"{iname} must lie in [0, H) with H={H} harmonics of degree < n_end={int(n_end)}, "
                         f"got values from {int(I.min())} to {int(I.max())}")
    try:
        I = np.broadcast_to(I, S.shape[1:])
    except ValueError as e:
        raise ValueError(f"{iname} is not broadcastable to {pname}.shape[1:]\n"
                         f"tuple({iname}.shape)={tuple(I.shape)}\ntuple({pname}.shape)={tuple(S.shape)}") from e
    return S, I.astype(np.int32)


def _multipole_source_source(op: _Operator, checked):
    """The source of the checked (positions S (c_ndim, ...), indices I S.shape[1:]) and the _RhsAxes of its layout, as
    _point_source_source; the indices are laid out with the positions."""
    S, I = checked
    pts, batched, axes, full = _source_positions(op, S, "multipole_source_position")
    idx = axes.lay_out(torch.as_tensor(np.broadcast_to(I, full)[..., None].copy(), device=op.dev))[..., 0]      # [nb, nrhs]
    idx = (idx if batched else idx[:1]).to(torch.int32).contiguous()
    return _MultipoleSources(pts, batched, op.per_degree, idx), axes


def _regular_wave_source(op: _Operator, checked):
    """The source of the checked (origins O (c_ndim, ...), indices I O.shape[1:]) of regular waves and the _RhsAxes of its layout, as
    _multipole_source_source without the containment check: the origin may lie anywhere, a ball's centre included."""
    S, I = checked
    pts, batched, axes, full = _source_positions(op, S, "regular_wave_origin", outside=False)
    idx = axes.lay_out(torch.as_tensor(np.broadcast_to(I, full)[..., None].copy(), device=op.dev))[..., 0]      # [nb, nrhs]
    idx = (idx if batched else idx[:1]).to(torch.int32).contiguous()
    return _RegularWaves(pts, batched, op.per_degree, idx), axes


def _check_expansion(c, k, position, coefficients, index, others, pname: str, cname: str, iname: str):
    """The checks of biem(regular_wave_origin=, regular_wave_coefficients=) and of the multipole_source pair under their names that need no
    device; `others`: every further incidence argument, all of which the pair excludes.  Returns the positions on the host as float64,
    the coefficients as given and the order n_in of their last axis."""
    if index is not None:
        raise ValueError(f"{cname} replaces {iname}: give the index of one harmonic or the coefficients of all, not both")
    if any(o is not None for o in others):
        raise ValueError(f"{cname} replaces uin / uin_grad / plane_wave_direction / point_source_position and the other closed forms: give one "
                         "source of the incident field, not several")
    if position is None:
        raise ValueError(f"{pname} and {cname} must be given together")
    S = _check_source_position(pname, c, k, position)
    pshape = _shape(coefficients)
    kind = coefficients.dtype if isinstance(coefficients, torch.Tensor) else np.asarray(coefficients).dtype
    if isinstance(kind, torch.dtype) and not (kind.is_complex or kind.is_floating_point) or not isinstance(kind, torch.dtype) and kind.kind not in "iufc":
        raise ValueError(f"{cname} must be a complex (or real) array, got dtype {kind}")
    if len(pshape) < 1:
        raise ValueError(f"{cname} must have shape {pname}.shape[1:] + (H_in,), got a scalar")
    n_in = _harmonic_order(c, int(pshape[-1]), cname)
    try:
        lead = np.broadcast_shapes(tuple(S.shape[1:]), tuple(pshape[:-1]))
        ok = len(lead) == S.ndim - 1
    except ValueError:
        ok = False
    if not ok:
        raise ValueError(f"{cname}.shape[:-1] is not broadcastable with {pname}.shape[1:]\n"
                         f"tuple({cname}.shape)={tuple(pshape)}\ntuple({pname}.shape)={tuple(S.shape)}")
    return S, coefficients, n_in


def _expansion_source(op: _Operator, checked, regular: bool):
    """The source of the checked (origins S (c_ndim, ...), coefficients P (..., H_in), n_in) and the _RhsAxes of its layout: trailing axes
    of S and of P on which the operator has size 1 are right-hand sides; where S has size 1 on all of them the origin is shared.  The
    coefficients go onto the axis of the list plan by label."""
    S, P, n_in = checked
    pname, cname = ("regular_wave_origin", "regular_wave_coefficients") if regular else ("multipole_source_position", "multipole_source_coefficients")
    batch, dev, d = op.batch, op.dev, S.shape[0]
    Pt = _to_dev(P, dev, torch.complex128)
    Pt = Pt.reshape((1,) * (S.ndim - Pt.ndim) + tuple(Pt.shape))
    try:
        full = tuple(np.broadcast_shapes(batch, S.shape[1:], tuple(Pt.shape[:-1])))
    except ValueError as e:
        raise ValueError(f"Shapes of the batch, {pname}[1:] and {cname}[:-1] are not broadcastable\n"
                         f"batch shape={batch}\ntuple({pname}.shape)={tuple(S.shape)}\ntuple({cname}.shape)={tuple(Pt.shape)}") from e
    axes = _RhsAxes.of(batch, full)
    shared = all(S.shape[1 + i] == 1 for i in axes.rhs_axes)
    S = S[list(op.perm)]                                              # canonical component i = the caller's perm[i], as the centres
    o_full = tuple(1 if (shared and i in axes.rhs_axes) else full[i] for i in range(len(full)))
    batched = int(any(S.shape[1 + i] != 1 for i in axes.op_axes))
    t = torch.as_tensor(np.moveaxis(np.broadcast_to(S, (d,) + o_full), 0, -1).copy(), device=dev)
    pts = _RhsAxes.of(batch, o_full).lay_out(t)                       # [nb, n_origin, d]
    pts = pts if batched else pts[:1].contiguous()
    if not regular:
        _check_sources_outside(op, pts, pname)
    tree = op.plan.tree
    n_list = max(n_in, int(op.n_end))
    lists = _plan(tree, n_list, dev)
    coef_batched = int(any(Pt.shape[i] != 1 for i in axes.op_axes))
    placed = torch.zeros(tuple(Pt.shape[:-1]) + (lists.H,), dtype=torch.complex128, device=dev)
    placed[..., torch.as_tensor(_label_positions(tree, n_in, n_list, dev), device=dev)] = Pt
    coef = axes.lay_out(placed.expand(full + (lists.H,)))             # [nb, nrhs, H_list]
    coef = coef if coef_batched else coef[:1].contiguous()
    index_map = torch.as_tensor(_label_positions(tree, int(op.n_end), n_list, dev).astype(np.int32), device=dev)
    return _Expansion(pts, batched, op.per_degree, coef, coef_batched, lists, index_map, int(n_in), bool(regular)), axes


def _nrhs(g) -> int:
    """Right-hand sides per system of a source: the samples of _boundary_samples (a tensor, or the unmixed pair of the degree-dependent
    case), _PlaneWaves or _PointSources."""
    if isinstance(g, _Expansion):
        return int(g.coef.shape[1])
    if isinstance(g, _CLOSED_FORM):
        return int(g.vectors.shape[1])
    return int((g if isinstance(g, torch.Tensor) else next(t for t in g if t is not None)).shape[1])


def _sample_ptrs(g, s0: int = 0):
    """The source arguments of an entry point from system s0 on: (d_g,) or (d_gu, d_gdn), a missing set as the null pointer; plane
    waves and point sources: (per_degree, d_dirs or d_src, batched); multipoles: d_idx after them."""
    if isinstance(g, _Expansion):
        return (int(g.per_degree),) + g.source_args(s0)
    if isinstance(g, _CLOSED_FORM):
        args = (int(g.per_degree), _ptr(g.vectors[s0:] if g.batched else g.vectors), g.batched)
        return args + (_ptr(g.index[s0:] if g.batched else g.index),) if isinstance(g, _MultipoleSources) else args
    if isinstance(g, torch.Tensor):
        return (_ptr(g[s0:]),)
    return tuple(_ptr(None if t is None else t[s0:]) for t in g)


def _pick_systems(g, idx: torch.Tensor):
    """The source of the systems idx (a device index tensor) alone."""
    if isinstance(g, _Expansion):
        pts, coef = (g.pts[idx].contiguous() if g.batched else g.pts), (g.coef[idx].contiguous() if g.coef_batched else g.coef)
        return _Expansion(pts, g.batched, g.per_degree, coef, g.coef_batched, g.lists, g.index_map, g.n_in, g.regular)
    if isinstance(g, _CLOSED_FORM):
        if not g.batched:
            return g
        more = (g.index[idx].contiguous(),) if isinstance(g, _MultipoleSources) else ()
        return type(g)(g.vectors[idx].contiguous(), 1, g.per_degree, *more)
    if isinstance(g, torch.Tensor):
        return g[idx].contiguous()
    return tuple(None if t is None else t[idx].contiguous() for t in g)


def _entry(base: str, per_degree: bool, label: Optional[str] = None):
    """The library entry `base`, with degree-dependent coefficients its `_n` form, and its label for L.check (`label`: one label for
    both forms)."""
    name = base + "_n" if per_degree else base
    return getattr(L.load(), name), label or name


def _source_entry(base: str, op: _Operator, g, label: Optional[str] = None):
    """The entry `base` for the source g: its `_pw` form for plane waves, `_ps` for point sources, `_ms` for multipoles, else _entry's
    choice."""
    if isinstance(g, _CLOSED_FORM):
        return getattr(L.load(), base + g.suffix), label or base + g.suffix
    return _entry(base, op.per_degree, label)


def _source_workspace_bytes(op: _Operator, g) -> int:
    """What the source adds at the tail of a path's workspace (plane waves: the harmonics of their directions; point sources: those
    of the unit vectors from every ball, and the radial table; multipoles: the table rows of one slice)."""
    return g.workspace_bytes(op, op.fl.nb) if isinstance(g, _CLOSED_FORM) else 0


def _factored_source_args(op: _Operator, g) -> tuple:
    """What biem_solve_factored* takes between the tables and the source arguments: nothing, the degree-dependent pair, or for plane
    waves, point sources and multipoles the wavenumbers, the centres and the coefficients."""
    fl = op.fl
    coef = (_ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched)
    if isinstance(g, _CLOSED_FORM):
        return (_ptr(fl.k), _ptr(fl.centers), fl.geom_batched) + coef
    return coef if op.per_degree else ()


def _ball_tables(op: _Operator, sp: int, fill: bool = True) -> torch.Tensor:
    """The per-ball tables [nb, B, 3, n_end] of biem_ball_tables (fill=False: only allocated, for an entry that writes them)."""
    fl, plan = op.fl, op.plan
    tab = torch.empty((fl.nb, fl.B, 3, op.n_end), dtype=torch.complex128, device=op.dev)
    if fill:
        entry, what = _entry("biem_ball_tables", op.per_degree)
        L.check(entry(plan.handle, fl.nb, fl.B, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.radii), fl.geom_batched,
                      _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, _ptr(tab), sp), what)
    return tab


def _rhs_project(op: _Operator, n: int, g, s0: int, f: torch.Tensor, sys_stride: int, elem_stride: int, rhs_stride: int, sp: int,
                 tab: Optional[torch.Tensor] = None) -> None:
    """The right-hand sides of the n systems from s0 on into f (natural order), by the source g: biem_rhs_project / biem_rhs_project_n
    of samples, biem_rhs_plane_wave of plane waves and biem_rhs_point_source of point sources (from `tab`, the ball tables of those n
    systems)."""
    fl, a0 = op.fl, s0 if op.fl.ab_batched else 0
    if isinstance(g, _CLOSED_FORM):
        wb = g.workspace_bytes(op, n)
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=op.dev)
        rc = getattr(L.load(), g.rhs_entry)(op.plan.handle, n, fl.B, _nrhs(g), _ptr(fl.k[s0:]), _ptr(fl.centers[s0:] if fl.geom_batched else fl.centers),
                                            fl.geom_batched, _ptr(tab), *_sample_ptrs(g, s0)[1:], _ptr(f), sys_stride, elem_stride, rhs_stride,
                                            *((0,) if isinstance(g, _Expansion) else ()), _ptr(work), wb, sp)      # (expansions: stage 0)
        _check_closed_form(g, rc, g.rhs_entry)
        return
    entry, what = _entry("biem_rhs_project", op.per_degree)
    coef = (_ptr(fl.alpha[a0:]), _ptr(fl.beta[a0:]), fl.ab_batched) if op.per_degree else ()
    L.check(entry(op.plan.handle, n, fl.B, _nrhs(g), *_sample_ptrs(g, s0), *coef, _ptr(f), sys_stride, elem_stride, rhs_stride, sp), what)
