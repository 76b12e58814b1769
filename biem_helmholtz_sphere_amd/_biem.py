"""Host-side mirror of the reference's solver API for the biem() hot path, computing on MI355X.

Same names, argument meaning and error behaviour as reference ``src/biem_helmholtz_sphere/_biem.py``
(``biem`` :453-819, ``BIEMResultCalculator`` :196-237, ``biem_u`` :822-977, ``plane_wave`` :329-388,
``point_source`` :391-450, ``max_memory``/``max_n_end`` :23-74).  All arithmetic of the path runs in
hand-written HIP kernels behind the C ABI of ``include/biem_mi355.h`` (``_lib.py``); PyTorch only owns
device memory and streams.  There is no CPU path: without the HIP library or a GPU every call raises.

Arrays may be torch tensors (any device; results come back on the inputs' device) or NumPy arrays /
Python scalars (moved to the GPU, results returned as NumPy).  The incident field stays an opaque
callable (reference :536-547) and is evaluated in the caller's array namespace.

This module holds the result record, biem() and the factorisation, and re-exports the modules of one concern each, imported in this
order without a cycle: ``_arrays``, ``_plans``, ``_incident``, ``_operator``, ``_fields``, ``_observables``.
"""
from __future__ import annotations

import os
import warnings
from typing import Any, Callable, Literal, Optional, Protocol, Tuple, TypedDict

import numpy as np
import torch

from . import _lib as L
from ._arrays import Array, _host_array, _ptr, _stream_ptr
from ._coords import canonical_tree
from ._fields import (USCAT_GRAD_N_END_MAX, _cluster_flat, biem_cluster_coefficients, biem_far_pattern, biem_u, biem_u_grad, biem_u_hess, biem_u_interior, biem_u_interior_grad,
                      biem_u_total, biem_u_total_grad)
from ._incident import (fluid_inclusion_bc, harmonic_labels, max_memory, max_n_end, multipole_expansion, multipole_source, plane_wave,
                        plane_wave_coefficients, point_source, regular_expansion, regular_wave)
from ._observables import BIEMPower, biem_force, biem_power
from ._operator import (_Operator, _RhsAxes, _ball_tables, _boundary_samples, _check_closed_form, _check_expansion, _check_incident, _check_multipole_source, _expansion_source,
                        _check_plane_wave_direction, _multipole_source_source, _regular_wave_source, _RegularWaves,
                        _check_point_source_position, _entry, _factored_source_args, _nrhs, _operator, _pick_systems, _plane_wave_source,
                        _point_source_source, _rhs_project, _sample_ptrs, _source_entry, _source_workspace_bytes, _validate_biem_inputs, _warn_biem_inputs)
from ._plans import _chain_plan_dim, _plan

try:  # numpy >= 1.25
    from numpy.exceptions import ComplexWarning
except ImportError:  # pragma: no cover
    from numpy import ComplexWarning  # type: ignore

# the reference promotes silent complex->real casts to errors module-wide (_biem.py:18)
warnings.filterwarnings("error", category=ComplexWarning)

# Beyond the public names, bench.py, the tests and the tools reach through this module for _plan, _ptr, _stream_ptr, _chain_plan_dim,
# _validate_biem_inputs, _warn_biem_inputs, USCAT_GRAD_N_END_MAX, L (imported above) and _last_solve_stats.
__all__ = [
    "BIEMFactorization", "BIEMKwargs", "BIEMPower", "BIEMResultCalculator", "BIEMResultCalculatorProtocol", "UinCallable", "biem",
    "biem_factorize", "biem_far_pattern", "biem_force", "biem_power", "biem_u", "biem_u_grad", "biem_u_hess", "biem_u_interior",
    "biem_u_interior_grad", "biem_u_total", "biem_u_total_grad", "fluid_inclusion_bc", "harmonic_labels", "max_memory", "max_n_end",
    "multipole_source", "plane_wave", "point_source", "regular_wave", "biem_cluster_coefficients", "regular_expansion",
    "multipole_expansion", "plane_wave_coefficients",
]

_last_solve_stats: dict = {}   # how the last biem() call solved its systems (tests / bench)
_ws_memo: dict = {}            # device -> (shape key of the last solve, its workspace bytes): see biem()


class BIEMKwargs(TypedDict, total=False):
    """The kwargs for the BIEM (reference :77-101)."""

    centers: Array
    radii: Array
    k: Array
    n_end: int
    eta: Array
    kind: Literal["inner", "outer"]
    force_matrix: bool


class UinCallable(Protocol):
    def __call__(self, x: Array, /, *, expand_x: bool = True) -> Array: ...


class BIEMResultCalculatorProtocol(Protocol):
    c: Any
    uin: Optional[UinCallable]
    centers: Array
    radii: Array
    k: Array
    n_end: int
    eta: Array
    kind: str
    density: Optional[Array]
    matrix: Optional[Array]

    def uscat(self, x: Array, /, far_field: bool = False, per_ball: bool = False, expand_x: bool = True) -> Array: ...

    def uscat_grad(self, x: Array, /, per_ball: bool = False, expand_x: bool = True) -> Array: ...

    def uscat_hess(self, x: Array, /, per_ball: bool = False, expand_x: bool = True) -> Array: ...


# --------------------------------------------------------------------------------------
# result object (reference :196-237)
# --------------------------------------------------------------------------------------
class BIEMResultCalculator:
    """Callable that computes the BIEMResult at the given cartesian coordinates.

    Field-for-field the reference's frozen kw-only record (:196-237).  ``centers`` is stored as ``[d, ..., B]``
    exactly like the reference does (:588,:810).  ``matrix`` (reference scaling, shape
    ``(..., B, harm, B, harm)``, up to 655 MB per system) is assembled on the GPU on first access instead of being
    retained by default.
    """

    __slots__ = ("c", "uin", "centers", "radii", "k", "n_end", "eta", "kind", "density", "_matrix")

    def __init__(self, *, c, centers, radii, k, n_end, eta, kind, uin=None, density=None, matrix=None):
        for name, val in (("c", c), ("uin", uin), ("centers", centers), ("radii", radii), ("k", k), ("n_end", n_end),
                          ("eta", eta), ("kind", kind), ("density", density), ("_matrix", matrix)):
            object.__setattr__(self, name, val)

    def __setattr__(self, name, value):   # frozen, like attrs.frozen
        raise AttributeError(f"BIEMResultCalculator is frozen: cannot assign to field {name!r}")

    def __delattr__(self, name):
        raise AttributeError(f"BIEMResultCalculator is frozen: cannot delete field {name!r}")

    def __repr__(self) -> str:
        return (f"BIEMResultCalculator(c={self.c!r}, n_end={self.n_end}, kind={self.kind!r}, "
                f"density={'None' if self.density is None else tuple(self.density.shape)})")

    @property
    def matrix(self) -> Optional[Array]:
        """The flattened matrix of the BIEM of shape (..., B, harm, B', harm'); None when the shortcut path ran."""
        m = self._matrix
        if callable(m):
            m = m()
            object.__setattr__(self, "_matrix", m)
        return m

    def uscat(self, x: Array, /, far_field: bool = False, per_ball: bool = False, expand_x: bool = True) -> Array:
        return biem_u(self, x, far_field=far_field, per_ball=per_ball, expand_x=expand_x)

    def uscat_grad(self, x: Array, /, per_ball: bool = False, expand_x: bool = True) -> Array:
        """Cartesian gradient of the scattered field, component axis first (see :func:`biem_u_grad`)."""
        return biem_u_grad(self, x, per_ball=per_ball, expand_x=expand_x)

    def uscat_hess(self, x: Array, /, per_ball: bool = False, expand_x: bool = True) -> Array:
        """Cartesian Hessian of the scattered field, both component axes first (see :func:`biem_u_hess`)."""
        return biem_u_hess(self, x, per_ball=per_ball, expand_x=expand_x)

    def uinterior(self, x: Array, /, *, k_interior: Array, density_ratio: Array, expand_x: bool = True) -> Array:
        """Total field inside penetrable fluid balls, NaN outside them (see :func:`biem_u_interior`)."""
        return biem_u_interior(self, x, k_interior=k_interior, density_ratio=density_ratio, expand_x=expand_x)

    def utotal(self, x: Array, /, *, k_interior: Array, density_ratio: Array, expand_x: bool = True) -> Array:
        """Total field inside and outside penetrable fluid balls (see :func:`biem_u_total`)."""
        return biem_u_total(self, x, k_interior=k_interior, density_ratio=density_ratio, expand_x=expand_x)

    def uinterior_grad(self, x: Array, /, *, k_interior: Array, density_ratio: Array, expand_x: bool = True) -> Array:
        """Gradient of the field inside penetrable fluid balls, component axis first (see :func:`biem_u_interior_grad`)."""
        return biem_u_interior_grad(self, x, k_interior=k_interior, density_ratio=density_ratio, expand_x=expand_x)

    def utotal_grad(self, x: Array, /, *, k_interior: Array, density_ratio: Array, uin_grad: Callable[[Array], Array],
                    expand_x: bool = True) -> Array:
        """Gradient of the total field inside and outside penetrable fluid balls (see :func:`biem_u_total_grad`)."""
        return biem_u_total_grad(self, x, k_interior=k_interior, density_ratio=density_ratio, uin_grad=uin_grad, expand_x=expand_x)

    def power(self, *, uin_grad: Callable[[Array], Array], uin: Callable[[Array], Array] | None = None, alpha: Array | complex = 1.0,
              beta: Array | complex = 0.0, alpha_n: Array | None = None, beta_n: Array | None = None) -> "BIEMPower":
        """Extinction, absorbed and scattered power of the solved problem (see :func:`biem_power`)."""
        return biem_power(self, uin_grad=uin_grad, uin=uin, alpha=alpha, beta=beta, alpha_n=alpha_n, beta_n=beta_n)

    def force(self, *, alpha: Array | complex = 1.0, beta: Array | complex = 0.0, alpha_n: Array | None = None,
              beta_n: Array | None = None) -> Array:
        """Time-averaged radiation force on each ball (see :func:`biem_force`)."""
        return biem_force(self, alpha=alpha, beta=beta, alpha_n=alpha_n, beta_n=beta_n)

    def far_pattern(self, directions: Array, /, per_ball: bool = False) -> Array:
        """The far-field pattern of the whole cluster about the origin (see :func:`biem_far_pattern`)."""
        return biem_far_pattern(self, directions, per_ball=per_ball)

    def cluster_coefficients(self, *, origin: Array | None = None, n_out: int | None = None) -> Array:
        """The scattered field of the whole cluster as one outgoing expansion about ``origin`` (see :func:`biem_cluster_coefficients`)."""
        return biem_cluster_coefficients(self, origin=origin, n_out=n_out)


def _reference_matrix(op: _Operator) -> Array:
    """The matrix of every system in the reference's scaling (``BIEMResultCalculator.matrix``), assembled on demand."""
    plan, fl, dev, lib = op.plan, op.fl, op.dev, L.load()
    nb, B, H = fl.nb, fl.B, plan.H
    with torch.cuda.device(dev):
        N = B * H
        tab = _ball_tables(op, _stream_ptr(dev))
        wb = int(lib.biem_fill_workspace_bytes(plan.handle, nb, B))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
        A = torch.empty((nb, N, N), dtype=torch.complex128, device=dev)
        L.check(lib.biem_fill(plan.handle, nb, B, _ptr(fl.k), _ptr(fl.centers), fl.geom_batched, _ptr(tab), L.FILL_REFERENCE,
                              _ptr(A), N, N * N, N, _ptr(work), wb, _stream_ptr(dev)), "biem_fill")
        return op.origin.give(A.reshape(op.batch + (B, H, B, H)))


def _result(op: _Operator, uin, density_t: Optional[torch.Tensor], axes: Optional[_RhsAxes], with_matrix: bool) -> BIEMResultCalculator:
    """What biem() returns: the operands and the density (axes: the layout _boundary_samples returned) in the caller's namespace."""
    origin = op.origin
    density = None if density_t is None else origin.give(axes.restore(density_t).contiguous())
    if uin is None:
        uin_wrapped = None
    else:
        ndim_first = op.k_t.ndim

        def uin_wrapped(x: Array, /, *, expand_x: bool = True) -> Array:   # reference :803-806
            if expand_x:
                x = x[(...,) + (None,) * ndim_first]
            return uin(x)

    real_out = lambda t: origin.give(t.to(origin.real_dtype), complex_out=False)
    return BIEMResultCalculator(
        c=op.c, n_end=op.n_end, kind=op.kind, uin=uin_wrapped, density=density,
        centers=real_out(torch.movedim(op.centers_t, -1, 0)),       # [..., B, v] -> [v, ..., B]  (reference :588)
        radii=real_out(op.radii_t), eta=real_out(op.eta_t), k=(origin.give(op.k_t) if op.k_complex else real_out(op.k_t.real)),
        matrix=(lambda: _reference_matrix(op)) if with_matrix else None)


# --------------------------------------------------------------------------------------
# the solver (reference :453-819)
# --------------------------------------------------------------------------------------
def _closed_form_request(c, k, n_end, uin, uin_grad, plane_wave_direction, point_source_position, multipole_source_position=None,
                         multipole_source_index=None, regular_wave_origin=None, regular_wave_index=None, regular_wave_coefficients=None,
                         multipole_source_coefficients=None):
    """The checks of plane_wave_direction / point_source_position / the multipole_source pair / the regular_wave pair that need no
    device.  None without any, else (argument name, the checked array on the host - multipoles and regular waves: the pair (positions,
    indices), with coefficients the triple (positions, coefficients, n_in) -, the argument as the caller passed it)."""
    if regular_wave_coefficients is not None:
        checked = _check_expansion(c, k, regular_wave_origin, regular_wave_coefficients, regular_wave_index,
                                   (uin, uin_grad, plane_wave_direction, point_source_position, multipole_source_position,
                                    multipole_source_index, multipole_source_coefficients),
                                   "regular_wave_origin", "regular_wave_coefficients", "regular_wave_index")
        return "regular_wave_coefficients", checked, regular_wave_origin
    if multipole_source_coefficients is not None:
        checked = _check_expansion(c, k, multipole_source_position, multipole_source_coefficients, multipole_source_index,
                                   (uin, uin_grad, plane_wave_direction, point_source_position, regular_wave_origin, regular_wave_index),
                                   "multipole_source_position", "multipole_source_coefficients", "multipole_source_index")
        return "multipole_source_coefficients", checked, multipole_source_position
    if regular_wave_origin is not None or regular_wave_index is not None:
        checked = _check_multipole_source(c, k, n_end, regular_wave_origin, regular_wave_index, uin, uin_grad, plane_wave_direction,
                                          point_source_position, "regular_wave_origin", "regular_wave_index",
                                          (multipole_source_position, multipole_source_index))
        return "regular_wave_origin", checked, regular_wave_origin
    if multipole_source_position is not None or multipole_source_index is not None:
        checked = _check_multipole_source(c, k, n_end, multipole_source_position, multipole_source_index, uin, uin_grad, plane_wave_direction,
                                          point_source_position)
        return "multipole_source_position", checked, multipole_source_position
    if point_source_position is not None:
        checked = _check_point_source_position(c, k, point_source_position, uin, uin_grad, plane_wave_direction)
        return "point_source_position", checked, point_source_position
    if plane_wave_direction is not None:
        return "plane_wave_direction", _check_plane_wave_direction(c, k, plane_wave_direction, uin, uin_grad), plane_wave_direction
    return None


def _incident_source(op: _Operator, uin, uin_grad, closed=None):
    """The source of the right-hand sides, the _RhsAxes of its layout and the callable the result keeps as `.uin`: the samples of
    (uin, uin_grad), or - `closed`: what _closed_form_request returned - plane waves or point sources in closed form, whose `.uin` is
    plane_wave's / point_source's (n = 0) / multipole_source's for the caller's k and argument (a floating tensor as it is, anything
    else as float64)."""
    if closed is None:
        _check_incident(op, uin, uin_grad)
        return _boundary_samples(op, uin, uin_grad) + (uin,)
    name, checked, given = closed
    if name in ("regular_wave_coefficients", "multipole_source_coefficients"):
        regular = name == "regular_wave_coefficients"
        arg = given if isinstance(given, torch.Tensor) and given.is_floating_point() else checked[0]
        field = (regular_expansion(op.c, k=op.k_given, origin=arg, coefficients=checked[1]) if regular
                 else multipole_expansion(op.c, k=op.k_given, source=arg, coefficients=checked[1]))
        return _expansion_source(op, checked, regular) + (field[0],)
    if name == "regular_wave_origin":
        arg = given if isinstance(given, torch.Tensor) and given.is_floating_point() else checked[0]
        return _regular_wave_source(op, checked) + (regular_wave(op.c, k=op.k_given, origin=arg, index=checked[1], n_end=op.n_end)[0],)
    if name == "multipole_source_position":
        arg = given if isinstance(given, torch.Tensor) and given.is_floating_point() else checked[0]
        return _multipole_source_source(op, checked) + (multipole_source(op.c, k=op.k_given, source=arg, index=checked[1], n_end=op.n_end)[0],)
    arg = given if isinstance(given, torch.Tensor) and given.is_floating_point() else checked
    if name == "point_source_position":
        return _point_source_source(op, checked) + (point_source(k=op.k_given, source=arg, n=0)[0],)
    return _plane_wave_source(op, checked) + (plane_wave(k=op.k_given, direction=arg)[0],)


def _solver() -> str:
    solver = os.environ.get("BIEM_SOLVER", "ldlt")
    if solver not in ("ldlt", "lu"):
        raise ValueError(f"BIEM_SOLVER must be 'ldlt' or 'lu', got {solver!r}")
    return solver


def _available_bytes(dev: torch.device) -> int:
    """Device memory this process can still get: free plus what torch's caching allocator holds unused."""
    free, _total = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


def _single_ball_density(op: _Operator, g, tab: torch.Tensor, density_t: torch.Tensor, sp: int) -> None:
    """Single ball: density = f / (blc (alpha h + beta k h'))    (reference :648-691)."""
    lib, plan, nb, B = L.load(), op.plan, op.fl.nb, op.fl.B
    H, nrhs = plan.H, _nrhs(g)
    f = torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device=op.dev)
    _rhs_project(op, nb, g, 0, f, nrhs * B * H, 1, B * H, sp, tab)
    L.check(lib.biem_density(plan.handle, nb, B, nrhs, _ptr(f), nrhs * B * H, 1, B * H, _ptr(tab), _ptr(density_t), sp), "biem_density")


def _lu_systems(info: torch.Tensor, solver: str) -> Tuple[torch.Tensor, list]:
    """Host indices of the systems the pivoted LU takes, and their codes: with BIEM_SOLVER=lu all of them (no codes, no copy), else
    those whose diagonal pivots the symmetric path rejected, info < 0."""
    if solver == "lu":
        return torch.arange(info.numel()), []
    # (the codes come to the host in ONE copy and the rejected systems are picked there: torch.nonzero on the device is five
    # launches and a synchronisation of its own, which one system per call pays in full)
    info_h = info.cpu()
    idx = torch.nonzero(info_h < 0).flatten()
    return idx, (info_h[idx].tolist() if idx.numel() > 0 else [])


def _workspace(dev: torch.device, key: tuple, wbytes: Optional[int] = None) -> Optional[torch.Tensor]:
    """The solve workspace.  Without `wbytes`: the block a repeated call of the same shape (`key`, the memo of the last solve) takes in
    advance, None if the last solve was another or the memory is not there.  With `wbytes`: a block of that size, remembered for the
    next call."""
    memo = _ws_memo.get(dev)
    if wbytes is None and (memo is None or memo[0] != key):
        return None
    with torch.cuda.device(dev):
        try:
            work = torch.empty(memo[1] if wbytes is None else wbytes, dtype=torch.uint8, device=dev)
        except torch.OutOfMemoryError:
            if wbytes is None:
                return None
            torch.cuda.empty_cache()       # cached blocks of other sizes (an earlier, different job): released, one more attempt
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    _ws_memo[dev] = (key, int(work.numel()))
    return work


def _choose_chunk(op: _Operator, nrhs: int, chunk: int, work_pre: Optional[torch.Tensor]) -> int:
    """How many system matrices are resident at once: the caller's `chunk` if positive, else chosen here."""
    if chunk > 0:
        return chunk
    nb, dev = op.fl.nb, op.dev
    # resident matrices per pass: as many as fit 85 % of the memory this process can still get (free + cached by
    # torch's allocator).  The per-system kernels of the LU (panel strips, diagonal-block inverses, back
    # substitution) are latency-bound on ONE CU per system, so they cost the same for 32 or 256 systems.
    per = max(1, int(L.load().biem_solve_workspace_bytes(op.plan.handle, 1, op.fl.B, nrhs, 1)))
    cap = os.environ.get("BIEM_MAX_RESIDENT_BYTES")      # a drop-in inside a larger torch program: bound the workspace
    if nb * per <= (1 << 30) and not cap:
        return nb                      # small jobs: everything resident, no memory query (it costs more than the solve)
    avail = _available_bytes(dev)
    if work_pre is not None:
        avail += int(work_pre.numel())     # (the block taken in advance is this call's own)
    budget = int(0.85 * avail)
    if cap:
        budget = min(budget, max(int(float(cap)), per))
    return max(1, min(nb, 32768, budget // per))      # 32768: grid dimension of the per-system kernels


def _resolve_with_lu(op: _Operator, e_lu, redo_h: torch.Tensor, g, density_t: torch.Tensor, chunk: int, work: torch.Tensor, sp: int) -> None:
    """The systems `redo_h` (host indices) again with the pivoted LU entry `e_lu`, their densities into density_t."""
    plan, fl, dev = op.plan, op.fl, op.dev
    nrhs, B, H = int(density_t.shape[1]), fl.B, plan.H
    redo = redo_h.to(dev)
    nr = int(redo.numel())
    pick = lambda t, batched: t[redo].contiguous() if batched else t
    k_r, eta_r = fl.k[redo].contiguous(), fl.eta[redo].contiguous()
    g_r = _pick_systems(g, redo)
    cen_r, rad_r = pick(fl.centers, fl.geom_batched), pick(fl.radii, fl.geom_batched)
    al_r, be_r = pick(fl.alpha, fl.ab_batched), pick(fl.beta, fl.ab_batched)
    dens_r = torch.empty((nr, nrhs, B, H), dtype=torch.complex128, device=dev)
    info_r = torch.zeros(nr, dtype=torch.int32, device=dev)
    L.check(e_lu(plan.handle, nr, B, nrhs, _ptr(k_r), _ptr(eta_r), _ptr(cen_r), _ptr(rad_r), fl.geom_batched,
                 _ptr(al_r), _ptr(be_r), fl.ab_batched, *_sample_ptrs(g_r), _ptr(dens_r), _ptr(info_r), min(chunk, nr),
                 _ptr(work), int(work.numel()), sp), "biem_solve")
    density_t[redo] = dens_r


def biem(c: Any, /, *, centers: Array, radii: Array, k: Array, n_end: int, alpha: Array | complex = 1.0, beta: Array | complex = 0.0,
         uin: Callable[[Array], Array] | None = None, uin_grad: Callable[[Array], Array] | None = None, eta: Array | None = None,
         kind: Literal["inner", "outer"] = "outer", force_matrix: bool = False,
         translational_coefficients_method: Literal["gumerov", "plane_wave", "triplet"] | None = None, chunk: int = 0,
         alpha_n: Array | None = None, beta_n: Array | None = None, plane_wave_direction: Array | None = None,
         point_source_position: Array | None = None, multipole_source_position: Array | None = None,
         multipole_source_index: Array | int | None = None, regular_wave_origin: Array | None = None,
         regular_wave_index: Array | int | None = None, regular_wave_coefficients: Array | None = None,
         multipole_source_coefficients: Array | None = None) -> BIEMResultCalculator:
    r"""Boundary Integral Equation Method (BIEM) for the Helmholtz equation on MI355X.

    Same contract as the reference ``biem`` (``_biem.py:453-581``): solves, per leading batch element,

        A_{b,n,p,b',n',p'} = blc_{n'}(rho_{b'}, eta) * { delta (alpha h_n + beta k h_n')(k rho_b)            b = b'
                                                        (S|R)_{n'p',np}(c_b - c_b') (alpha j_n + beta k j_n')(k rho_b)  b != b'
        sum A phi = f,   f_{b,n,p} = sum_q w_q (-alpha u_in - beta d_n u_in)(c_b + rho_b y_q) conj(Y_{n,p}(y_q))

    ``translational_coefficients_method`` is accepted for signature compatibility; this build always uses the
    exact closed form of SURVEY A.5 (the reference's "triplet" implementation is itself inexact).
    ``chunk`` (extension) bounds how many system matrices are resident at once (0 = choose).

    ``alpha_n`` / ``beta_n`` (extension, given together, shape ``(..., B, n_end)``, leading axes broadcasting like those of alpha and
    beta): boundary coefficients that depend on the harmonic degree, ``alpha_{b,n} u + beta_{b,n} d_n u = 0`` on ball b.  They take the
    place of alpha and beta (which then stay at their defaults) in gj, gh and f above, with n the degree of the row.  A radially
    symmetric inclusion the wave enters is such a condition: :func:`fluid_inclusion_bc`.  A ball that does not scatter some degree
    (gj_n = 0, e.g. a transparent sphere) has no symmetric form; its systems are solved by the pivoted LU.

    ``plane_wave_direction`` (extension, shape ``(c_ndim, ...)`` like the direction of :func:`plane_wave`, normalised here; not together
    with uin / uin_grad): the incident field is the plane wave ``e^{i k d.x}`` of the operator's own k, and its right-hand side is formed
    in closed form, ``f = -C_d i^n gj_n conj(Y_h(d)) e^{i k d.c_b}`` - exact, where the projection of samples aliases (a plane wave has
    content in every degree) - without sampling anything.  The result is that of ``biem(..., *plane_wave(k=k, direction=D))`` apart from
    that: trailing axes of D on which the operator has size 1 are right-hand sides of one factorisation, ``.uin`` is plane_wave's callable.

    ``point_source_position`` (extension, shape ``(c_ndim, ...)`` like the source of :func:`point_source`; not together with uin /
    uin_grad / plane_wave_direction): the incident field is the monopole ``h_0(k |x - s|)`` of the operator's own k,
    ``point_source(k=k, source=S, n=0)``, and its right-hand side is formed in closed form,
    ``f = -C_d gj_n h_n(k |s - c_b|) conj(Y_h((s - c_b)^))`` - exact, where the projection of samples aliases badly for a source close
    to a sphere (content of degree n decays only like ``(rho_b / |s - c_b|)^n``), and the transpose of the evaluation of the scattered
    field at s, so that reciprocity holds to rounding at every order.  Every source must lie strictly outside every ball, for kind
    "inner" and "outer" alike (``ValueError`` naming the first source and ball otherwise; tested on the device, one synchronisation per
    call).  The axes of S behave as those of plane_wave_direction, ``.uin`` is point_source's callable.  Orders n >= 1 of
    :func:`point_source` have no such expansion and stay with uin / uin_grad.  ``NotImplementedError`` for n_end > 320 (2-D only).

    ``multipole_source_position`` / ``multipole_source_index`` (extension, given together; positions of shape ``(c_ndim, ...)`` like
    point_source_position, the index an integer or an integer array broadcastable to the positions' trailing axes; not together with uin /
    uin_grad / plane_wave_direction / point_source_position): the incident field is the outgoing multipole
    ``h_n'(k |x - s|) Y_h'((x - s)^)`` of the operator's own k, h' a position on the harmonic axis (:func:`harmonic_labels`: the axis of
    ``density[..., H]``, in the canonical tree's labels), :func:`multipole_source`.  Normalisation: orthonormal Y_h and the project's
    radial functions; an index of degree 0 gives ``Y_0 h_0(k |x - s|)``, point_source_position's problem times the constant
    ``Y_0 = |S^{d-1}|^{-1/2}``.  The right-hand side is exact, ``f = -gj_n (S|R)_{h'->h}(c_b - s)``: a column of the translation operator
    the matrix is filled with, where the projection of samples aliases as for a point source, worse with every degree.  The axes behave
    as those of point_source_position, every source must lie strictly outside every ball (``ValueError``), ``.uin`` is
    multipole_source's callable.  A general multipole (a dipole along an arbitrary axis) is a linear combination: pass its
    coefficients, ``multipole_source_coefficients`` below.  ``NotImplementedError`` for n_end > 320 in 2-D and n_end > 160 elsewhere.

    ``regular_wave_origin`` / ``regular_wave_index`` (extension, given together, with the shapes and rules of the multipole pair; not
    together with any other incidence argument): the incident field is the regular wave ``j_n'(k |x - o|) Y_h'((x - o)^)`` about the
    origin ``o``, :func:`regular_wave` - the basis in which every source-free incident field (a beam given by its beam-shape
    coefficients, a standing wave) is written.  The right-hand side is exact, ``f = -gj_n (R|R)_{h'->h}(c_b - o)``.  The origin is
    unrestricted: outside the balls, inside one, or exactly on a ball's centre (nothing is checked, nothing synchronises).  A field of
    several harmonics: ``regular_wave_coefficients`` below; ``fac.tmatrix()`` solves all of them at once.

    ``regular_wave_origin`` / ``regular_wave_coefficients`` and ``multipole_source_position`` / ``multipole_source_coefficients``
    (extension; the coefficients in place of the index of the same pair, not together with any other incidence argument): the incident
    field is the whole expansion ``sum_h' p_h' j_n'(k |x - o|) Y_h'((x - o)^)`` (``h_n'`` about the source for the multipole pair) -
    :func:`regular_expansion` / :func:`multipole_expansion` -, one right-hand side for a beam, a standing wave or the near field of a
    neighbouring cluster, ``f = -gj_n sum_h' p_h' (R|R)_{h'->h}(c_b - o)``: one solve where the index pair takes one per harmonic, and
    the only way to ``force()`` of such a field, which is quadratic in it.  The coefficients P are complex of shape
    ``O.shape[1:] + (H_in,)`` up to broadcasting, the last axis along ``harmonic_labels(c, n_in)``; ``n_in`` is inferred from ``H_in``
    and is independent of ``n_end`` (a beam about the cluster's origin wants ``n_in`` of the order of ``k R_cluster``).  Trailing axes of
    O and of P on which the operator has size 1 are right-hand sides; an origin without such axes under coefficients with them is shared
    by all right-hand sides, whose translation tables are then formed once.  Sources must lie strictly outside every ball
    (``ValueError``), regular origins anywhere.  ``.uin`` is the expansion's callable.  ``NotImplementedError`` for max(n_in, n_end) above
    320 in 2-D and above 160 elsewhere.

    Solver: the reference passes every system to a general dense solve (``_biem.py:797``).  Here the system is first brought
    to its complex-symmetric form (real harmonics, symmetric scaling) and factored as U^T U (Cholesky-type, no conjugation)
    without interchanges - half the flops; a system in which a multiplier would exceed 100, or whose factor grew by more than
    200, is solved by the pivoted LU instead (``BIEM_SOLVER=lu`` in the environment: pivoted LU for all).  Both give the
    reference's ``density`` to rounding.
    """
    if translational_coefficients_method not in (None, "gumerov", "plane_wave", "triplet"):
        raise ValueError(f"Invalid translational_coefficients_method: {translational_coefficients_method}")
    closed = _closed_form_request(c, k, n_end, uin, uin_grad, plane_wave_direction, point_source_position, multipole_source_position,
                                  multipole_source_index, regular_wave_origin, regular_wave_index, regular_wave_coefficients,
                                  multipole_source_coefficients)
    op = _operator(c, centers, radii, k, n_end, alpha, beta, eta, kind, alpha_n, beta_n)
    lib = L.load()
    plan, fl, dev = op.plan, op.fl, op.dev
    B, nb, H = fl.B, fl.nb, plan.H
    sp = _stream_ptr(dev)

    has_rhs = not (uin is None and uin_grad is None and closed is None)
    g = axes = None
    # A repeated call of the same shape takes its workspace FIRST, before the boundary samples: the block the previous call
    # returned to torch's caching allocator is then still whole.  Taken after them, one of their mid-size temporaries may have
    # been carved out of it - and a second block of that size need not exist (cfg 3's whole batch: 164 of 288 GB).
    ws_key = (plan.tree, plan.chain, int(n_end), int(nb), int(B), int(chunk), os.environ.get("BIEM_MAX_RESIDENT_BYTES"))
    work_pre = _workspace(dev, ws_key) if has_rhs and nb > 0 and (B > 1 or force_matrix) else None
    if has_rhs:
        g, axes, uin = _incident_source(op, uin, uin_grad, closed)
        nrhs = _nrhs(g)

    use_matrix = (not has_rhs) or B > 1 or force_matrix          # reference :643-645
    density_t = None
    with torch.cuda.device(dev):
        if nb == 0:
            # an empty batch axis: nothing to solve, results of the right (empty) shape
            density_t = torch.empty((0, nrhs, B, H), dtype=torch.complex128, device=dev) if has_rhs else None
        elif not use_matrix:
            density_t = torch.empty((nb, nrhs, B, H), dtype=torch.complex128, device=dev)
            _single_ball_density(op, g, _ball_tables(op, sp), density_t, sp)
        elif has_rhs:
            chunk = _choose_chunk(op, nrhs, int(chunk), work_pre)
            wbytes = int(lib.biem_solve_workspace_bytes(plan.handle, nb, B, nrhs, chunk)) + _source_workspace_bytes(op, g)
            if work_pre is not None and work_pre.numel() != wbytes:
                work_pre = None                    # (another size after all: back to the allocator before the right one is taken)
            work = work_pre if work_pre is not None else _workspace(dev, ws_key, wbytes)
            density_t = torch.empty((nb, nrhs, B, H), dtype=torch.complex128, device=dev)
            info = torch.zeros(nb, dtype=torch.int32, device=dev)
            # The equilibrated system is complex symmetric in a real-harmonic basis (include/biem_mi355.h, biem_solve_ldlt):
            # U^T U factorisation without interchanges, half the flops of the LU.  Systems whose diagonal pivots were rejected
            # (info < 0: close to a resonance of a sphere, or strongly coupled spheres) are solved again with the pivoted LU,
            # which is what the reference's linalg.solve does for every system (_biem.py:797).  BIEM_SOLVER=lu: LU only.
            solver = _solver()
            # (degree-dependent coefficients: the *_n entries, alpha_n / beta_n for alpha / beta and the unmixed samples for g; plane
            # waves and point sources in closed form: the *_pw and *_ps entries)
            e_lu, what = _source_entry("biem_solve", op, g, "biem_solve")
            entry = _source_entry("biem_solve_ldlt", op, g)[0] if solver == "ldlt" else e_lu
            _check_closed_form(g, entry(plan.handle, nb, B, nrhs, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                                        _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, *_sample_ptrs(g), _ptr(density_t), _ptr(info), chunk,
                                        _ptr(work), wbytes, sp), what)
            lu_h, codes = _lu_systems(info, solver)
            if solver == "ldlt" and lu_h.numel() > 0:
                _resolve_with_lu(op, e_lu, lu_h, g, density_t, chunk, work, sp)
            _last_solve_stats["ldlt_systems"] = nb if solver == "ldlt" else 0
            _last_solve_stats["lu_systems"] = int(lu_h.numel())
            # why the symmetric path handed systems over (diagnostics): info = -(first row of the rejecting 64-row panel + 1), or
            # -(n_pad + 1) for the growth check
            _last_solve_stats.pop("rejected_info", None)
            if codes:
                _last_solve_stats["rejected_info"] = codes[:64]
            del work
    return _result(op, uin, density_t, axes, use_matrix)


# --------------------------------------------------------------------------------------
# factor once, solve many (an extension: the reference factors again on every call, :797)
# --------------------------------------------------------------------------------------
class BIEMFactorization:
    """The factored operator of one :func:`biem_factorize` call: solve any number of incident fields against it.

    The operator (geometry, k, eta, alpha, beta, kind) is fixed; :meth:`solve` takes ``uin`` / ``uin_grad`` and returns what
    ``biem(..., uin=uin, uin_grad=uin_grad)`` returns for the same arguments.  Systems are kept in U^T U form (``n_symmetric``)
    or, where the symmetric factorisation rejected them (or with ``BIEM_SOLVER=lu``), in pivoted LU form (``n_lu``).  The
    factors stay in device memory (``nbytes``) until the object is dropped or :meth:`close` is called; solving never
    modifies them.
    """

    def __init__(self, op: _Operator, *, tab, factors, ipiv, lu_runs, n_symmetric, n_lu, chunk):
        self._op = op
        self.c, self.n_end, self.kind = op.c, op.n_end, op.kind
        self._plan = op.plan                   # (read by tools/time_factorized_solve.py)
        self._tab, self._factors, self._ipiv, self._lu_runs = tab, factors, ipiv, lu_runs
        self.n_symmetric, self.n_lu, self._chunk = n_symmetric, n_lu, chunk
        self._closed = False

    @property
    def nbytes(self) -> int:
        """Device bytes held: factors, pivots of the LU-form systems and the per-ball tables."""
        return sum(int(t.numel() * t.element_size()) for t in (self._tab, self._factors, self._ipiv) if t is not None)

    def close(self) -> None:
        """Release the device memory now; :meth:`solve` raises afterwards."""
        self._tab = self._factors = self._ipiv = None
        self._closed = True

    def __repr__(self) -> str:
        return (f"BIEMFactorization(c={self.c!r}, n_end={self.n_end}, kind={self.kind!r}, batch={self._op.batch}, "
                f"n_symmetric={self.n_symmetric}, n_lu={self.n_lu}, nbytes={self.nbytes}{', closed' if self._closed else ''})")

    def solve(self, *, uin: Callable[[Array], Array] | None = None, uin_grad: Callable[[Array], Array] | None = None,
              plane_wave_direction: Array | None = None, point_source_position: Array | None = None,
              multipole_source_position: Array | None = None, multipole_source_index: Array | int | None = None,
              regular_wave_origin: Array | None = None, regular_wave_index: Array | int | None = None,
              regular_wave_coefficients: Array | None = None, multipole_source_coefficients: Array | None = None) -> BIEMResultCalculator:
        """Densities of the incident field (uin, uin_grad), or of plane waves along ``plane_wave_direction`` or of point sources at
        ``point_source_position`` (the monopoles ``h_0(k |x - s|)``, strictly outside every ball) in closed form, against the stored
        factors: ``biem()``'s result for the same field.  Many source positions against one factorisation are right-hand sides of one
        call: a trailing axis of the argument on which the operator has size 1.  ``multipole_source_position`` with
        ``multipole_source_index`` (given together): the outgoing multipoles ``h_n'(k |x - s|) Y_h'((x - s)^)`` in closed form, as in
        :func:`biem`.  ``regular_wave_origin`` with ``regular_wave_index``: the regular waves ``j_n'(k |x - o|) Y_h'((x - o)^)`` about
        any origin, as in :func:`biem`.  ``regular_wave_coefficients`` / ``multipole_source_coefficients`` in place of the index of their
        pair: the whole expansion as one right-hand side, as in :func:`biem`."""
        if self._closed:
            raise ValueError("BIEMFactorization is closed")
        op, lib = self._op, L.load()
        closed = _closed_form_request(op.c, op.k_given, op.n_end, uin, uin_grad, plane_wave_direction, point_source_position,
                                      multipole_source_position, multipole_source_index, regular_wave_origin, regular_wave_index,
                                      regular_wave_coefficients, multipole_source_coefficients)
        plan, fl, dev = op.plan, op.fl, op.dev
        B, H, nb = fl.B, plan.H, fl.nb
        has_rhs = not (uin is None and uin_grad is None and closed is None)
        density_t = axes = None
        if has_rhs:
            g, axes, uin = _incident_source(op, uin, uin_grad, closed)
            density_t = self._densities(g)
        return _result(op, uin, density_t, axes, B > 1 or not has_rhs)

    def _densities(self, g) -> torch.Tensor:
        """The densities [nb, nrhs, B, H] of the source g of right-hand sides against the stored factors."""
        op, lib = self._op, L.load()
        plan, fl, dev = op.plan, op.fl, op.dev
        B, H, nb = fl.B, plan.H, fl.nb
        nrhs = _nrhs(g)
        density_t = torch.empty((nb, nrhs, B, H), dtype=torch.complex128, device=dev)
        sp = _stream_ptr(dev)
        with torch.cuda.device(dev):
            if nb > 0 and self._factors is None:
                _single_ball_density(op, g, self._tab, density_t, sp)
            elif nb > 0:
                n_pad = int(self._factors.shape[-1])
                sst = n_pad * n_pad
                if self.n_symmetric > 0:
                    wb = int(lib.biem_solve_factored_workspace_bytes(plan.handle, nb, B, nrhs)) + _source_workspace_bytes(op, g)
                    work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
                    entry, what = _source_entry("biem_solve_factored", op, g)
                    _check_closed_form(g, entry(plan.handle, nb, B, nrhs, _ptr(self._factors), n_pad, sst, _ptr(self._tab), *_factored_source_args(op, g),
                                                *_sample_ptrs(g), _ptr(density_t), _ptr(work), wb, sp), what)
                    del work
                # LU-form systems (runs of consecutive systems): equilibrated right-hand sides in natural order, stored LU, density
                ldx = nrhs
                for s0, s1 in self._lu_runs:
                    n = s1 - s0
                    x = torch.zeros((n, n_pad, ldx), dtype=torch.complex128, device=dev)
                    xs = n_pad * ldx
                    _rhs_project(op, n, g, s0, x, xs, ldx, 1, sp, self._tab[s0:s1])
                    L.check(lib.biem_lu_solve(n, n_pad, nrhs, _ptr(self._factors[s0]), n_pad, sst, _ptr(self._ipiv[s0]), _ptr(x), ldx, xs, sp),
                            "biem_lu_solve")
                    L.check(lib.biem_density(plan.handle, n, B, nrhs, _ptr(x), xs, ldx, 1, _ptr(self._tab[s0]), _ptr(density_t[s0]), sp),
                            "biem_density")
        return density_t

    def tmatrix(self, *, origin: Array | None = None, n_out: int | None = None, rhs_chunk: int | None = None) -> Array:
        r"""The T-matrix of the cluster about ``origin``: ``T`` of shape ``(...(systems), H_out, H)``, complex128, which maps the regular
        coefficients ``p_h'`` of any incident field ``sum_h' p_h' j_n'(k |x - o|) Y_h'((x - o)^)`` to the outgoing coefficients
        ``A = T p`` of the scattered field ``sum_h'' A_h'' h_n''(k |x - o|) Y_h''((x - o)^)`` (valid outside the sphere about ``o`` that
        holds the cluster).  Column h' is :func:`biem_cluster_coefficients` of the solution for the regular wave of index h'
        (``regular_wave_origin`` / ``regular_wave_index``): H right-hand sides against the stored factors, in chunks of ``rhs_chunk``
        (default: as many as fit 85 % of the free device memory beside the factors; the result does not depend on it).  ``origin``
        has shape ``(c_ndim,)`` or ``(c_ndim, ...)`` broadcastable to the axes of the systems (default 0) and may lie anywhere;
        ``n_out >= n_end`` (default ``n_end``) is the order of the outgoing side, along ``harmonic_labels(c, n_out)``; the columns run
        along ``harmonic_labels(c, n_end)``.  ``kind="outer"`` only."""
        if self._closed:
            raise ValueError("BIEMFactorization is closed")
        op = self._op
        if op.kind != "outer":
            raise ValueError(f"Invalid kind: {op.kind} (kind='inner' has no outgoing expansion: tmatrix needs kind='outer')")
        tree, _ = canonical_tree(op.c.branching_types_expression_str)
        plan, fl, dev, batch = op.plan, op.fl, op.dev, tuple(op.batch)
        nb, B, H, d = fl.nb, fl.B, plan.H, op.c.c_ndim
        n_end = int(op.n_end)
        n_out = n_end if n_out is None else int(n_out)
        if n_out < n_end:
            raise ValueError(f"n_out={n_out} must be at least n_end={n_end}")
        if origin is None:
            O = np.zeros((d,) + (1,) * len(batch))
        else:
            O = _host_array(origin).astype(np.float64)
            if O.ndim < 1 or O.shape[0] != d:
                raise ValueError(f"origin must have shape ({d},) or ({d}, ...), got {tuple(O.shape)}")
            if O.ndim == 1:
                O = O.reshape((d,) + (1,) * len(batch))
            try:
                ok = O.ndim == len(batch) + 1 and tuple(np.broadcast_shapes(batch, O.shape[1:])) == batch
            except ValueError:
                ok = False
            if not ok:
                raise ValueError(f"origin[1:] of shape {tuple(O.shape[1:])} does not broadcast to the batch shape {batch}")
        O = O[list(op.perm)]                                                   # canonical axes, as the centres
        obatched = int(any(n != 1 for n in O.shape[1:]))
        flat = np.moveaxis(np.broadcast_to(O, (d,) + batch), 0, -1).reshape(nb, d) if obatched else O.reshape(1, d)
        of = torch.as_tensor(np.ascontiguousarray(flat), device=dev)
        H_out = _plan(tree, n_out, dev).H if n_out != n_end else H
        if rhs_chunk is None:
            lib = L.load()
            with torch.cuda.device(dev):
                per = (int(lib.biem_solve_factored_workspace_bytes(plan.handle, nb, B, 8)) // 8 if B > 1 else 0) + nb * B * (2 * H + H_out) * 16 + 1
                rhs_chunk = max(1, min(H, int(0.85 * _available_bytes(dev)) // per)) if nb > 0 else H
        rhs_chunk = int(rhs_chunk)
        if rhs_chunk < 1:
            raise ValueError(f"rhs_chunk={rhs_chunk} must be at least 1")
        T = torch.empty((nb, H_out, H), dtype=torch.complex128, device=dev)
        rows = of.shape[0]
        for h0 in range(0, H, rhs_chunk):
            n = min(rhs_chunk, H - h0)
            idx = torch.arange(h0, h0 + n, dtype=torch.int32, device=dev)[None].expand(rows, n).contiguous()
            g = _RegularWaves(of[:, None, :].expand(rows, n, d).contiguous(), obatched, op.per_degree, idx)
            A = _cluster_flat(tree, n_end, n_out, fl, of, obatched, self._densities(g), dev)      # [nb, n, H_out]
            T[:, :, h0:h0 + n] = A.transpose(1, 2)
        return op.origin.give(T.reshape(batch + (H_out, H)))


def biem_factorize(c: Any, /, *, centers: Array, radii: Array, k: Array, n_end: int, alpha: Array | complex = 1.0,
                   beta: Array | complex = 0.0, eta: Array | None = None, kind: Literal["inner", "outer"] = "outer", chunk: int = 0,
                   alpha_n: Array | None = None, beta_n: Array | None = None) -> BIEMFactorization:
    r"""Factor the BIEM operator of :func:`biem` once; solve incident fields against it later with ``.solve(uin=, uin_grad=)``.

    Arguments and their checks are those of :func:`biem` without the incident field; alpha and beta (or the degree-dependent pair
    alpha_n, beta_n) belong to the operator.
    The factors of all systems of the batch are kept on the device, ``nb x n_pad^2 x 16`` bytes (n_pad = B H rounded up to
    64); if they do not fit, ``torch.OutOfMemoryError`` states the bytes needed - the batch is never split silently, since
    factors that are not kept cannot be reused.  ``chunk`` bounds how many systems are filled and factored at once (0 =
    choose); it sizes the workspace on top of the factors, not the factors.  A single ball keeps only its tables (the
    shortcut of :func:`biem`).
    """
    op = _operator(c, centers, radii, k, n_end, alpha, beta, eta, kind, alpha_n, beta_n)
    lib = L.load()
    plan, fl, dev = op.plan, op.fl, op.dev
    B, nb, H = fl.B, fl.nb, plan.H
    sp = _stream_ptr(dev)
    solver = _solver()
    factors = ipiv = None
    lu_runs: list = []
    n_sym = n_lu = 0
    chunk = int(chunk)
    with torch.cuda.device(dev):
        tab = _ball_tables(op, sp, fill=nb > 0 and B == 1)       # (biem_factor_ldlt writes them for B > 1)
        if nb > 0 and B > 1:
            n_pad = int(lib.biem_lu_npad(B * H))
            fbytes = nb * n_pad * n_pad * 16
            wb = int(lib.biem_factor_workspace_bytes(plan.handle, nb, B, chunk))
            avail = _available_bytes(dev)
            if fbytes + wb > avail:
                raise torch.OutOfMemoryError(
                    f"biem_factorize: the factors of {nb} systems of {n_pad} unknowns need {fbytes} bytes "
                    f"(+ {wb} bytes of workspace), {avail} bytes are available on {dev}; factor fewer systems per call")
            try:
                factors = torch.empty((nb, n_pad, n_pad), dtype=torch.complex128, device=dev)
            except torch.OutOfMemoryError as e:
                raise torch.OutOfMemoryError(f"biem_factorize: the factors of {nb} systems need {fbytes} bytes: {e}") from e
            info = torch.zeros(nb, dtype=torch.int32, device=dev)
            work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
            factor, what = _entry("biem_factor_ldlt", op.per_degree, "biem_factor_ldlt")
            L.check(factor(plan.handle, nb, B, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                           _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, _ptr(factors), n_pad, n_pad * n_pad, _ptr(tab),
                           _ptr(info), chunk, _ptr(work), wb, sp), what)
            del work
            # systems the symmetric factorisation rejected (or all of them with BIEM_SOLVER=lu): pivoted LU of the equilibrated
            # system in the same slot, as biem() re-solves them
            idx = _lu_systems(info, solver)[0].numpy()
            redo = np.zeros(nb, dtype=bool)
            redo[idx] = True
            n_lu = int(idx.size)
            n_sym = nb - n_lu
            if n_lu > 0:
                ipiv = torch.zeros((nb, n_pad), dtype=torch.int32, device=dev)
                starts = [int(i) for i in idx if i == 0 or not redo[i - 1]]
                ends = [int(i) + 1 for i in idx if i == nb - 1 or not redo[i + 1]]
                per_chunk = chunk if chunk > 0 else max(1, min(nb, (4 << 30) // max(1, int(lib.biem_lu_workspace_bytes(1, n_pad, 0))
                                                                                        + int(lib.biem_fill_workspace_bytes(plan.handle, 1, B)))))
                for r0, r1 in zip(starts, ends):
                    for s0 in range(r0, r1, per_chunk):
                        s1 = min(r1, s0 + per_chunk)
                        lu_runs.append((s0, s1))
                        n = s1 - s0
                        fwb = int(lib.biem_fill_workspace_bytes(plan.handle, n, B))
                        lwb = int(lib.biem_lu_workspace_bytes(n, n_pad, 0))
                        work = torch.empty(max(fwb, lwb, 16), dtype=torch.uint8, device=dev)
                        cen = _ptr(fl.centers[s0]) if fl.geom_batched else _ptr(fl.centers)
                        L.check(lib.biem_fill(plan.handle, n, B, _ptr(fl.k[s0:]), cen, fl.geom_batched, _ptr(tab[s0]), L.FILL_EQUILIBRATED,
                                              _ptr(factors[s0]), n_pad, n_pad * n_pad, n_pad, _ptr(work), fwb, sp), "biem_fill")
                        L.check(lib.biem_lu_factor(n, n_pad, _ptr(factors[s0]), n_pad, n_pad * n_pad, _ptr(ipiv[s0]), _ptr(info[s0:]),
                                                   _ptr(work), lwb, sp), "biem_lu_factor")
                        del work
    return BIEMFactorization(op, tab=tab, factors=factors, ipiv=ipiv, lu_runs=lu_runs, n_symmetric=n_sym, n_lu=n_lu, chunk=chunk)
