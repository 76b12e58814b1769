"""Host-side mirror of the reference's solver API for the biem() hot path, computing on MI355X.

Same names, argument meaning and error behaviour as reference ``src/biem_helmholtz_sphere/_biem.py``
(``biem`` :453-819, ``BIEMResultCalculator`` :196-237, ``biem_u`` :822-977, ``plane_wave`` :329-388,
``point_source`` :391-450, ``max_memory``/``max_n_end`` :23-74).  All arithmetic of the path runs in
hand-written HIP kernels behind the C ABI of ``include/biem_mi355.h`` (``_lib.py``); PyTorch only owns
device memory and streams.  There is no CPU path: without the HIP library or a GPU every call raises.

Arrays may be torch tensors (any device; results come back on the inputs' device) or NumPy arrays /
Python scalars (moved to the GPU, results returned as NumPy).  The incident field stays an opaque
callable (reference :536-547) and is evaluated in the caller's array namespace.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from dataclasses import dataclass, replace
from typing import Any, Callable, Literal, Optional, Protocol, Tuple, TypedDict

import numpy as np
import torch

from . import _lib as L
from ._coords import SphericalCoordinates, canonical_tree, chain_dim, harm_count, n_end_from_harm

try:  # numpy >= 1.25
    from numpy.exceptions import ComplexWarning
except ImportError:  # pragma: no cover
    from numpy import ComplexWarning  # type: ignore

# the reference promotes silent complex->real casts to errors module-wide (_biem.py:18)
warnings.filterwarnings("error", category=ComplexWarning)

Array = Any

__all__ = [
    "BIEMFactorization", "BIEMKwargs", "BIEMPower", "BIEMResultCalculator", "BIEMResultCalculatorProtocol", "UinCallable", "biem",
    "biem_factorize", "biem_far_pattern", "biem_force", "biem_power", "biem_u", "biem_u_interior", "biem_u_interior_grad", "biem_u_total",
    "biem_u_total_grad", "fluid_inclusion_bc",
    "max_memory", "max_n_end", "plane_wave", "point_source",
]


# --------------------------------------------------------------------------------------
# memory guard (reference _biem.py:23-74, including its d<=3 element-count quirk)
# --------------------------------------------------------------------------------------
def _harm_n_ndim_le(n_end: int, c_ndim: int) -> int:
    """Number of harmonics of degree < n_end on S^{c_ndim-1} (``ush.harm_n_ndim_le``)."""
    if n_end <= 0:
        return 0
    if c_ndim == 2:
        return 2 * n_end - 1
    # dim of polynomials of degree <= n_end-1 restricted to harmonics: C(n+d-2, d-1) + C(n+d-3, d-1), n = n_end-1
    n = n_end - 1
    return math.comb(n + c_ndim - 1, c_ndim - 1) + math.comb(n + c_ndim - 2, c_ndim - 1)


_last_solve_stats: dict = {}   # how the last biem() call solved its systems (tests / bench)
_ws_memo: dict = {}            # device -> (shape key of the last solve, its workspace bytes): see biem()


def max_memory(*, c_ndim: int, n_end: int, n_balls: int) -> int:
    """Maximum memory usage in bytes (reference formula, :23-49)."""
    _COMPLEX128_SIZE = 16
    if c_ndim <= 3:
        return n_balls**2 * _harm_n_ndim_le(n_end, c_ndim) ** 2

    def inner(c_ndim: int, n_end: int) -> int:
        return (2 * n_end - 1) * n_end ** (c_ndim - 1)

    return n_balls**2 * inner(c_ndim, n_end) ** 2 * inner(c_ndim, 2 * n_end) * _COMPLEX128_SIZE


def max_n_end(*, c_ndim: int, memory_limit: int, n_balls: int) -> int:
    """Maximum n_end that fits in the given memory limit (:52-74)."""
    for i in range(1000):
        if max_memory(c_ndim=c_ndim, n_end=i, n_balls=n_balls) > memory_limit:
            break
    return i - 1


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


# --------------------------------------------------------------------------------------
# array plumbing
# --------------------------------------------------------------------------------------
@dataclass
class _Origin:
    """Where the caller's arrays live, so results can be handed back the same way."""

    kind: str                      # "numpy" | "torch"
    device: Any                    # torch.device of the inputs (torch) or None
    real_dtype: Any                # torch real dtype of `centers`

    @property
    def complex_dtype(self):
        return torch.complex64 if self.real_dtype == torch.float32 else torch.complex128

    def give(self, t: torch.Tensor, complex_out: bool = True) -> Array:
        if complex_out and t.dtype != self.complex_dtype:
            t = t.to(self.complex_dtype)
        if self.kind == "numpy":
            return t.cpu().numpy()
        return t.to(self.device)

    def user_array(self, t: torch.Tensor) -> Array:
        """A tensor of the compute device handed to a user callable in the caller's namespace."""
        t = t.to(self.real_dtype)
        if self.kind == "numpy":
            return t.cpu().numpy()
        return t.to(self.device)


def _compute_device(pref: Any = None) -> torch.device:
    if not torch.cuda.is_available():
        raise L.BiemLibraryError(
            "no HIP device visible: biem_helmholtz_sphere_amd computes on MI355X only and has no CPU fallback"
        )
    if isinstance(pref, torch.device) and pref.type == "cuda":
        return pref
    return torch.device("cuda", torch.cuda.current_device())


def _origin_of(*arrays: Any) -> Tuple[_Origin, torch.device]:
    tens = [a for a in arrays if isinstance(a, torch.Tensor)]
    if tens:
        dev = tens[0].device
        rd = tens[0].dtype if tens[0].dtype in (torch.float32, torch.float64) else torch.float64
        return _Origin("torch", dev, rd), _compute_device(dev)
    first = arrays[0] if arrays else None
    rd = torch.float32 if isinstance(first, np.ndarray) and first.dtype == np.float32 else torch.float64
    return _Origin("numpy", None, rd), _compute_device()


def _to_dev(a: Any, dev: torch.device, dtype: Any) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dtype)
    if isinstance(a, (int, float, complex)):           # Python scalars: a fill kernel instead of a (synchronous, pageable) host copy
        return torch.full((), a, dtype=dtype, device=dev)
    return torch.as_tensor(np.asarray(a), device=dev).to(dtype)


def _is_complex(a: Any) -> bool:
    if isinstance(a, torch.Tensor):
        return a.is_complex()
    return np.iscomplexobj(np.asarray(a)) if not isinstance(a, (int, float)) else False


def _stream_ptr(dev: torch.device) -> int:
    return int(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else int(t.data_ptr())


# --------------------------------------------------------------------------------------
# plans (tables per (tree, n_end, device)), cached for the life of the process
# --------------------------------------------------------------------------------------
def _chain_plan_dim(tree: str) -> int:
    """d if the tree's plan is built by the generic chain code: the chains d >= 5 always, ba / bba under BIEM_TREE_CHAIN=1 (tests)."""
    d = chain_dim(tree)
    if not d and tree in ("ba", "bba") and os.environ.get("BIEM_TREE_CHAIN") == "1":
        d = 3 if tree == "ba" else 4
    return d


class _Plan:
    def __init__(self, tree: str, n_end: int, dev: torch.device):
        lib = L.load()
        chain = _chain_plan_dim(tree)
        if tree not in L.TREE_IDS and not chain:
            raise NotImplementedError(f"coordinate tree {tree!r} is not built (available: {sorted(L.TREE_IDS)} and the standard chains)")
        self.tree, self.n_end, self.dev, self.chain = tree, n_end, dev, chain
        h = C.c_void_p()
        with torch.cuda.device(dev):
            if chain:
                L.check(lib.biem_plan_create_chain(chain, n_end, C.byref(h)), "biem_plan_create_chain")
            else:
                L.check(lib.biem_plan_create(L.TREE_IDS[tree], n_end, C.byref(h)), "biem_plan_create")
        self.handle = h
        d, H, Q, H2, nt = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        L.check(lib.biem_plan_info(h, C.byref(d), C.byref(H), C.byref(Q), C.byref(H2), C.byref(nt)))
        self.d, self.H, self.Q, self.H2, self.n_terms = d.value, H.value, Q.value, H2.value, nt.value
        y = np.zeros((self.Q, self.d))
        w = np.zeros(self.Q)
        L.check(lib.biem_plan_quadrature(h, y.ctypes.data, w.ctypes.data))
        self.quad_y = torch.as_tensor(y, device=dev)          # [Q, d] unit vectors
        self.y_by_axes: dict = {}                              # the same, [d, ...(quadrature axes)] per axis order of the caller's tree
        width = self.d - 1 if chain else 3
        lab = np.zeros((self.H, width), dtype=np.int32)
        deg = np.zeros(self.H, dtype=np.int32)
        L.check(lib.biem_plan_labels_n(h, width, lab.ctypes.data, deg.ctypes.data))
        self.labels, self.degrees = lab, deg

    def quad_shape(self) -> Tuple[int, ...]:
        """Tensor-product shape of the rule, one axis per spherical node (the reference's ...(f) axes)."""
        n = self.n_end
        if self.chain:
            return (n,) * (self.d - 2) + (2 * n,)
        return {"a": (2 * n,), "ba": (n, 2 * n), "bba": (n, n, 2 * n), "caa": (n, 2 * n, 2 * n)}[self.tree]


_PLANS: dict = {}


def _plan(tree: str, n_end: int, dev: torch.device) -> _Plan:
    key = (tree, int(n_end), dev.index if dev.index is not None else torch.cuda.current_device(), _chain_plan_dim(tree))
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = _Plan(tree, int(n_end), torch.device("cuda", key[2]))
    return p


# --------------------------------------------------------------------------------------
# incident fields (reference :329-450)
# --------------------------------------------------------------------------------------
def _bshape_ok(a: Tuple[int, ...], b: Tuple[int, ...]) -> bool:
    try:
        np.broadcast_shapes(tuple(a), tuple(b))
        return True
    except ValueError:
        return False


def _like(v: Any, x: Any) -> Any:
    """v (array or scalar of the creator's namespace) as an array usable with x."""
    if isinstance(x, torch.Tensor):
        if isinstance(v, torch.Tensor):
            return v.to(x.device)
        return torch.as_tensor(np.asarray(v), device=x.device)
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def plane_wave(*, k: Array, direction: Array) -> Tuple[Callable[[Array], Array], Callable[[Array], Array]]:
    r"""Plane wave :math:`u(x) = e^{i k d\cdot x}`, d = direction/||direction|| (reference :329-388).

    k has shape (...), direction (c_ndim, ...).  Returns (u, grad u); given x of shape (c_ndim, ...(any), ...)
    they return (...(any), ...) and (c_ndim, ...(any), ...).
    """
    k_ = k if isinstance(k, torch.Tensor) else np.asarray(k)
    d_ = direction if isinstance(direction, torch.Tensor) else np.asarray(direction)
    if not isinstance(d_, torch.Tensor) and d_.dtype.kind in "iu":
        d_ = d_.astype(np.float64)
    if not _bshape_ok(tuple(k_.shape), tuple(d_.shape[1:])):
        raise ValueError(
            "Shapes of k and direction[1:] are not broadcastable\n"
            f"tuple(k.shape)={tuple(k_.shape)}\ntuple(direction.shape)={tuple(d_.shape)}"
        )
    if d_.ndim != k_.ndim + 1:
        raise ValueError(f"direction.ndim={d_.ndim} is not k.ndim + 1={k_.ndim + 1}")
    if isinstance(d_, torch.Tensor):
        d_ = d_ / torch.linalg.vector_norm(d_, dim=0, keepdim=True)
    else:
        d_ = d_ / np.linalg.norm(d_, axis=0, keepdims=True)

    def _parts(x):
        dd, kk = _like(d_, x), _like(k_, x)
        dd = dd[(slice(None),) + (None,) * (x.ndim - dd.ndim)]
        if isinstance(x, torch.Tensor):
            dd = dd.to(x.dtype) if not dd.is_complex() else dd
            ip = torch.sum(dd * x, dim=0)
            return dd, kk, ip, torch.exp(1j * kk * ip)
        ip = np.sum(dd * x, axis=0)
        return dd, kk, ip, np.exp(1j * kk * ip)

    def inner(x: Array, /) -> Array:
        return _parts(x)[3]

    def inner_grad(x: Array, /) -> Array:
        dd, kk, _, e = _parts(x)
        return 1j * kk * dd * e[None, ...]

    return inner, inner_grad


def point_source(*, k: Array, source: Array, n: int) -> Tuple[Callable[[Array], Array], Callable[[Array], Array]]:
    r"""Point source :math:`u(x) = h^{(1)}_n(k\|x - source\|)` with the d-dimensional h_n (reference :391-450).

    The radial functions are evaluated by the HIP kernel behind ``biem_radial_complex`` (real or complex k).
    """
    k_ = k if isinstance(k, torch.Tensor) else np.asarray(k)
    s_ = source if isinstance(source, torch.Tensor) else np.asarray(source, dtype=np.float64)
    if not _bshape_ok(tuple(k_.shape), tuple(s_.shape[1:])):
        raise ValueError(f"Shapes of k and source[1:] are not broadcastable\n{tuple(k_.shape)=}\n{tuple(s_.shape)=}")
    if s_.ndim != k_.ndim + 1:
        raise ValueError(f"source.ndim={s_.ndim} is not k.ndim + 1={k_.ndim + 1}")
    n = int(n)

    def _radial(d: int, z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """h_n(z), h_n'(z) for a (real or complex) tensor z on a cuda device."""
        lib = L.load()
        zz = z.to(torch.complex128).contiguous().reshape(-1)
        out = torch.empty((zz.numel(), 2, n + 2), dtype=torch.complex128, device=zz.device)
        with torch.cuda.device(zz.device):
            L.check(lib.biem_radial_complex(d, n + 1, zz.numel(), _ptr(zz), _ptr(out), _stream_ptr(zz.device)), "biem_radial_complex")
        h, h1 = out[:, 1, n], out[:, 1, n + 1]
        hp = n / zz * h - h1
        return h.reshape(z.shape), hp.reshape(z.shape)

    def _prep(x):
        was_np = not isinstance(x, torch.Tensor)
        dev = _compute_device(None if was_np else x.device)
        xt = _to_dev(x, dev, torch.float64)
        st = _to_dev(s_, dev, torch.float64)
        kt = _to_dev(k_, dev, torch.complex128 if _is_complex(k_) else torch.float64)
        rel = xt - st[(slice(None),) + (None,) * (xt.ndim - st.ndim)]
        r = torch.linalg.vector_norm(rel, dim=0)
        return was_np, (None if was_np else x.device), rel, r, kt

    def _back(t, was_np, dev):
        return t.cpu().numpy() if was_np else t.to(dev)

    def inner(x: Array, /) -> Array:
        was_np, dev, rel, r, kt = _prep(x)
        h, _ = _radial(int(rel.shape[0]), (kt * r).expand(r.shape) if kt.ndim else kt * r)
        return _back(h, was_np, dev)

    def inner_grad(x: Array, /) -> Array:
        was_np, dev, rel, r, kt = _prep(x)
        _, hp = _radial(int(rel.shape[0]), kt * r)
        coeff = kt * hp / r
        return _back(coeff[None, ...] * rel, was_np, dev)

    return inner, inner_grad


def fluid_inclusion_bc(*, c_ndim: int, n_end: int, radii: Array, k_interior: Array, density_ratio: Array,
                       k: Array | None = None) -> Tuple[Array, Array]:
    r"""Degree-dependent boundary coefficients ``(alpha_n, beta_n)`` of penetrable fluid spheres, for ``biem(alpha_n=, beta_n=)``.

    Ball b holds a fluid of wavenumber ``k_interior`` (complex: absorbing) and density ``density_ratio`` times the exterior's.  The
    interior field :math:`\sum c_h j_n(k_b r) Y_h` with u and (1/density) d_n u continuous across the sphere leaves, with the interior
    eliminated and nothing divided,

        alpha_{b,n} = -k_b j_n'(k_b rho_b),      beta_{b,n} = delta_b j_n(k_b rho_b)

    (j_n the c_ndim-dimensional spherical Bessel function of ``biem_radial_complex``).  ``k_b = k, delta = 1`` is a transparent sphere
    (gj_n = 0), ``delta -> 0`` the sound-soft and ``delta -> infinity`` the sound-hard one.  A boundary condition may be scaled freely
    per degree: with the exterior wavenumber ``k`` (shape ``(...)``, as :func:`biem` takes it) every pair is returned scaled to
    ``max(|alpha_n|, |k beta_n|) = 1``, so no row underflows at high n; without it the interior wavenumber sets the scale,
    ``max(|alpha_n|, |k_b beta_n|) = 1`` (the same up to the contrast; the solution does not depend on it).

    ``radii``, ``k_interior`` and ``density_ratio`` broadcast to ``(..., B)``; the results have shape ``(..., B, n_end)``, complex128,
    in the namespace (and on the device) of the inputs.  ``k_interior * radii == 0`` is a ``ValueError`` (no interior field).
    """
    n_end = int(n_end)
    if n_end < 1:
        raise ValueError(f"n_end must be positive, got {n_end}")
    tens = [a for a in (radii, k_interior, density_ratio, k) if isinstance(a, torch.Tensor)]
    dev = _compute_device(tens[0].device if tens else None)
    rho, kb, delta = (_to_dev(a, dev, torch.complex128) for a in (radii, k_interior, density_ratio))
    ks = kb if k is None else _to_dev(k, dev, torch.complex128)[..., None]          # the wavenumber of the scale, along (..., B)
    shape = tuple(torch.broadcast_shapes(tuple(rho.shape), tuple(kb.shape), tuple(delta.shape), tuple(ks.shape)))
    z = (kb * rho).expand(shape).contiguous().reshape(-1)
    if bool(torch.any(z == 0)):
        raise ValueError("k_interior * radii must not be zero")
    out = torch.empty((z.numel(), 2, n_end + 1), dtype=torch.complex128, device=dev)
    if z.numel() > 0:
        with torch.cuda.device(dev):
            L.check(L.load().biem_radial_complex(int(c_ndim), n_end, z.numel(), _ptr(z), _ptr(out), _stream_ptr(dev)), "biem_radial_complex")
    j = out[:, 0, :].reshape(shape + (n_end + 1,))
    n = torch.arange(n_end, dtype=torch.float64, device=dev)
    zz = (kb * rho).expand(shape)[..., None]
    jp = n / zz * j[..., :n_end] - j[..., 1:]                        # j_n' = (n / z) j_n - j_{n+1}
    kbx = kb.expand(shape)[..., None]
    alpha_n = -kbx * jp
    beta_n = delta.expand(shape)[..., None] * j[..., :n_end]
    scale = torch.maximum(alpha_n.abs(), (ks.expand(shape)[..., None] * beta_n).abs())
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    alpha_n, beta_n = alpha_n / scale, beta_n / scale
    if tens:
        return alpha_n.to(tens[0].device), beta_n.to(tens[0].device)
    return alpha_n.cpu().numpy(), beta_n.cpu().numpy()


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


# --------------------------------------------------------------------------------------
# input checking (reference :240-326; error and warning texts are part of the API)
# --------------------------------------------------------------------------------------
def _shape(a: Any) -> Tuple[int, ...]:
    return tuple(a.shape) if isinstance(a, (torch.Tensor, np.ndarray)) else tuple(np.shape(a))


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
        raise ValueError(
            f"k.ndim={len(ks)}, eta.ndim={len(es)}, centers.ndim - 2={len(cs) - 2}, radii.ndim -1={len(rs) - 1}are not the same."
        )
    if len(als) != len(ks) + 1 or len(bes) != len(ks) + 1:
        raise ValueError(f"alpha and beta must be scalars or arrays of shape (..., B) with {len(ks) + 1} axes")
    try:
        batch = np.broadcast_shapes(ks, es, cs[:-2], rs[:-1], als[:-1], bes[:-1])
    except ValueError as e:
        raise ValueError(
            "Shapes of k, eta and "
            "centers.shape[:-2], radii.shape[:-1] "
            "are not broadcastable\n"
            f"tuple(k.shape)={ks}\ntuple(eta.shape)={es}\ntuple(centers.shape)={cs}\ntuple(radii.shape)={rs}\n"
            f"tuple(alpha.shape)={als}\ntuple(beta.shape)={bes}"
        ) from e
    try:
        np.broadcast_shapes(cs[:-1], rs, als, bes)
    except ValueError as e:
        raise ValueError(
            "centers.shape[:-1] and radii.shape "
            "are not broadcastable\n"
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
            "Shapes of alpha_n, beta_n and the batch shape + (B, n_end) "
            "are not broadcastable\n"
            f"tuple(alpha_n.shape)={ans}\ntuple(beta_n.shape)={bns}\nbatch shape={tuple(batch)}, B={B}, n_end={n_end}"
        ) from e


def _host_array(a: Any) -> np.ndarray:
    """Any accepted input (torch tensor on any device, NumPy array, list, scalar) as a NumPy array on the host."""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


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
        warnings.warn(
            "The solution may be incorrect"
            "if k is an eigenvalue for laplacian"
            "on the interior region with"
            "Neumann boundary condition.",
            UserWarning,
            stacklevel=4,
        )
    k_re = k_h.real
    bad = (np.iscomplexobj(k_h) and bool(np.any(k_h.imag < 0))) or bool(np.any((k_re if eta_h is None else eta_h * k_re) < 0))
    if bad:
        warnings.warn("The solution may be incorrectif not (Im k >= 0 and eta Re k >= 0).", UserWarning, stacklevel=4)


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
    alpha_t = _to_dev(alpha, dev, torch.complex128)
    if alpha_t.ndim == 0:
        alpha_t = alpha_t[(None,) * (k_t.ndim + 1)]
    beta_t = _to_dev(beta, dev, torch.complex128)
    if beta_t.ndim == 0:
        beta_t = beta_t[(None,) * (k_t.ndim + 1)]
    # trees with primed nodes run as their canonical tree in permuted axes (canonical component i = original perm[i])
    tree, perm = canonical_tree(c.branching_types_expression_str)
    plan = _plan(tree, n_end, dev)
    fl = _flatten(batch, centers_t if list(perm) == list(range(len(perm))) else centers_t[..., list(perm)], radii_t, k_t, eta_t,
                  alpha_t, beta_t, int(n_end) if per_degree else 0)
    return _Operator(c, n_end, kind, origin, dev, tuple(batch), perm, plan, fl, centers_t, radii_t, k_t, eta_t, _is_complex(k),
                     alpha, beta, alpha_t, beta_t, per_degree)


# --------------------------------------------------------------------------------------
# the solver (reference :453-819)
# --------------------------------------------------------------------------------------
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
        af = alpha_t.expand(tuple(batch) + (B,)).reshape(nb, B).contiguous()
        bf = beta_t.expand(tuple(batch) + (B,)).reshape(nb, B).contiguous()
    else:
        af = alpha_t.reshape(-1)[-alpha_t.shape[-1]:].expand(B).reshape(1, B).contiguous()
        bf = beta_t.reshape(-1)[-beta_t.shape[-1]:].expand(B).reshape(1, B).contiguous()
    return _Flat(nb, B, kf, ef, cf, rf, int(geom_b), af, bf, int(ab_b))


def _check_incident(op: _Operator, uin, uin_grad) -> None:
    """The boundary condition needs uin where alpha != 0 and uin_grad where beta != 0.  The zero tests run only when the matching
    callable is missing; Python scalars are decided on the host (a device tensor costs a synchronisation)."""
    def all_zero(v, v_t):
        return (v == 0) if isinstance(v, (int, float, complex)) else bool(torch.all(v_t == 0))
    if uin is None and not all_zero(op.alpha, op.alpha_t):
        raise ValueError("alpha is not zero, but uin is None. uin must be provided to compute the boundary condition.")
    if uin_grad is None and not all_zero(op.beta, op.beta_t):
        raise ValueError("beta is not zero, but uin_grad is None. uin_grad must be provided to compute the boundary condition.")


def _solver() -> str:
    solver = os.environ.get("BIEM_SOLVER", "ldlt")
    if solver not in ("ldlt", "lu"):
        raise ValueError(f"BIEM_SOLVER must be 'ldlt' or 'lu', got {solver!r}")
    return solver


def _available_bytes(dev: torch.device) -> int:
    """Device memory this process can still get: free plus what torch's caching allocator holds unused."""
    free, _total = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


def _ball_tables(op: _Operator, sp: int, fill: bool = True) -> torch.Tensor:
    """The per-ball tables [nb, B, 3, n_end] of biem_ball_tables (fill=False: only allocated, for an entry that writes them)."""
    fl, plan = op.fl, op.plan
    tab = torch.empty((fl.nb, fl.B, 3, op.n_end), dtype=torch.complex128, device=op.dev)
    if fill:
        entry, what = (L.load().biem_ball_tables_n, "biem_ball_tables_n") if op.per_degree else (L.load().biem_ball_tables, "biem_ball_tables")
        L.check(entry(plan.handle, fl.nb, fl.B, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.radii), fl.geom_batched,
                      _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, _ptr(tab), sp), what)
    return tab


def _nrhs(g) -> int:
    """Right-hand sides per system of the samples of _boundary_samples (a tensor, or the unmixed pair of the degree-dependent case)."""
    return int((g if isinstance(g, torch.Tensor) else next(t for t in g if t is not None)).shape[1])


def _sample_ptrs(g, s0: int = 0):
    """The sample arguments of an entry point from system s0 on: (d_g,) or (d_gu, d_gdn), a missing set as the null pointer."""
    if isinstance(g, torch.Tensor):
        return (_ptr(g[s0:]),)
    return tuple(_ptr(None if t is None else t[s0:]) for t in g)


def _rhs_project(op: _Operator, n: int, g, s0: int, f: torch.Tensor, sys_stride: int, elem_stride: int, rhs_stride: int, sp: int) -> None:
    """biem_rhs_project / biem_rhs_project_n of the n systems from s0 on into f (natural order)."""
    lib, plan, fl = L.load(), op.plan, op.fl
    nrhs = _nrhs(g)
    if op.per_degree:
        a0 = s0 if fl.ab_batched else 0
        L.check(lib.biem_rhs_project_n(plan.handle, n, fl.B, nrhs, *_sample_ptrs(g, s0), _ptr(fl.alpha[a0:]), _ptr(fl.beta[a0:]), fl.ab_batched,
                                       _ptr(f), sys_stride, elem_stride, rhs_stride, sp), "biem_rhs_project_n")
    else:
        L.check(lib.biem_rhs_project(plan.handle, n, fl.B, nrhs, *_sample_ptrs(g, s0), _ptr(f), sys_stride, elem_stride, rhs_stride, sp),
                "biem_rhs_project")


def _single_ball_density(op: _Operator, g: torch.Tensor, tab: torch.Tensor, density_t: torch.Tensor, sp: int) -> None:
    """Single ball: density = f / (blc (alpha h + beta k h'))    (reference :648-691)."""
    lib, plan, nb, B = L.load(), op.plan, op.fl.nb, op.fl.B
    H, nrhs = plan.H, _nrhs(g)
    f = torch.empty((nb, nrhs, B * H), dtype=torch.complex128, device=op.dev)
    _rhs_project(op, nb, g, 0, f, nrhs * B * H, 1, B * H, sp)
    L.check(lib.biem_density(plan.handle, nb, B, nrhs, _ptr(f), nrhs * B * H, 1, B * H, _ptr(tab), _ptr(density_t), sp), "biem_density")


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


def _result(op: _Operator, uin, density_t: Optional[torch.Tensor], axes, with_matrix: bool) -> BIEMResultCalculator:
    """What biem() returns: the operands and the density (axes: the layout _boundary_samples returned) in the caller's namespace."""
    origin = op.origin
    density = None if density_t is None else origin.give(_restore_batch(density_t, *axes).contiguous())
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
        c=op.c,
        centers=real_out(torch.movedim(op.centers_t, -1, 0)),       # [..., B, v] -> [v, ..., B]  (reference :588)
        radii=real_out(op.radii_t),
        k=(origin.give(op.k_t) if op.k_complex else real_out(op.k_t.real)),
        n_end=op.n_end,
        eta=real_out(op.eta_t),
        kind=op.kind,
        uin=uin_wrapped,
        density=density,
        matrix=(lambda: _reference_matrix(op)) if with_matrix else None,
    )


def _boundary_samples(op: _Operator, uin, uin_grad):
    """g[nb, nrhs, B, Q] = (-alpha u_in - beta d_n u_in)(c_b + rho_b y_q): the closure `f` of reference :611-624.  With degree-dependent
    coefficients the two parts stay apart and unweighted, g = (gu, gdn) = (u_in, d_n u_in) at those points (a missing callable: None):
    the degree is known only after the projection (biem_rhs_project_n).

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
    cen = (fl.centers if ident else fl.centers[..., inv]).reshape(((nb,) if fl.geom_batched else (1,)) + (B, d))
    rad = fl.radii.reshape(((nb,) if fl.geom_batched else (1,)) + (B,))
    if fl.geom_batched:
        cen = cen.reshape(tuple(batch) + (B, d))
        rad = rad.reshape(tuple(batch) + (B,))
    else:
        cen = cen.reshape((1,) * nbt + (B, d))
        rad = rad.reshape((1,) * nbt + (B,))
    # (d, ...(f), ...batch, B)
    cen_m = torch.movedim(cen, -1, 0)[(slice(None),) + (None,) * len(qshape)]
    x = rad[(None,) * (1 + len(qshape))] * x_rel + cen_m
    # (d, ...(f), B, ...batch): the layout the reference hands to uin (:620-621)
    x = torch.movedim(x, -1, 1 + len(qshape))
    x = x.expand((d,) + qshape + (B,) + tuple(batch))
    xu = origin.user_array(x)
    # alpha/beta along (B, ...batch)
    def ab(t):
        t = t.reshape(((nb,) if fl.ab_batched else (1,)) + (B,))
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
    # The incident field may vary along batch axes on which the operator (k, eta, geometry, alpha, beta) has size 1
    # (e.g. many incidence directions for one wavenumber): those axes become right-hand sides of ONE factorisation.
    # The reference broadcasts the matrix over them in btensorsolve (_biem.py:797), i.e. factors it again per incidence.
    nq = len(qshape)
    full = tuple(g.shape[nq + 1:])
    if len(full) != nbt:
        raise ValueError(f"uin/uin_grad returned an array with batch shape {full}, expected {nbt} batch axes like k")
    op_axes = [i for i in range(nbt) if batch[i] == full[i]]
    rhs_axes = [i for i in range(nbt) if batch[i] != full[i]]
    nrhs = int(np.prod([full[i] for i in rhs_axes])) if rhs_axes else 1
    def laid_out(t):
        t = t.reshape((Q, B) + full)
        t = t.permute([2 + i for i in op_axes] + [2 + i for i in rhs_axes] + [1, 0])      # (*op, *rhs, B, Q)
        return t.reshape(nb, nrhs, B, Q).contiguous()
    parts = [None if t is None else laid_out(t) for t in parts]
    return (tuple(parts) if op.per_degree else parts[0]), full, op_axes, rhs_axes


def _restore_batch(t: torch.Tensor, full, op_axes, rhs_axes) -> torch.Tensor:
    """[nb, nrhs, ...] in (op axes, rhs axes) order -> (*full, ...) in the caller's axis order."""
    tail = tuple(t.shape[2:])
    t = t.reshape(tuple(full[i] for i in op_axes) + tuple(full[i] for i in rhs_axes) + tail)
    order = op_axes + rhs_axes
    inv = [order.index(i) for i in range(len(full))]
    return t.permute(inv + [len(full) + j for j in range(len(tail))])


def biem(
    c: Any,
    /,
    *,
    centers: Array,
    radii: Array,
    k: Array,
    n_end: int,
    alpha: Array | complex = 1.0,
    beta: Array | complex = 0.0,
    uin: Callable[[Array], Array] | None = None,
    uin_grad: Callable[[Array], Array] | None = None,
    eta: Array | None = None,
    kind: Literal["inner", "outer"] = "outer",
    force_matrix: bool = False,
    translational_coefficients_method: Literal["gumerov", "plane_wave", "triplet"] | None = None,
    chunk: int = 0,
    alpha_n: Array | None = None,
    beta_n: Array | None = None,
) -> BIEMResultCalculator:
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

    Solver: the reference passes every system to a general dense solve (``_biem.py:797``).  Here the system is first brought
    to its complex-symmetric form (real harmonics, symmetric scaling) and factored as U^T U (Cholesky-type, no conjugation)
    without interchanges - half the flops; a system in which a multiplier would exceed 100, or whose factor grew by more than
    200, is solved by the pivoted LU instead (``BIEM_SOLVER=lu`` in the environment: pivoted LU for all).  Both give the
    reference's ``density`` to rounding.
    """
    if translational_coefficients_method not in (None, "gumerov", "plane_wave", "triplet"):
        raise ValueError(f"Invalid translational_coefficients_method: {translational_coefficients_method}")
    op = _operator(c, centers, radii, k, n_end, alpha, beta, eta, kind, alpha_n, beta_n)
    lib = L.load()
    plan, fl, dev = op.plan, op.fl, op.dev
    B, nb, H = fl.B, fl.nb, plan.H
    sp = _stream_ptr(dev)

    has_rhs = not (uin is None and uin_grad is None)
    g = axes = None
    # A repeated call of the same shape takes its workspace FIRST, before the boundary samples: the block the previous call
    # returned to torch's caching allocator is then still whole.  Taken after them, one of their mid-size temporaries may have
    # been carved out of it - and a second block of that size need not exist (cfg 3's whole batch: 164 of 288 GB).
    ws_key = (plan.tree, plan.chain, int(n_end), int(nb), int(B), int(chunk), os.environ.get("BIEM_MAX_RESIDENT_BYTES"))
    work_pre = None
    if has_rhs and nb > 0 and (B > 1 or force_matrix):
        memo = _ws_memo.get(dev)
        if memo is not None and memo[0] == ws_key:
            try:
                with torch.cuda.device(dev):
                    work_pre = torch.empty(memo[1], dtype=torch.uint8, device=dev)
            except torch.OutOfMemoryError:
                work_pre = None
    if has_rhs:
        _check_incident(op, uin, uin_grad)
        g, *axes = _boundary_samples(op, uin, uin_grad)
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
            chunk = int(chunk)
            if chunk <= 0:
                # resident matrices per pass: as many as fit 85 % of the memory this process can still get (free + cached by
                # torch's allocator).  The per-system kernels of the LU (panel strips, diagonal-block inverses, back
                # substitution) are latency-bound on ONE CU per system, so they cost the same for 32 or 256 systems.
                per = max(1, int(lib.biem_solve_workspace_bytes(plan.handle, 1, B, nrhs, 1)))
                if nb * per <= (1 << 30) and not os.environ.get("BIEM_MAX_RESIDENT_BYTES"):
                    chunk = nb                     # small jobs: everything resident, no memory query (it costs more than the solve)
                else:
                    avail = _available_bytes(dev)
                    if work_pre is not None:
                        avail += int(work_pre.numel())     # (the block taken in advance above is this call's own)
                    budget = int(0.85 * avail)
                    cap = os.environ.get("BIEM_MAX_RESIDENT_BYTES")      # a drop-in inside a larger torch program: bound the workspace
                    if cap:
                        budget = min(budget, max(int(float(cap)), per))
                    chunk = max(1, min(nb, 32768, budget // per))      # 32768: grid dimension of the per-system kernels
            wbytes = int(lib.biem_solve_workspace_bytes(plan.handle, nb, B, nrhs, chunk))
            if work_pre is not None and work_pre.numel() == wbytes:
                work = work_pre
            else:
                work_pre = None                    # (another size after all: back to the allocator before the right one is taken)
                try:
                    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
                except torch.OutOfMemoryError:
                    torch.cuda.empty_cache()       # cached blocks of other sizes (an earlier, different job): released, one more attempt
                    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            _ws_memo[dev] = (ws_key, wbytes)
            density_t = torch.empty((nb, nrhs, B, H), dtype=torch.complex128, device=dev)
            info = torch.zeros(nb, dtype=torch.int32, device=dev)
            # The equilibrated system is complex symmetric in a real-harmonic basis (include/biem_mi355.h, biem_solve_ldlt):
            # U^T U factorisation without interchanges, half the flops of the LU.  Systems whose diagonal pivots were rejected
            # (info < 0: close to a resonance of a sphere, or strongly coupled spheres) are solved again with the pivoted LU,
            # which is what the reference's linalg.solve does for every system (_biem.py:797).  BIEM_SOLVER=lu: LU only.
            solver = _solver()
            # (degree-dependent coefficients: the *_n entries, alpha_n / beta_n for alpha / beta and the unmixed samples for g)
            e_sym, e_lu = (lib.biem_solve_ldlt_n, lib.biem_solve_n) if op.per_degree else (lib.biem_solve_ldlt, lib.biem_solve)
            entry = e_sym if solver == "ldlt" else e_lu
            L.check(entry(plan.handle, nb, B, nrhs, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                          _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, *_sample_ptrs(g), _ptr(density_t), _ptr(info), chunk,
                          _ptr(work), wbytes, sp), "biem_solve")
            if solver == "ldlt":
                # (the codes come to the host in ONE copy and the rejected systems are picked there: torch.nonzero on the device is five
                # launches and a synchronisation of its own, which one system per call pays in full)
                info_h = info.cpu()
                redo_h = torch.nonzero(info_h < 0).flatten()
                redo = redo_h.to(dev) if redo_h.numel() > 0 else redo_h
                if redo.numel() > 0:
                    nr = int(redo.numel())
                    pick = lambda t, batched: t[redo].contiguous() if batched else t
                    k_r, eta_r = fl.k[redo].contiguous(), fl.eta[redo].contiguous()
                    g_r = g[redo].contiguous() if isinstance(g, torch.Tensor) else tuple(None if t is None else t[redo].contiguous() for t in g)
                    cen_r, rad_r = pick(fl.centers, fl.geom_batched), pick(fl.radii, fl.geom_batched)
                    al_r, be_r = pick(fl.alpha, fl.ab_batched), pick(fl.beta, fl.ab_batched)
                    dens_r = torch.empty((nr, nrhs, B, H), dtype=torch.complex128, device=dev)
                    info_r = torch.zeros(nr, dtype=torch.int32, device=dev)
                    L.check(e_lu(plan.handle, nr, B, nrhs, _ptr(k_r), _ptr(eta_r), _ptr(cen_r), _ptr(rad_r), fl.geom_batched,
                                 _ptr(al_r), _ptr(be_r), fl.ab_batched, *_sample_ptrs(g_r), _ptr(dens_r), _ptr(info_r), min(chunk, nr),
                                 _ptr(work), wbytes, sp), "biem_solve")
                    density_t[redo] = dens_r
            _last_solve_stats["ldlt_systems"] = nb if solver == "ldlt" else 0
            _last_solve_stats["lu_systems"] = (int(redo.numel()) if solver == "ldlt" else nb)
            # why the symmetric path handed systems over (diagnostics): info = -(first row of the rejecting 64-row panel + 1), or
            # -(n_pad + 1) for the growth check
            _last_solve_stats.pop("rejected_info", None)
            if solver == "ldlt" and redo.numel() > 0:
                _last_solve_stats["rejected_info"] = info_h[redo_h].tolist()[:64]
            del work
    return _result(op, uin, density_t, axes, use_matrix)


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


def _inverse_perm(perm) -> list:
    """inv with inv[perm[i]] = i.  The kernels' gradient components lie along the plan's canonical axes y_i = x_{perm[i]}: out[inv] hands
    them back along the caller's."""
    inv = [0] * len(perm)
    for i, q in enumerate(perm):
        inv[q] = i
    return inv


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


def _stacked(x: Array) -> Array:
    """A list / tuple of coordinate arrays as one array, component axis first."""
    if isinstance(x, (list, tuple)):
        return np.stack([np.asarray(v) for v in x], 0) if not isinstance(x[0], torch.Tensor) else torch.stack(list(x), 0)
    return x


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
    origin, dev = _origin_of(res.centers, res.radii, res.k, res.density, x)
    if isinstance(res.density, torch.Tensor) and res.density.dtype == torch.complex64:
        origin.real_dtype = torch.float32
    elif isinstance(res.density, np.ndarray) and res.density.dtype == np.complex64:
        origin.real_dtype = torch.float32
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


def _field(res: Any, x: Array, *, far_field: bool, per_ball: bool, expand_x: bool, grad: bool) -> Array:
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    if res.kind not in ("outer", "inner"):
        raise ValueError(f"Invalid kind: {res.kind}")
    c = res.c
    tree, perm = canonical_tree(c.branching_types_expression_str)
    if grad:
        _check_covered("uscat_grad", c, tree, n_end_from_harm(tree, int(res.density.shape[-1])), "uscat() only")
    lib = L.load()
    f = _field_operands(res, x, tree, perm, expand_x)
    origin, dev, fl, plan, pts, df, flags, xshape, batch = f.origin, f.dev, f.fl, f.plan, f.pts, f.density, f.flags, f.xshape, f.batch
    nb, B, d, P = fl.nb, fl.B, c.c_ndim, int(pts.shape[1])
    if far_field:
        flags |= L.USCAT_FAR_FIELD
    if per_ball:
        flags |= L.USCAT_PER_BALL
    if res.kind == "inner":
        flags |= L.USCAT_KIND_INNER

    out = torch.empty(((d,) if grad else ()) + ((P, nb, B) if per_ball else (P, nb)), dtype=torch.complex128, device=dev)
    fn, what = (lib.biem_uscat_grad, "biem_uscat_grad") if grad else (lib.biem_uscat, "biem_uscat")
    with torch.cuda.device(dev):
        wb = int(lib.biem_uscat_workspace_bytes(plan.handle, nb, B))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
        if P > 0 and nb > 0:
            rc = fn(plan.handle, nb, B, P, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                    _ptr(df), _ptr(pts), flags, _ptr(out), _ptr(work), wb, _stream_ptr(dev))
            if grad:
                _check_built(lib, rc, what)
            else:
                L.check(rc, what)
    if grad and list(perm) != list(range(d)):
        out = out[_inverse_perm(perm)]
    out = out.reshape(((d,) if grad else ()) + xshape + batch + ((B,) if per_ball else ()))
    return origin.give(out)


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

    lib = L.load()
    f = _field_operands(res, x, tree, perm, expand_x, extra_batch=(kis[:-1], dls[:-1]))
    dev, fl, batch = f.dev, f.fl, f.batch
    nb, P = fl.nb, int(f.pts.shape[1])
    kb_t, dl_t = (_to_dev(a, dev, torch.complex128) for a in (k_interior, density_ratio))
    fluid_b = any(s != 1 for s in tuple(kb_t.shape[:-1]) + tuple(dl_t.shape[:-1]))

    def per_ball(t):                                       # [nb, B], or [1, B] shared by all systems
        t = t.expand(tuple(torch.broadcast_shapes(tuple(t.shape), (B,))))
        return (t.expand(batch + (B,)).reshape(nb, B) if fluid_b else t.reshape(1, B)).contiguous()

    kb_f, dl_f = per_ball(kb_t), per_ball(dl_t)
    d = c.c_ndim
    out = torch.empty(((d,) if grad else ()) + (P, nb), dtype=torch.complex128, device=dev)
    fn, entry = (lib.biem_uinterior_grad, "biem_uinterior_grad") if grad else (lib.biem_uinterior, "biem_uinterior")
    with torch.cuda.device(dev):
        wb = int(lib.biem_uinterior_workspace_bytes(f.plan.handle, nb, B))
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
        if P > 0 and nb > 0:
            rc = fn(f.plan.handle, nb, B, P, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                    _ptr(kb_f), _ptr(dl_f), int(fluid_b), _ptr(f.density), _ptr(f.pts), f.flags, _ptr(out), _ptr(work), wb,
                    _stream_ptr(dev))
            _check_built(lib, rc, entry)
    if grad and list(perm) != list(range(d)):
        out = out[_inverse_perm(perm)]
    return f.origin.give(out.reshape(((d,) if grad else ()) + f.xshape + batch))


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


# --------------------------------------------------------------------------------------
# cross sections and the far-field pattern about the origin (an extension)
# --------------------------------------------------------------------------------------
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
    if res.kind != "outer":
        raise ValueError(f"Invalid kind: {res.kind} (the powers belong to an exterior problem, kind='outer')")
    k_h = _host_array(res.k)
    if np.iscomplexobj(k_h) and bool(np.any(k_h.imag != 0)):
        raise ValueError("The powers are defined for a real wavenumber: Im k must be zero for every system.")
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    if uin is None and res.uin is not None:
        stored = res.uin
        uin = lambda x: stored(x, expand_x=False)     # (the record's wrapper; _boundary_samples hands over the batch axes itself)
    if uin is None:
        raise ValueError("uin is None and the BIEMResult does not have uin. uin must be provided to compute the extinction.")
    if uin_grad is None:
        raise ValueError("uin_grad is None. uin_grad must be provided to compute the extinction.")
    as_array = lambda a: a if isinstance(a, (torch.Tensor, np.ndarray)) else np.asarray(a)
    centers = as_array(res.centers)
    centers = torch.movedim(centers, 0, -1) if isinstance(centers, torch.Tensor) else np.moveaxis(centers, 0, -1)
    with warnings.catch_warnings():                   # (biem() has given the warnings of these operands already)
        warnings.simplefilter("ignore", UserWarning)
        op = _operator(res.c, centers, as_array(res.radii), as_array(res.k), int(res.n_end), alpha, beta, as_array(res.eta), res.kind,
                       alpha_n, beta_n)
    plan, fl, dev = op.plan, op.fl, op.dev
    nb, B, H = fl.nb, fl.B, plan.H
    # the unweighted samples of the per-degree path, whatever the coefficients: U and V are projections of u_in and d_n u_in alone
    (gu, gdn), full, op_axes, rhs_axes = _boundary_samples(replace(op, per_degree=True), uin, uin_grad)
    nrhs = int(gu.shape[1])
    dens_t = _to_dev(res.density, dev, torch.complex128)
    if tuple(dens_t.shape) != tuple(full) + (B, H):
        raise ValueError(f"density has shape {tuple(dens_t.shape)}, but uin / uin_grad and the operator give {tuple(full) + (B, H)}")
    nf = len(full)
    dens_t = dens_t.permute(list(op_axes) + list(rhs_axes) + [nf, nf + 1]).reshape(nb, nrhs, B, H).contiguous()
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
            entry, what = (lib.biem_power_n, "biem_power_n") if op.per_degree else (lib.biem_power, "biem_power")
            _check_built(lib, entry(plan.handle, nb, B, nrhs, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.radii), fl.geom_batched, _ptr(fl.alpha),
                                    _ptr(fl.beta), fl.ab_batched, _ptr(tab), _ptr(dens_t), _ptr(pu), _ptr(pv), _ptr(out), sp), what)
    out = _restore_batch(out, full, op_axes, rhs_axes)
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
    if res.kind != "outer":
        raise ValueError(f"Invalid kind: {res.kind} (the force belongs to an exterior problem, kind='outer')")
    k_h = _host_array(res.k)
    if np.iscomplexobj(k_h) and bool(np.any(k_h.imag != 0)):
        raise ValueError("The force is defined for a real wavenumber: Im k must be zero for every system.")
    if res.density is None:
        raise ValueError("The BIEMResult does not have density.")
    as_array = lambda a: a if isinstance(a, (torch.Tensor, np.ndarray)) else np.asarray(a)
    centers = as_array(res.centers)
    centers = torch.movedim(centers, 0, -1) if isinstance(centers, torch.Tensor) else np.moveaxis(centers, 0, -1)
    with warnings.catch_warnings():                   # (biem() has given the warnings of these operands already)
        warnings.simplefilter("ignore", UserWarning)
        op = _operator(res.c, centers, as_array(res.radii), as_array(res.k), int(res.n_end), alpha, beta, as_array(res.eta), res.kind,
                       alpha_n, beta_n)
    plan, fl, dev = op.plan, op.fl, op.dev
    nb, B, H, d = fl.nb, fl.B, plan.H, plan.d
    dens_t = _to_dev(res.density, dev, torch.complex128)
    # batch axes of the density on which the operator has size 1 are right-hand sides (the layout of _boundary_samples)
    full, nbt = tuple(dens_t.shape[:-2]), len(op.batch)
    if len(full) != nbt or tuple(dens_t.shape[-2:]) != (B, H) or any(op.batch[i] not in (1, full[i]) for i in range(nbt)):
        raise ValueError(f"density has shape {tuple(dens_t.shape)}, but the operator gives {tuple(op.batch) + (B, H)}")
    op_axes = [i for i in range(nbt) if op.batch[i] == full[i]]
    rhs_axes = [i for i in range(nbt) if op.batch[i] != full[i]]
    nrhs = int(np.prod([full[i] for i in rhs_axes])) if rhs_axes else 1
    dens_t = dens_t.permute(op_axes + rhs_axes + [nbt, nbt + 1]).reshape(nb, nrhs, B, H).contiguous()
    out = torch.empty((nb, nrhs, B, d), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        if out.numel() > 0:
            tab = _ball_tables(op, sp)
            lib = L.load()
            entry, what = (lib.biem_force_n, "biem_force_n") if op.per_degree else (lib.biem_force, "biem_force")
            _check_built(lib, entry(plan.handle, nb, B, nrhs, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.radii), fl.geom_batched, _ptr(fl.alpha),
                                    _ptr(fl.beta), fl.ab_batched, _ptr(tab), _ptr(dens_t), _ptr(out), sp), what)
    out = torch.movedim(_restore_batch(out, full, op_axes, rhs_axes), -1, 0)     # (d, ...(first), B), the plan's axes
    if list(op.perm) != list(range(d)):
        out = out[_inverse_perm(op.perm)]
    return op.origin.give(out.contiguous(), complex_out=False)


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
    origin, dev = _origin_of(res.centers, res.radii, res.k, res.density, directions)
    if getattr(res.density, "dtype", None) in (torch.complex64, np.complex64):
        origin.real_dtype = torch.float32
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
    at_origin = BIEMResultCalculator(c=res.c, centers=torch.zeros_like(cen_t), radii=_to_dev(res.radii, dev, f64), k=k_t, n_end=res.n_end,
                                     eta=_to_dev(res.eta, dev, f64), kind=res.kind, density=_to_dev(res.density, dev, torch.complex128))
    pb = biem_u(at_origin, torch.where(ok, xh, e0), far_field=True, per_ball=True)         # (..., ...(first), B)
    nd, nfirst = x_t.ndim - 1, cen_t.ndim - 2
    dot = torch.sum(xh[(...,) + (None,) * (nfirst + 1)] * cen_t[(slice(None),) + (None,) * nd], dim=0)
    out = pb * torch.exp(-1j * k_t[..., None] * dot)   # (a direction that was zero: NaN through the phase)
    return origin.give(out if per_ball else out.sum(-1))


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

    def solve(self, *, uin: Callable[[Array], Array] | None = None,
              uin_grad: Callable[[Array], Array] | None = None) -> BIEMResultCalculator:
        """Densities of the incident field (uin, uin_grad) against the stored factors: ``biem()``'s result for the same field."""
        if self._closed:
            raise ValueError("BIEMFactorization is closed")
        op, lib = self._op, L.load()
        plan, fl, dev = op.plan, op.fl, op.dev
        B, H, nb = fl.B, plan.H, fl.nb
        has_rhs = not (uin is None and uin_grad is None)
        density_t = axes = None
        if has_rhs:
            _check_incident(op, uin, uin_grad)
            g, *axes = _boundary_samples(op, uin, uin_grad)
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
                        wb = int(lib.biem_solve_factored_workspace_bytes(plan.handle, nb, B, nrhs))
                        work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
                        if op.per_degree:
                            L.check(lib.biem_solve_factored_n(plan.handle, nb, B, nrhs, _ptr(self._factors), n_pad, sst, _ptr(self._tab),
                                                              _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, *_sample_ptrs(g),
                                                              _ptr(density_t), _ptr(work), wb, sp), "biem_solve_factored_n")
                        else:
                            L.check(lib.biem_solve_factored(plan.handle, nb, B, nrhs, _ptr(self._factors), n_pad, sst, _ptr(self._tab), _ptr(g),
                                                            _ptr(density_t), _ptr(work), wb, sp), "biem_solve_factored")
                        del work
                    # LU-form systems (runs of consecutive systems): equilibrated right-hand sides in natural order, stored LU, density
                    ldx = nrhs
                    for s0, s1 in self._lu_runs:
                        n = s1 - s0
                        x = torch.zeros((n, n_pad, ldx), dtype=torch.complex128, device=dev)
                        xs = n_pad * ldx
                        _rhs_project(op, n, g, s0, x, xs, ldx, 1, sp)
                        L.check(lib.biem_lu_solve(n, n_pad, nrhs, _ptr(self._factors[s0]), n_pad, sst, _ptr(self._ipiv[s0]), _ptr(x), ldx, xs, sp),
                                "biem_lu_solve")
                        L.check(lib.biem_density(plan.handle, n, B, nrhs, _ptr(x), xs, ldx, 1, _ptr(self._tab[s0]), _ptr(density_t[s0]), sp),
                                "biem_density")
        return _result(op, uin, density_t, axes, B > 1 or not has_rhs)


def biem_factorize(
    c: Any,
    /,
    *,
    centers: Array,
    radii: Array,
    k: Array,
    n_end: int,
    alpha: Array | complex = 1.0,
    beta: Array | complex = 0.0,
    eta: Array | None = None,
    kind: Literal["inner", "outer"] = "outer",
    chunk: int = 0,
    alpha_n: Array | None = None,
    beta_n: Array | None = None,
) -> BIEMFactorization:
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
            factor = lib.biem_factor_ldlt_n if op.per_degree else lib.biem_factor_ldlt
            L.check(factor(plan.handle, nb, B, _ptr(fl.k), _ptr(fl.eta), _ptr(fl.centers), _ptr(fl.radii), fl.geom_batched,
                           _ptr(fl.alpha), _ptr(fl.beta), fl.ab_batched, _ptr(factors), n_pad, n_pad * n_pad, _ptr(tab),
                           _ptr(info), chunk, _ptr(work), wb, sp), "biem_factor_ldlt")
            del work
            # systems the symmetric factorisation rejected (or all of them with BIEM_SOLVER=lu): pivoted LU of the equilibrated
            # system in the same slot, as biem() re-solves them
            redo = np.ones(nb, dtype=bool) if solver == "lu" else (info.cpu().numpy() < 0)
            n_lu = int(redo.sum())
            n_sym = nb - n_lu
            if n_lu > 0:
                ipiv = torch.zeros((nb, n_pad), dtype=torch.int32, device=dev)
                idx = np.flatnonzero(redo)
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
