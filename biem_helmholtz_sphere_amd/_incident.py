"""Incident fields (reference ``_biem.py:329-450``), the coefficients of penetrable fluid spheres and the memory guard (:23-74)."""
from __future__ import annotations

import math
from typing import Callable, Tuple

import numpy as np
import torch

from . import _lib as L
from ._arrays import Array, _bshape_ok, _compute_device, _host_array, _inverse_perm, _is_complex, _like, _ptr, _stream_ptr, _to_dev
from ._coords import canonical_tree
from ._plans import _plan


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


# --------------------------------------------------------------------------------------
# incident fields (reference :329-450)
# --------------------------------------------------------------------------------------
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
        raise ValueError("Shapes of k and direction[1:] are not broadcastable\n"
                         f"tuple(k.shape)={tuple(k_.shape)}\ntuple(direction.shape)={tuple(d_.shape)}")
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
        h, _ = _radial(int(rel.shape[0]), kt * r)      # (k and the source may each have batch axes the other has at size 1)
        return _back(h, was_np, dev)

    def inner_grad(x: Array, /) -> Array:
        was_np, dev, rel, r, kt = _prep(x)
        _, hp = _radial(int(rel.shape[0]), kt * r)
        coeff = kt * hp / r
        return _back(coeff[None, ...] * rel, was_np, dev)

    return inner, inner_grad


def harmonic_labels(c, /, n_end: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(labels [H, width], degrees [H])`` of the harmonic axis at order ``n_end``, NumPy: the axis of ``density[..., H]`` and the axis
    ``multipole_source_index`` counts along, in the labels of the canonical tree (a tree with primed nodes runs as its canonical tree in
    permuted axes).  Labels: (m, -, -) for a, (n, m, -) for ba, (n, l, m) for bba, (n, m1, m2) for caa, (l_0 .. l_{d-3}, m) for the chains.
    The axis at a larger n_end does not begin with this one for every tree: look an index up by its label, not by its position."""
    tree, _ = canonical_tree(c.branching_types_expression_str)
    plan = _plan(tree, int(n_end), _compute_device(None))
    return plan.labels.copy(), plan.degrees.copy()


def multipole_source(c, /, *, k: Array, source: Array, index, n_end: int) -> Tuple[Callable[[Array], Array], Callable[[Array], Array]]:
    r"""Outgoing multipole :math:`u(x) = h_{n'}(k\|x - source\|) Y_{h'}((x - source)/\|x - source\|)`, h' = ``index`` a position on the
    harmonic axis of order ``n_end`` (:func:`harmonic_labels`), n' its degree: a solution of the Helmholtz equation for every degree, which
    ``point_source(n=)`` with n > 0 is not.  Normalisation: orthonormal harmonics Y_h of the tree c and the project's radial functions
    h_n = sqrt(pi/2) H_{n+d/2-1}(z) / z^{d/2-1}; an index of degree 0 gives ``Y_0 h_0(k |x - s|)``, point_source's n = 0 field times the
    constant ``Y_0 = |S^{d-1}|^{-1/2}``.

    k has shape (...), source (c_ndim, ...), index is an integer or an integer array broadcastable to source.shape[1:].  Returns
    (u, grad u) with point_source's shapes: x of shape (c_ndim, ...(any), ...) gives (...(any), ...) and (c_ndim, ...(any), ...).  Both
    evaluate on the device through ``biem_multipole_field`` (the value kernels of the scattered field on one coefficient; the gradient by
    one step of the coefficient ladder in the plan of order n_end + 1)."""
    return _expansion_term(c, k, source, index, n_end, "source", regular=False)


def regular_wave(c, /, *, k: Array, origin: Array, index, n_end: int) -> Tuple[Callable[[Array], Array], Callable[[Array], Array]]:
    r"""Regular wave :math:`u(x) = j_{n'}(k\|x - origin\|) Y_{h'}((x - origin)/\|x - origin\|)`, h' = ``index`` a position on the harmonic
    axis of order ``n_end`` (:func:`harmonic_labels`): the basis in which every source-free solution of the Helmholtz equation is written
    about ``origin`` (beams by their beam-shape coefficients, standing waves), and the incident field of
    ``biem(regular_wave_origin=, regular_wave_index=)``.  Normalisation as :func:`multipole_source`, with the regular radial functions
    j_n = sqrt(pi/2) J_{n+d/2-1}(z) / z^{d/2-1}.

    Arguments, shapes and evaluation as :func:`multipole_source` (``biem_multipole_field`` with the kind-inner value kernels: the same
    coefficient, the regular radial function).  The field is entire: ``x = origin`` is an ordinary point of value and gradient."""
    return _expansion_term(c, k, origin, index, n_end, "origin", regular=True)


def _expansion_term(c, k, source, index, n_end, sname: str, *, regular: bool):
    """multipole_source (its argument `sname` = "source") and regular_wave ("origin", regular): one set of checks, one library entry."""
    tree, perm = canonical_tree(c.branching_types_expression_str)
    perm = list(perm)
    n_end = int(n_end)
    k_ = k if isinstance(k, torch.Tensor) else np.asarray(k)
    s_ = source if isinstance(source, torch.Tensor) else np.asarray(source, dtype=np.float64)
    i_ = np.asarray(index) if isinstance(index, (int, np.integer)) else _host_array(index)
    if i_.dtype.kind not in "iu":
        raise ValueError(f"index must be an integer or an integer array, got dtype {i_.dtype}")
    H = _harm_n_ndim_le(n_end, c.c_ndim)
    if i_.size and (int(i_.min()) < 0 or int(i_.max()) >= H):
        raise ValueError(f"index must lie in [0, H) with H={H} harmonics of degree < n_end={n_end}, got values from {int(i_.min())} to {int(i_.max())}")
    if s_.ndim < 1 or s_.shape[0] != c.c_ndim:
        raise ValueError(f"The first dimension of {sname} must be c.c_ndim={c.c_ndim}, but got shape {tuple(s_.shape)}")
    if not _bshape_ok(tuple(k_.shape), tuple(s_.shape[1:])) or not _bshape_ok(tuple(i_.shape), tuple(s_.shape[1:])):
        raise ValueError(f"Shapes of k, index and {sname}[1:] are not broadcastable\n{tuple(k_.shape)=}\n{tuple(i_.shape)=}\n{tuple(s_.shape)=}")
    if s_.ndim != k_.ndim + 1:
        raise ValueError(f"{sname}.ndim={s_.ndim} is not k.ndim + 1={k_.ndim + 1}")
    nd = k_.ndim
    raised: dict = {}                         # device index -> the indices on the axis of order n_end + 1 (the gradient's plan)

    def _raised_index(dev) -> np.ndarray:
        key = dev.index
        if key not in raised:
            small, big = _plan(tree, n_end, dev), _plan(tree, n_end + 1, dev)
            where = {tuple(lab) + (int(n),): j for j, (lab, n) in enumerate(zip(big.labels.tolist(), big.degrees.tolist()))}
            raised[key] = np.array([where[tuple(lab) + (int(n),)] for lab, n in zip(small.labels.tolist(), small.degrees.tolist())], dtype=np.int64)
        return raised[key][i_]

    def _field(x, grad: bool):
        was_np = not isinstance(x, torch.Tensor)
        back = None if was_np else x.device
        dev = _compute_device(back)
        xt = _to_dev(x, dev, torch.float64)
        d = int(xt.shape[0])
        if xt.ndim - 1 < nd:                                                       # (broadcasting against the batch prepends axes)
            xt = xt.reshape((d,) + (1,) * (nd - xt.ndim + 1) + tuple(xt.shape[1:]))
        lead, xb = tuple(xt.shape[1:xt.ndim - nd]), tuple(xt.shape[xt.ndim - nd:])
        st = _to_dev(s_, dev, torch.float64)
        kt = _to_dev(k_, dev, torch.complex128)
        batch = tuple(np.broadcast_shapes(tuple(kt.shape), tuple(st.shape[1:]), xb))
        nb, P = math.prod(batch), math.prod(lead)
        out_shape = ((d,) if grad else ()) + lead + batch
        if nb == 0 or P == 0:
            res = torch.empty(out_shape, dtype=torch.complex128, device=dev)
            return res.cpu().numpy() if was_np else res.to(back)
        plan = _plan(tree, n_end + 1 if grad else n_end, dev)
        idx = _raised_index(dev) if grad else i_
        kf = kt.expand(batch).reshape(nb).contiguous()
        sf = torch.movedim(st[perm], 0, -1).expand(batch + (d,)).reshape(nb, d).contiguous()
        jf = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(idx, batch)).reshape(nb).astype(np.int32), device=dev)
        xp = xt[perm]
        batched = any(n != 1 for n in xb)
        pts = (xp.expand((d,) + lead + batch).reshape(d, P, nb) if batched else xp.reshape(d, P)).contiguous()
        out = torch.empty(((d,) if grad else ()) + (P, nb), dtype=torch.complex128, device=dev)
        lib = L.load()
        with torch.cuda.device(dev):
            wb = int(lib.biem_multipole_field_workspace_bytes(plan.handle, nb))
            work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
            L.check(lib.biem_multipole_field(plan.handle, nb, P, _ptr(kf), _ptr(sf), _ptr(jf), _ptr(pts),
                                             (L.USCAT_POINTS_BATCHED if batched else 0) | (L.USCAT_KIND_INNER if regular else 0),
                                             int(grad), _ptr(out), _ptr(work), wb, _stream_ptr(dev)), "biem_multipole_field")
        res = out.reshape(out_shape)
        if grad:
            res = res[_inverse_perm(perm)]                                          # canonical component i is the caller's perm[i]
        return res.cpu().numpy() if was_np else res.to(back)

    def inner(x: Array, /) -> Array:
        return _field(x, False)

    def inner_grad(x: Array, /) -> Array:
        return _field(x, True)

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
