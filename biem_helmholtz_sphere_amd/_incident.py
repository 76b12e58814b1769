"""Incident fields (reference ``_biem.py:329-450``), the coefficients of penetrable fluid spheres and the memory guard (:23-74)."""
from __future__ import annotations

import math
from typing import Callable, Tuple

import numpy as np
import torch

from . import _lib as L
from ._arrays import Array, _bshape_ok, _compute_device, _host_array, _inverse_perm, _is_complex, _like, _ptr, _stream_ptr, _to_dev
from ._coords import canonical_tree, harm_count
from ._plans import _label_positions, _plan


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


def regular_expansion(c, /, *, k: Array, origin: Array, coefficients: Array) -> Tuple[Callable[[Array], Array], Callable[[Array], Array]]:
    r"""The source-free field :math:`u(x) = \sum_{h'} p_{h'} j_{n'}(k\|x - o\|) Y_{h'}((x - o)/\|x - o\|)` about ``origin`` o: a beam by its
    beam-shape coefficients, a standing wave, a plane wave by :func:`plane_wave_coefficients` - the incident field of
    ``biem(regular_wave_origin=, regular_wave_coefficients=)``.  ``coefficients`` is complex of shape ``origin.shape[1:] + (H_in,)`` up to
    broadcasting, the last axis along ``harmonic_labels(c, n_in)``; ``n_in`` is inferred from ``H_in`` (a length that is no harmonic
    count of the tree: ``ValueError``).  Normalisation as :func:`regular_wave`.

    Returns (u, grad u) with the shapes of :func:`regular_wave`, evaluated on the device through ``biem_expansion_field`` (the value
    kernels of the scattered field on the coefficient vector; the gradient by one step of the coefficient ladder in the plan of order
    n_in + 1).  The field is entire: ``x = origin`` is an ordinary point."""
    return _expansion_sum(c, k, origin, coefficients, "origin", regular=True)


def multipole_expansion(c, /, *, k: Array, source: Array, coefficients: Array) -> Tuple[Callable[[Array], Array], Callable[[Array], Array]]:
    r"""The outgoing field :math:`u(x) = \sum_{h'} p_{h'} h_{n'}(k\|x - s\|) Y_{h'}((x - s)/\|x - s\|)` radiated from ``source`` s: a general
    multipole, the field of a neighbouring cluster by its ``cluster_coefficients`` - the incident field of
    ``biem(multipole_source_position=, multipole_source_coefficients=)``.  Arguments, shapes and evaluation as
    :func:`regular_expansion`, normalisation as :func:`multipole_source`."""
    return _expansion_sum(c, k, source, coefficients, "source", regular=False)


def plane_wave_coefficients(c, /, *, k: Array, direction: Array, origin: Array, n_in: int) -> Array:
    r"""Regular coefficients of the plane wave ``e^{i k d.x}`` about ``origin`` o, truncated at order ``n_in``:
    :math:`p_h = C_d\, i^{n} \overline{Y_h(\hat d)}\, e^{i k \hat d\cdot o}`, ``C_d = (2 pi)^{d/2} sqrt(2 / pi)`` (4 pi in 3-D), along
    ``harmonic_labels(c, n_in)``; the harmonics by ``biem_harmonics`` on the device.  k has shape (...), direction and origin
    (c_ndim, ...); the result has shape ``direction.shape[1:] + (H_in,)`` broadcast against k and origin, complex128, a tensor where
    any input is one, else NumPy.  A beam given by its angular spectrum is a weighted sum of such vectors; the truncation drops what the
    wave holds in degrees >= n_in, of size ``(k R / 2)^{n_in} / n_in!`` at distance R from o."""
    tree, perm = canonical_tree(c.branching_types_expression_str)
    n_in = int(n_in)
    if n_in < 1:
        raise ValueError(f"n_in must be positive, got {n_in}")
    tens = [a for a in (direction, origin, k) if isinstance(a, torch.Tensor)]
    dev = _compute_device(tens[0].device if tens else None)
    dt, ot, kt = _to_dev(direction, dev, torch.float64), _to_dev(origin, dev, torch.float64), _to_dev(k, dev, torch.complex128)
    d = c.c_ndim
    if dt.ndim < 1 or dt.shape[0] != d or ot.ndim < 1 or ot.shape[0] != d:
        raise ValueError(f"The first dimension of direction and origin must be c.c_ndim={d}, but got shapes {tuple(dt.shape)} and {tuple(ot.shape)}")
    try:
        shape = tuple(torch.broadcast_shapes(tuple(dt.shape[1:]), tuple(ot.shape[1:]), tuple(kt.shape)))
    except RuntimeError as e:
        raise ValueError(f"Shapes of k, direction[1:] and origin[1:] are not broadcastable\n{tuple(kt.shape)=}\n{tuple(dt.shape)=}\n{tuple(ot.shape)=}") from e
    dh = dt / torch.linalg.vector_norm(dt, dim=0, keepdim=True)
    dirs = torch.movedim(dh[list(perm)], 0, -1).contiguous().reshape(-1, d)              # canonical axes, [count, d]
    plan = _plan(tree, n_in, dev)
    Y = torch.empty((dirs.shape[0], plan.H), dtype=torch.complex128, device=dev)
    if dirs.shape[0] > 0:
        with torch.cuda.device(dev):
            L.check(L.load().biem_harmonics(plan.handle, int(dirs.shape[0]), _ptr(dirs), _ptr(Y), _stream_ptr(dev)), "biem_harmonics")
    Cd = (2.0 * math.pi) ** (d / 2.0) * math.sqrt(2.0 / math.pi)
    phase = torch.as_tensor(1j ** (np.asarray(plan.degrees) % 4), dtype=torch.complex128, device=dev)   # (exact powers of i)
    ot = ot.reshape((d,) + (1,) * (dh.ndim - ot.ndim) + tuple(ot.shape[1:])) if ot.ndim < dh.ndim else ot
    p = Cd * phase * torch.conj(Y).reshape(tuple(dt.shape[1:]) + (plan.H,)) * torch.exp(1j * kt * torch.sum(dh * ot, dim=0))[..., None]
    p = p.expand(shape + (plan.H,)).contiguous()
    return p.to(tens[0].device) if tens else p.cpu().numpy()


def _harmonic_order(c, H_in: int, name: str) -> int:
    """The order n_in whose harmonic axis has H_in entries; ValueError naming the nearest valid lengths otherwise."""
    tree = canonical_tree(c.branching_types_expression_str)[0]
    n = 1
    while harm_count(tree, n) < H_in:
        n += 1
    if H_in < 1 or harm_count(tree, n) != H_in:
        below = f"{harm_count(tree, n - 1)} (n_in={n - 1}) and " if n > 1 and H_in >= 1 else ""
        raise ValueError(f"the last axis of {name} has length {H_in}, which is no harmonic count of the tree: the nearest valid lengths are "
                         f"{below}{harm_count(tree, n)} (n_in={n}); the axis runs along harmonic_labels(c, n_in)")
    return n


def _expansion_term(c, k, source, index, n_end, sname: str, *, regular: bool):
    """multipole_source (its argument `sname` = "source") and regular_wave ("origin", regular): one set of checks, one library entry."""
    n_end = int(n_end)
    i_ = np.asarray(index) if isinstance(index, (int, np.integer)) else _host_array(index)
    if i_.dtype.kind not in "iu":
        raise ValueError(f"index must be an integer or an integer array, got dtype {i_.dtype}")
    H = _harm_n_ndim_le(n_end, c.c_ndim)
    if i_.size and (int(i_.min()) < 0 or int(i_.max()) >= H):
        raise ValueError(f"index must lie in [0, H) with H={H} harmonics of degree < n_end={n_end}, got values from {int(i_.min())} to {int(i_.max())}")
    tree = canonical_tree(c.branching_types_expression_str)[0]

    def operand(dev, grad: bool, batch, nb):
        """The indices on the axis of the plan the field runs in: of order n_end, for the gradient of order n_end + 1 (by label)."""
        idx = _label_positions(tree, n_end, n_end + 1, dev)[i_] if grad else i_
        return torch.as_tensor(np.ascontiguousarray(np.broadcast_to(idx, batch)).reshape(nb).astype(np.int32), device=dev)

    return _expansion_field(c, k, source, tuple(i_.shape), "index", n_end, sname, regular, "biem_multipole_field", operand)


def _expansion_sum(c, k, source, coefficients, sname: str, *, regular: bool):
    """regular_expansion and multipole_expansion: _expansion_term's checks and evaluation with a coefficient vector for the index."""
    tree = canonical_tree(c.branching_types_expression_str)[0]
    pshape = tuple(coefficients.shape) if isinstance(coefficients, torch.Tensor) else tuple(np.shape(coefficients))
    if len(pshape) < 1:
        raise ValueError(f"coefficients must have shape {sname}.shape[1:] + (H_in,), got a scalar")
    n_in = _harmonic_order(c, int(pshape[-1]), "coefficients")

    def operand(dev, grad: bool, batch, nb):
        """The coefficient vectors [nb, H] on the axis of the plan the field runs in (the gradient: order n_in + 1, placed by label)."""
        pt = _to_dev(coefficients, dev, torch.complex128)
        pt = pt.reshape((1,) * (len(batch) + 1 - pt.ndim) + tuple(pt.shape)).expand(tuple(batch) + (pshape[-1],)).reshape(nb, pshape[-1])
        if not grad:
            return pt.contiguous()
        out = torch.zeros((nb, _plan(tree, n_in + 1, dev).H), dtype=torch.complex128, device=dev)
        out[:, torch.as_tensor(_label_positions(tree, n_in, n_in + 1, dev), device=dev)] = pt
        return out

    return _expansion_field(c, k, source, pshape[:-1], "coefficients[:-1]", n_in, sname, regular, "biem_expansion_field", operand)


def _expansion_field(c, k, source, ishape, iname: str, n_end: int, sname: str, regular: bool, entry: str, operand):
    """(u, grad u) of a field about `source` whose operand - an index per system (biem_multipole_field) or a coefficient vector
    (biem_expansion_field), of leading shape `ishape`, made by `operand(dev, grad, batch, nb)` on the axis of order n_end, the gradient's
    n_end + 1 - takes the place of the density in the value kernels."""
    tree, perm = canonical_tree(c.branching_types_expression_str)
    perm = list(perm)
    k_ = k if isinstance(k, torch.Tensor) else np.asarray(k)
    s_ = source if isinstance(source, torch.Tensor) else np.asarray(source, dtype=np.float64)
    if s_.ndim < 1 or s_.shape[0] != c.c_ndim:
        raise ValueError(f"The first dimension of {sname} must be c.c_ndim={c.c_ndim}, but got shape {tuple(s_.shape)}")
    if not _bshape_ok(tuple(k_.shape), tuple(s_.shape[1:])) or not _bshape_ok(tuple(ishape), tuple(s_.shape[1:])):
        raise ValueError(f"Shapes of k, {iname} and {sname}[1:] are not broadcastable\n{tuple(k_.shape)=}\n{tuple(ishape)=}\n{tuple(s_.shape)=}")
    if s_.ndim != k_.ndim + 1 or len(ishape) > k_.ndim:
        raise ValueError(f"{sname}.ndim={s_.ndim} is not k.ndim + 1={k_.ndim + 1}" if s_.ndim != k_.ndim + 1 else
                         f"{iname} has {len(ishape)} axes, more than k.ndim={k_.ndim}")
    nd = k_.ndim

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
        batch = tuple(np.broadcast_shapes(tuple(kt.shape), tuple(st.shape[1:]), xb, tuple(ishape)))
        nb, P = math.prod(batch), math.prod(lead)
        out_shape = ((d,) if grad else ()) + lead + batch
        if nb == 0 or P == 0:
            res = torch.empty(out_shape, dtype=torch.complex128, device=dev)
            return res.cpu().numpy() if was_np else res.to(back)
        plan = _plan(tree, n_end + 1 if grad else n_end, dev)
        kf = kt.expand(batch).reshape(nb).contiguous()
        sf = torch.movedim(st[perm], 0, -1).expand(batch + (d,)).reshape(nb, d).contiguous()
        jf = operand(dev, grad, batch, nb)
        xp = xt[perm]
        batched = any(n != 1 for n in xb)
        pts = (xp.expand((d,) + lead + batch).reshape(d, P, nb) if batched else xp.reshape(d, P)).contiguous()
        out = torch.empty(((d,) if grad else ()) + (P, nb), dtype=torch.complex128, device=dev)
        lib = L.load()
        with torch.cuda.device(dev):
            wb = int(lib.biem_multipole_field_workspace_bytes(plan.handle, nb))
            work = torch.empty(max(wb, 16), dtype=torch.uint8, device=dev)
            L.check(getattr(lib, entry)(plan.handle, nb, P, _ptr(kf), _ptr(sf), _ptr(jf), _ptr(pts),
                                        (L.USCAT_POINTS_BATCHED if batched else 0) | (L.USCAT_KIND_INNER if regular else 0),
                                        int(grad), _ptr(out), _ptr(work), wb, _stream_ptr(dev)), entry)
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
