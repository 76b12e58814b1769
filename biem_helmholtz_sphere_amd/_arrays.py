"""Array-namespace plumbing of the binding: where the caller's arrays live, how they reach the GPU and how results go back.

Arrays may be torch tensors (any device; results come back on the inputs' device) or NumPy arrays / Python scalars (moved to the
GPU, results returned as NumPy).  PyTorch only owns device memory and streams.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

Array = Any


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
        return t.cpu().numpy() if self.kind == "numpy" else t.to(self.device)

    def user_array(self, t: torch.Tensor) -> Array:
        """A tensor of the compute device handed to a user callable in the caller's namespace."""
        return self.give(t.to(self.real_dtype), complex_out=False)


def _compute_device(pref: Any = None) -> torch.device:
    if not torch.cuda.is_available():
        raise L.BiemLibraryError("no HIP device visible: biem_helmholtz_sphere_amd computes on MI355X only and has no CPU fallback")
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


def _result_origin(res: Any, x: Any) -> Tuple[_Origin, torch.device]:
    """_origin_of a result record's arrays and the points x; a complex64 density makes the results single precision."""
    origin, dev = _origin_of(res.centers, res.radii, res.k, res.density, x)
    dens = res.density
    if (isinstance(dens, torch.Tensor) and dens.dtype == torch.complex64) or (isinstance(dens, np.ndarray) and dens.dtype == np.complex64):
        origin.real_dtype = torch.float32
    return origin, dev


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


def _shape(a: Any) -> Tuple[int, ...]:
    return tuple(a.shape) if isinstance(a, (torch.Tensor, np.ndarray)) else tuple(np.shape(a))


def _host_array(a: Any) -> np.ndarray:
    """Any accepted input (torch tensor on any device, NumPy array, list, scalar) as a NumPy array on the host."""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _like(v: Any, x: Any) -> Any:
    """v (array or scalar of the creator's namespace) as an array usable with x."""
    if isinstance(x, torch.Tensor):
        if isinstance(v, torch.Tensor):
            return v.to(x.device)
        return torch.as_tensor(np.asarray(v), device=x.device)
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def _stacked(x: Array) -> Array:
    """A list / tuple of coordinate arrays as one array, component axis first."""
    if isinstance(x, (list, tuple)):
        return np.stack([np.asarray(v) for v in x], 0) if not isinstance(x[0], torch.Tensor) else torch.stack(list(x), 0)
    return x


def _bshape_ok(a: Tuple[int, ...], b: Tuple[int, ...]) -> bool:
    try:
        np.broadcast_shapes(tuple(a), tuple(b))
        return True
    except ValueError:
        return False


def _inverse_perm(perm) -> list:
    """inv with inv[perm[i]] = i.  The kernels' gradient components lie along the plan's canonical axes y_i = x_{perm[i]}: out[inv] hands
    them back along the caller's."""
    inv = [0] * len(perm)
    for i, q in enumerate(perm):
        inv[q] = i
    return inv


def _stream_ptr(dev: torch.device) -> int:
    return int(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else int(t.data_ptr())
