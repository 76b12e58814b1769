"""Plans (tables per (tree, n_end, device)), cached for the life of the process."""
from __future__ import annotations

import ctypes as C
import os
from typing import Tuple

import numpy as np
import torch

from . import _lib as L
from ._coords import chain_dim


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


_POSITIONS: dict = {}


def _label_positions(tree: str, n_small: int, n_big: int, dev: torch.device) -> np.ndarray:
    """Per harmonic of the plan of order n_small its position on the axis of the plan of order n_big >= n_small, matched by label and
    degree (int64; the axis of a larger order does not begin with the smaller one for every tree)."""
    small, big = _plan(tree, n_small, dev), _plan(tree, n_big, dev)
    key = (id(small), id(big))
    pos = _POSITIONS.get(key)
    if pos is None:
        if small is big:
            pos = np.arange(small.H, dtype=np.int64)
        else:
            where = {tuple(lab) + (int(n),): i for i, (lab, n) in enumerate(zip(big.labels.tolist(), big.degrees.tolist()))}
            pos = np.array([where[tuple(lab) + (int(n),)] for lab, n in zip(small.labels.tolist(), small.degrees.tolist())], dtype=np.int64)
        _POSITIONS[key] = pos
    return pos
