"""NumPy twin of the coefficient ladder behind uscat_hess() (helper module, not a test; CPU only).

For z = h (outer) or z = j (kind inner), with T^i_{h'h} = int y_i Y_h conj(Y_h') dOmega,

    d/dx_i [ z_n(k r) Y_h(e) ] = k [ z_{n-1}(k r) P_{n-1}(e_i Y_h) - z_{n+1}(k r) P_{n+1}(e_i Y_h) ],   P_{n'}(e_i Y_h) = sum_{h' of degree n'} T^i_{h'h} Y_h'

so (D_i c)_{h'} = k sgn(n_h - n_h') sum_h T^i_{h'h} c_h are the coefficients of d_i of the expansion sum_h c_h z_n Y_h, one degree longer.
The table is the plan's own (read from a host plan through ``biem_plan_force_terms``: no device), the radial functions and harmonics
that turn coefficients into a field are the oracle's, at the order n_end + 2 of the twice-laddered set.
"""
import ctypes as C
import math

import numpy as np
from scipy import sparse

from biem_helmholtz_sphere_amd import _lib
from oracle import biem_oracle as O

from test_chain_trees_host import chain

_TERMS, _SPARSE, _TABLES = {}, {}, {}


def oracle_tree(name):
    """The oracle's tree of a built name, the test-local chain for 'b' * (d - 2) + 'a' with d >= 5."""
    return O.tree(name) if name in O._TREES else chain(len(name) + 1)


def plan_terms(tree, n_end):
    """(d, labels [H, lw], deg [H], ptr [H + 1], col, comp, val) of the plan of a canonical tree (a, ba, bba, caa or a chain) at n_end:
    the coupling table as the plan lists it, rows h' in CSR order.  Computed once per (tree, n_end) and never modified."""
    key = (tree, n_end)
    if key in _TERMS:
        return _TERMS[key]
    lib = _lib.load()
    p = C.c_void_p()
    if tree in _lib.TREE_IDS:
        _lib.check(lib.biem_plan_create_host(_lib.TREE_IDS[tree], n_end, C.byref(p)), "biem_plan_create_host")
    else:
        _lib.check(lib.biem_plan_create_chain_host(len(tree) + 1, n_end, C.byref(p)), "biem_plan_create_chain_host")
    try:
        d, H = C.c_int(), C.c_int()
        _lib.check(lib.biem_plan_info(p, C.byref(d), C.byref(H), None, None, None))
        d, H = d.value, H.value
        lw = 3 if tree in _lib.TREE_IDS else d - 1
        lab, deg = np.zeros((H, lw), dtype=np.int32), np.zeros(H, dtype=np.int32)
        _lib.check(lib.biem_plan_labels_n(p, lw, lab.ctypes.data, deg.ctypes.data), "biem_plan_labels_n")
        n = C.c_longlong(-1)
        _lib.check(lib.biem_plan_force_terms(p, C.byref(n), None, None, None, None), "biem_plan_force_terms")
        ptr = np.zeros(H + 1, dtype=np.int64)
        col, comp = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        val = np.zeros(n.value, dtype=np.complex128)
        _lib.check(lib.biem_plan_force_terms(p, None, ptr.ctypes.data, col.ctypes.data, comp.ctypes.data, val.ctypes.data), "biem_plan_force_terms")
    finally:
        lib.biem_plan_destroy(p)
    assert (deg == oracle_tree(tree).degrees(n_end)).all()          # the plan lists its harmonics in the oracle's order
    for a in (lab, deg, ptr, col, comp, val):
        a.setflags(write=False)
    _TERMS[key] = (d, lab, deg, ptr, col, comp, val)
    return _TERMS[key]


def csr_tables(d, H, ptr, col, comp, val):
    """[T^0 .. T^{d-1}] as SciPy CSR [H, H] (rows h', columns h) from the listing of biem_plan_force_terms."""
    rows = np.repeat(np.arange(H), np.diff(ptr))
    return [sparse.csr_matrix((val[comp == i], (rows[comp == i], col[comp == i])), shape=(H, H)) for i in range(d)]


def plan_table_sparse(tree, n_end):
    """(d, labels [H, lw], deg [H], [T^i as CSR [H, H]]) of the plan: what the orders need whose dense table is gigabytes."""
    key = (tree, n_end)
    if key not in _SPARSE:
        d, lab, deg, ptr, col, comp, val = plan_terms(tree, n_end)
        _SPARSE[key] = (d, lab, deg, csr_tables(d, len(deg), ptr, col, comp, val))
    return _SPARSE[key]


def plan_table(tree, n_end):
    """(d, labels [H, lw], deg [H], T [d, H, H] dense) of the plan; computed once per (tree, n_end) and never modified."""
    key = (tree, n_end)
    if key not in _TABLES:
        d, lab, deg, ptr, col, comp, val = plan_terms(tree, n_end)
        H = len(deg)
        T = np.zeros((d, H, H), dtype=np.complex128)
        T[comp, np.repeat(np.arange(H), np.diff(ptr)), col] = val
        T.setflags(write=False)
        _TABLES[key] = (d, lab, deg, T)
    return _TABLES[key]


def embed(tree, n_end):
    """Position of every harmonic of the order-n_end plan in the plan of order n_end + 2, matched by label and degree."""
    _, lab, deg = plan_terms(tree, n_end)[:3]
    _, lab2, deg2 = plan_terms(tree, n_end + 2)[:3]
    where = {tuple(l) + (int(n),): i for i, (l, n) in enumerate(zip(lab2.tolist(), deg2.tolist()))}
    idx = np.array([where[tuple(l) + (int(n),)] for l, n in zip(lab.tolist(), deg.tolist())])
    assert len(set(idx.tolist())) == len(idx)
    return idx


def ladder(T, deg, k, c, i, n_src=None):
    """D_i c along canonical axis i; c[..., H] in the layout of the table.  Columns of degree >= n_src are skipped.  T is the dense
    [d, H, H] table or the list of CSR matrices of plan_table_sparse (the same sums over the stored entries alone)."""
    if sparse.issparse(T[i]):
        M = T[i].tocoo()
        w = M.data * np.sign(deg[M.col] - deg[M.row])
        if n_src is not None:
            w = w * (deg[M.col] < n_src)
        M = sparse.csr_matrix((w, (M.row, M.col)), shape=M.shape)
        flat = np.asarray(c, dtype=np.complex128).reshape(-1, M.shape[1])
        return k * (M @ flat.T).T.reshape(np.shape(c)[:-1] + (M.shape[0],))
    sgn = np.sign(deg[None, :] - deg[:, None]).astype(np.float64)        # [h', h]
    M = T[i] * sgn
    if n_src is not None:
        M = M * (deg < n_src)[None, :]
    return k * np.einsum("gh,...h->...g", M, c)


def hessian_coefs(tree, n_end, k, c, sparse_table=False):
    """D_j D_i c [d, d, ..., H2] in the layout of the plan of order n_end + 2 from c[..., H] in the order-n_end layout."""
    d, _, deg2, T = (plan_table_sparse if sparse_table else plan_table)(tree, n_end + 2)
    idx = embed(tree, n_end)
    c2 = np.zeros(c.shape[:-1] + (len(deg2),), dtype=np.complex128)
    c2[..., idx] = c
    g = [ladder(T, deg2, k, c2, i, n_end) for i in range(d)]
    return c2, np.stack([np.stack([ladder(T, deg2, k, g[i], j, n_end + 1) for j in range(d)]) for i in range(d)])


def near_coefs(name, n_end, k, eta, radii, density, kind):
    """c[b, h] = density blc_n(rho_b) as oracle.biem_oracle.uscat forms it (kind inner: blc from h_n, h_n' at k rho)."""
    tr = oracle_tree(name)
    d, deg = tr.d, tr.degrees(n_end)
    out = []
    for b, rho in enumerate(radii):
        j, h, jp, hp = O.radial_h(n_end - 1, d, k * rho)
        if kind == "inner":
            j, jp = h, hp
        blc = 1j * k ** (d - 1) * rho ** (d - 1) * jp - 1j * eta * (1j * k ** (d - 2) * rho ** (d - 1) * j)
        out.append(np.asarray(density[b]) * blc[deg])
    return np.stack(out)


def series(tree, n_end, k, kind, centers, coefs, x):
    """sum_b sum_h coefs[..., b, h] z_n(k |x - c_b|) Y_h at x[P, d] in the canonical axes of `tree` -> [..., P], unmasked."""
    tr = oracle_tree(tree)
    d, deg = tr.d, tr.degrees(n_end)
    out = 0.0
    for b, cb in enumerate(centers):
        rel = x - cb[None, :]
        r = np.linalg.norm(rel, axis=-1)
        rs = np.where(r > 0, r, 1.0)
        Y = tr.harmonics(rel / rs[:, None], n_end)
        zn = np.empty((n_end, len(x)), dtype=np.complex128)
        for p, rp in enumerate(rs):
            jj, hh, _, _ = O.radial_h(n_end - 1, d, k * rp)
            zn[:, p] = jj if kind == "inner" else hh
            if kind == "inner" and r[p] == 0.0:          # z_n(0) = delta_n0 sqrt(pi/2) 2^{1-d/2} / Gamma(d/2)
                zn[:, p] = 0.0
                zn[0, p] = math.sqrt(math.pi / 2) * 2.0 ** (1 - d / 2) / math.gamma(d / 2)
        out = out + np.einsum("...h,hp->...p", coefs[..., b, :], zn[deg, :] * Y)
    return out


def hessian(name, n_end, k, eta, kind, centers, radii, density, x, sparse_table=False):
    """The twin's Hessian [d, d, P] of the near field of a record at x[P, d], in the caller's axes of tree `name`, unmasked."""
    tr = oracle_tree(name)
    canon = tr.base or name
    perm = list(tr.perm) if tr.base else list(range(tr.d))            # canonical y_i = x_{perm[i]}
    c = near_coefs(name, n_end, k, eta, radii, density, kind)
    _, hc = hessian_coefs(canon, n_end, k, c, sparse_table)
    Hc = series(canon, n_end + 2, k, kind, np.asarray(centers)[:, perm], hc, np.asarray(x)[:, perm])
    out = np.empty_like(Hc)
    for i in range(tr.d):
        for j in range(tr.d):
            out[perm[i], perm[j]] = Hc[i, j]
    return out
