"""One application z = M^-1 r of each preconditioner that is applied "as a vector of its own"
(lsb_hip_solver_precond_dev), against an exact reference of the same operation.

A solve cannot see a wrong preconditioner: PCG reaches the right x with any SPD M, a few iterations
later.  Here z itself is compared with z* = M^-1 r computed in numpy / scipy -- float64 solves
refined three times with np.longdouble residuals, np.longdouble recurrences and products -- within a
rounding-error bound that follows from the operation (eps = 2^-52):

block-Jacobi  per block B_k = S[b0:b0+m, b0:b0+m] (blocks restart at every shard's first row)
                  ||z_k - z*_k||_2 <= C_BJ m eps cond_2(B_k) ||B_k^-1||_2 ||r_k||_2
Chebyshev     normwise, the recurrence of precond_setup / k_cheb_first / k_cheb_step with a[k], b[k],
              c0 recomputed here from the DEVICE's interval (Solver.cheb_interval)
                  ||z - z*||_2 <= C_CHEB (m + 1) (k_max + 8) eps (||z*||_2 + c0 ||D r||_2)
              (k_max = the longest row, D = dinv; a linear-growth model, not a rigorous bound), and the
              interval itself: |lmax - lmax_ref| <= 20 n eps lmax_ref against a numpy power iteration,
              lmin = lmax / max(30, 16 m^2) to 2 eps
FSAI          G* on lsb_csr_fsai_pattern(S, power, 128), row i from the exact S[J, J] y = e_last,
              g_i = y / sqrt(y_last); t* = G* r, z* = G*^T t*.  With rho_i = C_FSAI m_i eps cond_2(S[J_i, J_i]),
                  tau_i  = rho_i ||g_i|| ||r_J|| + (m_i + 1) eps |g_i|.|r_J|
                  beta_j = sum_{i: j in J_i} (|g_ij| tau_i + rho_i ||g_i|| |t_i|) + (c_j + 1) eps sum_i |g_ij| |t_i|
                  |z - z*|_j <= beta_j                         (c_j = entries of column j of G)

The constants are pinned on the CPU against the reference, never against the device:
test_bounds_hold_for_fp64_restatements runs a float64 numpy restatement of the product's algorithm
(in-place Gauss-Jordan without pivoting, then X^T r; the recurrence in float64 with scipy's SpMV;
np.linalg.cholesky per FSAI row and scipy's products) on the inputs of every GPU case and keeps it
within 1/4 of the bound -- the factor 4 is the room left for fused multiply-adds and other summation
orders on the device.  Each constant is chosen so that the restatement's worst ratio over all cases
lies between 1/16 and 1/4: C_BJ is four times what the restatement needs where a block is one row
(z = (1 / d) r: two roundings against a bound of one eps), C_CHEB and C_FSAI came down from 1.

Worst error / bound, the float64 restatement on the CPU and the device (MI355X, `-m gpu -s` prints every case):

                constant        restatement (CPU)                             device (GPU)
block-Jacobi    C_BJ   = 3.7    0.244  xn3b_A_18, 1-row blocks, normal r      0.244  the same case (the same roundings)
Chebyshev       C_CHEB = 0.25   0.068  lap3d 40 x 36 x 30, degree 3, unit r   0.055  the same over 3 shards, as launches
FSAI            C_FSAI = 0.5    0.073  xn3b_A_18, power 1, normal r           0.035  xn3b_A_18, power 1, sin r
The device's lmax is within 1.4e-5 of its allowance 20 n eps lmax (xn3b_A_18; bit for bit numpy's on the
stencils on one shard), the asymmetry |u.M^-1 v - v.M^-1 u| within 5e-5 of its allowance (Chebyshev; AMG 1.4e-5).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import lsbench_amd as la
from lsbench_amd import _lib

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is plain double here: the references would not be exact"
EPS = 2.0 ** -52

C_BJ, C_CHEB, C_FSAI = 3.7, 0.25, 0.5
RESTATED_WITHIN = 0.25

GOLDEN = ("xn3b_A_18", "tj7a_A_12")
BJ_SIZES = (1, 2, 8, 63, 64, 65, 100, 128, 129, 200, "n-1", "n", 1 << 20)
# (operator, block size, nvirt, line padding)
BJ_CASES = ([(name, bs, 1, 0) for name in GOLDEN for bs in BJ_SIZES]
            + [(name, bs, nv, 0) for name in GOLDEN for nv in (2, 3) for bs in (16, 100)]
            + [("lap3d:nx=12,ny=9,nz=7", bs, 1, 0) for bs in (7, 64)]
            + [("lap2d:nx=1024,ny=1100", 8, 1, 0)]
            + [("lap2d:nx=1000,ny=60", bs, 1, 1) for bs in (8, 100)])
CHEB_DEGREES = (1, 2, 3, 4, 7, 32, 40)
# (operator, options, environment); every one at every degree
CHEB_CONFIGS = (
    ("xn3b_A_18", {}, {}),
    ("lap2d:nx=301,ny=187", dict(spmv_variant="SPMV_SELL"), {"LSBENCH_HIP_CHEB_FUSE": "0"}),
    ("lap2d:nx=301,ny=187", dict(spmv_variant="SPMV_SELL"), {"LSBENCH_HIP_CHEB_FUSE": "1"}),
    ("lap2d:nx=301,ny=187", dict(spmv_variant="SPMV_SELL", precision="PREC_MIXED"), {"LSBENCH_HIP_CHEB_FUSE": "0"}),
    ("lap2d:nx=301,ny=187", dict(spmv_variant="SPMV_SELL", precision="PREC_MIXED"), {"LSBENCH_HIP_CHEB_FUSE": "1"}),
    ("lap3d:nx=40,ny=36,nz=30", dict(spmv_variant="SPMV_SELL", nvirt=3, comm="COMM_AUTO", overlap=0),
     {"LSBENCH_HIP_CHEB_FUSE": "0"}),
    ("lap3d:nx=40,ny=36,nz=30", dict(spmv_variant="SPMV_SELL", nvirt=3, comm="COMM_AUTO", overlap=0),
     {"LSBENCH_HIP_CHEB_FUSE": "1"}),
    ("lap3d:nx=40,ny=36,nz=30", dict(spmv_variant="SPMV_SELL", nvirt=4, comm="COMM_P2P", overlap=0),
     {"LSBENCH_HIP_CHEB_FUSE": "0"}),
    ("lap3d:nx=40,ny=36,nz=30", dict(spmv_variant="SPMV_SELL", nvirt=4, comm="COMM_P2P", overlap=0),
     {"LSBENCH_HIP_CHEB_FUSE": "1"}),
    ("lap2d:nx=1000,ny=60", {}, {"LSBENCH_HIP_PAD_LINES": "1"}),
    ("lap2d:nx=60,ny=50", dict(reorder=1), {}),
)
FSAI_CASES = (("xn3b_A_18", 1), ("xn3b_A_18", 2), ("xn3b_A_18", 3), ("tj7a_A_12", 1), ("tj7a_A_12", 2),
              ("lap3d:nx=9,ny=8,nz=7", 2), ("powerlaw:n=900,avg=9,max=300,seed=3,spd=1", 2),
              ("band:hb=31", 1), ("band:hb=32", 1))   # rows of exactly 32 and of exactly 33 entries


# ---- operators and right-hand sides --------------------------------------------------------------
def _scipy(offs, cols, vals):
    n = len(offs) - 1
    M = sp.csr_matrix((np.array(vals, np.float64), np.array(cols, np.int64), np.array(offs, np.int64)), shape=(n, n))
    M.sum_duplicates()
    M.sort_indices()
    return M


def _band(hb, n=150):
    """banded, symmetric, strictly diagonally dominant: row i of tril has min(i, hb) + 1 entries"""
    i = np.arange(n)
    L = sp.lil_matrix((n, n))
    for k in range(1, hb + 1):
        L.setdiag(-(1.0 + 0.5 * np.sin(i[k:] + 3.0 * k)) / (k + 1.0), -k)
    L = L.tocsr()
    M = L + L.T
    M = (M + sp.diags(1.0 + abs(M).sum(axis=1).A1)).tocsr()
    M.sort_indices()
    return M


_OPS = {}


def operator(name, matrix_path):
    """(scipy CSR of the operator the solver makes, what to hand to Solver, extra options)"""
    if name not in _OPS:
        if name in GOLDEN:               # LSB_OP_CHOLMOD_UPPER: the upper triangle mirrored
            A = la.lsbench_matrix_read(matrix_path(name))
            M = _scipy(A.offs, np.asarray(A.cols).astype(np.int64) - A.base, A.vals)
            S = (sp.triu(M, 0, format="csr") + sp.triu(M, 1, format="csr").T).tocsr()
            S.sort_indices()
            _OPS[name] = (S, A, {})
        elif name.startswith("band:"):
            S = _band(int(name.split("=")[1]))
            _OPS[name] = (S, la.Matrix.from_arrays(S.indptr, S.indices, S.data), dict(op_mode=_lib.OP_RAW))
        else:                            # LSB_OP_RAW: the CSR as it is
            A = la.lsbench_matrix_synth(name)
            S = _scipy(A.offs, np.asarray(A.cols).astype(np.int64) - A.base, A.vals)
            assert abs(S - S.T).max() == 0.0
            _OPS[name] = (S, A, dict(op_mode=_lib.OP_RAW))
    return _OPS[name]


def as_matrix(S):
    return la.Matrix.from_arrays(S.indptr, S.indices, S.data)


def rhs3(n, j):
    """the three right-hand sides of every case, as columns"""
    R = np.zeros((n, 3))
    R[:, 0] = np.sin(np.arange(n, dtype=np.float64)) + 0.5
    R[:, 1] = np.random.default_rng(20240229).standard_normal(n)
    R[j, 2] = 1.0
    return R


RNAMES = ("sin", "normal", "unit")


def padded(S):
    """lsb_csr_pad_lines(S, 128): (the padded operator, map[padded row] = row of S or -1)"""
    lib = _lib.load()
    nx, nxp = C.c_uint(0), C.c_uint(0)
    mp = C.POINTER(C.c_int)()
    A = as_matrix(S)
    P = lib.lsb_csr_pad_lines(A.ptr, 128, C.byref(nx), C.byref(nxp), C.byref(mp))
    assert P, "not a grid lsb_csr_pad_lines pads"
    p = P.contents
    offs = np.ctypeslib.as_array(p.offs, (p.nrows + 1,)).copy()
    Sp = _scipy(offs, np.ctypeslib.as_array(p.cols, (offs[-1],)).copy(),
                np.ctypeslib.as_array(p.vals, (offs[-1],)).copy())
    pmap = np.ctypeslib.as_array(mp, (p.nrows,)).astype(np.int64)
    _lib.libc_free(mp)
    lib.lsb_csr_free(P)
    return Sp, pmap


# ---- exact dense solves --------------------------------------------------------------------------
def _matmul_ld(stack, y):
    """stack @ y with np.longdouble products and sums, a few rows of the blocks at a time"""
    nb, m, _ = stack.shape
    out = np.empty(y.shape, LD)
    step = max(1, min(m, (1 << 22) // max(1, nb * m)))
    for i0 in range(0, m, step):
        out[:, i0:i0 + step] = np.matmul(stack[:, i0:i0 + step].astype(LD), y)
    return out


def exact_solve(stack, rhs):
    """stack[k] y[k] = rhs[k]: float64 solves, three refinements on np.longdouble residuals"""
    if stack.shape[1] > 512:
        lus = [scipy.linalg.lu_factor(B) for B in stack]
        solve = lambda b: np.stack([scipy.linalg.lu_solve(lu, bk) for lu, bk in zip(lus, b)])
    else:
        solve = lambda b: np.linalg.solve(stack, b)
    y = solve(rhs).astype(LD)
    for _ in range(3):
        res = rhs.astype(LD) - _matmul_ld(stack, y)
        y = y + solve(res.astype(np.float64)).astype(LD)
    return y


def spd_cond(stack):
    """(cond_2, ||.^-1||_2) of every symmetric positive definite block"""
    ev = np.linalg.eigvalsh(stack)
    assert (ev[:, 0] > 0).all()
    return ev[:, -1] / ev[:, 0], 1.0 / ev[:, 0]


# ---- block-Jacobi --------------------------------------------------------------------------------
def shard_bounds(S, nvirt):
    P = nvirt if nvirt > 1 else 1
    if P > S.shape[0] // 2:              # lsb_hip_solver_create
        P = 1
    return la.lsb_csr_partition_rows(as_matrix(S), P)


def bj_groups(S, bounds, bs):
    """the blocks by size: [(first rows, dense blocks (nb, m, m))]; blocks restart at every shard's first
    row, a block size above a shard's rows is that shard's rows"""
    n = S.shape[0]
    start = np.empty(n, np.int64)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        b = min(bs, hi - lo)
        i = np.arange(lo, hi)
        start[lo:hi] = lo + (i - lo) // b * b
    first = np.unique(start)
    size = np.diff(np.append(first, n))
    for lo in bounds[1:-1]:
        assert lo in first
    coo = S.tocoo()
    bid = np.searchsorted(first, start)
    keep = (coo.col >= start[coo.row]) & (coo.col < start[coo.row] + size[bid[coo.row]])
    er, ec, ev = coo.row[keep], coo.col[keep], coo.data[keep]
    out = []
    for m in np.unique(size):
        which = np.nonzero(size == m)[0]
        slot = -np.ones(len(first), np.int64)
        slot[which] = np.arange(len(which))
        stack = np.zeros((len(which), m, m))
        e = size[bid[er]] == m
        stack[slot[bid[er[e]]], er[e] - start[er[e]], ec[e] - start[er[e]]] = ev[e]
        out.append((first[which], stack))
    return out


def _rows_of(first, m):
    return first[:, None] + np.arange(m)[None, :]


_BJ_REF = {}


def bj_reference(key, S, bounds, bs, R):
    """per size class: (first rows, m, z* (nb, m, 3), m eps cond ||B^-1|| per block, r per block)"""
    if key not in _BJ_REF:
        ref = []
        for first, stack in bj_groups(S, bounds, bs):
            m = stack.shape[1]
            Rb = R[_rows_of(first, m)]                                   # (nb, m, 3)
            cond, ninv = spd_cond(stack)
            ref.append((first, m, exact_solve(stack, Rb), m * EPS * cond * ninv, Rb))
        _BJ_REF[key] = ref
    return _BJ_REF[key]


def bj_ratio(ref, Z):
    """worst over blocks and right-hand sides of ||z_k - z*_k|| / bound_k; a block with r_k = 0 must be 0"""
    worst = np.zeros(Z.shape[1])
    for first, m, zs, f, Rb in ref:
        err = np.sqrt((((Z[_rows_of(first, m)].astype(LD) - zs) ** 2).sum(axis=1)).astype(np.float64))
        bound = C_BJ * f[:, None] * np.linalg.norm(Rb, axis=1)
        assert (err[bound == 0.0] == 0.0).all()
        worst = np.maximum(worst, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0).max(axis=0))
    return worst


def bj_bound_norm(ref):
    """||bound||_2 over all blocks, per right-hand side"""
    return np.sqrt(sum(((C_BJ * f[:, None] * np.linalg.norm(Rb, axis=1)) ** 2).sum(axis=0) for _, _, _, f, Rb in ref))


def gauss_jordan(stack):
    """the product's inversion (k_gj_rowcol / k_gj_update) in float64: pivot p of every block per step"""
    A = stack.copy()
    m = A.shape[1]
    if m > 512:                           # rank-one updates by BLAS (dger), one block at a time
        for k in range(A.shape[0]):
            F = np.asfortranarray(A[k])
            for p in range(m):
                piv, col, row = F[p, p], F[:, p].copy(), F[p, :].copy()
                F = scipy.linalg.blas.dger(-1.0 / piv, col, row, a=F, overwrite_a=1)
                F[p, :], F[:, p] = row / piv, -col / piv
                F[p, p] = 1.0 / piv
            A[k] = F
        return A
    for p in range(m):
        piv, col, row = A[:, p, p].copy(), A[:, :, p].copy(), A[:, p, :].copy()
        A -= col[:, :, None] * row[:, None, :] / piv[:, None, None]
        A[:, p, :], A[:, :, p] = row / piv[:, None], -col / piv[:, None]
        A[:, p, p] = 1.0 / piv
    return A


def bj_setup(case, matrix_path):
    name, bs, nvirt, pad = case
    S, A, kw = operator(name, matrix_path)
    n = S.shape[0]
    bs = {"n-1": n - 1, "n": n}.get(bs, bs)
    R = rhs3(n, n - 1)
    pmap = None
    if pad:                               # blocks live in the padded numbering: r through the map, pad rows 0
        S, pmap = padded(S)
        Rp = np.zeros((S.shape[0], 3))
        Rp[pmap >= 0] = R[pmap[pmap >= 0]]
    else:
        Rp = R
    bounds = shard_bounds(S, nvirt)
    eff = min(bs, S.shape[0])             # (1 << 20 and n: the same blocks, the same reference)
    ref = bj_reference((name, eff, nvirt, pad), S, bounds, eff, Rp)
    return S, A, kw, bs, R, Rp, pmap, bounds, ref


# ---- Chebyshev -----------------------------------------------------------------------------------
def power_lmax(S, dinv):
    """precond_setup's estimate: 20 normalised steps of D^-1 S from the fixed start vector, 10 % on top"""
    n = S.shape[0]
    v = 1.0 + ((np.arange(n, dtype=np.uint64) * 7919) % 1024).astype(np.float64) / 1024.0
    vv, lam = v @ v, 1.0
    for _ in range(20):
        w = dinv * (S @ v)
        ww = w @ w
        lam = np.sqrt(ww / vv)
        v = w * (1.0 / np.sqrt(ww))
        vv = 1.0
    return 1.1 * lam


def cheb_coeffs(m, lmin, lmax):
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    a, b = [], []
    for _ in range(m):
        rho_new = 1.0 / (2.0 * sigma - rho)
        a.append(rho_new * rho), b.append(2.0 * rho_new / delta)
        rho = rho_new
    return 1.0 / theta, a, b


def cheb_apply(S, dinv, R, c0, a, b, T):
    """d = c0 D r, z = d; then d = a_k d + b_k D (r - S z), z += d -- in T (np.longdouble: the reference, its
    SpMV by np.add.reduceat over np.longdouble products; np.float64: the restatement, scipy's SpMV)"""
    Dv, Rt = dinv.astype(T)[:, None], R.astype(T)
    d = T(c0) * (Dv * Rt)
    z = d.copy()
    vals = S.data.astype(T)[:, None]
    for ak, bk in zip(a, b):
        w = np.add.reduceat(vals * z[S.indices], S.indptr[:-1], axis=0) if T is LD else S @ z
        d = T(ak) * d + T(bk) * (Dv * (Rt - w))
        z = z + d
    return z


def cheb_bound(S, dinv, R, zs, m, c0):
    kmax = int(np.diff(S.indptr).max())
    return C_CHEB * (m + 1) * (kmax + 8) * EPS * (np.linalg.norm(zs.astype(np.float64), axis=0)
                                                  + c0 * np.linalg.norm(dinv[:, None] * R, axis=0))


def cheb_ratio(Z, zs, bound):
    return np.linalg.norm((Z.astype(LD) - zs).astype(np.float64), axis=0) / bound


def cheb_degree(m):
    return min(max(m, 1), 32)            # LSB_CHEB_MAX


# ---- FSAI ----------------------------------------------------------------------------------------
def fsai_pattern(S, power):
    lib = _lib.load()
    A = as_matrix(S)
    T = lib.lsb_csr_fsai_pattern(A.ptr, power, 128)
    assert T
    t = T.contents
    n = S.shape[0]
    offs = np.ctypeslib.as_array(t.offs, (n + 1,)).astype(np.int64)
    cols = np.ctypeslib.as_array(t.cols, (max(int(t.nnz), 1),))[:int(t.nnz)].astype(np.int64)
    lib.lsb_fsai_pattern_free(T)
    return offs, cols


_FSAI_REF = {}


def fsai_reference(key, S, power):
    """(pattern offsets, columns, rows, row lengths, G* in np.longdouble, G by float64 Cholesky, cond_2 per row)"""
    if key not in _FSAI_REF:
        _FSAI_REF[key] = _fsai_reference(S, power)
    return _FSAI_REF[key]


def _fsai_reference(S, power):
    n = S.shape[0]
    offs, cols = fsai_pattern(S, power)
    mi = np.diff(offs)
    assert (cols[offs[1:] - 1] == np.arange(n)).all()
    Sd = S.toarray()
    gs, g64 = np.zeros(len(cols), LD), np.zeros(len(cols))
    cond = np.zeros(n)
    for m in np.unique(mi):
        rows = np.nonzero(mi == m)[0]
        for c0 in range(0, len(rows), 256):
            rr = rows[c0:c0 + 256]
            at = offs[rr][:, None] + np.arange(m)[None, :]
            J = cols[at]
            stack = Sd[J[:, :, None], J[:, None, :]]
            e = np.zeros((len(rr), m, 1))
            e[:, -1, 0] = 1.0
            y = exact_solve(stack, e)[:, :, 0]
            gs[at] = y / np.sqrt(y[:, -1:])
            cond[rr] = spd_cond(stack)[0]
            # the product's way in float64: Cholesky, L u = e_last (u = e_last / L_mm), L^T y = u, scale
            Lc = np.linalg.cholesky(stack)
            u = e / Lc[:, -1:, -1:]
            y6 = np.linalg.solve(np.swapaxes(Lc, 1, 2), u)[:, :, 0]
            g64[at] = y6 / np.sqrt(y6[:, -1:])
    rows = np.repeat(np.arange(n), mi)
    return offs, cols, rows, mi, gs, g64, cond


def fsai_exact(ref, R):
    """(z*, beta) per right-hand side"""
    offs, cols, rows, mi, gs, g64, cond = ref
    n = len(mi)
    Rl = R.astype(LD)
    t, z = np.zeros(R.shape, LD), np.zeros(R.shape, LD)
    np.add.at(t, rows, gs[:, None] * Rl[cols])
    np.add.at(z, cols, gs[:, None] * t[rows])
    aG = sp.csr_matrix((abs(gs).astype(np.float64), cols, offs), shape=(n, n))
    Pm = sp.csr_matrix((np.ones(len(cols)), cols, offs), shape=(n, n))
    gn = np.sqrt(np.add.reduceat((gs * gs).astype(np.float64), offs[:-1]))
    cj = np.bincount(cols, minlength=n)
    rho = C_FSAI * mi * EPS * cond
    rJ = np.sqrt(Pm @ (R * R))
    tau = (rho * gn)[:, None] * rJ + ((mi + 1) * EPS)[:, None] * (aG @ abs(R))
    at = abs(t).astype(np.float64)
    beta = aG.T @ tau + Pm.T @ ((rho * gn)[:, None] * at) + ((cj + 1) * EPS)[:, None] * (aG.T @ at)
    return z, beta


def fsai_ratio(Z, zs, beta):
    err = abs(Z.astype(LD) - zs).astype(np.float64)
    assert (err[beta == 0.0] == 0.0).all()
    return np.where(beta > 0, err / np.where(beta > 0, beta, 1.0), 0.0).max(axis=0)


def fsai_fp64(ref, R):
    offs, cols, rows, mi, gs, g64, cond = ref
    n = len(mi)
    G = sp.csr_matrix((g64, cols, offs), shape=(n, n))
    return G.T.tocsr() @ (G @ R)


def fsai_setup(case, matrix_path):
    name, power = case
    S, A, kw = operator(name, matrix_path)
    n = S.shape[0]
    R = rhs3(n, n - 1 - n // 7)
    ref = fsai_reference((name, power), S, power)
    return S, A, kw, R, ref


# ---- CPU: the bounds against float64 restatements ------------------------------------------------
def _report(what, worst):
    print("%s: worst error / bound %.3g at %s" % (what, worst[0], worst[1]))


@pytest.mark.parametrize("kind", ["bj", "cheb", "fsai"])
def test_bounds_hold_for_fp64_restatements(kind, matrix_path):
    """Every bound, on the inputs of every GPU case, against a float64 numpy restatement of the product's
    algorithm: within 1/4 of the bound, and the worst ratio not under 1/16 (a bound far above what float64
    does would let a real defect through)."""
    worst = (0.0, None)
    if kind == "bj":
        restated = {}
        for case in BJ_CASES:
            S, A, kw, bs, R, Rp, pmap, bounds, ref = bj_setup(case, matrix_path)
            key = (case[0], min(bs, S.shape[0])) + case[2:]   # (block sizes n and 1 << 20: the same inputs)
            if key not in restated:
                Z = np.zeros_like(Rp)
                for first, stack in bj_groups(S, bounds, min(bs, S.shape[0])):
                    m = stack.shape[1]
                    X = gauss_jordan(stack)
                    Z[_rows_of(first, m)] = np.einsum("kji,kjc->kic", X, Rp[_rows_of(first, m)])
                restated[key] = Z
            ratio = bj_ratio(ref, restated[key])
            print("bj", case, ratio)
            assert (ratio <= RESTATED_WITHIN).all(), (case, ratio)
            if ratio.max() > worst[0]:
                worst = (ratio.max(), (case, RNAMES[int(ratio.argmax())]))
    elif kind == "cheb":
        seen = set()
        for name, _, _ in CHEB_CONFIGS:
            if name in seen:
                continue
            seen.add(name)
            S, A, kw = operator(name, matrix_path)
            n = S.shape[0]
            dinv = 1.0 / S.diagonal()
            R = rhs3(n, n - 1 - n // 7)
            lmax = power_lmax(S, dinv)
            for deg in CHEB_DEGREES:
                m = cheb_degree(deg)
                c0, a, b = cheb_coeffs(m, lmax / max(30.0, 16.0 * m * m), lmax)
                zs = cheb_apply(S, dinv, R, c0, a, b, LD)
                ratio = cheb_ratio(cheb_apply(S, dinv, R, c0, a, b, np.float64), zs, cheb_bound(S, dinv, R, zs, m, c0))
                print("cheb", name, deg, ratio)
                assert (ratio <= RESTATED_WITHIN).all(), (name, deg, ratio)
                if ratio.max() > worst[0]:
                    worst = (ratio.max(), (name, deg, RNAMES[int(ratio.argmax())]))
    else:
        for case in FSAI_CASES:
            S, A, kw, R, ref = fsai_setup(case, matrix_path)
            zs, beta = fsai_exact(ref, R)
            ratio = fsai_ratio(fsai_fp64(ref, R), zs, beta)
            print("fsai", case, ratio, "||beta|| / ||z*||",
                  np.linalg.norm(beta, axis=0) / np.linalg.norm(zs.astype(np.float64), axis=0))
            assert (ratio <= RESTATED_WITHIN).all(), (case, ratio)
            if ratio.max() > worst[0]:
                worst = (ratio.max(), (case, RNAMES[int(ratio.argmax())]))
    _report(kind, worst)
    assert worst[0] >= RESTATED_WITHIN / 4, "the constant of this bound is too generous: %r" % (worst,)


def test_fsai_cases_reach_both_size_classes_and_the_cap(matrix_path):
    """Rows of G go by a wavefront up to 32 entries and by a workgroup beyond, and are cut at 128: the
    cases together hold a row of 1, of exactly 32, of exactly 33 and of 128 entries."""
    sizes = set()
    for name, power in FSAI_CASES:
        offs, _ = fsai_pattern(operator(name, matrix_path)[0], power)
        sizes |= set(np.diff(offs).tolist())
    assert {1, 32, 33, 128} <= sizes and max(sizes) == 128


def test_references_solve_what_they_say(matrix_path):
    """The references themselves: the refined block solves leave a residual at the level of np.longdouble,
    and the np.longdouble recurrence is the Chebyshev polynomial it claims to be -- on a diagonal operator
    z_i = (1 - T_m+1((theta - l_i) / delta) / T_m+1(theta / delta)) r_i / l_i in closed form."""
    S = operator("xn3b_A_18", matrix_path)[0]
    n = S.shape[0]
    R = rhs3(n, n - 1)
    for bs in (8, 200):
        for first, stack in bj_groups(S, np.array([0, n]), bs):
            m = stack.shape[1]
            Rb = R[_rows_of(first, m)]
            y = exact_solve(stack, Rb)
            res = np.abs(Rb.astype(LD) - _matmul_ld(stack, y)).astype(np.float64)
            scale = np.matmul(abs(stack), abs(y).astype(np.float64)) + abs(Rb)
            assert (res <= 4 * m * float(np.finfo(LD).eps) * scale).all()
    lam = np.linspace(0.02, 1.9, 97)
    D = sp.diags(lam).tocsr()
    r = rhs3(97, 5)
    for m in (1, 2, 3, 4, 7, 32):
        lmax = 2.0
        lmin = lmax / max(30.0, 16.0 * m * m)
        c0, a, b = cheb_coeffs(m, lmin, lmax)
        z = cheb_apply(D, np.ones(97), r, c0, a, b, LD).astype(np.float64)
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        Tm = lambda x: np.polynomial.chebyshev.chebval(x, [0.0] * (m + 1) + [1.0])   # d_0 is a step too
        want = (1.0 - Tm((theta - lam) / delta) / Tm(theta / delta)) / lam
        assert abs(z - want[:, None] * r).max() <= 1e-11 * abs(want).max()


# ---- GPU -----------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def apply_twice(s, R):
    """z = M^-1 r for every column of R through precond_dev into a NaN-filled buffer: no NaN left, and a
    second application gives the same bits"""
    import torch
    n = R.shape[0]
    Z = np.empty_like(R)
    for c in range(R.shape[1]):
        d_r = _dev(R[:, c])
        d_z = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        s.precond_dev(d_r, d_z)
        z1 = d_z.cpu().numpy()
        d_z.fill_(float("nan"))
        s.precond_dev(d_r, d_z)
        z2 = d_z.cpu().numpy()
        assert not np.isnan(z1).any() and np.isfinite(z1).all()
        assert np.array_equal(z1, z2)
        Z[:, c] = z1
    return Z


def _opts(hip, kw, **more):
    o = dict(kw)
    o.update(more)
    for k in ("spmv_variant", "precision", "comm"):
        if isinstance(o.get(k), str):
            o[k] = getattr(hip, o[k])
    return hip.default_opts(**o)


def _to_padded(Z, zs_p, pmap):
    """the device's z in the padded numbering; the pad rows, which precond_dev does not hand out, as exact"""
    Zp = zs_p.copy()
    Zp[pmap >= 0] = Z[pmap[pmap >= 0]]
    return Zp


def _bj_device(hip, monkeypatch, case, matrix_path):
    name, _, nvirt, pad = case
    S, A, kw, bs, R, Rp, pmap, bounds, ref = bj_setup(case, matrix_path)
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1" if pad else "0")
    s = hip.Solver(A, _opts(hip, kw, precond=hip.PRECOND_BLOCKJACOBI, block_size=bs, nvirt=nvirt))
    assert bool(s.padded) == bool(pad) and s.n_local == R.shape[0]
    assert s.comm_plan["shards_in_process"] == len(bounds) - 1
    Z = apply_twice(s, R)
    if pad:
        zs_p = np.zeros(Rp.shape)
        for first, m, zs, f, Rb in ref:
            zs_p[_rows_of(first, m)] = zs.astype(np.float64)
        assert (zs_p[pmap < 0] == 0.0).all()          # the pad rows couple only among themselves
        Z = _to_padded(Z, zs_p, pmap)
    return s, Z, ref, R


@pytest.mark.gpu
@pytest.mark.parametrize("case", BJ_CASES,
                         ids=lambda c: "%s-bs%s-nvirt%d%s" % (c[0], c[1], c[2], "-padded" if c[3] else ""))
def test_hip_block_jacobi_apply(hip, monkeypatch, case, matrix_path):
    """k_gj_rowcol / k_gj_update at set-up, k_bj_apply (blocks up to 64 rows) or k_bj_apply_part + k_bj_sum
    (column chunks of 128) per application: every block within its bound of the exact B_k^-1 r_k -- short last
    blocks, chunks wholly past one, a block size above n, blocks restarting at shard boundaries, the
    grid-stride loops, the padded numbering."""
    s, Z, ref, R = _bj_device(hip, monkeypatch, case, matrix_path)
    s.destroy()
    ratio = bj_ratio(ref, Z)
    print("block-Jacobi %r: error / bound %s" % (case, ratio))
    assert (ratio <= 1.0).all(), (case, ratio)


def _cheb_device(hip, monkeypatch, config, deg, matrix_path):
    name, okw, env = config
    S, A, kw = operator(name, matrix_path)
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    monkeypatch.delenv("LSBENCH_HIP_CHEB_FUSE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o = dict(kw)
    o.update(okw)
    s = hip.Solver(A, _opts(hip, o, precond=hip.PRECOND_CHEBYSHEV, cheb_degree=deg))
    return S, s


def _cheb_key(c):
    return c[0] + ("|" + c[1]["precision"] if "precision" in c[1] else "") + \
        ("|nvirt%d" % c[1]["nvirt"] if "nvirt" in c[1] else "")


@pytest.mark.gpu
@pytest.mark.parametrize("deg", CHEB_DEGREES)
@pytest.mark.parametrize("name", sorted(set(_cheb_key(c) for c in CHEB_CONFIGS)))
def test_hip_chebyshev_apply(hip, monkeypatch, name, deg, matrix_path):
    """k_cheb_first / k_cheb_step and the CHEB epilogue of k_spmv_sell16 against the np.longdouble recurrence
    on the device's own interval; the interval against a numpy power iteration; the steps in the epilogue
    and as launches of their own bit for bit the same."""
    configs = [c for c in CHEB_CONFIGS if _cheb_key(c) == name]
    m = cheb_degree(deg)
    got = []
    for config in configs:
        S, s = _cheb_device(hip, monkeypatch, config, deg, matrix_path)
        n = S.shape[0]
        dinv = 1.0 / S.diagonal()
        R = rhs3(n, n - 1 - n // 7)
        lmin, lmax = s.cheb_interval
        kept = not config[1].get("reorder") and "LSBENCH_HIP_PAD_LINES" not in config[2]
        assert bool(s.padded) == ("LSBENCH_HIP_PAD_LINES" in config[2]) and s.n_local == n
        if "spmv_variant" in config[1]:
            assert s.spmv_variant == hip.SPMV_SELL
        assert s.comm_plan["shards_in_process"] == config[1].get("nvirt", 1)
        # a degree above LSB_CHEB_MAX is clamped: the interval's ratio is that of degree 32
        assert abs(lmin - lmax / max(30.0, 16.0 * m * m)) <= 2 * EPS * lmin
        if kept:                          # the solver keeps the caller's numbering: the same start vector
            ref = power_lmax(S, dinv)
            print("Chebyshev %r degree %d: lmax %.17g, numpy %.17g, |difference| / (20 n eps lmax) %.3g"
                  % (config, deg, lmax, ref, abs(lmax - ref) / (20 * n * EPS * ref)))
            assert abs(lmax - ref) <= 20 * n * EPS * ref
        Z = apply_twice(s, R)
        s.destroy()
        c0, a, b = cheb_coeffs(m, lmin, lmax)
        zs = cheb_apply(S, dinv, R, c0, a, b, LD)
        ratio = cheb_ratio(Z, zs, cheb_bound(S, dinv, R, zs, m, c0))
        print("Chebyshev %r degree %d: error / bound %s" % (config, deg, ratio))
        assert (ratio <= 1.0).all(), (config, deg, ratio)
        got.append((Z, lmin, lmax))
    for Z, lmin, lmax in got[1:]:         # LSBENCH_HIP_CHEB_FUSE = 0 and 1
        assert (lmin, lmax) == got[0][1:] and np.array_equal(Z, got[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", FSAI_CASES, ids=lambda c: "%s-power%d" % c)
def test_hip_fsai_apply(hip, monkeypatch, case, matrix_path):
    """k_fsai_rows<64> (rows of G up to 32 entries) and <256> (up to the cap of 128), then z = G^T (G r) as two
    SpMVs: every component within beta_j of the exact G*^T G* r."""
    S, A, kw, R, ref = fsai_setup(case, matrix_path)
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    s = hip.Solver(A, _opts(hip, kw, precond=hip.PRECOND_FSAI, fsai_power=case[1]))
    Z = apply_twice(s, R)
    s.destroy()
    zs, beta = fsai_exact(ref, R)
    ratio = fsai_ratio(Z, zs, beta)
    print("FSAI %r: error / bound %s" % (case, ratio))
    assert (ratio <= 1.0).all(), (case, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bj", "cheb", "fsai", "amg"])
def test_hip_preconditioners_are_symmetric_and_definite(hip, monkeypatch, kind, matrix_path):
    """u . M^-1 v = v . M^-1 u within what the bounds of the two applications and the two host dots allow
    (the exact M^-1 is symmetric), and r . M^-1 r > 0."""
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    S, A, kw = operator("xn3b_A_18", matrix_path)
    n = S.shape[0]
    R = rhs3(n, n - 1)[:, :2]
    u, v = R[:, 0], R[:, 1]
    if kind == "bj":
        case = ("xn3b_A_18", 100, 1, 0)
        s, Z, ref, _ = _bj_device(hip, monkeypatch, case, matrix_path)
        Z = Z[:, :2]
        bn = bj_bound_norm(ref)[:2]
        slack = np.linalg.norm(u) * bn[1] + np.linalg.norm(v) * bn[0]
    elif kind == "cheb":
        S, s = _cheb_device(hip, monkeypatch, CHEB_CONFIGS[0], 4, matrix_path)
        Z = apply_twice(s, R)
        dinv = 1.0 / S.diagonal()
        c0, a, b = cheb_coeffs(4, *s.cheb_interval)
        bn = cheb_bound(S, dinv, R, cheb_apply(S, dinv, R, c0, a, b, LD), 4, c0)
        slack = np.linalg.norm(u) * bn[1] + np.linalg.norm(v) * bn[0]
    elif kind == "fsai":
        s = hip.Solver(A, _opts(hip, kw, precond=hip.PRECOND_FSAI, fsai_power=2))
        Z = apply_twice(s, R)
        _, beta = fsai_exact(fsai_reference(("xn3b_A_18", 2), S, 2), R)
        slack = abs(u) @ beta[:, 1] + abs(v) @ beta[:, 0]
    else:
        s = hip.Solver(A, _opts(hip, kw, precond=hip.PRECOND_AMG))
        Z = apply_twice(s, R)
        slack = 1e-12 * np.linalg.norm(u) * np.linalg.norm(Z[:, 1])
    s.destroy()
    slack += (n + 2) * EPS * (abs(u) @ abs(Z[:, 1]) + abs(v) @ abs(Z[:, 0]))
    asym = abs(u @ Z[:, 1] - v @ Z[:, 0])
    print("%s: |u.M^-1 v - v.M^-1 u| / allowed %.3g" % (kind, asym / slack))
    assert asym <= slack
    assert u @ Z[:, 0] > 0 and v @ Z[:, 1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cheb", "bj"])
def test_hip_precond_dev_is_an_apply_not_a_solve_step(hip, monkeypatch, kind, matrix_path):
    """precond_dev between two solves leaves the second one bit for bit the first (block-Jacobi with 100-row
    blocks: the form whose applications skip a block once the residual is small), and after a converged
    solve -- the state no longer RUNNING -- it still writes every element."""
    from oracle import oracle as O
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    S, A, kw = operator("xn3b_A_18", matrix_path)
    n = S.shape[0]
    b = O.rhs(n)
    extra = dict(precond=hip.PRECOND_CHEBYSHEV, cheb_degree=4) if kind == "cheb" else \
        dict(precond=hip.PRECOND_BLOCKJACOBI, block_size=100)
    s = hip.Solver(A, _opts(hip, kw, **extra))
    R = rhs3(n, n - 1)
    Z0 = apply_twice(s, R)                # before any solve
    x1, r1 = s.solve(b)
    assert r1.status == hip.STATUS_CONVERGED
    Z1 = apply_twice(s, R)                # after a converged solve: NaN-filled buffers, checked in apply_twice
    x2, r2 = s.solve(b)
    s.destroy()
    assert np.array_equal(Z0, Z1)
    assert r2.status == r1.status and r2.iters == r1.iters and np.array_equal(x1, x2)


@pytest.mark.gpu
def test_hip_precond_dev_refuses_what_it_does_not_apply(hip, matrix_path):
    """2 for the diagonal preconditioners (applied inside the sweeps, never as a vector) and for a NULL buffer"""
    import torch
    S, A, kw = operator("xn3b_A_18", matrix_path)
    lib = _lib.load()
    d = torch.zeros(S.shape[0], dtype=torch.float64, device="cuda:0")
    for precond in (hip.PRECOND_JACOBI, hip.PRECOND_NONE, hip.PRECOND_L1JACOBI):
        s = hip.Solver(A, _opts(hip, kw, precond=precond))
        assert lib.lsb_hip_solver_precond_dev(s._h, d.data_ptr(), d.data_ptr()) == 2
        assert lib.lsb_hip_solver_cheb_interval(s._h, None, None) == 2
        with pytest.raises(_lib.LsbenchHipError):
            s.precond_dev(d, d)
        s.destroy()
    s = hip.Solver(A, _opts(hip, kw, precond=hip.PRECOND_BLOCKJACOBI, block_size=8))
    assert lib.lsb_hip_solver_precond_dev(s._h, None, d.data_ptr()) == 2
    assert lib.lsb_hip_solver_precond_dev(s._h, d.data_ptr(), None) == 2
    assert lib.lsb_hip_solver_cheb_interval(s._h, None, None) == 2
    s.destroy()
