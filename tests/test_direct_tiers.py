"""The direct solver on a tiered inverse factor (lsb_hip_solver_create_direct; lsb_direct.c, hip_direct_t.hip,
hip_direct_drv.c), for operators whose single skyline W = L^-1 is over the entry budget.

    tiers      the elimination tree cut by subtree size: tier(k) = how many of the thresholds T_i (the smallest integer
               with T_i^m >= n^i) the subtree of k exceeds; rows numbered tier by tier, postorder inside a tier
    factor     W_tt = (L_tt)^-1 as skylines, the blocks of L below the diagonal as C (by rows) and C^T (by columns)
    round      forward y_t = W_tt ((P r)_t - C_t y_<t), backward x_t = W_tt^T (y_t - sum_s>t (C_s^T x_s)_t)

CPU: the surface; the structure of the factor against numpy restatements (tiers, trees, runs, coupling, the symbolic
count, one tier = the single skyline byte for byte); L^-T L^-1 = (P S P^T)^-1 on the small shapes; the rounds in numpy
with the library's arrays under test_direct.test_cpu_precondition's bounds; the symbolic count of a grid the single
skyline refuses; the refusals.  GPU: one application against numpy, the solves, the cross-checks.

Two of the shapes are not what they were taken for.  A0_02x02 is [[1, 1], [1, -1]]: indefinite, so no Cholesky factor
exists (it is ordered and counted here, and is the non-SPD refusal); and with n = 2 the one threshold of two tiers is
2, which no subtree exceeds: one tier.  The tier of one row is lap2d:nx=3,ny=1 (a path: subtrees 1, 2, 3, T_1 = 2)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from oracle import oracle as O
from test_amg import as_matrix, to_scipy
from test_amg_f32 import _relerr
from test_direct import depths, liu, op

A0, DIAG, SINGLE, PATH3 = "A0_02x02", "I1_05x05", "n1", "lap2d:nx=3,ny=1"
G2D, G3D, XN3B, TJ7A = "lap2d:nx=24,ny=20", "lap3d:nx=9,ny=8,nz=7", "xn3b_A_18", "tj7a_A_12"
SHAPES = [PATH3, DIAG, SINGLE, G2D, G3D, XN3B, TJ7A]  # every one SPD; A0 joins where nothing is factorised
SMALL = [PATH3, DIAG, SINGLE, G2D, G3D]               # at most 600 rows
TIERS = [2, 3, 4]
OVER = "lap2d:nx=512,ny=512"  # the smallest of 448^2, 512^2, 576^2, 640^2 whose single skyline is over the budget
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------ inputs and restatements
def operator(name, matrix_path):
    if name == A0:
        S = O.operator_upper(O.matrix_read(matrix_path(A0)))
        return to_scipy(S.offs, S.cols, S.vals)
    return op(name, matrix_path)


def thresholds(n, m):
    """T_1 .. T_(m-1): the smallest integer with T^m >= n^i, in Python's integers"""
    out = []
    for i in range(1, m):
        T = 1
        while T ** m < n ** i:
            T += 1
        out.append(T)
    return out


@functools.lru_cache(maxsize=None)
def _nd(name, matrix_path):
    S = operator(name, matrix_path)
    return S, la.lsb_csr_nd(as_matrix(S))


@functools.lru_cache(maxsize=None)
def _factor(name, matrix_path, tiers):
    """(S, the library's tiered factor as a dict, the blocks in scipy), made once"""
    S, perm = _nd(name, matrix_path)
    T = la.lsb_csr_tiered_inverse(as_matrix(S), perm, tiers)
    assert isinstance(T, dict), T
    return S, T, Blocks(T)


class Blocks:
    """W (block diagonal, n x n), C (n x n, strictly block lower) and C^T (from the library's second copy) as scipy
    CSRs in the tier-major numbering, and the numpy model of one application"""

    def __init__(self, T):
        n, lo = T["n"], T["lo"]
        self.n, self.lo, self.p = n, lo, T["perm"].astype(np.int64)
        first = T["first"].astype(np.int64)
        cols = np.concatenate([np.arange(int(f), k + 1) for k, f in enumerate(first)]) if n else np.zeros(0, int)
        self.W = sp.csr_matrix((T["vals"], cols, T["woff"].astype(np.int64)), shape=(n, n))
        lo1 = int(lo[min(1, T["ntier"])])
        cptr = np.concatenate([np.zeros(lo1, np.int64), T["coffs"].astype(np.int64)])
        self.C = sp.csr_matrix((T["cvals"], T["ccols"].astype(np.int64), cptr), shape=(n, n))
        # C^T: tier t's block has the rows j < lo[t]; stacked into one n x n matrix entry by entry
        rows, at, prev_end = [], 0, 0
        for t in range(1, T["ntier"]):
            offs = T["toffs"][at:at + int(lo[t]) + 1].astype(np.int64)
            rows.append(np.repeat(np.arange(int(lo[t])), np.diff(offs)))
            assert offs[0] == prev_end  # one block after another in tcols / tvals
            prev_end = int(offs[-1])
            at += int(lo[t]) + 1
        self.t_rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        self.Ct = sp.csr_matrix((T["tvals"], (self.t_rows, T["tcols"].astype(np.int64))), shape=(n, n))
        self.tiers = [(int(lo[t]), int(lo[t + 1])) for t in range(T["ntier"])]
        self._ops = {}

    def _pair(self, M, flip):
        """v -> M v with the sums of every row in the stored order, or -- flip -- in the opposite one"""
        if not flip:
            return lambda v: M @ v
        F = M[:, ::-1].tocsr()
        F.sort_indices()
        return lambda v: F @ v[::-1]

    def apply(self, r, flip=False):
        """z = P^T L^-T L^-1 P r by the tiers, every sum in the library's order (or all of them flipped)"""
        key = bool(flip)
        if key not in self._ops:
            ops = []
            for a, b in self.tiers:
                Wt = self.W[a:b, a:b].tocsr()
                Ct = self.C[a:b, :a].tocsr()
                ops.append((self._pair(Wt, flip), self._pair(Ct, flip), self._pair(Wt.T.tocsr(), flip),
                            self._pair(Ct.T.tocsr(), flip)))
            self._ops[key] = ops
        ops = self._ops[key]
        v = r[self.p]
        y, z = np.zeros(self.n), np.zeros(self.n)
        for (a, b), (W, Cf, _, _) in zip(self.tiers, ops):
            y[a:b] = W(v[a:b] - Cf(y[:a])) if a else W(v[a:b])
        for (a, b), (_, _, Wt, Cb) in reversed(list(zip(self.tiers, ops))):
            z[a:b] = Wt(y[a:b])
            if a:
                y[:a] -= Cb(z[a:b])
        out = np.empty(self.n)
        out[self.p] = z
        return out

    def rounds(self, S, b, nrounds):
        x, r, out = np.zeros_like(b), b.copy(), []
        for _ in range(nrounds):
            x = x + self.apply(r)
            r = b - S @ x
            out.append((x, float(np.linalg.norm(r) / np.linalg.norm(b))))
        return out


def rhs(n):
    """b_i = i, the reference's right-hand side; a single row gets 1 (b = 0 has no relative residual)"""
    return O.rhs(n) if n > 1 else np.ones(1)


def reference_x(name, S, b, golden_x):
    """the golden solution where the reference has one, else a sparse LU's"""
    if name in (XN3B, TJ7A, DIAG):
        return golden_x(name)
    return spla.spsolve(S.tocsc(), b) if S.shape[0] > 1 else b / S.toarray()[0]


# ------------------------------------------------------------------------------------ without a GPU
def test_surface():
    assert [f[0] for f in _lib.Opts._fields_][-1] == "amg_cheb_ratio" and list(_lib.Opts._TAIL) == ["fsai_blocks"]
    assert la.DIRECT_MAX_TIERS == 6
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    assert "#define LSB_DIRECT_MAX_TIERS 6" in header
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    for name in ("lsb_csr_tiered_inverse", "lsb_csr_tiered_count", "lsb_tierinv_free", "lsb_hip_solver_create_direct",
                 "lsb_hip_solver_direct_tier_info"):
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name) and name in exported, name
    assert not [s for s in exported if s.startswith("lsb_k_dirt")]  # the launchers stay inside
    assert lib.lsb_hip_solver_direct_tier_info(None, None, None, None, None, None) == 2
    # --direct-tiers: held beside the option table, not in struct lsb_hip_opts
    try:
        assert lib.hip_cdna4_set_option(b"direct-tiers", b"0") == 0
        assert lib.hip_cdna4_set_option(b"direct_tiers", b"6") == 0
        for bad in (b"7", b"-1", b"two", b""):
            assert lib.hip_cdna4_set_option(b"direct-tiers", bad) == 1
    finally:
        assert lib.hip_cdna4_set_option(b"direct-tiers", b"1") == 0
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    assert "--direct-tiers" in subprocess.run([drv, "--help"], capture_output=True, text=True).stdout
    assert thresholds(2, 2) == [2] and thresholds(3, 2) == [2] and thresholds(480, 3) == [8, 62]
    assert thresholds(1 << 20, 4) == [32, 1024, 32768] and thresholds(1, 6) == [1] * 5


@pytest.mark.parametrize("tiers", [1] + TIERS + [6])
@pytest.mark.parametrize("name", SHAPES + [A0])
def test_tiering_and_count(name, tiers, matrix_path):
    """lsb_csr_tiered_count against numpy: the tiers from the subtree sizes, the entries of the W_tt as the depths
    inside a tier, the coupling as the entries of L (row subtrees) that leave their tier.  Nothing is factorised."""
    S, perm = _nd(name, matrix_path)
    n = S.shape[0]
    parent = liu(S, perm)
    size = np.ones(n + 1, np.int64)
    for k in range(n):
        size[parent[k]] += size[k]
    T = thresholds(n, tiers)
    tier = np.array([sum(int(size[k]) > t for t in T) for k in range(n)], np.int64)
    assert all(parent[k] == n or tier[parent[k]] >= tier[k] for k in range(n))
    tdepth = np.zeros(n, np.int64)
    for k in range(n - 1, -1, -1):
        tdepth[k] = 1 + (tdepth[parent[k]] if parent[k] < n and tier[parent[k]] == tier[k] else 0)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    coupling, mark = 0, -np.ones(n, np.int64)
    for k in range(n):
        mark[k] = k
        row = int(perm[k])
        for c in S.indices[S.indptr[row]:S.indptr[row + 1]]:
            i = int(inv[c])
            while i < k and mark[i] != k:
                mark[i] = k
                coupling += int(tier[i] != tier[k])
                i = int(parent[i])
    got = la.lsb_csr_tiered_count(as_matrix(S), perm, tiers)
    print(name, "n", n, "tiers", tiers, "thresholds", T, "rows per tier", np.bincount(tier).tolist(), "count", got)
    assert got == (int(tdepth.sum()), coupling, int(depths(parent).max()))
    if tiers == 1:
        assert got[:1] + got[2:] == la.lsb_csr_skyline_count(as_matrix(S), perm) and coupling == 0
    assert la.lsb_csr_tiered_count(as_matrix(S), perm, 0) is None
    assert la.lsb_csr_tiered_count(as_matrix(S), perm, la.DIRECT_MAX_TIERS + 1) is None
    if n > 1:
        bad = perm.copy()
        bad[0] = bad[1]
        assert la.lsb_csr_tiered_count(as_matrix(S), bad, tiers) is None


@pytest.mark.parametrize("tiers", TIERS)
@pytest.mark.parametrize("name", SHAPES)
def test_structure(name, tiers, matrix_path):
    S, T, B = _factor(name, matrix_path, tiers)
    n, lo, nt = T["n"], T["lo"], T["ntier"]
    p = T["perm"].astype(np.int64)
    assert sorted(p.tolist()) == list(range(n))
    assert 1 <= nt <= tiers and lo[0] == 0 and lo[-1] == n and (np.diff(lo) > 0).all()
    tier = np.repeat(np.arange(nt), np.diff(lo))
    # the tree of the tier-major order climbs, tiers never decrease towards the root, and they follow the rule
    parent = liu(S, p)
    assert (parent > np.arange(n)).all()
    size = np.ones(n + 1, np.int64)
    for k in range(n):
        size[parent[k]] += size[k]
    raw = np.array([sum(int(size[k]) > t for t in thresholds(n, tiers)) for k in range(n)], np.int64)
    assert (np.diff(raw) >= 0).all() and (np.unique(raw, return_inverse=True)[1] == tier).all()  # empty tiers dropped
    up = np.where(parent < n, parent, 0)
    assert (tier[up][parent < n] >= tier[parent < n]).all()
    same = (parent < n) & (tier[up] == tier)
    assert (T["parent"] == np.where(same, parent, n)).all()
    # the skylines: the part of a subtree inside its tier, a run that ends at k; runs nest or abut inside a tier
    tsize = np.ones(n, np.int64)
    for k in range(n):
        if same[k]:
            tsize[parent[k]] += tsize[k]
    first = T["first"].astype(np.int64)
    assert (first == np.arange(n) + 1 - tsize).all() and (first >= lo[tier]).all()
    assert (np.diff(T["woff"].astype(np.int64)) == tsize).all()
    for k in range(1, n):
        if tier[k] == tier[k - 1] and first[k] < k:
            assert first[k] <= first[k - 1]
    run_end = np.arange(n)
    for k in range(n - 2, -1, -1):
        if T["parent"][k] == k + 1:
            run_end[k] = run_end[k + 1]
    assert (T["run_end"] == run_end).all() and (tier[run_end] == tier).all()
    # the coupling: rows of the tiers >= 1 only, columns ascending below the row's tier; C^T its transpose bit for bit
    C_, Ct = B.C, B.Ct
    assert C_.indptr[int(lo[min(1, nt)])] == 0 and len(T["coffs"]) == n - int(lo[min(1, nt)]) + 1
    for i in range(n):
        c = C_.indices[C_.indptr[i]:C_.indptr[i + 1]]
        assert (np.diff(c) > 0).all() and (c < lo[tier[i]]).all()
    assert (tier[T["tcols"].astype(np.int64)] > tier[B.t_rows]).all() if len(B.t_rows) else True
    at = 0
    for t in range(1, nt):  # tier t's block of C^T: its rows ascend inside tier t
        offs = T["toffs"][at:at + int(lo[t]) + 1].astype(np.int64)
        for j in range(int(lo[t])):
            r = T["tcols"][offs[j]:offs[j + 1]].astype(np.int64)
            assert (np.diff(r) > 0).all() and (r >= lo[t]).all() and (r < lo[t + 1]).all()
        at += int(lo[t]) + 1
    assert at == len(T["toffs"])
    X, Y = C_.T.tocsr(), Ct.tocsr()
    X.sort_indices(), Y.sort_indices()
    assert (X.indptr == Y.indptr).all() and (X.indices == Y.indices).all() and X.data.tobytes() == Y.data.tobytes()
    # the coupling is L itself: L_tt = W_tt^-1 on the diagonal, C below, and L L^T = P S P^T
    count = la.lsb_csr_tiered_count(as_matrix(S), _nd(name, matrix_path)[1], tiers)
    print(name, "n", n, "tiers asked", tiers, "got", nt, "lo", lo.tolist(), "W entries", int(T["woff"][-1]),
          "coupling", C_.nnz, "count", count)
    assert count[:2] == (int(T["woff"][-1]), C_.nnz) == (int(T["woff"][-1]), len(T["cvals"]))
    if name == PATH3 and tiers == 2:
        assert lo.tolist() == [0, 2, 3]  # a tier of one row
    if name in (DIAG, SINGLE):
        assert nt == 1 and C_.nnz == 0  # the tiers asked for collapse


@pytest.mark.parametrize("name", SHAPES)
def test_one_tier_is_the_single_skyline(name, matrix_path):
    S, perm = _nd(name, matrix_path)
    W = la.lsb_csr_skyline_inverse(as_matrix(S), perm)
    T = la.lsb_csr_tiered_inverse(as_matrix(S), perm, 1)
    assert T["ntier"] == 1 and T["lo"].tolist() == [0, S.shape[0]]
    for k in ("perm", "first", "woff", "vals", "parent", "run_end"):
        assert W[k].tobytes() == T[k].tobytes(), k
    assert len(T["ccols"]) == len(T["cvals"]) == len(T["tcols"]) == len(T["tvals"]) == 0
    assert T["coffs"].tolist() == [0] and len(T["toffs"]) == 0


@pytest.mark.parametrize("tiers", TIERS)
@pytest.mark.parametrize("name", SMALL)
def test_exactness(name, tiers, matrix_path):
    """L^-1 assembled densely from the tiers (the forward substitution on the identity), L^-T L^-1 against
    inv(P S P^T).  The bound: these operators have a condition number below 500 and at most 504 rows, and
    500 * 504 * 2^-52 = 6e-11 <= 1e-10, the figure test_direct.test_skyline_inverse allows the single skyline."""
    S, T, B = _factor(name, matrix_path, tiers)
    n = T["n"]
    Wd, Cd = B.W.toarray(), B.C.toarray()
    Linv = np.zeros((n, n))
    for a, b in B.tiers:
        Linv[a:b] = Wd[a:b, a:b] @ (np.eye(n)[a:b] - Cd[a:b, :a] @ Linv[:a])
    assert not np.triu(Linv, 1).any()
    Binv = np.linalg.inv(S[B.p][:, B.p].toarray())
    err = np.abs(Linv.T @ Linv - Binv).max() / np.abs(Binv).max()
    print(name, "n", n, "tiers", T["ntier"], "max |L^-T L^-1 - inv(P S P^T)| / max |inv|", err, "cond",
          np.linalg.cond(S.toarray()))
    assert err <= 1e-10


@pytest.mark.parametrize("tiers", TIERS)
@pytest.mark.parametrize("name", SHAPES)
def test_rounds_in_numpy(name, tiers, matrix_path, golden_x):
    """test_direct.test_cpu_precondition's bounds on the tiered factor: with the library's arrays in numpy on b_i = i,
    round 1 has a recomputed relres <= 1e-11, round 2 <= 1e-12, x is within 1e-10 of the reference solution."""
    S, T, B = _factor(name, matrix_path, tiers)
    b = rhs(S.shape[0])
    xr = reference_x(name, S, b, golden_x)
    (x1, r1), (x2, r2) = B.rounds(S, b, 2)
    e1, e2 = _relerr(x1, xr), _relerr(x2, xr)
    print(name, "n", S.shape[0], "tiers", T["ntier"], "relres after round 1, 2:", r1, r2, "x against the reference:",
          e1, e2)
    assert r1 <= 1e-11 and r2 <= 1e-12 and e1 <= 1e-10 and e2 <= 1e-10


def test_over_the_budget_symbolic():
    """The smallest of the grids 448^2, 512^2, 576^2, 640^2 that --krylov direct refuses today.  The lower bound of
    lsb_csr_nd_bounded trips on none of the four (7.2e7, 1.08e8, 1.54e8, 2.12e8 against 2^28 = 2.68e8); what refuses
    is the count of the finished ordering, lsb_csr_skyline_count: 2.22e8 at 448^2 (inside), 3.32e8 at 512^2.  For
    512^2 some number of tiers <= DIRECT_MAX_TIERS fits, by the symbolic count alone: nothing is factorised."""
    A = la.lsbench_matrix_synth(OVER)
    small = la.lsbench_matrix_synth("lap2d:nx=448,ny=448")
    assert la.lsb_csr_skyline_count(small, la.lsb_csr_nd(small))[0] <= _lib.DIRECT_MAX_ENTRIES
    perm = la.lsb_csr_nd(A)
    single = la.lsb_csr_skyline_count(A, perm)[0]
    assert single > _lib.DIRECT_MAX_ENTRIES
    fits = None
    for m in range(1, la.DIRECT_MAX_TIERS + 1):
        w, c, h = la.lsb_csr_tiered_count(A, perm, m)
        print(OVER, "tiers", m, "W entries", w, "coupling", c, "budgeted", w + 3 * c, "height", h)
        if fits is None and w + 3 * c <= _lib.DIRECT_MAX_ENTRIES:
            fits = m
        assert m > 1 or (w, c) == (single, 0)
    assert fits is not None and 2 <= fits <= la.DIRECT_MAX_TIERS


def test_refusals(matrix_path):
    S, perm = _nd(A0, matrix_path)  # [[1, 1], [1, -1]]
    for tiers in (0, 1, 2, 6):
        assert la.lsb_csr_tiered_inverse(as_matrix(S), perm, tiers) == 1  # not positive definite
    ok, pk = _nd(PATH3, matrix_path)
    assert la.lsb_csr_tiered_inverse(as_matrix(ok), pk, la.DIRECT_MAX_TIERS + 1) == 3
    assert la.lsb_csr_tiered_inverse(as_matrix(ok), np.array([0, 0, 1], np.uint32), 2) == 3  # no permutation
    auto = la.lsb_csr_tiered_inverse(as_matrix(ok), pk, 0)
    assert auto["ntier"] == 1  # the fewest that fit
    lib = _lib.load()
    o = la.default_opts(krylov=la.KRYLOV_DIRECT, op_mode=la.OP_RAW)
    for tiers in (-1, la.DIRECT_MAX_TIERS + 1):
        assert not lib.lsb_hip_solver_create_direct(as_matrix(ok).ptr, C.byref(o), tiers)
    o = la.default_opts(krylov=la.KRYLOV_PCG, op_mode=la.OP_RAW)
    assert not lib.lsb_hip_solver_create_direct(as_matrix(ok).ptr, C.byref(o), 2)


# ------------------------------------------------------------------------------------ on the GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")


def _solver(hip, name, matrix_path, tiers, **kw):
    kw.setdefault("op_mode", hip.OP_RAW)
    kw.setdefault("krylov", hip.KRYLOV_DIRECT)
    return hip.Solver.create_direct(as_matrix(operator(name, matrix_path)), hip.default_opts(**kw), tiers)


def _solve_dev(s, b, d_x=None, warm=False):
    d_x = _nan(len(b)) if d_x is None else d_x
    res = s.solve_dev(_dev(b), d_x, warm=True) if warm else s.solve_dev(_dev(b), d_x)
    return d_x.cpu().numpy(), res


@pytest.mark.gpu
@pytest.mark.parametrize("tiers", TIERS)
@pytest.mark.parametrize("name", SHAPES)
def test_one_application(hip, name, tiers, matrix_path, monkeypatch):
    """precond_dev against the numpy model on the same arrays, with the windows of k_dirt_rows staged (as dealt) and
    with at most 16 doubles staged, so that the wider windows are gathered.  The bound is test_direct's: four times
    what numpy itself moves between two summation orders, and no less than four units of fp64 rounding."""
    S, T, B = _factor(name, matrix_path, tiers)
    n = S.shape[0]
    r = np.sin(np.arange(n, dtype=np.float64)) + 0.5
    za, zb = B.apply(r), B.apply(r, flip=True)
    lens = np.arange(n) - T["first"].astype(np.int64) + 1
    out = []
    for cap in (None, 16):
        if cap:
            monkeypatch.setenv("LSBENCH_HIP_DIRECT_TIER_LDS", str(cap))
            if n >= 400:
                assert lens.max() > cap  # a row alone is wider than what is staged: gathered
        s = _solver(hip, name, matrix_path, tiers)
        info = s.direct_tier_info()
        assert info[0] == T["ntier"] and info[1] == int(T["woff"][-1]) and info[2] == len(T["cvals"])
        for _ in range(2):
            z = _nan(n)
            s.precond_dev(_dev(r), z)
            out.append(z.cpu().numpy())
        s.destroy()
    e_np, e_gpu = _relerr(zb, za), _relerr(out[0], za)
    bound = 4.0 * max(e_np, EPS)
    print(name, "n", n, "tiers", T["ntier"], "device against numpy", e_gpu, "numpy between two orders", e_np, "bound",
          bound)
    assert np.isfinite(out[0]).all()
    assert out[0].tobytes() == out[1].tobytes() == out[2].tobytes() == out[3].tobytes()  # staged = gathered, run = run
    assert bound <= 1e-13 and e_gpu <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("tiers", TIERS)
@pytest.mark.parametrize("name", SHAPES)
def test_solves(hip, name, tiers, matrix_path, golden_x):
    S = operator(name, matrix_path)
    n = S.shape[0]
    b = rhs(n)
    xr = reference_x(name, S, b, golden_x)
    got = []
    for graph in (1, 0):
        s = _solver(hip, name, matrix_path, tiers, tol=1e-12, maxit=10, use_graph=graph)
        x, res = _solve_dev(s, b)
        x2, res2 = _solve_dev(s, b)  # (the hinted solve)
        xh, resh = s.solve(b)        # host buffers
        s.destroy()
        true = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
        print(name, "tiers", tiers, "graph", graph, "rounds", res.iters, "relres", res.relres, "on the CPU", true,
              "reference", _relerr(x, xr))
        assert res.status == hip.STATUS_CONVERGED and res.iters <= 2 and res.relres <= 1e-12
        assert res.true_relres == res.relres and res.spmvs == res.iters
        assert true <= 1e-12 * (1 + 1e-3) and _relerr(x, xr) <= 1e-10
        for xx, rr in ((x2, res2), (np.asarray(xh), resh)):
            assert xx.tobytes() == x.tobytes()
            assert (rr.status, rr.iters, rr.spmvs, rr.relres) == (res.status, res.iters, res.spmvs, res.relres)
        got.append((x, res))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].relres == got[1][1].relres  # graphs = launches
    s = _solver(hip, name, matrix_path, tiers, tol=1e-10, maxit=10)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters) == (hip.STATUS_CONVERGED, 1) and res.relres <= 1e-10
    # the reference's direct protocol: one round, nothing recomputed, no residual launch
    s = _solver(hip, name, matrix_path, tiers, tol=0.0, maxit=1)
    x, res = _solve_dev(s, b)
    x2, res2 = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters, res.relres, res.spmvs) == (hip.STATUS_MAXIT, 1, -1.0, 0)
    assert _relerr(x, xr) <= 1e-10 and x2.tobytes() == x.tobytes()
    s = _solver(hip, name, matrix_path, tiers, tol=1e-12, maxit=0)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters) == (hip.STATUS_MAXIT, 0) and not x.any()


@pytest.mark.gpu
def test_cross_checks(hip, matrix_path, golden_x):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    S, T, B = _factor(XN3B, matrix_path, 3)
    n = S.shape[0]
    b = rhs(n)
    one = hip.Solver(as_matrix(S), hip.default_opts(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_DIRECT, tol=1e-12, maxit=10))
    x1, r1 = _solve_dev(one, b)
    assert one.direct_tier_info() == (1, one.direct_info[0], 0, [n], 2)
    one.destroy()
    same = _solver(hip, XN3B, matrix_path, 1, tol=1e-12, maxit=10)  # tiers = 1 is lsb_hip_solver_create
    xs, rs = _solve_dev(same, b)
    assert same.direct_tier_info()[0] == 1 and xs.tobytes() == x1.tobytes()
    same.destroy()
    s = _solver(hip, XN3B, matrix_path, 3, tol=1e-12, maxit=10)
    x3, r3 = _solve_dev(s, b)
    print("tiered against the single skyline", _relerr(x3, x1))
    assert r3.status == hip.STATUS_CONVERGED and _relerr(x3, x1) <= 1e-10
    nt, w, c, rows, launches = s.direct_tier_info()
    assert (nt, w, c, rows, launches) == (T["ntier"], int(T["woff"][-1]), len(T["cvals"]),
                                          np.diff(T["lo"]).tolist(), 4 * T["ntier"] - 2)
    entries, height, by = s.direct_info
    assert entries == w and height == int(depths(liu(S, T["perm"].astype(np.int64))).max())
    assert by == 16 * w + 24 * c + 104 * n
    # a warm start from the solution: at most one round
    x, res = _solve_dev(s, b, _dev(golden_x(XN3B)), warm=True)
    assert s.start_relres(1)[0] <= 1e-12 and res.status == hip.STATUS_CONVERGED and res.iters <= 1
    # a sequence runs
    s.seq_begin(2)
    for k in range(3):
        xq, rq = s.solve_seq(b * (1.0 + 0.25 * k))
        assert rq.status == hip.STATUS_CONVERGED and _relerr(xq, x1 * (1.0 + 0.25 * k)) <= 1e-10
    s.seq_begin(0)
    # blocks of right-hand sides are not for tiered solvers
    d_B = _dev(np.tile(b, (2, 1)))
    d_X = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda:0")
    res2 = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_direct_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res2) == 2
    assert lib.lsb_hip_solver_direct_apply_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_direct_multi_round_bytes(s._h, 2) == 0
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all())
    s.destroy()
    j = hip.Solver(as_matrix(S), hip.default_opts(op_mode=hip.OP_RAW))
    assert j.direct_tier_info() is None
    j.destroy()


ONE_TIER = ["lap2d:nx=12,ny=9", XN3B]  # 108 rows and 3461: one tier fits both


def _one_tier_opts(hip, **kw):
    return hip.default_opts(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_DIRECT, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ONE_TIER)
def test_one_tier_is_one_solver(hip, name, matrix_path):
    """lsb_hip_solver_create, create_direct(.., 1) and create_direct(.., 0) on an operator that fits one tier are the
    same solver: the same figures, the same bytes of x and of one application, served alike by the block entry points
    of the single skyline."""
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    S = operator(name, matrix_path)
    n = S.shape[0]
    b = rhs(n)
    B = np.stack([b, b + 1.0])
    r = np.sin(np.arange(n, dtype=np.float64)) + 0.5
    got = []
    for how in ("create", 1, 0):
        rec = {}
        for key, kw in (("tol", dict(tol=1e-12, maxit=10)), ("one", dict(tol=0.0, maxit=1))):
            o = _one_tier_opts(hip, **kw)
            s = hip.Solver(as_matrix(S), o) if how == "create" else hip.Solver.create_direct(as_matrix(S), o, how)
            rec["info"] = s.direct_info
            assert s.direct_tier_info() == (1, rec["info"][0], 0, [n], 2)
            assert rec["info"][2] == 16 * rec["info"][0] + 56 * n
            rec["bytes"] = [s.direct_multi_round_bytes(k) for k in (2, 4, 8)]
            assert rec["bytes"] == [16 * rec["info"][0] + (24 + 32 * k) * n for k in (2, 4, 8)]
            x, res = _solve_dev(s, b)
            rec[key] = [x.tobytes()]
            d_X = torch.full((2, n), float("nan"), dtype=torch.float64, device="cuda:0")
            res2 = (_lib.Result * 2)()
            assert lib.lsb_hip_solver_solve_direct_multi_dev(s._h, 2, _ptr(_dev(B)), n, _ptr(d_X), n, res2) == 0
            X = d_X.cpu().numpy()
            assert X[0].tobytes() == x.tobytes()
            x1, _ = _solve_dev(s, B[1])
            assert X[1].tobytes() == x1.tobytes()
            rec[key].append(X.tobytes())
            if key == "tol":
                assert res.status == hip.STATUS_CONVERGED and res2[0].status == res2[1].status == hip.STATUS_CONVERGED
                z = _nan(n)
                s.precond_dev(_dev(r), z)
                rec["z"] = z.cpu().numpy().tobytes()
                assert np.isfinite(z.cpu().numpy()).all()
            s.destroy()
        got.append(rec)
    for rec in got[1:]:
        assert rec == got[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ONE_TIER)
def test_one_tier_gathered_is_staged(hip, name, matrix_path, monkeypatch, capfd):
    """The gathered windows of the one-tier solver on small shapes: with at most 16 doubles of a window staged
    (LSBENCH_HIP_DIRECT_TIER_LDS at creation), one application has the bytes it has with every window staged -- at one
    column and through lsb_hip_solver_direct_apply_multi_dev at widths 2 and 8.  That the knob took hold is read off the
    verbose line of the upload ("windows of up to %u doubles in LDS"): without it a window wider than 16 doubles is staged,
    with it none is."""
    import re
    import torch
    S = operator(name, matrix_path)
    n = S.shape[0]
    i = np.arange(n, dtype=np.float64)
    R = np.stack([np.sin(i + 0.37 * c) + 0.5 for c in range(8)])
    out, staged = [], []
    monkeypatch.delenv("LSBENCH_HIP_DIRECT_TIER_LDS", raising=False)
    for cap in (None, 16):
        if cap:
            monkeypatch.setenv("LSBENCH_HIP_DIRECT_TIER_LDS", str(cap))
        capfd.readouterr()
        s = hip.Solver(as_matrix(S), _one_tier_opts(hip, verbose=1))
        staged.append(int(re.search(r"windows of up to (\d+) doubles in LDS", capfd.readouterr().err).group(1)))
        assert s.direct_tier_info()[0] == 1
        z = _nan(n)
        s.precond_dev(_dev(R[0]), z)
        rec = [z.cpu().numpy()]
        for k in (2, 8):
            d_Z = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda:0")
            s.direct_apply_multi_dev(_dev(R[:k]), d_Z)
            rec.append(d_Z.cpu().numpy())
            assert rec[-1][0].tobytes() == rec[0].tobytes()  # a column of a block: that column alone
        s.destroy()
        assert all(np.isfinite(a).all() for a in rec)
        out.append([a.tobytes() for a in rec])
    print(name, "n", n, "widest staged window without / with the knob:", staged)
    assert 16 < staged[0] <= n  # without the knob a window wider than 16 doubles is staged
    assert staged[1] <= 16      # ... with it none is: those windows are gathered
    assert out[0] == out[1]


@pytest.mark.gpu
def test_over_the_budget_and_the_driver(hip, matrix_path):
    """The grid --krylov direct refuses is solved with tiers = 0; the driver takes --direct-tiers, and without it
    refuses as before.  The tolerance here is 1e-10, not the 1e-12 of the small operators: with 262144 rows, b_i = i and
    ||x|| / ||b|| = 9.6e3 the residual b - S x itself is formed to about 2^-53 ||S|| ||x|| / ||b|| = 8.5e-12 of ||b|| at
    the worst, and measured at tol 1e-12 the recomputed residual stays at 3.2e-12 for all 10 rounds allowed (2.9e-12 on
    the host).  One round reaches 1.1e-11."""
    A = hip.lsbench_matrix_synth(OVER)
    n = A.nrows
    S = to_scipy(A.offs, np.asarray(A.cols) - A.base, A.vals)
    s = hip.Solver.create_direct(A, hip.default_opts(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_DIRECT, tol=1e-10, maxit=10), 0)
    nt, w, c, rows, launches = s.direct_tier_info()
    b = rhs(n)
    x, res = _solve_dev(s, b)
    s.destroy()
    true = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    print(OVER, "tiers", nt, "entries", w, "+", c, "rounds", res.iters, "relres", res.relres, "on the CPU", true)
    assert 2 <= nt <= hip.DIRECT_MAX_TIERS and w + 3 * c <= _lib.DIRECT_MAX_ENTRIES and sum(rows) == n
    assert res.status == hip.STATUS_CONVERGED and res.iters <= 2 and true <= 1e-10 * (1 + 1e-3)
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    base = [drv, "--solver", "hip", "--krylov", "direct", "--trials=2", "--matrix"]
    rc = subprocess.run(base + [matrix_path(XN3B), "--direct-tiers", "3"], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rec = rc.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[0]) <= 2 and int(f[2]) == 1 and float(f[1]) <= 1e-12
    grid = ["synth:" + OVER, "--operator", "raw"]
    rc = subprocess.run(base + grid, capture_output=True, text=True)
    assert rc.returncode != 0 and "LSB_DIRECT_MAX_ENTRIES" in rc.stderr, rc.stderr
    rc = subprocess.run(base + grid + ["--direct-tiers", "0", "--tol", "1e-10", "--maxit", "10"], capture_output=True,
                        text=True)
    assert rc.returncode == 0, rc.stderr
    rec = rc.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[0]) <= 2 and int(f[2]) == 1 and float(f[1]) <= 1e-10
