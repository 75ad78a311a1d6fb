"""The direct solver (opts.krylov = KRYLOV_DIRECT, --krylov direct; lsb_direct.c, hip_direct.hip, hip_direct_drv.c).

    creation   nested dissection (lsb_csr_nd), the symbolic count (lsb_csr_skyline_count), Cholesky and W = L^-1 as a
               skyline (lsb_csr_skyline_inverse): row k of W is the dense run of columns first[k] .. k
    round      x (+)= P^T W^T (W (P r)), then r = b - S x and the stop test on that recomputed residual

CPU: the surface; the ordering is a permutation on every kind of graph; the count against a numpy restatement of Liu's
algorithm and against the figures the method was proposed with; the factor against numpy (first, parent, run_end, W
(P S P^T) W^T = I); what it refuses; and what the GPU tests lean on -- with the library's W in numpy one round reaches
1e-11 and two reach 1e-12 on the seven reference matrices.  GPU: one application against numpy; the solves; warm
starts; the refusals and the driver."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

import lsbench_amd as la
from conftest import ROOT, SPD
from lsbench_amd import _lib
from oracle import oracle as O
from test_amg import as_matrix
from test_amg_f32 import POWERLAW, _op, _relerr
from test_mrhs import columns

XN3B, TJ7A, ONE, TRI, FOREST, DIAG, SINGLE = "xn3b_A_18", "tj7a_A_12", "lap2d:nx=12,ny=9", "tri300", "forest", \
    "I1_05x05", "n1"
WIDE = "lap2d:nx=100,ny=90"  # 9000 rows: the top rows' windows of P r are wider than k_dirt_rows stages in LDS
# the entries of W under the throw-away ordering the method was proposed with (BFS level sets, leaf size 32)
PROPOSED = {XN3B: 2.46e6, TJ7A: 4.27e6}
EPS = 2.0 ** -52
CONVERGED, BREAKDOWN, MAXIT_ST = 1, 2, 3


# ------------------------------------------------------------------------------------ inputs and restatements
def _lap2d(nx, ny):
    T = lambda m: sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    return (sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx))).tocsr()


def op(name, matrix_path):
    """the operator S as a scipy CSR with sorted rows"""
    if name == TRI:
        S = sp.diags([-np.ones(299), 2.5 * np.ones(300), -np.ones(299)], [-1, 0, 1]).tocsr()
    elif name == FOREST:  # two grids that share nothing
        S = sp.block_diag([_lap2d(9, 7), _lap2d(5, 11)]).tocsr()
    elif name == DIAG:
        S = sp.diags([np.arange(1.0, 6.0)], [0]).tocsr()
    elif name == SINGLE:
        S = sp.csr_matrix(np.array([[3.0]]))
    else:
        return _op(name, matrix_path)
    S.sort_indices()
    return S


def liu(S, perm):
    """parent[] (n on a root) of the elimination tree of P S P^T, perm[new] = old: Liu's algorithm, path compression"""
    n = S.shape[0]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    parent, anc = [n] * n, [n] * n
    indptr, indices = S.indptr, S.indices
    for k in range(n):
        row = int(perm[k])
        for c in indices[indptr[row]:indptr[row + 1]]:
            i = int(inv[c])
            while i < k:
                nxt = anc[i]
                anc[i] = k
                if nxt == n:
                    parent[i] = k
                i = nxt
    return np.array(parent, np.int64)


def depths(parent):
    n = len(parent)
    d = np.zeros(n + 1, np.int64)
    for k in range(n - 1, -1, -1):
        d[k] = d[parent[k]] + 1
    return d[:n]


@functools.lru_cache(maxsize=None)
def _factor(name, matrix_path):
    """(S, the library's ordering, its skyline factor as a dict, W as a scipy CSR in the new numbering), made once"""
    S = op(name, matrix_path)
    A = as_matrix(S)
    perm = la.lsb_csr_nd(A)
    W = la.lsb_csr_skyline_inverse(A, perm)
    assert isinstance(W, dict), W
    n = W["n"]
    lens = np.arange(n) - W["first"].astype(np.int64) + 1
    assert (np.diff(W["woff"].astype(np.int64)) == lens).all()
    cols = np.concatenate([np.arange(int(f), k + 1) for k, f in enumerate(W["first"])]) if n else np.zeros(0, int)
    Wm = sp.csr_matrix((W["vals"], cols, W["woff"].astype(np.int64)), shape=(n, n))
    return S, perm, W, Wm


def apply_np(W, Wm, r, flip=False):
    """z = P^T W^T (W (P r)) in numpy; flip: every sum in the opposite order"""
    p = W["perm"].astype(np.int64)
    if flip:
        n = len(p)
        Wf = Wm[:, ::-1].tocsr()
        Wf.sort_indices()
        Wtf = Wm.T.tocsr()[:, ::-1].tocsr()
        Wtf.sort_indices()
        t = Wf @ r[p][::-1]
        zp = Wtf @ t[::-1]
    else:
        zp = Wm.T.tocsr() @ (Wm @ r[p])
    z = np.empty_like(zp)
    z[p] = zp
    return z


def rounds_np(S, W, Wm, b, nrounds):
    """the device's rounds in numpy: [(x_k, recomputed relres_k)]"""
    x, r, out = np.zeros_like(b), b.copy(), []
    for _ in range(nrounds):
        x = x + apply_np(W, Wm, r)
        r = b - S @ x
        out.append((x, float(np.linalg.norm(r) / np.linalg.norm(b))))
    return out


# ------------------------------------------------------------------------------------ without a GPU
def test_surface():
    assert la.KRYLOV_DIRECT == 6 and _lib.KRYLOV_DIRECT == 6
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    assert "LSB_KRYLOV_DIRECT = 6" in header and "LSB_KRYLOV_RICHARDSON = 5" in header
    assert re.search(r"#define LSB_DIRECT_MAX_ENTRIES \(1ull << 28\)", header) and _lib.DIRECT_MAX_ENTRIES == 1 << 28
    assert "a few thousand to a few tens of thousands of rows" in re.sub(r"\s+", " ", header)
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    for name in ("lsb_csr_nd", "lsb_csr_nd_bounded", "lsb_csr_skyline_count", "lsb_csr_skyline_inverse",
                 "lsb_skyinv_free", "lsb_hip_solver_direct_info"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name) and name in exported, name
    assert not [s for s in exported if s.startswith("lsb_k_dir")]  # the launchers stay inside
    # struct lsb_hip_opts gained nothing
    assert [f[0] for f in _lib.Opts._fields_][-1] == "amg_cheb_ratio" and list(_lib.Opts._TAIL) == ["fsai_blocks"]
    o, got = la.default_opts(), _lib.Opts()
    try:
        assert lib.hip_cdna4_set_option(b"krylov", b"direct") == 0
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.krylov == 6
        assert lib.hip_cdna4_set_option(b"krylov", b"direct2") == 1
    finally:
        lib.lsb_hip_set_opts(C.byref(o))
    assert la.default_opts().krylov == la.KRYLOV_AUTO  # opt-in
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    assert "direct" in subprocess.run([drv, "--help"], capture_output=True, text=True).stdout
    assert lib.lsb_hip_solver_direct_info(None, None, None, None) == 2


@pytest.mark.parametrize("name", [XN3B, ONE, TRI, DIAG, FOREST, SINGLE])
def test_nd_is_a_permutation(name, matrix_path):
    S = op(name, matrix_path)
    n = S.shape[0]
    perm = la.lsb_csr_nd(as_matrix(S))
    assert len(perm) == n and sorted(perm.tolist()) == list(range(n))
    count, height = la.lsb_csr_skyline_count(as_matrix(S), perm)
    natural = la.lsb_csr_skyline_count(as_matrix(S), np.arange(n, dtype=np.uint32))
    print(name, "n", n, "entries", count, "height", height, "in the natural order", natural)
    if name == TRI:
        assert natural[1] == 300 and height <= 40
    if name == DIAG:
        assert (count, height) == (5, 1)  # all roots
    if name == SINGLE:
        assert (count, height) == (1, 1)
    # the bounded form: the same ordering under a budget it meets, a refusal with its lower bound under one it misses
    p2, lower = la.lsb_csr_nd(as_matrix(S), budget=1 << 40)
    assert p2.tolist() == perm.tolist() and n <= lower <= count
    p3, lower3 = la.lsb_csr_nd(as_matrix(S), budget=n - 1 if n > 1 else 0)
    assert p3 is None and lower3 > (n - 1 if n > 1 else 0)


@pytest.mark.parametrize("name", [XN3B, TJ7A, ONE, TRI, FOREST])
def test_skyline_count(name, matrix_path):
    S = op(name, matrix_path)
    A = as_matrix(S)
    perm = la.lsb_csr_nd(A)
    count, height = la.lsb_csr_skyline_count(A, perm)
    d = depths(liu(S, perm))
    print(name, "entries of W", count, "height", height, "proposed with", PROPOSED.get(name))
    assert count == int(d.sum()) and height == int(d.max())
    if name in PROPOSED:
        assert count < 1.1 * PROPOSED[name]
    bad = perm.copy()
    bad[0] = bad[1]
    assert la.lsb_csr_skyline_count(A, bad) == (0, 0)  # no permutation


@pytest.mark.parametrize("name", [ONE, TRI, FOREST, XN3B])
def test_skyline_inverse(name, matrix_path):
    S, perm, W, Wm = _factor(name, matrix_path)
    n = W["n"]
    p = W["perm"].astype(np.int64)
    assert sorted(p.tolist()) == list(range(n))
    parent = liu(S, p)
    assert (parent > np.arange(n)).all()  # a postorder: the tree climbs
    size = np.ones(n + 1, np.int64)
    for k in range(n):
        size[parent[k]] += size[k]
    run_end = np.arange(n)
    for k in range(n - 2, -1, -1):
        if parent[k] == k + 1:
            run_end[k] = run_end[k + 1]
    assert (W["parent"] == parent).all() and (W["first"] == np.arange(n) + 1 - size[:n]).all()
    assert (W["run_end"] == run_end).all()
    assert int(W["woff"][-1]) == la.lsb_csr_skyline_count(as_matrix(S), perm)[0]  # the postorder keeps the count
    jumps = []
    for j in range(0, n, max(1, n // 50)):
        k, c = j, 0
        while k < n:
            k, c = int(parent[run_end[k]]), c + 1
        jumps.append(c)
    D = Wm.toarray()
    assert not np.triu(D, 1).any()
    B = S[p][:, p].toarray()
    err = np.abs(D @ B @ D.T - np.eye(n)).max()
    print(name, "n", n, "entries", int(W["woff"][-1]), "max |W (P S P^T) W^T - I|", err, "jumps to the root",
          max(jumps))
    assert err <= 1e-10
    assert max(jumps) <= 2 + int(np.log2(n))


def test_inverse_refusals():
    ind = la.Matrix.from_arrays([0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0])
    assert la.lsb_csr_skyline_inverse(ind, la.lsb_csr_nd(ind)) == 1
    nan = la.Matrix.from_arrays([0, 2, 4], [0, 1, 0, 1], [2.0, float("nan"), float("nan"), 2.0])
    assert la.lsb_csr_skyline_inverse(nan, la.lsb_csr_nd(nan)) == 1
    ok = la.Matrix.from_arrays([0, 2, 4], [0, 1, 0, 1], [2.0, 1.0, 1.0, 2.0])
    assert la.lsb_csr_skyline_inverse(ok, np.array([0, 0], np.uint32)) == 3  # no permutation


@pytest.mark.parametrize("name", SPD)
def test_cpu_precondition(name, matrix_path, golden_x):
    """With the library's W in numpy on b_i = i: round 1 has a recomputed relres <= 1e-11, round 2 <= 1e-12, x is
    within 1e-10 of the golden solution; on xn3b_A_18 the same for the other columns of test_mrhs.columns."""
    S, perm, W, Wm = _factor(name, matrix_path)
    b = O.rhs(S.shape[0])
    (x1, r1), (x2, r2) = rounds_np(S, W, Wm, b, 2)
    e1, e2 = _relerr(x1, golden_x(name)), _relerr(x2, golden_x(name))
    print(name, "n", S.shape[0], "entries", int(W["woff"][-1]), "relres after round 1, 2:", r1, r2,
          "x against the golden x:", e1, e2)
    assert r1 <= 1e-11 and r2 <= 1e-12 and e1 <= 1e-10 and e2 <= 1e-10
    if name == XN3B:
        B = columns(S)
        for c in range(1, B.shape[1]):
            if not B[:, c].any():
                continue
            (_, q1), (_, q2) = rounds_np(S, W, Wm, np.ascontiguousarray(B[:, c]), 2)
            print("   column", c, "relres after round 1, 2:", q1, q2)
            assert q1 <= 1e-11 and q2 <= 1e-12


# ------------------------------------------------------------------------------------ on the GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")


def _solver(hip, name, matrix_path, **kw):
    """a direct solver on the operator the numpy side uses, as read"""
    kw.setdefault("op_mode", hip.OP_RAW)
    kw.setdefault("krylov", hip.KRYLOV_DIRECT)
    return hip.Solver(as_matrix(op(name, matrix_path)), hip.default_opts(**kw))


def _solve_dev(s, b, d_x=None, warm=False):
    d_x = _nan(len(b)) if d_x is None else d_x
    res = s.solve_dev(_dev(b), d_x, warm=warm) if warm else s.solve_dev(_dev(b), d_x)
    return d_x.cpu().numpy(), res


@pytest.mark.gpu
@pytest.mark.parametrize("name", [ONE, TRI, FOREST, POWERLAW, XN3B, WIDE])
def test_one_application(hip, name, matrix_path):
    """precond_dev against W^T (W r) formed in numpy from the same skyline.  The bound: four times what numpy itself
    moves between two summation orders, and no less than four units of fp64 rounding."""
    S, perm, W, Wm = _factor(name, matrix_path)
    n = S.shape[0]
    r = np.sin(np.arange(n, dtype=np.float64)) + 0.5
    za, zb = apply_np(W, Wm, r), apply_np(W, Wm, r, flip=True)
    if name == WIDE:  # the path that gathers P r from global memory: the root's row spans all columns
        with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_direct_drv.c")) as f:
            cap = int(re.search(r"#define DIR_LDS_CAP (\d+)u", f.read()).group(1))
        assert int(W["first"][n - 1]) == 0 and n > cap
    s = _solver(hip, name, matrix_path)
    assert s.direct_info[0] == int(W["woff"][-1])
    assert s.direct_info[1] == int(depths(W["parent"].astype(np.int64)).max())
    out = []
    for _ in range(2):
        z = _nan(n)
        s.precond_dev(_dev(r), z)
        out.append(z.cpu().numpy())
    if name == WIDE:  # ... and a solve through it
        b = O.rhs(n)
        x, res = _solve_dev(s, b)
        true = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
        print(name, "rounds", res.iters, "relres", res.relres, "on the CPU", true)
        assert res.status == hip.STATUS_CONVERGED and res.iters <= 2 and true <= 1e-12 * (1 + 1e-3)
    s.destroy()
    e_np, e_gpu = _relerr(zb, za), _relerr(out[0], za)
    bound = 4.0 * max(e_np, EPS)
    print(name, "n", n, "device against numpy", e_gpu, "numpy between two orders", e_np, "bound", bound)
    assert np.isfinite(out[0]).all() and out[0].tobytes() == out[1].tobytes()
    assert bound <= 1e-13 and e_gpu <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPD)
def test_solves(hip, name, matrix_path, golden_x):
    S = op(name, matrix_path)
    n = S.shape[0]
    b, xg = O.rhs(n), golden_x(name)
    got = []
    for graph in (1, 0):
        s = _solver(hip, name, matrix_path, tol=1e-12, maxit=10, use_graph=graph)
        assert not s.padded and s.iteration_bytes == 0
        x, res = _solve_dev(s, b)
        x2, res2 = _solve_dev(s, b)  # (the hinted solve)
        buf = _nan(n + 3)  # x 8 bytes past a 16-byte boundary
        off = 1 if buf.data_ptr() % 16 == 0 else 0
        assert (buf.data_ptr() + 8 * off) % 16 == 8
        x3, res3 = _solve_dev(s, b, buf[off:off + n])
        around = buf.cpu().numpy()
        assert np.isnan(around[:off]).all() and np.isnan(around[off + n:]).all()  # nothing written beside it
        xh, resh = s.solve(b)  # host buffers
        s.destroy()
        true = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
        print(name, "graph", graph, "rounds", res.iters, "relres", res.relres, "on the CPU", true, "golden",
              _relerr(x, xg))
        assert res.status == hip.STATUS_CONVERGED and res.iters <= 2 and res.relres <= 1e-12
        assert res.true_relres == res.relres and res.spmvs == res.iters
        assert true <= 1e-12 * (1 + 1e-3) and _relerr(x, xg) <= 1e-10
        for xx, rr in ((x2, res2), (x3, res3), (np.asarray(xh), resh)):
            assert xx.tobytes() == x.tobytes()
            assert (rr.status, rr.iters, rr.spmvs, rr.relres) == (res.status, res.iters, res.spmvs, res.relres)
        got.append((x, res))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].relres == got[1][1].relres
    # tol 1e-10: one round
    s = _solver(hip, name, matrix_path, tol=1e-10, maxit=10)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters) == (hip.STATUS_CONVERGED, 1) and res.relres <= 1e-10
    # the reference's direct protocol: one round, nothing recomputed
    s = _solver(hip, name, matrix_path, tol=0.0, maxit=1)
    x, res = _solve_dev(s, b)
    x2, res2 = _solve_dev(s, b)
    s.destroy()
    print(name, "tol 0, maxit 1: golden", _relerr(x, xg))
    assert (res.status, res.iters, res.relres, res.spmvs) == (hip.STATUS_MAXIT, 1, -1.0, 0)
    assert _relerr(x, xg) <= 1e-10 and x2.tobytes() == x.tobytes()
    # a tolerance nobody meets: MAXIT after the one round there is, with the figure it reached
    s = _solver(hip, name, matrix_path, tol=1e-30, maxit=1)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters, res.spmvs) == (hip.STATUS_MAXIT, 1, 1) and np.isfinite(res.relres) and res.relres > 0


@pytest.mark.gpu
def test_rounds_against_numpy_and_stop_rules(hip, matrix_path):
    S, perm, W, Wm = _factor(TJ7A, matrix_path)
    n = S.shape[0]
    b = O.rhs(n)
    want = rounds_np(S, W, Wm, b, 3)
    for N in (1, 2, 3):  # tol = 0: exactly N rounds, the last without a residual
        s = _solver(hip, TJ7A, matrix_path, tol=0.0, maxit=N, check_every=1 if N == 3 else 0)
        x, res = _solve_dev(s, b)
        s.destroy()
        print("rounds", N, "x against numpy's", _relerr(x, want[N - 1][0]))
        assert (res.status, res.iters, res.relres, res.spmvs) == (hip.STATUS_MAXIT, N, -1.0, N - 1)
        assert _relerr(x, want[N - 1][0]) <= 1e-12
    s = _solver(hip, TJ7A, matrix_path, tol=1e-12, maxit=10)
    x, res = _solve_dev(s, np.zeros(n))  # b = 0: x = 0
    assert res.status == hip.STATUS_CONVERGED and res.relres == 0.0 and not x.any()
    bad = b.copy()
    bad[n // 2] = float("nan")
    x, res = _solve_dev(s, bad)
    assert (res.status, res.iters) == (hip.STATUS_BREAKDOWN, 1)
    x, res = _solve_dev(s, b)  # ... and the solver is as good as before
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED and res.iters <= 2
    s = _solver(hip, TJ7A, matrix_path, tol=1e-12, maxit=0)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters) == (hip.STATUS_MAXIT, 0) and not x.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [XN3B, TJ7A])
def test_warm_start(hip, name, matrix_path, golden_x):
    n = op(name, matrix_path).shape[0]
    b = O.rhs(n)
    s = _solver(hip, name, matrix_path, tol=1e-12, maxit=10)
    cold, rc = _solve_dev(s, b)
    x, res = _solve_dev(s, b, _dev(golden_x(name)), warm=True)
    start = s.start_relres(1)[0]
    print(name, "from the golden x: start", start, "rounds", res.iters)
    assert start <= 1e-12 and res.status == hip.STATUS_CONVERGED and res.iters <= 1
    x, res = _solve_dev(s, b, _dev(np.zeros(n)), warm=True)
    s.destroy()
    print(name, "from 0 against the cold solve", _relerr(x, cold))
    assert res.status == hip.STATUS_CONVERGED and _relerr(x, cold) <= 1e-13


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import time
import lsbench_amd as la
assert la.hip_cdna4_init() == 0
A = la.lsbench_matrix_synth(sys.argv[2])
print("start", repr(time.time()), flush=True)
la.Solver(A, la.default_opts(krylov=la.KRYLOV_DIRECT, op_mode=la.OP_RAW, **eval(sys.argv[3])))
"""


@pytest.mark.gpu
def test_refusals_and_the_driver(hip, matrix_path, tmp_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    n = op(ONE, matrix_path).shape[0]
    s = _solver(hip, ONE, matrix_path)
    d_B = _dev(np.tile(O.rhs(n), (2, 1)))
    d_X = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_spmm_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_solve_block_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all())
    s.destroy()
    j = hip.Solver(as_matrix(op(ONE, matrix_path)), hip.default_opts(op_mode=hip.OP_RAW))
    assert j.direct_info is None
    j.destroy()
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    base = [drv, "--solver", "hip", "--krylov", "direct", "--trials=2", "--matrix"]
    rc = subprocess.run(base + [matrix_path(XN3B), "--nvirt", "2"], capture_output=True, text=True)
    assert rc.returncode != 0 and "direct" in rc.stderr, rc.stderr
    ind = tmp_path / "indefinite.txt"
    ind.write_text("4 0\n0 0 1\n0 1 2\n1 0 2\n1 1 1\n")
    rc = subprocess.run(base + [str(ind)], capture_output=True, text=True)
    assert rc.returncode != 0 and "direct" in rc.stderr and "positive definite" in rc.stderr, rc.stderr
    # persistent, and an operator over the budget: the library exits, so in child processes
    rc = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "lap2d:nx=20,ny=20", "dict(persistent=1)"],
                        capture_output=True, text=True)
    assert rc.returncode != 0 and "direct" in rc.stderr and "persistent" in rc.stderr, rc.stderr
    rc = subprocess.run([sys.executable, "-c", _CHILD, ROOT, "lap2d:nx=3162,ny=3162", "dict()"],
                        capture_output=True, text=True)
    took = time.time() - float(re.search(r"start ([0-9.e+-]+)", rc.stdout).group(1))  # (the library exits)
    print("the 10 M-row grid: refused", took, "s after Solver() was entered:", rc.stderr.strip().splitlines()[-1])
    assert rc.returncode != 0 and "direct" in rc.stderr and re.search(r"at least \d+ entries", rc.stderr), rc.stderr
    assert took < 5.0
    rc = subprocess.run(base + [matrix_path(XN3B)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rec = rc.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[0]) <= 2 and int(f[2]) == 1 and float(f[1]) <= 1e-12
