"""BiCGSTAB with right Jacobi preconditioning (opts.krylov = KRYLOV_BICGSTAB, hip_bicgstab.hip).

The oracle has no BiCGSTAB, so the yardstick is the plain numpy restatement below (`bicgstab`), pinned
here against a direct solve.  What it restates (x0 = 0, shadow residual r^ = r0 = b, M^-1 = diag(dinv)):

    bb = b.b ; rho = r^.r ; p = r ;  bb == 0: converged, 0 iterations
    repeat (k = 1, 2, ...; MAXIT when k-1 == maxit, before the iteration starts):
      p^ = dinv*p ; v = A p^ ; sigma = r^.v             breakdown if rho == 0 or sigma == 0
      alpha = rho/sigma ; s = r - alpha v ; ss = s.s
      if ss <= tol^2 bb:  x += alpha p^ ; r = s ; converged after k iterations      (half step)
      s^ = dinv*s ; t = A s^ ; ts = t.s ; tt = t.t       breakdown if tt == 0
      omega = ts/tt ; x += alpha p^ + omega s^ ; r = s - omega t ; rr = r.r ; rho' = r^.r
      if rr <= tol^2 bb: converged after k iterations
      breakdown if omega == 0
      beta = (rho'/rho)(alpha/omega) ; rho = rho' ; p = r + beta (p - omega v)

(a coefficient that is not finite is a breakdown too), and with verify: "converged" only when the residual
recomputed from x meets the tolerance; otherwise restart on it (r = b - A x, r^ = p = r, x kept), six times
at the most.  The iteration count of BiCGSTAB depends on the order in which the dot products are summed
(135 to 153 iterations on one of the matrices below), so counts are bounded, not pinned -- except on the
well-conditioned power-law operator; the EARLY iterates agree between summation orders to 2e-15 (2e-13 on
tj7a_A_18), which is what the per-iteration comparison uses."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from oracle import oracle as O

GAMMA = 1.585350372615855  # as tests/test_gmres.py
CONVERGED, BREAKDOWN, MAXIT = 1, 2, 3


# ------------------------------------------------------------------------------------ operators
def convdiff(nx, ny, c=0.6):
    """5-point diffusion + first-order convection: unsymmetric (tests/test_gmres.py)."""
    def t(n, lo, hi):
        return sp.diags([lo, 2.0, hi], [-1, 0, 1], shape=(n, n))
    A = sp.kron(sp.eye(ny), t(nx, -1 - c, -1 + c)) + sp.kron(t(ny, -1 - c / 2, -1 + c / 2), sp.eye(nx))
    A = A.tocsr()
    A.sort_indices()
    return A


def dominant_powerlaw(n, seed):
    thr, _ = O.powerlaw_table(GAMMA, 256)
    o, c, v = O.powerlaw(n, thr, seed)
    B = sp.csr_matrix((v, c, o.astype(np.int64)), shape=(n, n))
    A = (B + sp.diags(1.0 + np.asarray(abs(B).sum(axis=1)).ravel())).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def to_scipy(M):
    n = M.nrows
    A = sp.csr_matrix((M.vals.copy(), M.cols.astype(np.int64) - M.base, M.offs.astype(np.int64)), shape=(n, n))
    A.sort_indices()
    return A


def file_matrix(name, matrix_path):
    return to_scipy(la.lsbench_matrix_read(matrix_path(name)))


def small_operators(matrix_path):
    ops = {"convdiff": convdiff(60, 45), "powerlaw": dominant_powerlaw(4000, 3)}
    for name in ("xn3b_A_18", "tj7a_A_18", "xn3b_A_10"):
        ops[name] = file_matrix(name, matrix_path)
    return ops


def rhs(n):
    return np.arange(n, dtype=np.float64)  # b_i = i


def jacobi(A):
    return 1.0 / A.diagonal()


# ------------------------------------------------------------------------------------ the yardstick
def dot_reversed(a, b):
    return float(np.sum((a[::-1].astype(np.longdouble) * b[::-1].astype(np.longdouble))))


def dot_chunks(a, b):
    s = 0.0
    for i in range(0, len(a), 256):
        s += float(np.dot(a[i:i + 256], b[i:i + 256]))
    return s


def dot_exact(a, b):
    """The products rounded, their sum exact (math.fsum): the same bits on every machine, which np.dot's
    blocked sums are not -- used where a test asserts HOW FAR the recurrence drifts."""
    return math.fsum(a * b)


def bicgstab(A, b, dinv, tol, maxit, verify=False, dot=np.dot):
    """-> dict(x, iters, status, relres, true_relres, corrections, spmvs).  `iters` counts the iterations
    that formed an iterate (a breakdown in iteration k leaves k - 1)."""
    n = len(b)
    x = np.zeros(n)
    out = dict(x=x, iters=0, status=CONVERGED, relres=0.0, true_relres=-1.0, corrections=0, spmvs=0)
    bb = float(dot(b, b))
    if bb == 0.0:
        return out
    r, rhat, p = b.copy(), b.copy(), b.copy()
    rho, rr, thr = bb, bb, tol * tol * bb
    k = 0
    while True:
        while True:
            if k == maxit:
                status = MAXIT
                break
            if rho == 0.0 or not np.isfinite(rho):
                status = BREAKDOWN
                break
            ph = dinv * p
            v = A @ ph
            out["spmvs"] += 1
            sigma = float(dot(rhat, v))
            if sigma == 0.0 or not np.isfinite(sigma) or not np.isfinite(rho / sigma):
                status = BREAKDOWN
                break
            alpha = rho / sigma
            s = r - alpha * v
            ss = float(dot(s, s))
            if ss <= thr:
                x += alpha * ph
                r, rr, k, status = s, ss, k + 1, CONVERGED
                break
            sh = dinv * s
            t = A @ sh
            out["spmvs"] += 1
            ts, tt = float(dot(t, s)), float(dot(t, t))
            if tt == 0.0 or not np.isfinite(tt) or not np.isfinite(ts) or not np.isfinite(ts / tt):
                status = BREAKDOWN
                break
            omega = ts / tt
            x += alpha * ph + omega * sh
            r = s - omega * t
            rr, rho_new = float(dot(r, r)), float(dot(rhat, r))
            k += 1
            if rr <= thr:
                status = CONVERGED
                break
            if omega == 0.0:
                status = BREAKDOWN
                break
            beta = (rho_new / rho) * (alpha / omega)
            rho = rho_new
            p = r + beta * (p - omega * v)
        if not (verify and status == CONVERGED and tol > 0.0):
            break
        r = b - A @ x
        out["spmvs"] += 1
        rr = float(dot(r, r))
        out["true_relres"] = float(np.sqrt(rr / bb))
        if rr <= thr:
            break
        if out["corrections"] >= 6 or k >= maxit:
            status = MAXIT
            break
        out["corrections"] += 1
        rhat, p, rho = r.copy(), r.copy(), rr
    out.update(x=x, iters=k, status=status, relres=float(np.sqrt(rr / bb)))
    return out


def relerr(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def relres(A, x, b):
    return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------ without a GPU
def test_option_table_and_constants():
    lib = _lib.load()
    keep = la.default_opts()
    lib.lsb_hip_get_opts(C.byref(keep))
    try:
        assert lib.hip_cdna4_set_option(b"krylov", b"bicgstab") == 0
        got = _lib.Opts()
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.krylov == 4
        assert lib.hip_cdna4_set_option(b"krylov", b"bicgstabx") == 1
    finally:
        lib.lsb_hip_set_opts(C.byref(keep))
    assert la.KRYLOV_BICGSTAB == 4 and _lib.KRYLOV_BICGSTAB == 4
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        assert "LSB_KRYLOV_BICGSTAB = 4" in f.read()
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    r = subprocess.run([drv, "--help"], capture_output=True, text=True)
    assert "bicgstab" in r.stdout and "1e-4" in r.stdout


def _same(M, A):
    A = A.tocsr()
    A.sort_indices()
    assert M.base == 0 and M.nrows == A.shape[0]
    assert np.array_equal(M.offs, A.indptr) and np.array_equal(M.cols, A.indices)
    assert np.array_equal(M.vals, A.data)


def test_synth_conv_key():
    """lap2d / lap3d with conv=C: today's generator would ignore the key and hand back the Laplacian."""
    _same(la.lsbench_matrix_synth("lap2d:nx=60,ny=45,conv=0.6"), convdiff(60, 45))
    _same(la.lsbench_matrix_synth("lap2d:nx=37,ny=11,conv=0.3"), convdiff(37, 11, 0.3))
    plain, zero = la.lsbench_matrix_synth("lap2d:nx=60,ny=45"), la.lsbench_matrix_synth("lap2d:nx=60,ny=45,conv=0")
    assert np.array_equal(plain.offs, zero.offs) and np.array_equal(plain.cols, zero.cols)
    assert plain.vals.tobytes() == zero.vals.tobytes()
    plain3, zero3 = la.lsbench_matrix_synth("lap3d:nx=7,ny=5,nz=4"), la.lsbench_matrix_synth("lap3d:nx=7,ny=5,nz=4,conv=0")
    assert plain3.vals.tobytes() == zero3.vals.tobytes() and np.array_equal(plain3.cols, zero3.cols)
    # a row range equals the same rows of the whole
    whole = to_scipy(la.lsbench_matrix_synth("lap2d:nx=60,ny=45,conv=0.6"))
    part = la.lsbench_matrix_synth("lap2d:nx=60,ny=45,conv=0.6", 701, 1903)
    assert part.n_global == 2700 and part.nrows == 1202
    sub = whole[701:1903]
    assert np.array_equal(part.offs, sub.indptr) and np.array_equal(part.cols, sub.indices)
    assert np.array_equal(part.vals, sub.data)
    # 3-D against a Kronecker construction
    nx, ny, nz, c = 7, 5, 4, 0.6

    def t(n, lo, hi):
        return sp.diags([lo, 2.0, hi], [-1, 0, 1], shape=(n, n))
    A3 = (sp.kron(sp.eye(nz), sp.kron(sp.eye(ny), t(nx, -1 - c, -1 + c)))
          + sp.kron(sp.eye(nz), sp.kron(t(ny, -1 - c / 2, -1 + c / 2), sp.eye(nx)))
          + sp.kron(t(nz, -1 - c / 4, -1 + c / 4), sp.eye(nx * ny)))
    _same(la.lsbench_matrix_synth("lap3d:nx=7,ny=5,nz=4,conv=0.6"), A3)
    with pytest.raises(la.LsbenchHipError):  # one or the other
        la.lsbench_matrix_synth("lap2d:nx=60,ny=45,conv=0.6,coef=1")


@pytest.mark.parametrize("name", ["convdiff", "powerlaw", "xn3b_A_18", "tj7a_A_18", "xn3b_A_10"])
def test_yardstick_against_direct_solve(name, matrix_path):
    A = small_operators(matrix_path)[name]
    b = rhs(A.shape[0])
    xd = sla.spsolve(A.tocsc(), b)
    for dot in (np.dot, dot_reversed, dot_chunks):
        y = bicgstab(A, b, jacobi(A), 1e-10, 5000, dot=dot)
        print(name, dot.__name__, y["iters"], relres(A, y["x"], b), relerr(y["x"], xd))
        assert y["status"] == CONVERGED and y["relres"] <= 1e-10
        assert relres(A, y["x"], b) <= 2e-10
        assert relerr(y["x"], xd) <= 1e-8
    if name == "powerlaw":
        assert [bicgstab(A, b, jacobi(A), tol, 5000)["iters"] for tol in (1e-4, 1e-10, 1e-12)] == [6, 12, 14]


def test_yardstick_stop_rules_and_breakdown():
    A = convdiff(60, 45)
    b = rhs(A.shape[0])
    y = bicgstab(A, b, jacobi(A), 1e-14, 17)
    assert y["status"] == MAXIT and y["iters"] == 17 and y["spmvs"] == 34
    y = bicgstab(A, 0 * b, jacobi(A), 1e-10, 100)
    assert y["status"] == CONVERGED and y["iters"] == 0 and not y["x"].any()
    K = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    y = bicgstab(K, np.array([1.0, 0.0]), np.ones(2), 1e-10, 100)  # v = (0, -1): sigma = 0 in iteration 1
    assert y["status"] == BREAKDOWN and np.isfinite(y["x"]).all() and not y["x"].any()
    I = sp.diags([1.0, 2.0, 3.0, 4.0, 5.0]).tocsr()
    y = bicgstab(I, rhs(5), jacobi(I), 1e-12, 100)  # one half step
    assert y["status"] == CONVERGED and y["iters"] == 1 and y["spmvs"] == 1


def test_yardstick_restart_on_the_recomputed_residual():
    """lap2d 200 x 200, conv = 0.3: the recurrence says converged, the residual recomputed from x does not.
    How far it drifts depends on the summation order of the dot products -- np.dot here 2.6e-6 after 340
    iterations, one restart, 427 iterations, 7.5e-9; the same np.dot on another machine (other BLAS blocking)
    1.3e-8; sequential sums 4.0e-8; exact sums 1.1e-6 after 335, one restart, 418, 9.4e-9 -- so the drift is
    asserted on the exact sums, which are the same bits everywhere, and np.dot's figures are printed."""
    A = convdiff(200, 200, 0.3)
    b = rhs(A.shape[0])
    y = bicgstab(A, b, jacobi(A), 1e-8, 20000)
    print("np.dot:", y["iters"], relres(A, y["x"], b))
    assert y["status"] == CONVERGED and y["relres"] <= 1e-8  # (its drift is printed, not asserted)
    y0 = bicgstab(A, b, jacobi(A), 1e-8, 20000, dot=dot_exact)
    assert y0["status"] == CONVERGED and y0["relres"] <= 1e-8
    assert relres(A, y0["x"], b) > 1e-7
    y1 = bicgstab(A, b, jacobi(A), 1e-8, 20000, verify=True, dot=dot_exact)
    print("restart:", y0["iters"], relres(A, y0["x"], b), y1["iters"], y1["corrections"], y1["true_relres"])
    assert y1["status"] == CONVERGED and 1 <= y1["corrections"] <= 6 and y1["iters"] > y0["iters"]
    assert relres(A, y1["x"], b) <= 1e-8 * (1 + 1e-6)


# ------------------------------------------------------------------------------------ on the GPU
def _matrix(hip, A):
    return hip.Matrix.from_arrays(A.indptr, A.indices, A.data)


def _opts(hip, **kw):
    base = dict(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_BICGSTAB, tol=1e-10, maxit=5000)
    base.update(kw)
    return hip.default_opts(**base)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["convdiff", "powerlaw", "xn3b_A_18"])
def test_hip_early_iterates_match_the_yardstick(hip, name, matrix_path):
    """After 1 .. 6 iterations x agrees with the yardstick's to 1e-10 (summation orders differ by 2e-15 there;
    a wrong coefficient shows at 1e-3 or worse)."""
    A = small_operators(matrix_path)[name]
    b = rhs(A.shape[0])
    M = _matrix(hip, A)
    for k in range(1, 7):
        y = bicgstab(A, b, jacobi(A), 1e-14, k)
        s = hip.Solver(M, _opts(hip, tol=1e-14, maxit=k))
        x, res = s.solve(b)
        s.destroy()
        print(name, k, relerr(x, y["x"]))
        assert res.status == hip.STATUS_MAXIT and res.iters == k and y["iters"] == k
        assert res.spmvs == 2 * k
        assert relerr(x, y["x"]) <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["convdiff", "powerlaw", "xn3b_A_18", "tj7a_A_18", "xn3b_A_10"])
def test_hip_full_solves(hip, name, matrix_path):
    A = small_operators(matrix_path)[name]
    b = rhs(A.shape[0])
    y = bicgstab(A, b, jacobi(A), 1e-10, 5000)
    s = hip.Solver(_matrix(hip, A), _opts(hip))
    x, res = s.solve(b)
    x2, res2 = s.solve(b)  # the state is reset between solves
    s.destroy()
    xd = sla.spsolve(A.tocsc(), b)
    print(name, "iters", res.iters, "yardstick", y["iters"], "relres", res.relres, relres(A, x, b), relerr(x, xd))
    assert res.status == hip.STATUS_CONVERGED and res.relres <= 1e-10
    assert relres(A, x, b) <= 2e-10
    assert relerr(x, xd) <= 1e-8
    assert 0.7 * y["iters"] <= res.iters <= 1.3 * y["iters"]
    assert res2.iters == res.iters and np.array_equal(x, x2)


@pytest.mark.gpu
@pytest.mark.parametrize("tol,iters", [(1e-4, 6), (1e-10, 12), (1e-12, 14)])
def test_hip_iteration_count_on_the_powerlaw_operator(hip, tol, iters):
    A = dominant_powerlaw(4000, 3)
    b = rhs(A.shape[0])
    assert bicgstab(A, b, jacobi(A), tol, 5000)["iters"] == iters
    s = hip.Solver(_matrix(hip, A), _opts(hip, tol=tol))
    x, res = s.solve(b)
    s.destroy()
    print("powerlaw", tol, res.iters)
    assert res.status == hip.STATUS_CONVERGED and res.iters == iters


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["xn3b_A_18", "tj7a_A_18"])
def test_hip_cholmod_operator_reaches_the_golden_vector(hip, name, matrix_path, golden_x):
    A = hip.lsbench_matrix_read(matrix_path(name))
    b = rhs(A.nrows)
    s = hip.Solver(A, hip.default_opts(krylov=hip.KRYLOV_BICGSTAB, tol=1e-12, verify=1))
    x, res = s.solve(b)
    s.destroy()
    xg = golden_x(name)
    print(name, res.iters, res.corrections, res.true_relres, relerr(x, xg))
    assert res.status == hip.STATUS_CONVERGED and 0.0 <= res.true_relres <= 1e-12
    assert relerr(x, xg) <= 1e-10


@pytest.mark.gpu
def test_hip_toy_matrices(hip, matrix_path, golden_x):
    for name, iters in (("A0_02x02", 2), ("A1_02x02", 2), ("I1_05x05", 1)):
        A = hip.lsbench_matrix_read(matrix_path(name))
        s = hip.Solver(A, hip.default_opts(krylov=hip.KRYLOV_BICGSTAB, tol=1e-12))
        x, res = s.solve(rhs(A.nrows))
        s.destroy()
        print(name, res.iters, res.status, x)
        assert res.status == hip.STATUS_CONVERGED and res.iters == iters
        assert np.allclose(x, golden_x(name), rtol=1e-14, atol=1e-15)
        if name == "I1_05x05":
            assert res.spmvs == 1  # one half step


@pytest.mark.gpu
def test_hip_verify_restarts_on_the_recomputed_residual(hip):
    A = convdiff(200, 200, 0.3)
    b = rhs(A.shape[0])
    y0 = bicgstab(A, b, jacobi(A), 1e-8, 20000, dot=dot_exact)  # (exact sums: the same bits on every machine)
    assert y0["status"] == CONVERGED and relres(A, y0["x"], b) > 1e-7  # the case is known to drift
    M = la.lsbench_matrix_synth("lap2d:nx=200,ny=200,conv=0.3")
    s = hip.Solver(M, _opts(hip, tol=1e-8, maxit=20000, verify=0))
    x, res = s.solve(b)
    s.destroy()
    print("verify = 0: iters", res.iters, "relres", res.relres, "recomputed", relres(A, x, b))
    assert res.status == hip.STATUS_CONVERGED and res.relres <= 1e-8 and res.true_relres < 0.0
    s = hip.Solver(M, _opts(hip, tol=1e-8, maxit=20000, verify=1))
    x, res = s.solve(b)
    x2, res2 = s.solve(b)
    s.destroy()
    true = relres(A, x, b)
    print("verify = 1: iters", res.iters, "corrections", res.corrections, "true_relres", res.true_relres, "cpu", true)
    assert res.status == hip.STATUS_CONVERGED and 1 <= res.corrections <= 6
    assert true <= 1e-8 * (1 + 1e-6)
    assert abs(res.true_relres - true) <= 1e-3 * true
    assert res2.iters == res.iters and res2.corrections == res.corrections and np.array_equal(x, x2)


@pytest.mark.gpu
def test_hip_breakdown_and_zero_rhs(hip):
    K = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    K.sort_indices()
    s = hip.Solver(_matrix(hip, K), _opts(hip, precond=hip.PRECOND_NONE, maxit=100))
    x, res = s.solve(np.array([1.0, 0.0]))
    s.destroy()
    assert res.status == hip.STATUS_BREAKDOWN and np.isfinite(x).all()
    assert res.iters == 0 and res.spmvs == 1  # the product of the iteration that broke down counts
    A = convdiff(60, 45)
    s = hip.Solver(_matrix(hip, A), _opts(hip))
    x, res = s.solve(np.zeros(A.shape[0]))
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED and res.iters == 0 and not x.any()


@pytest.mark.gpu
def test_hip_strong_convection_is_reported_truthfully(hip):
    """300 x 300, conv = 0.6: outside what the method solves with this right-hand side (the yardstick's
    residual grows to 1e7).  Whatever the status: no NaN or Inf in x, and `converged` only with a recomputed
    residual that meets the tolerance."""
    M = la.lsbench_matrix_synth("lap2d:nx=300,ny=300,conv=0.6")
    A = to_scipy(M)
    b = rhs(A.shape[0])
    s = hip.Solver(M, _opts(hip, tol=1e-8, maxit=20000, verify=1))
    x, res = s.solve(b)
    s.destroy()
    print("300^2 conv=0.6: status", res.status, "iters", res.iters, "corrections", res.corrections,
          "relres", res.relres, "recomputed", relres(A, x, b))
    assert np.isfinite(x).all()
    if res.status == hip.STATUS_CONVERGED:
        assert relres(A, x, b) <= 1e-8 * (1 + 1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nvirt", [("convdiff", 2), ("convdiff", 5), ("powerlaw", 3)])
def test_hip_over_row_range_shards(hip, name, nvirt, matrix_path):
    A = {"convdiff": convdiff(60, 45), "powerlaw": dominant_powerlaw(4000, 3)}[name]
    b = rhs(A.shape[0])
    y = bicgstab(A, b, jacobi(A), 1e-10, 5000)
    M = _matrix(hip, A)
    s1 = hip.Solver(M, _opts(hip))
    x1, r1 = s1.solve(b)
    s1.destroy()
    sp_ = hip.Solver(M, _opts(hip, nvirt=nvirt))
    xp, rp = sp_.solve(b)
    xq, rq = sp_.solve(b)
    sp_.destroy()
    print(name, nvirt, "iters", rp.iters, "one shard", r1.iters, "yardstick", y["iters"])
    assert rp.status == hip.STATUS_CONVERGED
    assert 0.7 * y["iters"] <= rp.iters <= 1.3 * y["iters"]
    assert rq.iters == rp.iters and np.array_equal(xp, xq)
    assert relerr(xp, x1) <= 1e-8
    assert relres(A, xp, b) <= 2e-10


@pytest.mark.gpu
def test_hip_shards_on_the_rare_paths(hip):
    """What the sharded driver does off the main road: the restart of verify (an exchange and an all-reduce
    outside the iteration), the half step (the launch behind it reduces partials nobody wrote), a breakdown,
    and the other two diagonals."""
    A = convdiff(200, 200, 0.3)
    b = rhs(A.shape[0])
    M = la.lsbench_matrix_synth("lap2d:nx=200,ny=200,conv=0.3")
    s = hip.Solver(M, _opts(hip, tol=1e-8, maxit=20000, verify=1, nvirt=3))
    x, res = s.solve(b)
    x2, res2 = s.solve(b)
    s.destroy()
    true = relres(A, x, b)
    print("nvirt 3, verify: iters", res.iters, "corrections", res.corrections, res.true_relres, true)
    assert res.status == hip.STATUS_CONVERGED and res.corrections <= 6 and true <= 1e-8 * (1 + 1e-6)
    assert abs(res.true_relres - true) <= 1e-3 * true
    assert res2.iters == res.iters and np.array_equal(x, x2)
    # the half step: a diagonal operator is solved by x = alpha p^ of iteration 1
    D = sp.diags(np.arange(1.0, 41.0)).tocsr()
    s = hip.Solver(_matrix(hip, D), _opts(hip, tol=1e-12, nvirt=2))
    x, res = s.solve(rhs(40))
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED and res.iters == 1 and res.spmvs == 1
    assert np.allclose(x, rhs(40) / np.arange(1.0, 41.0), rtol=1e-14, atol=0)
    # breakdown: a block-diagonal skew operator, b = e_1 in every block: sigma = 0 in iteration 1
    K = sp.kron(sp.eye(8), sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))).tocsr()
    K.sort_indices()
    s = hip.Solver(_matrix(hip, K), _opts(hip, precond=hip.PRECOND_NONE, maxit=100, nvirt=2))
    x, res = s.solve(np.tile([1.0, 0.0], 8))
    s.destroy()
    assert res.status == hip.STATUS_BREAKDOWN and res.iters == 0 and res.spmvs == 1 and not x.any()
    A = convdiff(60, 45)
    b = rhs(A.shape[0])
    for pc in (hip.PRECOND_NONE, hip.PRECOND_L1JACOBI):
        s = hip.Solver(_matrix(hip, A), _opts(hip, precond=pc, nvirt=2))
        x, res = s.solve(b)
        s.destroy()
        assert res.status == hip.STATUS_CONVERGED and relres(A, x, b) <= 2e-10


@pytest.mark.gpu
def test_hip_preconditioner_choices_and_reordering(hip):
    A = convdiff(60, 45)
    b = rhs(A.shape[0])
    M = _matrix(hip, A)
    xs = {}
    for key, kw in (("jacobi", {}), ("none", dict(precond=hip.PRECOND_NONE)), ("l1", dict(precond=hip.PRECOND_L1JACOBI)),
                    ("rcm", dict(reorder=1))):
        s = hip.Solver(M, _opts(hip, **kw))
        xs[key], res = s.solve(b)
        s.destroy()
        print(key, res.iters, res.relres)
        assert res.status == hip.STATUS_CONVERGED and relres(A, xs[key], b) <= 2e-10
    for key in ("none", "l1", "rcm"):
        assert relerr(xs[key], xs["jacobi"]) <= 1e-8


@pytest.mark.gpu
def test_hip_on_the_fast_spmv_forms(hip):
    """1000 x 1000, conv = 0.1: 5 M non-zeros (above the timing pass's threshold), line-padded, constant slots.
    The yardstick with the restart on this operator (about two minutes on a CPU, so recorded, not re-run):
    one restart, 2241 iterations, recomputed residual 9.3e-9; without it the recurrence stops after 1921
    iterations at a recomputed residual of 3.9e-6."""
    M = la.lsbench_matrix_synth("lap2d:nx=1000,ny=1000,conv=0.1")
    A = to_scipy(M)
    b = rhs(A.shape[0])
    s = hip.Solver(M, _opts(hip, tol=1e-8, maxit=20000, verify=1))
    x, res = s.solve(b)
    layout, itbytes, rows = s.spmv_layout_bytes, s.iteration_bytes, s.n_local + s.padded
    s.destroy()
    true = relres(A, x, b)
    print("1000^2 conv=0.1: iters", res.iters, "corrections", res.corrections, "true_relres", res.true_relres,
          "cpu", true, "padded rows", rows - A.shape[0])
    assert res.status == hip.STATUS_CONVERGED and res.corrections <= 6
    assert true <= 1e-8 * (1 + 1e-6)
    assert rows > A.shape[0]  # line-padded
    # two SpMVs + 18 vector passes (the Jacobi diagonal is one constant: 20 - 2)
    assert layout > 0 and itbytes == 2 * layout + 8 * 18 * rows


@pytest.mark.gpu
def test_driver_runs_the_reference_setting(hip, matrix_path):
    """driver --solver hip --krylov bicgstab --operator raw --tol 1e-4: BiCGSTAB + Jacobi stopped on a residual
    reduction of 1e-4 is what the reference's Ginkgo backend runs."""
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    r = subprocess.run([drv, "--solver", "hip", "--matrix", matrix_path("xn3b_A_18"), "--krylov", "bicgstab",
                        "--operator", "raw", "--tol", "1e-4", "--trials=2", "--verbose", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    i = lines.index("===matrix,n,nnz,trials,solver,ordering,elapsed===")
    f = lines[i + 1].split(",")
    assert (int(f[1]), int(f[2]), int(f[3]), int(f[4])) == (3461, 76591, 2, 6)
    x = np.array([float(l.split("=")[1]) for l in lines if l.startswith("x[")])
    A = file_matrix("xn3b_A_18", matrix_path)
    assert len(x) == 3461 and relres(A, x, rhs(3461)) <= 2e-4  # (x is printed with a few digits)
