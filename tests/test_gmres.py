"""GMRES(m): the oracle's restatement against scipy
on the CPU, the HIP path against the oracle and a sparse direct solve on the
GPU.  Operators: a convection-diffusion stencil (unsymmetric), the RAW file
matrix of the reference (symmetric only to 1e-7), a diagonally dominant
power-law matrix."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from oracle import oracle as O

GAMMA = 1.585350372615855


def convdiff(nx, ny, c=0.6):
    """5-point diffusion + first-order upwind convection: unsymmetric, M-matrix."""
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


def operators():
    return {"convdiff": convdiff(60, 45), "powerlaw": dominant_powerlaw(4000, 3)}


@functools.lru_cache(maxsize=None)
def operator(name):
    """The two operators above and their twins of odd order (2655 and 4001 rows: the basis
    kernels' odd last element, the pad behind every basis column)."""
    return {"convdiff": lambda: convdiff(60, 45), "powerlaw": lambda: dominant_powerlaw(4000, 3),
            "convdiff_odd": lambda: convdiff(59, 45), "powerlaw_odd": lambda: dominant_powerlaw(4001, 3)}[name]()


LD = np.longdouble
EARLY_RESTART, EARLY_TOL = 5, 1e-14
EARLY_CUTS = [1, 2, 4, 5, 6, 11]  # inside a cycle, at its end, just behind a restart, in the third cycle


def gmres_jacobi_longdouble(A, b, tol, maxit, restart):
    """The oracle's algorithm (oracle/lsb_oracle.c orc_gmres_jacobi: GMRES(m), right Jacobi
    preconditioning, x0 = 0, classical Gram-Schmidt twice, Givens rotations, the same stop
    rules) in numpy longdouble.  Returns (x, inner iterations, relres estimate, status)."""
    n, m = A.shape[0], restart
    indptr, cols, vals = A.indptr, A.indices, A.data.astype(LD)
    assert (np.diff(indptr) > 0).all()

    def spmv(v):
        return np.add.reduceat(vals * v[cols], indptr[:-1])
    dinv = 1 / A.diagonal().astype(LD)
    b = b.astype(LD)
    x, ax = np.zeros(n, LD), np.zeros(n, LD)
    V = np.zeros((m + 1, n), LD)
    R, g, y = np.zeros((m, m), LD), np.zeros(m + 1, LD), np.zeros(m, LD)
    cs, sn = np.zeros(m, LD), np.zeros(m, LD)
    status, it, bnorm, thresh, resid = 0, 0, LD(0), LD(0), LD(0)
    cycle = 0
    while status == 0:
        if cycle > 0:
            ax = spmv(x)
        V[0] = b - ax
        beta = np.sqrt(V[0] @ V[0])
        if cycle == 0:
            bnorm, thresh = beta, LD(tol) * beta
        cycle += 1
        resid = beta
        if beta <= thresh or beta == 0:
            status = 1
            break
        if it >= maxit:
            status = 3
            break
        g[:] = 0
        g[0] = beta
        hnorm, jlast = beta, 0
        for j in range(m):
            if status != 0:
                break
            V[j] /= hnorm
            w = spmv(dinv * V[j])
            h = np.zeros(j + 2, LD)
            for _ in range(2):
                hp = V[:j + 1] @ w
                w = w - hp @ V[:j + 1]
                h[:j + 1] += hp
            V[j + 1] = w
            hnorm = np.sqrt(w @ w)
            h[j + 1] = hnorm
            for i in range(j):
                h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], -sn[i] * h[i] + cs[i] * h[i + 1]
            d = np.sqrt(h[j] * h[j] + h[j + 1] * h[j + 1])
            cs[j], sn[j] = (h[j] / d, h[j + 1] / d) if d != 0 else (1, 0)
            h[j] = d
            R[:j + 1, j] = h[:j + 1]
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            resid = abs(g[j + 1])
            jlast = j + 1
            it += 1
            if d == 0:
                status = 2
            elif resid <= thresh or hnorm == 0:
                status = 1
            elif it >= maxit:
                status = 3
        for i in reversed(range(jlast)):
            s = g[i] - R[i, i + 1:jlast] @ y[i + 1:jlast]
            y[i] = s / R[i, i] if R[i, i] != 0 else 0
        x = x + dinv * (y[:jlast] @ V[:jlast])
    return x, it, (resid / bnorm if bnorm > 0 else LD(0)), status


@functools.lru_cache(maxsize=None)
def early_cut(name, k):
    """The fp64 oracle stopped after k inner steps (maxit = k), and its distance d_k from the
    longdouble twin stopped at the same place: (x, relres, d_k of x, d_k of relres)."""
    A = operator(name)
    b = O.rhs(A.shape[0])
    xo, ito, relo, sto = O.gmres_jacobi(A.indptr, A.indices, A.data, b, EARLY_TOL, k, EARLY_RESTART)
    xt, itt, relt, stt = gmres_jacobi_longdouble(A, b, EARLY_TOL, k, EARLY_RESTART)
    assert (sto, ito) == (3, k) and (stt, itt) == (3, k)
    dx = float(np.linalg.norm(xo.astype(LD) - xt) / np.linalg.norm(xt))
    drel = float(abs(LD(relo) - relt) / relt)
    xo.setflags(write=False)
    return xo, relo, dx, drel


@pytest.mark.parametrize("name", ["convdiff", "powerlaw"])
@pytest.mark.parametrize("restart", [5, 30])
def test_oracle_gmres_vs_direct(name, restart):
    A = operators()[name]
    n = A.shape[0]
    b = O.rhs(n)
    x, it, rel, st = O.gmres_jacobi(A.indptr, A.indices, A.data, b, 1e-10, 5000, restart)
    xd = sla.spsolve(A.tocsc(), b)
    assert st == 1 and rel <= 1e-10
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) <= 2e-10  # estimate == true residual
    assert np.linalg.norm(x - xd) / np.linalg.norm(xd) <= 1e-7
    # a symmetric positive definite operator: GMRES agrees with the PCG oracle
    o, c, v = O.lap2d(20, 17)
    xg, itg, _, stg = O.gmres_jacobi(o, c, v, O.rhs(340), 1e-11, 5000, 30)
    xc, _, _, _ = O.pcg_jacobi(o, c, v, O.rhs(340), 1e-12)
    assert stg == 1 and np.linalg.norm(xg - xc) / np.linalg.norm(xc) <= 1e-9


def test_oracle_gmres_stop_rules():
    A = operators()["convdiff"]
    b = O.rhs(A.shape[0])
    x, it, rel, st = O.gmres_jacobi(A.indptr, A.indices, A.data, b, 1e-14, 17, 5)
    assert st == 3 and it == 17
    x, it, rel, st = O.gmres_jacobi(A.indptr, A.indices, A.data, 0 * b, 1e-10, 100, 5)
    assert st == 1 and it == 0 and not x.any()


@pytest.mark.parametrize("name", ["convdiff_odd", "powerlaw_odd"])
def test_early_iterates_oracle_vs_longdouble_twin(name):
    """d_k: how far the fp64 oracle, cut after k inner steps of GMRES(5), is from the same
    algorithm in longdouble -- the scale of what fp64 rounding does to these iterates, and
    the unit test_hip_gmres_early_iterates measures the GPU in.  The twin is anchored on its
    own: a cut finishes the open cycle, so its residual estimate is the true residual of its x."""
    A = operator(name)
    b = O.rhs(A.shape[0])
    for k in EARLY_CUTS:
        xo, relo, dx, drel = early_cut(name, k)
        print("%s k=%d: relres %.3e  d_k(x) %.2e  d_k(relres) %.2e" % (name, k, relo, dx, drel))
        xt, itt, relt, stt = gmres_jacobi_longdouble(A, b, EARLY_TOL, k, EARLY_RESTART)
        Al, bl = A.data.astype(LD), b.astype(LD)
        true = np.linalg.norm(bl - np.add.reduceat(Al * xt[A.indices], A.indptr[:-1])) / np.linalg.norm(bl)
        assert abs(true - relt) <= 1e-12 * relt
        # the oracle follows the exact iterates to many more digits than any comparison below asks for
        assert dx <= 1e-10 and drel <= 1e-10


# ---------------------------------------------------------------------------- GPU

def _matrix(hip, A):
    return hip.Matrix.from_arrays(A.indptr, A.indices, A.data)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["convdiff", "powerlaw", "convdiff_odd", "powerlaw_odd"])
@pytest.mark.parametrize("restart", [5, 30, 32])
def test_hip_gmres_matches_oracle(hip, name, restart):
    A = operator(name)
    n = A.shape[0]
    b = O.rhs(n)
    xo, ito, relo, sto = O.gmres_jacobi(A.indptr, A.indices, A.data, b, 1e-10, 5000, restart)
    s = hip.Solver(_matrix(hip, A), hip.default_opts(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_GMRES,
                                                     restart=restart, tol=1e-10, maxit=5000))
    x, res = s.solve(b)
    x2, res2 = s.solve(b)  # state is reset between solves
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED and res.relres <= 1e-10
    assert abs(int(res.iters) - ito) <= max(2, ito // 50)
    assert res2.iters == res.iters and np.array_equal(x, x2)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-7
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) <= 2e-10
    xd = sla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xd) / np.linalg.norm(xd) <= 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("nvirt", [1, 3])
@pytest.mark.parametrize("name", ["convdiff_odd", "powerlaw_odd"])
def test_hip_gmres_early_iterates(hip, name, nvirt):
    """GMRES(5) cut after k = 1, 2, 4, 5, 6, 11 inner steps (maxit = k, tol 1e-14) on the two
    operators of odd order, on one shard and on three: MAXIT after exactly k steps, and x and
    the residual estimate are the oracle's at the same cut.  No restart has repaired anything
    yet at k <= 5, and a wrong rotation, a wrong y or a wrong update of x shows in x at once.

    The GPU sums in another order than the oracle but in the same precision, so its distance
    from the oracle has the scale of d_k, the oracle's own distance from the longdouble twin
    (test_early_iterates_oracle_vs_longdouble_twin); allowed: 32 d_k, at least 1e-14.
    Measured (d_k on the CPU; the GPU's distance from the oracle on an MI355X, one shard / three):

      operator      k   d_k(x)   GPU x               d_k(relres)  GPU relres
      convdiff_odd  1   1.2e-16  3.1e-16 / 5.3e-17   1.7e-17      0       / 1.2e-16
      convdiff_odd  2   5.6e-16  3.1e-16 / 7.0e-16   7.7e-17      2.5e-16 / 2.5e-16
      convdiff_odd  4   4.0e-16  2.3e-16 / 7.6e-16   3.0e-17      1.4e-16 / 5.4e-16
      convdiff_odd  5   1.9e-16  4.0e-16 / 3.2e-16   9.0e-17      1.4e-16 / 7.0e-16
      convdiff_odd  6   1.5e-16  3.1e-16 / 4.2e-16   5.5e-18      1.4e-16 / 0
      convdiff_odd  11  2.0e-16  2.3e-16 / 3.1e-16   1.0e-16      1.6e-16 / 3.2e-16
      powerlaw_odd  1   6.9e-16  5.0e-16 / 5.0e-16   5.0e-16      5.0e-16 / 5.0e-16
      powerlaw_odd  2   3.4e-16  2.6e-16 / 2.6e-16   7.5e-16      5.8e-16 / 5.8e-16
      powerlaw_odd  4   2.3e-16  2.6e-16 / 2.6e-16   2.2e-16      4.5e-16 / 4.5e-16
      powerlaw_odd  5   1.9e-16  2.2e-16 / 2.3e-16   4.8e-16      8.5e-16 / 8.5e-16
      powerlaw_odd  6   1.1e-16  1.2e-16 / 1.2e-16   2.3e-15      4.8e-15 / 4.0e-15
      powerlaw_odd  11  9.0e-17  8.7e-17 / 8.7e-17   3.4e-13      3.5e-13 / 1.7e-13

    (The estimate of powerlaw_odd at k = 11 is 1.6e-5 of ||b||: the restart residual b - A x
    loses four to five digits to cancellation, in the oracle as on the GPU.)"""
    A = operator(name)
    b = O.rhs(A.shape[0])
    M = _matrix(hip, A)
    fails = []
    for k in EARLY_CUTS:
        xo, relo, dx, drel = early_cut(name, k)
        kw = dict(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_GMRES, restart=EARLY_RESTART, tol=EARLY_TOL, maxit=k)
        if nvirt > 1:
            kw["nvirt"] = nvirt
        s = hip.Solver(M, hip.default_opts(**kw))
        x, res = s.solve(b)
        s.destroy()
        assert res.status == hip.STATUS_MAXIT and res.iters == k
        ex = float(np.linalg.norm(x - xo) / np.linalg.norm(xo))
        er = abs(res.relres - relo) / relo
        print("%s nvirt=%d k=%d: |x - oracle| %.2e (d_k %.2e)  |relres - oracle| %.2e (d_k %.2e)"
              % (name, nvirt, k, ex, dx, er, drel))
        if not (ex <= max(32 * dx, 1e-14) and er <= max(32 * drel, 1e-14)):
            fails.append((k, ex, er))
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("name,nvirt", [("convdiff", 2), ("convdiff", 5), ("powerlaw", 3)])
def test_hip_gmres_over_row_range_shards(hip, name, nvirt):
    """GMRES(m) with the operator split into row-range shards: halo exchange in
    front of every SpMV, ONE all-reduce per Gram-Schmidt pass (all j+1
    coefficients together) and one per norm; every shard keeps its own copy of
    the small state and must take the same decisions."""
    A = operators()[name]
    b = O.rhs(A.shape[0])
    M = _matrix(hip, A)
    kw = dict(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_GMRES, restart=20, tol=1e-10, maxit=5000)
    s1 = hip.Solver(M, hip.default_opts(**kw))
    x1, r1 = s1.solve(b)
    s1.destroy()
    sp_ = hip.Solver(M, hip.default_opts(nvirt=nvirt, **kw))
    xp, rp = sp_.solve(b)
    xq, rq = sp_.solve(b)
    sp_.destroy()
    assert rp.status == hip.STATUS_CONVERGED and abs(int(rp.iters) - int(r1.iters)) <= 2
    assert rq.iters == rp.iters and np.array_equal(xp, xq)
    assert np.linalg.norm(xp - x1) / np.linalg.norm(x1) <= 1e-8
    assert np.linalg.norm(b - A @ xp) / np.linalg.norm(b) <= 2e-10


@pytest.mark.gpu
def test_hip_gmres_on_the_raw_reference_matrix(hip, matrix_path, golden_x, golden_meta):
    """The file matrix as-is (unsymmetric by 3.6e-7): GMRES solves A x = b, which
    is NOT CHOLMOD's operator -- the answer differs from the golden vector by
    the documented 6.6e-7, and matches a direct solve of the raw matrix."""
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    b = O.rhs(n)
    s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_GMRES, restart=32,
                                       tol=1e-12, maxit=20000))
    x, res = s.solve(b)
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED
    M = sp.csr_matrix((A.vals, A.cols.astype(np.int64) - 1, A.offs.astype(np.int64)), shape=(n, n))
    xd = sla.spsolve(M.tocsc(), b)
    assert np.linalg.norm(x - xd) / np.linalg.norm(xd) <= 1e-9
    xg = golden_x("xn3b_A_18")
    err = np.linalg.norm(x - xg) / np.linalg.norm(xg)
    assert abs(err - golden_meta["matrices"]["xn3b_A_18"]["raw_vs_S"]) <= 1e-8
    # with the CHOLMOD operator GMRES reaches the golden vector like PCG does
    s = hip.Solver(A, hip.default_opts(krylov=hip.KRYLOV_GMRES, restart=32, tol=1e-12))
    x, res = s.solve(b)
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED
    assert np.linalg.norm(x - xg) / np.linalg.norm(xg) <= 1e-10


@pytest.mark.gpu
def test_hip_gmres_stop_rules(hip):
    A = operators()["convdiff"]
    b = O.rhs(A.shape[0])
    M = _matrix(hip, A)
    s = hip.Solver(M, hip.default_opts(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_GMRES, restart=5,
                                       tol=1e-14, maxit=17))
    x, res = s.solve(b)
    assert res.status == hip.STATUS_MAXIT and res.iters == 17
    xo, ito, _, sto = O.gmres_jacobi(A.indptr, A.indices, A.data, b, 1e-14, 17, 5)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-8  # same partial solution
    x, res = s.solve(np.zeros_like(b))
    assert res.status == hip.STATUS_CONVERGED and res.iters == 0 and not x.any()
    s.destroy()
