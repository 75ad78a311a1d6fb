"""Solves from an initial guess: lsb_hip_solver_solve_x0[_dev], solve_multi_x0_dev and start_relres
(hip_solve.c: solve_x0_core and k_x0_start; hip_mrhs_drv.c and hip_mrhs_x0.hip: the in-place start of a batch).

The yardsticks: the cold solve of the same solver (x0 = 0 must reproduce it), the golden solution, the
extended-precision residual `relres_exact` of test_mrhs.py, and the numpy restatement `pcg_x0` below of the
semantics -- the stop rule stays relative to ||b||, b = 0 gives x = 0, an x0 within the tolerance is returned
untouched."""
import ctypes as C
import fractions
import functools
import math
import os
import re

import numpy as np
import pytest

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from oracle import oracle as O
from test_mrhs import _block, _host, _lap2d, columns, eleven, oracle_operator, relerr, relres_exact

CONVERGED, BREAKDOWN, MAXIT = 1, 2, 3
FOUR = ("lsb_hip_solver_solve_x0", "lsb_hip_solver_solve_x0_dev", "lsb_hip_solver_solve_multi_x0_dev",
        "lsb_hip_solver_start_relres")


def pcg_x0(S, b, x0, tol, maxit=20000):
    """Jacobi-PCG for S x = b from x0 as a correction solve S e = b - S x0 from e = 0, stopped at
    ||r|| <= tol ||b|| (never relative to ||b - S x0||).  -> dict(x, iters, status, relres, start)."""
    d = 1.0 / S.diagonal()
    bb = float(b @ b)
    if bb == 0.0:
        return dict(x=np.zeros(len(b)), iters=0, status=CONVERGED, relres=0.0, start=0.0)
    r = b - S @ x0
    rr = float(r @ r)
    start = math.sqrt(rr / bb)
    if tol > 0.0 and rr <= tol * tol * bb:
        return dict(x=x0, iters=0, status=CONVERGED, relres=start, start=start)
    e = np.zeros(len(b))
    p = d * r
    rz = float(r @ p)
    it, status = 0, MAXIT
    while it < maxit:
        q = S @ p
        pq = float(p @ q)
        if pq == 0.0 or not np.isfinite(pq):
            status = BREAKDOWN
            break
        alpha = rz / pq
        e += alpha * p
        r -= alpha * q
        z = d * r
        rz_new, rr = float(r @ z), float(r @ r)
        it += 1
        if rr <= tol * tol * bb:
            status = CONVERGED
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return dict(x=x0 + e, iters=it, status=status, relres=math.sqrt(rr / bb), start=start)


def relres_rational(S, x, b):
    """||b - S x|| / ||b|| in exact rational arithmetic (every double is an integer over a power of two), rounded
    once to a double before the square root: good to 2^-52 of itself wherever the residual sits."""
    def dyadic(v):
        n, d = float(v).as_integer_ratio()
        return n, d.bit_length() - 1

    def add(acc, term):  # (N, k) stands for N / 2^k
        (N, k), (n, j) = acc, term
        if j > k:
            N, k = N << (j - k), j
        return N + (n << (k - j)), k

    S = S.tocsr()
    rr, bb = (0, 0), (0, 0)
    for i in range(S.shape[0]):
        n, k = dyadic(b[i])
        bb = add(bb, (n * n, 2 * k))
        acc = (n, k)
        for j in range(S.indptr[i], S.indptr[i + 1]):
            (vn, vk), (xn, xk) = dyadic(S.data[j]), dyadic(x[S.indices[j]])
            acc = add(acc, (-vn * xn, vk + xk))
        rr = add(rr, (acc[0] * acc[0], 2 * acc[1]))
    return math.sqrt(float(fractions.Fraction(rr[0] << bb[1], bb[0] << rr[1])))


@functools.lru_cache(maxsize=None)
def _stages(path):
    """the restatement on b_i = i: cold to 1e-12, cold to 1e-6, warm from that to 1e-12"""
    _, S = oracle_operator(path)
    b = O.rhs(S.shape[0])
    zero = np.zeros(len(b))
    cold12, cold6 = pcg_x0(S, b, zero, 1e-12), pcg_x0(S, b, zero, 1e-6)
    return S, b, cold12, cold6, pcg_x0(S, b, cold6["x"], 1e-12)


# ------------------------------------------------------------------------------------ without a GPU
def test_the_four_functions_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in FOUR:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib.hip, name)
    for m in ("solve", "solve_dev", "solve_multi_dev", "start_relres"):
        assert callable(getattr(la.Solver, m))
    # before hip_cdna4_init the three solves answer 1 ahead of any look at their arguments; on a process that has
    # initialised the backend the null arguments are what is refused: 2
    up = int(lib.hip.lsb_hip_is_initialized())
    res = _lib.Result()
    assert lib.lsb_hip_solver_solve_x0(None, None, None, C.byref(res)) == (2 if up else 1)
    assert lib.lsb_hip_solver_solve_x0_dev(None, None, None, C.byref(res)) == (2 if up else 1)
    assert lib.lsb_hip_solver_solve_multi_x0_dev(None, 1, None, 0, None, 0, C.byref(res)) == (2 if up else 1)
    out = (C.c_double * 1)()
    assert lib.lsb_hip_solver_start_relres(None, 1, out) == 2


@pytest.mark.parametrize("name", ["xn3b_A_18", "tj7a_A_18", "xn3b_A_10"])
def test_cpu_restatement_a_warm_start_saves_iterations(name, matrix_path):
    """From the restatement's own 1e-6 solution to 1e-12 (seen: 135 / 267, 138 / 354, 160 / 321 iterations; the
    recomputed residual 9.2e-13 .. 9.7e-13 with numpy's dot, 1.02e-12 with another summation order on tj7a -- the
    recurrence residual drifts past tol there, hence 2 x)."""
    S, b, cold12, cold6, warm = _stages(matrix_path(name))
    true = relres_exact(S, warm["x"], b)
    print(name, "cold", cold12["iters"], cold6["iters"], "warm", warm["iters"], "recomputed", true,
          "to the cold x", relerr(warm["x"], cold12["x"]))
    assert cold12["status"] == cold6["status"] == warm["status"] == CONVERGED
    assert warm["iters"] <= 0.7 * cold12["iters"]
    assert true <= 2e-12
    # the early exits of the restatement itself
    assert pcg_x0(S, 0 * b, cold6["x"], 1e-12)["iters"] == 0 and not pcg_x0(S, 0 * b, cold6["x"], 1e-12)["x"].any()
    again = pcg_x0(S, b, cold12["x"], 1e-8)
    assert again["iters"] == 0 and again["x"] is cold12["x"] and again["start"] <= 1e-11


# ------------------------------------------------------------------------------------ on the GPU
def _dev(v):
    import torch
    return torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0")  # (a copy: v may be read-only)


def _opts(hip, kw):
    return hip.default_opts(**{k: getattr(hip, v) if isinstance(v, str) else v for k, v in kw.items()})


def _cold(s, b):
    import torch
    d_x = torch.full((len(b),), -3.0, dtype=torch.float64, device="cuda:0")
    res = s.solve_dev(_dev(b), d_x)
    return d_x.cpu().numpy(), res


def _warm(s, b, x0):
    d_x = _dev(x0)
    res = s.solve_dev(_dev(b), d_x, warm=True)
    return d_x.cpu().numpy(), res


def _start_rc(s, nrhs=1):
    out = (C.c_double * max(nrhs, 1))()
    return _lib.load().lsb_hip_solver_start_relres(s._h, nrhs, out)


@functools.lru_cache(maxsize=None)
def _xn3b(path):
    """the operator, b_i = i and the solutions of the default solver at 1e-6 and 1e-12, computed once"""
    _, S = oracle_operator(path)
    b = O.rhs(S.shape[0])
    out = {}
    for tol in (1e-6, 1e-12):
        s = la.Solver(la.lsbench_matrix_read(path), la.default_opts(tol=tol))
        out[tol], res = _cold(s, b)
        assert res.status == CONVERGED
        s.destroy()
    for v in out.values():
        v.setflags(write=False)
    return S, b, out[1e-6], out[1e-12]


AMG = dict(precond="PRECOND_AMG")
X0_ZERO = {
    "jacobi": {}, "graph": dict(use_graph=1), "nograph": dict(use_graph=0), "fsai": dict(precond="PRECOND_FSAI"),
    "amg": AMG, "amg-fp32": dict(precond="PRECOND_AMG", amg_precision="AMG_PREC_FP32"),
    "cheb": dict(precond="PRECOND_CHEBYSHEV"), "pcg1": dict(krylov="KRYLOV_PCG1"), "gmres": dict(krylov="KRYLOV_GMRES", restart=32),
    "bicgstab": dict(krylov="KRYLOV_BICGSTAB"),
    "richardson": dict(krylov="KRYLOV_RICHARDSON", precond="PRECOND_AMG", maxit=2, tol=0.0),
    "mixed": dict(precision="PREC_MIXED"), "nvirt2": dict(nvirt=2), "reorder": dict(reorder=1),
}


def _check_x0_zero(s, b):
    xc, rc = _cold(s, b)
    assert _start_rc(s) == 2  # the last solve was a cold one
    xw, rw = _warm(s, b, np.zeros(len(b)))
    print("cold", rc.iters, rc.status, rc.relres, "warm", rw.iters, rw.status, rw.relres)
    assert np.array_equal(xw, xc)
    assert (rw.iters, rw.status, rw.relres) == (rc.iters, rc.status, rc.relres)
    assert s.start_relres()[0] == 1.0
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(X0_ZERO))
def test_x0_zero_is_the_cold_solve(hip, what, matrix_path):
    kw = dict(tol=1e-10)
    kw.update(X0_ZERO[what])
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    s = hip.Solver(A, _opts(hip, kw))
    rc = _check_x0_zero(s, O.rhs(A.nrows))
    s.destroy()
    if what == "richardson":
        assert rc.status == MAXIT and rc.iters == 2
    else:
        assert rc.status == CONVERGED and rc.iters > 17


@pytest.mark.gpu
def test_x0_zero_under_verify(hip, matrix_path):
    """What the header promises where the two solves recompute b - S x differently (the cold one with the fp64 SpMV,
    the warm one in twice the working precision): no correction run either way at this tolerance, so x, iters and
    status are the cold solve's, and relres = true_relres differ by no more than the forward bound of the fp64
    residual, (len + 2) 2^-53 || |S||x| + |b| || / ||b|| with len the longest row."""
    path = matrix_path("xn3b_A_18")
    _, S = oracle_operator(path)
    b = O.rhs(S.shape[0])
    s = hip.Solver(hip.lsbench_matrix_read(path), hip.default_opts(tol=1e-10, verify=1))
    xc, rc = _cold(s, b)
    xw, rw = _warm(s, b, np.zeros(len(b)))
    s.destroy()
    bound = (int(np.diff(S.tocsr().indptr).max()) + 2) * 2.0 ** -53 * \
        float(np.linalg.norm(abs(S) @ np.abs(xc) + np.abs(b)) / np.linalg.norm(b))
    print("cold", rc.iters, rc.corrections, rc.true_relres, "warm", rw.iters, rw.corrections, rw.true_relres,
          "bound", bound, "exact", relres_exact(S, xw, b))
    assert rc.status == rw.status == CONVERGED and rc.corrections == rw.corrections == 0
    assert np.array_equal(xw, xc) and rw.iters == rc.iters
    assert rw.relres == rw.true_relres and rc.relres == rc.true_relres
    assert 0.0 <= rw.true_relres <= 1e-10 and abs(rw.true_relres - rc.true_relres) <= bound
    assert abs(rw.true_relres - relres_exact(S, xw, b)) <= 1e-3 * rw.true_relres


@pytest.mark.gpu
def test_x0_zero_is_the_cold_solve_on_the_raw_grid(hip):
    """the sliced-ELL and template paths"""
    s = hip.Solver(hip.lsbench_matrix_synth("lap2d:nx=60,ny=45"), hip.default_opts(op_mode=hip.OP_RAW, tol=1e-10))
    rc = _check_x0_zero(s, O.rhs(60 * 45))
    s.destroy()
    assert rc.status == CONVERGED


@pytest.mark.gpu
def test_x0_zero_is_the_cold_solve_on_the_padded_grid(hip):
    """the two-launch form of a line-padded solver; then a start from that solution costs nothing"""
    n = 1000 * 1000
    s = hip.Solver(hip.lsbench_matrix_synth("lap2d:nx=1000,ny=1000"), hip.default_opts(op_mode=hip.OP_RAW, tol=1e-6))
    assert s.padded > 0 and s.n_local == n
    b = O.rhs(n)
    rc = _check_x0_zero(s, b)
    assert rc.status == CONVERGED
    s.destroy()


@pytest.mark.gpu
def test_a_good_x0_costs_nothing(hip, matrix_path):
    import torch
    path = matrix_path("xn3b_A_18")
    S, b, _, x12 = _xn3b(path)
    n = len(b)
    s = hip.Solver(hip.lsbench_matrix_read(path), hip.default_opts(tol=1e-8))
    for off in (0, 1):  # a 16-byte aligned x, and one that is only 8-byte aligned
        buf = torch.zeros(n + 2, dtype=torch.float64, device="cuda:0")
        d_x = buf[off:off + n]
        assert d_x.data_ptr() % 16 == 8 * off
        d_x.copy_(_dev(x12))
        res = s.solve_dev(_dev(b), d_x, warm=True)
        assert res.status == CONVERGED and res.iters == 0
        assert d_x.cpu().numpy().tobytes() == x12.tobytes()
        assert 0.0 < s.start_relres()[0] <= 1e-11 and res.relres == s.start_relres()[0]
    xh, resh = s.solve(b, x0=x12)  # host buffers
    assert resh.iters == 0 and xh.tobytes() == x12.tobytes()
    s.destroy()
    # a re-numbered solver leaves it where it is too
    s = hip.Solver(hip.lsbench_matrix_read(path), hip.default_opts(tol=1e-8, reorder=1))
    xw, res = _warm(s, b, x12)
    s.destroy()
    assert res.status == CONVERGED and res.iters == 0 and xw.tobytes() == x12.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["jacobi", "fsai", "amg"])
def test_two_stages(hip, what, matrix_path, golden_x):
    path = matrix_path("xn3b_A_18")
    S, b, x6, _ = _xn3b(path)
    s = hip.Solver(hip.lsbench_matrix_read(path), _opts(hip, dict(tol=1e-12, **X0_ZERO[what])))
    _, rc = _cold(s, b)
    xw, rw = _warm(s, b, x6)
    true = relres_exact(S, xw, b)
    print(what, "cold", rc.iters, "warm", rw.iters, rw.relres, "recomputed", true, "start", s.start_relres()[0])
    assert rw.status == CONVERGED
    assert true <= 2e-12
    assert relerr(xw, golden_x("xn3b_A_18")) <= 1e-10
    assert rw.iters < rc.iters
    assert rw.relres <= 1e-12
    if what == "jacobi":
        # a different rounding of r0 can move the crossing of the stop test by an iteration or two, not more
        ref = pcg_x0(S, b, x6, 1e-12)
        print("restatement", ref["iters"])
        assert abs(int(rw.iters) - ref["iters"]) <= 2
    xw2, rw2 = _warm(s, b, x6)  # a second call repeats the first
    s.destroy()
    assert xw2.tobytes() == xw.tobytes() and (rw2.iters, rw2.relres) == (rw.iters, rw.relres)


@pytest.mark.gpu
def test_zero_rhs_gives_zero(hip, matrix_path):
    path = matrix_path("xn3b_A_18")
    A = hip.lsbench_matrix_read(path)
    x0 = np.random.default_rng(3).standard_normal(A.nrows)
    for kw in ({}, dict(reorder=1)):
        s = hip.Solver(A, hip.default_opts(tol=1e-12, **kw))
        xw, rw = _warm(s, np.zeros(A.nrows), x0)
        assert rw.status == CONVERGED and rw.iters == 0 and not xw.any()
        assert s.start_relres()[0] == 0.0
        s.destroy()


@pytest.mark.gpu
def test_maxit_caps_the_iterations_from_x0(hip, matrix_path):
    """relres is reported relative to ||b||: the scaling back from ||b - S x0|| is in"""
    path = matrix_path("xn3b_A_18")
    S, b, x6, _ = _xn3b(path)
    s = hip.Solver(hip.lsbench_matrix_read(path), hip.default_opts(tol=1e-12, maxit=17))
    xw, rw = _warm(s, b, x6)
    s.destroy()
    true = relres_exact(S, xw, b)
    print("relres", rw.relres, "recomputed", true)
    assert rw.status == MAXIT and rw.iters == 17
    assert abs(rw.relres - true) <= 1e-3 * true


@pytest.mark.gpu
def test_start_relres(hip, matrix_path):
    path = matrix_path("xn3b_A_18")
    S, b, _, _ = _xn3b(path)
    x0 = np.random.default_rng(5).standard_normal(len(b))
    s = hip.Solver(hip.lsbench_matrix_read(path), hip.default_opts(tol=1e-8))
    _warm(s, b, x0)
    got, ref = s.start_relres()[0], relres_exact(S, x0, b)
    print("start_relres", got, "numpy", ref)
    assert abs(got - ref) <= 1e-10 * ref
    assert _start_rc(s, 2) == 2  # the last solve had one column
    _cold(s, b)
    assert _start_rc(s) == 2
    with pytest.raises(_lib.LsbenchHipError):
        s.start_relres()
    s.destroy()


@pytest.mark.gpu
def test_verify_from_x0(hip, matrix_path):
    """opts.verify on the original (b, x) behind a warm start.  At this level -- u || |S||x| + |b| || / ||b|| =
    7.8e-14 on this operator -- a residual formed by an fp64 SpMV is mostly its own rounding (8.858e-14 against
    8.768e-14 exact: 1 % off; numpy's fp64 value is 3 % off, see relres_exact), so behind a warm start opts.verify
    recomputes b - S x off the CSR arrays as in twice the working precision (k_resid_csr2), as the batches do."""
    path = matrix_path("xn3b_A_18")
    S, b, x6, _ = _xn3b(path)
    tol = 1e-13
    s = hip.Solver(hip.lsbench_matrix_read(path), hip.default_opts(tol=tol, verify=1))
    xw, rw = _warm(s, b, x6)
    s.destroy()
    cpu = relres_exact(S, xw, b)
    print("iters", rw.iters, "corrections", rw.corrections, "true_relres", rw.true_relres, "cpu, exact", cpu,
          "cpu, fp64", float(np.linalg.norm(b - S @ xw) / np.linalg.norm(b)))
    assert rw.status == CONVERGED and 0.0 <= rw.true_relres <= tol
    assert abs(rw.true_relres - cpu) <= 1e-3 * cpu


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["bicgstab", "richardson"])
def test_other_drivers_verify_from_x0(hip, what, matrix_path):
    """Their cold solve restarts in place on the recomputed residual; behind a warm start the same contract --
    converged means the recomputed residual meets tol -- is kept by correction solves."""
    if what == "bicgstab":
        path = matrix_path("xn3b_A_18")
        S, b, x6, _ = _xn3b(path)
        M, kw, tol = hip.lsbench_matrix_read(path), dict(krylov="KRYLOV_BICGSTAB"), 1e-12
    else:
        S, b = _lap2d(60, 45), O.rhs(60 * 45)
        M = hip.lsbench_matrix_synth("lap2d:nx=60,ny=45")
        kw, tol = dict(op_mode=hip.OP_RAW, krylov="KRYLOV_RICHARDSON", precond="PRECOND_AMG", maxit=2000), 1e-10
        s = hip.Solver(M, _opts(hip, dict(tol=1e-6, **kw)))
        x6, r6 = _cold(s, b)
        s.destroy()
        assert r6.status == CONVERGED
    s = hip.Solver(M, _opts(hip, dict(tol=tol, verify=1, **kw)))
    _, rc = _cold(s, b)
    xw, rw = _warm(s, b, x6)
    s.destroy()
    cpu = relres_exact(S, xw, b)
    print(what, "cold", rc.iters, "warm", rw.iters, "corrections", rw.corrections, "true_relres", rw.true_relres,
          "cpu, exact", cpu)
    assert rc.status == CONVERGED and rw.status == CONVERGED
    assert 0.0 <= rw.true_relres <= tol and rw.relres == rw.true_relres and rw.corrections <= 6
    assert cpu <= 2 * tol
    assert rw.iters < rc.iters


def _solve_block(s, B, X0, warm, fill=-7.0):
    import torch
    n, k = B.shape
    d_B = _block(B, n + 5)
    d_X = _block(X0, n + 7, fill=fill)
    res = s.solve_multi_dev(d_B, d_X, warm=warm)
    assert bool((d_X[:, n:] == fill).all())  # the slack behind a column is the caller's
    return _host(d_X, n), res


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["jacobi", "amg"])
def test_blocks(hip, what, matrix_path):
    path = matrix_path("xn3b_A_18")
    _, S = oracle_operator(path)
    n = S.shape[0]
    B = columns(S)[:, [0, 2, 3, 1, 4]]  # i, S.1, e0, zero, randn
    tol = 1e-12
    kw = X0_ZERO[what]
    A = hip.lsbench_matrix_read(path)
    # the starting points: column 1 from a solver at 1e-12 whose "converged" is the recomputed residual's (the
    # recurrence's may sit a few per cent above it), column 2 from one at 1e-6
    s = hip.Solver(A, _opts(hip, dict(tol=tol, verify=1, **kw)))
    X12, _ = _solve_block(s, B, np.zeros_like(B), False)
    s.destroy()
    s = hip.Solver(A, _opts(hip, dict(tol=1e-6, **kw)))
    X6, _ = _solve_block(s, B, np.zeros_like(B), False)
    s.destroy()
    rng = np.random.default_rng(9)
    X0 = np.stack([np.zeros(n), X12[:, 1], X6[:, 2], rng.standard_normal(n), rng.standard_normal(n)], axis=1)

    s = hip.Solver(A, _opts(hip, dict(tol=tol, **kw)))
    Xc, rc = _solve_block(s, B, np.zeros_like(B), False)
    assert _start_rc(s, 5) == 2
    Xw, rw = _solve_block(s, B, X0, True)
    start = s.start_relres(5)
    print([(r.iters, r.status) for r in rc], [(r.iters, r.status) for r in rw], start)
    # x0 = 0: the column of the cold call
    assert np.array_equal(Xw[:, 0], Xc[:, 0]) and (rw[0].iters, rw[0].status, rw[0].relres) == (rc[0].iters, rc[0].status, rc[0].relres)
    # a good x0 costs nothing
    assert rw[1].status == CONVERGED and rw[1].iters == 0 and Xw[:, 1].tobytes() == X0[:, 1].tobytes()
    assert rw[2].status == CONVERGED and 0 < rw[2].iters < rc[2].iters
    if what == "jacobi":
        ref = pcg_x0(S, B[:, 2], X0[:, 2], tol)
        print("restatement", ref["iters"])
        assert abs(int(rw[2].iters) - ref["iters"]) <= 2
    assert rw[3].status == CONVERGED and rw[3].iters == 0 and not Xw[:, 3].any()
    assert rw[4].status == CONVERGED and relerr(Xw[:, 4], Xc[:, 4]) <= 50 * tol
    # the starting residuals, 1e-10 relative in every column.  The reference of the columns that start far from the
    # solution is the extended-precision residual, good to about 2^-64 len ||b|| / ||r|| of itself; for the one that
    # starts at 1e-12 that would be 1e-6, so its reference is formed in exact rational arithmetic
    assert start[0] == 1.0 and start[3] == 0.0
    for c in (1, 2, 4):
        ref = (relres_rational if c == 1 else relres_exact)(S, X0[:, c], B[:, c])
        print("column", c, "start_relres", start[c], "reference", ref)
        assert abs(start[c] - ref) <= 1e-10 * ref
    assert start[1] <= tol
    Xw2, rw2 = _solve_block(s, B, X0, True)  # run to run
    assert Xw2.tobytes() == Xw.tobytes() and [r.iters for r in rw2] == [r.iters for r in rw]

    # a batch of 8 and one of 3, x0 = 0 in all: the cold call
    B11 = eleven(S)
    Xc, rc = _solve_block(s, B11, np.zeros_like(B11), False)
    Xw, rw = _solve_block(s, B11, np.zeros_like(B11), True)
    s.destroy()
    assert np.array_equal(Xw, Xc)
    assert [(r.iters, r.status, r.relres) for r in rw] == [(r.iters, r.status, r.relres) for r in rc]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(precond="PRECOND_FSAI"), dict(nvirt=2), dict(krylov="KRYLOV_GMRES")],
                         ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_refusals(hip, kw, matrix_path):
    import torch
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    s = hip.Solver(A, _opts(hip, kw))
    lib = _lib.load()
    d_B = torch.ones(2, n, dtype=torch.float64, device="cuda:0")
    d_X = torch.full((2, n), 0.25, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_multi_x0_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
    assert bool((d_X == 0.25).all())
    assert lib.lsb_hip_solver_solve_x0_dev(s._h, d_B.data_ptr(), None, res) == 2
    s.destroy()


@pytest.mark.gpu
def test_null_arguments_on_an_initialised_process(hip, matrix_path):
    import torch
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    s = hip.Solver(A, hip.default_opts())
    lib = _lib.load()
    assert int(lib.hip.lsb_hip_is_initialized())
    d_B = torch.ones(2, n, dtype=torch.float64, device="cuda:0")
    d_X = torch.full((2, n), 0.25, dtype=torch.float64, device="cuda:0")
    b, x = np.ones(n), np.full(n, 0.25)
    res = (_lib.Result * 2)()
    out = (C.c_double * 2)()
    for h, pb, px in ((None, b.ctypes.data, x.ctypes.data), (s._h, None, x.ctypes.data), (s._h, b.ctypes.data, None)):
        assert lib.lsb_hip_solver_solve_x0(h, pb, px, res) == 2
    for h, pb, px in ((None, d_B.data_ptr(), d_X.data_ptr()), (s._h, None, d_X.data_ptr()), (s._h, d_B.data_ptr(), None)):
        assert lib.lsb_hip_solver_solve_x0_dev(h, pb, px, res) == 2
        assert lib.lsb_hip_solver_solve_multi_x0_dev(h, 2, pb, n, px, n, res) == 2
    assert lib.lsb_hip_solver_solve_multi_x0_dev(s._h, 0, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
    assert lib.lsb_hip_solver_solve_multi_x0_dev(s._h, 2, d_B.data_ptr(), n - 1, d_X.data_ptr(), n, res) == 2
    assert lib.lsb_hip_solver_solve_multi_x0_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n - 1, res) == 2
    assert lib.lsb_hip_solver_start_relres(s._h, 1, None) == 2 and lib.lsb_hip_solver_start_relres(None, 1, out) == 2
    assert bool((d_X == 0.25).all()) and (x == 0.25).all()
    s.destroy()
