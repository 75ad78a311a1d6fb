"""Multicolour Gauss-Seidel smoothing in the AMG V-cycle (opts.amg_smoother = AMG_SMOOTH_MCGS, --amg-smoother mcgs).

The smoother is restated here in numpy on top of test_amg.Hier (`Mcgs`).  On a level with matrix A:

    colouring   greedy: rows in ascending order, each takes the smallest colour that none of its stored
                off-diagonal neighbours already holds (`colour`)
    step c      on (x, b), in place, the rows i of colour c only:  x_i <- x_i + (b_i - sum_j a_ij x_j) / a_ii
    sweeps      forward = colours 0 .. C - 1, backward = C - 1 .. 0
    cycle       nu forward sweeps from the zero guess, the residual, the coarse correction, x += P e, nu backward sweeps
    cap         a level whose colouring has more than `cap` colours (16) keeps the l1-Jacobi sweeps of Hier.vcycle

`M32` is its float32 twin in the manner of test_amg_f32.H32.

CPU: lsb_amg_colour against the rule, the colour-sorted copy, the check and its refusals, the numpy cycle is a
symmetric positive definite preconditioner with lambda_max(M^-1 S) <= 1, AMG-PCG with it takes fewer iterations than
with l1-Jacobi, the surface.  GPU: one application against numpy in fp64 and fp32, solves, Richardson and a warm
start, re-numbered solvers, the refusals and the driver."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lsbench_amd as la
from conftest import ROOT, SPD
from lsbench_amd import _lib
from oracle import oracle as O
from test_amg import GRIDS, Hier, as_matrix, operator, pcg

MCGS = la.AMG_SMOOTH_MCGS  # (without the feature: no such constant, every test of this file fails here)
CAP = 16
F = np.float32
SYMBOLS = ("lsb_amg_colour", "lsb_csr_mcgs", "lsb_mcgs_free", "lsb_mcgs_check", "lsb_hip_solver_amg_colours")
# (operator, tol) -> AMG-PCG iterations of b_i = i at nu = 1 / 2: l1-Jacobi, mcgs with the cap at 16, and the colours
# of the smoothed levels, from the numpy restatement when the smoother was proposed (printed beside what it gives now)
TABLE = {("xn3b_A_18", 1e-12): ((128, 91), (66, 40), (16, 39)),
         ("tj7a_A_18", 1e-12): ((116, 82), (65, 39), (12, 33)),
         ("tj7a_A_12", 1e-12): ((120, 85), (67, 41), (12, 34)),
         ("lap2d:nx=130,ny=70", 1e-10): ((23, 16), (14, 11), (2, 4)),
         ("lap2d:nx=300,ny=300", 1e-8): ((23, 17), (14, 12), (2, 5, 10)),
         ("lap3d:nx=24,ny=20,nz=18", 1e-10): ((27, 20), (17, 12), (2, 15))}
LAP3D = "lap3d:nx=24,ny=20,nz=18"
# one application on the GPU: mixed levels with a colouring exactly at the cap and ragged colours; three smoothed
# levels; two levels whose rows are no multiple of a workgroup's; one level, nothing to smooth
CYCLES = ["xn3b_A_18", "lap2d:nx=300,ny=300", "lap3d:nx=9,ny=8,nz=7", "lap2d:nx=12,ny=10"]


# ------------------------------------------------------------------------------------ the restatement
def colour(A):
    """the greedy rule on the stored pattern of a scipy CSR: (colour of every row, number of colours)"""
    n = A.shape[0]
    col = -np.ones(n, np.int64)
    ip, ix = A.indptr, A.indices
    for i in range(n):
        nb = ix[ip[i]:ip[i + 1]]
        used = col[nb[nb != i]]
        used = set(used[used >= 0].tolist())
        c = 0
        while c in used:
            c += 1
        col[i] = c
    return col, int(col.max()) + 1 if n else 0


class Mcgs:
    """The V-cycle of a test_amg.Hier with multicolour Gauss-Seidel on the levels of at most `cap` colours."""

    def __init__(self, H, cap=CAP, dtype=np.float64):
        self.H, self.cap, self.dt = H, cap, dtype
        self.A = [A.astype(dtype) for A in H.A]
        self.P = [P.astype(dtype) for P in H.P]
        self.R = [R.astype(dtype) for R in H.R]
        self.cinv = H.cinv.astype(dtype)
        self.minv = [m.astype(dtype) for m in H.minv]
        self.dinv = [(1.0 / A.diagonal()).astype(dtype) for A in H.A]
        self.col, self.found, self.rows, self.sub = [], [], [], []
        for A in H.A[:-1]:
            col, nc = colour(A)
            self.col.append(col)
            self.found.append(nc)
            rows = [np.nonzero(col == k)[0] for k in range(nc)] if nc <= cap else []
            self.rows.append(rows)
            self.sub.append([A[r].astype(dtype) for r in rows])
        self.ncol = [len(r) for r in self.rows]  # per smoothed level: the colours, 0 beyond the cap

    def sweep(self, l, x, b, backward):
        order = range(self.ncol[l] - 1, -1, -1) if backward else range(self.ncol[l])
        dinv = self.dinv[l]
        for k in order:
            r = self.rows[l][k]
            x[r] = x[r] + dinv[r] * (b[r] - self.sub[l][k] @ x)
        return x

    def vcycle(self, b, nu=1):
        def rec(l, b):
            if l == len(self.A) - 1:
                return self.cinv @ b
            A, m, gs = self.A[l], self.minv[l], self.ncol[l] > 0
            if gs:
                x = np.zeros_like(b)
                for _ in range(nu):
                    x = self.sweep(l, x, b, False)
            else:
                x = m * b
                for _ in range(nu - 1):
                    x = x + m * (b - A @ x)
            x = x + self.P[l] @ rec(l + 1, self.R[l] @ (b - A @ x))
            for _ in range(nu):
                x = self.sweep(l, x, b, True) if gs else x + m * (b - A @ x)
            assert x.dtype == self.dt
            return x
        return rec(0, b.astype(self.dt)).astype(np.float64)


def M32(H, cap=CAP):
    """the same cycle on a hierarchy cast to float32: r rounded once, every sum in fp32, z widened at the end"""
    return Mcgs(H, cap, F)


_CACHE = {}


def _op(name, matrix_path):
    if ("S", name) not in _CACHE:
        _CACHE[("S", name)] = operator(name, matrix_path)
    return _CACHE[("S", name)]


def _hier(name, matrix_path):
    if ("H", name) not in _CACHE:
        _CACHE[("H", name)] = Hier(_op(name, matrix_path))
    return _CACHE[("H", name)]


def _mcgs(name, matrix_path, cap=CAP, f32=False):
    key = ("M", name, cap, f32)
    if key not in _CACHE:
        _CACHE[key] = Mcgs(_hier(name, matrix_path), cap, F if f32 else np.float64)
    return _CACHE[key]


def _np_pcg(name, matrix_path, tol, nu, gs=True, maxit=20000):
    """(x, iterations, status) of numpy PCG on b_i = i around the mcgs cycle (or Hier's l1-Jacobi one), made once"""
    key = ("pcg", name, tol, nu, gs, maxit)
    if key not in _CACHE:
        S = _op(name, matrix_path)
        v = _mcgs(name, matrix_path).vcycle if gs else _hier(name, matrix_path).vcycle
        _CACHE[key] = pcg(S, O.rhs(S.shape[0]), lambda r: v(r, nu), tol, maxit)
    return _CACHE[key]


def _relerr(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _levels(S):
    """every level's matrix of the hierarchy of S, the coarsest included"""
    return Hier(S).A


# ------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("name", GRIDS + SPD)
def test_colouring_follows_the_rule_and_the_copy_is_the_matrix(name, matrix_path):
    for l, A in enumerate(_levels(operator(name, matrix_path))):
        M = as_matrix(A)
        col, nc = la.lsb_amg_colour(M)
        ref, nref = colour(A)
        assert nc == nref and np.array_equal(col, ref), (name, l)
        # valid: no stored off-diagonal pair shares a colour
        coo = A.tocoo()
        off = coo.row != coo.col
        assert not (col[coo.row[off]] == col[coo.col[off]]).any()
        assert set(np.unique(col)) == set(range(nc))
        # the copy: colour by colour, ascending rows inside a colour, the rows entry for entry
        cp = la.lsb_csr_mcgs(M, col, nc)
        order = np.argsort(col, kind="stable")
        assert np.array_equal(cp["rowid"], order)
        assert np.array_equal(cp["cbeg"], np.concatenate([[0], np.cumsum(np.bincount(col, minlength=nc))]))
        lens = np.diff(A.indptr)[order]
        assert np.array_equal(cp["offs"], np.concatenate([[0], np.cumsum(lens)]))
        B = A[order]
        assert np.array_equal(cp["cols"], B.indices) and cp["vals"].tobytes() == B.data.tobytes()
        assert la.lsb_mcgs_check(M, col, cp) == (0, "")
        print(name, "level", l, A.shape[0], "rows,", nc, "colours")


def test_the_check_refuses_what_would_race(matrix_path):
    A = _levels(operator("lap2d:nx=23,ny=17", None))[0]
    M = as_matrix(A)
    col, nc = la.lsb_amg_colour(M)
    cp = la.lsb_csr_mcgs(M, col, nc)
    assert la.lsb_mcgs_check(M, col, cp) == (0, "")
    # two neighbouring rows in one colour (the copy re-made for that colouring, so nothing else is wrong)
    bad = col.copy()
    bad[1] = bad[0]
    rc, why = la.lsb_mcgs_check(M, bad, la.lsb_csr_mcgs(M, bad, nc))
    assert rc != 0 and "different colours" in why, (rc, why)
    # rowid with a duplicate
    dup = dict(cp, rowid=cp["rowid"].copy())
    dup["rowid"][3] = dup["rowid"][2]
    rc, why = la.lsb_mcgs_check(M, col, dup)
    assert rc != 0 and "permutation" in why, (rc, why)
    # a row in the range of another colour; a changed value; a diagonal that is not positive
    sw = dict(cp, rowid=cp["rowid"].copy())
    a, b = int(cp["cbeg"][1]) - 1, int(cp["cbeg"][1])
    sw["rowid"][[a, b]] = sw["rowid"][[b, a]]
    rc, why = la.lsb_mcgs_check(M, col, sw)
    assert rc != 0 and "range of its colour" in why, (rc, why)
    ch = dict(cp, vals=cp["vals"].copy())
    ch["vals"][7] += 1e-9
    rc, why = la.lsb_mcgs_check(M, col, ch)
    assert rc != 0 and "entry for entry" in why, (rc, why)
    N = A.copy()
    N.data[N.indptr[5]:N.indptr[6]][N.indices[N.indptr[5]:N.indptr[6]] == 5] = 0.0
    MN = as_matrix(N)
    rc, why = la.lsb_mcgs_check(MN, col, la.lsb_csr_mcgs(MN, col, nc))
    assert rc != 0 and "diagonal" in why, (rc, why)
    # an unsymmetric pattern: a_ij stored in one row only is still looked at
    U = A.tolil()
    U[0, 2] = -0.5
    U = U.tocsr()
    U.sort_indices()
    MU = as_matrix(U)
    assert col[0] == col[2]
    rc, why = la.lsb_mcgs_check(MU, col, la.lsb_csr_mcgs(MU, col, nc))
    assert rc != 0 and "different colours" in why, (rc, why)
    assert la.lsb_csr_mcgs(M, np.full_like(col, nc), nc) is None  # a colour out of range


@pytest.mark.parametrize("coarse", [256, 40])
@pytest.mark.parametrize("cap", [CAP, 2])
@pytest.mark.parametrize("name", ["lap2d:nx=23,ny=17", "lap3d:nx=9,ny=8,nz=7"])
def test_the_numpy_cycle_is_an_spd_preconditioner(name, cap, coarse):
    """coarse = 256 is the default hierarchy, two levels on these operators; coarse = 40 coarsens once more, and the
    cap at 2 then leaves Gauss-Seidel on the fine level and l1-Jacobi below it: mixed levels"""
    S = _op(name, None)
    M = Mcgs(Hier(S, coarse=coarse), cap)
    assert len(M.A) >= (2 if coarse == 256 else 3) and M.ncol[0] == 2
    if cap == 2 and coarse == 40:
        assert 0 in M.ncol, M.found
    n = S.shape[0]
    for nu in (1, 2):
        B = np.stack([M.vcycle(e, nu) for e in np.eye(n)], axis=1)
        asym = np.linalg.norm(B - B.T) / np.linalg.norm(B)
        lam = np.linalg.eigvalsh(0.5 * (B + B.T))
        Lc = np.linalg.cholesky(S.toarray())
        lms = np.linalg.eigvalsh(Lc.T @ (0.5 * (B + B.T)) @ Lc)
        print(name, "coarse", coarse, "cap", cap, "colours", M.ncol, "nu", nu, "asymmetry", asym, "lambda_min(M^-1)",
              lam[0], "lambda(M^-1 S) in", (lms[0], lms[-1]))
        assert asym <= 1e-12
        assert lam[0] > 0.0
        assert lms[-1] <= 1.0 + 1e-10


@pytest.mark.parametrize("name,tol", sorted(TABLE))
def test_amg_pcg_takes_fewer_iterations_than_l1_jacobi(name, tol, matrix_path):
    l1_rec, gs_rec, colours = TABLE[(name, tol)]
    M = _mcgs(name, matrix_path)
    print(name, "colours per smoothed level", M.found, "recorded", colours)
    for k, nu in enumerate((1, 2)):
        _, it1, st1 = _np_pcg(name, matrix_path, tol, nu, gs=False)
        _, itg, stg = _np_pcg(name, matrix_path, tol, nu)
        print(name, "nu", nu, "iterations l1-Jacobi", it1, "mcgs", itg, "recorded", l1_rec[k], gs_rec[k])
        assert st1 == 1 and stg == 1
        assert itg < it1
        if nu == 1:
            assert itg <= 0.75 * it1, (itg, it1)


@pytest.mark.parametrize("name", SPD)
def test_amg_pcg_reaches_the_golden_solution(name, matrix_path, golden_x):
    x, it, st = _np_pcg(name, matrix_path, 1e-12, 1)
    assert st == 1 and _relerr(x, golden_x(name)) <= 1e-10


def test_surface():
    o = la.default_opts()
    assert o.amg_smoother == 0 and o.amg_sweeps == 1 and o.amg_tail_rows == 0  # the defaults do not change
    assert (la.AMG_SMOOTH_L1JACOBI, la.AMG_SMOOTH_CHEB, la.AMG_SMOOTH_MCGS) == (0, 1, 2) and _lib.AMG_SMOOTH_MCGS == 2
    assert _lib.Opts._fields_[-2][0] == "amg_smoother" and _lib.Opts._fields_[-1][0] == "amg_cheb_ratio"
    lib = _lib.load()
    got = _lib.Opts()
    try:
        assert lib.hip_cdna4_set_option(b"amg-smoother", b"mcgs") == 0
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.amg_smoother == 2
        assert lib.hip_cdna4_set_option(b"amg-smoother", b"gs") == 1
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.amg_smoother == 2
    finally:
        lib.lsb_hip_set_opts(C.byref(o))
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    r = subprocess.run([drv, "--help"], capture_output=True, text=True)
    assert "<l1|cheb|mcgs>" in r.stdout
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    assert "LSB_AMG_SMOOTH_MCGS = 2" in header and re.search(r"#define LSB_AMG_MCGS_COLOURS 16\b", header)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name), name
    assert callable(la.Solver.amg_colours)
    up = int(lib.hip.lsb_hip_is_initialized())
    assert lib.lsb_hip_solver_amg_colours(None, 0, None) == (2 if up else 1)
    assert lib.lsb_hip_solver_amg_cheb_interval(None, 0, None, None) == (2 if up else 1)


# ------------------------------------------------------------------------------------ on the GPU
_BAD_SMOOTHER = r"""
import sys
sys.path.insert(0, sys.argv[1])
import lsbench_amd as la
assert la.hip_cdna4_init() == 0
la.Solver(la.lsbench_matrix_synth("lap2d:nx=20,ny=20"), la.default_opts(precond=la.PRECOND_AMG, amg_smoother=3))
"""


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _solver(hip, name, matrix_path, **kw):
    """a mcgs solver on the operator the numpy side uses, as read"""
    kw.setdefault("op_mode", hip.OP_RAW)
    kw.setdefault("amg_smoother", MCGS)
    return hip.Solver(as_matrix(_op(name, matrix_path)), hip.default_opts(precond=hip.PRECOND_AMG, **kw))


def _apply(s, r):
    """z of two precond_dev calls on a z pre-filled with NaN, which must agree byte for byte"""
    import torch
    d_r = _dev(r)
    zs = []
    for _ in range(2):
        d_z = torch.full((len(r),), float("nan"), dtype=torch.float64, device="cuda:0")
        s.precond_dev(d_r, d_z)
        zs.append(d_z.cpu().numpy())
    assert zs[0].tobytes() == zs[1].tobytes() and np.isfinite(zs[0]).all()
    return zs[0]


def _r(n):
    return np.sin(np.arange(n, dtype=np.float64)) + 0.5


def _check_colours(s, M):
    nlev = len(M.A)
    assert s.amg_info == (nlev, 0)  # no one-launch tail under mcgs
    for l in range(nlev - 1):
        assert s.amg_colours(l) == M.ncol[l], (l, s.amg_colours(l), M.ncol, M.found)
    assert s.amg_colours(nlev - 1) is None and s.amg_colours(nlev + 3) is None
    assert s.amg_cheb_interval(0) is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", CYCLES)
def test_one_application_against_numpy(hip, name, matrix_path):
    S = _op(name, matrix_path)
    M = _mcgs(name, matrix_path)
    r = _r(S.shape[0])
    if name == "xn3b_A_18":
        assert M.found[:2] == [16, 39] and M.ncol[:2] == [16, 0]  # exactly at the cap; beyond it
    if name == "lap2d:nx=300,ny=300":
        assert M.ncol == [2, 5, 10]
    for nu in (1, 2):
        s = _solver(hip, name, matrix_path, amg_sweeps=nu, amg_tail_rows=1 << 30)
        _check_colours(s, M)
        z = _apply(s, r)
        s.destroy()
        zr = M.vcycle(r, nu)
        print(name, "nu", nu, "colours", M.ncol, "device against numpy", _relerr(z, zr))
        assert np.linalg.norm(z - zr) <= 1e-12 * np.linalg.norm(zr)
        if len(M.A) == 1:  # nothing to smooth: the l1 solver's bytes
            s = _solver(hip, name, matrix_path, amg_sweeps=nu, amg_smoother=hip.AMG_SMOOTH_L1JACOBI)
            assert s.amg_colours(0) is None
            z1 = _apply(s, r)
            s.destroy()
            assert z.tobytes() == z1.tobytes()


@pytest.mark.gpu
def test_the_cap_from_the_environment(hip, monkeypatch):
    name = "lap2d:nx=300,ny=300"
    S = _op(name, None)
    M = _mcgs(name, None, cap=2)
    assert M.ncol == [2, 0, 0]
    r = _r(S.shape[0])
    monkeypatch.setenv("LSBENCH_HIP_AMG_MCGS_COLOURS", "2")
    s = _solver(hip, name, None)
    monkeypatch.delenv("LSBENCH_HIP_AMG_MCGS_COLOURS")
    _check_colours(s, M)
    z = _apply(s, r)
    s.destroy()
    zr = M.vcycle(r, 1)
    assert np.linalg.norm(z - zr) <= 1e-12 * np.linalg.norm(zr)
    assert _relerr(z, _mcgs(name, None).vcycle(r, 1)) > 1e-6  # (another cycle than the default cap's)


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("name", CYCLES)
def test_one_application_in_fp32(hip, name, nu, matrix_path):
    S = _op(name, matrix_path)
    M, M_32 = _mcgs(name, matrix_path), _mcgs(name, matrix_path, f32=True)
    r = _r(S.shape[0])
    s = _solver(hip, name, matrix_path, amg_sweeps=nu, amg_precision=hip.AMG_PREC_FP32)
    assert s.amg_precision == 1
    _check_colours(s, M)
    z = _apply(s, r)
    s.destroy()
    s = _solver(hip, name, matrix_path, amg_sweeps=nu)
    zd = _apply(s, r)
    s.destroy()
    z64 = M.vcycle(r, nu)
    e_gpu, e_np = _relerr(z, z64), _relerr(M_32.vcycle(r, nu), z64)
    print(name, "nu", nu, "device fp32 against numpy fp64", e_gpu, "numpy fp32 against numpy fp64", e_np)
    assert z.tobytes() != zd.tobytes()
    assert e_gpu <= 4.0 * max(e_np, 2.0 ** -24)


_L1_ITERS = {}


def _l1_iters(hip, name, matrix_path, tol):
    if name not in _L1_ITERS:
        s = _solver(hip, name, matrix_path, tol=tol, amg_smoother=hip.AMG_SMOOTH_L1JACOBI)
        _, r = s.solve(O.rhs(_op(name, matrix_path).shape[0]))
        s.destroy()
        assert r.status == hip.STATUS_CONVERGED
        _L1_ITERS[name] = int(r.iters)
    return _L1_ITERS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("name,tol", [(n, 1e-12) for n in SPD] + [(LAP3D, 1e-10)])
def test_solves(hip, name, tol, f32, matrix_path, golden_x):
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    xr, itr, stat = _np_pcg(name, matrix_path, tol, 1)
    assert stat == 1
    kw = dict(tol=tol, amg_precision=hip.AMG_PREC_FP32 if f32 else hip.AMG_PREC_FP64)
    xs = []
    for graph in (0, 1):
        s = _solver(hip, name, matrix_path, use_graph=graph, **kw)
        x, r = s.solve(b)
        x2, r2 = s.solve(b)
        s.destroy()
        print(name, "fp32" if f32 else "fp64", "graph", graph, "iterations", r.iters, "numpy", itr, "relres", r.relres)
        assert r.status == hip.STATUS_CONVERGED
        assert x.tobytes() == x2.tobytes() and r.iters == r2.iters
        assert abs(int(r.iters) - itr) <= max(2, 0.04 * itr), (r.iters, itr)
        if name in SPD:
            assert _relerr(x, golden_x(name)) <= 1e-10
        else:
            assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
        xs.append((x, int(r.iters)))
    assert xs[0][0].tobytes() == xs[1][0].tobytes() and xs[0][1] == xs[1][1]
    s = _solver(hip, name, matrix_path, maxit=5, **kw)
    x, r = s.solve(b)
    s.destroy()
    assert r.status == hip.STATUS_MAXIT and r.iters == 5
    it1 = _l1_iters(hip, name, matrix_path, tol)
    print(name, "l1-Jacobi solver", it1, "iterations")
    assert xs[0][1] < it1


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
def test_richardson_and_a_warm_start(hip, f32, matrix_path):
    import torch
    name = "xn3b_A_18"
    n = _op(name, matrix_path).shape[0]
    b = O.rhs(n)
    prec = hip.AMG_PREC_FP32 if f32 else hip.AMG_PREC_FP64
    s = _solver(hip, name, matrix_path, krylov=hip.KRYLOV_RICHARDSON, maxit=2, tol=0.0, amg_precision=prec)
    d_b = _dev(b)
    d_x = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    res = s.solve_dev(d_b, d_x)
    assert (res.status, res.iters) == (hip.STATUS_MAXIT, 2)
    x, r = torch.zeros_like(d_b), d_b.clone()  # the replay of test_richardson.py
    for _ in range(2):
        z = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        q = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        s.precond_dev(r, z)
        s.spmv_dev(z, q)
        x = x + z
        r = r - q
    s.destroy()
    assert np.isfinite(d_x.cpu().numpy()).all() and d_x.cpu().numpy().tobytes() == x.cpu().numpy().tobytes()
    # a good x0 costs nothing and stays where it is
    name = "lap2d:nx=130,ny=70"
    b = O.rhs(_op(name, None).shape[0])
    for krylov in (hip.KRYLOV_AUTO, hip.KRYLOV_RICHARDSON):
        s = _solver(hip, name, None, tol=1e-12, krylov=krylov, amg_precision=prec, maxit=400)
        x_cold, rc = s.solve(b)
        s.destroy()
        assert rc.status == hip.STATUS_CONVERGED and rc.iters > 0
        s = _solver(hip, name, None, tol=1e-8, krylov=krylov, amg_precision=prec)
        xw, rw = s.solve(b, x0=x_cold)
        s.destroy()
        assert rw.status == hip.STATUS_CONVERGED and rw.iters == 0 and xw.tobytes() == x_cold.tobytes()


@pytest.mark.gpu
def test_verify_and_renumbered_solvers(hip, monkeypatch, matrix_path):
    name = "xn3b_A_18"
    b = O.rhs(_op(name, matrix_path).shape[0])
    s = _solver(hip, name, matrix_path, tol=1e-12, verify=1)
    x, r = s.solve(b)
    s.destroy()
    assert r.status == hip.STATUS_CONVERGED and 0.0 <= r.true_relres <= 1e-12 and r.corrections <= 6
    opts = dict(op_mode=hip.OP_RAW, precond=hip.PRECOND_AMG, amg_smoother=MCGS)
    A = hip.lsbench_matrix_synth("lap2d:nx=60,ny=50")
    b = O.rhs(A.nrows)
    xs = {}
    for ro in (0, 1):
        s = hip.Solver(A, hip.default_opts(reorder=ro, **opts))
        assert s.amg_colours(0) == 2
        x, r = s.solve(b)
        s.destroy()
        assert r.status == 1
        xs[ro] = x
    assert np.linalg.norm(xs[1] - xs[0]) <= 1e-10 * np.linalg.norm(xs[0])
    # lines of 2050 rows padded to whole slices against the unpadded solve
    A = hip.lsbench_matrix_synth("lap2d:nx=2050,ny=12")
    b = O.rhs(A.nrows)
    out = {}
    for pad in ("0", "1"):
        monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", pad)
        s = hip.Solver(A, hip.default_opts(tol=1e-12, **opts))
        assert bool(s.padded) == (pad == "1") and s.n_local == A.nrows
        x, r = s.solve(b)
        s.destroy()
        assert r.status == 1
        out[pad] = x
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    assert np.linalg.norm(out["1"] - out["0"]) <= 1e-10 * np.linalg.norm(out["0"])


@pytest.mark.gpu
def test_refusals_and_the_driver(hip, matrix_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    name = "xn3b_A_18"
    S = _op(name, matrix_path)
    n = S.shape[0]
    s = _solver(hip, name, matrix_path)
    B = np.stack([O.rhs(n), _r(n)])
    d_B = _dev(B)
    d_X = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_solve_multi_x0_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    X = np.full((2, n), 7.0)
    assert lib.lsb_hip_solver_solve_multi(s._h, 2, B.ctypes.data, n, X.ctypes.data, n, res) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (X == 7.0).all()
    assert lib.lsb_hip_solver_spmm_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 0  # the SpMM keeps working
    Y = d_X.cpu().numpy()
    for c in range(2):
        assert np.linalg.norm(Y[c] - S @ B[c]) <= 1e-13 * np.linalg.norm(S @ B[c])
    s.destroy()
    rc = subprocess.run([sys.executable, "-c", _BAD_SMOOTHER, ROOT], capture_output=True, text=True)
    assert rc.returncode != 0 and "no AMG smoother 3" in rc.stderr, rc.stderr
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    base = [drv, "--solver", "hip", "--precond", "amg", "--amg-smoother", "mcgs", "--trials=1"]
    r = subprocess.run(base + ["--matrix", "synth:lap2d:nx=40,ny=30", "--operator", "raw", "--nvirt", "2"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "one shard" in r.stderr
    for k in ("gmres", "cg1"):
        r = subprocess.run(base + ["--matrix", matrix_path(name), "--krylov", k], capture_output=True, text=True)
        assert r.returncode != 0 and "classic PCG" in r.stderr, r.stderr
    r = subprocess.run([drv, "--solver", "hip", "--matrix", matrix_path(name), "--precond", "amg", "--amg-smoother",
                        "mcgs", "--trials=3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rec = r.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[2]) == 1 and 0 < int(f[0]) < 128
