"""Several right-hand sides under AMG: lsb_hip_solver_precond_multi_dev and solve_multi[_dev] on an AMG solver
(hip_mrhs_amg.hip, amg_cycle in hip_amg_drv.c, hip_mrhs_drv.c).

The yardsticks: the single-column V-cycle of the same solver, byte for byte (a column of the block cycle does the
single cycle's arithmetic); test_amg.py's numpy V-cycle and AMG-PCG with the bounds test_amg.py holds the single
solve to; a sparse direct solve; and, for opts.verify, `pcg_restart_amg` below, test_mrhs.py's restatement of the
in-place restart with the V-cycle in the place of the diagonal."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from oracle import oracle as O
from test_amg import Hier, as_matrix, operator, pcg
from test_mrhs import _block, _host, _solve, columns, eleven, relerr, relres_exact

CONVERGED, MAXIT = 1, 3
NAME = "lsb_hip_solver_precond_multi_dev"


# ------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def _op(name, matrix_path):
    return operator(name, matrix_path)


@functools.lru_cache(maxsize=None)
def _hier(name, matrix_path):
    return Hier(_op(name, matrix_path))


@functools.lru_cache(maxsize=None)
def _rhs(name, matrix_path, key):
    S = _op(name, matrix_path)
    B = {"five": columns(S), "eleven": eleven(S),
         "two": np.stack([O.rhs(S.shape[0]), np.random.default_rng(7).standard_normal(S.shape[0])], axis=1)}[key]
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def _numpy_pcg(name, matrix_path, key, tol, maxit=20000):
    """[(x, iters, status)] of the numpy AMG-PCG per column; a zero column is (0, 0, CONVERGED)"""
    S, H, B = _op(name, matrix_path), _hier(name, matrix_path), _rhs(name, matrix_path, key)
    out = []
    for c in range(B.shape[1]):
        b = B[:, c].copy()
        out.append(pcg(S, b, H.vcycle, tol, maxit) if b.any() else (np.zeros_like(b), 0, CONVERGED))
    return out


@functools.lru_cache(maxsize=None)
def _direct(name, matrix_path, key):
    return spla.splu(_op(name, matrix_path).tocsc()).solve(np.array(_rhs(name, matrix_path, key)))


@functools.lru_cache(maxsize=None)
def _numpy_vcycles(name, matrix_path, nu):
    H, R = _hier(name, matrix_path), _rhs(name, matrix_path, "eleven")
    return np.stack([H.vcycle(R[:, c].copy(), nu) for c in range(R.shape[1])], axis=1)


def pcg_restart_amg(S, b, M, tol, maxit=20000):
    """AMG-PCG from x0 = 0 with the check on the RECOMPUTED residual and the in-place restart (r = b - S x,
    z = M r, p = z, x kept, bb and the threshold unchanged, iterations counted on; 6 at the most).
    -> dict(x, iters, status, corrections, true_relres, first_stop=(iters, recomputed relres))."""
    x = np.zeros(len(b))
    bb = b @ b
    r = b.copy()
    p = M(r)
    rz = r @ p
    it, corr, first, true = 0, 0, None, -1.0
    status = CONVERGED
    while True:
        while True:
            q = S @ p
            alpha = rz / (p @ q)
            x += alpha * p
            r -= alpha * q
            it += 1
            if r @ r <= tol * tol * bb:
                status = CONVERGED
                break
            if it >= maxit:
                status = MAXIT
                break
            z = M(r)
            rz_new = r @ z
            p = z + (rz_new / rz) * p
            rz = rz_new
        if status != CONVERGED:
            break
        r = b - S @ x
        true = math.sqrt((r @ r) / bb)
        if first is None:
            first = (it, true)
        if true <= tol:
            break
        if corr >= 6 or it >= maxit:
            status = MAXIT
            break
        corr += 1
        p = M(r)
        rz = r @ p
    return dict(x=x, iters=it, status=status, corrections=corr, true_relres=true, first_stop=first)


# ------------------------------------------------------------------------------------ without a GPU
def test_the_function_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert NAME in _lib.SIGNATURES and hasattr(lib.hip, NAME)
    assert callable(la.Solver.precond_multi_dev)
    up = int(lib.hip.lsb_hip_is_initialized())
    assert lib.lsb_hip_solver_precond_multi_dev(None, 1, None, 0, None, 0) == (2 if up else 1)


def test_cpu_precondition_amg_pcg_converges_on_every_column(matrix_path):
    """What the GPU tests lean on: the numpy AMG-PCG at tol = 1e-12 converges on every non-zero column of
    eleven(S) of xn3b_A_18 and agrees with a sparse direct solve to 1e-10 (seen: 83-128 iterations, worst error
    1.03e-11 on column 7, 3.3e-12 on the five of columns(S))."""
    B = _rhs("xn3b_A_18", matrix_path, "eleven")
    ref, X = _numpy_pcg("xn3b_A_18", matrix_path, "eleven", 1e-12), _direct("xn3b_A_18", matrix_path, "eleven")
    for c in range(B.shape[1]):
        x, it, st = ref[c]
        if not B[:, c].any():
            assert it == 0
            continue
        print("column", c, "iterations", it, "error against the direct solve", relerr(x, X[:, c]))
        assert st == CONVERGED and it > 5 and relerr(x, X[:, c]) <= 1e-10


def test_cpu_precondition_column_i_of_tj7a_needs_a_restart(matrix_path):
    """The verify test's input: on tj7a_A_12, b_i = i, tol = 1e-12, the recurrence's first stop has a recomputed
    residual ABOVE the tolerance (seen: stop at iteration 120 with 2.83e-12, 2 in-place restarts, 122 iterations,
    8.2e-13; tj7a_A_18: 1 restart, 1.37e-12 at iteration 116) -- well inside the cap of 6 rounds."""
    for name in ("tj7a_A_12", "tj7a_A_18"):
        S, H = _op(name, matrix_path), _hier(name, matrix_path)
        b = O.rhs(S.shape[0])
        y = pcg_restart_amg(S, b, H.vcycle, 1e-12)
        print(name, y["first_stop"], y["iters"], y["corrections"], y["true_relres"])
        assert y["status"] == CONVERGED and 1 <= y["corrections"] <= 6
        assert y["first_stop"][1] > 1e-12 and y["true_relres"] <= 1e-12


# ------------------------------------------------------------------------------------ on the GPU
def _amg_solver(hip, name, matrix_path, **kw):
    """(solver, S): the reference matrices as read from their files, the synthetic ones with the CSR as handed in"""
    S = _op(name, matrix_path)
    if ":" in name:
        M = hip.lsbench_matrix_synth(name) if not name.startswith("powerlaw") else as_matrix(S)
        kw.setdefault("op_mode", hip.OP_RAW)
    else:
        M = hip.lsbench_matrix_read(matrix_path(name))
    return hip.Solver(M, hip.default_opts(precond=hip.PRECOND_AMG, **kw)), S


def _cycle_multi(s, R, gap=3):
    """Z of precond_multi_dev with ldz = n + gap; the gap rows hold a NaN sentinel that must survive"""
    import torch
    n, k = R.shape
    d_Z = torch.full((k, n + gap), float("nan"), dtype=torch.float64, device="cuda:0")
    s.precond_multi_dev(_block(R, n + 5), d_Z)
    assert bool(torch.isnan(d_Z[:, n:]).all())
    Z = _host(d_Z, n)
    assert not np.isnan(Z).any()
    return Z


def _cycle_single(s, R):
    import torch
    n, k = R.shape
    out = np.empty_like(R)
    d_z = torch.empty(n, dtype=torch.float64, device="cuda:0")
    for c in range(k):
        d_z.fill_(float("nan"))
        s.precond_dev(torch.from_numpy(np.ascontiguousarray(R[:, c])).to("cuda:0"), d_z)
        out[:, c] = d_z.cpu().numpy()
    return out


def _check_cycle_bytes(s, R):
    Z1 = _cycle_single(s, R)
    Z = _cycle_multi(s, R)
    for c in range(R.shape[1]):
        assert Z[:, c].tobytes() == Z1[:, c].tobytes(), c
    assert not Z[:, 1].any()  # the zero column
    for k in (2, 3, 5):  # widths 2, 4, 8 (11: 8 + 4), padded
        Zk = _cycle_multi(s, R[:, :k])
        assert Zk.tobytes() == Z[:, :k].tobytes(), k
    assert _cycle_multi(s, R).tobytes() == Z.tobytes()  # a second call
    return Z


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("name", ["xn3b_A_18", "lap2d:nx=130,ny=70", "powerlaw:n=900,avg=9,max=300,seed=3,spd=1",
                                  "lap2d:nx=12,ny=9"])
def test_vcycle_bit_for_bit(hip, name, nu, matrix_path):
    """Lane counts from 2 (P, R) to 64 (coarse Galerkin operators, the dense solve); lap2d 12 x 9 is one level."""
    R = np.array(_rhs(name, matrix_path, "eleven"))
    s, S = _amg_solver(hip, name, matrix_path, amg_sweeps=nu)
    lev, _ = s.amg_info
    assert lev == len(_hier(name, matrix_path).A) and (lev == 1) == (name == "lap2d:nx=12,ny=9")
    Z = _check_cycle_bytes(s, R)
    s.destroy()
    Zr = _numpy_vcycles(name, matrix_path, nu)
    for c in range(R.shape[1]):
        if R[:, c].any():
            assert np.linalg.norm(Z[:, c] - Zr[:, c]) <= 1e-12 * np.linalg.norm(Zr[:, c]), c
    s, _ = _amg_solver(hip, name, matrix_path, amg_sweeps=nu, amg_tail_rows=4096)  # the tail is ignored for blocks
    assert _cycle_multi(s, R).tobytes() == Z.tobytes()
    s.destroy()


@pytest.mark.gpu
def test_vcycle_bit_for_bit_reordered_and_padded(hip, matrix_path, monkeypatch):
    name = "lap2d:nx=60,ny=50"
    s, _ = _amg_solver(hip, name, matrix_path, reorder=1)
    _check_cycle_bytes(s, np.array(_rhs(name, matrix_path, "eleven")))
    s.destroy()
    name = "lap2d:nx=2050,ny=12"
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1")
    s, _ = _amg_solver(hip, name, matrix_path)
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    assert s.padded > 0
    _check_cycle_bytes(s, np.array(_rhs(name, matrix_path, "eleven")))
    s.destroy()


def _check_against_numpy(res, X, B, ref, Xd=None, cols=None, tol_x=1e-10):
    for c in (range(B.shape[1]) if cols is None else cols):
        xr, itr, st = ref[c]
        print("column", c, "iters", res[c].iters, "numpy", itr, "status", res[c].status)
        assert res[c].status == CONVERGED and st == CONVERGED
        if not B[:, c].any():
            assert res[c].iters == 0 and not X[:, c].any()
            continue
        assert abs(int(res[c].iters) - itr) <= max(2, 0.04 * itr), (c, res[c].iters, itr)
        err = relerr(X[:, c], xr if Xd is None else Xd[:, c])
        print("   error", err)
        assert err <= tol_x


@pytest.mark.gpu
def test_solves_match_numpy_per_column(hip, matrix_path, golden_x):
    name, tol = "xn3b_A_18", 1e-12
    B = np.array(_rhs(name, matrix_path, "five"))
    ref, Xd = _numpy_pcg(name, matrix_path, "five", tol), _direct(name, matrix_path, "five")
    xs = {}
    for graph in (0, 1):
        s, _ = _amg_solver(hip, name, matrix_path, tol=tol, use_graph=graph)
        X, res = _solve(s, B)
        _check_against_numpy(res, X, B, ref, Xd)
        assert all(r.true_relres < 0.0 for r in res)
        assert len({r.seconds for r in res}) == 1 and len({r.spmvs for r in res}) == 1
        assert res[0].spmvs == max(r.iters for r in res)
        X2, res2 = _solve(s, B)  # a second call repeats the first
        assert X2.tobytes() == X.tobytes() and [r.iters for r in res2] == [r.iters for r in res]
        Xh, resh = s.solve_multi(B)  # host buffers
        assert Xh.tobytes() == X.tobytes() and [r.iters for r in resh] == [r.iters for r in res]
        s.destroy()
        xs[graph] = X
    assert xs[0].tobytes() == xs[1].tobytes()
    assert relerr(xs[0][:, 0], golden_x(name)) <= 1e-10


@pytest.mark.gpu
def test_solves_match_numpy_on_tj7a(hip, matrix_path):
    name, tol = "tj7a_A_18", 1e-12
    B = np.array(_rhs(name, matrix_path, "five"))
    s, _ = _amg_solver(hip, name, matrix_path, tol=tol)
    X, res = _solve(s, B)
    s.destroy()
    _check_against_numpy(res, X, B, _numpy_pcg(name, matrix_path, "five", tol), _direct(name, matrix_path, "five"))


@pytest.mark.gpu
def test_against_single_solves_of_the_same_solver(hip, matrix_path):
    import torch
    name, tol = "xn3b_A_18", 1e-12
    B = np.array(_rhs(name, matrix_path, "five"))
    n = B.shape[0]
    s, _ = _amg_solver(hip, name, matrix_path, tol=tol)
    d_x = torch.empty(n, dtype=torch.float64, device="cuda:0")
    single = []
    for c in range(5):
        r1 = s.solve_dev(torch.from_numpy(np.ascontiguousarray(B[:, c])).to("cuda:0"), d_x)
        single.append((d_x.cpu().numpy(), r1))
    X1, res1 = _solve(s, B[:, :1])  # one column IS solve_dev
    assert X1[:, 0].tobytes() == single[0][0].tobytes()
    assert res1[0].iters == single[0][1].iters and res1[0].status == single[0][1].status
    X, res = _solve(s, B)
    s.destroy()
    for c in (0, 2, 3, 4):
        x1, r1 = single[c]
        print("column", c, "batch", res[c].iters, "single", r1.iters, "difference", relerr(X[:, c], x1))
        assert res[c].status == CONVERGED and r1.status == CONVERGED
        assert abs(int(res[c].iters) - int(r1.iters)) <= max(2, 0.04 * r1.iters)
        assert relerr(X[:, c], x1) <= 50 * tol


@pytest.mark.gpu
def test_columns_do_not_see_each_other(hip, matrix_path):
    name = "xn3b_A_18"
    B = np.array(_rhs(name, matrix_path, "five"))[:, [0, 3, 2, 4]]  # i, e0, S.1, randn
    s, _ = _amg_solver(hip, name, matrix_path, tol=1e-12)
    X, res = _solve(s, B)
    for c in (0, 1):
        Bc = np.zeros_like(B)
        Bc[:, c] = B[:, c]
        Xc, resc = _solve(s, Bc)
        assert Xc[:, c].tobytes() == X[:, c].tobytes() and resc[c].iters == res[c].iters
        assert not Xc[:, [k for k in range(4) if k != c]].any()
    s.destroy()


@pytest.mark.gpu
def test_eleven_columns_run_as_two_batches(hip, matrix_path):
    name, tol = "xn3b_A_18", 1e-12
    B = np.array(_rhs(name, matrix_path, "eleven"))
    assert B.shape[1] == 11 and np.array_equal(B[:, 0], B[:, 8])
    s, _ = _amg_solver(hip, name, matrix_path, tol=tol)
    X, res = _solve(s, B)
    s.destroy()
    _check_against_numpy(res, X, B, _numpy_pcg(name, matrix_path, "eleven", tol), _direct(name, matrix_path, "eleven"))
    assert len({r.seconds for r in res[:8]}) == 1 and len({r.seconds for r in res[8:]}) == 1
    assert len({r.spmvs for r in res[:8]}) == 1 and res[0].spmvs == max(r.iters for r in res[:8])
    assert len({r.spmvs for r in res[8:]}) == 1 and res[8].spmvs == max(r.iters for r in res[8:])


@pytest.mark.gpu
def test_stop_rules_maxit(hip, matrix_path):
    name = "xn3b_A_18"
    B = np.array(_rhs(name, matrix_path, "five"))
    ref5 = _numpy_pcg(name, matrix_path, "five", 1e-12, 5)
    s, _ = _amg_solver(hip, name, matrix_path, tol=1e-12, maxit=5)
    X, res = _solve(s, B)
    s.destroy()
    for c in range(5):
        if B[:, c].any():
            assert ref5[c][1] == 5 and ref5[c][2] == MAXIT
            assert res[c].status == MAXIT and res[c].iters == 5
            assert np.linalg.norm(X[:, c] - ref5[c][0]) <= 1e-9 * np.linalg.norm(ref5[c][0])
        else:
            assert res[c].status == CONVERGED and res[c].iters == 0 and not X[:, c].any()
    assert res[0].spmvs == 5


@pytest.mark.gpu
def test_verify_restarts_in_place(hip, matrix_path):
    """Figures of the reference run: column 0 stops first at iteration 120 with a recomputed 2.83e-12, 2 restarts."""
    name, tol = "tj7a_A_12", 1e-12
    S = _op(name, matrix_path)
    B = np.array(_rhs(name, matrix_path, "five"))
    s, _ = _amg_solver(hip, name, matrix_path, tol=tol, verify=1)
    X, res = _solve(s, B)
    X2, res2 = _solve(s, B)
    s.destroy()
    print([(r.iters, r.status, r.corrections, r.true_relres) for r in res])
    assert 1 <= res[0].corrections <= 6
    for c in (0, 2, 3, 4):
        cpu = relres_exact(S, X[:, c], B[:, c])
        print("column", c, "true_relres", res[c].true_relres, "cpu, exact", cpu)
        assert res[c].status == CONVERGED and 0.0 <= res[c].true_relres <= tol
        assert abs(res[c].true_relres - cpu) <= 1e-3 * cpu
    assert res[1].status == CONVERGED and res[1].iters == 0 and not X[:, 1].any()
    assert X2.tobytes() == X.tobytes()
    assert [(r.iters, r.corrections, r.true_relres) for r in res2] == [(r.iters, r.corrections, r.true_relres) for r in res]
    s, _ = _amg_solver(hip, name, matrix_path, tol=tol, verify=0)
    _, res0 = _solve(s, B)
    s.destroy()
    assert all(r.true_relres < 0.0 and r.corrections == 0 for r in res0)


@pytest.mark.gpu
def test_grids(hip, matrix_path, monkeypatch):
    # a 3-D stencil, the CSR as handed in, against numpy
    name, tol = "lap3d:nx=24,ny=20,nz=18", 1e-10
    B = np.array(_rhs(name, matrix_path, "five"))
    s, _ = _amg_solver(hip, name, matrix_path, tol=tol)
    X, res = _solve(s, B)
    s.destroy()
    _check_against_numpy(res, X, B, _numpy_pcg(name, matrix_path, "five", tol), tol_x=1e-8)
    # a line-padded 2-D grid against the unpadded solve
    name = "lap2d:nx=2050,ny=12"
    B = np.array(_rhs(name, matrix_path, "two"))
    out = {}
    for pad in ("0", "1"):
        monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", pad)
        s, _ = _amg_solver(hip, name, matrix_path, tol=1e-12)
        assert bool(s.padded) == (pad == "1") and s.n_local == B.shape[0]
        out[pad], res = _solve(s, B)
        s.destroy()
        assert all(r.status == CONVERGED for r in res)
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    for c in range(2):
        assert relerr(out["1"][:, c], out["0"][:, c]) <= 1e-10
    # reverse Cuthill-McKee: the same solutions
    name = "lap2d:nx=60,ny=50"
    B = np.array(_rhs(name, matrix_path, "five"))
    xs = {}
    for ro in (0, 1):
        s, _ = _amg_solver(hip, name, matrix_path, reorder=ro)
        xs[ro], res = _solve(s, B)
        s.destroy()
        assert all(r.status == CONVERGED for r in res)
    for c in (0, 2, 3, 4):
        assert relerr(xs[1][:, c], xs[0][:, c]) <= 1e-10
    assert not xs[1][:, 1].any()


@pytest.mark.gpu
def test_refusals(hip, matrix_path):
    import torch
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    lib = _lib.load()
    d_R = torch.ones(2, n, dtype=torch.float64, device="cuda:0")
    d_Z = torch.zeros(2, n, dtype=torch.float64, device="cuda:0")
    for kw in (dict(), dict(precond=hip.PRECOND_FSAI)):  # Jacobi, FSAI
        s = hip.Solver(A, hip.default_opts(**kw))
        assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, d_R.data_ptr(), n, d_Z.data_ptr(), n) == 2
        s.destroy()
    s = hip.Solver(A, hip.default_opts(precond=hip.PRECOND_AMG))
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 0, d_R.data_ptr(), n, d_Z.data_ptr(), n) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, d_R.data_ptr(), n - 1, d_Z.data_ptr(), n) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, d_R.data_ptr(), n, d_Z.data_ptr(), n - 1) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, None, n, d_Z.data_ptr(), n) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, d_R.data_ptr(), n, None, n) == 2
    assert not bool(d_Z.any())
    for k in (1, 2, 8):
        assert s.multi_iteration_bytes(k) == 0
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, d_R.data_ptr(), n, d_Z.data_ptr(), n) == 0
    assert bool(d_Z.any())
    s.destroy()
