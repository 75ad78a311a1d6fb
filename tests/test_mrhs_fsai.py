"""FSAI-preconditioned PCG on blocks of right-hand sides (opts.fsai_blocks = 1; hip_mrhs_fsai.hip, hip_mrhs_drv.c):
lsb_hip_solver_precond_multi_dev, solve_multi[_dev] and solve_multi_x0_dev on an FSAI solver.

The yardsticks: test_precond_apply.py's exact G*^T G* r with its componentwise bound for the block apply; the oracle's
FSAI-PCG (O.pcg_prec, kind "fsai") per column for the solves, with the iteration margin of
test_hip_fsai_follows_the_oracle; the golden x; the extended-precision residual of test_mrhs.py.  Every GPU test
builds its solver with fsai_blocks = 1: without the feature each of them meets the answer 2.

lsb_hip_solver_multi_iteration_bytes of such a solver is
    12 (nnz_S + nnz_G + nnz_G^T) + 12 (n + 1) + 8 n 16 Kp:
S, G and G^T streamed once each whatever the width (12 B per entry, n + 1 row offsets each), and 16 vector passes per
column -- the SpMM 2 (p in, q out); k_mrhs_fsai_xr_gr 6 (q and r gathered, p and x of the own rows in, x and t out);
k_mrhs_fsai_gt_dots 5 (t gathered, q and r of the own rows in, r and z out); k_amg_mrhs_update_p 3 (z and p in, p out).
No pass is shared between two launches."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from oracle import oracle as O
from test_mrhs import _block, _host, _scipy_matrix, _solve, oracle_operator, relerr, relres, relres_exact
from test_precond_apply import C_FSAI, fsai_exact, fsai_ratio, fsai_reference, fsai_setup
from test_warm_start import _solve_block

CONVERGED, MAXIT = 1, 3
NAME = "lsb_hip_solver_fsai_nnz"
NAMES5 = ("i", "e0", "sin i", "ones", "normal")
APPLY_CASES = (("xn3b_A_18", 1), ("xn3b_A_18", 3), ("tj7a_A_12", 2))
assert C_FSAI == 0.5  # the constant the block apply is held to: the single-column apply's, same two products


# ------------------------------------------------------------------------------------ inputs and references, once
def five(n):
    """(i, e0, sin i, ones, randn(seed 7)) as an (n, 5) array: Kp = 8 with three padding columns"""
    e0 = np.zeros(n)
    e0[0] = 1.0
    return np.stack([O.rhs(n), e0, np.sin(np.arange(n, dtype=np.float64)), np.ones(n),
                     np.random.default_rng(7).standard_normal(n)], axis=1)


@functools.lru_cache(maxsize=None)
def _oracle(path, power, tol, maxit=20000):
    """[(x, iters, status)] of the oracle's FSAI-PCG for the five columns"""
    So, _ = oracle_operator(path)
    B = five(So.nrows)
    out = []
    for c in range(5):
        x, it, _, st, _, _ = O.pcg_prec(So.offs, So.cols, So.vals, np.ascontiguousarray(B[:, c]), tol, maxit=maxit,
                                        kind="fsai", param=power)
        x.setflags(write=False)
        out.append((x, int(it), int(st)))
    return out


def _margin(ito):
    return max(2, ito // 25)  # test_hip_fsai_follows_the_oracle's


# ------------------------------------------------------------------------------------ without a GPU
def test_the_switch_is_off_by_default_and_the_last_field():
    o = la.default_opts()
    assert o.fsai_blocks == 0
    assert la.default_opts(fsai_blocks=1).fsai_blocks == 1
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    body = re.search(r"struct lsb_hip_opts \{(.*?)\n\};", header, re.S).group(1)
    members = re.findall(r"^\s*(?:unsigned|int|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    # the C struct: every member the binding lists as a field, in that order, then the switch, last.  The binding keeps
    # what was appended behind amg_cheb_ratio in a tail behind its fields (_lib.Opts._TAIL), at the offset the
    # struct gives it: the fields end on a multiple of 8 (a double is the last of them), an int follows at once
    assert members == [f for f, _ in _lib.Opts._fields_] + ["fsai_blocks"]
    assert C.sizeof(_lib.Opts) % 8 == 0 and _lib.Opts._TAIL["fsai_blocks"] == (0, C.c_int)
    # both directions through the library, which knows the struct's real layout; no field moves
    lib = _lib.load()
    before, got = _lib.Opts(), _lib.Opts()
    lib.lsb_hip_get_opts(C.byref(before))
    try:
        lib.lsb_hip_set_opts(C.byref(la.default_opts(fsai_blocks=1, maxit=77, amg_cheb_ratio=3.5)))
        lib.lsb_hip_get_opts(C.byref(got))
        ref = la.default_opts(maxit=77, amg_cheb_ratio=3.5)
        assert got.fsai_blocks == 1
        assert all(getattr(got, f) == getattr(ref, f) for f, _ in _lib.Opts._fields_)
    finally:
        lib.lsb_hip_set_opts(C.byref(before))


def test_set_option_round_trips():
    lib = _lib.load()
    o = _lib.Opts()
    lib.lsb_hip_get_opts(C.byref(o))
    before = o.fsai_blocks
    try:
        assert lib.hip_cdna4_set_option(b"fsai-blocks", b"1") == 0
        lib.lsb_hip_get_opts(C.byref(o))
        assert o.fsai_blocks == 1
        assert lib.hip_cdna4_set_option(b"fsai_blocks", b"0") == 0
        lib.lsb_hip_get_opts(C.byref(o))
        assert o.fsai_blocks == 0
    finally:
        lib.hip_cdna4_set_option(b"fsai-blocks", b"%d" % before)


def test_the_function_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert NAME in _lib.SIGNATURES and hasattr(lib.hip, NAME)
    assert isinstance(la.Solver.fsai_nnz, property)
    assert lib.lsb_hip_solver_fsai_nnz(None, None, None) == 2
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "lsb_core.c")) as f:
        assert "--fsai-blocks" in f.read()


def test_cpu_precondition_the_columns_stop_at_different_iterations(matrix_path):
    """What the GPU tests lean on: with the oracle's FSAI-PCG on xn3b_A_18 every column converges, the columns take
    at least three distinct iteration counts, and at power 3, tol = 1e-12 e0 stops at least 13 iterations before i.
    Measured when this was written, (power, tol): (i, e0, sin i, ones, normal):
      (1, 1e-12): 115, 88, 111, 115, 111    (3, 1e-12): 52, 39, 50, 52, 49    (3, 1e-6): 31, 15, 29, 30, 28"""
    path = matrix_path("xn3b_A_18")
    for power, tol in ((1, 1e-12), (3, 1e-12), (3, 1e-6)):
        orc = _oracle(path, power, tol)
        its = [it for _, it, _ in orc]
        print("power", power, "tol", tol, dict(zip(NAMES5, its)))
        assert all(st == CONVERGED for _, _, st in orc)
        assert len(set(its)) >= 3 and min(its) > 7
    its = [it for _, it, _ in _oracle(path, 3, 1e-12)]
    assert its[0] - its[1] >= 13


# ------------------------------------------------------------------------------------ on the GPU
def _solver(hip, A, kw=None, **more):
    o = dict(kw or {})
    o.update(more)
    o.setdefault("precond", hip.PRECOND_FSAI)
    o.setdefault("fsai_blocks", 1)
    return hip.Solver(A, hip.default_opts(**o))


def _apply_multi(s, R, gap=3):
    """Z of precond_multi_dev with ldr = n + 5, ldz = n + gap; the rows behind n hold a NaN sentinel that survives"""
    import torch
    n, k = R.shape
    d_Z = torch.full((k + 1, n + gap), float("nan"), dtype=torch.float64, device="cuda:0")
    s.precond_multi_dev(_block(R, n + 5), d_Z[:k])
    assert bool(torch.isnan(d_Z[:k, n:]).all()) and bool(torch.isnan(d_Z[k]).all())  # behind n, and beyond nrhs
    Z = _host(d_Z[:k], n)
    assert np.isfinite(Z).all()
    return Z


def _apply_single(s, R):
    import torch
    out = np.empty_like(R)
    d_z = torch.empty(R.shape[0], dtype=torch.float64, device="cuda:0")
    for c in range(R.shape[1]):
        s.precond_dev(torch.from_numpy(np.ascontiguousarray(R[:, c])).to("cuda:0"), d_z)
        out[:, c] = d_z.cpu().numpy()
    return out


def _check_apply(s, R3, ref, widths, what):
    """error / bound <= 1 per column of precond_multi_dev on the columns of R3 repeated up to every width"""
    zs3, beta3 = fsai_exact(ref, R3)
    Z1 = _apply_single(s, R3)
    for nrhs in widths:
        idx = [c % R3.shape[1] for c in range(nrhs)]
        Z = _apply_multi(s, R3[:, idx])
        ratio = fsai_ratio(Z, zs3[:, idx], beta3[:, idx])
        same = [Z[:, c].tobytes() == Z1[:, idx[c]].tobytes() for c in range(nrhs)]
        print("%s nrhs %d: error / bound %s; the bits of precond_dev: %s" % (what, nrhs, ratio, same))
        assert (ratio <= 1.0).all(), (what, nrhs, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("case", APPLY_CASES, ids=lambda c: "%s-power%d" % c)
def test_block_apply_against_the_exact_reference(hip, monkeypatch, case, matrix_path):
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    S, A, kw, R, ref = fsai_setup(case, matrix_path)
    s = _solver(hip, A, kw, fsai_power=case[1])
    _check_apply(s, R, ref, (2, 3, 8, 11), "FSAI %r" % (case,))
    s.destroy()


def _small_operators(hip, matrix_path):
    """name -> (Matrix, options, the operator as scipy): G diagonal and n below one workgroup's slot count; two rows"""
    two = sp.csr_matrix(np.array([[2.0, -1.0], [-1.0, 3.0]]))
    return {"I1_05x05": (hip.lsbench_matrix_read(matrix_path("I1_05x05")), {}, oracle_operator(matrix_path("I1_05x05"))[1]),
            "two_rows": (_scipy_matrix(hip, two), dict(op_mode=hip.OP_RAW), two)}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 4, 8, 16, 32, 64])
def test_every_lane_count(hip, lanes, matrix_path, monkeypatch):
    """LSBENCH_HIP_MRHS_FSAI_LANES at power 2: the block apply within its bound, and -- the row kernels of the
    iteration, at every width -- solves at 1e-8 whose recomputed residual is within twice the tolerance (the
    recurrence's is within it; the two differ by rounding, orders of magnitude below 1e-8) and whose iteration counts
    follow the oracle's."""
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    monkeypatch.setenv("LSBENCH_HIP_MRHS_FSAI_LANES", str(lanes))
    tol = 1e-8
    S, A, kw, R, ref = fsai_setup(("xn3b_A_18", 2), matrix_path)
    s = _solver(hip, A, kw, fsai_power=2, tol=tol)
    _check_apply(s, R, ref, (2, 3, 8), "lanes %d" % lanes)
    B = five(S.shape[0])
    orc = _oracle(matrix_path("xn3b_A_18"), 2, tol)
    for k in (2, 3, 5):
        X, res = _solve(s, B[:, :k])
        for c in range(k):
            print("lanes", lanes, "width", k, NAMES5[c], res[c].iters, "oracle", orc[c][1], relres(S, X[:, c], B[:, c]))
            assert res[c].status == CONVERGED and abs(int(res[c].iters) - orc[c][1]) <= _margin(orc[c][1])
            assert relres(S, X[:, c], B[:, c]) <= 2 * tol
    s.destroy()
    for name, (M, okw, So) in _small_operators(hip, matrix_path).items():
        n = So.shape[0]
        s = _solver(hip, M, okw, fsai_power=2, tol=tol)
        R = np.stack([np.sin(np.arange(n)) + 0.5, np.random.default_rng(3).standard_normal(n), np.eye(n)[:, n - 1]], axis=1)
        _check_apply(s, R, fsai_reference((name, 2), So.tocsr(), 2), (2, 3, 8), "%s lanes %d" % (name, lanes))
        X, res = _solve(s, R)
        for c in range(3):
            assert res[c].status == CONVERGED and relres(So, X[:, c], R[:, c]) <= 2 * tol
        s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [1e-6, 1e-12])
@pytest.mark.parametrize("power", [1, 3])
def test_solves_match_the_oracle_per_column(hip, power, tol, matrix_path, golden_x):
    path = matrix_path("xn3b_A_18")
    A = hip.lsbench_matrix_read(path)
    B = five(A.nrows)
    orc = _oracle(path, power, tol)
    xs = {}
    for graph in (0, 1):
        s = _solver(hip, A, fsai_power=power, tol=tol, use_graph=graph)
        X, res = _solve(s, B)
        for c in range(5):
            xo, ito, sto = orc[c]
            err = relerr(X[:, c], xo)
            print("power", power, "tol", tol, NAMES5[c], "iters", res[c].iters, "oracle", ito, "error", err)
            assert res[c].status == CONVERGED and sto == CONVERGED
            assert abs(int(res[c].iters) - ito) <= _margin(ito)
            if tol == 1e-12:
                assert err <= 1e-10
        assert len({r.spmvs for r in res}) == 1 and res[0].spmvs == max(r.iters for r in res)
        X2, res2 = _solve(s, B)  # a second call repeats the first
        assert X2.tobytes() == X.tobytes() and [r.iters for r in res2] == [r.iters for r in res]
        s.destroy()
        xs[graph] = X
    assert xs[0].tobytes() == xs[1].tobytes()
    if tol == 1e-12:
        assert relerr(xs[0][:, 0], golden_x("xn3b_A_18")) <= 1e-10


@pytest.mark.gpu
def test_columns_do_not_see_each_other(hip, matrix_path):
    """Column i beside different neighbours at the same Kp = 4 -- e0, which stops 13 iterations earlier, a zero
    column, and alone among zeros -- has the same x bits and iteration count."""
    path = matrix_path("xn3b_A_18")
    A = hip.lsbench_matrix_read(path)
    B5 = five(A.nrows)
    zero = np.zeros(A.nrows)
    s = _solver(hip, A, fsai_power=3, tol=1e-12)
    X, res = _solve(s, np.stack([B5[:, 0], B5[:, 1], B5[:, 2], B5[:, 4]], axis=1))
    assert res[0].iters - res[1].iters >= 13 - 2 * 2  # (each count within the oracle's margin of 2)
    for at, Bn in ((0, np.stack([B5[:, 0], zero, zero, zero], axis=1)),
                   (0, np.stack([B5[:, 0], zero, B5[:, 3], B5[:, 1]], axis=1)),
                   (2, np.stack([B5[:, 4], B5[:, 1], B5[:, 0], zero], axis=1))):
        Xn, resn = _solve(s, Bn)
        assert Xn[:, at].tobytes() == X[:, 0].tobytes() and resn[at].iters == res[0].iters
        for c in range(4):
            if not Bn[:, c].any():
                assert resn[c].status == CONVERGED and resn[c].iters == 0 and not Xn[:, c].any()
    s.destroy()


@pytest.mark.gpu
def test_one_column_is_solve_dev_and_eleven_run_as_two_batches(hip, matrix_path):
    import torch
    path = matrix_path("xn3b_A_18")
    A = hip.lsbench_matrix_read(path)
    n = A.nrows
    B5 = five(n)
    s = _solver(hip, A, fsai_power=3, tol=1e-12)
    d_x = torch.empty(n, dtype=torch.float64, device="cuda:0")
    r1 = s.solve_dev(torch.from_numpy(np.ascontiguousarray(B5[:, 0])).to("cuda:0"), d_x)
    X, res = _solve(s, B5[:, :1])
    assert X[:, 0].tobytes() == d_x.cpu().numpy().tobytes() and (res[0].iters, res[0].status) == (r1.iters, r1.status)
    rng = np.random.default_rng(11)
    B11 = np.concatenate([B5, np.stack([3.0 * B5[:, 0] + B5[:, 3], rng.standard_normal(n), np.zeros(n), B5[:, 0],
                                        rng.standard_normal(n), 0.5 * B5[:, 3]], axis=1)], axis=1)
    X, res = _solve(s, B11)
    X8, res8 = _solve(s, B11[:, :8])
    X3, res3 = _solve(s, B11[:, 8:])
    s.destroy()
    assert len({r.seconds for r in res[:8]}) == 1 and len({r.seconds for r in res[8:]}) == 1
    assert res[0].seconds != res[8].seconds
    assert X[:, :8].tobytes() == X8.tobytes() and X[:, 8:].tobytes() == X3.tobytes()
    assert [r.iters for r in res] == [r.iters for r in res8] + [r.iters for r in res3]
    orc = _oracle(path, 3, 1e-12)
    for c in range(11):
        if not B11[:, c].any():
            assert res[c].status == CONVERGED and res[c].iters == 0 and not X[:, c].any()
        else:
            assert res[c].status == CONVERGED
    for c in range(5):
        assert relerr(X[:, c], orc[c][0]) <= 1e-10
    assert relerr(X[:, 8], orc[0][0]) <= 1e-10  # column 8 is column 0's b, in the second batch (Kp = 4)


@pytest.mark.gpu
def test_stop_rules_maxit(hip, matrix_path):
    path = matrix_path("xn3b_A_18")
    A = hip.lsbench_matrix_read(path)
    B = five(A.nrows)
    orc = _oracle(path, 2, 1e-12, 7)
    s = _solver(hip, A, fsai_power=2, tol=1e-12, maxit=7)
    X, res = _solve(s, B)
    s.destroy()
    for c in range(5):
        xo, ito, sto = orc[c]
        print(NAMES5[c], res[c].iters, res[c].status, relerr(X[:, c], xo))
        assert res[c].status == MAXIT and res[c].iters == 7 == ito
        assert relerr(X[:, c], xo) <= 1e-9
    assert res[0].spmvs == 7


@pytest.mark.gpu
def test_warm_start(hip, matrix_path):
    path = matrix_path("xn3b_A_18")
    _, S = oracle_operator(path)
    n = S.shape[0]
    B = five(n)
    tol = 1e-12
    orc = _oracle(path, 3, tol)
    s = _solver(hip, hip.lsbench_matrix_read(path), fsai_power=3, tol=tol, verify=1)
    X12, _ = _solve_block(s, B, np.zeros_like(B), False)  # "converged" is the recomputed residual's
    s.destroy()
    rng = np.random.default_rng(9)
    # i: x* + 1e-3 noise; e0: x0 = 0; sin i: the converged x; ones: x* + 1e-3 noise; normal: x0 = 0
    X0 = np.stack([orc[0][0] + 1e-3 * rng.standard_normal(n), np.zeros(n), X12[:, 2],
                   orc[3][0] + 1e-3 * rng.standard_normal(n), np.zeros(n)], axis=1)
    s = _solver(hip, hip.lsbench_matrix_read(path), fsai_power=3, tol=tol)
    Xc, rc = _solve_block(s, B, np.zeros_like(B), False)
    Xw, rw = _solve_block(s, B, X0, True)
    start = s.start_relres(5)
    Xw2, rw2 = _solve_block(s, B, X0, True)
    s.destroy()
    print([(r.iters, r.status) for r in rc], [(r.iters, r.status) for r in rw], start)
    for c in (0, 3):
        assert rw[c].status == CONVERGED and 0 < rw[c].iters < rc[c].iters
        assert relerr(Xw[:, c], orc[c][0]) <= 1e-10
    for c in (1, 4):  # x0 = 0: the column of the cold batch
        assert np.array_equal(Xw[:, c], Xc[:, c])
        assert (rw[c].iters, rw[c].status, rw[c].relres) == (rc[c].iters, rc[c].status, rc[c].relres)
        assert start[c] == 1.0
    assert rw[2].status == CONVERGED and rw[2].iters == 0 and Xw[:, 2].tobytes() == X0[:, 2].tobytes()
    for c in (0, 3):
        ref = relres_exact(S, X0[:, c], B[:, c])
        print(NAMES5[c], "start_relres", start[c], "numpy, extended precision", ref)
        assert abs(start[c] - ref) <= 1e-10 * ref
    assert Xw2.tobytes() == Xw.tobytes() and [r.iters for r in rw2] == [r.iters for r in rw]


@pytest.mark.gpu
def test_verify_at_1e13(hip, matrix_path):
    path = matrix_path("xn3b_A_18")
    _, S = oracle_operator(path)
    B = five(S.shape[0])
    tol = 1e-13
    A = hip.lsbench_matrix_read(path)
    s = _solver(hip, A, fsai_power=3, tol=tol, verify=1)
    X, res = _solve(s, B)
    X2, res2 = _solve(s, B)
    s.destroy()
    s = _solver(hip, A, fsai_power=3, tol=tol, verify=0)
    X0, res0 = _solve(s, B)
    s.destroy()
    print([(r.iters, r.status, r.corrections, r.true_relres) for r in res])
    assert all(r.true_relres < 0.0 and r.corrections == 0 for r in res0)
    for c in range(5):
        assert res[c].status in (CONVERGED, MAXIT) and 0 <= res[c].corrections <= 6
        cpu = relres_exact(S, X[:, c], B[:, c])
        print(NAMES5[c], "true_relres", res[c].true_relres, "cpu, exact", cpu)
        if res[c].status == CONVERGED:
            assert 0.0 <= res[c].true_relres <= tol
            assert abs(res[c].true_relres - cpu) <= 1e-3 * cpu  # (test_mrhs.py's margin for the same launch)
        if res[c].corrections == 0:  # did not restart: the bits of the run without verify
            assert X[:, c].tobytes() == X0[:, c].tobytes() and res[c].iters == res0[c].iters
    assert any(r.status == CONVERGED for r in res)
    assert X2.tobytes() == X.tobytes()
    assert [(r.iters, r.corrections, r.true_relres) for r in res2] == [(r.iters, r.corrections, r.true_relres) for r in res]


@pytest.mark.gpu
def test_reordered_solver(hip, matrix_path):
    path = matrix_path("xn3b_A_18")
    A = hip.lsbench_matrix_read(path)
    B = five(A.nrows)
    out = []
    for reorder in (0, 1):
        s = _solver(hip, A, fsai_power=2, tol=1e-12, reorder=reorder)
        out.append(_solve(s, B))
        s.destroy()
    (X0, r0), (X1, r1) = out
    for c in range(5):
        print(NAMES5[c], r0[c].iters, r1[c].iters, relerr(X1[:, c], X0[:, c]))
        assert r1[c].status == CONVERGED and relerr(X1[:, c], X0[:, c]) <= 1e-10


@pytest.mark.gpu
def test_refusals_that_remain_bicgstab(hip, matrix_path):
    """BiCGSTAB takes the diagonal preconditioners only: with --precond fsai the library refuses to create the solver
    at all (the process exits with a message), with the switch as without it, so there is no handle to ask for a
    block.  Through the driver, which also carries --fsai-blocks from the command line to the option table."""
    import subprocess
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    r = subprocess.run([drv, "--solver", "hip", "--matrix", matrix_path("xn3b_A_18"), "--precond", "fsai",
                        "--fsai-blocks", "1", "--krylov", "bicgstab", "--trials=1"], capture_output=True, text=True)
    assert r.returncode != 0 and "bicgstab" in r.stderr and "FSAI" in r.stderr and "fsai-blocks" not in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(krylov="KRYLOV_PCG1"), dict(krylov="KRYLOV_GMRES"),
                                dict(precision="PREC_MIXED")], ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_refusals_that_remain(hip, kw, matrix_path):
    import torch
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    s = _solver(hip, A, {k: getattr(hip, v) for k, v in kw.items()}, fsai_power=1)
    lib = _lib.load()
    d_B = torch.ones(2, n, dtype=torch.float64, device="cuda:0")
    d_X = torch.full((2, n), 0.25, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_multi_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
    assert lib.lsb_hip_solver_solve_multi_x0_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n) == 2
    assert bool((d_X == 0.25).all())
    assert s.multi_iteration_bytes(2) == 0
    s.destroy()


@pytest.mark.gpu
def test_multi_iteration_bytes(hip, matrix_path):
    """The formula of the module's docstring, with what the solver reports of itself; the switch is ignored under
    another preconditioner."""
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    for power in (1, 3):
        s = _solver(hip, A, fsai_power=power)
        n, nnz = s.n_local, s.nnz_local
        g, gt = s.fsai_nnz
        assert g == gt > n and s.padded == 0
        for nrhs, kp in ((2, 2), (3, 4), (8, 8)):
            assert s.multi_iteration_bytes(nrhs) == 12 * (nnz + g + gt) + 12 * (n + 1) + 8 * n * 16 * kp
        s.destroy()
    s = hip.Solver(A, hip.default_opts(fsai_blocks=1))
    n, nnz = s.n_local, s.nnz_local
    assert s.fsai_nnz is None
    assert s.multi_iteration_bytes(8) == 12 * nnz + 4 * (n + 1) + 8 * n * (11 * 8 + 2)
    s.destroy()
