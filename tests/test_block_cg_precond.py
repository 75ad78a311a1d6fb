"""Block-CG under FSAI and AMG (lsb_hip_solver_solve_block_precond[_dev], hip_bcg_m.hip): ONE Krylov space for a block of
right-hand sides, preconditioned by an operator.

The yardstick is block_pcg_m below: test_block_cg.block_pcg with D^-1 replaced by a linear callable M on blocks --
Z = M(B), P = Z sigma^-1, G = W~^T M(W~), P = M(W~) zeta^-1 + P zeta^T, the two directions formed as M(W) -- checked
on its own without a GPU against block_pcg (M = diag(S)^-1) and against the single-column PCG of test_amg under the numpy V-cycle and under the FSAI reference of
test_precond_apply.  On the GPU its M is the solver's own precond_multi_dev, which test_precond_apply.py,
test_mrhs_fsai.py and test_mrhs_amg.py check against exact references: the comparison then isolates the new code.

Figures seen on an MI355X are in the docstrings of the tests."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from test_amg import Hier, pcg
from test_block_cg import (BREAKDOWN, CONVERGED, MAXIT, PIVOT_FLOOR, RUNNING, WIDTHS, _operator, _path, _relerr_cols,
                           _solver, _xref, block_pcg, columns8)
from test_mrhs import _block, _host, _lap2d, relres_exact
from test_precond_apply import fsai_reference

THREE = ("lsb_hip_solver_solve_block_precond_dev", "lsb_hip_solver_solve_block_precond",
         "lsb_hip_solver_block_precond_iteration_bytes")
OPERATORS = ("xn3b_A_18", "tj7a_A_18", "lap2d")
FSAI_POWER = 3  # lsb_hip_opts_default's
RATIO_FLOOR = 0.09  # the Gram matrices' eigenvalue ratio test_block_cg.py's bounds for the cuts rest on


# ------------------------------------------------------------------------------------ the restatement
def _sym(A):
    return np.triu(A) + np.triu(A, 1).T  # the kernels keep the upper triangle


def _ratio(A):
    """smallest / largest eigenvalue of A scaled to unit diagonal"""
    d = np.sqrt(np.diag(A))
    ev = np.linalg.eigvalsh(A / np.outer(d, d))
    return float(ev[0] / ev[-1])


def block_pcg_m(S, B, M, tol, maxit=20000):
    """-> dict(rc, X, iters, status[k], rr[k], bb[k], relres[k], nspmm, ratio_gamma, ratio_g).  M: (n, k) -> (n, k),
    linear, symmetric positive definite.  rc 3: rank-deficient at the start.  ratio_*: the smallest eigenvalue ratio of
    the unit-diagonal Gamma and G the run met.
    The preconditioned direction M(W~) zeta^-1 is formed as M(W~ zeta^-1) = M(W): M is applied to the normalised block,
    as block_pcg applies D^-1 to W, at the price of a second application of M per iteration (the Gram matrix needs
    M(W~)).  The two are the same matrix by linearity -- the device forms the first, from its stored Z~ -- and with
    M = diag(S)^-1 every operation of the restatement is then block_pcg's, bit for bit."""
    n, k = B.shape
    Z = M(B)
    G = B.T @ Z  # (as block_pcg: not mirrored here; the two triangles differ by the product's rounding)
    bb = np.einsum("ic,ic->c", B, B)
    out = dict(rc=0, X=np.zeros((n, k)), iters=0, status=[BREAKDOWN] * k, rr=bb.copy(), bb=bb, nspmm=0,
               ratio_gamma=1.0, ratio_g=1.0)
    d = np.sqrt(np.diag(G))
    with np.errstate(all="ignore"):
        Gs = G / np.outer(d, d)  # a zero column: 0 / 0, a pivot that is not finite
    try:
        Ls = np.linalg.cholesky(Gs)
        piv = np.diag(Ls) ** 2
    except np.linalg.LinAlgError:
        piv = np.array([0.0])
    if not np.all(np.isfinite(Gs)) or not np.all(np.isfinite(piv)) or piv.min() <= PIVOT_FLOOR:
        out["rc"] = 3
        return out
    L = d[:, None] * Ls
    sigma = L.T.copy()
    W = sl.solve_triangular(L, B.T, lower=True).T  # B sigma^-1
    P = M(W)  # = Z sigma^-1: M is linear
    X = np.zeros((n, k))
    thr = tol * tol * bb
    status = [RUNNING] * k
    it = nspmm = 0
    rr = bb.copy()
    rgam, rg = 1.0, _ratio(G)
    if maxit <= 0:
        status = [MAXIT] * k
    while status[0] == RUNNING:
        Q = S @ P
        nspmm += 1
        Gam = _sym(P.T @ Q)
        try:
            Cf = np.linalg.cholesky(Gam)
        except np.linalg.LinAlgError:
            status = [BREAKDOWN] * k
            break
        rgam = min(rgam, _ratio(Gam))
        Ci = sl.solve_triangular(Cf, np.eye(k), lower=True)
        xi = Ci.T @ Ci
        X += P @ (xi @ sigma)
        Wt = W - Q @ xi
        Zt = M(Wt)
        G = _sym(Wt.T @ Zt)
        H = Wt.T @ Wt
        rr = np.einsum("ic,ij,jc->c", sigma, H, sigma)
        it += 1
        if np.all(rr <= thr):
            status = [CONVERGED] * k
            break
        if it >= maxit:
            status = [CONVERGED if rr[c] <= thr[c] else MAXIT for c in range(k)]
            break
        try:
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            status = [BREAKDOWN] * k
            break
        rg = min(rg, _ratio(G))
        zeta = L.T
        W = sl.solve_triangular(L, Wt.T, lower=True).T  # Wt zeta^-1
        P = M(W) + P @ zeta.T  # M(W) = Zt zeta^-1: M is linear
        sigma = zeta @ sigma
    out.update(X=X, iters=it, status=status, rr=rr, relres=np.sqrt(rr / bb), nspmm=nspmm, ratio_gamma=rgam,
               ratio_g=rg)
    return out


# ------------------------------------------------------------------------------------ the CPU's preconditioners
@functools.lru_cache(maxsize=None)
def _cpu_m(kind, name, path):
    """M on blocks: the numpy V-cycle of test_amg column by column, or G^T (G .) with the fp64 factor of
    test_precond_apply.fsai_reference (its G "by float64 Cholesky", the product's way)"""
    S, _ = _operator(name, path)
    n = S.shape[0]
    if kind == "amg":
        H = Hier(S)
        return lambda R: np.stack([H.vcycle(np.ascontiguousarray(R[:, c])) for c in range(R.shape[1])], axis=1)
    offs, cols, rows, mi, gs, g64, cond = fsai_reference(("block_cg_precond", name, FSAI_POWER), S, FSAI_POWER)
    G = sp.csr_matrix((g64, cols, offs), shape=(n, n))
    Gt = G.T.tocsr()
    return lambda R: Gt @ (G @ R)


@functools.lru_cache(maxsize=None)
def _cpu_single(kind, name, path, tol):
    S, B = _operator(name, path)
    M = _cpu_m(kind, name, path)
    return [pcg(S, np.ascontiguousarray(B[:, c]), lambda r: M(r[:, None])[:, 0], tol)[1] for c in range(8)]


# ------------------------------------------------------------------------------------ without a GPU
def test_the_three_functions_are_declared_exported_and_bound():
    import inspect
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in THREE:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib.hip, name)
    assert callable(la.Solver.block_precond_iteration_bytes)
    for m in ("solve_block_dev", "solve_block"):
        assert inspect.signature(getattr(la.Solver, m)).parameters["precond"].default is False
    up = int(lib.hip.lsb_hip_is_initialized())
    res = _lib.Result()
    assert lib.lsb_hip_solver_solve_block_precond_dev(None, 2, None, 0, None, 0, C.byref(res)) == (2 if up else 1)
    assert lib.lsb_hip_solver_solve_block_precond(None, 2, None, 0, None, 0, C.byref(res)) == (2 if up else 1)
    assert lib.lsb_hip_solver_block_precond_iteration_bytes(None, 2) == 0


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("name", OPERATORS)
def test_cpu_the_restatement_under_the_diagonal_is_block_pcg(name, k, matrix_path):
    """With M = diag(S)^-1 every operation of the restatement is block_pcg's (it applies M to W = W~ zeta^-1, as
    block_pcg applies D^-1), so the two agree bit for bit: the same count and statuses at tol 1e-10, X 0 apart, where
    1e-12 relative is asserted.  (Formed as (D^-1 W~) zeta^-1 the direction differs by one rounding per element, and
    after 140 .. 250 iterations at this tolerance that moves the count by one in one or two of the twelve cases: the
    recurrence's ||r||^2 at the stop is then tens of per cent apart.)"""
    path = _path(name, matrix_path)
    S, B8 = _operator(name, path)
    dinv = 1.0 / S.diagonal()
    y = block_pcg(S, B8[:, :k], 1e-10)
    m = block_pcg_m(S, B8[:, :k], lambda R: dinv[:, None] * R, 1e-10)
    err = _relerr_cols(m["X"], y["X"])
    print(name, k, "iters", m["iters"], y["iters"], "X apart", max(err))
    assert m["rc"] == y["rc"] == 0 and m["iters"] == y["iters"] and m["status"] == y["status"]
    assert m["nspmm"] == y["nspmm"] and max(err) <= 1e-12


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("name", OPERATORS)
@pytest.mark.parametrize("kind", ["fsai", "amg"])
def test_cpu_the_restatement_converges_in_no_more_iterations_than_the_slowest_column(kind, name, k, matrix_path):
    """Seen at tol 1e-10, block at k = 2, 3, 4, 8 / slowest single column of the 8.  FSAI(3) on the project's capped
    pattern: xn3b 39, 35, 33, 26 / 45; tj7a 50, 46, 42, 36 / 58; lap2d 33, 29, 25, 20 / 42 -- the block of 8 takes 0.58,
    0.62 and 0.48 of the slowest column's count, and <= 0.75 is asserted.  The numpy V-cycle: xn3b 103, 100, 95, 88 /
    108; tj7a 96, 95, 95, 93 / 99; lap2d 18, 18, 18, 18 / 18 -- the order alone is asserted (against the slowest of the
    block's own columns).  Smallest eigenvalue ratio of the unit-diagonal Gram matrices met: Gamma 0.39 .. 0.92
    everywhere; G under FSAI 0.19 (xn3b, k = 2), 4e-4 (xn3b, k >= 3: the column e0), 0.11 .. 0.21 (tj7a), 0.065 .. 0.097
    (lap2d); under the V-cycle 0.033 .. 0.039 (xn3b), 0.052 (tj7a), 4e-3 (lap2d)."""
    tol = 1e-10
    path = _path(name, matrix_path)
    S, B = _operator(name, path)
    y = block_pcg_m(S, B[:, :k], _cpu_m(kind, name, path), tol)
    single = _cpu_single(kind, name, path, tol)
    worst = max(relres_exact(S, y["X"][:, c], B[:, c]) for c in range(k))
    print(kind, name, k, "block", y["iters"], "single", single, "recomputed", worst, "ratios", y["ratio_gamma"],
          y["ratio_g"])
    assert y["rc"] == 0 and y["status"] == [CONVERGED] * k
    assert y["iters"] <= max(single[:k])
    assert worst <= tol
    if kind == "fsai" and k == 8:
        assert y["iters"] <= 0.75 * max(single)


def test_cpu_the_restatement_applies_the_rank_rule():
    S = _lap2d(40, 30).tocsr()
    dinv = 1.0 / S.diagonal()
    B = columns8(S)[:, :3].copy()
    B[:, 2] = B[:, 0]
    assert block_pcg_m(S, B, lambda R: dinv[:, None] * R, 1e-10)["rc"] == 3
    B[:, 2] = 0.0
    assert block_pcg_m(S, B, lambda R: dinv[:, None] * R, 1e-10)["rc"] == 3


# ------------------------------------------------------------------------------------ on the GPU
CONFIGS = {"fsai": dict(precond=_lib.PRECOND_FSAI, fsai_blocks=1),
           "amg": dict(precond=_lib.PRECOND_AMG),
           "amg-cheb": dict(precond=_lib.PRECOND_AMG, amg_smoother=_lib.AMG_SMOOTH_CHEB)}
CASES = [("fsai", "xn3b_A_18"), ("fsai", "tj7a_A_18"), ("amg", "xn3b_A_18"), ("amg", "lap2d"),
         ("amg-cheb", "xn3b_A_18"), ("amg-cheb", "lap2d")]
CASE_IDS = ["%s-%s" % c for c in CASES]


def _solve_block_m(s, B, pad=5, fill=-7.0):
    """-> (rc, X, [Result], the slack is untouched)"""
    import torch
    n, k = B.shape
    d_B = _block(B, n + pad)
    d_X = torch.full((k, n + pad + 2), fill, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * k)()
    rc = _lib.load().lsb_hip_solver_solve_block_precond_dev(s._h, k, d_B.data_ptr(), n + pad, d_X.data_ptr(),
                                                            n + pad + 2, res)
    assert bool((d_X[:, n:] == fill).all())  # the slack behind a column is the caller's
    return rc, _host(d_X, n), list(res)


def _device_m(s, n):
    """the solver's own z = M^-1 r on blocks"""
    import torch

    def M(R):
        d_R = _block(np.ascontiguousarray(R), n)
        d_Z = torch.zeros_like(d_R)
        s.precond_multi_dev(d_R, d_Z)
        return _host(d_Z, n)
    return M


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_parity_with_the_restatement(hip, case, k, matrix_path):
    """Seen: the restatement's count in every one of the 48 runs.  Iterations at tol 1e-10 / 1e-12 for k = 2, 3, 4, 8 --
    FSAI: xn3b 39 / 44, 35 / 40, 33 / 37, 26 / 30 against 45 / 52 of solve_multi's slowest column; tj7a 50 / 55, 46 / 51,
    42 / 47, 36 / 40 against 58 / 66.  AMG, l1-Jacobi: xn3b 103 / 119, 100 / 115, 95 / 109, 88 / 101 against 108 / 128;
    lap2d 18 / 21 at every width against 18 / 22.  AMG, Chebyshev: xn3b 84 / 98, 82 / 95, 78 / 91, 71 / 82 against
    88 / 104; lap2d 18 / 21, 18 / 21, 17 / 21, 17 / 20 against 18 / 21.  At 1e-12 the errors against x_ref stay below
    1.6e-13; at 1e-10 the recomputed residuals below 9.53e-11."""
    import torch
    cfg, name = case
    path = _path(name, matrix_path)
    S, B8 = _operator(name, path)
    B = B8[:, :k]
    n = S.shape[0]
    for tol in (1e-10, 1e-12):
        s = _solver(hip, name, matrix_path, tol=tol, **CONFIGS[cfg])
        assert s.n_local == n
        y = block_pcg_m(S, B, _device_m(s, n), tol)
        rc, X, res = _solve_block_m(s, B)
        rr, bb = s.block_norms(k)
        d_X = torch.zeros(k, n, dtype=torch.float64, device="cuda:0")
        multi = s.solve_multi_dev(_block(B, n), d_X)
        s.destroy()
        it = res[0].iters
        print(cfg, name, k, tol, "iters", it, "restatement", y["iters"], "solve_multi", [r.iters for r in multi],
              "relres", [r.relres for r in res])
        assert rc == 0 and all(r.status == CONVERGED for r in res)
        assert all(r.iters == it for r in res) and res[0].spmvs == it
        assert abs(it - y["iters"]) <= max(2, y["iters"] // 25)
        if cfg == "fsai":
            assert it <= max(r.iters for r in multi)
        for c in range(k):
            assert res[c].relres == np.sqrt(rr[c] / bb[c]) and res[c].relres <= tol
            assert res[c].true_relres < 0.0
        if tol == 1e-12:
            err = _relerr_cols(X, _xref(name, path)[:, :k])
            print("   error against x_ref", err)
            assert max(err) <= 1e-10
        else:
            true = [relres_exact(S, X[:, c], B[:, c]) for c in range(k)]
            print("   recomputed", true)
            assert max(true) <= 2 * tol  # (the factor 2: an allowance for recurrence drift)


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_maxit_cuts(hip, case, k, matrix_path):
    """The cuts at 1, 2, 3 and 8 iterations against the restatement under the solver's own M.  Bounds: test_block_cg.py's
    -- 1e-13 relative at one iteration, 1e-11 at two and three -- which rest on the unit-diagonal Gram matrices'
    eigenvalue ratio staying >= 0.09; where the restatement meets a smaller ratio of Gamma or G up to the cut the bound
    is scaled by 0.09 / ratio.
    Seen, smallest ratio of Gamma / of G up to the cut, and the largest error over the widths.  One iteration: Gamma
    0.73 .. 0.93, G 0.24 .. 0.57 (the start's alone), errors 3.0e-15 .. 5.7e-15.  Two, three and eight: FSAI xn3b 0.56 /
    3.9e-4 (the column e0), errors <= 5.5e-14; FSAI tj7a 0.45 / 0.11, <= 1.1e-14; AMG xn3b 0.63 / 0.033, <= 2.9e-15; AMG
    lap2d 0.91 / 4.1e-3, <= 1.7e-15; Chebyshev xn3b 0.65 / 0.028, <= 4.5e-15; lap2d 0.86 / 0.060, <= 1.0e-15 -- so the
    scaled bounds stand two to four orders above what is seen, and so would the unscaled ones."""
    cfg, name = case
    path = _path(name, matrix_path)
    S, B8 = _operator(name, path)
    B = B8[:, :k]
    n = S.shape[0]
    tol = 1e-10
    for m, bound in ((1, 1e-13), (2, 1e-11), (3, 1e-11), (8, None)):
        s = _solver(hip, name, matrix_path, tol=tol, maxit=m, **CONFIGS[cfg])
        y = block_pcg_m(S, B, _device_m(s, n), tol, m)
        rc, X, res = _solve_block_m(s, B)
        s.destroy()
        err = _relerr_cols(X, y["X"])
        ratio = min(y["ratio_gamma"], y["ratio_g"])
        print(cfg, name, k, "maxit", m, "ratios", y["ratio_gamma"], y["ratio_g"], "error against the restatement",
              max(err))
        assert rc == 0 and all(r.iters == m and r.spmvs == m for r in res)
        assert [r.status for r in res] == y["status"]
        if bound:
            assert max(err) <= bound * max(1.0, RATIO_FLOOR / ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,k", [("fsai", 3), ("fsai", 8), ("amg", 3), ("amg-cheb", 4)])
def test_the_bits_do_not_depend_on_how_the_loop_is_driven(hip, cfg, k, matrix_path):
    """Run to run, across two solvers, polled every iteration (the un-gated preconditioner launches behind the stop
    change nothing), without graphs, through host buffers, and on a second call that enqueues the hinted count."""
    S, B8 = _operator("xn3b_A_18", matrix_path("xn3b_A_18"))
    B = B8[:, :k]
    tol = 1e-10
    s1 = _solver(hip, "xn3b_A_18", matrix_path, tol=tol, **CONFIGS[cfg])
    s2 = _solver(hip, "xn3b_A_18", matrix_path, tol=tol, **CONFIGS[cfg])
    runs = [_solve_block_m(s1, B), _solve_block_m(s1, B), _solve_block_m(s2, B)]
    Xh, resh = s2.solve_block(B, precond=True)
    s1.destroy(), s2.destroy()
    for kw in (dict(check_every=1), dict(use_graph=0)):
        s = _solver(hip, "xn3b_A_18", matrix_path, tol=tol, **dict(CONFIGS[cfg], **kw))
        runs.append(_solve_block_m(s, B))
        s.destroy()
    rc, X, res = runs[0]
    assert rc == 0 and all(r.status == CONVERGED for r in res)
    for rc2, X2, res2 in runs[1:]:
        assert rc2 == 0 and X2.tobytes() == X.tobytes()
        assert [r.iters for r in res2] == [r.iters for r in res] and [r.relres for r in res2] == [r.relres for r in res]
    assert np.ascontiguousarray(Xh).tobytes() == X.tobytes()
    assert [r.iters for r in resh] == [r.iters for r in res] and [r.relres for r in resh] == [r.relres for r in res]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["fsai", "amg"])
def test_rank_rules(hip, cfg, matrix_path):
    S, B8 = _operator("xn3b_A_18", matrix_path("xn3b_A_18"))
    n = S.shape[0]
    tol = 1e-10
    s = _solver(hip, "xn3b_A_18", matrix_path, tol=tol, **CONFIGS[cfg])
    M = _device_m(s, n)
    dup = B8[:, :3].copy()
    dup[:, 2] = dup[:, 0]
    zero = B8[:, :4].copy()
    zero[:, 1] = 0.0
    for B in (dup, zero):
        rc, X, res = _solve_block_m(s, B, fill=7.0)
        assert rc == 3 and bool((X == 7.0).all()) and all(r.status == BREAKDOWN for r in res)
        assert block_pcg_m(S, B, M, tol)["rc"] == 3
    near = B8[:, :2].copy()
    near[:, 1] = near[:, 0] + 1e-3 * np.linalg.norm(near[:, 0]) / np.sqrt(n) * np.random.default_rng(3).standard_normal(n)
    rc, X, res = _solve_block_m(s, near)
    Xh, resh = s.solve_block(dup, precond=True)  # the host form of a refusal: every status BREAKDOWN
    s.destroy()
    true = [relres_exact(S, X[:, c], near[:, c]) for c in range(2)]
    print(cfg, "nearly dependent columns: iters", res[0].iters, "recomputed", true)
    assert rc == 0 and all(r.status == CONVERGED for r in res) and max(true) <= 2 * tol
    assert all(r.status == BREAKDOWN for r in resh)


@pytest.mark.gpu
def test_a_reordered_fsai_solver(hip, matrix_path):
    S, B8 = _operator("tj7a_A_18", matrix_path("tj7a_A_18"))
    B = B8[:, :4]
    tol = 1e-8
    s = _solver(hip, "tj7a_A_18", matrix_path, tol=tol, reorder=1, **CONFIGS["fsai"])
    rc, X, res = _solve_block_m(s, B)
    s.destroy()
    true = [relres_exact(S, X[:, c], B[:, c]) for c in range(4)]
    print("reorder=1: iters", res[0].iters, "recomputed", true)
    assert rc == 0 and all(r.status == CONVERGED for r in res) and max(true) <= 2 * tol


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["fsai", "amg"])
def test_verify_recomputes_the_residual(hip, cfg, matrix_path):
    S, B8 = _operator("xn3b_A_18", matrix_path("xn3b_A_18"))
    B = B8[:, :3]
    tol = 1e-10
    s = _solver(hip, "xn3b_A_18", matrix_path, tol=tol, verify=1, **CONFIGS[cfg])
    rc, X, res = _solve_block_m(s, B)
    s.destroy()
    assert rc == 0 and res[0].spmvs == res[0].iters + 1
    for c in range(3):
        cpu = relres_exact(S, X[:, c], B[:, c])
        print(cfg, "column", c, "status", res[c].status, "true_relres", res[c].true_relres, "cpu, exact", cpu)
        assert res[c].true_relres >= 0.0 and res[c].relres == res[c].true_relres
        assert abs(res[c].true_relres - cpu) <= 1e-3 * cpu  # test_mrhs.py's bound for the verify round
        assert res[c].status == (CONVERGED if res[c].true_relres <= tol else MAXIT)


@pytest.mark.gpu
def test_a_jacobi_solver_is_solve_block_and_one_column_is_solve_dev(hip, matrix_path):
    import torch
    S, B8 = _operator("xn3b_A_18", matrix_path("xn3b_A_18"))
    n = S.shape[0]
    B = B8[:, :3]
    lib = _lib.load()
    s = _solver(hip, "xn3b_A_18", matrix_path, tol=1e-10)
    rc, X, res = _solve_block_m(s, B)
    d_X = torch.zeros(3, n, dtype=torch.float64, device="cuda:0")
    plain = s.solve_block_dev(_block(B, n), d_X)
    assert s.block_precond_iteration_bytes(3) == s.block_iteration_bytes(3) > 0
    s.destroy()
    assert rc == 0 and X.tobytes() == _host(d_X, n).tobytes()
    assert [(r.iters, r.status, r.relres) for r in res] == [(r.iters, r.status, r.relres) for r in plain]
    # one column of a served solver is solve_dev
    s = _solver(hip, "xn3b_A_18", matrix_path, tol=1e-10, **CONFIGS["fsai"])
    d_B = _block(B, n)
    d_x = torch.empty(n, dtype=torch.float64, device="cuda:0")
    r1 = s.solve_dev(d_B[0], d_x)
    one = (_lib.Result * 1)()
    assert lib.lsb_hip_solver_solve_block_precond_dev(s._h, 1, d_B.data_ptr(), n, d_X.data_ptr(), n, one) == 0
    s.destroy()
    assert d_X[0].cpu().numpy().tobytes() == d_x.cpu().numpy().tobytes()
    assert one[0].iters == r1.iters and one[0].status == r1.status


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(precond="PRECOND_AMG", amg_smoother="AMG_SMOOTH_MCGS"),
                                dict(precond="PRECOND_AMG", amg_precision="AMG_PREC_FP32"),
                                dict(precond="PRECOND_FSAI"), dict(precond="PRECOND_CHEBYSHEV"),
                                dict(precond="PRECOND_BLOCKJACOBI"), dict(nvirt=2), dict(precision="PREC_MIXED"),
                                dict(krylov="KRYLOV_BICGSTAB"), dict(krylov="KRYLOV_GMRES"),
                                dict(krylov="KRYLOV_RICHARDSON", precond="PRECOND_AMG")],
                         ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_refusals(hip, kw, matrix_path):
    import torch
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    s = hip.Solver(A, hip.default_opts(**{k: getattr(_lib, v) if isinstance(v, str) else v for k, v in kw.items()}))
    lib = _lib.load()
    d_B = torch.rand(2, n, dtype=torch.float64, device="cuda:0")
    d_X = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_block_precond_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
    assert lib.lsb_hip_solver_solve_block_precond_dev(s._h, 1, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
    Bh, Xh = np.ones((n, 2), order="F"), np.full((n, 2), 7.0, order="F")
    assert lib.lsb_hip_solver_solve_block_precond(s._h, 2, Bh.ctypes.data, n, Xh.ctypes.data, n, res) == 2
    assert bool((d_X == 7.0).all()) and bool((Xh == 7.0).all())
    assert s.block_precond_iteration_bytes(2) == 0
    s.destroy()


@pytest.mark.gpu
def test_bad_arguments_and_solve_block_itself_still_refuses(hip, matrix_path):
    import torch
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    n = A.nrows
    lib = _lib.load()
    d_B = torch.rand(9, n, dtype=torch.float64, device="cuda:0")
    d_X = torch.full((9, n), 7.0, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 9)()
    for cfg in ("fsai", "amg"):
        s = hip.Solver(A, hip.default_opts(tol=1e-10, **CONFIGS[cfg]))
        f = lib.lsb_hip_solver_solve_block_precond_dev
        assert f(s._h, 9, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
        assert f(s._h, 0, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
        assert f(s._h, 2, d_B.data_ptr(), n - 1, d_X.data_ptr(), n, res) == 2
        assert f(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n - 1, res) == 2
        assert f(s._h, 2, None, n, d_X.data_ptr(), n, res) == 2
        assert f(s._h, 2, d_B.data_ptr(), n, None, n, res) == 2
        assert f(None, 2, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
        assert s.block_precond_iteration_bytes(9) == 0 and s.block_precond_iteration_bytes(0) == 0
        # the diagonal entry point keeps refusing what it refused
        assert lib.lsb_hip_solver_solve_block_dev(s._h, 2, d_B.data_ptr(), n, d_X.data_ptr(), n, res) == 2
        assert s.block_iteration_bytes(2) == 0
        s.destroy()
    assert bool((d_X == 7.0).all())


@pytest.mark.gpu
def test_block_precond_iteration_bytes(hip, matrix_path):
    A = hip.lsbench_matrix_read(matrix_path("xn3b_A_18"))
    s = hip.Solver(A, hip.default_opts(**CONFIGS["fsai"]))
    n, nnz = s.n_local, s.nnz_local
    g, gt = s.fsai_nnz
    assert s.padded == 0
    # S, G and G^T once; per column the SpMM 2 passes, pass A 6, the product with G 2, with G^T and the Gram sums 3, pass B 5
    for nrhs, kp in ((2, 2), (3, 4), (4, 4), (8, 8)):
        assert s.block_precond_iteration_bytes(nrhs) == 12 * (nnz + g + gt) + 12 * (n + 1) + 8 * n * (2 + 6 + 2 + 3 + 5) * kp
    s.destroy()
    s = hip.Solver(A, hip.default_opts(**CONFIGS["amg"]))
    assert s.block_precond_iteration_bytes(2) == 0
    s.destroy()
