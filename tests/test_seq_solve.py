"""Successive right-hand sides on the GPU: lsb_hip_solver_seq_begin / solve_seq[_dev] / seq_info / seq_basis_dev
(hip_seq_drv.c, hip_seq.hip) against the numpy model of seq_family.py, the cold solves of the same solver, and the
rules of include/lsbench_hip.h.  Except where named otherwise: xn3b_A_18 and lap2d:nx=60,ny=50 under Jacobi-PCG at tol
1e-10, the drifting family of right-hand sides."""
import ctypes as C
import functools

import numpy as np
import pytest

import lsbench_amd as la
from lsbench_amd import _lib
from seq_family import CONVERGED, rhs_3d, rhs_drift, run_model
from test_mrhs import _lap2d, oracle_operator

OPS = ("xn3b_A_18", "lap2d")
TOL = 1e-10


def _dev(v):
    import torch
    return torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0")


def _matrix(name, matrix_path):
    """(Matrix, option keywords, the operator as scipy)"""
    if name == "lap2d":
        return la.lsbench_matrix_synth("lap2d:nx=60,ny=50"), dict(op_mode=la.OP_RAW), _lap2d(60, 50)
    path = matrix_path(name)
    return la.lsbench_matrix_read(path), {}, oracle_operator(path)[1].tocsr()


def _solver(name, matrix_path, **kw):
    A, base, S = _matrix(name, matrix_path)
    base = dict(base, tol=TOL)
    base.update({k: getattr(la, v) if isinstance(v, str) else v for k, v in kw.items()})
    return la.Solver(A, la.default_opts(**base)), S


def _seq(s, b):
    """one solve of the sequence -> (x, result, starting residual or None after a cold solve)"""
    import torch
    d_x = torch.full((len(b),), 7.0, dtype=torch.float64, device="cuda:0")
    res = s.solve_seq_dev(_dev(b), d_x)
    out = (C.c_double * 1)()
    rc = _lib.load().lsb_hip_solver_start_relres(s._h, 1, out)
    return d_x.cpu().numpy(), res, (out[0] if rc == 0 else None)


def _cold(s, b):
    import torch
    d_x = torch.full((len(b),), 7.0, dtype=torch.float64, device="cuda:0")
    res = s.solve_dev(_dev(b), d_x)
    return d_x.cpu().numpy(), res


def _sequence(s, n, family, steps):
    return [_seq(s, family(n, t)) for t in range(steps)]


@functools.lru_cache(maxsize=None)
def _model(name, path, depth, family, steps):
    S = oracle_operator(path)[1].tocsr() if path else _lap2d(60, 50)
    iters, start, _ = run_model(S, depth, TOL, family, steps)
    return iters, start


def _model_of(name, matrix_path, depth, family, steps):
    return _model(name, matrix_path(name) if name != "lap2d" else None, depth, family, steps)


@functools.lru_cache(maxsize=None)
def _drift(name, path_of):
    """The sequence of tests 3, 4 and 8, run once per operator: nine drifting solves at depth 8 under opts.verify,
    the basis read back, the nine cold solves of the same solver, and the same sequence again behind seq_begin."""
    import torch
    s, S = _solver(name, path_of, verify=1)
    n = S.shape[0]
    s.seq_begin(8)
    first = _sequence(s, n, rhs_drift, 8)
    info = s.seq_info  # the basis at its fullest: the ninth solve restarts it
    X, SX = [], []
    for k in range(info[1]):
        d_a, d_b = torch.zeros(n, dtype=torch.float64, device="cuda:0"), torch.zeros(n, dtype=torch.float64, device="cuda:0")
        s.seq_basis_dev(k, d_a, d_b)
        X.append(d_a.cpu().numpy()), SX.append(d_b.cpu().numpy())
    first.append(_seq(s, rhs_drift(n, 8)))
    assert s.seq_info[:3] == (8, 1, 1)
    cold = [_cold(s, rhs_drift(n, t)) for t in range(9)]
    s.seq_begin(8)
    assert s.seq_info[1:3] == (0, 0)
    again = _sequence(s, n, rhs_drift, 9)
    s.destroy()
    return dict(S=S, first=first, info=info, X=np.array(X), SX=np.array(SX), cold=cold, again=again)


# 1. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seq_begin_exists_and_answers_0(hip, matrix_path):
    """without the feature nothing in this file passes"""
    lib = _lib.load()
    assert hasattr(lib.hip, "lsb_hip_solver_seq_begin")
    s, _ = _solver("xn3b_A_18", matrix_path)
    assert lib.lsb_hip_solver_seq_begin(s._h, 8) == 0
    depth, held, restarts, nbytes = s.seq_info
    assert (depth, held, restarts) == (8, 0, 0) and nbytes >= 2 * 8 * 8 * s.n_local
    s.destroy()


# 2. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_the_first_solve_of_a_sequence_is_the_cold_solve(hip, name, matrix_path):
    s, S = _solver(name, matrix_path)
    b = rhs_drift(S.shape[0], 0)
    xc, rc = _cold(s, b)
    s.seq_begin(8)
    xs, rs, start = _seq(s, b)
    info = s.seq_info
    s.destroy()
    assert xs.tobytes() == xc.tobytes()
    assert (rs.iters, rs.status, rs.relres, rs.spmvs) == (rc.iters, rc.status, rc.relres, rc.spmvs)
    assert rs.status == CONVERGED and start is None and info[1] == 1


# 3. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_the_drifting_family_at_depth_8(hip, name, matrix_path):
    """Nine solves under opts.verify against the model.  Seen on an MI355X, device minus model per solve: xn3b_A_18
    +1, 0, 0, 0, 0, +1, 0, 0, 0 (1354 against 1352; nine cold solves 2126: 0.64), the grid 0 nine times (1310 of
    2014: 0.65); the starting residuals agree with the model's to the digits printed, 1.08e-8 against 1.07e-8 on the
    last solve of xn3b_A_18."""
    run = _drift(name, matrix_path)
    model_iters, model_start = _model_of(name, matrix_path, 8, rhs_drift, 9)
    iters = [r.iters for _, r, _ in run["first"]]
    cold = [r.iters for _, r in run["cold"]]
    starts = [st for _, _, st in run["first"]]
    print(name, "device", iters, sum(iters), "model", model_iters, sum(model_iters), "cold", cold, sum(cold))
    print(name, "differences", [a - b for a, b in zip(iters, model_iters)])
    print(name, "start", ["%.2e" % s for s in starts[1:]], "model", ["%.2e" % s for s in model_start[1:]])
    for _, r, _ in run["first"]:
        assert r.status == CONVERGED and 0.0 <= r.true_relres <= TOL
    assert all(r.status == CONVERGED for _, r in run["cold"])
    assert sum(iters) <= 0.75 * sum(cold)
    assert starts[0] is None
    for t in range(1, 9):
        assert starts[t] <= 3.0 * model_start[t], t
        assert abs(iters[t] - model_iters[t]) <= 2 + 0.02 * model_iters[t], t
    assert abs(iters[0] - model_iters[0]) <= 2 + 0.02 * model_iters[0]


# 4. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_the_basis_is_s_orthonormal_and_its_products_are_products(hip, name, matrix_path):
    """The eight pairs held after the eighth solve.  Seen on an MI355X: max |X^T S X - I| 5.7e-16 (xn3b_A_18) and
    4.4e-16 (the grid); ||S x_k - (S x)_k|| / ||(S x)_k|| between 3.0e-15 and 2.6e-14."""
    run = _drift(name, matrix_path)
    X, SX, S = run["X"], run["SX"], run["S"]
    assert run["info"][:3] == (8, 8, 0) and X.shape[0] == 8
    gram = np.abs(X @ SX.T - np.eye(8)).max()
    rel = [float(np.linalg.norm(S @ X[k] - SX[k]) / np.linalg.norm(SX[k])) for k in range(8)]
    print(name, "max |X^T S X - I|", gram, "||S x_k - (S x)_k|| / ||(S x)_k||", ["%.1e" % r for r in rel])
    assert gram <= 1e-13
    assert max(rel) <= 1e-12


# 5. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_the_three_dimensional_family_at_depth_4(hip, name, matrix_path):
    s, S = _solver(name, matrix_path)
    n = S.shape[0]
    s.seq_begin(4)
    iters, infos = [], []
    for t in range(5):
        _, r, _ = _seq(s, rhs_3d(n, t))
        assert r.status == CONVERGED
        iters.append(r.iters), infos.append(s.seq_info)
    s.destroy()
    print(name, iters, "model", _model_of(name, matrix_path, 4, rhs_3d, 5)[0])
    assert iters[3] <= 0.1 * iters[0] and iters[4] <= 0.1 * iters[0]
    assert [i[1] for i in infos] == [1, 2, 3, 4, 1]
    assert [i[2] for i in infos] == [0, 0, 0, 0, 1]


# 6. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_the_same_b_twice(hip, name, matrix_path):
    tol = 1e-8
    s, S = _solver(name, matrix_path, tol=tol)
    b = rhs_drift(S.shape[0], 0)
    s.seq_begin(4)
    _, r1, _ = _seq(s, b)
    held = s.seq_info[1]
    x2, r2, start = _seq(s, b)
    held2 = s.seq_info[1]
    s.destroy()
    print(name, "first", r1.iters, "second", r2.iters, "start / tol", start / tol)
    assert r1.status == r2.status == CONVERGED and held == 1
    assert start <= 2.0 * tol and r2.iters <= 3
    if r2.iters == 0:
        assert held2 == held
    assert np.linalg.norm(b - S @ x2) <= 4.0 * tol * np.linalg.norm(b)


# 7. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_uncorrelated_right_hand_sides_lose_nothing(hip, name, matrix_path):
    s, S = _solver(name, matrix_path)
    n = S.shape[0]
    bs = [np.random.default_rng(t).standard_normal(n) for t in range(6)]
    cold = [_cold(s, b)[1] for b in bs]
    s.seq_begin(4)
    seq = [_seq(s, b)[1] for b in bs]
    s.destroy()
    print(name, "cold", [r.iters for r in cold], "sequence", [r.iters for r in seq])
    for rc, rs in zip(cold, seq):
        assert rc.status == rs.status == CONVERGED
        assert abs(rs.iters - rc.iters) <= 0.05 * rc.iters


# 8. -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_a_sequence_repeats_bit_for_bit(hip, name, matrix_path):
    run = _drift(name, matrix_path)
    for (x1, r1, s1), (x2, r2, s2) in zip(run["first"], run["again"]):
        assert x1.tobytes() == x2.tobytes() and r1.iters == r2.iters and r1.status == r2.status and s1 == s2


# 9. -------------------------------------------------------------------------------------------------
AROUND = {
    "reorder": dict(reorder=1),
    "fsai": dict(precond="PRECOND_FSAI"),
    "amg-l1": dict(precond="PRECOND_AMG", amg_smoother="AMG_SMOOTH_L1JACOBI"),
    "amg-cheb": dict(precond="PRECOND_AMG", amg_smoother="AMG_SMOOTH_CHEB"),
    "amg-mcgs": dict(precond="PRECOND_AMG", amg_smoother="AMG_SMOOTH_MCGS"),
    "pcg1": dict(krylov="KRYLOV_PCG1"),
    "mixed": dict(precision="PREC_MIXED"),
    "nograph": dict(use_graph=0),
}


def _five(s, n):
    s.seq_begin(4)
    out = _sequence(s, n, rhs_drift, 5)
    return out, s.seq_info


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(AROUND))
@pytest.mark.parametrize("name", OPS)
def test_around_the_solve_layer(hip, name, what, matrix_path):
    s, S = _solver(name, matrix_path, **AROUND[what])
    out, info = _five(s, S.shape[0])
    s.destroy()
    iters = [r.iters for _, r, _ in out]
    print(name, what, iters, info)
    assert all(r.status == CONVERGED for _, r, _ in out)
    assert iters[4] < iters[0]
    for t, (x, _, _) in enumerate(out):
        b = rhs_drift(S.shape[0], t)
        assert np.linalg.norm(b - S @ x) <= 10.0 * TOL * np.linalg.norm(b)


@pytest.mark.gpu
def test_on_a_line_padded_grid(hip, monkeypatch):
    A = hip.lsbench_matrix_synth("lap2d:nx=2050,ny=12")
    n = A.nrows
    out = {}
    for pad in ("0", "1"):
        monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", pad)
        s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, tol=TOL))  # the grid itself, as everywhere in here
        assert bool(s.padded) == (pad == "1") and s.n_local == n
        out[pad], info = _five(s, n)
        s.destroy()
        assert info[:3] == (4, 1, 1)  # the fifth solve found the basis full
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    iters = [r.iters for _, r, _ in out["1"]]
    print("padded", iters, "unpadded", [r.iters for _, r, _ in out["0"]])
    assert all(r.status == CONVERGED for _, r, _ in out["0"] + out["1"])
    assert iters[4] < iters[0]
    for (xp, _, _), (xu, _, _) in zip(out["1"], out["0"]):
        assert np.linalg.norm(xp - xu) <= 1e-8 * np.linalg.norm(xu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_under_the_direct_solver(hip, name, matrix_path):
    s, S = _solver(name, matrix_path, krylov="KRYLOV_DIRECT")
    n = S.shape[0]
    s.seq_begin(4)
    held = 0
    for t in range(5):
        _, r, _ = _seq(s, rhs_drift(n, t))
        now = s.seq_info[1]
        print(name, t, r.iters, r.relres, now)
        assert r.status == CONVERGED
        assert now in (held, held + 1) or (held == 4 and now == 1)
        held = now
    s.destroy()


# 10. ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS)
def test_other_solves_in_between_change_nothing(hip, name, matrix_path):
    import torch
    outs = []
    for between in (False, True):
        s, S = _solver(name, matrix_path)
        n = S.shape[0]
        s.seq_begin(4)
        _seq(s, rhs_drift(n, 0)), _seq(s, rhs_drift(n, 1))
        if between:
            _cold(s, rhs_3d(n, 5))
            d_B = torch.stack([_dev(rhs_3d(n, 1)), _dev(rhs_drift(n, 7))])
            d_X = torch.zeros_like(d_B)
            assert all(r.status == CONVERGED for r in s.solve_multi_dev(d_B, d_X))
        info = s.seq_info
        x, r, start = _seq(s, rhs_drift(n, 2))
        outs.append((info, x, r.iters, r.status, start, s.seq_info))
        s.destroy()
    a, b = outs
    assert a[0] == b[0] and a[5] == b[5] and a[0][1] == 2
    assert a[1].tobytes() == b[1].tobytes() and a[2:5] == b[2:5]


# 11. ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_arguments(hip, matrix_path):
    import torch
    lib = _lib.load()
    res = _lib.Result()
    s, S = _solver("xn3b_A_18", matrix_path)
    n = S.shape[0]
    d_b, d_x = _dev(rhs_drift(n, 0)), torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0")

    def untouched():
        return bool((d_x == 7.0).all())
    assert s.seq_info == (0, 0, 0, 0)  # seq_begin was never called
    assert lib.lsb_hip_solver_solve_seq_dev(s._h, d_b.data_ptr(), d_x.data_ptr(), C.byref(res)) == 2 and untouched()
    x_host = np.full(n, 7.0)
    assert lib.lsb_hip_solver_solve_seq(s._h, rhs_drift(n, 0).ctypes.data, x_host.ctypes.data, C.byref(res)) == 2
    assert (x_host == 7.0).all()
    assert lib.lsb_hip_solver_seq_begin(s._h, 17) == 2 and s.seq_info == (0, 0, 0, 0)
    assert lib.lsb_hip_solver_seq_begin(s._h, 4) == 0
    assert lib.lsb_hip_solver_solve_seq_dev(s._h, None, d_x.data_ptr(), C.byref(res)) == 2 and untouched()
    assert lib.lsb_hip_solver_solve_seq_dev(s._h, d_b.data_ptr(), None, C.byref(res)) == 2
    assert lib.lsb_hip_solver_solve_seq(s._h, None, x_host.ctypes.data, C.byref(res)) == 2 and (x_host == 7.0).all()
    assert lib.lsb_hip_solver_seq_basis_dev(s._h, 0, d_x.data_ptr(), d_x.data_ptr()) == 2 and untouched()  # k = held
    assert lib.lsb_hip_solver_seq_begin(s._h, 17) == 2 and s.seq_info[0] == 4  # a refusal leaves what is there
    s.solve_seq_dev(d_b, torch.zeros(n, dtype=torch.float64, device="cuda:0"))
    assert s.seq_info[1] == 1
    assert lib.lsb_hip_solver_seq_basis_dev(s._h, 1, d_x.data_ptr(), d_x.data_ptr()) == 2 and untouched()
    # the host entry point solves what the device one does
    x_host, r_host = s.solve_seq(rhs_drift(n, 1))
    assert r_host.status == CONVERGED and s.seq_info[1] == 2
    b1 = rhs_drift(n, 1)
    assert np.linalg.norm(b1 - S @ x_host) <= 10.0 * TOL * np.linalg.norm(b1)
    # another depth re-allocates and empties; 0 gives everything back
    nbytes = s.seq_info[3]
    assert lib.lsb_hip_solver_seq_begin(s._h, 8) == 0
    assert s.seq_info[:3] == (8, 0, 0) and s.seq_info[3] > nbytes
    assert lib.lsb_hip_solver_seq_begin(s._h, 0) == 0 and s.seq_info == (0, 0, 0, 0)
    assert lib.lsb_hip_solver_solve_seq_dev(s._h, d_b.data_ptr(), d_x.data_ptr(), C.byref(res)) == 2 and untouched()
    s.destroy()
    # solvers the projection does not serve
    for kw in (dict(nvirt=2), dict(krylov="KRYLOV_GMRES", restart=32), dict(krylov="KRYLOV_BICGSTAB")):
        s, _ = _solver("xn3b_A_18", matrix_path, **kw)
        assert lib.lsb_hip_solver_seq_begin(s._h, 4) == 2 and s.seq_info == (0, 0, 0, 0)
        assert lib.lsb_hip_solver_solve_seq_dev(s._h, d_b.data_ptr(), d_x.data_ptr(), C.byref(res)) == 2 and untouched()
        s.destroy()
