"""The direct solver on blocks of right-hand sides (lsb_hip_solver_solve_direct_multi[_dev], _direct_apply_multi_dev,
_direct_multi_round_bytes; hip_direct_m.hip, hip_direct_m_drv.c): W streamed once per product for a block of columns.

The contract makes the tests exact: a column solved in a block is, bit for bit, that column solved alone by solve_dev
(or applied alone by precond_dev) on the same solver -- x, iters, status, relres, true_relres, spmvs.

CPU: the surface.  GPU: one application at every width on every path of k_dirt_rows_m (every window staged; the
gathered path at width 8 only; the gathered path at every width); the solves; columns that stop on their own; the
layout of the caller's blocks; the refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from test_amg import as_matrix
from test_amg_f32 import _relerr
from test_direct import (EPS, FOREST, ONE, POWERLAW, TJ7A, TRI, WIDE, XN3B, _factor, apply_np, op)
from test_mrhs import columns, eleven

CONVERGED, BREAKDOWN, MAXIT_ST = 1, 2, 3
FOUR = ("lsb_hip_solver_solve_direct_multi_dev", "lsb_hip_solver_solve_direct_multi",
        "lsb_hip_solver_direct_apply_multi_dev", "lsb_hip_solver_direct_multi_round_bytes")


def _cap():
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_direct_drv.c")) as f:
        return int(re.search(r"#define DIR_LDS_CAP (\d+)u", f.read()).group(1))


# ------------------------------------------------------------------------------------ without a GPU
def test_surface():
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    for name in FOUR:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name) and name in exported, name
    assert not [s for s in exported if s.startswith("lsb_k_dir")]  # the launchers stay inside
    for m in ("solve_direct_multi_dev", "solve_direct_multi", "direct_apply_multi_dev", "direct_multi_round_bytes"):
        assert callable(getattr(la.Solver, m)), m
    assert "Warm starts on blocks are not built" in re.sub(r"\s+", " ", header)
    # struct lsb_hip_opts gained nothing
    assert [f[0] for f in _lib.Opts._fields_][-1] == "amg_cheb_ratio" and list(_lib.Opts._TAIL) == ["fsai_blocks"]
    # a null solver: 2 once the backend is up, 1 before (whichever this process is in), 0 bytes either way
    up = int(lib.hip.lsb_hip_is_initialized())
    res = _lib.Result()
    want = 2 if up else 1
    assert lib.lsb_hip_solver_solve_direct_multi_dev(None, 1, None, 0, None, 0, C.byref(res)) == want
    assert lib.lsb_hip_solver_solve_direct_multi(None, 1, None, 0, None, 0, C.byref(res)) == want
    assert lib.lsb_hip_solver_direct_apply_multi_dev(None, 1, None, 0, None, 0) == want
    assert lib.lsb_hip_solver_direct_multi_round_bytes(None, 2) == 0


# ------------------------------------------------------------------------------------ on the GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _full(shape, v):
    import torch
    return torch.full(shape, v, dtype=torch.float64, device="cuda:0")


def _solver(hip, name, matrix_path, **kw):
    """a direct solver on the operator the numpy side uses, as read"""
    kw.setdefault("op_mode", hip.OP_RAW)
    kw.setdefault("krylov", hip.KRYLOV_DIRECT)
    return hip.Solver(as_matrix(op(name, matrix_path)), hip.default_opts(**kw))


def _fields(r):
    return (r.status, r.iters, r.relres, r.true_relres, r.spmvs)


def _alone(s, B):
    """every column of B (n, k) solved alone by solve_dev on s: [(x, fields)]"""
    out = []
    for c in range(B.shape[1]):
        d_x = _full((B.shape[0],), float("nan"))
        res = s.solve_dev(_dev(B[:, c]), d_x)
        out.append((d_x.cpu().numpy(), _fields(res)))
    return out


def _block(s, B):
    """B (n, k) solved as blocks by solve_direct_multi_dev: (X (n, k), [fields])"""
    d_X = _full((B.shape[1], B.shape[0]), float("nan"))
    res = s.solve_direct_multi_dev(_dev(B.T), d_X)
    return d_X.cpu().numpy().T, [_fields(r) for r in res]


def _same(got, want):
    """fields equal, NaN == NaN"""
    return all((a == b) or (isinstance(a, float) and np.isnan(a) and np.isnan(b)) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [ONE, TRI, FOREST, POWERLAW, XN3B, WIDE])
def test_one_application(hip, name, matrix_path):
    """direct_apply_multi_dev on 2, 3 and 8 columns against precond_dev on each column alone: the same bytes.  ONE and
    TRI stage every window at every width; XN3B's root row is gathered at width 8 only; WIDE's at every width."""
    S, perm, W, Wm = _factor(name, matrix_path)
    n = S.shape[0]
    cap = _cap()
    first = W["first"].astype(np.int64)
    widest = int((np.arange(n) - first + 1).max())  # the longest row: some window is at least this wide
    if name in (ONE, TRI):
        assert n <= cap // 8  # every window staged at every width
    if name == XN3B:
        assert n > cap // 8 and int(first[n - 1]) == 0 and n <= cap // 2  # gathered at width 8, staged at width 2
    if name == WIDE:
        assert int(first[n - 1]) == 0 and widest > cap // 2  # gathered at every width
    i = np.arange(n, dtype=np.float64)
    R = np.stack([np.sin(i + 0.37 * c) + 0.5 for c in range(8)], axis=1)
    R[:, 1] = 0.0  # one zero column
    s = _solver(hip, name, matrix_path)
    alone = []
    for c in range(8):
        z = _full((n,), float("nan"))
        s.precond_dev(_dev(R[:, c]), z)
        alone.append(z.cpu().numpy())
    assert not alone[1].any()
    for nrhs in (2, 3, 8):
        out = []
        for _ in range(2):
            d_Z = _full((nrhs, n), float("nan"))
            s.direct_apply_multi_dev(_dev(R[:, :nrhs].T), d_Z)
            out.append(d_Z.cpu().numpy())
        assert out[0].tobytes() == out[1].tobytes()  # run twice: the same bytes
        for c in range(nrhs):
            assert np.isfinite(out[0][c]).all()
            assert out[0][c].tobytes() == alone[c].tobytes(), (name, nrhs, c)
        if name == XN3B and nrhs == 8:  # ... and against numpy, by test_direct.test_one_application's bound
            for c in (0, 7):
                za, zb = apply_np(W, Wm, R[:, c]), apply_np(W, Wm, R[:, c], flip=True)
                e_np, e_gpu = _relerr(zb, za), _relerr(out[0][c], za)
                bound = 4.0 * max(e_np, EPS)
                print(name, "column", c, "device against numpy", e_gpu, "numpy between two orders", e_np, "bound",
                      bound)
                assert bound <= 1e-13 and e_gpu <= bound
    s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [XN3B, TJ7A])
def test_solves(hip, name, matrix_path):
    """Every column of a block against solve_dev on that column alone on the same solver: the bytes of x and
    (status, iters, relres, true_relres, spmvs).  XN3B: 5 columns, a zero column among them, padded to 8; TJ7A: 11
    columns, a block of 8 and one of 3."""
    S = op(name, matrix_path)
    n = S.shape[0]
    B = columns(S) if name == XN3B else eleven(S)
    k = B.shape[1]
    settings = [dict(tol=1e-12, maxit=10, use_graph=1), dict(tol=1e-12, maxit=10, use_graph=0),
                dict(tol=1e-10, maxit=10), dict(tol=0.0, maxit=1), dict(tol=0.0, maxit=3)]
    for kw in settings:
        s = _solver(hip, name, matrix_path, **kw)
        assert s.direct_multi_round_bytes(k) == s.direct_info[2] + 32 * n * 7
        assert s.direct_multi_round_bytes(1) == s.direct_info[2]
        want = _alone(s, B)
        X, got = _block(s, B)
        X2, got2 = _block(s, B)  # (the hinted block)
        Xh, resh = s.solve_direct_multi(B)  # host buffers
        s.destroy()
        print(name, kw, "fields of column 0:", got[0])
        for c in range(k):
            assert _same(got[c], want[c][1]) and _same(got2[c], want[c][1]), (kw, c, got[c], want[c][1])
            assert _same(_fields(resh[c]), want[c][1]), (kw, c)
            for Y in (X, X2, np.asarray(Xh)):
                assert np.ascontiguousarray(Y[:, c]).tobytes() == want[c][0].tobytes(), (kw, c)
        if kw["tol"] == 0.0:
            assert all(g == (MAXIT_ST, kw["maxit"], -1.0, -1.0, kw["maxit"] - 1) for g in got)
        else:
            assert all(g[0] == CONVERGED and g[1] <= 2 and g[2] <= kw["tol"] for g in got)
        if name == XN3B and kw["tol"] == 1e-12:  # test_direct.test_cpu_precondition: numpy with this W gets there
            assert not X[:, 1].any() and got[1][2] == 0.0
            for c in range(k):
                if B[:, c].any():
                    true = np.linalg.norm(B[:, c] - S @ X[:, c]) / np.linalg.norm(B[:, c])
                    print("   column", c, "rounds", got[c][1], "relres", got[c][2], "on the CPU", true)
                    assert true <= 1e-12 * (1 + 1e-3)


@pytest.mark.gpu
def test_columns_stop_on_their_own(hip, matrix_path):
    """tol 1e-30, maxit 3 on a block of four: the zero column converges after round 1, the column with a NaN breaks
    down after round 1, the other two run all three rounds with the bits of the same column alone -- the freezing, and
    a NaN that stays in its column."""
    S = op(TJ7A, matrix_path)
    n = S.shape[0]
    bad = np.arange(1.0, n + 1.0)
    bad[n // 2] = float("nan")
    B = np.stack([np.arange(1.0, n + 1.0), np.zeros(n), bad, S @ np.ones(n)], axis=1)
    s = _solver(hip, TJ7A, matrix_path, tol=1e-30, maxit=3)
    want = _alone(s, B)
    X, got = _block(s, B)
    print("fields:", got)
    assert (got[1][0], got[1][1], got[1][2]) == (CONVERGED, 1, 0.0) and not X[:, 1].any()
    assert (got[2][0], got[2][1]) == (BREAKDOWN, 1)
    for c in (0, 3):
        assert (got[c][0], got[c][1]) == (MAXIT_ST, 3) and np.isfinite(X[:, c]).all()
        assert X[:, c].tobytes() == want[c][0].tobytes()
    for c in range(4):
        assert _same(got[c], want[c][1]), (c, got[c], want[c][1])
    # ... and the solver solves a clean block as before
    Bc = B[:, [0, 3]]
    X2, got2 = _block(s, Bc)
    s.destroy()
    for j, c in enumerate((0, 3)):
        assert X2[:, j].tobytes() == want[c][0].tobytes() and _same(got2[j], want[c][1])
    s = _solver(hip, TJ7A, matrix_path, tol=1e-12, maxit=0)
    X, got = _block(s, Bc)
    s.destroy()
    assert not X.any() and all((g[0], g[1]) == (MAXIT_ST, 0) for g in got)


@pytest.mark.gpu
def test_layout(hip, matrix_path):
    """ld = n + 3 and X starting 8 bytes past a 16-byte boundary: the slack stays the caller's; one column is the
    forwarded path."""
    import torch
    S = op(XN3B, matrix_path)
    n = S.shape[0]
    B = columns(S)[:, [0, 2, 4]]
    s = _solver(hip, XN3B, matrix_path, tol=1e-12, maxit=10)
    want = _alone(s, B)
    ld = n + 3
    d_B = _full((3, ld), float("nan"))
    d_B[:, :n] = _dev(B.T)
    buf = _full((3 * ld + 2,), 7.0)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    assert (buf.data_ptr() + 8 * off) % 16 == 8
    d_X = buf[off:off + 3 * ld].view(3, ld)
    res = s.solve_direct_multi_dev(d_B, d_X)
    d_Z = buf.clone()[off:off + 3 * ld].view(3, ld)
    d_Z[:] = 7.0
    s.direct_apply_multi_dev(d_B, d_Z)
    around = buf.cpu().numpy()
    X = around[off:off + 3 * ld].reshape(3, ld)
    assert (around[:off] == 7.0).all() and (around[off + 3 * ld:] == 7.0).all() and (X[:, n:] == 7.0).all()
    assert bool((d_Z[:, n:] == 7.0).all()) and bool(torch.isfinite(d_Z[:, :n]).all())
    assert bool(torch.isnan(d_B[:, n:]).all())
    for c in range(3):
        assert X[c, :n].tobytes() == want[c][0].tobytes() and _same(_fields(res[c]), want[c][1])
    # nrhs = 1: forwarded to solve_dev / precond_dev
    d_x1 = _full((1, n), float("nan"))
    res1 = s.solve_direct_multi_dev(_dev(B[:, :1].T), d_x1)
    assert d_x1.cpu().numpy()[0].tobytes() == want[0][0].tobytes() and _same(_fields(res1[0]), want[0][1])
    z1, za = _full((1, n), float("nan")), _full((n,), float("nan"))
    s.direct_apply_multi_dev(_dev(B[:, :1].T), z1)
    s.precond_dev(_dev(B[:, 0]), za)
    assert z1.cpu().numpy()[0].tobytes() == za.cpu().numpy().tobytes()
    s.destroy()


@pytest.mark.gpu
def test_refusals(hip, matrix_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    S = op(ONE, matrix_path)
    n = S.shape[0]
    B = np.asfortranarray(np.tile(np.arange(1.0, n + 1.0)[:, None], (1, 2)))
    d_B = _dev(B.T)
    d_X = _full((2, n), 7.0)
    res = (_lib.Result * 2)()
    j = hip.Solver(as_matrix(S), hip.default_opts(op_mode=hip.OP_RAW))  # Jacobi-PCG: not a direct solver
    X = np.full((n, 2), 7.0, order="F")
    assert lib.lsb_hip_solver_solve_direct_multi_dev(j._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_direct_apply_multi_dev(j._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_solve_direct_multi(j._h, 2, B.ctypes.data, n, X.ctypes.data, n, res) == 2
    assert j.direct_multi_round_bytes(2) == 0
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (X == 7.0).all()
    j.destroy()
    s = _solver(hip, ONE, matrix_path)
    assert s.direct_multi_round_bytes(0) == 0
    for fn in (lib.lsb_hip_solver_solve_direct_multi_dev, lib.lsb_hip_solver_direct_apply_multi_dev):
        extra = (res,) if fn is lib.lsb_hip_solver_solve_direct_multi_dev else ()
        assert fn(s._h, 0, _ptr(d_B), n, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n - 1, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n, _ptr(d_X), n - 1, *extra) == 2
        assert fn(s._h, 2, None, n, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n, None, n, *extra) == 2
    assert lib.lsb_hip_solver_solve_direct_multi(s._h, 0, B.ctypes.data, n, X.ctypes.data, n, res) == 2
    assert lib.lsb_hip_solver_solve_direct_multi(s._h, 2, B.ctypes.data, n - 1, X.ctypes.data, n, res) == 2
    assert lib.lsb_hip_solver_solve_direct_multi(s._h, 2, None, n, X.ctypes.data, n, res) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (X == 7.0).all()
    assert lib.lsb_hip_solver_solve_direct_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 0  # ... and serves
    assert res[0].status == CONVERGED and bool(torch.isfinite(d_X).all())
    s.destroy()
