"""The direct solver on a tiered factor on blocks of right-hand sides (lsb_hip_solver_solve_direct_tier_multi[_dev],
_direct_tier_apply_multi_dev, _direct_tier_multi_round_bytes; hip_direct_tm.hip, hip_direct_drv.c,
hip_direct_m_drv.c): the 4 m - 2 launches of the tiers on 2, 4 or 8 columns at once, the factor and its coupling loaded
once per product for all of them.

The contract makes the tests exact: a column solved in a block is, bit for bit, that column solved alone by solve_dev
(or applied alone by precond_dev) on the same tiered solver -- x, iters, status, relres, true_relres, spmvs.

What the shapes give (checked on the CPU from the factor):

    PATH3 / 2            tiers of 2 and 1 rows, one coupling entry
    DIAG, SINGLE / 2     one tier, no coupling
    G2D / 2, 3, 4        really 2 / 3 / 4 tiers, rows of C of 0, 1 and up to some tens of entries, rows of Y that some
                         tier's C^T does not reach
    XN3B / 2             the longest row of W has 2505 entries: its window is staged at width 2 and gathered at 4 and 8
    XN3B / 3             rows of C of more than 256 entries: 64 lanes per row

CPU: the surface.  GPU: one application at every width with the windows staged as dealt and with at most 16 doubles
staged; the solves; columns that stop on their own; the layout of the caller's blocks; forwarding and refusals."""
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
from test_direct_tiers import DIAG, G2D, G3D, PATH3, SINGLE, TJ7A, XN3B, Blocks, _factor, _solver, operator
from test_mrhs import columns, eleven

EPS = 2.0 ** -52
CONVERGED, BREAKDOWN, MAXIT_ST = 1, 2, 3
FOUR = ("lsb_hip_solver_solve_direct_tier_multi_dev", "lsb_hip_solver_solve_direct_tier_multi",
        "lsb_hip_solver_direct_tier_apply_multi_dev", "lsb_hip_solver_direct_tier_multi_round_bytes")
APPLY = [(PATH3, 2), (DIAG, 2), (SINGLE, 2), (G2D, 2), (G2D, 3), (G2D, 4), (G3D, 3), (XN3B, 2), (XN3B, 3)]


def _cap():
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_direct_drv.c")) as f:
        return int(re.search(r"#define DIR_LDS_CAP (\d+)u", f.read()).group(1))


# ------------------------------------------------------------------------------------ without a GPU
def test_surface():
    """Fails without the feature: the four entry points and the four methods are what it adds."""
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    for name in FOUR:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name) and name in exported, name
    assert not [s for s in exported if s.startswith("lsb_k_dirt")]  # the launchers stay inside
    for m in ("solve_direct_tier_multi_dev", "solve_direct_tier_multi", "direct_tier_apply_multi_dev",
              "direct_tier_multi_round_bytes"):
        assert callable(getattr(la.Solver, m)), m
    # a null solver: 2 once the backend is up, 1 before (whichever this process is in), 0 bytes either way
    up = int(lib.hip.lsb_hip_is_initialized())
    res = _lib.Result()
    want = 2 if up else 1
    assert lib.lsb_hip_solver_solve_direct_tier_multi_dev(None, 2, None, 0, None, 0, C.byref(res)) == want
    assert lib.lsb_hip_solver_solve_direct_tier_multi(None, 2, None, 0, None, 0, C.byref(res)) == want
    assert lib.lsb_hip_solver_direct_tier_apply_multi_dev(None, 2, None, 0, None, 0) == want
    assert lib.lsb_hip_solver_direct_tier_multi_round_bytes(None, 2) == 0


@pytest.mark.parametrize("name,tiers", APPLY)
def test_shapes(name, tiers, matrix_path):
    """what the GPU tests rely on these shapes for, from the factor itself"""
    S, T, B = _factor(name, matrix_path, tiers)
    n, nt, lo = T["n"], T["ntier"], T["lo"]
    lens = np.arange(n) - T["first"].astype(np.int64) + 1
    clen = np.diff(B.C.indptr)[int(lo[min(1, nt)]):]
    print(name, "tiers", nt, "rows per tier", np.diff(lo).tolist(), "longest row of W", int(lens.max()),
          "rows of C from", int(clen.min()) if len(clen) else 0, "to", int(clen.max()) if len(clen) else 0)
    if name == PATH3:
        assert np.diff(lo).tolist() == [2, 1] and B.C.nnz == 1
    if name in (DIAG, SINGLE):
        assert nt == 1 and B.C.nnz == 0
    if name == G2D:
        assert nt == tiers and clen.min() == 0 and (clen == 1).any() and clen.max() > 16  # empty rows of C too
        unreached = 0
        at = 0
        for t in range(1, nt):
            offs = T["toffs"][at:at + int(lo[t]) + 1].astype(np.int64)
            unreached += int((np.diff(offs) == 0).sum())
            at += int(lo[t]) + 1
        assert unreached > 0  # k_dirt_bwd_m leaves such a row of Y as it is
    if (name, tiers) == (XN3B, 2):
        cap = _cap()
        assert np.diff(lo).tolist() == [956, 2505] and lens.max() == 2505
        assert cap // 4 < lens.max() <= cap // 2  # staged at width 2, gathered at 4 and 8
    if (name, tiers) == (XN3B, 3):
        assert clen.max() > 256  # 64 lanes per row of C


# ------------------------------------------------------------------------------------ on the GPU
def _dev(a):
    import torch
    a = np.asarray(a, np.float64)
    return torch.from_numpy(a.ravel()).to("cuda:0").view(a.shape)  # (row strides of torch's own, at one row too)


def _full(shape, v):
    import torch
    return torch.full(shape, v, dtype=torch.float64, device="cuda:0")


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
    """B (n, k) solved as blocks by solve_direct_tier_multi_dev: (X (n, k), [fields])"""
    d_X = _full((B.shape[1], B.shape[0]), float("nan"))
    res = s.solve_direct_tier_multi_dev(_dev(B.T), d_X)
    return d_X.cpu().numpy().T, [_fields(r) for r in res]


def _same(got, want):
    """fields equal, NaN == NaN"""
    return all((a == b) or (isinstance(a, float) and np.isnan(a) and np.isnan(b)) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name,tiers", APPLY)
def test_one_application(hip, name, tiers, matrix_path, monkeypatch):
    """direct_tier_apply_multi_dev on 2, 3 and 8 columns against precond_dev on each column alone on the same solver:
    the same bytes, twice, with the windows of k_dirt_rows_m staged as dealt and with at most 16 doubles staged (windows
    of at most 16 / kp rows), so that the wider ones are gathered."""
    S, T, B = _factor(name, matrix_path, tiers)
    n = S.shape[0]
    lens = np.arange(n) - T["first"].astype(np.int64) + 1
    i = np.arange(n, dtype=np.float64)
    R = np.stack([np.sin(i + 0.37 * c) + 0.5 for c in range(8)], axis=1)
    R[:, 1] = 0.0  # one zero column
    first = None
    monkeypatch.delenv("LSBENCH_HIP_DIRECT_TIER_LDS", raising=False)
    for cap in (None, 16):
        if cap:
            monkeypatch.setenv("LSBENCH_HIP_DIRECT_TIER_LDS", str(cap))
            if n >= 400:
                assert lens.max() > cap  # a row alone is wider than what is staged: gathered
        s = _solver(hip, name, matrix_path, tiers)
        assert s.direct_tier_info()[0] == T["ntier"]
        alone = []
        for c in range(8):
            z = _full((n,), float("nan"))
            s.precond_dev(_dev(R[:, c]), z)
            alone.append(z.cpu().numpy())
        assert not alone[1].any()
        if first is None:
            first = alone
        for c in range(8):
            assert alone[c].tobytes() == first[c].tobytes()  # (the single-column kernels: staged = gathered)
        for nrhs in (2, 3, 8):
            out = []
            for _ in range(2):
                d_Z = _full((nrhs, n), float("nan"))
                s.direct_tier_apply_multi_dev(_dev(R[:, :nrhs].T), d_Z)
                out.append(d_Z.cpu().numpy())
            assert out[0].tobytes() == out[1].tobytes()  # run twice: the same bytes
            for c in range(nrhs):
                assert np.isfinite(out[0][c]).all()
                assert out[0][c].tobytes() == alone[c].tobytes(), (name, tiers, cap, nrhs, c)
            if (name, tiers) == (XN3B, 3) and nrhs == 8:  # ... and against numpy, by test_one_application's bound
                for c in (0, 7):
                    za, zb = B.apply(R[:, c]), B.apply(R[:, c], flip=True)
                    e_np, e_gpu = _relerr(zb, za), _relerr(out[0][c], za)
                    bound = 4.0 * max(e_np, EPS)
                    print(name, "column", c, "device against numpy", e_gpu, "numpy between two orders", e_np, "bound",
                          bound)
                    assert bound <= 1e-13 and e_gpu <= bound
        s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name,tiers", [(XN3B, 2), (TJ7A, 3), (G2D, 4)])
def test_solves(hip, name, tiers, matrix_path):
    """Every column of a block against solve_dev on that column alone on the same tiered solver: the bytes of x and
    (status, iters, relres, true_relres, spmvs).  XN3B: 5 columns, a zero column among them, padded to 8; TJ7A: 11
    columns, a block of 8 and one of 3; G2D: 2 columns."""
    S = operator(name, matrix_path)
    n = S.shape[0]
    B = columns(S) if name == XN3B else eleven(S) if name == TJ7A else columns(S)[:, [0, 2]]
    k = B.shape[1]
    settings = [dict(tol=1e-12, maxit=10, use_graph=1), dict(tol=1e-12, maxit=10, use_graph=0),
                dict(tol=1e-10, maxit=10), dict(tol=0.0, maxit=1), dict(tol=0.0, maxit=3)]
    for kw in settings:
        s = _solver(hip, name, matrix_path, tiers, **kw)
        rb = s.direct_tier_multi_round_bytes
        assert rb(1) == s.direct_info[2] and rb(8) - rb(4) == 2 * (rb(4) - rb(2)) and rb(4) > rb(2) > rb(1)
        assert rb(3) == rb(4) and rb(11) == rb(8) and rb(0) == 0
        want = _alone(s, B)
        X, got = _block(s, B)
        X2, got2 = _block(s, B)  # (the hinted block)
        Xh, resh = s.solve_direct_tier_multi(B)  # host buffers
        s.destroy()
        print(name, tiers, kw, "fields of column 0:", got[0])
        for c in range(k):
            assert _same(got[c], want[c][1]) and _same(got2[c], want[c][1]), (kw, c, got[c], want[c][1])
            assert _same(_fields(resh[c]), want[c][1]), (kw, c)
            for Y in (X, X2, np.asarray(Xh)):
                assert np.ascontiguousarray(Y[:, c]).tobytes() == want[c][0].tobytes(), (kw, c)
        if kw["tol"] == 0.0:
            assert all(g == (MAXIT_ST, kw["maxit"], -1.0, -1.0, kw["maxit"] - 1) for g in got)
        else:
            assert all(g[0] == CONVERGED and g[1] <= 2 and g[2] <= kw["tol"] for g in got)
        if name == XN3B and kw["tol"] == 1e-12:
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
    S = operator(TJ7A, matrix_path)
    n = S.shape[0]
    bad = np.arange(1.0, n + 1.0)
    bad[n // 2] = float("nan")
    B = np.stack([np.arange(1.0, n + 1.0), np.zeros(n), bad, S @ np.ones(n)], axis=1)
    s = _solver(hip, TJ7A, matrix_path, 2, tol=1e-30, maxit=3)
    assert s.direct_tier_info()[0] == 2
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
    s = _solver(hip, TJ7A, matrix_path, 2, tol=1e-12, maxit=0)
    X, got = _block(s, Bc)
    s.destroy()
    assert not X.any() and all((g[0], g[1]) == (MAXIT_ST, 0) for g in got)


@pytest.mark.gpu
def test_layout(hip, matrix_path):
    """ld = n + 3 and X starting 8 bytes past a 16-byte boundary: the slack stays the caller's; one column is the
    forwarded path."""
    import torch
    S = operator(XN3B, matrix_path)
    n = S.shape[0]
    B = columns(S)[:, [0, 2, 4]]
    s = _solver(hip, XN3B, matrix_path, 2, tol=1e-12, maxit=10)
    want = _alone(s, B)
    ld = n + 3
    d_B = _full((3, ld), float("nan"))
    d_B[:, :n] = _dev(B.T)
    buf = _full((3 * ld + 2,), 7.0)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    assert (buf.data_ptr() + 8 * off) % 16 == 8
    d_X = buf[off:off + 3 * ld].view(3, ld)
    res = s.solve_direct_tier_multi_dev(d_B, d_X)
    d_Z = buf.clone()[off:off + 3 * ld].view(3, ld)
    d_Z[:] = 7.0
    s.direct_tier_apply_multi_dev(d_B, d_Z)
    around = buf.cpu().numpy()
    X = around[off:off + 3 * ld].reshape(3, ld)
    assert (around[:off] == 7.0).all() and (around[off + 3 * ld:] == 7.0).all() and (X[:, n:] == 7.0).all()
    assert bool((d_Z[:, n:] == 7.0).all()) and bool(torch.isfinite(d_Z[:, :n]).all())
    assert bool(torch.isnan(d_B[:, n:]).all())
    for c in range(3):
        assert X[c, :n].tobytes() == want[c][0].tobytes() and _same(_fields(res[c]), want[c][1])
    # nrhs = 1: forwarded to solve_dev / precond_dev
    d_x1 = _full((1, n), float("nan"))
    res1 = s.solve_direct_tier_multi_dev(_dev(B[:, :1].T), d_x1)
    assert d_x1.cpu().numpy()[0].tobytes() == want[0][0].tobytes() and _same(_fields(res1[0]), want[0][1])
    z1, za = _full((1, n), float("nan")), _full((n,), float("nan"))
    s.direct_tier_apply_multi_dev(_dev(B[:, :1].T), z1)
    s.precond_dev(_dev(B[:, 0]), za)
    assert z1.cpu().numpy()[0].tobytes() == za.cpu().numpy().tobytes()
    s.destroy()


@pytest.mark.gpu
def test_forwarding_and_refusals(hip, matrix_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    S = operator(G2D, matrix_path)
    n = S.shape[0]
    B = columns(S)[:, [0, 2, 4]]
    # a single skyline, made either way: the new entry points are the old ones
    o = dict(op_mode=hip.OP_RAW, krylov=hip.KRYLOV_DIRECT, tol=1e-12, maxit=10)
    for s in (hip.Solver(as_matrix(S), hip.default_opts(**o)), _solver(hip, G2D, matrix_path, 1, tol=1e-12, maxit=10)):
        assert s.direct_tier_info()[0] == 1
        d_X = _full((3, n), float("nan"))
        old = s.solve_direct_multi_dev(_dev(B.T), d_X)
        Xo = d_X.cpu().numpy()
        X, got = _block(s, B)
        assert X.T.tobytes() == Xo.tobytes() and all(_same(g, _fields(r)) for g, r in zip(got, old))
        Xh, resh = s.solve_direct_tier_multi(B)
        assert np.ascontiguousarray(np.asarray(Xh).T).tobytes() == Xo.tobytes()
        assert all(_same(_fields(a), _fields(r)) for a, r in zip(resh, old))
        za, zb = _full((3, n), float("nan")), _full((3, n), float("nan"))
        s.direct_apply_multi_dev(_dev(B.T), za)
        s.direct_tier_apply_multi_dev(_dev(B.T), zb)
        assert za.cpu().numpy().tobytes() == zb.cpu().numpy().tobytes() and bool(torch.isfinite(zb).all())
        for k in (1, 2, 3, 8, 11):
            assert s.direct_tier_multi_round_bytes(k) == s.direct_multi_round_bytes(k) > 0
        s.destroy()
    # not a direct solver: 2, nothing written
    d_B = _dev(B[:, :2].T)
    d_X = _full((2, n), 7.0)
    res = (_lib.Result * 2)()
    Bh = np.asfortranarray(B[:, :2])
    Xh = np.full((n, 2), 7.0, order="F")
    j = hip.Solver(as_matrix(S), hip.default_opts(op_mode=hip.OP_RAW))  # Jacobi-PCG
    assert lib.lsb_hip_solver_solve_direct_tier_multi_dev(j._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_direct_tier_apply_multi_dev(j._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_solve_direct_tier_multi(j._h, 2, Bh.ctypes.data, n, Xh.ctypes.data, n, res) == 2
    assert j.direct_tier_multi_round_bytes(2) == 0
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (Xh == 7.0).all()
    j.destroy()
    # bad arguments on a tiered solver: 2, nothing written, and it still serves
    s = _solver(hip, G2D, matrix_path, 3, tol=1e-12, maxit=10)
    assert s.direct_tier_info()[0] == 3 and s.direct_tier_multi_round_bytes(0) == 0
    for fn in (lib.lsb_hip_solver_solve_direct_tier_multi_dev, lib.lsb_hip_solver_direct_tier_apply_multi_dev):
        extra = (res,) if fn is lib.lsb_hip_solver_solve_direct_tier_multi_dev else ()
        assert fn(s._h, 0, _ptr(d_B), n, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n - 1, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n, _ptr(d_X), n - 1, *extra) == 2
        assert fn(s._h, 2, None, n, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n, None, n, *extra) == 2
    assert lib.lsb_hip_solver_solve_direct_tier_multi(s._h, 0, Bh.ctypes.data, n, Xh.ctypes.data, n, res) == 2
    assert lib.lsb_hip_solver_solve_direct_tier_multi(s._h, 2, Bh.ctypes.data, n - 1, Xh.ctypes.data, n, res) == 2
    assert lib.lsb_hip_solver_solve_direct_tier_multi(s._h, 2, None, n, Xh.ctypes.data, n, res) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (Xh == 7.0).all()
    # the old entry points keep answering 2 on it
    assert lib.lsb_hip_solver_solve_direct_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_direct_multi_round_bytes(s._h, 2) == 0
    assert lib.lsb_hip_solver_solve_direct_tier_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 0  # ... serves
    assert res[0].status == CONVERGED and res[1].status == CONVERGED and bool(torch.isfinite(d_X).all())
    s.destroy()
