"""AMG as the solver on blocks of right-hand sides (lsb_hip_solver_amg_solve_multi[_dev], _amg_cycle_multi_dev,
_amg_solve_multi_bytes; hip_rich_m.hip, hip_rich_m_drv.c, and the fp32 V-cycle on blocks, hip_amg_f32_m.hip): the
stationary V-cycle iteration of test_richardson.py per column of a block, the hierarchy streamed once per cycle.

The yardsticks are the single-column entry points and numpy.  A column of amg_cycle_multi_dev has the bytes of
precond_dev on that column alone; a solve is, bit for bit, the iteration replayed from torch through amg_cycle_multi_dev
and spmm_dev; a column's x, iters, status and relres do not depend on the block it runs in; the cycle counts are those
of test_richardson.richardson around the numpy cycles of test_amg_f32._cycles, to +-1.

CPU: the surface, and the numpy iteration on the five columns of test_mrhs.columns on every operator of
test_richardson.OPS -- its cycle counts are what the GPU tests compare against.  GPU: the six groups below."""
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
from test_amg_f32 import _cycles, _hier, _op, _relerr
from test_mrhs import columns, eleven
from test_richardson import LAP2D, LAP3D, MAXIT, ONE, OPS, XN3B, richardson
from test_amg_f32 import POWERLAW

CONVERGED, BREAKDOWN, MAXIT_ST = 1, 2, 3
FOUR = ("lsb_hip_solver_amg_solve_multi_dev", "lsb_hip_solver_amg_solve_multi", "lsb_hip_solver_amg_cycle_multi_dev",
        "lsb_hip_solver_amg_solve_multi_bytes")
# (Chebyshev smoother, fp32 cycle) of the three flavours that are served
FLAVOURS = [(0, 0), (1, 0), (0, 1)]


# ------------------------------------------------------------------------------------ the restatement
_COUNTS = {}


def np_counts(name, matrix_path, f32):
    """the numpy iteration with l1-Jacobi at nu = 1 to 1e-10 on each of the five columns, made once:
    [(cycles to 1e-8, cycles to 1e-10, status)] -- (0, 0, CONVERGED) for the zero column"""
    key = (name, f32)
    if key not in _COUNTS:
        S = _op(name, matrix_path)
        B = columns(S)
        v = _cycles(name, matrix_path, False)[1 if f32 else 0]
        out = []
        for c in range(B.shape[1]):
            _, it, st, _, first, _ = richardson(S, B[:, c], lambda r: v(r, 1), 1e-10, MAXIT, marks=(1e-8, 1e-10))
            out.append((first.get(1e-8, 0), it, st))
        _COUNTS[key] = out
    return _COUNTS[key]


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
    for m in ("amg_solve_multi_dev", "amg_solve_multi", "amg_cycle_multi_dev", "amg_solve_multi_bytes"):
        assert callable(getattr(la.Solver, m)), m
    # what test_richardson.test_surface pins still holds: no word with "rich" before a "(" in the header, no exported
    # name of the iteration's; the new launchers stay inside
    assert not re.search(r"\b\w*rich\w*\s*\(", header, re.I)
    assert exported and not [s for s in exported if "richardson" in s.lower() or s.startswith("lsb_k_rich")]
    assert not [s for s in exported if re.fullmatch(r"lsb_k_amg32_\w+_m", s)]
    assert "Warm starts on blocks are not built" in re.sub(r"\s+", " ", header[header.index(FOUR[0]) - 4000:])
    # struct lsb_hip_opts gained nothing
    assert [f[0] for f in _lib.Opts._fields_][-1] == "amg_cheb_ratio" and list(_lib.Opts._TAIL) == ["fsai_blocks"]
    # a null solver: 2 once the backend is up, 1 before (whichever this process is in), 0 bytes either way
    up = int(lib.hip.lsb_hip_is_initialized())
    res = _lib.Result()
    want = 2 if up else 1
    assert lib.lsb_hip_solver_amg_solve_multi_dev(None, 1, None, 0, None, 0, C.byref(res)) == want
    assert lib.lsb_hip_solver_amg_solve_multi(None, 1, None, 0, None, 0, C.byref(res)) == want
    assert lib.lsb_hip_solver_amg_cycle_multi_dev(None, 1, None, 0, None, 0) == want
    assert lib.lsb_hip_solver_amg_solve_multi_bytes(None, 2) == 0


@pytest.mark.parametrize("name", OPS)
def test_restatement(name, matrix_path):
    """numpy Richardson per column, tol 1e-8, nu = 1, l1-Jacobi in fp64 and in fp32: every non-zero column converges,
    the zero column stops at 0 cycles; on the two grids at least three distinct counts occur, so the GPU tests exercise
    frozen columns.  The counts are printed; the GPU tests take them from np_counts."""
    for f32 in (0, 1):
        got = np_counts(name, matrix_path, f32)
        print(name, "fp32" if f32 else "fp64", "cycles to 1e-8:", " / ".join(str(g[0]) for g in got),
              "to 1e-10:", " / ".join(str(g[1]) for g in got))
        assert len(got) == 5 and got[1] == (0, 0, CONVERGED)
        for c in (0, 2, 3, 4):
            assert got[c][2] == CONVERGED and 1 <= got[c][0] <= got[c][1] <= MAXIT, (c, got[c])
        if name in (LAP2D, LAP3D):
            assert len({g[0] for g in got}) >= 3
    if name == ONE:  # one level: the dense solve is exact after one cycle
        assert [g[0] for g in np_counts(name, matrix_path, 0)] == [1, 0, 1, 1, 1]
    # as counted when the method was proposed, with l1-Jacobi in fp64 and in fp32 alike
    proposed = {LAP2D: [51, 0, 36, 35, 55], LAP3D: [149, 0, 132, 78, 115]}
    if name in proposed:
        assert [g[0] for g in np_counts(name, matrix_path, 0)] == proposed[name]
        assert [g[0] for g in np_counts(name, matrix_path, 1)] == proposed[name]


# ------------------------------------------------------------------------------------ on the GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _full(shape, v):
    import torch
    return torch.full(shape, v, dtype=torch.float64, device="cuda:0")


def _kw(hip, cheb=0, f32=0, nu=1, **kw):
    kw.update(amg_sweeps=nu, amg_smoother=hip.AMG_SMOOTH_CHEB if cheb else hip.AMG_SMOOTH_L1JACOBI,
              amg_precision=hip.AMG_PREC_FP32 if f32 else hip.AMG_PREC_FP64)
    return kw


def _solver(hip, name, matrix_path, **kw):
    """a Richardson solver on the operator the numpy side uses, as read"""
    kw.setdefault("op_mode", hip.OP_RAW)
    kw.setdefault("krylov", hip.KRYLOV_RICHARDSON)
    kw.setdefault("precond", hip.PRECOND_AMG)
    return hip.Solver(as_matrix(_op(name, matrix_path)), hip.default_opts(**kw))


def _fields(r):
    return (r.status, r.iters, r.relres, r.spmvs)


def _block(s, B):
    """B (n, k) solved as blocks by amg_solve_multi_dev into an X pre-filled with NaN: (X (n, k), [fields])"""
    d_X = _full((B.shape[1], B.shape[0]), float("nan"))
    res = s.amg_solve_multi_dev(_dev(B.T), d_X)
    return d_X.cpu().numpy().T, [_fields(r) for r in res]


def _cycle_block(s, R):
    """Z (n, k) of amg_cycle_multi_dev on R (n, k), into a Z pre-filled with NaN"""
    d_Z = _full((R.shape[1], R.shape[0]), float("nan"))
    s.amg_cycle_multi_dev(_dev(R.T), d_Z)
    return d_Z.cpu().numpy().T


def _cycle_alone(s, R):
    out = []
    for c in range(R.shape[1]):
        z = _full((R.shape[0],), float("nan"))
        s.precond_dev(_dev(R[:, c]), z)
        out.append(z.cpu().numpy())
    return out


def _check_cycle(s, R, tag):
    """widths 2, 3 (one padded column), 5 and 8, each twice: a column has the bytes of precond_dev on it alone; then
    a NaN column stays in its column"""
    n = R.shape[0]
    alone = _cycle_alone(s, R)
    assert not alone[1].any() and all(np.isfinite(z).all() for z in alone)
    for nrhs in (2, 3, 5, 8):
        Z, Z2 = _cycle_block(s, R[:, :nrhs]), _cycle_block(s, R[:, :nrhs])
        assert Z.tobytes() == Z2.tobytes(), (tag, nrhs)
        for c in range(nrhs):
            assert np.ascontiguousarray(Z[:, c]).tobytes() == alone[c].tobytes(), (tag, nrhs, c)
    bad = R[:, :5].copy()
    bad[:, 3] = R[:, 0]
    bad[n // 2, 3] = float("nan")
    Z = _cycle_block(s, bad)
    assert np.isnan(Z[:, 3]).any()
    for c in (0, 1, 2, 4):
        assert np.ascontiguousarray(Z[:, c]).tobytes() == alone[c].tobytes(), (tag, "beside a NaN column", c)


# ---- 1. a column of amg_cycle_multi_dev has the bytes of precond_dev on that column alone
@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("cheb,f32", FLAVOURS)
@pytest.mark.parametrize("name", OPS)
def test_cycle_has_the_bits_of_the_single_cycle(hip, name, cheb, f32, nu, matrix_path):
    R = eleven(_op(name, matrix_path))[:, :8]
    s = _solver(hip, name, matrix_path, **_kw(hip, cheb, f32, nu))
    assert s.amg_precision == f32
    _check_cycle(s, R, (name, cheb, f32, nu))
    s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("cheb,f32", FLAVOURS)
def test_cycle_on_renumbered_solvers(hip, cheb, f32, monkeypatch):
    A = hip.lsbench_matrix_synth("lap2d:nx=60,ny=50")
    rng = np.random.default_rng(5)
    R = rng.standard_normal((A.nrows, 8))
    R[:, 1] = 0.0
    base = dict(op_mode=hip.OP_RAW, precond=hip.PRECOND_AMG, krylov=hip.KRYLOV_RICHARDSON)
    s = hip.Solver(A, hip.default_opts(reorder=1, **_kw(hip, cheb, f32, **base)))
    _check_cycle(s, R, ("re-ordered", cheb, f32))
    s.destroy()
    A = hip.lsbench_matrix_synth("lap2d:nx=2050,ny=12")
    R = rng.standard_normal((A.nrows, 8))
    R[:, 1] = 0.0
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1")
    s = hip.Solver(A, hip.default_opts(**_kw(hip, cheb, f32, **base)))
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    assert s.padded and s.n_local == A.nrows
    _check_cycle(s, R, ("line-padded", cheb, f32))
    s.destroy()


# ---- 2. replay, bit for bit
def _replay(s, j, B, cycles):
    """the iteration driven from torch through public entry points -- Z by amg_cycle_multi_dev on s, Q by spmm_dev of
    the Jacobi solver j: {k: (X_k (n, cols), [||r_c|| / ||b_c||])}"""
    import torch
    d_B = _dev(B.T)
    X, R = torch.zeros_like(d_B), d_B.clone()
    bn = np.linalg.norm(B, axis=0)
    out = {}
    for k in range(1, cycles + 1):
        Z, Q = _full(tuple(d_B.shape), float("nan")), _full(tuple(d_B.shape), float("nan"))
        s.amg_cycle_multi_dev(R, Z)
        j.spmm_dev(Z, Q)
        X = X + Z
        R = R - Q
        rn = np.linalg.norm(R.cpu().numpy(), axis=1)
        out[k] = (X.cpu().numpy().T, [float(rn[c] / bn[c]) if bn[c] else 0.0 for c in range(B.shape[1])])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cheb,f32", FLAVOURS)
@pytest.mark.parametrize("name", OPS)
def test_replay_bit_for_bit(hip, name, cheb, f32, matrix_path):
    S = _op(name, matrix_path)
    B = columns(S)
    j = hip.Solver(as_matrix(S), hip.default_opts(op_mode=hip.OP_RAW))  # a default Jacobi solver: its spmm_dev
    want = None
    for N in (5, 2, 1):
        s = _solver(hip, name, matrix_path, tol=0.0, maxit=N, **_kw(hip, cheb, f32))
        if want is None:
            want = _replay(s, j, B, 5)
        X, got = _block(s, B)
        s.destroy()
        print(name, "cheb", cheb, "f32", f32, "cycles", N, "relres", [g[2] for g in got], "the replay's", want[N][1])
        assert np.isfinite(X).all()
        for c in range(5):
            if c == 1:
                assert got[c] == (CONVERGED, 0, 0.0, 0) and not X[:, c].any()
                continue
            assert (got[c][0], got[c][1], got[c][3]) == (MAXIT_ST, N, N), (c, got[c])
            assert np.ascontiguousarray(X[:, c]).tobytes() == np.ascontiguousarray(want[N][0][:, c]).tobytes(), (N, c)
            assert abs(got[c][2] - want[N][1][c]) <= 1e-12 * want[N][1][c], (N, c, got[c][2], want[N][1][c])
    j.destroy()


# ---- 3. width and company do not matter
@pytest.mark.gpu
@pytest.mark.parametrize("name,cheb,f32", [(LAP2D, 0, 0), (LAP3D, 0, 1), (POWERLAW, 1, 0), (ONE, 0, 1), (XN3B, 0, 1)])
def test_width_and_company_do_not_matter(hip, name, cheb, f32, matrix_path):
    """a column's x, iters, status and relres are the same bytes in a block of 2, of 5 and of 8, among 11 columns
    (8 + 3), with graphs on and off, from host buffers, and with X 8 bytes past a 16-byte boundary (the slack
    untouched)"""
    S = _op(name, matrix_path)
    n = S.shape[0]
    B11 = eleven(S)  # columns 0 .. 4 are columns(S); column 8 is column 0 again
    tol = 1e-8 if name != XN3B else 1e-4  # (XN3B: 1247 cycles to 1e-8; the property does not need them)
    ref = None
    for graph in (1, 0):
        s = _solver(hip, name, matrix_path, tol=tol, maxit=MAXIT, use_graph=graph, **_kw(hip, cheb, f32))
        X11, f11 = _block(s, B11)
        X11b, f11b = _block(s, B11)  # (the hinted blocks)
        assert X11.tobytes() == X11b.tobytes() and f11 == f11b
        if ref is None:
            ref = (X11, f11)
            print(name, "cheb", cheb, "f32", f32, "cycles per column:", [f[1] for f in f11])
            assert all(f[0] == CONVERGED for f in f11)
            if name in (LAP2D, LAP3D):  # (test_restatement: columns freeze while others run on)
                assert len({f[1] for f in f11[:5]}) >= 3
        assert X11.tobytes() == ref[0].tobytes() and f11 == ref[1], graph
        assert X11[:, 8].tobytes() == X11[:, 0].tobytes() and f11[8] == f11[0]
        for cols in ([0, 2], [0, 1, 2, 3, 4], list(range(8)), [4, 3]):
            X, f = _block(s, B11[:, cols])
            for i, c in enumerate(cols):
                assert X[:, i].tobytes() == ref[0][:, c].tobytes() and f[i] == ref[1][c], (graph, cols, c)
        if graph:
            Xh, rh = s.amg_solve_multi(B11[:, :5])  # host buffers
            assert all(np.asarray(Xh)[:, c].tobytes() == ref[0][:, c].tobytes() for c in range(5))
            assert [_fields(r) for r in rh] == ref[1][:5]
            # ld = n + 3 and X starting 8 bytes past a 16-byte boundary: the slack stays the caller's
            ld = n + 3
            d_B = _full((5, ld), float("nan"))
            d_B[:, :n] = _dev(B11[:, :5].T)
            buf = _full((5 * ld + 2,), 7.0)
            off = 1 if buf.data_ptr() % 16 == 0 else 0
            assert (buf.data_ptr() + 8 * off) % 16 == 8
            res = s.amg_solve_multi_dev(d_B, buf[off:off + 5 * ld].view(5, ld))
            around = buf.cpu().numpy()
            X = around[off:off + 5 * ld].reshape(5, ld)
            assert (around[:off] == 7.0).all() and (around[off + 5 * ld:] == 7.0).all() and (X[:, n:] == 7.0).all()
            for c in range(5):
                assert X[c, :n].tobytes() == ref[0][:, c].tobytes() and _fields(res[c]) == ref[1][c], c
        s.destroy()


# ---- 4. against the single solve and numpy
@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("name", OPS)
def test_against_the_single_solve_and_numpy(hip, name, f32, matrix_path):
    S = _op(name, matrix_path)
    B = columns(S)
    counts, counts64 = np_counts(name, matrix_path, f32), np_counts(name, matrix_path, 0)
    for k, tol in enumerate((1e-8, 1e-10)):
        s = _solver(hip, name, matrix_path, tol=tol, maxit=MAXIT, **_kw(hip, 0, f32))
        X, got = _block(s, B)
        x0 = _full((S.shape[0],), float("nan"))
        r0 = s.solve_dev(_dev(B[:, 0]), x0)
        s.destroy()
        x0 = x0.cpu().numpy()
        print(name, "f32", f32, "tol", tol, "cycles", [g[1] for g in got], "numpy's", [c[k] for c in counts],
              "the fp64 cycle's in numpy", [c[k] for c in counts64], "solve_dev on column 0:", r0.iters,
              "x against it", _relerr(X[:, 0], x0))
        for c in range(5):
            assert got[c][0] == CONVERGED and got[c][3] == got[c][1], (c, got[c])
            assert abs(int(got[c][1]) - counts[c][k]) <= 1, (c, got[c][1], counts[c][k])
            if f32:
                assert abs(int(got[c][1]) - counts64[c][k]) <= 1, (c, got[c][1], counts64[c][k])
            if c == 1:
                assert got[c][1] == 0 and not X[:, c].any()
                continue
            true = np.linalg.norm(B[:, c] - S @ X[:, c]) / np.linalg.norm(B[:, c])
            print("   column", c, "relres", got[c][2], "recomputed on the CPU", true)
            assert true <= tol * (1 + 1e-6), (c, true)
        assert r0.status == CONVERGED and _relerr(X[:, 0], x0) <= 1e-12


# ---- 5. stop rules
@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("f32", [0, 1])
def test_stop_rules(hip, f32, graph, matrix_path):
    S = _op(LAP2D, matrix_path)
    n = S.shape[0]
    B = columns(S)
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=MAXIT, use_graph=graph, **_kw(hip, 0, f32))
    X, got = _block(s, B)
    # the zero column: CONVERGED, 0 cycles, x = 0, while the others run on
    assert got[1] == (CONVERGED, 0, 0.0, 0) and not X[:, 1].any()
    assert all(got[c][0] == CONVERGED and got[c][1] > 5 for c in (0, 2, 3, 4))
    # a column holding one NaN: BREAKDOWN at cycle 1, and the other columns keep the bytes they have without it
    bad = B.copy()
    bad[n // 2, 3] = float("nan")
    Xb, gotb = _block(s, bad)
    assert (gotb[3][0], gotb[3][1]) == (BREAKDOWN, 1)
    for c in (0, 1, 2, 4):
        assert Xb[:, c].tobytes() == X[:, c].tobytes() and gotb[c] == got[c], c
    # ... and the solver is as good as before
    X2, got2 = _block(s, B)
    s.destroy()
    assert X2.tobytes() == X.tobytes() and got2 == got
    # a maxit below some columns' counts: those are MAXIT at that cycle, the others as before
    cut = sorted(g[1] for g in got)[2]
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=cut, use_graph=graph, **_kw(hip, 0, f32))
    Xc, gotc = _block(s, B)
    s.destroy()
    for c in range(5):
        if got[c][1] <= cut:
            assert gotc[c] == got[c] and Xc[:, c].tobytes() == X[:, c].tobytes(), c
        else:
            assert (gotc[c][0], gotc[c][1], gotc[c][3]) == (MAXIT_ST, cut, cut) and gotc[c][2] > 1e-8, c
    # maxit = 0: nothing to do
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=0, use_graph=graph, **_kw(hip, 0, f32))
    X0, got0 = _block(s, B)
    s.destroy()
    assert not X0.any() and got0[1][:2] == (CONVERGED, 0) and all(got0[c][:2] == (MAXIT_ST, 0) for c in (0, 2, 3, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
def test_verify(hip, f32, matrix_path):
    """verify = 1: each column's true_relres meets tol and agrees with the CPU's to two digits; spmvs counts the
    recomputed residuals; without verify true_relres is -1"""
    S = _op(LAP2D, matrix_path)
    B = columns(S)
    tol = 1e-10
    s = _solver(hip, LAP2D, matrix_path, tol=tol, maxit=MAXIT, **_kw(hip, 0, f32))
    d_X = _full((5, S.shape[0]), float("nan"))
    assert all(r.true_relres == -1.0 and r.corrections == 0 for r in s.amg_solve_multi_dev(_dev(B.T), d_X))
    s.destroy()
    s = _solver(hip, LAP2D, matrix_path, tol=tol, maxit=MAXIT, verify=1, **_kw(hip, 0, f32))
    res = s.amg_solve_multi_dev(_dev(B.T), d_X)
    s.destroy()
    X = d_X.cpu().numpy().T
    for c, r in enumerate(res):
        if c == 1:
            assert (r.status, r.iters, r.spmvs, r.true_relres) == (CONVERGED, 0, 0, -1.0)
            continue
        true = np.linalg.norm(B[:, c] - S @ X[:, c]) / np.linalg.norm(B[:, c])
        print("column", c, "cycles", r.iters, "products", r.spmvs, "corrections", r.corrections, "true_relres",
              r.true_relres, "on the CPU", true)
        assert r.status == CONVERGED and 0.0 <= r.true_relres <= tol and r.corrections <= 6
        assert r.spmvs == r.iters + r.corrections + 1 and r.relres == r.true_relres
        assert abs(r.true_relres - true) <= 1e-2 * true


# ---- 6. refusals, and the bytes
@pytest.mark.gpu
def test_refusals(hip, matrix_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    S = _op(ONE, matrix_path)
    n = S.shape[0]
    B = np.asfortranarray(np.tile(np.arange(1.0, n + 1.0)[:, None], (1, 2)))
    d_B = _dev(B.T)
    d_X = _full((2, n), 7.0)
    X = np.full((n, 2), 7.0, order="F")
    res = (_lib.Result * 2)()
    rich = dict(krylov=hip.KRYLOV_RICHARDSON, precond=hip.PRECOND_AMG)
    others = [dict(precond=hip.PRECOND_AMG),  # AMG under PCG
              dict(),  # Jacobi
              dict(krylov=hip.KRYLOV_DIRECT),
              dict(amg_smoother=hip.AMG_SMOOTH_MCGS, **rich),
              dict(amg_smoother=hip.AMG_SMOOTH_CHEB, amg_precision=hip.AMG_PREC_FP32, **rich)]
    for kw in others:
        o = hip.Solver(as_matrix(S), hip.default_opts(op_mode=hip.OP_RAW, **kw))
        assert lib.lsb_hip_solver_amg_solve_multi_dev(o._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2, kw
        assert lib.lsb_hip_solver_amg_cycle_multi_dev(o._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2, kw
        assert lib.lsb_hip_solver_amg_solve_multi(o._h, 2, B.ctypes.data, n, X.ctypes.data, n, res) == 2, kw
        assert o.amg_solve_multi_bytes(2) == 0
        o.destroy()
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (X == 7.0).all()
    s = _solver(hip, ONE, matrix_path)
    assert s.amg_solve_multi_bytes(0) == 0
    for fn in (lib.lsb_hip_solver_amg_solve_multi_dev, lib.lsb_hip_solver_amg_cycle_multi_dev):
        extra = (res,) if fn is lib.lsb_hip_solver_amg_solve_multi_dev else ()
        assert fn(s._h, 0, _ptr(d_B), n, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n - 1, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n, _ptr(d_X), n - 1, *extra) == 2
        assert fn(s._h, 2, None, n, _ptr(d_X), n, *extra) == 2
        assert fn(s._h, 2, _ptr(d_B), n, None, n, *extra) == 2
    assert lib.lsb_hip_solver_amg_solve_multi(s._h, 0, B.ctypes.data, n, X.ctypes.data, n, res) == 2
    assert lib.lsb_hip_solver_amg_solve_multi(s._h, 2, B.ctypes.data, n - 1, X.ctypes.data, n, res) == 2
    assert lib.lsb_hip_solver_amg_solve_multi(s._h, 2, None, n, X.ctypes.data, n, res) == 2
    # the old entry points still answer 2 on a Richardson solver
    assert lib.lsb_hip_solver_solve_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_spmm_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_solve_block_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all()) and (X == 7.0).all()
    assert lib.lsb_hip_solver_amg_solve_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 0  # ... and serves
    assert res[0].status == CONVERGED and res[0].iters <= 2 and bool(torch.isfinite(d_X).all())
    # one column is forwarded to solve_dev / precond_dev
    x1, xa = _full((1, n), float("nan")), _full((n,), float("nan"))
    r1 = s.amg_solve_multi_dev(d_B[:1], x1)
    ra = s.solve_dev(d_B[0], xa)
    assert x1.cpu().numpy()[0].tobytes() == xa.cpu().numpy().tobytes() and _fields(r1[0]) == _fields(ra)
    s.amg_cycle_multi_dev(d_B[:1], x1)
    s.precond_dev(d_B[0], xa)
    assert x1.cpu().numpy()[0].tobytes() == xa.cpu().numpy().tobytes()
    s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("cheb,f32", FLAVOURS)
def test_bytes(hip, cheb, f32, matrix_path):
    """amg_solve_multi_bytes: at one column the single cycle's figure; per column of the width a constant that holds the
    SpMM's 16 n and the update's 48 n; on the one-level operator every term written out"""
    for name in (LAP2D, ONE):
        S = _op(name, matrix_path)
        n, nnz = S.shape[0], S.nnz
        s = _solver(hip, name, matrix_path, **_kw(hip, cheb, f32))
        by = {k: s.amg_solve_multi_bytes(k) for k in (1, 2, 3, 4, 5, 8, 11)}
        cyc = s.amg_cycle_bytes
        s.destroy()
        print(name, "cheb", cheb, "f32", f32, "bytes per cycle:", by, "the V-cycle alone:", cyc)
        assert by[1] == cyc + 12 * nnz + 64 * n
        assert by[3] == by[4] and by[5] == by[8] == by[11]
        per = by[2] - by[1]
        assert per > 64 * n and by[4] - by[2] == 2 * per and by[8] - by[4] == 4 * per
        if name == ONE:  # the dense inverse once, its two vector passes and the two ends per column
            mat, vec = (4 * n * n, 16 * n) if f32 else (8 * n * n, 16 * n)
            assert by[8] == mat + 12 * nnz + 8 * (vec + 64 * n)
