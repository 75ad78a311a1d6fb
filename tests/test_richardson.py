"""AMG as the solver: stationary V-cycle iterations (opts.krylov = KRYLOV_RICHARDSON, --krylov richardson;
hip_rich.hip, hip_rich_drv.c).

    x = 0, r = b;  cycle k:  z = M^-1 r (one V-cycle), q = S z, x += z, r -= q, iters = k,
    stop: r.r <= tol^2 b.b CONVERGED, r.r not finite BREAKDOWN, k >= maxit MAXIT (tol = 0 never converges)

The iteration is restated here in numpy (`richardson`) around the cycles the other AMG tests restate: test_amg.Hier
(l1-Jacobi, fp64), test_amg_cheb.Cheb (Chebyshev smoother), test_amg_f32.H32 (either, in float32).

CPU: the surface, and what the GPU tests lean on -- the numpy iteration reaches 1e-10 on every operator below with
every cycle, in the cycle counts measured when the method was proposed, and the fp32 cycle takes the fp64 cycle's
count within `margin`.  GPU: the solve against a replay of its own cycles through the solver's public entry points,
bit for bit; against numpy; the same bits from graphs, repeated solves, any poll interval and an x that is only
8-byte aligned; the stop rules; the fp32 cycle; re-numbered solvers; verify; the refusals and the driver."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from oracle import oracle as O
from test_amg import as_matrix
from test_amg_f32 import POWERLAW, _cycles, _hier, _op, _relerr

XN3B, LAP2D, ONE, LAP3D = "xn3b_A_18", "lap2d:nx=130,ny=70", "lap2d:nx=12,ny=9", "lap3d:nx=24,ny=20,nz=18"
# the smallest operators that reach every lane count and every level shape: lanes up to 64 on the coarse levels,
# three levels, ragged rows, one level (the dense solve alone), a 3-D stencil
OPS = [XN3B, LAP2D, POWERLAW, ONE, LAP3D]
# (operator, nu) -> cycles to 1e-8 and to 1e-10 of the numpy iteration with Hier.vcycle and b_i = i, as measured
# when the method was proposed; the counts at nu = 1 are asserted to +-1 (a threshold crossed in the last digit)
TABLE = {(LAP2D, 1): (51, 66), (LAP2D, 2): (27, 35), (LAP3D, 1): (149, 187), (LAP3D, 2): (81, 102),
         (XN3B, 1): (1247, 1610), (XN3B, 2): (625, 806)}
MAXIT = 4000
CONVERGED, BREAKDOWN, MAXIT_ST = 1, 2, 3


def margin(it64):
    """cycles the fp32 cycle may take more or fewer than the fp64 cycle: the project's rule for PCG around the two
    cycles (test_amg_f32.py), max(2, 4 %).  test_cpu_precondition prints the numpy pairs it is taken from; numpy alone
    stays inside it on every operator, so it is not widened."""
    return max(2, 0.04 * it64)


# ------------------------------------------------------------------------------------ the restatement
def richardson(S, b, M, tol, maxit, marks=(), keep=()):
    """the device's iteration.  Returns (x, cycles, status, relres, first cycle at which relres <= each of `marks`,
    {k: x_k for k in keep})"""
    x = np.zeros_like(b)
    r = b.copy()
    bb = b @ b
    thresh2 = tol * tol * bb
    first, kept = {}, {}
    if bb == 0.0:
        return x, 0, CONVERGED, 0.0, first, kept
    status, k, rr = MAXIT_ST, 0, bb
    while k < maxit:
        z = M(r)
        q = S @ z
        x = x + z
        r = r - q
        k += 1
        rr = r @ r
        if k in keep:
            kept[k] = x.copy()
        for m in marks:
            if m not in first and rr <= m * m * bb:
                first[m] = k
        if thresh2 > 0.0 and rr <= thresh2:
            status = CONVERGED
            break
        if not np.isfinite(rr):
            status = BREAKDOWN
            break
    return x, k, status, float(np.sqrt(rr / bb)), first, kept


_RUNS = {}


def _np_run(name, matrix_path, cheb=False, f32=False, nu=1):
    """the numpy iteration to 1e-10 on b_i = i, made once: (x, cycles, status, relres, first crossings of 1e-8 and
    1e-10, {5: x_5})"""
    key = (name, cheb, f32, nu)
    if key not in _RUNS:
        S = _op(name, matrix_path)
        v64, v32 = _cycles(name, matrix_path, cheb)
        v = v32 if f32 else v64
        _RUNS[key] = richardson(S, O.rhs(S.shape[0]), lambda r: v(r, nu), 1e-10, MAXIT, marks=(1e-8, 1e-10), keep=(5,))
    return _RUNS[key]


# ------------------------------------------------------------------------------------ without a GPU
def test_surface():
    assert la.KRYLOV_RICHARDSON == 5 and _lib.KRYLOV_RICHARDSON == 5
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    assert "LSB_KRYLOV_RICHARDSON = 5" in header and "LSB_KRYLOV_BICGSTAB = 4" in header
    assert "RICHARDSON" in header[header.index("int krylov;"):header.index("int restart;")]
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_cdna4.c")) as f:
        src = f.read()
    assert re.search(r'\{"richardson",\s*LSB_KRYLOV_RICHARDSON\}', src[src.index("CH_KRYLOV[]"):])
    lib = _lib.load()
    o, got = la.default_opts(), _lib.Opts()
    try:
        assert lib.hip_cdna4_set_option(b"krylov", b"richardson") == 0
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.krylov == 5
        assert lib.hip_cdna4_set_option(b"krylov", b"richardson2") == 1
    finally:
        lib.lsb_hip_set_opts(C.byref(o))
    assert la.default_opts().krylov == la.KRYLOV_AUTO  # a protocol and a diagnostic, not the default
    # nothing new in the C-ABI: the header declares no function for it and the library exports none
    assert not re.search(r"\b\w*rich\w*\s*\(", header, re.I)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in nm.splitlines() if ln.split()]
    assert names and not [s for s in names if "richardson" in s.lower() or s.startswith("lsb_k_rich")]
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    assert "richardson" in subprocess.run([drv, "--help"], capture_output=True, text=True).stdout


def test_restatement_stop_rules():
    S = _op(ONE, None)
    H, _ = _hier(ONE, None)
    assert len(H.A) == 1
    b = O.rhs(S.shape[0])
    x, k, st, rel, _, _ = richardson(S, b, H.vcycle, 1e-8, 50)
    assert (k, st) == (1, CONVERGED) and rel < 1e-12  # one level: the dense solve is exact after one cycle
    x, k, st, rel, _, _ = richardson(S, b, H.vcycle, 0.0, 3)
    assert (k, st) == (3, MAXIT_ST)  # tol = 0 never converges
    assert richardson(S, 0.0 * b, H.vcycle, 1e-8, 50)[1:3] == (0, CONVERGED)
    bad = b.copy()
    bad[3] = float("nan")
    assert richardson(S, bad, H.vcycle, 1e-8, 50)[1:3] == (1, BREAKDOWN)


@pytest.mark.parametrize("name", OPS)
def test_cpu_precondition(name, matrix_path):
    """The numpy iteration reaches 1e-10 on b_i = i with every cycle the device has; with Hier.vcycle at nu = 1 in the
    counts of TABLE to +-1; the fp32 cycle in the fp64 cycle's count within `margin` (the pairs are printed)."""
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    for cheb in (False, True):
        for nu in (1, 2):
            x64, it64, st64, rel64, first64, _ = _np_run(name, matrix_path, cheb, False, nu)
            x32, it32, st32, rel32, first32, _ = _np_run(name, matrix_path, cheb, True, nu)
            print(name, "Chebyshev" if cheb else "l1-Jacobi", "nu", nu, "cycles to 1e-8 / 1e-10: fp64 cycle",
                  first64.get(1e-8), it64, "fp32 cycle", first32.get(1e-8), it32, "margin", margin(it64),
                  "factor per cycle", rel64 ** (1.0 / it64), "x, fp32 against fp64 cycle", _relerr(x32, x64),
                  "true residuals", np.linalg.norm(b - S @ x64) / np.linalg.norm(b),
                  np.linalg.norm(b - S @ x32) / np.linalg.norm(b))
            assert st64 == CONVERGED and st32 == CONVERGED and it64 <= MAXIT and first64[1e-10] == it64
            assert np.linalg.norm(b - S @ x64) <= 1e-10 * (1 + 1e-6) * np.linalg.norm(b)
            assert np.linalg.norm(b - S @ x32) <= 1e-10 * (1 + 1e-6) * np.linalg.norm(b)
            assert abs(it32 - it64) <= margin(it64), (it32, it64)
            assert abs(first32[1e-8] - first64[1e-8]) <= margin(first64[1e-8]), (first32, first64)
            if not cheb and nu == 1 and (name, nu) in TABLE:
                assert abs(first64[1e-8] - TABLE[name, nu][0]) <= 1 and abs(it64 - TABLE[name, nu][1]) <= 1
            if not cheb and (name, nu) in TABLE:
                print("   the table:", TABLE[name, nu])
    if name == ONE:
        assert _np_run(name, matrix_path)[1] == 1


# ------------------------------------------------------------------------------------ on the GPU
_PERSISTENT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import lsbench_amd as la
assert la.hip_cdna4_init() == 0
la.Solver(la.lsbench_matrix_synth("lap2d:nx=20,ny=20"),
          la.default_opts(precond=la.PRECOND_AMG, krylov=la.KRYLOV_RICHARDSON, persistent=1))
"""


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")


def _kw(hip, cheb=0, f32=0, nu=1, **kw):
    kw.update(amg_sweeps=nu, amg_smoother=hip.AMG_SMOOTH_CHEB if cheb else hip.AMG_SMOOTH_L1JACOBI,
              amg_precision=hip.AMG_PREC_FP32 if f32 else hip.AMG_PREC_FP64)
    return kw


def _solver(hip, name, matrix_path, **kw):
    """a Richardson solver on the operator the numpy side uses, as read"""
    kw.setdefault("op_mode", hip.OP_RAW)
    kw.setdefault("krylov", hip.KRYLOV_RICHARDSON)
    return hip.Solver(as_matrix(_op(name, matrix_path)), hip.default_opts(precond=hip.PRECOND_AMG, **kw))


def _solve_dev(s, b, d_x=None):
    """(x, result) of solve_dev into an x pre-filled with NaN"""
    d_x = _nan(len(b)) if d_x is None else d_x
    res = s.solve_dev(_dev(b), d_x)
    return d_x.cpu().numpy(), res


def _replay(s, b, cycles):
    """the iteration driven from torch through the solver's public entry points: {k: (x_k, ||r_k|| / ||b||)}"""
    import torch
    d_b = _dev(b)
    x, r = torch.zeros_like(d_b), d_b.clone()
    out = {}
    for k in range(1, cycles + 1):
        z, q = _nan(len(b)), _nan(len(b))
        s.precond_dev(r, z)
        s.spmv_dev(z, q)
        x = x + z
        r = r - q
        out[k] = (x.cpu().numpy(), float(np.linalg.norm(r.cpu().numpy()) / np.linalg.norm(b)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("cheb", [0, 1])
@pytest.mark.parametrize("name", OPS)
def test_replay_bit_for_bit(hip, name, cheb, f32, nu, matrix_path):
    b = O.rhs(_op(name, matrix_path).shape[0])
    want = None
    for N in (5, 2, 1):
        s = _solver(hip, name, matrix_path, tol=0.0, maxit=N, **_kw(hip, cheb, f32, nu))
        assert s.iteration_bytes == 0
        if want is None:
            want = _replay(s, b, 5)
        x, res = _solve_dev(s, b)
        s.destroy()
        print(name, "cheb", cheb, "f32", f32, "nu", nu, "cycles", N, "relres", res.relres, "the replay's", want[N][1])
        assert (res.status, res.iters, res.spmvs) == (hip.STATUS_MAXIT, N, N)
        assert np.isfinite(x).all()
        assert x.tobytes() == want[N][0].tobytes()
        assert abs(res.relres - want[N][1]) <= 1e-12 * want[N][1]


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("name", OPS)
def test_against_numpy(hip, name, nu, matrix_path):
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    xr, itr, _, _, first, kept = _np_run(name, matrix_path, False, False, nu)
    s = _solver(hip, name, matrix_path, tol=0.0, maxit=5, **_kw(hip, nu=nu))
    x5, res = _solve_dev(s, b)
    s.destroy()
    if 5 in kept:
        print(name, "nu", nu, "x after 5 cycles against numpy's", _relerr(x5, kept[5]))
        assert res.iters == 5 and _relerr(x5, kept[5]) <= 1e-12
    else:
        assert name == ONE and itr == 1
    for tol in (1e-8, 1e-10):
        s = _solver(hip, name, matrix_path, tol=tol, maxit=MAXIT, **_kw(hip, nu=nu))
        x, res = _solve_dev(s, b)
        s.destroy()
        true = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
        print(name, "nu", nu, "tol", tol, "cycles", res.iters, "numpy's", first[tol], "relres", res.relres,
              "recomputed on the CPU", true, "factor per cycle", res.relres ** (1.0 / res.iters))
        assert res.status == hip.STATUS_CONVERGED and res.spmvs == res.iters
        assert abs(int(res.iters) - first[tol]) <= 1
        assert true <= tol * (1 + 1e-6)


@pytest.mark.gpu
def test_golden_solution(hip, matrix_path, golden_x):
    b = O.rhs(_op(XN3B, matrix_path).shape[0])
    s = _solver(hip, XN3B, matrix_path, tol=1e-12, maxit=MAXIT, **_kw(hip, nu=2))
    x, res = _solve_dev(s, b)
    s.destroy()
    print("cycles", res.iters, "relres", res.relres, "against the golden x", _relerr(x, golden_x(XN3B)))
    assert res.status == hip.STATUS_CONVERGED and _relerr(x, golden_x(XN3B)) <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name,cheb,f32", [(XN3B, 0, 0), (LAP2D, 1, 1), (POWERLAW, 0, 1), (ONE, 0, 0), (LAP3D, 1, 0)])
def test_same_bits_same_counts(hip, name, cheb, f32, matrix_path):
    """graphs or plain launches, a second solve, any poll interval, the one-launch tail, an x that is only 8-byte
    aligned: the same x, cycle count and relres"""
    n = _op(name, matrix_path).shape[0]
    b = O.rhs(n)
    base = dict(tol=1e-8, maxit=MAXIT, **_kw(hip, cheb, f32))
    got = []
    for extra in (dict(use_graph=1), dict(use_graph=0), dict(check_every=1), dict(check_every=3),
                  dict(use_graph=0, check_every=3), dict(amg_tail_rows=1 << 30)):
        s = _solver(hip, name, matrix_path, **dict(base, **extra))
        assert not s.padded
        x, res = _solve_dev(s, b)
        x2, res2 = _solve_dev(s, b)  # (the hinted solve)
        # x 8 bytes past a 16-byte boundary: the 8-byte form of the sweeps
        buf = _nan(n + 3)
        off = 1 if buf.data_ptr() % 16 == 0 else 0
        assert (buf.data_ptr() + 8 * off) % 16 == 8
        x3, res3 = _solve_dev(s, b, buf[off:off + n])
        around = buf.cpu().numpy()
        assert np.isnan(around[:off]).all() and np.isnan(around[off + n:]).all()  # nothing written beside it
        s.destroy()
        for xx, rr in ((x2, res2), (x3, res3)):
            assert xx.tobytes() == x.tobytes()
            assert (rr.status, rr.iters, rr.spmvs, rr.relres) == (res.status, res.iters, res.spmvs, res.relres)
        got.append((x, res))
    print(name, "cheb", cheb, "f32", f32, "cycles", got[0][1].iters, "relres", got[0][1].relres)
    assert got[0][1].status == hip.STATUS_CONVERGED
    for x, res in got[1:]:
        assert x.tobytes() == got[0][0].tobytes()
        assert (res.status, res.iters, res.spmvs, res.relres) == (got[0][1].status, got[0][1].iters, got[0][1].spmvs,
                                                                  got[0][1].relres)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_stop_rules(hip, graph, matrix_path):
    n = _op(LAP2D, matrix_path).shape[0]
    b = O.rhs(n)
    itr = _np_run(LAP2D, matrix_path)[4][1e-8]
    # a maxit below convergence; x is the iterate of that cycle
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=itr - 10, use_graph=graph)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters, res.spmvs) == (hip.STATUS_MAXIT, itr - 10, itr - 10) and res.relres > 1e-8
    # x stops where the state does: CONVERGED at cycle k leaves x_k, whatever was enqueued behind it
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=MAXIT, use_graph=graph, check_every=7)
    x, res = _solve_dev(s, b)
    s.destroy()
    s = _solver(hip, LAP2D, matrix_path, tol=0.0, maxit=int(res.iters), use_graph=graph)
    xk, resk = _solve_dev(s, b)
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED and resk.status == hip.STATUS_MAXIT
    assert x.tobytes() == xk.tobytes() and res.relres == resk.relres
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=MAXIT, use_graph=graph)
    # b = 0: x = 0, no cycle
    x, res = _solve_dev(s, np.zeros(n))
    assert (res.status, res.iters, res.spmvs, res.relres) == (hip.STATUS_CONVERGED, 0, 0, 0.0) and not x.any()
    # a NaN in b: BREAKDOWN within one chunk, and the call returns
    bad = b.copy()
    bad[n // 2] = float("nan")
    x, res = _solve_dev(s, bad)
    assert res.status == hip.STATUS_BREAKDOWN and res.iters == 1
    # ... and the solver is as good as before
    x, res = _solve_dev(s, b)
    s.destroy()
    assert res.status == hip.STATUS_CONVERGED and abs(int(res.iters) - itr) <= 1
    # maxit = 0: nothing to do
    s = _solver(hip, LAP2D, matrix_path, tol=1e-8, maxit=0, use_graph=graph)
    x, res = _solve_dev(s, b)
    s.destroy()
    assert (res.status, res.iters) == (hip.STATUS_MAXIT, 0) and not x.any()


@pytest.mark.gpu
@pytest.mark.parametrize("cheb", [0, 1])
@pytest.mark.parametrize("name", OPS)
def test_fp32_cycle(hip, name, cheb, matrix_path):
    S = _op(name, matrix_path)
    H, _ = _hier(name, matrix_path)
    n = S.shape[0]
    b = O.rhs(n)
    out = {}
    for f32 in (0, 1):
        s = _solver(hip, name, matrix_path, tol=1e-10, maxit=MAXIT, **_kw(hip, cheb, f32))
        assert s.amg_precision == f32
        z = _nan(n)
        s.precond_dev(_dev(b), z)  # the first z of the solve
        x, res = _solve_dev(s, b)
        s.destroy()
        assert res.status == hip.STATUS_CONVERGED
        out[f32] = (x, res, z.cpu().numpy())
    (x64, r64, z64), (x32, r32, z32) = out[0], out[1]
    true = np.linalg.norm(b - S @ x32) / np.linalg.norm(b)
    print(name, "cheb", cheb, "cycles fp32 cycle", r32.iters, "fp64 cycle", r64.iters, "margin", margin(r64.iters),
          "recomputed on the CPU", true, "x against the fp64 cycle's", _relerr(x32, x64))
    assert true <= 1e-10 * (1 + 1e-6)
    assert abs(int(r32.iters) - int(r64.iters)) <= margin(r64.iters)
    assert _relerr(x32, x64) <= 1e-8
    if len(H.A) > 1:
        assert z32.tobytes() != z64.tobytes()
    else:
        assert name == ONE


@pytest.mark.gpu
def test_renumbered_solvers(hip, monkeypatch):
    ri = dict(op_mode=hip.OP_RAW, precond=hip.PRECOND_AMG, krylov=hip.KRYLOV_RICHARDSON, tol=1e-12, maxit=MAXIT)
    A = hip.lsbench_matrix_synth("lap2d:nx=60,ny=50")
    b = O.rhs(A.nrows)
    xs = {}
    for ro in (0, 1):
        s = hip.Solver(A, hip.default_opts(reorder=ro, **ri))
        x, r = _solve_dev(s, b)
        s.destroy()
        assert r.status == 1 and np.isfinite(x).all()
        xs[ro] = x
    assert np.linalg.norm(xs[1] - xs[0]) <= 1e-10 * np.linalg.norm(xs[0])
    # lines of 2050 rows padded to whole slices against the unpadded solve
    A = hip.lsbench_matrix_synth("lap2d:nx=2050,ny=12")
    b = O.rhs(A.nrows)
    out = {}
    for pad in ("0", "1"):
        monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", pad)
        s = hip.Solver(A, hip.default_opts(**ri))
        assert bool(s.padded) == (pad == "1") and s.n_local == A.nrows
        x, r = _solve_dev(s, b)
        s.destroy()
        print("padded", pad, "cycles", r.iters)
        assert r.status == 1 and np.isfinite(x).all()
        out[pad] = x
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    assert np.linalg.norm(out["1"] - out["0"]) <= 1e-10 * np.linalg.norm(out["0"])


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
def test_verify(hip, f32, matrix_path):
    name, tol = LAP2D, 1e-12
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    s = _solver(hip, name, matrix_path, tol=tol, maxit=MAXIT, verify=1, **_kw(hip, 0, f32, 2))
    x, r = _solve_dev(s, b)
    s.destroy()
    print("cycles", r.iters, "products", r.spmvs, "corrections", r.corrections, "true_relres", r.true_relres,
          "on the CPU", np.linalg.norm(b - S @ x) / np.linalg.norm(b))
    assert r.status == hip.STATUS_CONVERGED and 0.0 <= r.true_relres <= tol and r.corrections <= 6
    assert r.spmvs == r.iters + r.corrections + 1 and r.relres == r.true_relres


@pytest.mark.gpu
def test_refusals_and_the_driver(hip, matrix_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    n = _op(XN3B, matrix_path).shape[0]
    s = _solver(hip, XN3B, matrix_path)
    d_B = _dev(np.tile(O.rhs(n), (2, 1)))
    d_X = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_spmm_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all())
    assert s.iteration_bytes == 0 and s.amg_cycle_bytes > 0
    s.destroy()
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    base = [drv, "--solver", "hip", "--matrix", matrix_path(XN3B), "--krylov", "richardson", "--trials=1"]
    for more in (["--precond", "jacobi"], ["--precond", "amg", "--nvirt", "2"], []):
        rc = subprocess.run(base + more, capture_output=True, text=True)
        assert rc.returncode != 0 and "richardson" in rc.stderr, (more, rc.stderr)
    # the persistent form is refused at creation too (the library exits: a child process)
    rc = subprocess.run([sys.executable, "-c", _PERSISTENT, ROOT], capture_output=True, text=True)
    assert rc.returncode != 0 and "richardson" in rc.stderr, rc.stderr
    rc = subprocess.run([drv, "--solver", "hip", "--matrix", matrix_path(XN3B), "--precond", "amg", "--krylov",
                         "richardson", "--maxit", "2", "--tol", "0", "--trials=3"], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rec = rc.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[0]) == 2 and int(f[2]) == 3
    rc = subprocess.run([drv, "--solver", "hip", "--matrix", matrix_path(XN3B), "--precond", "amg", "--krylov",
                         "gmres", "--trials=1"], capture_output=True, text=True)
    assert rc.returncode != 0 and "classic PCG" in rc.stderr
