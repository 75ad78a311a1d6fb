"""The AMG V-cycle in fp32 inside fp64 PCG (opts.amg_precision = AMG_PREC_FP32, --amg-precision fp32).

The cycle is restated here in numpy on top of test_amg.Hier (`H32`): every matrix of the hierarchy, minv (or the
Chebyshev smoother's dinv) and the coarse inverse cast to float32, r rounded once, the recursion of Hier.vcycle (or
of test_amg_cheb.Cheb, with float32 coefficients) on float32 arrays -- scipy and numpy then sum in fp32 -- and z
widened at the end.  It rounds the same algorithm as the device in another summation order, so its error against
the fp64 cycle is the size the device's may have.

CPU: the options and symbols, lsb_csr_pack_f32 word for word, and what the GPU solves lean on (fp64 PCG around the
H32 cycle takes the iterations of PCG around the fp64 cycle).  GPU: one application against numpy, solves against
the fp64-cycle solver, verify, re-numbered solvers, the byte count, the refusals and the driver."""
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
from test_amg import Hier, as_matrix, operator, pcg
from test_amg_cheb import Cheb, cheb_coeffs

POWERLAW = "powerlaw:n=900,avg=9,max=300,seed=3,spd=1"
SYMBOLS = ("lsb_hip_solver_amg_precision", "lsb_hip_solver_amg_cycle_bytes", "lsb_csr_pack_f32")
# (operator, tol) of the solves; the first two are reference matrices with a golden solution
SOLVES = [("xn3b_A_18", 1e-12), ("tj7a_A_12", 1e-12), ("lap2d:nx=130,ny=70", 1e-10), ("lap3d:nx=24,ny=20,nz=18", 1e-10)]
CYCLES = ["xn3b_A_18", "lap2d:nx=130,ny=70", POWERLAW, "lap2d:nx=12,ny=10"]
F = np.float32


# ------------------------------------------------------------------------------------ the restatement
class H32:
    """The V-cycle of a test_amg.Hier in float32; cheb: a test_amg_cheb.Cheb of the same hierarchy, or None (l1-Jacobi)"""

    def __init__(self, H, cheb=None):
        self.A = [A.astype(F) for A in H.A]
        self.P = [P.astype(F) for P in H.P]
        self.R = [R.astype(F) for R in H.R]
        self.cinv = H.cinv.astype(F)
        self.minv = [m.astype(F) for m in H.minv]
        self.cheb = cheb
        if cheb is not None:
            self.dinv = [d.astype(F) for d in cheb.dinv]
        for M in self.A + self.P + self.R:
            assert M.dtype == F and np.isfinite(M.data).all()

    def _smooth(self, l, b, x, nu, pre):
        A = self.A[l]
        if self.cheb is None:
            m = self.minv[l]
            if pre:
                x = m * b
            for _ in range(nu - 1 if pre else nu):
                x = x + m * (b - A @ x)
            return x
        c1, c2 = cheb_coeffs(self.cheb.hi[l], self.cheb.ratio, nu)
        dinv, d = self.dinv[l], None
        for k in range(nu):
            r = b if (pre and k == 0) else b - A @ x
            m = F(c2[k]) * dinv
            d = m * r if c1[k] == 0.0 else F(c1[k]) * d + m * r
            x = d if (pre and k == 0) else x + d
        return x

    def vcycle(self, r, nu=1):
        def rec(l, b):
            if l == len(self.A) - 1:
                return self.cinv @ b
            x = self._smooth(l, b, None, nu, True)
            xc = rec(l + 1, self.R[l] @ (b - self.A[l] @ x))
            x = self._smooth(l, b, x + self.P[l] @ xc, nu, False)
            assert x.dtype == F
            return x
        return rec(0, r.astype(F)).astype(np.float64)


_CACHE = {}


def _op(name, matrix_path):
    if ("S", name) not in _CACHE:
        _CACHE[("S", name)] = operator(name, matrix_path)
    return _CACHE[("S", name)]


def _hier(name, matrix_path):
    """(Hier, Cheb at ratio 10) of an operator, made once"""
    if ("H", name) not in _CACHE:
        H = Hier(_op(name, matrix_path))
        _CACHE[("H", name)] = (H, Cheb(H, 10.0))
    return _CACHE[("H", name)]


def _cycles(name, matrix_path, cheb):
    """(the fp64 numpy cycle, the H32 cycle) as functions of (r, nu)"""
    H, Ch = _hier(name, matrix_path)
    key = ("H32", name, cheb)
    if key not in _CACHE:
        _CACHE[key] = H32(H, Ch if cheb else None)
    return (Ch.vcycle if cheb else H.vcycle), _CACHE[key].vcycle


def _relerr(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------ without a GPU
def test_surface():
    o = la.default_opts()
    assert o.amg_precision == 0 and (la.AMG_PREC_FP64, la.AMG_PREC_FP32) == (0, 1)
    names = [f[0] for f in _lib.Opts._fields_]  # between amg_tail_rows and amg_smoother, where five ints left a hole
    assert names[names.index("amg_tail_rows") + 1] == "amg_precision"
    assert _lib.Opts.amg_cheb_ratio.offset == _lib.Opts.amg_precision.offset + 8  # (no hole left, none made)
    lib = _lib.load()
    try:
        got = _lib.Opts()
        assert lib.hip_cdna4_set_option(b"amg-precision", b"fp32") == 0
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.amg_precision == 1
        assert lib.hip_cdna4_set_option(b"amg-precision", b"fp16") == 1
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.amg_precision == 1
        assert lib.hip_cdna4_set_option(b"amg-precision", b"fp64") == 0
        lib.lsb_hip_get_opts(C.byref(got))
        assert got.amg_precision == 0
    finally:
        lib.lsb_hip_set_opts(C.byref(o))
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    r = subprocess.run([drv, "--help"], capture_output=True, text=True)
    assert "--amg-precision" in r.stdout
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    assert "LSB_AMG_PREC_FP64 = 0" in header and "LSB_AMG_PREC_FP32 = 1" in header
    body = header[header.index("struct lsb_hip_opts {"):header.index("enum { LSB_PREC_FP64")]
    assert re.findall(r"^  (?:int|unsigned|double) (\w+);", body, re.M) == names  # the header's order is the mirror's
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name), name
    assert isinstance(la.Solver.amg_precision, property) and isinstance(la.Solver.amg_cycle_bytes, property)
    assert lib.lsb_hip_solver_amg_precision(None) == 2 and lib.lsb_hip_solver_amg_cycle_bytes(None) == 0


def _pack(M):
    lib = _lib.load()
    p = lib.lsb_csr_pack_f32(M.ptr)
    if not p:
        return None
    nnz = int(np.asarray(M.offs)[-1])
    w = np.ctypeslib.as_array(p, shape=(max(nnz, 1),)).astype(np.uint64, copy=True)[:nnz]
    _lib.libc_free(p)
    return w


def _words(cols0, vals):
    bits = np.asarray(vals, np.float64).astype(F).view(np.uint32).astype(np.uint64)
    return np.asarray(cols0, np.uint64) | (bits << np.uint64(32))


@pytest.mark.parametrize("name", ["xn3b_A_18", "lap2d:nx=130,ny=70,coef=7"])
def test_pack_f32(name, matrix_path):
    S = _op(name, matrix_path)
    w = _pack(as_matrix(S))
    assert w is not None and w.dtype == np.uint64 and len(w) == S.nnz
    assert np.array_equal(w, _words(S.indices, S.data))
    inexact = int((S.data.astype(F).astype(np.float64) != S.data).sum())
    print(name, S.nnz, "entries,", inexact, "of them round")
    if "coef" in name:
        assert inexact > S.nnz // 2
    # base = 1: the words hold 0-based columns
    w1 = _pack(la.Matrix.from_arrays(S.indptr, S.indices + 1, S.data, base=1))
    assert np.array_equal(w1, w)


def test_pack_f32_toy_and_refusals(matrix_path):
    A = la.lsbench_matrix_read(matrix_path("I1_05x05"))  # a file with base 1, no empty row
    assert A.base == 1
    w = _pack(A)
    assert np.array_equal(w, _words(np.asarray(A.cols) - 1, A.vals))
    assert np.array_equal(w & np.uint64(0xffffffff), np.arange(5, dtype=np.uint64))
    offs, cols = [0, 1, 2], [0, 1]
    assert _pack(la.Matrix.from_arrays(offs, cols, [1e39, 1e39])) is None
    assert _pack(la.Matrix.from_arrays(offs, cols, [1.0, -3.5e38])) is None  # rounds to -inf
    assert _pack(la.Matrix.from_arrays(offs, cols, [1.0, float("nan")])) is None
    assert _pack(la.Matrix.from_arrays(offs, cols, [1.0, float("inf")])) is None
    w = _pack(la.Matrix.from_arrays(offs, cols, [3.4e38, 1e-40]))  # the largest floats and subnormals are kept
    assert w is not None and np.array_equal(w, _words(cols, [3.4e38, 1e-40])) and (w[1] >> np.uint64(32)) != 0
    w = _pack(la.Matrix.from_arrays([0, 0, 0], [], []))  # no entry: still an allocation to free
    assert w is not None and len(w) == 0


@pytest.mark.parametrize("name,tol", SOLVES)
def test_cpu_precondition_pcg_takes_the_fp64_cycles_iterations(name, tol, matrix_path):
    """fp64 PCG around the H32 cycle against PCG around the fp64 cycle: the margin test_hip_amg_pcg_follows_numpy
    grants the device against numpy.  Measured: the same count in every case."""
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    r = np.sin(np.arange(S.shape[0], dtype=np.float64)) + 0.5
    for cheb in (False, True):
        v64, v32 = _cycles(name, matrix_path, cheb)
        for nu in (1, 2):
            x64, it64, st64 = pcg(S, b, lambda q: v64(q, nu), tol)
            x32, it32, st32 = pcg(S, b, lambda q: v32(q, nu), tol)
            print(name, "Chebyshev" if cheb else "l1-Jacobi", "nu", nu, "iterations fp64", it64, "fp32", it32,
                  "one application, fp32 against fp64:", _relerr(v32(r, nu), v64(r, nu)),
                  "true residual", np.linalg.norm(b - S @ x32) / np.linalg.norm(b))
            assert st64 == 1 and st32 == 1
            assert abs(it32 - it64) <= max(2, 0.04 * it64), (it32, it64)


# ------------------------------------------------------------------------------------ on the GPU
_BAD_PRECISION = r"""
import sys
sys.path.insert(0, sys.argv[1])
import lsbench_amd as la
assert la.hip_cdna4_init() == 0
la.Solver(la.lsbench_matrix_synth("lap2d:nx=20,ny=20"), la.default_opts(precond=la.PRECOND_AMG, amg_precision=2))
"""


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _solver(hip, name, matrix_path, **kw):
    """a solver on the operator the numpy side uses, as read"""
    kw.setdefault("op_mode", hip.OP_RAW)
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


@pytest.mark.gpu
@pytest.mark.parametrize("cheb", [0, 1])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("name", CYCLES)
def test_one_application_against_numpy(hip, name, nu, cheb, matrix_path):
    S = _op(name, matrix_path)
    H, _ = _hier(name, matrix_path)
    v64, v32 = _cycles(name, matrix_path, bool(cheb))
    r = np.sin(np.arange(S.shape[0], dtype=np.float64)) + 0.5
    kw = dict(amg_sweeps=nu, amg_smoother=hip.AMG_SMOOTH_CHEB if cheb else hip.AMG_SMOOTH_L1JACOBI)
    s = _solver(hip, name, matrix_path, amg_precision=hip.AMG_PREC_FP32, amg_tail_rows=1 << 30, **kw)
    assert s.amg_precision == 1 and s.amg_info == (len(H.A), 0)
    z = _apply(s, r)
    s.destroy()
    s = _solver(hip, name, matrix_path, **kw)
    assert s.amg_precision == 0 and s.amg_info[0] == len(H.A)
    zd = _apply(s, r)
    s.destroy()
    z64 = v64(r, nu)
    e_gpu, e_np = _relerr(z, z64), _relerr(v32(r, nu), z64)
    print(name, "nu", nu, "Chebyshev" if cheb else "l1-Jacobi", len(H.A), "levels: device fp32 against numpy fp64",
          e_gpu, "numpy fp32 against numpy fp64", e_np, "device fp64 against numpy fp64", _relerr(zd, z64))
    if len(H.A) > 1:
        assert z.tobytes() != zd.tobytes()
    else:
        assert name == "lap2d:nx=12,ny=10"
    assert e_gpu <= 4.0 * max(e_np, 2.0 ** -24)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("name,tol,nu,cheb", [(n, t, 1, 0) for n, t in SOLVES] + [("xn3b_A_18", 1e-12, 2, 1)])
def test_solves_follow_the_fp64_cycle(hip, name, tol, nu, cheb, graph, matrix_path, golden_x):
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    kw = dict(tol=tol, use_graph=graph, amg_sweeps=nu,
              amg_smoother=hip.AMG_SMOOTH_CHEB if cheb else hip.AMG_SMOOTH_L1JACOBI)
    s = _solver(hip, name, matrix_path, amg_precision=hip.AMG_PREC_FP32, **kw)
    x, r = s.solve(b)
    x2, r2 = s.solve(b)
    s.destroy()
    s = _solver(hip, name, matrix_path, **kw)
    x64, r64 = s.solve(b)
    s.destroy()
    print(name, "graph", graph, "nu", nu, "cheb", cheb, "iterations fp32 cycle", r.iters, "fp64 cycle", r64.iters,
          "relres", r.relres, "x against the fp64 cycle's", _relerr(x, x64))
    assert r.status == hip.STATUS_CONVERGED and r64.status == hip.STATUS_CONVERGED
    assert x.tobytes() == x2.tobytes() and r.iters == r2.iters
    assert abs(int(r.iters) - int(r64.iters)) <= max(2, 0.04 * r64.iters), (r.iters, r64.iters)
    if name in ("xn3b_A_18", "tj7a_A_12"):
        assert _relerr(x, golden_x(name)) <= 1e-10
    else:
        assert np.linalg.norm(x - x64) <= 1e-8 * np.linalg.norm(x64)
    s = _solver(hip, name, matrix_path, amg_precision=hip.AMG_PREC_FP32, maxit=5, **kw)
    x, r = s.solve(b)
    s.destroy()
    assert r.status == hip.STATUS_MAXIT and r.iters == 5


@pytest.mark.gpu
def test_verify(hip, matrix_path):
    """the restart on the recomputed residual around a cycle that is not gated"""
    name, tol = "xn3b_A_18", 1e-12
    S = _op(name, matrix_path)
    b = O.rhs(S.shape[0])
    s = _solver(hip, name, matrix_path, amg_precision=hip.AMG_PREC_FP32, tol=tol, verify=1)
    x, r = s.solve(b)
    s.destroy()
    print("iterations", r.iters, "corrections", r.corrections, "true_relres", r.true_relres, "on the CPU",
          np.linalg.norm(b - S @ x) / np.linalg.norm(b))
    assert r.status == hip.STATUS_CONVERGED and 0.0 <= r.true_relres <= tol and r.corrections <= 6


@pytest.mark.gpu
def test_renumbered_solvers(hip, monkeypatch):
    f32 = dict(op_mode=hip.OP_RAW, precond=hip.PRECOND_AMG, amg_precision=hip.AMG_PREC_FP32)
    A = hip.lsbench_matrix_synth("lap2d:nx=60,ny=50")
    b = O.rhs(A.nrows)
    xs = {}
    for ro in (0, 1):
        s = hip.Solver(A, hip.default_opts(reorder=ro, **f32))
        assert s.amg_precision == 1
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
        s = hip.Solver(A, hip.default_opts(tol=1e-12, **f32))
        assert bool(s.padded) == (pad == "1") and s.n_local == A.nrows
        x, r = s.solve(b)
        s.destroy()
        assert r.status == 1
        out[pad] = x
    monkeypatch.delenv("LSBENCH_HIP_PAD_LINES")
    assert np.linalg.norm(out["1"] - out["0"]) <= 1e-10 * np.linalg.norm(out["0"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["xn3b_A_18", "lap2d:nx=130,ny=70"])
def test_bytes(hip, name, matrix_path):
    """per level 8 M + 44 n against 12 M + 88 n at nu = 1 (M the entries streamed), the coarse inverse half; level 0
    adds 12 n for the two fp64 ends and the copy of r: less than 2/3 whatever the hierarchy"""
    for nu in (1, 2):
        for cheb in (0, 1):
            kw = dict(amg_sweeps=nu, amg_smoother=hip.AMG_SMOOTH_CHEB if cheb else hip.AMG_SMOOTH_L1JACOBI)
            s = _solver(hip, name, matrix_path, amg_precision=hip.AMG_PREC_FP32, **kw)
            b32 = s.amg_cycle_bytes
            s.destroy()
            s = _solver(hip, name, matrix_path, **kw)
            b64 = s.amg_cycle_bytes
            s.destroy()
            print(name, "nu", nu, "cheb", cheb, "bytes per application: fp32", b32, "fp64", b64, "ratio", b32 / b64)
            assert 0 < 3 * b32 < 2 * b64
    s = hip.Solver(as_matrix(_op(name, matrix_path)), hip.default_opts(op_mode=hip.OP_RAW))
    assert s.amg_cycle_bytes == 0 and s.amg_precision is None
    s.destroy()


@pytest.mark.gpu
def test_refusals_and_the_driver(hip, matrix_path, tmp_path):
    import torch
    from lsbench_amd.api import _ptr
    lib = _lib.load()
    name = "xn3b_A_18"
    n = _op(name, matrix_path).shape[0]
    s = _solver(hip, name, matrix_path, amg_precision=hip.AMG_PREC_FP32)
    d_B = _dev(np.tile(O.rhs(n), (2, 1)))
    d_X = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda:0")
    res = (_lib.Result * 2)()
    assert lib.lsb_hip_solver_solve_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n, res) == 2
    assert lib.lsb_hip_solver_spmm_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    assert lib.lsb_hip_solver_precond_multi_dev(s._h, 2, _ptr(d_B), n, _ptr(d_X), n) == 2
    torch.cuda.synchronize()
    assert bool((d_X == 7.0).all())
    s.destroy()
    # an explicit fp64 is the default solver, byte for byte
    r = np.sin(np.arange(n, dtype=np.float64)) + 0.5
    zs = []
    for kw in ({}, {"amg_precision": hip.AMG_PREC_FP64}):
        s = _solver(hip, name, matrix_path, **kw)
        zs.append(_apply(s, r))
        s.destroy()
    assert zs[0].tobytes() == zs[1].tobytes()
    # another integer is refused at creation, as an unknown smoother is (the library exits: a child process)
    rc = subprocess.run([sys.executable, "-c", _BAD_PRECISION, ROOT], capture_output=True, text=True)
    assert rc.returncode != 0 and "no AMG precision 2" in rc.stderr, rc.stderr
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    base = [drv, "--solver", "hip", "--precond", "amg", "--trials=1"]
    rc = subprocess.run(base + ["--matrix", matrix_path(name), "--amg-precision", "fp16"], capture_output=True, text=True)
    assert rc.returncode != 0
    big = tmp_path / "big_2x2.txt"
    big.write_text("2 0\n0 0 1e39\n1 1 1e39\n")
    rc = subprocess.run(base + ["--matrix", str(big), "--amg-precision", "fp32"], capture_output=True, text=True)
    assert rc.returncode != 0 and "fp32" in rc.stderr, rc.stderr
    rc = subprocess.run(base + ["--matrix", str(big)], capture_output=True, text=True)  # (fp64 serves it)
    assert rc.returncode == 0, rc.stderr
    rc = subprocess.run([drv, "--solver", "hip", "--matrix", matrix_path(name), "--precond", "amg", "--amg-precision",
                         "fp32", "--trials=3"], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr
    rec = rc.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[2]) == 1 and 0 < int(f[0]) < 267
