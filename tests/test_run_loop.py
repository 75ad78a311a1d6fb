"""The host loop the iteration drivers share (hip_run.c: run_loop, the graph cache, the chunk rule), through the public
API only: PCG in three of its forms, BiCGSTAB, Richardson and the batch of right-hand sides.

How the host feeds the device -- captured graphs or plain launches, any poll interval, a hint from the previous solve
that is right, too long or too short -- must not show in the answer: the device decides when to stop, and what is
enqueued behind the stop are no-op launches.  So every variation gives the bytes of x and the (status, iterations,
products) of a fresh solver with default options.

The right-hand sides.  b1 is O.rhs (b_i = i; the batch: five envelopes of it).  b2 is built to stop after a handful of
iterations: a sum of three eigenvectors of D^-1 S -- product sines on the grids, scipy's eigsh / eigs elsewhere -- so a
Krylov method is done in three steps (BiCGSTAB: the real part of one complex pair, two steps).  A default poll interval
is at most 50 iterations (300 us of work over a floor of 6 us per iteration; BiCGSTAB 25), and b1 takes 95 - 200, so
the counts of b1 and b2 differ by more than one interval in each direction: a hint too long leaves more than a chunk
of no-op launches, a hint too short is followed by more than one chunk.

Two drivers cannot have that spread, and assert only that the counts differ (the hint is wrong in each direction):
  - Richardson on lap2d:nx=130,ny=70 takes 51 cycles on b_i = i and 52 on the smoothest mode, the slowest there is
    (a stationary iteration: the count follows the contraction factor, not b), and 18 on a checkerboard;
  - AMG-PCG of the batch on xn3b_A_18 takes 87 iterations on b1 and 49 on this b2 (eigenvectors of D^-1 S, not of
    M^-1 S: they are not easy for it), and no vector is known that it solves in fewer than 37.
"""
import numpy as np
import pytest

from oracle import oracle as O

TUNE = 6 | 64 | 256  # 16-bit codes, templates, the z-column walk (test_col_cache.py)
NCOL = 5
CHUNK = 50           # no default poll interval is longer

# case -> (operator, what it adds to the default options, a batch?, the spread of counts between b1 and b2 is asserted)
CASES = {
    "pcg": ("lap2d:nx=37,ny=23", dict(), False, True),
    "pcg1": ("lap2d:nx=37,ny=23", dict(krylov="KRYLOV_PCG1"), False, True),
    "col": ("lap3d:nx=128,ny=64,nz=21", dict(spmv_variant="SPMV_SELL", spmv_tune=TUNE), False, True),
    "bicgstab": ("lap2d:nx=60,ny=45,conv=0.6", dict(krylov="KRYLOV_BICGSTAB"), False, True),
    "richardson": ("lap2d:nx=130,ny=70", dict(precond="PRECOND_AMG", krylov="KRYLOV_RICHARDSON"), False, False),
    "multi-jacobi": ("xn3b_A_18", dict(), True, True),
    "multi-amg": ("xn3b_A_18", dict(precond="PRECOND_AMG"), True, False),
}
VARIATIONS = ([dict(use_graph=1), dict(use_graph=0)] + [dict(check_every=c) for c in (1, 2, 3, 7)] +
              [dict(check_every=c, use_graph=0) for c in (1, 2, 3, 7)])

_MATRIX, _RHS, _REF = {}, {}, {}


def _matrix(hip, case, matrix_path):
    name = CASES[case][0]
    if name not in _MATRIX:
        _MATRIX[name] = hip.lsbench_matrix_synth(name) if ":" in name else hip.lsbench_matrix_read(matrix_path(name))
    return _MATRIX[name]


def _grid_modes(dims):
    """the sum of three eigenvectors of the Dirichlet Laplacian on a grid (x fastest): products of sines"""
    out = 0.0
    for k in (1, 2, 3):
        v = np.ones(1)
        for m in reversed(dims):
            v = np.outer(v, np.sin(np.pi * k * np.arange(1, m + 1) / (m + 1))).ravel()
        out = out + v
    return out


def _rhs(hip, case, matrix_path):
    """(b1, b2), read-only; a batch: (n, NCOL) each"""
    if case in _RHS:
        return _RHS[case]
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    name, _, batch, _ = CASES[case]
    A = _matrix(hip, case, matrix_path)
    n = A.nrows
    i = np.arange(n, dtype=np.float64)
    if batch:
        Ao = O.matrix_read(matrix_path(name))
        S = O.operator_upper(Ao)
        S = sp.csr_matrix((S.vals, S.cols, S.offs), shape=(n, n))
        d = S.diagonal()
        Dh = sp.diags(1.0 / np.sqrt(d))
        _, v = spl.eigsh((Dh @ S @ Dh).tocsr(), k=NCOL + 2, which="LA", tol=0, v0=np.ones(n))
        v = np.sqrt(d)[:, None] * v
        b1 = np.stack([O.rhs(n), O.rhs(n) * np.where(i % 2 == 0, 1.0, -1.0), np.sin(i) + 0.5, np.ones(n),
                       O.rhs(n) * np.sin(np.pi * (i + 1) / (n + 1))], axis=1)
        b2 = np.stack([v[:, c] + v[:, c + 1] + v[:, c + 2] for c in range(NCOL)], axis=1)
    elif case == "bicgstab":
        S = sp.csr_matrix((A.vals, A.cols, A.offs), shape=(n, n))
        _, v = spl.eigs(sp.diags(1.0 / S.diagonal()) @ S, k=2, which="LR", tol=0, v0=np.ones(n))
        b1, b2 = O.rhs(n), S.diagonal() * v[:, 0].real
    elif case == "richardson":
        b1, b2 = O.rhs(n), np.array([(-1.0) ** (k % 130 + k // 130) for k in range(n)])
    else:
        dims = [int(kv.split("=")[1]) for kv in name.split(":")[1].split(",")]
        b1, b2 = O.rhs(n), _grid_modes(dims)
    b1, b2 = np.ascontiguousarray(b1), np.ascontiguousarray(b2)
    b1.setflags(write=False), b2.setflags(write=False)
    _RHS[case] = (b1, b2)
    return _RHS[case]


def _solver(hip, case, matrix_path, monkeypatch, **kw):
    name, extra, _, _ = CASES[case]
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1")
    monkeypatch.delenv("LSBENCH_HIP_COL_K", raising=False)
    opts = dict(tol=1e-8)
    if ":" in name:
        opts["op_mode"] = hip.OP_RAW
    opts.update({k: getattr(hip, v) if isinstance(v, str) else v for k, v in extra.items()})
    opts.update(kw)
    s = hip.Solver(_matrix(hip, case, matrix_path), hip.default_opts(**opts))
    if case == "col":
        assert s.fused_p == 2
    return s


def _solve(s, case, b):
    """(the bytes of x, ((status, iters, spmvs), ...) one per column) of a solve into an x pre-filled with NaN"""
    import torch
    d_b = torch.from_numpy(np.array(b.T if CASES[case][2] else b, order="C")).to("cuda:0")
    d_x = torch.full_like(d_b, float("nan"))
    res = s.solve_multi_dev(d_b, d_x) if CASES[case][2] else [s.solve_dev(d_b, d_x)]
    return d_x.cpu().numpy().tobytes(), tuple((int(r.status), int(r.iters), int(r.spmvs)) for r in res)


def _reference(hip, case, which, matrix_path, monkeypatch):
    """a fresh solver with default options at tol 1e-8 on b1 (which = 0) or b2 (1): made once, never changed"""
    if (case, which) not in _REF:
        s = _solver(hip, case, matrix_path, monkeypatch)
        _REF[case, which] = _solve(s, case, _rhs(hip, case, matrix_path)[which])
        s.destroy()
        assert all(st == hip.STATUS_CONVERGED for st, _, _ in _REF[case, which][1])
    return _REF[case, which]


def _count(ref):
    """what the batch's hint counts is its longest column"""
    return max(it for _, it, _ in ref[1])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", VARIATIONS, ids=lambda e: ",".join("%s=%d" % kv for kv in sorted(e.items())))
@pytest.mark.parametrize("case", list(CASES))
def test_graphs_and_poll_intervals_leave_no_trace(hip, case, extra, matrix_path, monkeypatch):
    b = _rhs(hip, case, matrix_path)[0]
    ref = _reference(hip, case, 0, matrix_path, monkeypatch)
    s = _solver(hip, case, matrix_path, monkeypatch, **extra)
    first, second = _solve(s, case, b), _solve(s, case, b)  # (the second: hinted)
    s.destroy()
    print(case, extra, ref[1], first[1], second[1])
    assert first[1] == ref[1] and second[1] == ref[1]
    assert first[0] == ref[0] and second[0] == ref[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_hint_too_long_and_too_short(hip, case, matrix_path, monkeypatch):
    b = _rhs(hip, case, matrix_path)
    ref = [_reference(hip, case, w, matrix_path, monkeypatch) for w in (0, 1)]
    n1, n2 = _count(ref[0]), _count(ref[1])
    print(case, "iterations of b1", n1, "of b2", n2)
    if CASES[case][3]:
        assert n1 - n2 > CHUNK
    else:
        assert n1 != n2
    s = _solver(hip, case, matrix_path, monkeypatch)
    for w in (0, 1, 0):
        got = _solve(s, case, b[w])
        assert got[1] == ref[w][1]
        assert got[0] == ref[w][0]
    s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_maxit_below_the_count(hip, case, matrix_path, monkeypatch):
    """with no previous solve (chunks) and behind one (the hint is maxit): MAXIT at maxit"""
    b = _rhs(hip, case, matrix_path)[0]
    ref = _reference(hip, case, 0, matrix_path, monkeypatch)
    maxit = min(it for _, it, _ in ref[1]) - 3
    assert maxit > 0
    s = _solver(hip, case, matrix_path, monkeypatch, maxit=maxit)
    first, second = _solve(s, case, b), _solve(s, case, b)
    s.destroy()
    for got in (first, second):
        assert [(st, it) for st, it, _ in got[1]] == [(hip.STATUS_MAXIT, maxit)] * len(ref[1])
    assert first == second
