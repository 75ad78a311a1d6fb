"""Successive right-hand sides without a GPU: the C-ABI surface of lsb_hip_solver_seq_* / solve_seq[_dev], the Python
prototypes, struct lsb_hip_opts left alone, and the numpy model of seq_family.py pinned to the iteration counts it was
written down with -- the model is what tests/test_seq_solve.py compares the device with."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib
from seq_family import CONVERGED, SeqModel, pcg_from, rhs_3d, rhs_drift, run_model
from test_mrhs import _lap2d, oracle_operator

SYMBOLS = ("lsb_hip_solver_seq_begin", "lsb_hip_solver_solve_seq_dev", "lsb_hip_solver_solve_seq",
           "lsb_hip_solver_seq_info", "lsb_hip_solver_seq_basis_dev", "lsb_hip_solver_seq_last_us")
LAUNCHERS = ("lsb_k_seq_grid", "lsb_k_seq_dots", "lsb_k_seq_combine", "lsb_k_seq_orth", "lsb_k_seq_store")

# nine solves of the drifting family at tol 1e-10: the counts of a cold solve (lowest, highest, total) and of the
# sequence at depth 8; five solves of the three-dimensional family at depth 4
TABLE = {
    "xn3b_A_18": dict(cold=(233, 238, 2127), seq=[238, 224, 204, 168, 150, 137, 105, 81, 45], ratio=0.64,
                      three=[234, 234, 224, 6, 5]),
    "lap2d": dict(cold=(220, 224, 2014), seq=[223, 210, 197, 161, 150, 138, 102, 79, 50], ratio=0.65,
                  three=[222, 222, 212, 7, 7]),
}
START = [1.0, 1.3e-1, 1.2e-2, 5.1e-4, 6.2e-5, 7.5e-6, 6.5e-7, 3.8e-8, 1.1e-8]  # xn3b_A_18, as printed to two digits


@functools.lru_cache(maxsize=None)
def operator(name, path):
    return oracle_operator(path)[1].tocsr() if path else _lap2d(60, 50)


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "lsb_impl.h")) as f:
        impl = f.read()
    assert re.search(r"^#define LSB_SEQ_MAX_DEPTH 16$", header, re.M)
    assert la.SEQ_MAX_DEPTH == 16
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib.hip, name), name
    for name in LAUNCHERS:
        assert re.search(r"\b%s\(" % name, impl) and hasattr(lib.hip, name), name
    for m in ("seq_begin", "solve_seq", "solve_seq_dev", "seq_basis_dev"):
        assert callable(getattr(la.Solver, m)), m
    assert isinstance(la.Solver.seq_info, property)
    # before hip_cdna4_init the calls that would touch the device answer 1 ahead of any look at their arguments; on
    # a process that has initialised the backend the null arguments are what is refused: 2
    up = int(lib.hip.lsb_hip_is_initialized())
    res = _lib.Result()
    assert lib.lsb_hip_solver_seq_begin(None, 4) == (2 if up else 1)
    assert lib.lsb_hip_solver_solve_seq_dev(None, None, None, C.byref(res)) == (2 if up else 1)
    assert lib.lsb_hip_solver_solve_seq(None, None, None, C.byref(res)) == (2 if up else 1)
    assert lib.lsb_hip_solver_seq_basis_dev(None, 0, None, None) == (2 if up else 1)
    assert lib.lsb_hip_solver_seq_info(None, None, None, None, None) == 2


def test_the_options_struct_did_not_grow():
    """the depth is an argument of seq_begin, not an option"""
    assert list(_lib.Opts._TAIL) == ["fsai_blocks"]
    assert _lib.Opts._fields_[-1][0] == "amg_cheb_ratio"
    assert not [f for f, _ in _lib.Opts._fields_ if "seq" in f]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_model_reproduces_its_tables(name, matrix_path):
    """The counts the model was written down with, on this operator.  Exact: the sequences at depth 8 and on the
    three-dimensional family, their totals, the cold totals, the ratio to two digits.  The cold solves of the grid
    were written down as 220 .. 224, total 2012; numpy here gives 223 .. 224, total 2014 -- inside the range, the
    ratio rounds to the same 0.65, and 2014 is what is pinned."""
    S = operator(name, matrix_path(name) if name != "lap2d" else None)
    n, want = S.shape[0], TABLE[name]
    dinv = 1.0 / S.diagonal()
    cold = [pcg_from(S, dinv, rhs_drift(n, t), None, 1e-10)[2] for t in range(9)]
    iters, start, m = run_model(S, 8, 1e-10, rhs_drift, 9)
    print(name, "cold", cold, sum(cold), "depth 8", iters, sum(iters), "start", ["%.1e" % s for s in start],
          "orthonormal to", m.orthonormality())
    lo, hi, total = want["cold"]
    assert lo <= min(cold) and max(cold) <= hi
    assert sum(cold) == total
    assert iters == want["seq"]
    assert round(sum(iters) / sum(cold), 2) == want["ratio"]
    assert (m.held, m.restarts) == (1, 1)  # the ninth solve found the basis full
    m8 = run_model(S, 8, 1e-10, rhs_drift, 8)[2]
    assert (m8.held, m8.restarts) == (8, 0) and m8.orthonormality() <= 7e-16
    if name == "xn3b_A_18":
        assert ["%.1e" % s for s in start] == ["%.1e" % s for s in START]
    it3, _, m3 = run_model(S, 4, 1e-10, rhs_3d, 5)
    assert it3 == want["three"] and (m3.held, m3.restarts) == (1, 1)


def test_the_model_on_a_repeated_and_on_uncorrelated_right_hand_sides():
    """the same b twice at tol 1e-8: the second solve starts below tol and takes no iteration, the basis stays; six
    uncorrelated right-hand sides start at 1.0 and take a cold solve's iterations"""
    S = operator("lap2d", None)
    n = S.shape[0]
    m = SeqModel(S, 4, 1e-8)
    b = rhs_drift(n, 0)
    first, again = m.solve(b), m.solve(b)
    assert first["status"] == again["status"] == CONVERGED
    assert again["iters"] == 0 and again["start"] <= 1e-8 and m.held == 1
    m = SeqModel(S, 4, 1e-10)
    for t in range(6):
        b = np.random.default_rng(t).standard_normal(n)
        cold = pcg_from(S, 1.0 / S.diagonal(), b, None, 1e-10)[2]
        out = m.solve(b)
        assert abs(out["iters"] - cold) <= 0.05 * cold and out["start"] >= 0.99
