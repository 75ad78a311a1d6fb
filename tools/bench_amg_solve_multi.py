#!/usr/bin/env python3
"""AMG as the solver on blocks of right-hand sides (amg_solve_multi_dev) against its single solve on one MI355X.

The premise under test: a stationary V-cycle iteration is streams of the hierarchy's matrices, one product with S and
six vector passes, so a block of columns, which reads each matrix once for all of them, should solve more columns per
second than single solves -- on a large grid in proportion to the matrix bytes shared, on a launch-bound matrix
because the launches are shared.  Per operator and protocol, in ONE process on ONE solver, `--reps` (5) times
alternating between the widths
  1             solve_dev on one column: the single solve, the yardstick
  2, 4, 8       amg_solve_multi_dev on a block of that many columns (b_i = i + c in column c)
under the protocols of the reference's AMG backends
  hypre         tol 0, maxit 2, l1-Jacobi, the cycle in fp64 (src/hypre.c:185-186)
  amgx          tol 0, maxit 1, l1-Jacobi, the cycle in fp32 (src/amgx.c:78-85)
`--solves` calls per repetition and width after `--warm` untimed ones (ten times as many on an operator of fewer than
100 000 rows, whose solve is a few dozen microseconds), device buffers, a host clock around work that ends in a device
synchronise.  One JSON line on stdout: per operator, protocol and width
  columns_per_s   median, min, max over the repetitions: columns solved per second
  us_per_cycle    likewise: time of a block over its cycles
  cycle_gb_s      lsb_hip_solver_amg_solve_multi_bytes over the cycle time, likewise
  x_single        columns_per_s over width 1's: [slowest over fastest, median over median, fastest over slowest]
  gain            the width's slowest repetition solves more columns per second than the fastest repetition of width 1
Progress goes to stderr.  Run it twice, in fresh processes.

Usage: python tools/bench_amg_solve_multi.py [--operators lap2d:nx=3162,ny=3162,xn3b_A_18] [--reps 5] [--solves 20]
                                             [--warm 5]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_direct import file_matrix  # noqa: E402

WIDTHS = (1, 2, 4, 8)


def operators(text):
    """a comma-separated list in which a synthetic spec carries commas of its own: split before every name"""
    return [s for s in re.split(r",(?=[A-Za-z0-9_]+(?::|$|,))", text) if s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", default="lap2d:nx=3162,ny=3162,xn3b_A_18")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    import torch

    import lsbench_amd as la
    assert la.hip_cdna4_init() == 0, "needs an MI355X"

    def stats(v):
        v = np.array(v)
        return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}

    out = {}
    with tempfile.TemporaryDirectory(prefix="lsb_amg_solve_multi_") as tmp:
        for name in operators(a.operators):
            synth = ":" in name
            A = la.lsbench_matrix_synth(name) if synth else file_matrix(la, name, tmp)
            n = A.nrows
            small = n < 100000
            solves, warm = (10 * a.solves, 10 * a.warm) if small else (a.solves, a.warm)
            B = np.stack([np.arange(n, dtype=np.float64) + c for c in range(max(WIDTHS))])
            d_B = torch.from_numpy(B).to("cuda:0")
            d_X = torch.zeros_like(d_B)
            base = dict(krylov=la.KRYLOV_RICHARDSON, precond=la.PRECOND_AMG, amg_smoother=la.AMG_SMOOTH_L1JACOBI,
                        tol=0.0)
            if synth:
                base["op_mode"] = la.OP_RAW
            protocols = {"hypre": dict(maxit=2, amg_precision=la.AMG_PREC_FP64),
                         "amgx": dict(maxit=1, amg_precision=la.AMG_PREC_FP32)}
            res = {}
            for p, kw in protocols.items():
                t0 = time.perf_counter()
                s = la.Solver(A, la.default_opts(**dict(base, **kw)))
                setup = time.perf_counter() - t0

                def block(k):
                    if k == 1:
                        return [s.solve_dev(d_B[0], d_X[0])]
                    return s.amg_solve_multi_dev(d_B[:k], d_X[:k])

                rec = {}
                for k in WIDTHS:
                    for _ in range(warm):
                        r = block(k)
                    torch.cuda.synchronize()
                    assert all(int(q.iters) == kw["maxit"] and q.status == la.STATUS_MAXIT for q in r)
                    rec[k] = {"t": [], "cycles": kw["maxit"], "relres": max(float(q.relres) for q in r),
                              "cycle_bytes": s.amg_solve_multi_bytes(k)}
                    print(name, p, "width", k, "relres", rec[k]["relres"], file=sys.stderr, flush=True)
                for rep in range(a.reps):
                    for k in WIDTHS:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(solves):
                            block(k)
                        torch.cuda.synchronize()
                        rec[k]["t"].append((time.perf_counter() - t0) / solves)
                    print(name, p, "rep", rep, {k: "%.0f columns/s" % (k / rec[k]["t"][-1]) for k in WIDTHS},
                          file=sys.stderr, flush=True)
                res[p] = {"setup_s": round(setup, 2), "levels": s.amg_info[0], "amg_cycle_bytes": s.amg_cycle_bytes,
                          "solves": solves, "warm": warm}
                one = np.array(rec[1]["t"])
                for k in WIDTHS:
                    t = np.array(rec[k].pop("t"))
                    cyc = t / rec[k]["cycles"]
                    res[p][str(k)] = dict(rec[k], columns_per_s=stats(k / t), us_per_cycle=stats(1e6 * cyc),
                                          cycle_gb_s=stats(1e-9 * rec[k]["cycle_bytes"] / cyc),
                                          x_single=[float(k / t.max() * one.min()),
                                                    float(k / np.median(t) * np.median(one)),
                                                    float(k / t.min() * one.max())],
                                          gain=bool(k > 1 and k / t.max() > 1.0 / one.min()))
                s.destroy()
            out[name] = dict(n=n, nnz=int(A.nnz), protocols=res)
    print(json.dumps({"bench": "amg_solve_multi", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                      "solves": a.solves, "warm": a.warm, "operators": out}))


if __name__ == "__main__":
    main()
