#!/usr/bin/env python3
"""The direct solver on blocks of right-hand sides (solve_direct_multi_dev) against its single solve on one MI355X.

The premise under test: if the latency of the row records and the stream of W dominate a direct solve, a block of 8
columns should cost little more than one column.  Per operator and protocol, in ONE process on ONE solver, `--reps` (5)
times alternating between the widths
  1             solve_dev on one column: the single solve, the yardstick
  2, 4, 8       solve_direct_multi_dev on a block of that many columns (b_i = i + c in column c)
under the protocols
  direct_1      tol 0, maxit 1 (one round, nothing recomputed: the reference's protocol, src/cholmod-impl.h:59-62)
  direct_tol    --tol (1e-10): rounds until the recomputed residual of every column meets it
`--solves` (200) calls per repetition and width after `--warm` (20) untimed ones, device buffers, a host clock around
work that ends in a device synchronise.  One JSON line on stdout: per operator, protocol and width
  columns_per_s   [min, max] over the repetitions: columns solved per second
  us_per_block    [min, max]
  round_gb_s      lsb_hip_solver_direct_multi_round_bytes x rounds over the time, [min, max]
  x_single        columns_per_s over width 1's, [slowest over fastest, fastest over slowest]
  gain            the width's slowest repetition solves more columns per second than the fastest repetition of width 1
Progress goes to stderr.

Usage: python tools/bench_direct_multi.py [--operators xn3b_A_18,tj7a_A_12] [--reps 5] [--solves 200] [--warm 20]
                                          [--tol 1e-10]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_direct import file_matrix  # noqa: E402

WIDTHS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", default="xn3b_A_18,tj7a_A_12")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-10)
    a = ap.parse_args()
    import torch

    import lsbench_amd as la
    assert la.hip_cdna4_init() == 0, "needs an MI355X"
    out = {}
    with tempfile.TemporaryDirectory(prefix="lsb_direct_multi_") as tmp:
        for name in a.operators.split(","):
            A = file_matrix(la, name, tmp)
            n = A.nrows
            B = np.stack([np.arange(n, dtype=np.float64) + c for c in range(max(WIDTHS))])
            d_B = torch.from_numpy(B).to("cuda:0")
            d_X = torch.zeros_like(d_B)
            protocols = {"direct_1": dict(tol=0.0, maxit=1), "direct_tol": dict(tol=a.tol)}
            res = {}
            for p, kw in protocols.items():
                s = la.Solver(A, la.default_opts(krylov=la.KRYLOV_DIRECT, **kw))

                def block(k):
                    if k == 1:
                        return [s.solve_dev(d_B[0], d_X[0])]
                    return s.solve_direct_multi_dev(d_B[:k], d_X[:k])

                rec = {}
                for k in WIDTHS:
                    for _ in range(a.warm):
                        r = block(k)
                    torch.cuda.synchronize()
                    rec[k] = {"t": [], "rounds": max(int(q.iters) for q in r), "status": [int(q.status) for q in r],
                              "relres": max(float(q.relres) for q in r), "round_bytes": s.direct_multi_round_bytes(k)}
                    print(name, p, "width", k, "rounds", rec[k]["rounds"], "status", rec[k]["status"], "relres",
                          rec[k]["relres"], file=sys.stderr, flush=True)
                for rep in range(a.reps):
                    for k in WIDTHS:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(a.solves):
                            block(k)
                        torch.cuda.synchronize()
                        rec[k]["t"].append((time.perf_counter() - t0) / a.solves)
                    print(name, p, "rep", rep, {k: "%.0f columns/s" % (k / rec[k]["t"][-1]) for k in WIDTHS},
                          file=sys.stderr, flush=True)
                res[p] = {}
                one = rec[1]["t"]
                for k in WIDTHS:
                    t = rec[k].pop("t")
                    gb = 1e-9 * rec[k]["round_bytes"] * rec[k]["rounds"]
                    res[p][str(k)] = dict(rec[k], columns_per_s=[k / max(t), k / min(t)],
                                          us_per_block=[1e6 * min(t), 1e6 * max(t)],
                                          round_gb_s=[gb / max(t), gb / min(t)],
                                          x_single=[(k / max(t)) * min(one), (k / min(t)) * max(one)],
                                          gain=bool(k > 1 and k / max(t) > 1.0 / min(one)))
                e, h, by = s.direct_info
                res[p]["entries"], res[p]["height"] = e, h
                s.destroy()
            out[name] = dict(n=n, nnz=int(A.nnz), protocols=res)
    print(json.dumps({"bench": "direct_multi", "reps": a.reps, "solves": a.solves, "warm": a.warm, "tol": a.tol,
                      "operators": out}))


if __name__ == "__main__":
    main()
