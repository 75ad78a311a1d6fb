#!/usr/bin/env python3
"""Blocks of right-hand sides on a tiered direct solver (solve_direct_tier_multi_dev) against its single solve on one
MI355X.

The premise under test: a round on a tiered factor is nearly all the two passes over the W_tt, a second column adds only
its vectors, so a block of 8 columns should cost little more than one column.  Nothing is promised; this measures.

Every operator runs in a child process of its own under `--limit` seconds (a child that fails or runs out of time ends
the run: nothing more is started on the device).  In a child, per protocol ONE solver, device buffers, `--warm` untimed
calls per width, then `--reps` (5) repetitions alternating between the widths
  1             solve_dev on one column: the single solve, the yardstick
  2, 4, 8       solve_direct_tier_multi_dev on a block of that many columns (b_i = i + c in column c)
under the protocols
  direct_1      tol 0, maxit 1 (one round, nothing recomputed: the reference's direct protocol)
  direct_tol    --tol (1e-10): rounds until the recomputed residual of every column meets it
An operator is NAME@TIERS (tiers 0: the fewest that fit the entry budget).  With `+single` behind it the single
skyline's solve_direct_multi_dev on a block of 8 on the same operator is timed in the same alternation (width "s8").
One JSON line per operator on stdout; per protocol and width
  columns_per_s   [slowest, fastest] over the repetitions
  us_per_block    [fastest, slowest]
  round_gb_s      lsb_hip_solver_direct_tier_multi_round_bytes x rounds over the time, [slowest, fastest]
  x_single        columns_per_s over width 1's, [slowest over fastest, fastest over slowest]
Progress goes to stderr.

Usage: python tools/bench_direct_tier_multi.py [--operators "A@2;B@0+single"] [--reps 5] [--solves 50] [--warm 5]
                                               [--tol 1e-10] [--limit 400]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_direct_tiers import matrix  # noqa: E402

WIDTHS = (1, 2, 4, 8)
DEFAULT = "lap2d:nx=512,ny=512@0;lap2d:nx=1024,ny=1024@0;lap2d:nx=128,ny=128@2+single;xn3b_A_18@2"


def child(a, spec):
    import torch

    import lsbench_amd as la
    assert la.hip_cdna4_init() == 0, "needs an MI355X"
    single = spec.endswith("+single")
    name, tiers = (spec[:-len("+single")] if single else spec).rsplit("@", 1)
    tiers = int(tiers)
    with tempfile.TemporaryDirectory(prefix="lsb_tier_multi_") as tmp:
        A = matrix(la, name, tmp)
    n = A.nrows
    B = np.stack([np.arange(n, dtype=np.float64) + c for c in range(max(WIDTHS))])
    d_B = torch.from_numpy(B).to("cuda:0")
    d_X = torch.zeros_like(d_B)
    widths = list(WIDTHS) + (["s8"] if single else [])
    res = {}
    for p, kw in {"direct_1": dict(tol=0.0, maxit=1), "direct_tol": dict(tol=a.tol)}.items():
        o = la.default_opts(op_mode=la.OP_RAW, krylov=la.KRYLOV_DIRECT, **kw)
        t0 = time.perf_counter()
        s = la.Solver.create_direct(A, o, tiers)
        create_s = time.perf_counter() - t0
        s1 = la.Solver(A, o) if single else None

        def block(k):
            if k == "s8":
                return s1.solve_direct_multi_dev(d_B, d_X)
            if k == 1:
                return [s.solve_dev(d_B[0], d_X[0])]
            return s.solve_direct_tier_multi_dev(d_B[:k], d_X[:k])

        rec = {}
        for k in widths:
            for _ in range(a.warm):
                r = block(k)
            torch.cuda.synchronize()
            by = s1.direct_multi_round_bytes(8) if k == "s8" else s.direct_tier_multi_round_bytes(k)
            rec[k] = {"t": [], "rounds": max(int(q.iters) for q in r), "status": [int(q.status) for q in r],
                      "relres": max(float(q.relres) for q in r), "round_bytes": by}
            print(name, p, "width", k, "rounds", rec[k]["rounds"], "status", rec[k]["status"], "relres",
                  rec[k]["relres"], file=sys.stderr, flush=True)
        for rep in range(a.reps):
            for k in widths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.solves):
                    block(k)
                torch.cuda.synchronize()
                rec[k]["t"].append((time.perf_counter() - t0) / a.solves)
            print(name, p, "rep", rep, {k: "%.0f columns/s" % ((8 if k == "s8" else k) / rec[k]["t"][-1])
                                        for k in widths}, file=sys.stderr, flush=True)
        one = rec[1]["t"]
        out = {}
        for k in widths:
            t = rec[k].pop("t")
            kc = 8 if k == "s8" else k
            gb = 1e-9 * rec[k]["round_bytes"] * rec[k]["rounds"]
            out[str(k)] = dict(rec[k], columns_per_s=[kc / max(t), kc / min(t)],
                               us_per_block=[1e6 * min(t), 1e6 * max(t)], round_gb_s=[gb / max(t), gb / min(t)],
                               x_single=[(kc / max(t)) * min(one), (kc / min(t)) * max(one)])
        nt, w, c, rows, launches = s.direct_tier_info()
        out.update(create_s=create_s, tiers=nt, w_entries=w, coupling_entries=c, tier_rows=rows,
                   launches_per_round=launches)
        res[p] = out
        s.destroy()
        if s1:
            s1.destroy()
    print(json.dumps({"bench": "direct_tier_multi", "operator": name, "tiers_asked": tiers, "n": n, "nnz": int(A.nnz),
                      "reps": a.reps, "solves": a.solves, "warm": a.warm, "tol": a.tol, "protocols": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a, a.child)
    for spec in [x for x in a.operators.split(";") if x]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", spec, "--reps", str(a.reps), "--solves",
               str(a.solves), "--warm", str(a.warm), "--tol", repr(a.tol)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("bench_direct_tier_multi: %s ended with %d; nothing more is started" % (spec, rc), file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
