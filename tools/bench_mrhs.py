#!/usr/bin/env python3
"""Several right-hand sides at once against the same number of single solves, one MI355X.

On ONE solver per operator, in one process, `--reps` (5) times alternating between
  (a) nrhs calls of solve_dev -- the existing, unchanged path -- and
  (b) one solve_multi_dev of nrhs columns,
for nrhs in 2, 4, 8.  The columns are b_c = (c + 1) i, so every column takes the same iterations either way (to
one or two: the scaling rounds) and (a) is a fair baseline.  Each shape is warmed up first (two untimed rounds
each way: the second solve of a shape enqueues the first one's iteration count in one go, and under use_graph
builds the graph of that count).  Times are a host clock around work that ends in a device synchronise.
One JSON line on stdout: per operator and nrhs
  rhs_per_s_single / rhs_per_s_multi   right-hand sides per second, [min, max] over the repetitions
  us_per_iter_single / _multi          microseconds per iteration (of one solve / of the batch), [min, max]
  multi_iteration_bytes, frac_of_8TBs  what an iteration of the batch must move, over its time, over 8 TB/s
  gain                                 true only where (b)'s slowest repetition beats (a)'s fastest
--precond amg: the same protocol on an AMG solver (single AMG solves against batches under AMG on that solver);
multi_iteration_bytes is 0 there (an iteration around a V-cycle has another shape) and so is frac_of_8TBs.
--precond fsai [--fsai-power K]: the same protocol on an FSAI solver created with fsai_blocks = 1, whose single-column
paths are the default FSAI solver's: (a) nrhs single FSAI solves (the fused three-launch iteration where it applies)
against (b) one batch (four launches an iteration) on that solver.
--verbose: the solver's own report at creation (the AMG hierarchy level by level) on stderr, and per width the
device memory in use behind the first batch (device_mem_mb: everything the process holds, the solver included).
--block: block-CG proper beside the independent recurrences -- per width one solve_block_dev and one solve_multi_dev on
the same solver and the same B (column 0 is b_i = i, the others standard normal draws of seed 7: a block must have full
rank, which the columns (c + 1) i above have not), alternating, after the same two warm-up rounds.  Per width under
"block": iterations of both forms (solve_multi: per column), seconds per solve (the median over the repetitions, and
[min, max]), and bytes per iteration over the time per iteration of each form, in GB/s.  With --precond fsai|amg the
block form is solve_block_dev(precond=True) on that solver (lsb_hip_solver_solve_block_precond_dev) and its bytes are
block_precond_iteration_bytes: 0 under AMG, as multi_iteration_bytes, and so are the GB/s.
Progress goes to stderr.

Usage: python tools/bench_mrhs.py [--operators xn3b,tj7a,coef,lap2d] [--reps 5] [--n 3162] [--nrhs 2,4,8]
                                  [--fixed-iters N] [--precond jacobi|amg|fsai] [--fsai-power K] [--verbose] [--block]
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def file_matrix(la, name, tmp):
    p = os.path.join(ROOT, "tests", "golden", "matrices", name + ".txt")
    if not os.path.exists(p):
        out = os.path.join(tmp, name + ".txt")
        with gzip.open(p + ".gz", "rb") as fi, open(out, "wb") as fo:
            fo.write(fi.read())
        p = out
    return la.lsbench_matrix_read(p)


def block_leg(la, torch, s, n, nrhs, reps, key, precond):
    """solve_block_dev (precond: its preconditioned entry point) beside solve_multi_dev on one solver and one B"""
    g = torch.Generator().manual_seed(7)
    B = torch.randn(nrhs, n, dtype=torch.float64, generator=g)
    B[0] = torch.arange(n, dtype=torch.float64)
    d_B = B.to("cuda:0")
    d_X = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda:0")

    def run(f):
        t = time.perf_counter()
        res = f(d_B, d_X)
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        assert all(r.status == la.STATUS_CONVERGED for r in res), [r.status for r in res]
        return t, [int(r.iters) for r in res]

    def block(d_B, d_X):
        return s.solve_block_dev(d_B, d_X, precond=precond)

    for _ in range(2):
        run(s.solve_multi_dev), run(block)
    tm, tb, itm, itb = [], [], None, None
    for k in range(reps):
        t, itm = run(s.solve_multi_dev)
        tm.append(t)
        t, itb = run(block)
        tb.append(t)
        print("%s nrhs %d rep %d: multi %.4f s, block %.4f s" % (key, nrhs, k, tm[-1], tb[-1]), file=sys.stderr,
              flush=True)
    tm, tb = np.array(tm), np.array(tb)
    mb = s.multi_iteration_bytes(nrhs)
    bb = s.block_precond_iteration_bytes(nrhs) if precond else s.block_iteration_bytes(nrhs)
    return {"iters_multi": itm, "iters_block": itb[0],
            "s_per_solve_multi": round(float(np.median(tm)), 6), "s_per_solve_block": round(float(np.median(tb)), 6),
            "s_minmax_multi": [round(float(tm.min()), 6), round(float(tm.max()), 6)],
            "s_minmax_block": [round(float(tb.min()), 6), round(float(tb.max()), 6)],
            "multi_iteration_bytes": int(mb), "block_iteration_bytes": int(bb),
            "GBs_multi": round(mb * max(itm) / float(np.median(tm)) / 1e9, 1),
            "GBs_block": round(bb * itb[0] / float(np.median(tb)) / 1e9, 1),
            "block_over_multi_time": round(float(np.median(tb) / np.median(tm)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", default="xn3b,tj7a,coef,lap2d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=3162, help="grid side of the two synthetic operators")
    ap.add_argument("--nrhs", default="2,4,8")
    ap.add_argument("--fixed-iters", type=int, default=0,
                    help="cut every solve at this many iterations (tol = 0): for a kernel trace, not for rates")
    ap.add_argument("--precond", choices=("jacobi", "amg", "fsai"), default="jacobi")
    ap.add_argument("--fsai-power", type=int, default=3)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--block", action="store_true", help="block-CG proper beside solve_multi (see above)")
    ap.add_argument("--tol", type=float, default=0.0, help="override the operators' tolerances")
    a = ap.parse_args()

    import torch

    import lsbench_amd as la

    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    torch.cuda.set_device(0)
    rc = la.hip_cdna4_init()
    assert rc == 0 or la._lib.load().lsb_hip_stream()
    tmp = tempfile.mkdtemp()
    ops = {"xn3b": (lambda: file_matrix(la, "xn3b_A_18", tmp), dict(tol=1e-12), "tests/golden/matrices/xn3b_A_18"),
           "tj7a": (lambda: file_matrix(la, "tj7a_A_18", tmp), dict(tol=1e-12), "tests/golden/matrices/tj7a_A_18"),
           "coef": (lambda: la.lsbench_matrix_synth("lap2d:nx=%d,ny=%d,coef=1" % (a.n, a.n)),
                    dict(tol=1e-8, op_mode=la.OP_RAW), "lap2d:nx=%d,ny=%d,coef=1" % (a.n, a.n)),
           "lap2d": (lambda: la.lsbench_matrix_synth("lap2d:nx=%d,ny=%d" % (a.n, a.n)),
                     dict(tol=1e-8, op_mode=la.OP_RAW), "lap2d:nx=%d,ny=%d" % (a.n, a.n))}
    out = []
    for key in a.operators.split(","):
        make, kw, label = ops[key]
        M = make()
        t0 = time.time()
        if a.tol > 0.0:
            kw = dict(kw, tol=a.tol)
        if a.fixed_iters:
            kw = dict(kw, tol=0.0)
        if a.precond == "amg":
            kw = dict(kw, precond=la.PRECOND_AMG)
        if a.precond == "fsai":
            kw = dict(kw, precond=la.PRECOND_FSAI, fsai_power=a.fsai_power, fsai_blocks=1)
        if a.verbose:
            kw = dict(kw, verbose=1)
        s = la.Solver(M, la.default_opts(maxit=a.fixed_iters or 100000, **kw))
        n = s.n_local
        rec = {"operator": label, "rows": n, "nnz": int(s.nnz_local), "tol": kw["tol"], "setup_s": round(time.time() - t0, 2),
               "padded_rows": int(s.padded), "precond": a.precond + ("(%d)" % a.fsai_power if a.precond == "fsai" else ""), "iteration_bytes_single": int(s.iteration_bytes), "reps": a.reps, "nrhs": {}}
        if a.block:
            assert not a.fixed_iters, "--block: to a tolerance"
            rec["block"] = {}
        for nrhs in [int(v) for v in a.nrhs.split(",")]:
            if a.block:
                rec["block"][str(nrhs)] = block_leg(la, torch, s, n, nrhs, a.reps, key, a.precond != "jacobi")
                continue
            d_B = torch.arange(n, dtype=torch.float64, device="cuda:0")[None, :] * \
                torch.arange(1, nrhs + 1, dtype=torch.float64, device="cuda:0")[:, None]
            d_X = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda:0")
            ts, tm, its, itm = [], [], None, None

            def single():
                t = time.perf_counter()
                it = [int(s.solve_dev(d_B[c], d_X[c]).iters) for c in range(nrhs)]
                torch.cuda.synchronize()
                return time.perf_counter() - t, it

            def multi():
                t = time.perf_counter()
                res = s.solve_multi_dev(d_B, d_X)
                torch.cuda.synchronize()
                want = la.STATUS_MAXIT if a.fixed_iters else la.STATUS_CONVERGED
                assert all(r.status == want for r in res), [r.status for r in res]
                return time.perf_counter() - t, [int(r.iters) for r in res]

            mem_mb = None
            for _ in range(2):  # warm-up of both shapes: the iteration hint, then the graph of that count
                single(), multi()
                if a.verbose and mem_mb is None:
                    free, total = torch.cuda.mem_get_info()
                    mem_mb = round((total - free) / 2.0 ** 20, 1)
            for k in range(a.reps):
                t, its = single()
                ts.append(t)
                t, itm = multi()
                tm.append(t)
                print("%s nrhs %d rep %d: single %.4f s, multi %.4f s" % (key, nrhs, k, ts[-1], tm[-1]),
                      file=sys.stderr, flush=True)
            ts, tm = np.array(ts), np.array(tm)
            mb = s.multi_iteration_bytes(nrhs)
            us_m = tm * 1e6 / max(itm)
            rec["nrhs"][str(nrhs)] = {
                "iters_single": its, "iters_multi": itm,
                "rhs_per_s_single": [round(nrhs / ts.max(), 3), round(nrhs / ts.min(), 3)],
                "rhs_per_s_multi": [round(nrhs / tm.max(), 3), round(nrhs / tm.min(), 3)],
                "us_per_iter_single": [round(float(ts.min() * 1e6 / sum(its)), 3), round(float(ts.max() * 1e6 / sum(its)), 3)],
                "us_per_iter_multi": [round(float(us_m.min()), 3), round(float(us_m.max()), 3)],
                "multi_iteration_bytes": int(mb),
                "frac_of_8TBs": [round(mb / (float(us_m.max()) * 1e-6) / 8e12, 4), round(mb / (float(us_m.min()) * 1e-6) / 8e12, 4)],
                "gain": bool(tm.max() < ts.min())}
            if mem_mb is not None:
                rec["nrhs"][str(nrhs)]["device_mem_mb"] = mem_mb
            del d_B, d_X
        s.destroy()
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps({"bench": "mrhs", "operators": out}), flush=True)


if __name__ == "__main__":
    main()
