#!/usr/bin/env python3
"""The direct solver on a tiered inverse factor (Solver.create_direct) on one MI355X: against the single skyline where
both exist, and against the fastest iterative form and a CPU sparse LU where the single skyline is over the budget.

Every operator runs in a child process of its own under `--limit` seconds (a child that fails or runs out of time ends
the run: nothing more is started on the device).  In a child, one fresh solver per configuration, `--reps` (5)
repetitions alternating between the configurations, `--solves` solve_dev calls of b_i = i per repetition after
`--warm` untimed ones.  Times are a host clock around work that ends in a device synchronise.

  compare   (--operators, separated by ';', default xn3b_A_18;tj7a_A_12;lap2d:nx=128,ny=128;lap2d:nx=256,ny=256)
            tiers 1, 2, 3, 4, each at tol 0 / maxit 1 (one round: the reference's direct protocol) and at --tol
            (1e-10); per configuration solves/s [min, max], us per round, the tiers, entries, launches and the bytes
            model of a round divided by its time (GB/s)
  beyond    (--beyond, default lap2d:nx=512,ny=512;lap2d:nx=1024,ny=1024)
            tiers 0 (the fewest that fit) at both settings, with the seconds creation took (ordering, symbolic count,
            sequential Cholesky and the W_tt on the host, upload), against AMG-PCG with the fp32 cycle at --tol in the
            same process
  --cpu     no device: scipy's splu (COLAMD) of the --beyond operators, factorised once, then solves timed -- the CPU
            stand-in of the reference's direct backends

One JSON line per operator on stdout; progress on stderr.

Usage: python tools/bench_direct_tiers.py [--operators "A;B"] [--beyond "C;D"] [--reps 5] [--solves 100] [--warm 10]
                                          [--tol 1e-10] [--limit 500] [--cpu]
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def matrix(la, name, tmp):
    """(Matrix as the solver takes it with op_mode RAW, both triangles)"""
    if ":" in name:
        return la.lsbench_matrix_synth(name)
    p = os.path.join(ROOT, "tests", "golden", "matrices", name + ".txt")
    if not os.path.exists(p):
        out = os.path.join(tmp, name + ".txt")
        with gzip.open(p + ".gz", "rb") as fi, open(out, "wb") as fo:
            fo.write(fi.read())
        p = out
    return la.lsb_csr_symmetrize_upper(la.lsbench_matrix_read(p))


def scipy_of(A):
    import scipy.sparse as sp
    n = A.nrows
    return sp.csr_matrix((np.array(A.vals), np.array(A.cols, np.int64) - A.base, np.array(A.offs, np.int64)),
                         shape=(n, n))


def child(a, name, beyond):
    import torch

    import lsbench_amd as la
    assert la.hip_cdna4_init() == 0, "needs an MI355X"
    with tempfile.TemporaryDirectory(prefix="lsb_tiers_") as tmp:
        A = matrix(la, name, tmp)
    n = A.nrows
    S = scipy_of(A)
    b = np.arange(n, dtype=np.float64)
    d_b = torch.from_numpy(b).to("cuda:0")
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    configs = {}
    for tiers in ((0,) if beyond else (1, 2, 3, 4)):
        configs["tiers%d_one" % tiers] = (tiers, dict(krylov=la.KRYLOV_DIRECT, tol=0.0, maxit=1))
        configs["tiers%d_tol" % tiers] = (tiers, dict(krylov=la.KRYLOV_DIRECT, tol=a.tol))
    if beyond:
        configs["amg_f32_pcg"] = (None, dict(precond=la.PRECOND_AMG, amg_precision=la.AMG_PREC_FP32, tol=a.tol))
    solvers, rec = {}, {}
    for f, (tiers, kw) in configs.items():
        t0 = time.perf_counter()
        o = la.default_opts(op_mode=la.OP_RAW, **kw)
        solvers[f] = la.Solver(A, o) if tiers is None else la.Solver.create_direct(A, o, tiers)
        rec[f] = {"create_s": time.perf_counter() - t0, "t": []}
        for _ in range(a.warm):
            res = solvers[f].solve_dev(d_b, d_x)
        torch.cuda.synchronize()
        x = d_x.cpu().numpy()
        rec[f].update(iters=int(res.iters), status=int(res.status), relres=float(res.relres),
                      true_relres=float(np.linalg.norm(b - S @ x) / np.linalg.norm(b)))
        print(name, f, "created in %.2f s" % rec[f]["create_s"], "iters", res.iters, "status", res.status, "true relres",
              rec[f]["true_relres"], file=sys.stderr, flush=True)
    for rep in range(a.reps):
        for f in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.solves):
                solvers[f].solve_dev(d_b, d_x)
            torch.cuda.synchronize()
            rec[f]["t"].append((time.perf_counter() - t0) / a.solves)
        print(name, "rep", rep, {f: "%.0f/s" % (1.0 / rec[f]["t"][-1]) for f in configs}, file=sys.stderr, flush=True)
    out = {}
    for f in configs:
        t = rec[f].pop("t")
        it = max(rec[f]["iters"], 1)
        out[f] = dict(rec[f], solves_per_s=[1.0 / max(t), 1.0 / min(t)], us_per_round=[1e6 * min(t) / it, 1e6 * max(t) / it])
        info = solvers[f].direct_tier_info()
        if info:
            nt, w, c, rows, launches = info
            by = solvers[f].direct_info[2]
            out[f].update(tiers=nt, w_entries=w, coupling_entries=c, tier_rows=rows, launches_per_round=launches,
                          bytes_per_round=by, model_gb_per_s=[1e-9 * by * it / max(t), 1e-9 * by * it / min(t)])
        solvers[f].destroy()
    print(json.dumps({"bench": "direct_tiers", "operator": name, "n": n, "nnz": int(A.nnz), "reps": a.reps,
                      "solves": a.solves, "tol": a.tol, "configs": out}), flush=True)


def cpu(a):
    import scipy.sparse.linalg as spla

    import lsbench_amd as la
    for name in a.beyond.split(";"):
        A = matrix(la, name, None)
        S = scipy_of(A).tocsc()
        b = np.arange(A.nrows, dtype=np.float64)
        t0 = time.perf_counter()
        lu = spla.splu(S)
        fact = time.perf_counter() - t0
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            x = lu.solve(b)
            t.append(time.perf_counter() - t0)
        print(json.dumps({"bench": "direct_tiers_cpu_splu", "operator": name, "n": A.nrows, "factor_s": fact,
                          "solves_per_s": [1.0 / max(t), 1.0 / min(t)],
                          "true_relres": float(np.linalg.norm(b - S @ x) / np.linalg.norm(b))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", default="xn3b_A_18;tj7a_A_12;lap2d:nx=128,ny=128;lap2d:nx=256,ny=256")
    ap.add_argument("--beyond", default="lap2d:nx=512,ny=512;lap2d:nx=1024,ny=1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=100)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-beyond", action="store_true")
    a = ap.parse_args()
    if a.cpu:
        return cpu(a)
    if a.child:
        return child(a, a.child, a.child_beyond)
    jobs = [(n, False) for n in a.operators.split(";") if n] + [(n, True) for n in a.beyond.split(";") if n]
    for name, beyond in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--solves",
               str(a.solves), "--warm", str(a.warm), "--tol", repr(a.tol)] + (["--child-beyond"] if beyond else [])
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("bench_direct_tiers: %s ended with %d; nothing more is started" % (name, rc), file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
