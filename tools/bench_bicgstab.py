#!/usr/bin/env python3
"""BiCGSTAB against GMRES(30) on unsymmetric / general-valued 10 M-row operators, one MI355X.

bench.py's --krylov list is fixed, so this is the measurement of opts.krylov = KRYLOV_BICGSTAB.  Per operator
and method one JSON line on stdout:

  * us_per_iter     from solves cut at a fixed maxit (no convergence needed): `--warmup` untimed and
                    `--solves` timed solves of `--iters` iterations each, host clock around the solve (it
                    ends in a device synchronise); median, with min and max beside it.  A BiCGSTAB
                    iteration holds two products with the operator, a GMRES inner step one:
                    `us_per_two_products` is the like-for-like number.
  * iteration_bytes what one iteration must move (two SpMV layouts + the sweeps' vector passes) and
                    frac_of_8TBs = those bytes over the median time over 8 TB/s; null for GMRES, whose
                    step has no fixed byte count.
  * converge        a solve to --tol with verify = 1: status, iterations, corrections, solves/s and the
                    residual recomputed with scipy on the CPU -- solves/s only where it converged.

Usage: python tools/bench_bicgstab.py [--n 3162] [--iters 200] [--warmup 5] [--solves 20] [--no-converge]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3162, help="grid side (rows = n^2)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--conv-maxit", type=int, default=20000)
    ap.add_argument("--no-converge", action="store_true")
    ap.add_argument("--operators", default="conv,coef")
    a = ap.parse_args()

    import scipy.sparse as sp
    import torch

    import lsbench_amd as la

    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    torch.cuda.set_device(0)
    rc = la.hip_cdna4_init()
    assert rc == 0 or la._lib.load().lsb_hip_stream()
    specs = {"conv": "lap2d:nx=%d,ny=%d,conv=0.1" % (a.n, a.n), "coef": "lap2d:nx=%d,ny=%d,coef=1" % (a.n, a.n)}
    methods = (("bicgstab", la.KRYLOV_BICGSTAB, 2), ("gmres30", la.KRYLOV_GMRES, 1))
    for key in a.operators.split(","):
        M = la.lsbench_matrix_synth(specs[key])
        n = M.nrows
        A = sp.csr_matrix((M.vals, M.cols.astype(np.int64), M.offs.astype(np.int64)), shape=(n, n))
        b = np.arange(n, dtype=np.float64)
        d_b = torch.from_numpy(b).to("cuda:0")
        d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        bn = float(np.linalg.norm(b))
        for name, kry, products in methods:
            kw = dict(op_mode=la.OP_RAW, krylov=kry, restart=30, tol=0.0, maxit=a.iters, verify=0)
            t0 = time.time()
            s = la.Solver(M, la.default_opts(**kw))
            rec = {"operator": specs[key], "rows": n, "nnz": int(M.nnz), "method": name, "setup_s": round(time.time() - t0, 2),
                   "iters_per_solve": a.iters, "warmup": a.warmup, "solves": a.solves,
                   "spmv_variant": int(s.spmv_variant), "spmv_flags": int(s.spmv_flags), "padded_rows": int(s.padded)}
            us = []
            for k in range(a.warmup + a.solves):
                res = s.solve_dev(d_b, d_x)
                torch.cuda.synchronize()
                assert int(res.iters) == a.iters and res.status == la.STATUS_MAXIT, (res.iters, res.status)
                if k >= a.warmup:
                    us.append(res.seconds * 1e6 / a.iters)
            us = np.array(us)
            med = float(np.median(us))
            rec.update(us_per_iter=round(med, 2), us_per_iter_min=round(float(us.min()), 2),
                       us_per_iter_max=round(float(us.max()), 2), products_per_iter=products,
                       us_per_two_products=round(med * 2 / products, 2))
            ib = int(s.iteration_bytes) if kry == la.KRYLOV_BICGSTAB else 0
            rec.update(spmv_layout_bytes=int(s.spmv_layout_bytes), iteration_bytes=ib or None,
                       frac_of_8TBs=round(ib / (med * 1e-6) / 8e12, 3) if ib else None)
            s.destroy()
            if not a.no_converge:
                kw.update(tol=a.tol, maxit=a.conv_maxit, verify=1)
                s = la.Solver(M, la.default_opts(**kw))
                s.solve_dev(d_b, d_x)  # (the second solve enqueues the first one's iteration count in one go)
                res = s.solve_dev(d_b, d_x)
                torch.cuda.synchronize()
                s.destroy()
                x = d_x.cpu().numpy()
                ok = res.status == la.STATUS_CONVERGED
                rec["converge"] = {"tol": a.tol, "maxit": a.conv_maxit, "status": int(res.status), "converged": bool(ok),
                                   "iters": int(res.iters), "corrections": int(res.corrections),
                                   "relres": float(res.relres), "seconds": round(float(res.seconds), 4),
                                   "solves_per_s": round(1.0 / res.seconds, 4) if ok else None,
                                   "recomputed_relres_cpu": float(np.linalg.norm(b - A @ x) / bn)
                                   if np.isfinite(x).all() else None}
            print(json.dumps(rec), flush=True)
        del A, M


if __name__ == "__main__":
    main()
