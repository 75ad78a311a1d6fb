#!/usr/bin/env python3
"""AMG as the solver (opts.krylov = KRYLOV_RICHARDSON) against AMG-PCG on one MI355X.

bench.py's --krylov list is fixed, so this is the measurement of the stationary V-cycle iteration.  Per operator
and per cycle variant (l1-Jacobi / Chebyshev smoother x fp64 / fp32 cycle) one JSON line on stdout:

  * us_per_cycle / us_per_pcg_iter   solves cut at a fixed count (tol = 0, maxit = --iters) on two solvers of the
                    same hierarchy, one Richardson, one classic PCG, alternating: `--warmup` untimed and `--solves`
                    timed solves each, host clock around the solve (it ends in a device synchronise); median,
                    with min and max beside it.
  * protocol        the reference's AMG protocol (src/hypre.c:185-186, src/amgx.c:78-85): maxit = 2, tol = 0, in
                    solves/s over `--protocol-solves` solves, and the relative residual those two cycles reach.
  * converge        Richardson and AMG-PCG to --tol: status, cycles or iterations, seconds of the second (hinted)
                    solve, the convergence factor per cycle relres^(1/cycles), and the residual recomputed on
                    the device through spmv_dev.

Usage: python tools/bench_richardson.py [--spec lap2d:nx=3162,ny=3162] [--iters 20] [--warmup 2] [--solves 5]
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
    ap.add_argument("--spec", default="lap2d:nx=3162,ny=3162")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--protocol-solves", type=int, default=30)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--conv-maxit", type=int, default=5000)
    ap.add_argument("--nu", type=int, default=1)
    ap.add_argument("--variants", default="l1-fp64,l1-fp32,cheb-fp64,cheb-fp32")
    a = ap.parse_args()

    import torch

    import lsbench_amd as la

    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    torch.cuda.set_device(0)
    rc = la.hip_cdna4_init()
    assert rc == 0 or la._lib.load().lsb_hip_stream()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}),
          flush=True)
    M = la.lsbench_matrix_synth(a.spec)
    n = M.nrows
    d_b = torch.arange(n, dtype=torch.float64, device="cuda:0")
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    d_y = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    bn = float(torch.linalg.norm(d_b))

    def timed(s, count, status):
        res = s.solve_dev(d_b, d_x)
        torch.cuda.synchronize()
        assert int(res.iters) == count and res.status == status, (res.iters, res.status)
        return res

    def stats(v):
        v = np.array(v)
        return {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2)}

    for variant in a.variants.split(","):
        sm, pr = variant.split("-")
        amg = dict(op_mode=la.OP_RAW, precond=la.PRECOND_AMG, amg_sweeps=a.nu,
                   amg_smoother=la.AMG_SMOOTH_CHEB if sm == "cheb" else la.AMG_SMOOTH_L1JACOBI,
                   amg_precision=la.AMG_PREC_FP32 if pr == "fp32" else la.AMG_PREC_FP64)
        rich, pcg = dict(amg, krylov=la.KRYLOV_RICHARDSON), dict(amg, krylov=la.KRYLOV_PCG)
        t0 = time.time()
        sr = la.Solver(M, la.default_opts(tol=0.0, maxit=a.iters, **rich))
        setup = time.time() - t0
        sp = la.Solver(M, la.default_opts(tol=0.0, maxit=a.iters, **pcg))
        rec = {"operator": a.spec, "rows": n, "nnz": int(M.nnz), "variant": variant, "nu": a.nu,
               "setup_s": round(setup, 2), "levels": sr.amg_info[0], "amg_cycle_bytes": sr.amg_cycle_bytes,
               "count_per_solve": a.iters, "warmup": a.warmup, "solves": a.solves, "padded_rows": int(sr.padded)}
        us_r, us_p = [], []
        for k in range(a.warmup + a.solves):  # alternating, on one box in one process
            r = timed(sr, a.iters, la.STATUS_MAXIT)
            p = timed(sp, a.iters, la.STATUS_MAXIT)
            if k >= a.warmup:
                us_r.append(r.seconds * 1e6 / a.iters)
                us_p.append(p.seconds * 1e6 / a.iters)
        rec.update(us_per_cycle=stats(us_r), us_per_pcg_iter=stats(us_p))
        sr.destroy()
        sp.destroy()
        # the reference's protocol: two cycles, no tolerance
        s = la.Solver(M, la.default_opts(tol=0.0, maxit=2, **rich))
        for _ in range(5):
            res = timed(s, 2, la.STATUS_MAXIT)
        t0 = time.time()
        for _ in range(a.protocol_solves):
            res = s.solve_dev(d_b, d_x)
        torch.cuda.synchronize()
        dt = time.time() - t0
        s.destroy()
        rec["protocol"] = {"maxit": 2, "tol": 0, "solves": a.protocol_solves, "solves_per_s": round(a.protocol_solves / dt, 2),
                           "relres_after_2_cycles": float(res.relres)}
        # to a tolerance: far more cycles than PCG iterations
        for name, kw in (("richardson", rich), ("pcg", pcg)):
            s = la.Solver(M, la.default_opts(tol=a.tol, maxit=a.conv_maxit, **kw))
            s.solve_dev(d_b, d_x)  # (the second solve enqueues the first one's count in one go)
            res = s.solve_dev(d_b, d_x)
            torch.cuda.synchronize()
            s.spmv_dev(d_x, d_y)
            s.destroy()
            true = float(torch.linalg.norm(d_b - d_y)) / bn
            it = max(int(res.iters), 1)
            rec["converge_" + name] = {"tol": a.tol, "maxit": a.conv_maxit, "status": int(res.status),
                                       "count": int(res.iters), "relres": float(res.relres),
                                       "seconds": round(float(res.seconds), 4),
                                       "factor_per_cycle": round(float(res.relres) ** (1.0 / it), 4) if res.relres > 0 else None,
                                       "recomputed_relres": true}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
