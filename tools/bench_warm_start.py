"""What a solve from an initial guess costs over a cold solve (profiles/r13_warm_start.txt): solve_dev against
solve_x0_dev with x0 = 0 on one solver in one process, alternating, five of each after two untimed of each, on
tests/golden/matrices/xn3b_A_18 (tol 1e-12) and on lap2d:nx=1000,ny=1000 (raw, tol 1e-6, line-padded inside the
solver).  res.seconds is the library's clock around the solve, wall the caller's around the call.

    python tools/bench_warm_start.py"""
import gzip
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsbench_amd as la  # noqa: E402

assert la.hip_cdna4_init() == 0
out = []


def run(name, M, opts, n):
    s = la.Solver(M, opts)
    d_b = torch.arange(1, n + 1, dtype=torch.float64, device="cuda:0")
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    for _ in range(2):  # both paths once, untimed: hints, graphs, the work buffers
        s.solve_dev(d_b, d_x)
        d_x.zero_()
        s.solve_dev(d_b, d_x, warm=True)
    cold, warm, cw, ww, its = [], [], [], [], None
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = s.solve_dev(d_b, d_x)
        cw.append(time.perf_counter() - t)
        cold.append(r.seconds)
        xc = d_x.clone()
        d_x.zero_()
        torch.cuda.synchronize()
        t = time.perf_counter()
        rw = s.solve_dev(d_b, d_x, warm=True)
        ww.append(time.perf_counter() - t)
        warm.append(rw.seconds)
        assert torch.equal(xc, d_x) and rw.iters == r.iters
        its = r.iters
    s.destroy()
    f = lambda v: " ".join("%9.1f" % (1e6 * x) for x in v)
    out.append("%s: n = %d, %d iterations per solve, us per solve\n"
               "  solve_dev     res.seconds %s   wall %s\n"
               "  solve_x0_dev  res.seconds %s   wall %s\n"
               "  difference of the medians: res.seconds %.1f us, wall %.1f us (%.2f %% of the cold solve)\n"
               % (name, n, its, f(cold), f(cw), f(warm), f(ww), 1e6 * (np.median(warm) - np.median(cold)),
                  1e6 * (np.median(ww) - np.median(cw)), 100 * (np.median(ww) - np.median(cw)) / np.median(cw)))


gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "matrices")
with tempfile.TemporaryDirectory() as tmp:
    p = os.path.join(tmp, "xn3b_A_18.txt")
    with gzip.open(os.path.join(gold, "xn3b_A_18.txt.gz"), "rb") as fi, open(p, "wb") as fo:
        fo.write(fi.read())
    A = la.lsbench_matrix_read(p)
    run("xn3b_A_18, tol 1e-12", A, la.default_opts(tol=1e-12), A.nrows)
run("lap2d 1000 x 1000 (line-padded, two-launch form), tol 1e-6", la.lsbench_matrix_synth("lap2d:nx=1000,ny=1000"),
    la.default_opts(op_mode=la.OP_RAW, tol=1e-6), 1000 * 1000)
print("\n".join(out))
