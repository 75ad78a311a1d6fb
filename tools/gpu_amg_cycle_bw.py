#!/usr/bin/env python
"""Time of one application of the AMG V-cycle, fp64 against fp32 (--amg-precision), and the bandwidth it achieves:
lsb_hip_solver_amg_cycle_bytes over that time.  Needs an MI355X.

    python tools/gpu_amg_cycle_bw.py MATRIX_FILE | synth:SPEC [all]

An application is timed through Solver.precond_dev (device events around REPS back-to-back calls after a warm-up,
the variants alternating, two rounds).  That call also copies r in and z out, 32 n bytes in all; they are added to
the bytes, and the line says so.  nu = 1 and 2, l1-Jacobi; with `all` also the Chebyshev smoother and multicolour
Gauss-Seidel (--amg-smoother cheb, mcgs), each in both precisions."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsbench_amd as la  # noqa: E402

REPS = 50
SMOOTHERS = {la.AMG_SMOOTH_L1JACOBI: "l1", la.AMG_SMOOTH_CHEB: "cheb", la.AMG_SMOOTH_MCGS: "mcgs"}


def main():
    name = sys.argv[1]
    assert torch.cuda.is_available(), "needs an MI355X"
    assert la.hip_cdna4_init() == 0 or la._lib.load().lsb_hip_stream()
    synth = name.startswith("synth:")
    A = la.lsbench_matrix_synth(name[6:]) if synth else la.lsbench_matrix_read(name)
    n = A.nrows
    d_r = torch.from_numpy(np.sin(np.arange(n, dtype=np.float64)) + 0.5).to("cuda:0")
    d_z = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    smoothers = list(SMOOTHERS) if sys.argv[2:] == ["all"] else [la.AMG_SMOOTH_L1JACOBI]
    for nu in (1, 2):
        sol = {}
        for sm in smoothers:
            for prec in (la.AMG_PREC_FP64, la.AMG_PREC_FP32):
                kw = dict(op_mode=la.OP_RAW) if synth else {}
                sol[(sm, prec)] = la.Solver(A, la.default_opts(precond=la.PRECOND_AMG, amg_sweeps=nu, amg_smoother=sm,
                                                               amg_precision=prec, **kw))
        for rnd in range(2):
            for (sm, prec), s in sol.items():
                for _ in range(5):
                    s.precond_dev(d_r, d_z)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(REPS):
                    s.precond_dev(d_r, d_z)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / REPS
                by = s.amg_cycle_bytes
                print("%s nu=%d %s %s round %d: %d levels, %.1f us per application (with the copies of r and z), "
                      "cycle bytes %d (+ %d copied): %.3f TB/s" % (name, nu, SMOOTHERS[sm], "fp32" if prec else "fp64",
                                                                  rnd, s.amg_info[0], us, by, 32 * n,
                                                                  (by + 32 * n) / us * 1e-6))
        for s in sol.values():
            s.destroy()


if __name__ == "__main__":
    main()
