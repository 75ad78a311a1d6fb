"""What a projection onto earlier solutions buys on a sequence of slowly changing right-hand sides
(lsb_hip_solver_solve_seq_dev; profiles/r22_seq.txt): per configuration ONE solver and the drifting family of
tests/seq_family.py, solved three ways that alternate, `--reps` times each after one untimed pass --
    cold      solve_dev from zero, every right-hand side
    x0        solve_x0_dev from the previous solution
    seq d     solve_seq_dev behind seq_begin(d), d = 4, 8, 16
-- and per way the iterations of one pass, solves/s (median over the repetitions of steps / wall seconds of a pass),
the device microseconds of a projection and of an update and seq_info's bytes.  The microseconds come from ONE more
pass per depth behind the timed ones, with the solver's events turned on (lsb_hip_solver_seq_last_us; medians over
the solves that had a projection, an update): the timed passes record no events and ask for none.

The configurations: xn3b_A_18 and tj7a_A_12 under Jacobi, FSAI(3) and AMG with the Chebyshev smoother (tol 1e-10): 24
right-hand sides, 5 repetitions, depths 4, 8, 16; lap2d:nx=3162,ny=3162 (raw, tol 1e-8: the two-launch form,
line-padded) under Jacobi and under AMG: a Jacobi solve there takes about a second, so its protocol is 6 right-hand
sides, 1 repetition, depth 8 -- what was run (profiles/r22_seq.txt).  --steps, --reps, --depths override both.

Without --one this process never opens the GPU: it runs one child per configuration, one at a time, each under its own
`timeout -k 10`, and stops at the first that does not end well.

    python tools/bench_seq.py [--configs xn3b_A_18:jacobi,lap2d:amg] [--steps N] [--reps N] [--depths 4,8,16]"""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SMALL = ("xn3b_A_18", "tj7a_A_12")
CONFIGS = [m + ":" + p for m in SMALL for p in ("jacobi", "fsai", "amg")] + ["lap2d:jacobi", "lap2d:amg"]
PROTOCOL = {"lap2d": (6, 1, "8")}  # steps, repetitions, depths; every other operator: (24, 5, "4,8,16")
LIMIT = {"lap2d": 600}  # seconds a child may take (seen: 60 under Jacobi with its protocol); the small operators: 240


def one(config, steps, reps, depths):
    import numpy as np
    import torch

    import lsbench_amd as la
    from seq_family import rhs_drift

    assert la.hip_cdna4_init() == 0
    op, pre = config.split(":")
    kw = {"jacobi": {}, "fsai": dict(precond=la.PRECOND_FSAI),
          "amg": dict(precond=la.PRECOND_AMG, amg_smoother=la.AMG_SMOOTH_CHEB)}[pre]
    if op == "lap2d":
        A = la.lsbench_matrix_synth("lap2d:nx=3162,ny=3162")
        opts = la.default_opts(op_mode=la.OP_RAW, tol=1e-8, maxit=40000, **kw)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, op + ".txt")
            with gzip.open(os.path.join(ROOT, "tests", "golden", "matrices", op + ".txt.gz"), "rb") as fi, \
                    open(p, "wb") as fo:
                fo.write(fi.read())
            A = la.lsbench_matrix_read(p)
        opts = la.default_opts(tol=1e-10, **kw)
    n = A.nrows
    s = la.Solver(A, opts)
    B = [torch.from_numpy(rhs_drift(n, t)).to("cuda:0") for t in range(steps)]
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    ways = ["cold", "x0"] + ["seq %d" % d for d in depths]

    def a_pass(way, events=False):
        """-> (wall seconds, iterations, statuses, projection us, update us, bytes)"""
        proj, upd, iters, bad, nbytes = [], [], 0, 0, 0
        if way.startswith("seq"):
            s.seq_begin(int(way.split()[1]))
            if events:
                s.seq_last_us  # the first look turns the recording on
        d_x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            if way == "cold":
                r = s.solve_dev(B[t], d_x)
            elif way == "x0":
                r = s.solve_dev(B[t], d_x, warm=True)
            else:
                r = s.solve_seq_dev(B[t], d_x)
                if events:
                    p_us, u_us = s.seq_last_us
                    if p_us > 0.0:
                        proj.append(p_us)
                    if u_us > 0.0:
                        upd.append(u_us)
            iters += r.iters
            bad += r.status != la.STATUS_CONVERGED
        wall = time.perf_counter() - t0
        if way.startswith("seq"):
            nbytes = s.seq_info[3]
            s.seq_begin(0)
        return wall, iters, bad, proj, upd, nbytes

    for way in ways:  # untimed: hints, graphs, the work buffers
        a_pass(way)
    got = {w: [] for w in ways}
    for _ in range(reps):
        for way in ways:
            got[way].append(a_pass(way))
    ev = {w: a_pass(w, events=True) for w in ways if w.startswith("seq")}  # behind the timed passes
    s.destroy()
    med = lambda v: float(np.median(v)) if len(v) else 0.0
    print("%s: n = %d, %d right-hand sides, %d repetitions, tol %.0e" % (config, n, steps, reps, opts.tol))
    print("  %-7s %10s %10s %12s %12s %14s %5s" % ("way", "iterations", "solves/s", "project us", "update us",
                                                    "bytes", "bad"))
    cold_rate = med([steps / g[0] for g in got["cold"]])
    for way in ways:
        g = got[way]
        rate = med([steps / x[0] for x in g])
        print("  %-7s %10d %10.1f %12.1f %12.1f %14d %5d   x %.2f of cold"
              % (way, g[-1][1], rate, med(ev[way][3]) if way in ev else 0.0, med(ev[way][4]) if way in ev else 0.0,
                 g[-1][5],
                 sum(x[2] for x in g), rate / cold_rate))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", help="(internal) run this configuration in this process")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, help="right-hand sides; default: the operator's protocol")
    ap.add_argument("--reps", type=int)
    ap.add_argument("--depths")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.steps, a.reps, [int(d) for d in a.depths.split(",")])
    for config in a.configs.split(","):
        if config not in CONFIGS:
            sys.exit("unknown configuration %r; known: %s" % (config, " ".join(CONFIGS)))
    for config in a.configs.split(","):  # one GPU process at a time; nothing is started behind one that failed
        op = config.split(":")[0]
        steps, reps, depths = PROTOCOL.get(op, (24, 5, "4,8,16"))
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT.get(op, 240)), sys.executable, os.path.abspath(__file__),
                              "--one", config, "--steps", str(a.steps or steps), "--reps", str(a.reps or reps),
                              "--depths", a.depths or depths])
        if rc != 0:
            sys.exit("bench_seq: %s ended with status %d; stopping" % (config, rc))


if __name__ == "__main__":
    main()
