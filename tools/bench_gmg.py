#!/usr/bin/env python3
"""Geometric multigrid (--precond gmg) against AMG and Jacobi on one MI355X, by the driver's protocol.

bench.py's preconditioner list is fixed, so this is the measurement of GMG-PCG.  Every figure comes from a FRESH
process: the driver itself (`driver --solver hip --operator raw --tol T --trials N`: N warm-up solves, then N timed
ones), `--repeats` times per configuration, one JSON line per run on stdout:

  * config 3 (lap2d 3162 x 3162) and config 4 (lap3d 400^3): gmg at nu = 1 with the fused steps (the default) and
    with the plain ones (LSBENCH_HIP_GMG_FUSE=0), gmg at nu = 2, amg, amg with the fp32 cycle (config 3), jacobi --
    iterations, status, relres, solves per second;
  * one ungraphed application of the cycle through precond_dev against gmg_cycle_bytes, nu = 1 fused, nu = 1 plain
    and nu = 2 (a child of this script each; the entry point's own two copies of n doubles are in the time and are
    added to the bytes);
  * the refusal of an operator that is no grid (tests/golden's xn3b_A_18).

A child that ends in any way but the expected one ends the script: nothing more is started on that GPU.

Usage: python tools/bench_gmg.py [--repeats 3] [--tol 1e-8] [--only cfg3,cfg4,apply,refuse] [--skip cfg4:amg]
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRV = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
SPECS = {"cfg3": "lap2d:nx=3162,ny=3162", "cfg4": "lap3d:nx=400,ny=400,nz=400"}
# name -> (driver flags, trials: a solve of milliseconds wants more of them than one of seconds, environment)
RUNS = {
    "gmg-nu1": (["--precond", "gmg", "--amg-sweeps", "1"], 20, {}),
    "gmg-nu1-plain": (["--precond", "gmg", "--amg-sweeps", "1"], 20, {"LSBENCH_HIP_GMG_FUSE": "0"}),
    "gmg-nu2": (["--precond", "gmg", "--amg-sweeps", "2"], 20, {}),
    "amg": (["--precond", "amg"], 5, {}),
    "amg-fp32": (["--precond", "amg", "--amg-precision", "fp32"], 5, {}),
    "jacobi": (["--precond", "jacobi"], 2, {}),
}
STOP = "a child process hung, died or failed: nothing more is started on this GPU"


def driver(spec, flags, trials, tol, limit, env):
    cmd = [DRV, "--solver", "hip", "--matrix", "synth:" + spec, "--operator", "raw", "--tol", repr(tol),
           "--trials=%d" % trials] + flags
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        return {"timeout_s": limit}
    out = {"rc": r.returncode, "wall_s": round(time.time() - t0, 1)}
    lines = r.stdout.splitlines()
    head = "===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards==="
    if r.returncode == 0 and head in lines:
        f = lines[lines.index(head) + 1].split(",")
        out.update(iterations=int(f[0]), relres=float(f[1]), status=int(f[2]), solves_per_sec=float(f[4]))
    else:
        out["stderr"] = r.stderr[-300:]
    return out


def apply_child(spec, nu, reps):  # (LSBENCH_HIP_GMG_FUSE is the parent's to set)
    """one solver, the cycle through precond_dev: us per application, the model's bytes"""
    import numpy as np
    import torch

    import lsbench_amd as la
    torch.cuda.set_device(0)
    rc = la.hip_cdna4_init()
    assert rc == 0 or la._lib.load().lsb_hip_stream()
    M = la.lsbench_matrix_synth(spec)
    n = M.nrows
    s = la.Solver(M, la.default_opts(op_mode=la.OP_RAW, precond=la.PRECOND_GMG, amg_sweeps=nu, use_graph=0))
    d_r = torch.arange(n, dtype=torch.float64, device="cuda:0")
    d_z = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    for _ in range(3):
        s.precond_dev(d_r, d_z)
    us = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.precond_dev(d_r, d_z)  # (ends in a synchronise of the solver's stream)
        us.append((time.perf_counter() - t0) * 1e6)
    lev, dims, pitch = s.gmg_info
    copies = 32 * (n + int(s.padded))
    by = s.gmg_cycle_bytes
    med = float(np.median(us))
    print(json.dumps({"apply": spec, "nu": nu, "fuse": os.environ.get("LSBENCH_HIP_GMG_FUSE", "1"), "levels": lev, "pitch": pitch, "gmg_cycle_bytes": by,
                      "entry_point_copy_bytes": copies, "us_median": round(med, 1), "us_min": round(min(us), 1),
                      "us_max": round(max(us), 1), "GBps_model_plus_copies": round((by + copies) / med * 1e-3, 1)}),
          flush=True)
    s.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--only", default="cfg3,cfg4,apply,refuse")
    ap.add_argument("--skip", default="", help="comma list of cfg:run, e.g. cfg4:amg")
    ap.add_argument("--limit", type=int, default=400, help="seconds one driver process may take")
    ap.add_argument("--apply-child", nargs=2, metavar=("SPEC", "NU"))
    a = ap.parse_args()
    if a.apply_child:
        apply_child(a.apply_child[0], int(a.apply_child[1]), 20)
        return
    only, skip = a.only.split(","), set(a.skip.split(","))
    if "refuse" in only:
        with tempfile.TemporaryDirectory(prefix="lsb_gmg_") as tmp:
            path = os.path.join(tmp, "xn3b_A_18.txt")
            with gzip.open(os.path.join(ROOT, "tests", "golden", "matrices", "xn3b_A_18.txt.gz"), "rb") as fi, \
                    open(path, "wb") as fo:
                fo.write(fi.read())
            r = subprocess.run([DRV, "--solver", "hip", "--matrix", path, "--precond", "gmg", "--trials=1"],
                               capture_output=True, text=True, timeout=120)
        refused = r.returncode == 1 and "constant-coefficient grid" in r.stderr
        print(json.dumps({"refusal": "xn3b_A_18", "rc": r.returncode, "refused": refused,
                          "message": r.stderr.strip().splitlines()[-1][:200] if r.stderr.strip() else ""}), flush=True)
        if not refused:  # it ran, or it ended some other way
            sys.exit(STOP)
    for cfg in ("cfg3", "cfg4"):
        if cfg not in only:
            continue
        for name, (flags, trials, env) in RUNS.items():
            if "%s:%s" % (cfg, name) in skip or (cfg == "cfg4" and name == "amg-fp32"):
                continue
            for rep in range(a.repeats):
                rec = {"config": cfg, "operator": SPECS[cfg], "run": name, "repeat": rep, "tol": a.tol, "trials": trials}
                rec.update(driver(SPECS[cfg], flags, trials, a.tol, a.limit, env))
                print(json.dumps(rec), flush=True)
                if rec.get("rc") != 0:  # a time limit included
                    sys.exit(STOP)
    if "apply" in only:
        for cfg in ("cfg3", "cfg4"):
            for nu, fuse in ((1, "1"), (1, "0"), (2, "1")):
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--apply-child", SPECS[cfg], str(nu)],
                                        timeout=a.limit, env=dict(os.environ, LSBENCH_HIP_GMG_FUSE=fuse)).returncode
                except subprocess.TimeoutExpired:
                    rc = None
                if rc != 0:
                    print(json.dumps({"apply": SPECS[cfg], "nu": nu, "fuse": fuse, "rc": rc}), flush=True)
                    sys.exit(STOP)


if __name__ == "__main__":
    main()
