#!/usr/bin/env python3
"""The direct solver (opts.krylov = KRYLOV_DIRECT) against the iterative forms on one MI355X.

The reference's protocol: factorise once, untimed, then time solves (src/cholmod-impl.h:25-26, 59-62).  Per operator,
in ONE process, one solver per form, `--reps` (5) times alternating between
  direct_1      the direct solver at tol 0, maxit 1 (one round: the reference's direct protocol)
  direct_tol    the direct solver at --tol (1e-12): rounds until the recomputed residual meets it
  fsai3         FSAI(3)-PCG
  bj_dense      one-block block-Jacobi PCG (block_size >= n: a dense inverse inside the PCG loop)
  jacobi        Jacobi-PCG
`--solves` (200) solve_dev calls of b_i = i per repetition, after `--warm` (20) untimed ones (the second solve of a
solver enqueues the first one's count in one go and, under use_graph, builds its graph).  Times are a host clock
around work that ends in a device synchronise.  One JSON line on stdout: per operator and form
  solves_per_s   [min, max] over the repetitions
  us_per_solve   [min, max]
  iters          iterations (rounds) of a solve, and us_per_iter = us_per_solve / iters, [min, max]
  relres         what the last solve reported (-1: nothing recomputed), true_relres: ||b - S x|| / ||b|| on the host
create_s is what creating the solver took (the direct solver: ordering, factor and upload).  For the direct solver also
its entries, tree height and bytes per round; "beats_fsai3" / "beats_bj_dense": its slowest repetition is faster than
the fastest of FSAI(3)-PCG / of the dense inverse.  Progress goes to stderr.

Usage: python tools/bench_direct.py [--operators xn3b_A_18,tj7a_A_12] [--reps 5] [--solves 200] [--warm 20]
                                    [--tol 1e-12]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", default="xn3b_A_18,tj7a_A_12")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-12)
    a = ap.parse_args()
    import scipy.sparse as sp
    import torch

    import lsbench_amd as la
    assert la.hip_cdna4_init() == 0, "needs an MI355X"
    out = {}
    with tempfile.TemporaryDirectory(prefix="lsb_direct_") as tmp:
        for name in a.operators.split(","):
            A = file_matrix(la, name, tmp)
            S = la.lsb_csr_symmetrize_upper(A)
            n = A.nrows
            Ss = sp.csr_matrix((np.array(S.vals), np.array(S.cols, np.int64) - S.base, np.array(S.offs, np.int64)),
                               shape=(n, n))
            forms = {
                "direct_1": dict(krylov=la.KRYLOV_DIRECT, tol=0.0, maxit=1),
                "direct_tol": dict(krylov=la.KRYLOV_DIRECT, tol=a.tol),
                "fsai3": dict(precond=la.PRECOND_FSAI, fsai_power=3, tol=a.tol),
                "bj_dense": dict(precond=la.PRECOND_BLOCKJACOBI, block_size=n, tol=a.tol),
                "jacobi": dict(precond=la.PRECOND_JACOBI, tol=a.tol),
            }
            b = np.arange(n, dtype=np.float64)
            d_b = torch.from_numpy(b).to("cuda:0")
            d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
            solvers, rec = {}, {}
            for f, kw in forms.items():
                t0 = time.perf_counter()
                solvers[f] = la.Solver(A, la.default_opts(**kw))
                rec[f] = {"create_s": time.perf_counter() - t0, "t": []}
                for _ in range(a.warm):
                    res = solvers[f].solve_dev(d_b, d_x)
                torch.cuda.synchronize()
                x = d_x.cpu().numpy()
                rec[f].update(iters=int(res.iters), status=int(res.status), relres=float(res.relres),
                              true_relres=float(np.linalg.norm(b - Ss @ x) / np.linalg.norm(b)))
                print(name, f, "iters", res.iters, "status", res.status, "relres", res.relres, "true",
                      rec[f]["true_relres"], file=sys.stderr, flush=True)
            for rep in range(a.reps):
                for f in forms:
                    s = solvers[f]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.solves):
                        s.solve_dev(d_b, d_x)
                    torch.cuda.synchronize()
                    rec[f]["t"].append((time.perf_counter() - t0) / a.solves)
                print(name, "rep", rep, {f: "%.0f/s" % (1.0 / rec[f]["t"][-1]) for f in forms}, file=sys.stderr,
                      flush=True)
            res = {}
            for f in forms:
                t = rec[f].pop("t")
                it = max(rec[f]["iters"], 1)
                res[f] = dict(rec[f], solves_per_s=[1.0 / max(t), 1.0 / min(t)],
                              us_per_solve=[1e6 * min(t), 1e6 * max(t)],
                              us_per_iter=[1e6 * min(t) / it, 1e6 * max(t) / it])
                if f.startswith("direct"):
                    e, h, by = solvers[f].direct_info
                    res[f].update(entries=e, height=h, bytes_per_round=by)
            for f in ("direct_1", "direct_tol"):
                res[f]["beats_fsai3"] = bool(res[f]["solves_per_s"][0] > res["fsai3"]["solves_per_s"][1])
                res[f]["beats_bj_dense"] = bool(res[f]["solves_per_s"][0] > res["bj_dense"]["solves_per_s"][1])
            for s in solvers.values():
                s.destroy()
            out[name] = dict(n=n, nnz=int(A.nnz), forms=res)
    print(json.dumps({"bench": "direct", "reps": a.reps, "solves": a.solves, "tol": a.tol, "operators": out}))


if __name__ == "__main__":
    main()
