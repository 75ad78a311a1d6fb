"""Successive right-hand sides: the two families of right-hand sides that the tests and tools/bench_seq.py share, and
the numpy model the device is compared with -- Jacobi-PCG with the project's stop rule, the projection on an
S-orthonormal basis of earlier solutions, the update with two Gram-Schmidt passes and Fischer's restart, as
include/lsbench_hip.h states them for lsb_hip_solver_solve_seq.  No test in here; numpy only."""
import math

import numpy as np

CONVERGED, BREAKDOWN, MAXIT = 1, 2, 3


def rhs_drift(n, t):
    """b_t,i = i (1 + 0.1 sin 0.3 t) + n sin 2 pi (s + 0.02 t) + 0.3 n cos(6 pi s (1 + 0.01 t)), s = i / n"""
    i = np.arange(n, dtype=np.float64)
    s = i / n
    return i * (1.0 + 0.1 * math.sin(0.3 * t)) + n * np.sin(2.0 * np.pi * (s + 0.02 * t)) + \
        0.3 * n * np.cos(6.0 * np.pi * s * (1.0 + 0.01 * t))


def rhs_3d(n, t):
    """b_t = v0 (1 + 0.1 t) + v1 sin(0.7 t + 0.2) + v2 cos 1.3 t with v0 = i, v1 = n sin 2 pi s, v2 = n cos 6 pi s"""
    i = np.arange(n, dtype=np.float64)
    s = i / n
    return i * (1.0 + 0.1 * t) + n * np.sin(2.0 * np.pi * s) * math.sin(0.7 * t + 0.2) + \
        n * np.cos(6.0 * np.pi * s) * math.cos(1.3 * t)


def pcg_from(S, dinv, b, x0, tol, maxit=20000):
    """Jacobi-PCG for S x = b from x0 (None: from zero), stopped at ||r|| <= tol ||b|| -- never relative to
    ||b - S x0||.  -> (x, e = x - x0, iters, status, start = ||b - S x0|| / ||b||)"""
    bb = float(b @ b)
    if bb == 0.0:
        return np.zeros(len(b)), np.zeros(len(b)), 0, CONVERGED, 0.0
    x = np.zeros(len(b)) if x0 is None else x0.copy()
    r = b.copy() if x0 is None else b - S @ x0
    rr = float(r @ r)
    start = math.sqrt(rr / bb)
    if x0 is not None and tol > 0.0 and rr <= tol * tol * bb:
        return x, np.zeros(len(b)), 0, CONVERGED, start
    p = dinv * r
    rz = float(r @ p)
    it, status = 0, MAXIT
    while it < maxit:
        q = S @ p
        pq = float(p @ q)
        if pq == 0.0 or not np.isfinite(pq):
            status = BREAKDOWN
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        rz_new, rr = float(r @ z), float(r @ r)
        it += 1
        if rr <= tol * tol * bb:
            status = CONVERGED
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, (x if x0 is None else x - x0), it, status, start


class SeqModel:
    """A solver with a basis of `depth` earlier solutions: solve(b) is lsb_hip_solver_solve_seq."""

    def __init__(self, S, depth, tol):
        self.S, self.depth, self.tol = S.tocsr(), depth, tol
        self.dinv = 1.0 / S.diagonal()
        self.X, self.SX, self.restarts = [], [], 0

    @property
    def held(self):
        return len(self.X)

    def solve(self, b):
        """-> dict(x, iters, status, start)"""
        if not self.X:
            x0 = None
        else:
            X = np.array(self.X)
            x0 = X.T @ (X @ b)
        x, e, iters, status, start = pcg_from(self.S, self.dinv, b, x0, self.tol)
        if status == CONVERGED and iters > 0 and self.tol > 0.0:
            self._update(x, e)
        return dict(x=x, iters=iters, status=status, start=start)

    def _update(self, x, e):
        d = e.copy()
        if self.held == self.depth:  # Fischer's restart: the whole current solution
            self.X, self.SX, d = [], [], x.copy()
            self.restarts += 1
        w = self.S @ d
        if self.X:
            X, SX = np.array(self.X), np.array(self.SX)
            for _ in range(2):
                beta = X @ w
                d -= X.T @ beta
                w -= SX.T @ beta
        nu = float(d @ w)
        if np.isfinite(nu) and nu > 0.0:
            self.X.append(d / math.sqrt(nu))
            self.SX.append(w / math.sqrt(nu))

    def orthonormality(self):
        """max |X^T (S X) - I|"""
        X, SX = np.array(self.X), np.array(self.SX)
        return float(np.abs(X @ SX.T - np.eye(len(X))).max())


def run_model(S, depth, tol, family, steps):
    """(iters, start) per step of `steps` solves of family(n, t), t = 0 .., and the model"""
    m = SeqModel(S, depth, tol)
    out = [m.solve(family(S.shape[0], t)) for t in range(steps)]
    return [o["iters"] for o in out], [o["start"] for o in out], m
