"""Geometric multigrid on grids (LSB_PRECOND_GMG, --precond gmg): the rules of lsb_gmg.c restated in numpy (Hier),
detection and the level plan against the restatement, the cycle's symmetry and definiteness, the iteration counts the
delta rule buys, and on the GPU the kernels of hip_gmg.hip against the same rules in np.longdouble, the plain against
the fused steps bit for bit, solves, refusals and config 3 at full size.

The bound on one application.  z* is the cycle in np.longdouble (64-bit mantissa: its own error is 2^-11 of fp64's
and is left out).  A cycle of `levels` levels with nu sweeps is, on every level, 2 nu + 1 stencil passes (x = w b and
2 nu - 1 sweeps, the residual, the prolongation's add) of a handful of roundings each, whose errors the transfer
operators carry between the levels with norms of order one:

    || z - z* ||_2 <= C_GMG levels (2 nu + 1) eps || z* ||_2,      C_GMG = 3

The coarsest level is a product with a dense inverse formed in fp64, whose error grows with that level's condition
number: the one-level cases, where nothing else is in the count, are the ones that set the constant.  C_GMG is pinned
by test_fp64_restatement_pins_the_constant: the worst ratio of the fp64 restatement over all GPU cases, right-hand
sides and nu = 1, 2, 3 must lie between 1/16 and 1/4 of the bound.  Measured worst ratios, as fractions of the bound:

    restatement: 0.169  ((70, 3), one level of 210 rows, nu = 1, the normal right-hand side)
    device:      0.689  (the same case; (2050, 12) 0.177, (5, 4) 0.120, every other case below 0.1)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lsbench_amd as la
from conftest import ROOT
from lsbench_amd import _lib

EPS = 2.0 ** -52
LD = np.longdouble
C_GMG = 3.0
COARSE_MAX = 4096


# ---- the rules, element for element --------------------------------------------------------------
def plan(dims, coarse=256, max_levels=20):
    """[(n_d), (delta_d)] per level; None where the coarsest level is above 4096 rows"""
    lv = [(tuple(dims), tuple(1.0 for _ in dims))]
    while True:
        n, dl = lv[-1]
        if int(np.prod(n)) <= coarse or min(n) < 4 or len(lv) >= max_levels:
            return lv if int(np.prod(n)) <= COARSE_MAX else None
        lv.append((tuple(m // 2 for m in n),
                   tuple((1.0 + d) / 2 if m % 2 else d / 2 for m, d in zip(n, dl))))


def _axis(a, ax, sl):
    idx = [slice(None)] * a.ndim
    idx[ax] = sl
    return a[tuple(idx)]


class Level:
    """one level: arrays are shaped (nz, ny, nx) / (ny, nx), C order = row (k ny + j) nx + i; axis of dimension d
    is ndim - 1 - d"""

    def __init__(self, n, delta, c, dt):
        self.n, self.delta, self.c, self.dt, self.dim = n, delta, dt(c), dt, len(n)
        self.shape = tuple(reversed(n))
        corr = np.zeros(self.shape, dt)
        for d in range(self.dim):
            last = np.zeros(n[d], dt)
            last[-1] = dt(1) / dt(delta[d]) - dt(1)
            sh = [1] * self.dim
            sh[self.dim - 1 - d] = n[d]
            corr = corr + last.reshape(sh)
        self.D = self.c * (dt(2 * self.dim) + corr)
        omega = dt(4) / dt(5) if self.dim == 2 else dt(6) / dt(7)
        self.w = omega / self.D

    def apply(self, x):
        s = np.zeros(self.shape, self.dt)
        for ax in range(self.dim):
            _axis(s, ax, slice(1, None))[...] += _axis(x, ax, slice(None, -1))
            _axis(s, ax, slice(None, -1))[...] += _axis(x, ax, slice(1, None))
        return self.D * x - self.c * s

    def _p1(self, xc, d):
        """the 1-D rule along dimension d: n' -> n"""
        ax, n, dl = self.dim - 1 - d, self.n[d], self.dt(self.delta[d])
        nc = n // 2
        sh = list(xc.shape)
        sh[ax] = n
        out = np.zeros(sh, self.dt)
        _axis(out, ax, slice(1, 2 * nc, 2))[...] = xc
        pad = list(xc.shape)
        pad[ax] = 1
        z = np.zeros(pad, self.dt)
        e = np.concatenate([z, xc, z], axis=ax)
        half = (_axis(e, ax, slice(None, -1)) + _axis(e, ax, slice(1, None))) / self.dt(2)  # j = 0 .. n'
        nev = (n + 1) // 2
        _axis(out, ax, slice(0, None, 2))[...] = _axis(half, ax, slice(0, nev))
        if n % 2:
            _axis(out, ax, slice(n - 1, n))[...] = _axis(xc, ax, slice(nc - 1, nc)) * (dl / (self.dt(1) + dl))
        return out

    def _r1(self, r, d):
        """its transpose: n -> n'"""
        ax, n, dl = self.dim - 1 - d, self.n[d], self.dt(self.delta[d])
        nc = n // 2
        out = _axis(r, ax, slice(1, 2 * nc, 2)) + _axis(r, ax, slice(0, 2 * nc, 2)) / self.dt(2)
        right = _axis(r, ax, slice(2, 2 * nc + 1, 2))  # fine 2 j + 2: nc of them (n odd) or nc - 1 (n even)
        wr = np.full(right.shape[ax], self.dt(1) / self.dt(2), self.dt)
        if n % 2:
            wr[-1] = dl / (self.dt(1) + dl)
        sh = [1] * self.dim
        sh[ax] = len(wr)
        out = out.copy()
        _axis(out, ax, slice(0, len(wr)))[...] += right * wr.reshape(sh)
        return out

    def prolong(self, xc):
        for d in range(self.dim):
            xc = self._p1(xc, d)
        return xc

    def restrict(self, r):
        for d in range(self.dim):
            r = self._r1(r, d)
        return r * (self.dt(4) / self.dt(2 ** self.dim))

    def dense(self):
        m = int(np.prod(self.n))
        A = np.empty((m, m), self.dt)
        for q in range(m):
            e = np.zeros(m, self.dt)
            e[q] = 1
            A[:, q] = self.apply(e.reshape(self.shape)).ravel()
        return A


class Hier:
    def __init__(self, dims, c=1.0, coarse=256, max_levels=20, dt=np.float64, delta_rule=True):
        self.dims, self.dt = tuple(dims), dt
        lv = plan(dims, coarse, max_levels)
        assert lv is not None
        self.plan = lv
        self.lv = [Level(n, dl if delta_rule else tuple(1.0 for _ in dl), c, dt) for n, dl in lv]
        # the coarsest level: the dense inverse in fp64 (symmetrised, as lsb_amg_coarse_inverse leaves it)
        A64 = Level(lv[-1][0], lv[-1][1] if delta_rule else tuple(1.0 for _ in lv[-1][1]), c, np.float64).dense()
        inv = np.linalg.inv(A64)
        self.cinv = 0.5 * (inv + inv.T)

    def coarse(self, b):
        L = self.lv[-1]
        x = (self.cinv @ b.ravel().astype(np.float64)).astype(self.dt)
        if self.dt is not np.float64:  # the exact solve: refined in the wide format
            for _ in range(4):
                r = b.ravel() - L.apply(x.reshape(L.shape)).ravel()
                x = x + (self.cinv @ r.astype(np.float64)).astype(self.dt)
        return x.reshape(L.shape)

    def vcycle(self, r, nu=1):
        def rec(l, b):
            L = self.lv[l]
            if l == len(self.lv) - 1:
                return self.coarse(b)
            x = L.w * b
            for _ in range(nu - 1):
                x = x + L.w * (b - L.apply(x))
            x = x + L.prolong(rec(l + 1, L.restrict(b - L.apply(x))))
            for _ in range(nu):
                x = x + L.w * (b - L.apply(x))
            return x
        return rec(0, np.asarray(r, self.dt).reshape(self.lv[0].shape)).ravel()


def pcg(L0, b, M, tol, maxit=200):
    """The device's classic PCG (stop test on r.r after the update), the operator applied as the stencil."""
    def S(v):
        return L0.apply(v.reshape(L0.shape)).ravel()
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = r @ z
    thresh2 = tol * tol * (b @ b)
    it = 0
    while it < maxit:
        q = S(p)
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        it += 1
        if r @ r <= thresh2:
            return x, it, 1
        z = M(r)
        rzn = r @ z
        p = z + (rzn / rz) * p
        rz = rzn
    return x, it, 3


def spec_of(dims):
    return ("lap2d:nx=%d,ny=%d" if len(dims) == 2 else "lap3d:nx=%d,ny=%d,nz=%d") % tuple(dims)


def matrix_of(dims, scale=1.0):
    A = la.lsbench_matrix_synth(spec_of(dims))
    if scale == 1.0:
        return A
    return la.Matrix.from_arrays(A.offs.copy(), A.cols.copy(), A.vals * scale, A.base)


# ---- host logic ----------------------------------------------------------------------------------
def test_detection_accepts_the_grid_laplacians():
    rc, g = la.lsb_gmg_detect(la.lsbench_matrix_synth("lap2d:nx=12,ny=9"))
    assert rc == 0 and g == {"dim": 2, "n": (12, 9, 1), "c": 1.0}
    rc, g = la.lsb_gmg_detect(la.lsbench_matrix_synth("lap3d:nx=9,ny=8,nz=7"))
    assert rc == 0 and g == {"dim": 3, "n": (9, 8, 7), "c": 1.0}
    rc, g = la.lsb_gmg_detect(matrix_of((12, 9), 0.375))
    assert rc == 0 and g == {"dim": 2, "n": (12, 9, 1), "c": 0.375}
    rc, g = la.lsb_gmg_detect(matrix_of((9, 8, 7), 0.375))
    assert rc == 0 and g == {"dim": 3, "n": (9, 8, 7), "c": 0.375}


def test_detection_refuses_everything_else(matrix_path):
    for spec in ("lap2d:nx=12,ny=9,coef=3", "lap2d:nx=12,ny=9,conv=0.1", "lap3d:nx=9,ny=8,nz=7,coef=3"):
        rc, g = la.lsb_gmg_detect(la.lsbench_matrix_synth(spec))
        assert rc != 0 and g is None, spec
    for name in ("xn3b_A_18", "I1_05x05"):
        rc, g = la.lsb_gmg_detect(la.lsbench_matrix_read(matrix_path(name)))
        assert rc != 0 and g is None, name
    A = la.lsbench_matrix_synth("lap2d:nx=12,ny=9")
    vals = A.vals.copy()
    vals[vals > 0] += 1e-3  # a grid whose diagonal is 4 c + 1e-3
    assert la.lsb_gmg_detect(la.Matrix.from_arrays(A.offs.copy(), A.cols.copy(), vals, A.base))[0] == 4
    # a 1-D operator
    n = 40
    offs = np.cumsum([0] + [2 if i in (0, n - 1) else 3 for i in range(n)])
    cols = np.concatenate([[j for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)])
    vals = np.where(cols == np.repeat(np.arange(n), np.diff(offs)), 2.0, -1.0)
    assert la.lsb_gmg_detect(la.Matrix.from_arrays(offs, cols, vals))[0] != 0


@pytest.mark.parametrize("dims", [(12, 9), (33, 20), (1024, 1000), (3162, 3162), (9, 8, 7), (400, 400, 400),
                                  (3162, 8)])
def test_plan_equals_the_restatement(dims):
    for coarse, cap in ((256, 20), (8, 20), (256, 3)):
        want = plan(dims, coarse, cap)
        got = la.lsb_gmg_plan(dims, coarse, cap)
        assert got == want, (dims, coarse, cap)
    assert la.lsb_gmg_plan((30000, 4)) is None and plan((30000, 4)) is None  # a very thin grid: refused


@pytest.mark.parametrize("dims", [(12, 9), (10, 7, 6)])
def test_cycle_is_symmetric_positive_definite(dims):
    n = int(np.prod(dims))
    for nu in (1, 2):
        H = Hier(dims, coarse=8)
        assert len(H.lv) >= 2
        M = np.column_stack([H.vcycle(e, nu) for e in np.eye(n)])
        asym = np.abs(M - M.T).max() / np.abs(M).max()
        lam = np.linalg.eigvalsh(0.5 * (M + M.T))
        print("%s nu=%d: asymmetry %.2e, eigenvalues of M^-1 in [%.3e, %.3e]" % (dims, nu, asym, lam[0], lam[-1]))
        assert asym <= 1e-14 and lam[0] > 0


@pytest.mark.parametrize("dims", [(64, 64), (253, 190), (1000, 1000), (1024, 1024), (100, 100, 100)])
def test_pcg_iterations_stay_flat(dims):
    n = int(np.prod(dims))
    b = np.arange(n, dtype=np.float64)
    H = Hier(dims)
    x, it, st = pcg(H.lv[0], b, H.vcycle, 1e-8)
    print("%s: %d levels, %d GMG-PCG iterations" % (dims, len(H.lv), it))
    assert st == 1 and it <= 16
    assert np.linalg.norm(b - H.lv[0].apply(x.reshape(H.lv[0].shape)).ravel()) <= 1e-7 * np.linalg.norm(b)


def test_pcg_needs_the_delta_rule():
    """plain rediscretisation (delta = 1 on every level) on an even size: well above the 16 the rule keeps"""
    dims = (256, 256)
    b = np.arange(int(np.prod(dims)), dtype=np.float64)
    H = Hier(dims, delta_rule=False)
    _, it, _ = pcg(H.lv[0], b, H.vcycle, 1e-8)
    H = Hier(dims)
    _, it_rule, _ = pcg(H.lv[0], b, H.vcycle, 1e-8)
    print("256 x 256: %d iterations without the delta rule, %d with it" % (it, it_rule))
    assert it_rule <= 16 < it


# ---- the cases of the GPU tests, and the constant ------------------------------------------------
# (grid, amg_coarse, scale of the values)
CASES = [((12, 9), 8, 1.0), ((33, 20), 8, 1.0), ((129, 67), 256, 1.0), ((5, 4), 256, 1.0), ((70, 3), 256, 1.0),
         ((2050, 12), 256, 1.0), ((9, 8, 7), 16, 1.0), ((24, 20, 18), 256, 1.0), ((17, 16, 33), 256, 1.0),
         ((65, 5, 4), 256, 1.0), ((33, 20), 8, 0.375)]
NUS = (1, 2, 3)
_REF = {}


def rhs3(n):
    i = np.arange(n, dtype=np.float64)
    return [np.sin(i) + 0.5, np.ones(n), np.random.default_rng(20240607).standard_normal(n)]


def reference(case):
    """per nu: the three right-hand sides' z in longdouble (rounded to fp64 only for the comparison's norm), the
    fp64 restatement's, and the number of levels; computed once"""
    if case not in _REF:
        dims, coarse, scale = case
        Hl, H = Hier(dims, c=scale, coarse=coarse, dt=LD), Hier(dims, c=scale, coarse=coarse)
        R = rhs3(int(np.prod(dims)))
        _REF[case] = {nu: ([Hl.vcycle(r.astype(LD), nu) for r in R], [H.vcycle(r, nu) for r in R], len(H.lv))
                      for nu in NUS}
    return _REF[case]


def bound(zs, levels, nu):
    return C_GMG * levels * (2 * nu + 1) * EPS * float(np.sqrt((zs * zs).sum()))


def ratio(z, zs, levels, nu):
    d = z.astype(LD) - zs
    return float(np.sqrt((d * d).sum())) / bound(zs, levels, nu)


def test_fp64_restatement_pins_the_constant():
    worst, at = 0.0, None
    for case in CASES:
        ref = reference(case)
        for nu in NUS:
            zl, z64, levels = ref[nu]
            for k in range(3):
                q = ratio(z64[k], zl[k], levels, nu)
                if q > worst:
                    worst, at = q, (case, nu, k)
    print("fp64 restatement: worst ratio %.3f of the bound at %s" % (worst, at))
    assert 1.0 / 16 <= worst <= 1.0 / 4


def test_one_level_is_the_exact_solve():
    Hl = Hier((5, 4), dt=LD)
    assert len(Hl.lv) == 1
    r = rhs3(20)[0].astype(LD)
    z = Hl.vcycle(r)
    assert np.abs(Hl.lv[0].apply(z.reshape(4, 5)).ravel() - r).max() <= 1e-17


def test_options_and_surface():
    assert la.PRECOND_GMG == 7
    lib = _lib.load()
    o = la.default_opts()
    assert lib.hip_cdna4_set_option(b"precond", b"gmg") == 0
    got = _lib.Opts()
    lib.lsb_hip_get_opts(C.byref(got))
    assert got.precond == 7
    lib.lsb_hip_set_opts(C.byref(o))
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    r = subprocess.run([drv, "--help"], capture_output=True, text=True)
    assert "gmg" in r.stdout
    # the options struct is what it was: no new member, the same tail
    names = [f[0] for f in _lib.Opts._fields_]
    assert names[-8:] == ["amg_theta", "amg_sweeps", "amg_coarse", "amg_max_levels", "amg_tail_rows", "amg_precision",
                          "amg_smoother", "amg_cheb_ratio"] and len(names) == 34
    assert _lib.Opts._TAIL == {"fsai_blocks": (0, C.c_int)} and _lib.Opts._TAIL_BYTES == 8
    assert C.sizeof(_lib.Opts) == _lib.Opts.amg_cheb_ratio.offset + 8


# ---- GPU -----------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def _apply(s, r):
    """z = M^-1 r through precond_dev into a NaN-filled buffer, twice: no NaN left, the same bits"""
    import torch
    d_r = _dev(r)
    d_z = torch.full((len(r),), float("nan"), dtype=torch.float64, device="cuda:0")
    s.precond_dev(d_r, d_z)
    z1 = d_z.cpu().numpy()
    d_z.fill_(float("nan"))
    s.precond_dev(d_r, d_z)
    z2 = d_z.cpu().numpy()
    assert np.isfinite(z1).all() and np.array_equal(z1, z2)
    return z1


def _gmg_opts(hip, **kw):
    return hip.default_opts(op_mode=hip.OP_RAW, precond=hip.PRECOND_GMG, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%g-%g" % ("x".join(map(str, c[0])), c[1], c[2]))
def test_hip_cycle_matches_longdouble(hip, monkeypatch, case):
    """precond_dev against the longdouble cycle within the bound, bitwise repeatable, the plain and the fused steps
    the same bits, the levels the plan's; (2050, 12) also line-padded, the pad rows of z exactly 0."""
    import torch
    dims, coarse, scale = case
    A = matrix_of(dims, scale)
    n = A.nrows
    R = rhs3(n)
    ref = reference(case)
    want = plan(dims, coarse)
    worst = 0.0
    for pad in (("0", "1") if dims == (2050, 12) else ("0",)):
        monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", pad)
        for nu in NUS:
            zl, _, levels = ref[nu]
            Z = {}
            for fuse in ("0", "1"):
                monkeypatch.setenv("LSBENCH_HIP_GMG_FUSE", fuse)
                s = hip.Solver(A, _gmg_opts(hip, amg_sweeps=nu, amg_coarse=coarse))
                assert bool(s.padded) == (pad == "1") and s.n_local == n
                lev, gdims, pitch = s.gmg_info
                assert lev == levels == len(want) and gdims == tuple(dims) + (1,) * (3 - len(dims))
                assert pitch == (dims[0] if pad == "0" else -(-dims[0] // 128) * 128)
                for l, (nl, dl) in enumerate(want):
                    gn, gd = s.gmg_level(l)
                    assert gn[:len(dims)] == nl and gd[:len(dims)] == dl
                assert s.gmg_level(lev) is None and s.gmg_cycle_bytes > 0 and s.amg_cycle_bytes == 0
                Z[fuse] = [_apply(s, r) for r in R]
                if pad == "1":  # in the solver's own numbering: the pad rows of z are exactly 0, the others the same
                    assert s.padded == (pitch - dims[0]) * dims[1]
                    rp = np.zeros((dims[1], pitch))
                    rp[:, :dims[0]] = R[0].reshape(dims[1], dims[0])
                    zp = torch.full((pitch * dims[1],), float("nan"), dtype=torch.float64, device="cuda:0")
                    s.precond_padded_dev(_dev(rp.ravel()), zp)
                    zp = zp.cpu().numpy().reshape(dims[1], pitch)
                    assert np.array_equal(zp[:, dims[0]:], np.zeros((dims[1], pitch - dims[0])))
                    assert not np.signbit(zp[:, dims[0]:]).any()
                    assert np.array_equal(zp[:, :dims[0]].ravel(), Z[fuse][0])
                s.destroy()
            for k in range(3):
                assert np.array_equal(Z["0"][k], Z["1"][k]), (nu, k)
                q = ratio(Z["1"][k], zl[k], levels, nu)
                worst = max(worst, q)
                assert q <= 1.0, (pad, nu, k, q)
        if len(want) == 1:  # one level: z = A^-1 r
            L0 = Hier(dims, c=scale, coarse=coarse, dt=LD).lv[0]
            res = L0.apply(Z["1"][0].astype(LD).reshape(L0.shape)).ravel() - R[0]
            assert np.abs(res).max() <= 1e-12 * np.abs(R[0]).max()
    print("%s: device worst ratio %.3f of the bound" % (case, worst))


@pytest.mark.gpu
def test_hip_padded_cycle_leaves_the_pad_rows_zero(hip, monkeypatch):
    """(2050, 12) line-padded: a solve's x is gathered back from the padded numbering, and a NaN or a non-zero on a
    pad row of z would reach the real rows through the next direction; the padded and the unpadded solver agree on
    z bit for bit (the fine-level kernels index by pitch, nothing else differs)."""
    dims = (2050, 12)
    A = matrix_of(dims)
    R = rhs3(A.nrows)
    Z = {}
    for pad in ("0", "1"):
        monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", pad)
        s = hip.Solver(A, _gmg_opts(hip))
        assert bool(s.padded) == (pad == "1")
        Z[pad] = [_apply(s, r) for r in R]
        x, r = s.solve(R[0])
        assert r.status == hip.STATUS_CONVERGED and np.isfinite(x).all()
        s.destroy()
    for k in range(3):
        assert np.array_equal(Z["0"][k], Z["1"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(129, 67), (24, 20, 18)])
def test_hip_cycle_is_symmetric_and_definite(hip, monkeypatch, dims):
    """|u . M^-1 v - v . M^-1 u| within what the bounds of the two applications and the two host dots allow, the
    allowance of test_precond_apply.py; r . M^-1 r > 0."""
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    A = matrix_of(dims)
    n = A.nrows
    u, v = rhs3(n)[0], rhs3(n)[2]
    s = hip.Solver(A, _gmg_opts(hip))
    levels = s.gmg_info[0]
    zu, zv = _apply(s, u), _apply(s, v)
    s.destroy()
    bn = [C_GMG * levels * 3 * EPS * np.linalg.norm(z) for z in (zu, zv)]
    slack = np.linalg.norm(u) * bn[1] + np.linalg.norm(v) * bn[0]
    slack += (n + 2) * EPS * (abs(u) @ abs(zv) + abs(v) @ abs(zu))
    asym = abs(u @ zv - v @ zu)
    print("%s: |u.M^-1 v - v.M^-1 u| / allowed %.3g" % (dims, asym / slack))
    assert asym <= slack and u @ zu > 0 and v @ zv > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(300, 300), (24, 20, 18), (2050, 12)])
def test_hip_gmg_pcg_follows_numpy(hip, monkeypatch, dims):
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1" if dims == (2050, 12) else "0")
    A = matrix_of(dims)
    n = A.nrows
    b = np.arange(n, dtype=np.float64)
    H = Hier(dims)
    xr, itr, st = pcg(H.lv[0], b, H.vcycle, 1e-10)
    x5, it5, st5 = pcg(H.lv[0], b, H.vcycle, 1e-10, maxit=5)
    assert st == 1 and (it5, st5) == (5, 3)
    for graph in (0, 1):
        s = hip.Solver(A, _gmg_opts(hip, tol=1e-10, use_graph=graph))
        assert bool(s.padded) == (dims == (2050, 12))
        x, r = s.solve(b)
        x2, r2 = s.solve(b)
        print("%s graph=%d: %d iterations (numpy %d), relres %.2e" % (dims, graph, r.iters, itr, r.relres))
        assert r.status == hip.STATUS_CONVERGED and np.array_equal(x, x2) and r.iters == r2.iters
        assert abs(int(r.iters) - itr) <= max(2, 0.04 * itr), (r.iters, itr)
        assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
        # a warm start from the solution, and the sequence of right-hand sides, return it
        xw, rw = s.solve(b, x0=x)
        assert rw.status == hip.STATUS_CONVERGED and np.linalg.norm(xw - x) <= 1e-10 * np.linalg.norm(x)
        s.seq_begin(2)
        xs, rs = s.solve_seq(b)
        xs2, rs2 = s.solve_seq(b)
        assert rs.status == rs2.status == hip.STATUS_CONVERGED
        assert np.linalg.norm(xs - x) <= 1e-10 * np.linalg.norm(x) and np.linalg.norm(xs2 - x) <= 1e-10 * np.linalg.norm(x)
        s.destroy()
        s = hip.Solver(A, _gmg_opts(hip, tol=1e-10, use_graph=graph, maxit=5))
        x, r = s.solve(b)
        s.destroy()
        assert r.status == hip.STATUS_MAXIT and r.iters == 5
        assert np.linalg.norm(x - x5) <= 1e-9 * np.linalg.norm(x5)
    s = hip.Solver(A, _gmg_opts(hip, tol=1e-10, verify=1))
    x, r = s.solve(b)
    s.destroy()
    assert r.status == hip.STATUS_CONVERGED and r.true_relres <= 1e-10


@pytest.mark.gpu
def test_hip_gmg_refusals(hip, matrix_path):
    import torch
    drv = os.path.join(ROOT, "lsbench_amd", "csrc", "driver")
    grid = ["--matrix", "synth:lap2d:nx=40,ny=30", "--operator", "raw"]

    def refused(args, text):
        r = subprocess.run([drv, "--solver", "hip", "--precond", "gmg", "--trials=1"] + args, capture_output=True,
                           text=True)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr[-400:])
    refused(["--matrix", matrix_path("xn3b_A_18")], "constant-coefficient grid")
    refused(["--matrix", "synth:lap2d:nx=40,ny=30,coef=3", "--operator", "raw"], "constant-coefficient grid")
    # shards: --nvirt here.  --ngpus and a distributed solver need more than the one GPU of the test machine; they reach
    # the same refusal through gmg_check's `sharded` flag (lsb_hip_solver_create_dist) and precond_shard_gmg's test of
    # the shard's row range.  --precision fp32 and mixed precision are one enum value (LSB_PREC_MIXED).
    refused(grid + ["--nvirt", "2"], "one shard")
    refused(grid + ["--reorder", "1"], "re-ordered")
    for k in ("gmres", "bicgstab", "cg1", "richardson"):
        refused(grid + ["--krylov", k], "classic PCG")
    refused(grid + ["--precision", "fp32"], "fp64")
    refused(["--matrix", "synth:lap2d:nx=30000,ny=4", "--operator", "raw"], "too thin")
    r = subprocess.run([drv, "--solver", "hip", "--precond", "gmg", "--trials=2"] + grid, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rec = r.stdout.splitlines()
    f = rec[rec.index("===hip_cdna4:iterations,relres,status,tol,solves_per_sec,nshards===") + 1].split(",")
    assert int(f[2]) == 1 and 0 < int(f[0]) <= 20
    # the block entry points answer 2
    A = matrix_of((40, 30))
    n = A.nrows
    s = hip.Solver(A, _gmg_opts(hip))
    lib = _lib.load()
    B = torch.ones((2, n), dtype=torch.float64, device="cuda:0")
    X = torch.zeros((2, n), dtype=torch.float64, device="cuda:0")
    args = (s._h, 2, B.data_ptr(), n, X.data_ptr(), n)
    for fn in ("lsb_hip_solver_solve_multi_dev", "lsb_hip_solver_solve_block_dev",
               "lsb_hip_solver_solve_block_precond_dev", "lsb_hip_solver_amg_solve_multi_dev"):
        assert getattr(lib, fn)(*args, None) == 2, fn
    for fn in ("lsb_hip_solver_precond_multi_dev", "lsb_hip_solver_amg_cycle_multi_dev"):
        assert getattr(lib, fn)(*args) == 2, fn
    assert s.amg_precision is None
    s.destroy()
    s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW))
    assert s.gmg_info is None and s.gmg_level(0) is None and s.gmg_cycle_bytes == 0
    s.destroy()


@pytest.mark.gpu
def test_hip_gmg_full_size(hip):
    """Config 3: the 5-point operator on 3162 x 3162 points, tol 1e-8."""
    A = hip.lsbench_matrix_synth("lap2d:nx=3162,ny=3162")
    n = A.nrows
    b = np.arange(n, dtype=np.float64)
    s = hip.Solver(A, _gmg_opts(hip, tol=1e-8))
    lev, dims, pitch = s.gmg_info
    x, r = s.solve(b)
    s.destroy()
    L0 = Level((3162, 3162), (1.0, 1.0), 1.0, np.float64)
    res = np.linalg.norm(b - L0.apply(x.reshape(L0.shape)).ravel()) / np.linalg.norm(b)
    print("config 3 GMG-PCG: %d levels, pitch %d, %d iterations, %.3f s, true relres %.2e"
          % (lev, pitch, r.iters, r.seconds, res))
    assert r.status == 1 and res <= 1e-8 and r.iters <= 16
