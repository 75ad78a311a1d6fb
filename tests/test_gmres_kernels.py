"""The GMRES(m) kernels of lsbench_amd/csrc/hip_gmres.hip one by one, each
against its rule restated in numpy longdouble.

The end-to-end tests of test_gmres.py cannot see an error inside the Arnoldi
loop: the second Gram-Schmidt pass removes most of a wrong coefficient of the
first, a slightly skew basis costs only iterations, and every restart
recomputes r = b - A x.  Here every launcher is called on its own through
ctypes, as the driver (hip_gmres_drv.c) calls it, on inputs of mixed sign and
magnitude (1e-3 .. 1e3) from a fixed seed.  Everything a kernel must not read
-- basis columns that are not in use, the pad element behind an odd column,
coefficient slots past cnt -- holds NaN, so a stray read that reaches a result
shows.

Without a GPU: the mirror of struct lsb_gmres_state and the argument tables are
checked against lsb_impl.h, and the small-algebra restatements (rotations,
back substitution) against numpy's QR and least squares.

Every tolerance below is derived from the arithmetic the rule needs (u = eps/2
per rounding), none is measured.  A sum is judged by its longest addition
chain L: a term passes through at most L additions, each of relative error u,
so the error is at most L u sum|terms| to first order; the tests allow
2 L eps sum|terms|."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MAXR, PARTIALS, WG = 32, 512, 256  # LSB_GMRES_MAX_RESTART, LSB_GMRES_PARTIALS, workgroup size
MAXV = MAXR + 1
HLEN = 40                          # doubles of a coefficient buffer (>= MAXV + 3, what update_w stages)
RUNNING, CONVERGED, BREAKDOWN, MAXIT = 0, 1, 2, 3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")

NS = [1, 2, 3, 255, 1023, 1024, 1025, 2049, 4097]
CNTS = [1, 2, 3, 4, 5, 8, 31, 32]
N_CAPPED = 512 * 1024 + 1025  # asks for 514 workgroups, gets LSB_GMRES_PARTIALS


class GmState(C.Structure):
    """struct lsb_gmres_state (lsb_impl.h); test_state_mirror_matches_header guards it."""
    _fields_ = [("bnorm", C.c_double), ("thresh", C.c_double), ("beta", C.c_double),
                ("resid", C.c_double), ("hnorm", C.c_double),
                ("g", C.c_double * MAXV), ("cs", C.c_double * MAXR), ("sn", C.c_double * MAXR),
                ("y", C.c_double * MAXR), ("R", C.c_double * (MAXR * MAXR)),
                ("iters", C.c_int), ("status", C.c_int), ("maxit", C.c_int), ("restart", C.c_int),
                ("jlast", C.c_int), ("cycle_open", C.c_int)]


_vp, _sz, _u, _i, _d = C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_double
# name -> (restype, argtypes), from the prototypes of lsb_impl.h; test_launcher_tables_match_header guards it
LAUNCHERS = {
    "lsb_k_gm_grid": (_u, [_u]),
    "lsb_k_gm_resid": (None, [_u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_gm_begin": (None, [_vp, _vp, _u, _d, _i, _i, _i, _vp]),
    "lsb_k_gm_scale_prec": (None, [_u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_gm_multidot": (None, [_u, _vp, _sz, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "lsb_k_gm_update_w": (None, [_u, _vp, _sz, _i, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_gm_hess": (None, [_vp, _i, _vp, _vp, _vp, _u, _vp]),
    "lsb_k_gm_finish_cycle": (None, [_u, _vp, _sz, _vp, _vp, _vp, _vp]),
}


# ------------------------------------------------------------------ restatements (longdouble)

def ref_hess_step(cs, sn, gj, hcol, hn):
    """Column j of the Hessenberg matrix through the j rotations already stored, then the
    rotation that annihilates its subdiagonal entry hn.  hcol: the j + 1 entries above it.
    Returns (column j of R: j + 1 entries, c, s, new g[j], g[j + 1])."""
    j = len(hcol) - 1
    col = np.append(np.asarray(hcol, LD), LD(hn))
    for i in range(j):
        G = np.array([[cs[i], sn[i]], [-sn[i], cs[i]]], LD)
        col[i:i + 2] = G @ col[i:i + 2]
    a, b = col[j], col[j + 1]
    d = np.sqrt(a * a + b * b)
    c, s = (a / d, b / d) if d != 0 else (LD(1), LD(0))
    col[j] = d
    return col[:j + 1], c, s, c * LD(gj), -s * LD(gj)


def ref_rotate(H, beta):
    """All columns of an (m + 1) x m upper-Hessenberg H: R (m x m), g (m + 1), cs, sn."""
    m = H.shape[1]
    R, g = np.zeros((m, m), LD), np.zeros(m + 1, LD)
    cs, sn = np.zeros(m, LD), np.zeros(m, LD)
    g[0] = beta
    for j in range(m):
        R[:j + 1, j], cs[j], sn[j], g[j], g[j + 1] = ref_hess_step(cs, sn, g[j], H[:j + 1, j], H[j + 1, j])
    return R, g, cs, sn


def ref_solve_y(R, g):
    """y = R^-1 g by back substitution, R m x m upper triangular; a zero pivot gives y[i] = 0."""
    m = R.shape[0]
    y = np.zeros(m, LD)
    for i in reversed(range(m)):
        y[i] = (LD(g[i]) - np.dot(R[i, i + 1:].astype(LD), y[i + 1:])) / LD(R[i, i]) if R[i, i] != 0 else 0
    return y


def _rand(rng, *shape):
    """mixed signs, magnitudes log-uniform over [1e-3, 1e3]"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def _hessenberg(rng, m):
    """(m + 1) x m upper Hessenberg, well conditioned: the rows below the first are a triangle
    with diagonal in [1, 2] and entries of at most 1/(2m) above it (Gershgorin: its singular
    values lie in [1/2, 5/2]); the first row only adds to H^T H."""
    H = np.triu(rng.uniform(-1.0, 1.0, size=(m + 1, m)) / (2 * m), -1)
    H[np.arange(1, m + 1), np.arange(m)] = rng.choice([-1.0, 1.0], size=m) * rng.uniform(1.0, 2.0, size=m)
    H[0, :] = rng.uniform(-1.0, 1.0, size=m)
    return H


def _triangle(rng, m):
    """m x m upper triangle, diagonal in [1, 2] (either sign), off-diagonal magnitudes <= 1/(2m)"""
    R = np.triu(rng.uniform(-1.0, 1.0, size=(m, m)) / (2 * m), 1)
    R[np.arange(m), np.arange(m)] = rng.choice([-1.0, 1.0], size=m) * rng.uniform(1.0, 2.0, size=m)
    return R


# ------------------------------------------------------------------------ without a GPU

def _header():
    with open(os.path.join(CSRC, "lsb_impl.h")) as f:
        return f.read()


def test_launcher_tables_match_header():
    """argtypes / restype of every launcher as lsb_impl.h declares them: a pointer (and the
    stream) c_void_p, size_t c_size_t, unsigned c_uint, double c_double, int c_int."""
    text = _header()

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _vp
        words = decl.split()
        if words[0] == "void" and len(words) == 1:
            return None
        return {"size_t": _sz, "unsigned": _u, "double": _d, "int": _i}[words[0]]
    for name, (res, args) in LAUNCHERS.items():
        m = re.search(r"^([\w ]+?)\s*\b%s\(([^)]*)\);" % name, text, re.M)
        assert m, name + " is not declared in lsb_impl.h"
        assert ctype(m.group(1)) == res, name
        assert [ctype(p) for p in m.group(2).split(",")] == args, name


def test_state_mirror_matches_header(tmp_path):
    """sizeof and every offsetof of struct lsb_gmres_state, and the two constants, from a C
    program compiled against lsb_impl.h with the include paths of the csrc Makefile."""
    names = [f[0] for f in GmState._fields_]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"lsb_impl.h\"\n"
        "#define O(m) printf(#m \" %zu\\n\", offsetof(struct lsb_gmres_state, m));\n"
        "int main(void) {\n"
        "  printf(\"sizeof %zu\\n\", sizeof(struct lsb_gmres_state));\n"
        "  printf(\"MAX_RESTART %d\\nPARTIALS %d\\n\", LSB_GMRES_MAX_RESTART, LSB_GMRES_PARTIALS);\n"
        "  " + " ".join("O(%s)" % n for n in names) + "\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-I" + os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include")]
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11"] + inc + [str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(GmState)
    assert int(out["MAX_RESTART"]) == MAXR and int(out["PARTIALS"]) == PARTIALS
    for n in names:
        assert int(out[n]) == getattr(GmState, n).offset, n
    d8 = C.sizeof(C.c_double)
    assert (GmState.g.size, GmState.cs.size, GmState.sn.size, GmState.y.size, GmState.R.size) == \
        (33 * d8, 32 * d8, 32 * d8, 32 * d8, 1024 * d8)


@pytest.mark.parametrize("m", [1, 2, 5, 32])
def test_rotation_restatement_vs_qr_and_lstsq(m):
    """ref_hess_step column by column is a QR factorisation of H: |R| is numpy's |R| (the two
    differ by row signs only), |g[m]| the least-squares residual of H y = beta e1 and
    R^-1 g its solution.  H is well conditioned by construction (cond <= 8 asserted), so
    the factor and the solution move by a small multiple of the backward error of numpy's own
    fp64 factorisation, m eps ||H||; the two derived quantities get that bound times cond(H)
    (residual) and cond(H)^2 (solution), the first-order least-squares perturbation bound."""
    rng = np.random.default_rng(1000 + m)
    H = _hessenberg(rng, m)
    beta = 0.75
    norm, cond = np.linalg.norm(H, 2), np.linalg.cond(H)
    assert cond <= 8.0
    R, g, cs, sn = ref_rotate(H.astype(LD), LD(beta))
    assert np.abs(cs * cs + sn * sn - 1).max() <= 4 * np.finfo(LD).eps
    Rq = np.linalg.qr(H, mode="r")
    assert np.abs(np.abs(R.astype(np.float64)) - np.abs(Rq)).max() <= m * EPS * norm
    rhs = np.zeros(m + 1)
    rhs[0] = beta
    yl = np.linalg.lstsq(H, rhs, rcond=None)[0]
    res = np.linalg.norm(H @ yl - rhs)
    assert abs(abs(float(g[m])) - res) <= m * EPS * norm * cond * beta
    y = ref_solve_y(R, g[:m]).astype(np.float64)
    assert np.abs(y - yl).max() <= m * EPS * cond ** 2 * max(np.abs(yl).max(), beta)


@pytest.mark.parametrize("m", [1, 2, 5, 32])
def test_back_substitution_bound_holds_for_plain_fp64(m):
    """The triangle the finish_cycle cases use (diagonal in [1, 2], off-diagonal magnitudes
    <= 1/(2m)): ref_solve_y agrees with numpy's solver, and a plain fp64 back substitution
    stays within 4 m eps max|y| of it -- the bound asked of the GPU is one a correct fp64
    implementation meets.  (Row i: m - 1 - i products and subtractions and one division;
    the off-diagonal row sums are below 1/2, so errors of later entries are not amplified.)"""
    rng = np.random.default_rng(2000 + m)
    R, g = _triangle(rng, m), _rand(rng, m)
    y = ref_solve_y(R, g)
    ynp = np.linalg.solve(R, g)
    assert np.abs(y.astype(np.float64) - ynp).max() <= 4 * m * EPS * np.abs(ynp).max()
    y64 = np.zeros(m)
    for i in reversed(range(m)):
        s = g[i]
        for k in range(i + 1, m):
            s -= R[i, k] * y64[k]
        y64[i] = s / R[i, i]
    assert np.abs(y64 - y).max() <= 4 * m * EPS * float(np.abs(y).max())
    R[m // 2, m // 2] = 0.0
    y0 = ref_solve_y(R, g)
    assert y0[m // 2] == 0 and np.isfinite(y0.astype(np.float64)).all()


# ------------------------------------------------------------------------------- GPU plumbing

def _bits(a):
    return np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)


def _same(a, b):
    """bit for bit, NaN included"""
    return np.array_equal(_bits(a), _bits(b))


class _Dev:
    """Device buffers of one case and the launchers with their C signatures."""

    def __init__(self, la):
        self.lib = la._lib.load()
        self.k = self.lib.hip
        for name, (res, args) in LAUNCHERS.items():
            fn = getattr(self.k, name)
            fn.restype, fn.argtypes = res, args
        self.stream = self.lib.lsb_hip_stream()
        assert self.stream, "no stream: the backend is not initialised"
        self._ptrs = []

    def put(self, a):
        a = np.ascontiguousarray(a, np.float64)
        assert a.nbytes > 0
        p = self.lib.lsb_hip_malloc(a.nbytes)
        assert p
        self._ptrs.append(p)
        self.write(p, a)
        return p

    def write(self, p, a):
        a = np.ascontiguousarray(a, np.float64)
        assert self.lib.lsb_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0

    def get(self, p, count):
        a = np.empty(count, np.float64)
        assert self.lib.lsb_hip_memcpy_d2h(a.ctypes.data, p, a.nbytes) == 0
        return a

    def put_state(self, st):
        p = self.lib.lsb_hip_malloc(C.sizeof(GmState))
        assert p
        self._ptrs.append(p)
        self.write_state(p, st)
        return p

    def write_state(self, p, st):
        assert self.lib.lsb_hip_memcpy_h2d(p, C.addressof(st), C.sizeof(GmState)) == 0

    def get_state(self, p):
        st = GmState()
        assert self.lib.lsb_hip_memcpy_d2h(C.addressof(st), p, C.sizeof(GmState)) == 0
        return st

    def sync(self):
        assert self.lib.lsb_hip_sync() == 0

    def grid(self, n):
        return int(self.k.lsb_k_gm_grid(n))

    def close(self):
        while self._ptrs:
            self.lib.lsb_hip_free(self._ptrs.pop())


@contextlib.contextmanager
def _device(la):
    dev = _Dev(la)
    try:
        yield dev
    finally:
        dev.close()


def _state(status=RUNNING, cycle_open=1, **kw):
    """A state whose every double is a distinct finite sentinel and whose ints are odd values,
    then the named members."""
    st = GmState()
    nd = GmState.iters.offset // 8
    C.memmove(C.addressof(st), (-(np.arange(nd) + 1000.0) / 7.0).ctypes.data, nd * 8)
    st.iters, st.maxit, st.restart, st.jlast = 7, 1000, MAXR, 3
    st.status, st.cycle_open = status, cycle_open
    for k, v in kw.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            getattr(st, k)[:len(v)] = [float(t) for t in v]
        else:
            setattr(st, k, v)
    return st


def _copy(st):
    return GmState.from_buffer_copy(bytes(st))


def _arr(member):
    return np.array(member[:], np.float64)


class _Case:
    pass


def _alloc_case(dev, n, cnt, j=0, V=None, h=None, h2=None, partials=None, state=None):
    """Upload one case.  The basis is the driver's at restart 32 (33 columns of ld doubles, ld the
    next even number >= n); every shape a launcher relies on is asserted before anything runs."""
    c = _Case()
    c.n, c.cnt, c.j = n, cnt, j
    c.ld = (n + 1) & ~1
    c.V = np.full((MAXV, c.ld), np.nan) if V is None else np.ascontiguousarray(V, np.float64)
    c.h = np.full(HLEN, np.nan) if h is None else np.ascontiguousarray(h, np.float64)
    c.h2 = np.full(HLEN, np.nan) if h2 is None else np.ascontiguousarray(h2, np.float64)
    c.partials = np.full(PARTIALS * MAXV, np.nan) if partials is None else \
        np.ascontiguousarray(partials, np.float64)
    c.state = _state() if state is None else state
    assert 1 <= n < 2 ** 31
    assert c.ld % 2 == 0 and c.ld >= n
    assert c.V.ndim == 2 and c.V.shape[1] == c.ld and c.V.size >= (cnt + 1) * c.ld
    assert c.partials.size == PARTIALS * (MAXR + 1)
    assert c.h.size >= MAXV and c.h2.size >= MAXV
    assert 1 <= cnt <= MAXR
    assert 0 <= j <= MAXR - 1
    assert 1 <= dev.grid(n) <= PARTIALS
    c.dV, c.dh, c.dh2 = dev.put(c.V), dev.put(c.h), dev.put(c.h2)
    c.dpart, c.dst = dev.put(c.partials), dev.put_state(c.state)
    c.col = lambda k: c.dV + k * c.ld * 8
    return c


def _basis(rng, n, cnt):
    """cnt basis columns and w behind them (column cnt), NaN in the pad and in every other column"""
    ld = (n + 1) & ~1
    V = np.full((MAXV, ld), np.nan)
    V[:cnt + 1, :n] = _rand(rng, cnt + 1, n)
    return V


def _chain(lane_adds, final_parts=0):
    """Longest addition chain of a workgroup-reduced sum: the additions of one lane's own loop
    (2 per turn where a turn takes a pair of elements), 6 for the wave butterfly, 2 for the four
    waves; with a final kernel over final_parts partials, the turns of its lane loop and the 8
    of its own reduction.  The odd last element (one more addition in one lane) and the
    rounding of the products are inside the factor 2 of the bound 2 L eps = 4 L u."""
    L = lane_adds + 6 + 2
    if final_parts:
        L += -(-final_parts // WG) + 8
    return L


def _turns(items, grid):
    return -(-items // (grid * WG))


# --------------------------------------------------------------------------------- multidot

def _check_multidot(la, n, cnt):
    rng = np.random.default_rng(31 * n + cnt)
    V = _basis(rng, n, cnt)
    prod = V[:cnt, :n].astype(LD) * V[cnt, :n].astype(LD)
    ref, mag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    tail = -(np.arange(HLEN) + 3.0) / 11.0  # what h[cnt:] holds and must keep
    h_new = np.where(np.arange(HLEN) < cnt, np.nan, tail)
    h_acc = np.where(np.arange(HLEN) < cnt, _rand(rng, HLEN), tail)
    with _device(la) as dev:
        grid = dev.grid(n)
        L = _chain(2 * _turns(n // 2, grid), grid)
        tol = 2 * L * EPS * mag
        c = _alloc_case(dev, n, cnt, V=V, h=h_new)
        w = c.col(cnt)

        def run(accumulate):
            dev.k.lsb_k_gm_multidot(n, c.dV, c.ld, cnt, w, c.dpart, c.dh, accumulate, c.dst, dev.stream)
            dev.sync()
            return dev.get(c.dh, HLEN), dev.get(c.dpart, grid * MAXV)
        h1, p1 = run(0)
        dev.write(c.dh, h_new)
        dev.write(c.dpart, c.partials)
        h2, p2 = run(0)
        assert _same(h1, h2) and _same(p1, p2), "two runs of one case differ"
        assert _same(h1[cnt:], tail[cnt:])
        err = np.abs(h1[:cnt].astype(LD) - ref)
        print("multidot n=%d cnt=%d grid=%d L=%d: max err/tol %.3g" % (n, cnt, grid, L, float((err / tol).max())))
        assert (err <= tol).all(), (err / tol).astype(np.float64)
        # accumulate: one more addition, h0 + dot, rounded once (eps |result| allows for it twice over)
        dev.write(c.dh, h_acc)
        h3, _ = run(1)
        assert _same(h3[cnt:], tail[cnt:])
        ref3 = h_acc[:cnt].astype(LD) + ref
        err3 = np.abs(h3[:cnt].astype(LD) - ref3)
        assert (err3 <= tol + EPS * np.abs(ref3)).all(), (err3 / tol).astype(np.float64)
        assert _same(dev.get(c.dV, V.size), V) and bytes(dev.get_state(c.dst)) == bytes(c.state)


@pytest.mark.gpu
@pytest.mark.parametrize("cnt", CNTS)
@pytest.mark.parametrize("n", NS)
def test_multidot(hip, n, cnt):
    """h[k] = V[k] . w for k < cnt (k_gm_multidot + k_gm_multidot_final), w in column cnt as in the
    driver: odd tails, counts on both sides of the four-column groups, one and several
    workgroups, a second grid-stride turn; overwrite and accumulate; h[cnt:] kept; repeatable
    bit for bit."""
    _check_multidot(hip, n, cnt)


@pytest.mark.gpu
def test_multidot_beyond_the_grid_cap(hip):
    with _device(hip) as dev:
        assert dev.grid(N_CAPPED) == PARTIALS == 512
    _check_multidot(hip, N_CAPPED, 5)


# --------------------------------------------------------------------------------- update_w

def _check_update_w(la, n, cnt):
    rng = np.random.default_rng(37 * n + cnt)
    V = _basis(rng, n, cnt)
    h = np.full(HLEN, np.nan)  # finite below cnt only: the kernel's own zero fill must cover the rest
    h[:cnt] = _rand(rng, cnt)
    terms = h[:cnt, None].astype(LD) * V[:cnt, :n].astype(LD)
    w0 = V[cnt, :n].astype(LD)
    ref = w0 - terms.sum(axis=0)
    tol = (cnt + 2) * EPS * (np.abs(w0) + np.abs(terms).sum(axis=0))
    with _device(la) as dev:
        grid = dev.grid(n)
        c = _alloc_case(dev, n, cnt, V=V, h=h)
        dev.k.lsb_k_gm_update_w(n, c.dV, c.ld, cnt, c.dh, c.col(cnt), c.dpart, c.dst, dev.stream)
        dev.sync()
        Vg = dev.get(c.dV, V.size).reshape(V.shape)
        parts = dev.get(c.dpart, PARTIALS * MAXV)
        assert bytes(dev.get_state(c.dst)) == bytes(c.state) and _same(dev.get(c.dh, HLEN), h)
    w = Vg[cnt, :n]
    err = np.abs(w.astype(LD) - ref)
    print("update_w n=%d cnt=%d grid=%d: max err/tol %.3g" % (n, cnt, grid, float((err / tol).max())))
    assert (err <= tol).all(), "w wrong at %s" % np.flatnonzero(~(err <= tol))[:8]
    keep = np.ones(V.shape, bool)
    keep[cnt, :n] = False
    assert _same(Vg[keep], V[keep]), "the kernel wrote outside w"
    # ||w||^2 of the w it wrote: one partial per workgroup, the rest of the buffer untouched
    ss = (w.astype(LD) ** 2).sum()
    L = _chain(2 * _turns(n // 2, grid))
    assert abs(parts[:grid].astype(LD).sum() - ss) <= 2 * L * EPS * ss
    assert np.isnan(parts[grid:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cnt", CNTS)
@pytest.mark.parametrize("n", NS)
def test_update_w(hip, n, cnt):
    """w -= sum_k h[k] V[k] element by element ((cnt + 2) roundings bound every element: cnt fused
    steps, none of them worse than a product and a subtraction), and the partial sums of w^2.
    h holds NaN from index cnt on, the basis NaN in the columns behind w."""
    _check_update_w(hip, n, cnt)


@pytest.mark.gpu
def test_update_w_beyond_the_grid_cap(hip):
    _check_update_w(hip, N_CAPPED, 5)


# ---------------------------------------------------------------------------- resid and begin

def _check_begin_fields(st, beta_ref, nparts):
    """what every k_gm_begin that runs sets: beta from the partials, resid, hnorm, g, jlast"""
    L = _chain(0, nparts) - 8  # the final kernel's part of the chain only
    # the sum of squares is within L u, its root within L u / 2 + u = (L / 4 + 1 / 2) eps
    assert abs(LD(st.beta) - beta_ref) <= (L / 4 + 0.5) * EPS * beta_ref
    assert st.resid == st.beta and st.hnorm == st.beta and st.g[0] == st.beta
    assert not np.any(_arr(st.g)[1:]) and st.jlast == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 1025, 2049])
def test_resid_then_first_begin(hip, n):
    """k_gm_resid: v0 = b - ax bit for bit (one subtraction), its partials; it runs with the cycle
    closed (it gates on status alone).  k_gm_begin(first = 1) on a state full of leftovers sets
    every scalar of a fresh solve and leaves the rotations, y and R alone."""
    rng = np.random.default_rng(41 * n)
    b, ax = _rand(rng, n), _rand(rng, n)
    with _device(hip) as dev:
        st0 = _state(status=RUNNING, cycle_open=0)
        c = _alloc_case(dev, n, 1, state=st0)
        db, dax = dev.put(b), dev.put(ax)
        grid = dev.grid(n)
        dev.k.lsb_k_gm_resid(n, db, dax, c.col(0), c.dpart, c.dst, dev.stream)
        dev.sync()
        Vg = dev.get(c.dV, c.V.size).reshape(c.V.shape)
        parts = dev.get(c.dpart, PARTIALS * MAXV)
        assert bytes(dev.get_state(c.dst)) == bytes(st0)
        assert _same(Vg[0, :n], b - ax) and np.isnan(Vg[0, n:]).all() and np.isnan(Vg[1:]).all()
        ss = ((b - ax).astype(LD) ** 2).sum()
        assert abs(parts[:grid].astype(LD).sum() - ss) <= 2 * _chain(_turns(n, grid)) * EPS * ss  # (one element, one addition a turn)
        assert np.isnan(parts[grid:]).all()
        # a state left over from an earlier solve: first = 1 does not look at it
        st1 = _state(status=MAXIT, cycle_open=0, iters=99, jlast=5)
        dev.write_state(c.dst, st1)
        tol = 1e-10
        dev.k.lsb_k_gm_begin(c.dst, c.dpart, grid, tol, 123, 17, 1, dev.stream)
        dev.sync()
        st = dev.get_state(c.dst)
    _check_begin_fields(st, np.sqrt(parts[:grid].astype(LD).sum()), grid)
    assert st.bnorm == st.beta and st.thresh == np.float64(tol) * np.float64(st.bnorm)
    assert (st.iters, st.maxit, st.restart, st.status, st.cycle_open) == (0, 123, 17, RUNNING, 1)
    for name in ("cs", "sn", "y", "R"):
        assert _same(_arr(getattr(st, name)), _arr(getattr(st1, name))), name


@pytest.mark.gpu
def test_begin_on_a_restart_and_its_exits(hip):
    """first = 0: bnorm, thresh, iters, maxit and restart stay, the cycle reopens with the new
    beta; beta <= thresh ends CONVERGED, iters >= maxit ends MAXIT, b = 0 ends CONVERGED at
    once, each with the cycle closed; a state that is no longer RUNNING is left alone."""
    rng = np.random.default_rng(43)
    nparts = 300  # more than one turn of the final loop
    partials = np.full(PARTIALS * MAXV, np.nan)
    partials[:nparts] = np.abs(_rand(rng, nparts))
    beta_ref = np.sqrt(partials[:nparts].astype(LD).sum())
    beta = float(beta_ref)

    def untouched(st, st0, names):
        for f, _ in GmState._fields_:
            if f not in names:
                a, b = getattr(st, f), getattr(st0, f)
                assert (a == b) if isinstance(a, (int, float)) else _same(_arr(a), _arr(b)), f
    with _device(hip) as dev:
        c = _alloc_case(dev, 3, 1, partials=partials)

        def begin(st0, first=0, tol=1e-3, maxit=55, restart=4):
            dev.write_state(c.dst, st0)
            dev.k.lsb_k_gm_begin(c.dst, c.dpart, nparts, tol, maxit, restart, first, dev.stream)
            dev.sync()
            return dev.get_state(c.dst)
        changed = ("beta", "resid", "hnorm", "g", "jlast", "cycle_open", "status")
        # the ordinary restart (arguments tol, maxit, restart are not read again)
        st0 = _state(cycle_open=0, bnorm=4 * beta, thresh=beta / 8, iters=9, maxit=50, restart=5, jlast=5)
        st = begin(st0)
        _check_begin_fields(st, beta_ref, nparts)
        assert (st.status, st.cycle_open) == (RUNNING, 1)
        untouched(st, st0, changed)
        # converged at the restart
        st0 = _state(cycle_open=0, bnorm=4 * beta, thresh=2 * beta, iters=9, maxit=50)
        st = begin(st0)
        _check_begin_fields(st, beta_ref, nparts)
        assert (st.status, st.cycle_open) == (CONVERGED, 0)
        untouched(st, st0, changed)
        # out of iterations at the restart
        st0 = _state(cycle_open=0, bnorm=4 * beta, thresh=beta / 8, iters=50, maxit=50)
        st = begin(st0)
        _check_begin_fields(st, beta_ref, nparts)
        assert (st.status, st.cycle_open) == (MAXIT, 0)
        untouched(st, st0, changed)
        # no longer running: nothing happens, whatever cycle_open says
        for status in (CONVERGED, BREAKDOWN, MAXIT):
            st0 = _state(status=status, cycle_open=1)
            assert bytes(begin(st0)) == bytes(st0)
        # b = 0 through both kernels
        n = 3
        dz = dev.put(np.zeros(n))
        dev.write_state(c.dst, _state(cycle_open=0))
        dev.k.lsb_k_gm_resid(n, dz, dz, c.col(0), c.dpart, c.dst, dev.stream)
        dev.sync()
        dev.write_state(c.dst, _state(status=BREAKDOWN, cycle_open=1))
        dev.k.lsb_k_gm_begin(c.dst, c.dpart, dev.grid(n), 1e-10, 77, 5, 1, dev.stream)
        dev.sync()
        st = dev.get_state(c.dst)
        assert (st.bnorm, st.thresh, st.beta, st.resid) == (0.0, 0.0, 0.0, 0.0)
        assert (st.status, st.cycle_open, st.iters, st.maxit) == (CONVERGED, 0, 0, 77)
        assert not dev.get(c.col(0), n).any()


# -------------------------------------------------------------------------------- scale_prec

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 1025])
def test_scale_prec_in_place(hip, n):
    """v = w / hnorm in place and z = dinv v, as the driver calls it (w == v).  The kernel
    multiplies by a rounded reciprocal: two roundings for v (relative error 2u <= 2 ulp), a
    third for z (3u <= 3 ulp)."""
    rng = np.random.default_rng(47 * n)
    V = _basis(rng, n, 1)
    dinv, hnorm = _rand(rng, n), 3.7e-2
    with _device(hip) as dev:
        st0 = _state(hnorm=hnorm)
        c = _alloc_case(dev, n, 1, V=V, state=st0)
        dd, dz = dev.put(dinv), dev.put(np.full(c.ld, np.nan))
        dev.k.lsb_k_gm_scale_prec(n, c.col(0), c.col(0), dd, dz, c.dst, dev.stream)
        dev.sync()
        Vg = dev.get(c.dV, V.size).reshape(V.shape)
        z = dev.get(dz, c.ld)
        assert bytes(dev.get_state(c.dst)) == bytes(st0)
    vref = V[0, :n].astype(LD) / LD(hnorm)
    zref = dinv.astype(LD) * vref
    assert (np.abs(Vg[0, :n].astype(LD) - vref) <= 2 * np.spacing(np.abs(vref.astype(np.float64)))).all()
    assert (np.abs(z[:n].astype(LD) - zref) <= 3 * np.spacing(np.abs(zref.astype(np.float64)))).all()
    keep = np.ones(V.shape, bool)
    keep[0, :n] = False
    assert _same(Vg[keep], V[keep]) and np.isnan(z[n:]).all()


# -------------------------------------------------------------------------------------- hess

def _hess_inputs(rng, j, hn=None):
    """the two Gram-Schmidt passes' coefficients (NaN past j) and the one partial ||w||^2.
    ||w|| is drawn from [1, 1e3]: the rotation's divisor d = sqrt(a^2 + ||w||^2) is then >= 1,
    and (4 j + 8) eps ||column|| bounds c and s as well (see test_hess_steps_in_sequence)."""
    h1, h2 = np.full(HLEN, np.nan), np.full(HLEN, np.nan)
    h1[:j + 1], h2[:j + 1] = _rand(rng, j + 1), _rand(rng, j + 1)
    hn = 10.0 ** rng.uniform(0.0, 3.0) if hn is None else hn
    partials = np.full(PARTIALS * MAXV, np.nan)
    partials[0] = hn * hn
    return h1, h2, partials


@pytest.mark.gpu
def test_hess_steps_in_sequence(hip):
    """k_gm_hess for j = 0 .. 31 on one device state.  Each step is judged on its own: the
    restatement takes the rotations and g[j] the GPU stored so far and applies one column.

    Bound (4 j + 8) eps ||column||_2, column = (h1 + h2, ||w||): the sum h1 + h2 costs u per
    entry; a rotation, two products and a sum, moves the column by at most (1 + sqrt 2) u
    ||column||, j of them (2.5 j + 1) u ||column|| =: e.  d = sqrt(a^2 + b^2) adds 2.5 u d.
    c = a / d and s = b / d: 2 e / d + 3 u; with d >= 1 (see _hess_inputs) and ||column|| >= d
    that is below (2.5 j + 2.5) eps ||column||.  g[j] and g[j + 1] are c and s times |g[j]| <=
    beta = 0.75 and one more rounding.  hnorm is one square root of the partial."""
    rng = np.random.default_rng(53)
    beta = 0.75
    g0 = np.zeros(MAXV)
    g0[0] = beta
    st_prev = _state(thresh=1e-300, beta=beta, resid=beta, hnorm=beta, bnorm=beta, g=g0,
                     iters=7, maxit=1000, restart=MAXR, jlast=0)
    with _device(hip) as dev:
        c = _alloc_case(dev, 3, 1, j=0, state=st_prev)
        for j in range(MAXR):
            assert 0 <= j <= MAXR - 1
            h1, h2, partials = _hess_inputs(rng, j)
            dev.write(c.dh, h1), dev.write(c.dh2, h2), dev.write(c.dpart, partials)
            dev.k.lsb_k_gm_hess(c.dst, j, c.dh, c.dh2, c.dpart, 1, dev.stream)
            dev.sync()
            st = dev.get_state(c.dst)
            hn = np.sqrt(LD(partials[0]))
            hcol = h1[:j + 1].astype(LD) + h2[:j + 1].astype(LD)
            tol = (4 * j + 8) * EPS * float(np.sqrt((hcol * hcol).sum() + hn * hn))
            col, cc, ss, gj, gj1 = ref_hess_step(_arr(st_prev.cs).astype(LD), _arr(st_prev.sn).astype(LD),
                                                 st_prev.g[j], hcol, hn)
            R = _arr(st.R).reshape(MAXR, MAXR)
            got = np.concatenate([R[:j + 1, j], [st.cs[j], st.sn[j], st.g[j], st.g[j + 1], st.resid, st.hnorm]])
            want = np.concatenate([col, [cc, ss, gj, gj1, abs(gj1), hn]])
            err = np.abs(got.astype(LD) - want)
            assert (err <= tol).all(), "step %d: err/tol %s" % (j, (err / tol).astype(np.float64))
            assert abs(st.cs[j] ** 2 + st.sn[j] ** 2 - 1.0) <= 8 * EPS  # (c, s within 3.5 u each)
            assert (st.jlast, st.iters, st.status, st.cycle_open) == (j + 1, 7 + j + 1, RUNNING, 1)
            # everything else is as it was: R outside rows 0..j of column j, the older rotations, y, ...
            exp = _copy(st_prev)
            for i in range(j + 1):
                exp.R[i * MAXR + j] = st.R[i * MAXR + j]
            exp.cs[j], exp.sn[j], exp.g[j], exp.g[j + 1] = st.cs[j], st.sn[j], st.g[j], st.g[j + 1]
            exp.resid, exp.hnorm, exp.jlast, exp.iters = st.resid, st.hnorm, st.jlast, st.iters
            assert bytes(exp) == bytes(st), "step %d wrote outside its column" % j
            st_prev = st


@pytest.mark.gpu
def test_hess_status_rules(hip):
    """Each stop rule of k_gm_hess alone, at j = 0 on a fresh cycle."""
    rng = np.random.default_rng(59)
    beta = 0.75
    g0 = np.zeros(MAXV)
    g0[0] = beta

    def fresh(**kw):
        kw = dict(dict(thresh=1e-300, beta=beta, resid=beta, hnorm=beta, g=g0, iters=7, maxit=1000, jlast=0), **kw)
        return _state(**kw)
    with _device(hip) as dev:
        c = _alloc_case(dev, 3, 1, j=0)

        def step(st0, h1, h2, partials):
            dev.write_state(c.dst, st0)
            dev.write(c.dh, h1), dev.write(c.dh2, h2), dev.write(c.dpart, partials)
            dev.k.lsb_k_gm_hess(c.dst, 0, c.dh, c.dh2, c.dpart, 1, dev.stream)
            dev.sync()
            return dev.get_state(c.dst)
        h1, h2, partials = _hess_inputs(rng, 0)
        assert step(fresh(), h1, h2, partials).status == RUNNING
        # the residual estimate is at the threshold: CONVERGED
        st = step(fresh(thresh=beta), h1, h2, partials)
        assert (st.status, st.iters, st.jlast) == (CONVERGED, 8, 1) and st.resid <= beta
        # the last allowed iteration: MAXIT
        st = step(fresh(iters=999), h1, h2, partials)
        assert (st.status, st.iters) == (MAXIT, 1000)
        # converged and out of iterations: CONVERGED wins
        assert step(fresh(thresh=beta, iters=999), h1, h2, partials).status == CONVERGED
        # ||w|| = 0, a != 0: the Krylov space is exhausted.  A negative threshold keeps the residual
        # rule (0 <= thresh) out of it.
        z = partials.copy()
        z[0] = 0.0
        st = step(fresh(thresh=-1.0), h1, h2, z)
        assert (st.status, st.hnorm, st.sn[0], st.resid) == (CONVERGED, 0.0, 0.0, 0.0)
        a = abs(h1[0] + h2[0])  # d = sqrt(a^2), c = a / d, g[0] = c beta: a rounding or two each
        assert abs(abs(st.cs[0]) - 1.0) <= 2 * EPS and abs(abs(st.R[0]) - a) <= 2 * EPS * a
        assert abs(abs(st.g[0]) - beta) <= 2 * EPS * beta
        # a = b = 0 (the two passes cancel): BREAKDOWN with the identity rotation, ahead of every other rule
        h2c = h2.copy()
        h2c[0] = -h1[0]
        st = step(fresh(thresh=beta, iters=999), h1, h2c, z)
        assert (st.status, st.cs[0], st.sn[0], st.R[0], st.g[0], st.g[1]) == (BREAKDOWN, 1.0, 0.0, 0.0, beta, 0.0)
        assert (st.iters, st.jlast, st.resid) == (1000, 1, 0.0)


# ------------------------------------------------------------------------------ finish_cycle

def _finish_case(rng, n, m, zero_pivot=None, **state):
    V = np.full((MAXV, (n + 1) & ~1), np.nan)
    V[:m, :n] = _rand(rng, m, n)
    R = np.full((MAXR, MAXR), np.nan)  # only the m x m upper triangle is the kernel's to read
    T = _triangle(rng, m)
    if zero_pivot is not None:
        T[zero_pivot, zero_pivot] = 0.0
    R[:m, :m] = np.where(np.triu(np.ones((m, m), bool)), T, np.nan)
    g = np.full(MAXV, np.nan)
    g[:m] = _rand(rng, m)
    st = _state(jlast=m, g=g, R=R.ravel(), y=np.full(MAXR, np.nan), **state)
    return V, T, g, st, _rand(rng, n), _rand(rng, n)


def _run_finish(dev, n, m, V, st0, dinv, x0):
    c = _alloc_case(dev, n, m, j=m - 1, V=V, state=st0)
    dd, dx = dev.put(dinv), dev.put(x0)
    dev.k.lsb_k_gm_finish_cycle(n, c.dV, c.ld, dd, dx, c.dst, dev.stream)
    dev.sync()
    assert _same(dev.get(c.dV, V.size), V) and _same(dev.get(dd, n), dinv)
    return dev.get_state(c.dst), dev.get(dx, n)


def _check_finish(st, x, n, m, V, T, g, st0, dinv, x0):
    y = _arr(st.y)
    yref = ref_solve_y(T, g[:m])
    assert (np.abs(y[:m].astype(LD) - yref) <= 4 * m * EPS * np.abs(yref).max()).all()
    terms = y[:m, None].astype(LD) * V[:m, :n].astype(LD)  # with the y the GPU holds: x is judged alone
    xref = x0.astype(LD) + dinv.astype(LD) * terms.sum(axis=0)
    tol = (m + 3) * EPS * (np.abs(x0) + np.abs(dinv) * np.abs(terms).sum(axis=0))
    err = np.abs(x.astype(LD) - xref)
    assert (err <= tol).all(), "x wrong at %s" % np.flatnonzero(~(err <= tol))[:8]
    exp = _copy(st0)
    exp.y[:m] = list(y[:m])
    exp.cycle_open = 0
    assert bytes(exp) == bytes(st), "finish_cycle changed more than y[:m] and cycle_open"


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 5, 32])
@pytest.mark.parametrize("n", [1, 3, 1025])
def test_finish_cycle(hip, n, m):
    """y = R^-1 g over the jlast columns of the cycle, x += dinv sum_k y[k] V[k], the cycle closed.
    x, element by element: m products and sums, the product with dinv and the sum with x --
    (m + 3) roundings.  The same with the status CONVERGED and the cycle still open: that is
    the last update of every solve that converges."""
    for status in (RUNNING, CONVERGED, MAXIT):
        rng = np.random.default_rng(61 * n + m)
        V, T, g, st0, dinv, x0 = _finish_case(rng, n, m, status=status, cycle_open=1)
        with _device(hip) as dev:
            st, x = _run_finish(dev, n, m, V, st0, dinv, x0)
        _check_finish(st, x, n, m, V, T, g, st0, dinv, x0)
        assert not _same(x, x0) and st.status == status


@pytest.mark.gpu
def test_finish_cycle_zero_pivot_and_closed_cycle(hip):
    n, m = 1025, 5
    rng = np.random.default_rng(67)
    V, T, g, st0, dinv, x0 = _finish_case(rng, n, m, zero_pivot=2, cycle_open=1)
    with _device(hip) as dev:
        st, x = _run_finish(dev, n, m, V, st0, dinv, x0)
    assert st.y[2] == 0.0 and np.isfinite(x).all()
    _check_finish(st, x, n, m, V, T, g, st0, dinv, x0)
    # the cycle is closed already: neither y nor x moves
    for status in (RUNNING, CONVERGED):
        V, T, g, st0, dinv, x0 = _finish_case(rng, n, m, status=status, cycle_open=0)
        with _device(hip) as dev:
            st, x = _run_finish(dev, n, m, V, st0, dinv, x0)
        assert bytes(st) == bytes(st0) and _same(x, x0)


# ------------------------------------------------------------------------------------ gating

@pytest.mark.gpu
@pytest.mark.parametrize("status,cycle_open", [(CONVERGED, 1), (RUNNING, 0)])
def test_idle_kernels_write_nothing(hip, status, cycle_open):
    """scale_prec, multidot, update_w and hess with a finished status, and with a running state
    whose cycle is closed: every buffer and the state come back bit for bit.  k_gm_resid gates
    on the status alone (test_resid_then_first_begin runs it with the cycle closed)."""
    n, cnt, j = 1025, 3, 2
    rng = np.random.default_rng(71)
    V = _basis(rng, n, cnt)
    h, h2 = _rand(rng, HLEN), _rand(rng, HLEN)
    partials = _rand(rng, PARTIALS * MAXV)
    dinv, z = _rand(rng, n), _rand(rng, n)
    b, ax = _rand(rng, n), _rand(rng, n)
    st0 = _state(status=status, cycle_open=cycle_open, hnorm=2.5, jlast=j)
    with _device(hip) as dev:
        c = _alloc_case(dev, n, cnt, j=j, V=V, h=h, h2=h2, partials=partials, state=st0)
        dd, dz, db, dax = dev.put(dinv), dev.put(z), dev.put(b), dev.put(ax)
        w, s = c.col(cnt), dev.stream
        launches = [
            lambda: dev.k.lsb_k_gm_scale_prec(n, c.col(0), c.col(0), dd, dz, c.dst, s),
            lambda: dev.k.lsb_k_gm_multidot(n, c.dV, c.ld, cnt, w, c.dpart, c.dh, 0, c.dst, s),
            lambda: dev.k.lsb_k_gm_multidot(n, c.dV, c.ld, cnt, w, c.dpart, c.dh, 1, c.dst, s),
            lambda: dev.k.lsb_k_gm_update_w(n, c.dV, c.ld, cnt, c.dh, w, c.dpart, c.dst, s),
            lambda: dev.k.lsb_k_gm_hess(c.dst, j, c.dh, c.dh2, c.dpart, dev.grid(n), s),
        ]
        if status != RUNNING:
            launches.append(lambda: dev.k.lsb_k_gm_resid(n, db, dax, c.col(0), c.dpart, c.dst, s))
        for i, launch in enumerate(launches):
            launch()
            dev.sync()
            assert _same(dev.get(c.dV, V.size), V), i
            assert _same(dev.get(c.dh, HLEN), h) and _same(dev.get(c.dh2, HLEN), h2), i
            assert _same(dev.get(c.dpart, partials.size), partials) and _same(dev.get(dz, n), z), i
            assert bytes(dev.get_state(c.dst)) == bytes(st0), i
