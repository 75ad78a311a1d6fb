"""The kernels of lsbench_amd/csrc/hip_seq.hip one by one, each launcher called through ctypes as hip_seq_drv.c calls it
and compared with an exact reference: fractions.Fraction on the small shapes, and on the shape whose grid-stride loop
takes a second turn operands on a dyadic grid so coarse that every product and every sum is exact in fp64 whatever
the order (there the device must hit the reference to the bit, which is inside every bound below).

Bounds, with u = 2^-53, derived from the arithmetic and not measured.  A dot product of n terms, whatever the tree: a
term passes through fewer than n roundings, so |error| <= n u sum|x_i v_i|.  An fma chain of m steps on one element:
each step rounds once, on a partial sum no larger than the sum of the magnitudes, so |error| <= m u sum|terms| (the
starting value of d or w among the terms).  The store is one correctly rounded division by a correctly rounded
square root: within 1 ulp of numpy's d / sqrt(nu).

Everything a kernel must not read -- columns k >= m of the basis, the pad element behind an odd column -- holds NaN."""
import contextlib
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

U = 2.0 ** -53
WG, GRID_CAP, MAXD = 256, 768, 16
N_SECOND_TURN = 2 * WG * GRID_CAP + 3  # one pair more than the capped grid takes in one turn, and an odd last row
NS = [1, 63, 64, 65, 257]
MS = [1, 2, 7, 16]

_vp, _sz, _u = C.c_void_p, C.c_size_t, C.c_uint
LAUNCHERS = {
    "lsb_k_seq_grid": (_u, [_u]),
    "lsb_k_seq_dots": (None, [_u, _u, _vp, _sz, _vp, _vp, _vp, _vp]),
    "lsb_k_seq_combine": (None, [_u, _u, _vp, _sz, _vp, _vp, _vp]),
    "lsb_k_seq_orth": (None, [_u, _u, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_seq_store": (None, [_u, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}


def test_launcher_table_matches_header():
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "lsb_impl.h")) as f:
        text = f.read()

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _vp
        words = decl.split()
        if words == ["void"]:
            return None
        return {"size_t": _sz, "unsigned": _u}[words[0]]
    for name, (res, args) in LAUNCHERS.items():
        m = re.search(r"^([\w ]+?)\s*\b%s\(([^)]*)\);" % name, text, re.M)
        assert m, name + " is not declared in lsb_impl.h"
        assert ctype(m.group(1)) == res and [ctype(p) for p in m.group(2).split(",")] == args, name


# ------------------------------------------------------------------------------------------- plumbing
def _bits(a):
    return np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _Dev:
    def __init__(self, la):
        self.lib = la._lib.load()
        self.k = self.lib.hip
        for name, (res, args) in LAUNCHERS.items():
            fn = getattr(self.k, name)
            fn.restype, fn.argtypes = res, args
        self.stream = self.lib.lsb_hip_stream()
        assert self.stream, "no stream: the backend is not initialised"
        self._ptrs = []

    def put(self, a, offset=0):
        """offset: doubles in front of the data (1: an address that is only 8-byte aligned)"""
        a = np.ascontiguousarray(a, np.float64)
        p = self.lib.lsb_hip_malloc(a.nbytes + 8 * offset + 8)
        assert p and p % 16 == 0
        self._ptrs.append(p)
        assert self.lib.lsb_hip_memcpy_h2d(p + 8 * offset, a.ctypes.data, a.nbytes) == 0
        return p + 8 * offset

    def get(self, p, count):
        a = np.empty(count, np.float64)
        assert self.lib.lsb_hip_memcpy_d2h(a.ctypes.data, p, a.nbytes) == 0
        return a

    def sync(self):
        assert self.lib.lsb_hip_sync() == 0

    def close(self):
        while self._ptrs:
            self.lib.lsb_hip_free(self._ptrs.pop())


@contextlib.contextmanager
def _device(la):
    dev = _Dev(la)
    try:
        yield dev
    finally:
        dev.sync()
        dev.close()


def _values(rng, shape, coarse):
    """mixed signs; full doubles over six decades, or (coarse) multiples of 2^-11 below 1"""
    if coarse:
        return rng.integers(-2047, 2048, size=shape).astype(np.float64) / 2048.0
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def _basis(rng, n, m, coarse):
    """MAXD columns with an even leading dimension; NaN in the columns >= m and behind an odd column"""
    ld = (n + 1) & ~1
    B = np.full((MAXD, ld), np.nan)
    B[:m, :n] = _values(rng, (m, n), coarse)
    return B, ld


def _exact_dots(X, v, m, n, coarse):
    """(sum, sum of magnitudes) per column"""
    if coarse:  # every product is a multiple of 2^-22 below 1 and the sum below 2^19: exact in fp64 in any order
        P = X[:m, :n] * v[None, :n]
        return [math.fsum(P[k]) for k in range(m)], [math.fsum(np.abs(P[k])) for k in range(m)]
    fv = [Fraction(t) for t in v[:n]]
    out, mag = [], []
    for k in range(m):
        terms = [Fraction(t) * f for t, f in zip(X[k, :n], fv)]
        out.append(sum(terms))
        mag.append(float(sum(abs(t) for t in terms)))
    return out, mag


def _exact_chain(start, coef, X, m, n):
    """start_i + sum_k coef_k X[k][i] per element as (value, sum of magnitudes); start None: 0"""
    vals, mags = [], []
    for i in range(n):
        terms = [Fraction(coef[k]) * Fraction(X[k, i]) for k in range(m)]
        if start is not None:
            terms.append(Fraction(start[i]))
        vals.append(sum(terms))
        mags.append(float(sum(abs(t) for t in terms)))
    return vals, np.array(mags)


def _check_elements(got, exact, mags, m, what):
    err = np.array([abs(float(Fraction(g) - e)) for g, e in zip(got, exact)])
    bound = m * U * mags
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if len(err) else 0.0
    print(what, "worst error / bound", worst)
    assert (err <= bound).all(), what


def _shapes():
    return [(n, m) for n in NS for m in MS] + [(N_SECOND_TURN, m) for m in MS]


# ----------------------------------------------------------------------------------------- the kernels
@pytest.mark.gpu
def test_the_grid_takes_a_second_turn_where_the_tests_say(hip):
    with _device(hip) as dev:
        assert [int(dev.k.lsb_k_seq_grid(n)) for n in (1, 2, 512, 513, 514)] == [1, 1, 1, 1, 2]
        assert int(dev.k.lsb_k_seq_grid(N_SECOND_TURN - 3)) == GRID_CAP == int(dev.k.lsb_k_seq_grid(N_SECOND_TURN))
        assert (N_SECOND_TURN // 2) > GRID_CAP * WG


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", _shapes())
def test_dots(hip, n, m):
    coarse = n == N_SECOND_TURN
    rng = np.random.default_rng(100 * m + n % 97)
    X, ld = _basis(rng, n, m, coarse)
    v = _values(rng, n, coarse)
    with _device(hip) as dev:
        g = int(dev.k.lsb_k_seq_grid(n))
        d_X, d_parts = dev.put(X), dev.put(np.full(g * (MAXD + 2), np.nan))
        runs = []
        for off in (0, 0, 1):  # twice on a 16-byte aligned v, once on one that is only 8-byte aligned
            d_v, d_a = dev.put(v, off), dev.put(np.full(MAXD, -7.0))
            dev.k.lsb_k_seq_dots(n, m, d_X, ld, d_v, d_parts, d_a, dev.stream)
            dev.sync()
            runs.append(dev.get(d_a, MAXD))
    got = runs[0]
    assert _same(runs[1], got) and _same(runs[2], got)
    assert (got[m:] == -7.0).all()
    exact, mag = _exact_dots(X, v, m, n, coarse)
    for k in range(m):
        err = abs(float(Fraction(got[k]) - Fraction(exact[k])))
        assert err <= n * U * mag[k], (k, got[k], float(exact[k]), err, n * U * mag[k])
        if coarse:
            assert got[k] == exact[k]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", _shapes())
def test_combine(hip, n, m):
    coarse = n == N_SECOND_TURN
    rng = np.random.default_rng(200 * m + n % 97)
    X, ld = _basis(rng, n, m, coarse)
    alpha = np.full(MAXD, np.nan)
    alpha[:m] = _values(rng, m, coarse)
    with _device(hip) as dev:
        d_X, d_a = dev.put(X), dev.put(alpha)
        runs = []
        for off in (0, 0, 1):
            d_x0 = dev.put(np.full(n + 3, -7.0), off)
            dev.k.lsb_k_seq_combine(n, m, d_X, ld, d_a, d_x0, dev.stream)
            dev.sync()
            runs.append(dev.get(d_x0, n + 3))
    got = runs[0]
    assert _same(runs[1], got) and _same(runs[2], got)
    assert (got[n:] == -7.0).all()
    if coarse:  # multiples of 2^-22, at most 16 of them below 1: exact
        assert np.array_equal(got[:n], alpha[:m] @ X[:m, :n])
    else:
        exact, mags = _exact_chain(None, alpha, X, m, n)
        _check_elements(got[:n], exact, mags, m, "combine")


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", _shapes())
def test_orth(hip, n, m):
    """d' and w' element by element, and the sums of the same launch against k_seq_dots on what it wrote: the two
    share their expressions and their reduction, so bit for bit"""
    coarse = n == N_SECOND_TURN
    rng = np.random.default_rng(300 * m + n % 97)
    X, ld = _basis(rng, n, m, coarse)
    SX, _ = _basis(rng, n, m, coarse)
    d, w = _values(rng, n, coarse), _values(rng, n, coarse)
    beta = np.full(MAXD, np.nan)
    beta[:m] = _values(rng, m, coarse)
    with _device(hip) as dev:
        g = int(dev.k.lsb_k_seq_grid(n))
        d_X, d_SX, d_b = dev.put(X), dev.put(SX), dev.put(beta)
        d_parts = dev.put(np.full(g * (MAXD + 2), np.nan))
        runs = []
        for off in (0, 0, 1):
            d_d, d_w, d_out = dev.put(np.append(d, -7.0), off), dev.put(np.append(w, -7.0), off), dev.put(np.full(MAXD + 2, -7.0))
            dev.k.lsb_k_seq_orth(n, m, d_X, d_SX, ld, d_b, d_d, d_w, d_parts, d_out, dev.stream)
            dev.sync()
            runs.append((dev.get(d_d, n + 1), dev.get(d_w, n + 1), dev.get(d_out, MAXD + 2)))
        d1, w1, out = runs[0]
        for r in runs[1:]:
            assert _same(r[0], d1) and _same(r[1], w1) and _same(r[2], out)
        assert d1[n] == -7.0 and w1[n] == -7.0 and (out[m + 2:] == -7.0).all()
        # the sums, by k_seq_dots on the vectors just written (ld: any even number >= n for a single column)
        d_d1, d_w1, d_d0, d_w0 = dev.put(d1[:n]), dev.put(w1[:n]), dev.put(d), dev.put(w)
        d_s = dev.put(np.full(MAXD + 2, -7.0))
        dev.k.lsb_k_seq_dots(n, m, d_X, ld, d_w1, d_parts, d_s, dev.stream)
        dev.k.lsb_k_seq_dots(n, 1, d_d1, ld, d_w1, d_parts, d_s + 8 * m, dev.stream)
        dev.k.lsb_k_seq_dots(n, 1, d_d0, ld, d_w0, d_parts, d_s + 8 * (m + 1), dev.stream)
        dev.sync()
        sums = dev.get(d_s, MAXD + 2)
    assert _same(out[:m + 2], sums[:m + 2]), (out[:m + 2], sums[:m + 2])
    if coarse:  # multiples of 2^-22 below 17: exact
        assert np.array_equal(d1[:n], d - beta[:m] @ X[:m, :n]) and np.array_equal(w1[:n], w - beta[:m] @ SX[:m, :n])
    else:
        for got, start, B, what in ((d1, d, X, "d'"), (w1, w, SX, "w'")):
            exact, mags = _exact_chain(start, -beta, B, m, n)
            _check_elements(got[:n], exact, mags, m, what)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS + [N_SECOND_TURN])
def test_store(hip, n):
    rng = np.random.default_rng(400 + n % 97)
    d, w = _values(rng, n, False), _values(rng, n, False)
    with _device(hip) as dev:
        d_d, d_w = dev.put(d), dev.put(w)
        for nu in (3.7e-5, 1.0, 2.9e11):
            runs = []
            for off in (0, 0, 1):
                d_xs, d_sxs = dev.put(np.full(n + 3, -7.0), off), dev.put(np.full(n + 3, -7.0), off)
                d_sc, d_rec = dev.put([nu, 123.25]), dev.put([-7.0] * 4)
                dev.k.lsb_k_seq_store(n, d_d, d_w, d_xs, d_sxs, d_sc, d_sc + 8, d_rec, dev.stream)
                dev.sync()
                runs.append((dev.get(d_xs, n + 3), dev.get(d_sxs, n + 3), dev.get(d_rec, 4)))
            xs, sxs, rec = runs[0]
            for r in runs[1:]:
                assert _same(r[0], xs) and _same(r[1], sxs) and _same(r[2], rec)
            assert list(rec) == [123.25, nu, 1.0, -7.0]
            assert (xs[n:] == -7.0).all() and (sxs[n:] == -7.0).all()
            for got, src in ((xs, d), (sxs, w)):
                want = src / np.sqrt(nu)
                assert (np.abs(got[:n] - want) <= np.spacing(np.abs(want))).all()
        # nothing but the record where nu is not a finite positive number: set in the device record, nothing faults
        for nu in (0.0, -1.0, float("nan"), float("inf")):
            d_xs, d_sxs = dev.put(np.full(n + 3, -7.0)), dev.put(np.full(n + 3, -7.0))
            d_sc, d_rec = dev.put([nu, 5.5]), dev.put([-7.0] * 4)
            dev.k.lsb_k_seq_store(n, d_d, d_w, d_xs, d_sxs, d_sc, d_sc + 8, d_rec, dev.stream)
            dev.sync()
            rec = dev.get(d_rec, 4)
            assert rec[0] == 5.5 and _same(rec[1], nu) and rec[2] == 0.0 and rec[3] == -7.0
            assert (dev.get(d_xs, n + 3) == -7.0).all() and (dev.get(d_sxs, n + 3) == -7.0).all()
