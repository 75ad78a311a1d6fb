"""The block-CG kernels of lsbench_amd/csrc/hip_bcg.hip and hip_bcg_m.hip (shared pieces: hip_mrhs_k.h) one by one,
each against its rule restated in numpy longdouble.

The end-to-end tests of test_block_cg.py and test_block_cg_precond.py cannot see a wrong coefficient: the method
corrects itself, a transposed zeta, an xs built with the wrong sigma, a Gram entry dealt to the wrong lane or a record
dropped by small_sum_records all converge a few iterations late, inside every bound those tests have.  Here every
launcher is called on its own through ctypes, as hip_bcg_drv.c calls it, on inputs of mixed sign and magnitude
(1e-3 .. 1e3) from a fixed seed.  Everything a kernel must not read holds NaN -- the lower triangle of an
upper-triangular matrix of the state, what lies beyond kp in the stride-8 matrices, the buffer behind the last
record -- and everything it must not write holds a sentinel that is compared bit for bit.

Without a GPU: the mirror of struct lsb_blockcg_state and the argument tables against lsb_impl.h, the longdouble
restatements of the small phases against numpy's factorisations and against the matrices block_pcg (test_block_cg.py)
forms on the 40 x 30 Laplacian, and the inputs of the pivot-floor cases in exact arithmetic.

Tolerances.  None is measured on the code under test; u = eps / 2 is one rounding, k = kp.

 (S) A sum, or a short chain of fma, whose longest addition chain is L: a term passes through at most L additions, the
     error is at most L u sum|terms| to first order, the tests allow 2 L eps sum|terms| (test_gmres_kernels.py's
     rule; the rounding of a product formed outside the fma is inside the factor).  The chains:
       a vector element of a pass      k fused steps (k + 1 where D^-1 w is added in front)
       a record of a streaming pass    (trips of a lane) + 6 butterfly steps + 2 LDS additions
       a record of a row kernel        (trips of a lane) + log2(64 / lanes) butterfly steps + 2 LDS additions
       a row of Q = S P                ceil(entries / lanes) fused steps + log2(lanes) butterfly steps
       small_sum_records               ceil(nrecords / NR) + NR, NR = 1024 // W
       xs = xi sigma, sigma = zeta sigma   k ; rr_c = sigma_c^T H sigma_c: two nested chains, 2 k
     The error (S) of a summed Gram matrix is called dA below and is added wherever that matrix is the input.
 (C) A Cholesky factor F^T F = A computed in any order satisfies |F^T F - A| <= gamma_{k+1} |F^T| |F| elementwise
     (Higham, Accuracy and Stability, thm 10.3).  The start also takes d = sqrt(diag), forms d_i d_j, divides by it and
     scales the factor back: five more roundings.  Allowed: (k + 6) eps |F^T| |F| + dA, about twice the bound.
 (I) Column c of the inverse of a triangle by substitution solves (L + dL) x = e_c with |dL| <= gamma_k |L|, so
     |L X - I| <= gamma_k |L| |X|; zinv zeta - I is its transpose.  Allowed: (k + 1) eps |zinv| |zeta|.
 (F) Forward comparisons need a condition number, which comes from the INPUT: part A builds every Gram matrix as
     D M D, M with a diagonal in [1, 2] and off-diagonal magnitudes <= 1 / (2 k) -- eigenvalues in [1/2, 5/2] by
     Gershgorin, cond <= 5 (asserted) -- and D a diagonal of signed powers of two (2^-10 .. 2^10), a scaling that every
     step of the factorisation, of the substitution and of the products commutes with exactly, so the bounds of M hold
     entry by entry after scaling.  Part E takes the eigenvalues of the matrix the device summed.
       factor: ||dL||_F <= cond / sqrt 2 * ||dA||_F / ||A|| * ||L|| (Sun; Higham thm 10.8), ||dA||_F <= k gamma_{k+6}
               ||A|| by (C).  Allowed per entry: cond k (k + 6) eps sqrt(lambda_max), times the scale of its column.
       xi = C^-T C^-1: the factor's backward error moves the inverse by cond ||A^-1|| k (k + 1) u, the substitution's
               residual ((I), twice) by 2 k^2 sqrt(cond) ||A^-1|| u, the product by k^2 ||A^-1|| u: together
               <= (4 k^2 + k) cond ||A^-1|| u.  Allowed per entry: 4 k (k + 1) cond eps ||A^-1||, scaled, plus
               2 |A^-1| dA |A^-1|.
       a pivot of the unit-diagonal matrix is the square of a diagonal entry of its factor (<= sqrt(3/2)):
               2 sqrt(3/2) times the factor's allowance.

xi is symmetric to the bit -- entry (i, j) and entry (j, i) are the same fma chain with commuted factors -- which
test_gamma asserts; an xs formed from the transposed xi is therefore the same xs, and no test can tell the two apart."""
import contextlib
import ctypes as C
import fractions
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
BS, WGS, WG = 8, 1024, 256           # LSB_MRHS_MAX, threads of k_bcg_small, threads of every other kernel
PASS_CAP, MAX_PARTIALS, NXCD = 512, 2048, 8  # BCG_PASS_GRID, LSB_MAX_PARTIALS, XCDs the row kernels' grid is aligned to
RUNNING, CONVERGED, BREAKDOWN, MAXIT = 0, 1, 2, 3
START, GAMMA, G, VERIFY = 0, 1, 2, 3  # lsb_k_blockcg_small's phase
KPS = (2, 4, 8)
LANES = (2, 4, 8, 16, 32, 64)
FLOOR = 1e-10                        # the rank rule of the start
PAD = 3                              # rows (or records) of slack behind every device array
SLACK = -7.25

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")

NS = [1, 2, 255, 256, 257, 65536, 65537]
N_CAPPED = 512 * 1024 + 1025  # asks for 514 workgroups, gets BCG_PASS_GRID; a ragged fifth trip


class BcgState(C.Structure):
    """struct lsb_blockcg_state (lsb_impl.h); test_state_mirror_matches_header guards it."""
    _fields_ = [("xi", C.c_double * (BS * BS)), ("xs", C.c_double * (BS * BS)), ("zeta", C.c_double * (BS * BS)),
                ("zinv", C.c_double * (BS * BS)), ("sigma", C.c_double * (BS * BS)),
                ("rr", C.c_double * BS), ("bb", C.c_double * BS), ("thresh2", C.c_double * BS),
                ("true_relres", C.c_double * BS), ("tol", C.c_double), ("min_pivot", C.c_double),
                ("status", C.c_int * BS), ("iters", C.c_int), ("maxit", C.c_int), ("nrhs", C.c_int),
                ("running", C.c_int), ("nspmm", C.c_int), ("rank_bad", C.c_int)]


MATS = ("xi", "xs", "zeta", "zinv", "sigma")

_vp, _sz, _u, _i, _d = C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_double
# name -> (restype, argtypes), from the prototypes of lsb_impl.h; test_launcher_tables_match_header guards it.
# The 13 launchers and, last, the record width lsb_k_blockcg_tri.
LAUNCHERS = {
    "lsb_k_spmm_grid": (_u, [_u, _u]),
    "lsb_k_spmm_csr": (None, [_u, _u, _vp, _vp, _vp, _u, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_init": (None, [_u, _u, _vp, _vp, _d, _vp, _vp, _vp]),
    "lsb_k_blockcg_small": (None, [_u, _i, _vp, _vp, _u, _u, _d, _i, _vp]),
    "lsb_k_blockcg_start": (None, [_u, _u, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_spmm": (None, [_u, _u, _vp, _vp, _vp, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_pass_a": (None, [_u, _u, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_pass_b": (None, [_u, _u, _vp, _vp, _vp, _d, _vp, _vp]),
    "lsb_k_blockcg_m_pass_a": (None, [_u, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_m_gram": (None, [_u, _i, _u, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_m_gt_gram": (None, [_u, _u, _vp, _vp, _vp, _u, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_m_start": (None, [_u, _u, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_m_pass_b": (None, [_u, _u, _vp, _vp, _vp, _vp, _vp]),
    "lsb_k_blockcg_tri": (_u, [_u]),
}


# ------------------------------------------------------------------------------ the launchers' own rules
def tri_of(kp):
    return kp * (kp + 1) // 2


def _ceil(a, b):
    return -(-a // b)


def rows_per_wg(n, g, lanes):
    """the contiguous range of rows a workgroup of a row kernel owns: a multiple of its WG / lanes rows per trip"""
    slots = WG // lanes
    return _ceil(_ceil(n, g), slots) * slots


def small_width(phase, kp):
    """doubles of a record that k_bcg_small sums in the phase"""
    return {START: tri_of(kp) + kp, GAMMA: tri_of(kp), G: 2 * tri_of(kp), VERIFY: kp}[phase]


def pass_grid(n):
    """workgroups of a streaming pass (pass_grid, hip_mrhs_k.h)"""
    g = -(-max(n, 1) // WG)
    if g > 256:
        g = max(-(-n // (4 * WG)), 256)
    return min(g, PASS_CAP)


def spmm_grid(n, lanes):
    """workgroups of a row kernel (lsb_k_spmm_grid)"""
    g = -(-max(-(-n // (WG // lanes)), 1) // NXCD) * NXCD
    return min(g, MAX_PARTIALS)


def sum_chain(nrecords, W):
    NR = WGS // W
    return -(-nrecords // NR) + NR


# ------------------------------------------------------------------ restatements (longdouble)
def ref_chol(A, floor=0.0):
    """A = L L^T, right-looking as small_chol.  -> (L, bad, the smallest pivot); bad: a pivot that is not > floor or
    not finite, and then L is nobody's to use."""
    A = np.array(A, LD)
    k = A.shape[0]
    bad, piv = False, LD(np.inf)
    with np.errstate(all="ignore"):
        for j in range(k):
            d = A[j, j]
            if not (d > floor) or not np.isfinite(d):
                bad = True
            if not (d >= piv):
                piv = d
            A[j, j] = np.sqrt(d)
            A[j + 1:, j] /= A[j, j]
            for i in range(j + 1, k):
                A[i, j + 1:i + 1] -= A[i, j] * A[j + 1:i + 1, j]
    return np.tril(A), bad, piv


def ref_linv(L):
    """L^-1 of a lower triangle, column by column by forward substitution as small_linv"""
    k = L.shape[0]
    X = np.zeros((k, k), LD)
    with np.errstate(all="ignore"):
        for c in range(k):
            X[c, c] = 1 / L[c, c]
            for i in range(c + 1, k):
                X[i, c] = -(L[i, c:i] @ X[c:i, c]) / L[i, i]
    return X


def tri_sym(tri, kp, nrhs):
    """the symmetric matrix of an upper-triangle record (row by row), the identity on the padding's diagonal"""
    A = np.zeros((kp, kp), LD)
    A[np.triu_indices(kp)] = np.asarray(tri, LD)[:tri_of(kp)]
    A = A + np.triu(A, 1).T
    for i in range(nrhs, kp):
        A[i, i] = 1
    return A


def ref_start(A):
    """START: A scaled to unit diagonal, factored with the floor; sigma = L^T, zinv = sigma^-1"""
    A = np.asarray(A, LD)
    with np.errstate(all="ignore"):
        d = np.sqrt(np.diag(A))
        As = A / np.outer(d, d)
        Ls, bad, piv = ref_chol(As, FLOOR)
        L = d[:, None] * Ls
        return dict(bad=bad, piv=piv, d=d, As=As, sigma=L.T, zinv=ref_linv(L).T)


def ref_gamma(A, sigma):
    """GAMMA: xi = A^-1 through the factor, xs = xi sigma (sigma upper triangular)"""
    Cf, bad, _ = ref_chol(A)
    Ci = ref_linv(Cf)
    with np.errstate(all="ignore"):
        xi = Ci.T @ Ci
        return dict(bad=bad, xi=xi, xs=xi @ np.triu(np.asarray(sigma, LD)))


def ref_g(A, H, sigma):
    """G: rr_c = sigma_c^T H sigma_c with the incoming sigma; zeta = L^T of A, its inverse, sigma = zeta sigma"""
    s = np.triu(np.asarray(sigma, LD))
    H = np.asarray(H, LD)
    L, bad, _ = ref_chol(A)
    with np.errstate(all="ignore"):
        k = s.shape[0]  # (column c meets rows and columns 0 .. c alone: a NaN further down is not its own)
        rr = np.array([s[:c + 1, c] @ H[:c + 1, :c + 1] @ s[:c + 1, c] for c in range(k)], LD)
        rr_mag = np.array([np.abs(s[:c + 1, c]) @ np.abs(H[:c + 1, :c + 1]) @ np.abs(s[:c + 1, c]) for c in range(k)], LD)
        return dict(bad=bad, rr=rr, rr_mag=rr_mag, zeta=L.T, zinv=ref_linv(L).T, sigma=L.T @ s)


def eig_bounds(M):
    """(cond, lambda_max, 1 / lambda_min) of the symmetric matrix whose conditioning a forward bound needs"""
    ev = np.linalg.eigvalsh(np.asarray(M, np.float64))
    assert ev[0] > 0
    return float(ev[-1] / ev[0]), float(ev[-1]), float(1 / ev[0])


def tol_factor(M, k):
    cond, hi, _ = eig_bounds(M)
    return cond * k * (k + 6) * EPS * math.sqrt(hi)


def tol_inverse(M, k):
    cond, _, ninv = eig_bounds(M)
    return 4 * k * (k + 1) * cond * EPS * ninv


# ------------------------------------------------------------------------------------ inputs
def _rand(rng, *shape):
    """mixed signs, magnitudes log-uniform over [1e-3, 1e3]"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def _pow2(rng, k):
    """signed powers of two, 2^-10 .. 2^10: a scaling that commutes with every rounding"""
    return rng.choice([-1.0, 1.0], size=k) * 2.0 ** rng.integers(-10, 11, size=k)


def _gram(rng, k, scaled=True):
    """-> (D M D, M, d): M symmetric, diagonal in [1, 2], off-diagonal magnitudes <= 1 / (2 k): eigenvalues in
    [1/2, 5/2] by Gershgorin; D = diag(d) signed powers of two (the product is exact, so D M D is symmetric)"""
    M = np.triu(rng.uniform(-1.0, 1.0, size=(k, k)) / (2 * k), 1)
    M = M + M.T
    M[np.arange(k), np.arange(k)] = rng.uniform(1.0, 2.0, size=k)
    d = _pow2(rng, k) if scaled else np.ones(k)
    A = d[:, None] * M * d[None, :]
    assert np.array_equal(A, A.T) and eig_bounds(M)[0] <= 5.0
    return A, M, d


def _upper(rng, k):
    """a full-looking upper triangle of mixed sign and magnitude"""
    return np.triu(_rand(rng, k, k))


def _tri(A):
    return np.asarray(A)[np.triu_indices(A.shape[0])]


def _floor_case(kp, bits):
    """The Gram record of the rank rule at its floor: diagonal 1 except the last two columns, 4 and 1/16, whose
    correlation is c = 1 - 2^-bits.  -> (the record T + kp as fp64, c as a Fraction)"""
    c = 1 - fractions.Fraction(1, 2 ** bits)
    A = np.eye(kp)
    A[kp - 2, kp - 2], A[kp - 1, kp - 1] = 4.0, 1.0 / 16
    A[kp - 2, kp - 1] = A[kp - 1, kp - 2] = float(c / 2)  # c sqrt(4 / 16)
    return np.concatenate([_tri(A), np.ones(kp)]), c


# ------------------------------------------------------------------------ without a GPU
def _header():
    with open(os.path.join(CSRC, "lsb_impl.h")) as f:
        return f.read()


def test_launcher_tables_match_header():
    """argtypes / restype of every launcher as lsb_impl.h declares them: a pointer (and the stream) c_void_p, size_t
    c_size_t, unsigned c_uint, double c_double, int c_int."""
    text = _header()

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _vp
        words = decl.split()
        if words[0] == "void" and len(words) == 1:
            return None
        return {"size_t": _sz, "unsigned": _u, "double": _d, "int": _i}[words[0]]
    assert len(LAUNCHERS) == 13 + 1
    for name, (res, args) in LAUNCHERS.items():
        m = re.search(r"^([\w ]+?)\s*\b%s\(([^)]*)\);" % name, text, re.M)
        assert m, name + " is not declared in lsb_impl.h"
        assert ctype(m.group(1)) == res, name
        assert [ctype(p) for p in m.group(2).split(",")] == args, name
    declared = set(re.findall(r"\b(lsb_k_blockcg_\w+)\(", text))
    assert declared == {n for n in LAUNCHERS if n.startswith("lsb_k_blockcg_")}, "a launcher without a test"


def test_state_mirror_matches_header(tmp_path):
    """sizeof and every offsetof of struct lsb_blockcg_state, and the constants, from a C program compiled against
    lsb_impl.h with the include paths of the csrc Makefile."""
    names = [f[0] for f in BcgState._fields_]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include \"lsb_impl.h\"\n"
        "#define O(m) printf(#m \" %zu\\n\", offsetof(struct lsb_blockcg_state, m));\n"
        "int main(void) {\n"
        "  printf(\"sizeof %zu\\n\", sizeof(struct lsb_blockcg_state));\n"
        "  printf(\"MRHS_MAX %d\\nMAX_PARTIALS %d\\nGRID_CAP %d\\n\", LSB_MRHS_MAX, LSB_MAX_PARTIALS, LSB_STREAM_GRID_CAP);\n"
        "  printf(\"PHASES %d %d %d %d\\n\", LSB_BLOCKCG_START, LSB_BLOCKCG_GAMMA, LSB_BLOCKCG_G, LSB_BLOCKCG_VERIFY);\n"
        "  printf(\"STATUS %d %d %d %d\\n\", LSB_STATUS_RUNNING, LSB_STATUS_CONVERGED, LSB_STATUS_BREAKDOWN, LSB_STATUS_MAXIT);\n"
        "  " + " ".join("O(%s)" % n for n in names) + "\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-I" + os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include")]
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11"] + inc + [str(src), "-o", str(exe)], check=True)
    out = dict(line.split(None, 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(BcgState)
    assert int(out["MRHS_MAX"]) == BS and int(out["MAX_PARTIALS"]) == MAX_PARTIALS
    assert int(out["GRID_CAP"]) >= PASS_CAP
    assert out["PHASES"].split() == [str(v) for v in (START, GAMMA, G, VERIFY)]
    assert out["STATUS"].split() == [str(v) for v in (RUNNING, CONVERGED, BREAKDOWN, MAXIT)]
    for n in names:
        assert int(out[n]) == getattr(BcgState, n).offset, n
    assert all(getattr(BcgState, n).size == BS * BS * 8 for n in MATS)
    assert BcgState.status.offset % 8 == 0  # _state fills the doubles in front of it as one array


def test_the_grid_rules_restated():
    """pass_grid and spmm_grid at the sizes the GPU cases rely on (the GPU cases compare them with what the launchers
    report)"""
    assert [pass_grid(n) for n in NS] == [1, 1, 1, 1, 2, 256, 256]
    assert pass_grid(N_CAPPED) == PASS_CAP and -(-N_CAPPED // (PASS_CAP * WG)) == 5
    assert spmm_grid(1, 64) == 8 and spmm_grid(33, 64) == 16 and spmm_grid(33, 2) == 8
    for L, n in ((64, 8197), (2, 262147)):
        g = spmm_grid(n, L)
        assert g == MAX_PARTIALS and n > MAX_PARTIALS * (WG // L) and rows_per_wg(n, g, L) == 2 * (WG // L)


@pytest.mark.parametrize("k", KPS)
def test_restatements_vs_numpy(k):
    """ref_start, ref_gamma and ref_g on the constructed matrices against numpy.linalg.cholesky and inv: the factor
    and the inverse agree within the forward bounds (F) -- numpy's own fp64 factorisation has the backward error
    those bounds start from --, the identities hold to longdouble rounding."""
    rng = np.random.default_rng(100 + k)
    epl = float(np.finfo(LD).eps)
    A, M, d = _gram(rng, k)
    ad = np.abs(d)
    r = ref_start(A)
    assert not r["bad"]
    assert (np.abs(r["sigma"].T @ r["sigma"] - A) <= 8 * k * epl * (np.abs(r["sigma"]).T @ np.abs(r["sigma"]))).all()
    assert (np.abs(r["zinv"] @ r["sigma"] - np.eye(k)) <= 8 * k * epl * (np.abs(r["zinv"]) @ np.abs(r["sigma"]))).all()
    As = np.asarray(r["As"], np.float64)
    assert eig_bounds(As)[0] <= 3.0 + 1e-12  # unit diagonal, off-diagonal magnitudes <= 1 / (2 k): [1/2, 3/2]
    tf = tol_factor(As, k) * np.sqrt(np.diag(A))
    assert (np.abs(r["sigma"] - np.linalg.cholesky(A).T) <= tf[None, :]).all()
    piv = np.diag(np.linalg.cholesky(As)).min() ** 2
    assert abs(float(r["piv"]) - piv) <= 2 * math.sqrt(1.5) * tol_factor(As, k)
    sigma = _upper(rng, k)
    g = ref_gamma(A, sigma)
    assert not g["bad"]
    assert (np.abs(g["xi"] - np.linalg.inv(A)) <= tol_inverse(M, k) / np.outer(ad, ad)).all()
    H = _rand(rng, k, k)
    H = np.triu(H) + np.triu(H, 1).T
    q = ref_g(A, H, sigma)
    assert (np.abs(q["zeta"] - np.linalg.cholesky(A).T) <= (tol_factor(M, k) * ad)[None, :]).all()
    assert (np.abs(q["zinv"] @ q["zeta"] - np.eye(k)) <= 8 * k * epl * (np.abs(q["zinv"]) @ np.abs(q["zeta"]))).all()
    rr64 = np.einsum("ic,ij,jc->c", sigma, H, sigma)
    assert (np.abs(q["rr"] - rr64) <= 4 * k * EPS * q["rr_mag"]).all()
    assert (np.abs(q["sigma"] - np.linalg.cholesky(A).T @ sigma)
            <= 2 * k * EPS * (np.abs(q["zeta"]) @ np.abs(sigma)) + tol_factor(M, k) * ad.max() * np.abs(sigma).sum(axis=0)).all()
    # what is not positive is bad, in each rule's own sense
    assert ref_chol(-A)[1] and ref_chol(np.full((k, k), np.nan))[1] and ref_start(np.zeros((k, k)))["bad"]


@pytest.mark.parametrize("k", KPS)
def test_restatements_vs_block_pcg(k):
    """The matrices block_pcg forms at its start and in its first two iterations on the 40 x 30 Laplacian: the
    restatements, fed its Gram matrices, give its sigma, xi, zeta, rr and next sigma within the forward bounds (F)
    with the eigenvalues of those matrices."""
    from test_block_cg import LAP, block_pcg, columns8
    from test_mrhs import _lap2d
    S = _lap2d(*LAP).tocsr()
    B = columns8(S)[:, :k]
    trace = []
    block_pcg(S, B, 1e-10, maxit=3, trace=trace)
    assert len(trace) >= 3
    r = ref_start(trace[0]["G"])
    tf = tol_factor(r["As"], k) * np.sqrt(np.diag(trace[0]["G"]))
    assert not r["bad"] and (np.abs(r["sigma"] - trace[0]["sigma"]) <= tf[None, :]).all()
    sigma = trace[0]["sigma"]
    for t in trace[1:3]:
        g = ref_gamma(t["Gam"], sigma)
        assert not g["bad"] and np.abs(g["xi"] - t["xi"]).max() <= tol_inverse(t["Gam"], k)
        Gs = np.triu(t["G"]) + np.triu(t["G"], 1).T
        q = ref_g(Gs, t["H"], sigma)
        assert not q["bad"] and np.abs(q["zeta"] - t["zeta"]).max() <= tol_factor(Gs, k)
        assert (np.abs(q["rr"] - t["rr"]) <= 4 * k * EPS * q["rr_mag"]).all()
        assert (np.abs(q["sigma"] - t["sigma"]) <= 2 * k * EPS * (np.abs(q["zeta"]) @ np.abs(sigma))
                + tol_factor(Gs, k) * np.abs(sigma).sum(axis=0)).all()
        sigma = t["sigma"]


@pytest.mark.parametrize("kp", KPS)
def test_pivot_floor_inputs_in_exact_arithmetic(kp):
    """The two records of the rank rule at its floor hold exactly what they claim (fractions.Fraction): after the
    scaling to unit diagonal, which is exact on powers of two, the last pivot is 1 - c^2; with c = 1 - 2^-32 it lies
    above the floor -- the fp64 constant 1e-10 -- and with c = 1 - 2^-36 below it."""
    F = fractions.Fraction
    floor = F(FLOOR)
    for bits, above in ((32, True), (36, False)):
        rec, c = _floor_case(kp, bits)
        A = tri_sym(rec, kp, kp)
        a, b, o = F(float(A[kp - 2, kp - 2])), F(float(A[kp - 1, kp - 1])), F(float(A[kp - 2, kp - 1]))
        assert (a, b) == (4, F(1, 16)) and o == c / 2          # the record holds c / 2 exactly
        assert math.sqrt(float(a)) == 2.0 and math.sqrt(float(b)) == 0.25
        cs = o / (2 * F(1, 4))                                  # the scaled off-diagonal entry
        assert cs == c and F(float(cs)) == cs
        pivot = 1 - cs * cs
        assert (pivot > floor) == above and (pivot < floor) == (not above)
        assert abs(float(pivot) - (4.7e-10 if above else 2.9e-11)) <= 0.05 * float(pivot)
        # every other pivot is 1, and fp64 gets this one within one rounding of c^2
        assert abs(F(1.0 - float(cs) * float(cs)) - pivot) <= F(EPS)
        assert (float(ref_start(A)["piv"]) > FLOOR) == above


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

    def put(self, a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype)
        assert a.nbytes > 0
        p = self.lib.lsb_hip_malloc(a.nbytes)
        assert p
        self._ptrs.append(p)
        assert self.lib.lsb_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    def write(self, p, a):
        a = np.ascontiguousarray(a, np.float64)
        assert self.lib.lsb_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0

    def get(self, p, shape):
        a = np.empty(shape, np.float64)
        assert self.lib.lsb_hip_memcpy_d2h(a.ctypes.data, p, a.nbytes) == 0
        return a

    def put_state(self, st):
        p = self.lib.lsb_hip_malloc(C.sizeof(BcgState))
        assert p
        self._ptrs.append(p)
        self.write_state(p, st)
        return p

    def write_state(self, p, st):
        assert self.lib.lsb_hip_memcpy_h2d(p, C.addressof(st), C.sizeof(BcgState)) == 0

    def get_state(self, p):
        st = BcgState()
        assert self.lib.lsb_hip_memcpy_d2h(C.addressof(st), p, C.sizeof(BcgState)) == 0
        return st

    def sync(self):
        assert self.lib.lsb_hip_sync() == 0

    def close(self):
        while self._ptrs:
            self.lib.lsb_hip_free(self._ptrs.pop())

    # the launchers as the driver calls them, each followed by a synchronisation; those that report a record count
    # return it
    def small(self, kp, phase, dst, drec, nrec, nrhs=0, tol=0.0, maxit=0):
        assert kp in KPS and nrec >= 1
        self.k.lsb_k_blockcg_small(kp, phase, dst, drec, nrec, nrhs, tol, maxit, self.stream)
        self.sync()

    def _counted(self, fn, *args):
        nr = C.c_uint(0xFFFFFFFF)
        fn(*args, C.addressof(nr), self.stream)
        self.sync()
        return nr.value

    def init(self, kp, n, b, dinv, dc, rec):
        return self._counted(self.k.lsb_k_blockcg_init, kp, n, b, dinv, dc, rec)

    def start(self, kp, n, b, dinv, dc, w, p, x, st):
        self.k.lsb_k_blockcg_start(kp, n, b, dinv, dc, w, p, x, st, self.stream)
        self.sync()

    def pass_a(self, kp, n, w, q, p, x, dinv, dc, st, rec):
        return self._counted(self.k.lsb_k_blockcg_pass_a, kp, n, w, q, p, x, dinv, dc, st, rec)

    def pass_b(self, kp, n, w, p, dinv, dc, st):
        self.k.lsb_k_blockcg_pass_b(kp, n, w, p, dinv, dc, st, self.stream)
        self.sync()

    def m_pass_a(self, kp, n, w, q, p, x, st):
        self.k.lsb_k_blockcg_m_pass_a(kp, n, w, q, p, x, st, self.stream)
        self.sync()

    def m_gram(self, kp, start, n, a, z, rec, st):
        nr = C.c_uint(0xFFFFFFFF)
        self.k.lsb_k_blockcg_m_gram(kp, start, n, a, z, rec, C.addressof(nr), st, self.stream)
        self.sync()
        return nr.value

    def m_start(self, kp, n, b, z, w, p, x, st):
        self.k.lsb_k_blockcg_m_start(kp, n, b, z, w, p, x, st, self.stream)
        self.sync()

    def m_pass_b(self, kp, n, w, z, p, st):
        self.k.lsb_k_blockcg_m_pass_b(kp, n, w, z, p, st, self.stream)
        self.sync()

    def spmm(self, kp, n, csr, lanes, p, q, rec, st):
        nr = C.c_uint(0xFFFFFFFF)
        self.k.lsb_k_blockcg_spmm(kp, n, csr[0], csr[1], csr[2], lanes, p, q, rec, C.addressof(nr), st, self.stream)
        self.sync()
        return nr.value

    def gt_gram(self, kp, n, csr, lanes, t, wt, z, rec, st):
        nr = C.c_uint(0xFFFFFFFF)
        self.k.lsb_k_blockcg_m_gt_gram(kp, n, csr[0], csr[1], csr[2], lanes, t, wt, z, rec, C.addressof(nr), st,
                                       self.stream)
        self.sync()
        return nr.value

    def spmm_csr(self, kp, n, csr, lanes, x, y, partials):
        nr = C.c_uint(0xFFFFFFFF)
        self.k.lsb_k_spmm_csr(kp, n, csr[0], csr[1], csr[2], lanes, x, y, None, partials, C.addressof(nr), None,
                              self.stream)
        self.sync()
        return nr.value


@contextlib.contextmanager
def _device(la):
    dev = _Dev(la)
    try:
        yield dev
    finally:
        dev.close()


NDBL = BcgState.status.offset // 8  # doubles in front of the ints


def _mat(st, name, kp=BS):
    return np.array(getattr(st, name)[:], np.float64).reshape(BS, BS)[:kp, :kp]


def _vec(member):
    return np.array(member[:], np.float64)


def _embed(M, upper=False):
    """a kp x kp matrix in the stride-8 layout; NaN beyond kp and, of an upper-triangular matrix, below the diagonal"""
    kp = M.shape[0]
    A = np.full((BS, BS), np.nan)
    A[:kp, :kp] = np.where(np.triu(np.ones((kp, kp), bool)), M, np.nan) if upper else M
    return A.ravel()


def _state(nrhs=BS, **kw):
    """A state whose every double is a distinct finite sentinel and whose ints look like a block in its loop, then the
    named members (arrays may be shorter than the member)."""
    st = BcgState()
    C.memmove(C.addressof(st), (-(np.arange(NDBL) + 1000.0) / 7.0).ctypes.data, NDBL * 8)
    st.status[:] = [RUNNING] * nrhs + [CONVERGED] * (BS - nrhs)
    st.iters, st.maxit, st.nrhs, st.running, st.nspmm, st.rank_bad = 3, 1000, nrhs, 1, 3, 0
    for k, v in kw.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            m = getattr(st, k)
            vals = np.asarray(v).ravel()
            m[:len(vals)] = [type(m[0])(t) for t in vals]
        else:
            setattr(st, k, v)
    return st


def _copy(st):
    return BcgState.from_buffer_copy(bytes(st))


def _set_block(st, name, M):
    """the kp x kp block of a matrix of the state"""
    kp = M.shape[0]
    m = getattr(st, name)
    for i in range(kp):
        m[i * BS:i * BS + kp] = [float(v) for v in M[i]]


def _member_bytes(st, f):
    off, size = getattr(BcgState, f).offset, getattr(BcgState, f).size
    return bytes(st)[off:off + size]


def _diff(a, b):
    """the members in which two states differ, for a failure's message"""
    return [f for f, _ in BcgState._fields_ if _member_bytes(a, f) != _member_bytes(b, f)]


def _records(rng, nrec, W, target=None):
    """nrec records of width W of mixed sign and magnitude and PAD records of NaN behind them; where target (a prefix
    of the components) is given, one record is replaced so that those components sum to it (up to its rounding).
    -> (the buffer, the longdouble sums, the allowance (S) of k_bcg_small's sums)"""
    R = _rand(rng, nrec, W)
    if target is not None:
        t = np.asarray(target, LD)
        j = int(rng.integers(nrec))
        R[j, :t.size] = 0.0
        R[j, :t.size] = (t - R[:, :t.size].astype(LD).sum(axis=0)).astype(np.float64)
    buf = np.full((nrec + PAD, W), np.nan)
    buf[:nrec] = R
    with np.errstate(invalid="ignore"):
        sums = R.astype(LD).sum(axis=0)
        allow = 2 * sum_chain(nrec, W) * EPS * np.abs(R).astype(LD).sum(axis=0)
    return buf, sums, allow


def _nrecords(W):
    NR = WGS // W
    return sorted({v for v in (1, 2, NR - 1, NR, NR + 1, 4 * NR, 4 * NR + 1, 16 * NR + 1, 512, 768, 2048) if v >= 1})


def _tri_allow(allow, kp):
    """the allowance of a summed triangle as a symmetric matrix (0 where it is NaN: the padding's diagonal)"""
    return np.nan_to_num(np.asarray(tri_sym(np.nan_to_num(np.asarray(allow[:tri_of(kp)], np.float64)), kp, kp)))


# ------------------------------------------------------------------- checks of the small phases
def _check_factor(F, zinv, A, dA, kp, M, scale, what):
    """an upper factor F of A = F^T F the device stored, and its inverse: (C), (I), (F)"""
    F, zinv = F.astype(LD), zinv.astype(LD)
    assert not np.tril(F, -1).any() and not np.tril(zinv, -1).any(), what + ": not upper triangular"
    back = np.abs(F.T @ F - A)
    allow = (kp + 6) * EPS * (np.abs(F).T @ np.abs(F)) + dA
    assert (back <= allow).all(), "%s: F^T F - A, err/allowed %s" % (what, (back / allow).astype(np.float64))
    res = np.abs(zinv @ F - np.eye(kp))
    allow = (kp + 1) * EPS * (np.abs(zinv) @ np.abs(F))
    assert (res <= allow).all(), "%s: zinv F - I, err/allowed %s" % (what, (res / allow).astype(np.float64))
    L, bad, _ = ref_chol(A)
    assert not bad
    # (F); a summed input moves the factor of M = D^-1 A D^-1 as any other perturbation dM = D^-1 dA D^-1 does:
    # cond / sqrt 2 * ||dM||_F / lambda_max * sqrt(lambda_max)
    cond, hi, _ = eig_bounds(M)
    fwd = np.abs(F - L.T)
    dM = float(np.linalg.norm(np.asarray(dA, np.float64) / np.outer(scale, scale)))
    allow = (tol_factor(M, kp) + cond * dM / math.sqrt(hi)) * np.abs(scale)[None, :]
    assert (fwd <= allow).all(), "%s: the factor, err/allowed %s" % (what, (fwd / allow).astype(np.float64))


def check_start(st, Gtri, dG, bbsum, dbb, kp, nrhs, tol, maxit, piv_allow=None):
    """the whole state after START, from the longdouble sums of the records it was given"""
    A = tri_sym(Gtri, kp, nrhs)
    r = ref_start(A)
    bad = r["bad"]
    eye = np.eye(BS)
    for name in ("xi", "xs"):
        assert _same(_mat(st, name), eye), name
    sigma, zeta, zinv = _mat(st, "sigma"), _mat(st, "zeta"), _mat(st, "zinv")
    assert _same(zeta, sigma)
    outside = np.ones((BS, BS), bool)
    outside[:nrhs, :nrhs] = False  # the padding and what lies beyond kp: the identity, exactly
    for name, Mx in (("sigma", sigma), ("zinv", zinv)):
        assert np.array_equal(Mx[outside], eye[outside]), name + " is not the identity on the padding"
    if bad:
        assert _same(sigma, eye) and _same(zinv, eye)
    else:
        As = np.asarray(r["As"], np.float64)
        d = np.asarray(r["d"], np.float64)
        dA = _tri_allow(dG, kp)
        _check_factor(sigma[:kp, :kp], zinv[:kp, :kp], A, dA, kp, As, d, "START")
        allow = 2 * math.sqrt(1.5) * (tol_factor(As, kp) + eig_bounds(As)[0] * float(np.abs(dA / np.outer(d, d)).sum())) \
            if piv_allow is None else piv_allow
        assert abs(LD(st.min_pivot) - r["piv"]) <= allow, (st.min_pivot, float(r["piv"]), allow)
    bb = _vec(st.bb)
    assert (np.abs(bb[:nrhs].astype(LD) - bbsum[:nrhs]) <= dbb[:nrhs]).all(), "bb"
    assert not bb[nrhs:].any() and _same(_vec(st.rr), bb)
    assert _same(_vec(st.thresh2), np.float64(tol) * np.float64(tol) * bb)
    assert _same(_vec(st.true_relres), np.full(BS, -1.0))
    want = BREAKDOWN if bad else (MAXIT if maxit <= 0 else RUNNING)
    assert st.status[:] == [want] * nrhs + [CONVERGED] * (BS - nrhs)
    assert (st.tol, st.iters, st.maxit, st.nrhs, st.nspmm) == (tol, 0, maxit, nrhs, 0)
    assert (st.running, st.rank_bad) == (int(not bad and maxit > 0), int(bad))
    return bad


def check_gamma(st0, st, Gtri, dG, kp, M=None, d=None):
    """the state after GAMMA against the state before it and the longdouble sums of the records"""
    nrhs = st0.nrhs
    A = tri_sym(Gtri, kp, nrhs)
    sigma0 = np.triu(_mat(st0, "sigma", kp))
    r = ref_gamma(A, np.nan_to_num(sigma0))
    exp = _copy(st0)
    exp.nspmm += 1
    if r["bad"]:
        exp.status[:nrhs] = [BREAKDOWN] * nrhs
        exp.running = 0
    else:
        _set_block(exp, "xi", _mat(st, "xi", kp))
        _set_block(exp, "xs", _mat(st, "xs", kp))
    assert bytes(exp) == bytes(st), "GAMMA changed %s" % _diff(exp, st)
    if r["bad"]:
        return True
    xi, xs = _mat(st, "xi", kp), _mat(st, "xs", kp)
    assert _same(xi, xi.T), "xi is not symmetric to the bit"
    M = np.asarray(A, np.float64) if M is None else M
    d = np.ones(kp) if d is None else np.abs(d)
    Ainv = np.abs(r["xi"])
    allow = tol_inverse(M, kp) / np.outer(d, d) + 2 * (Ainv @ _tri_allow(dG, kp) @ Ainv)
    err = np.abs(xi.astype(LD) - r["xi"])
    assert (err <= allow).all(), "xi: err/allowed %s" % (err / allow).astype(np.float64)
    s0 = np.nan_to_num(sigma0).astype(LD)
    err = np.abs(xs.astype(LD) - xi.astype(LD) @ s0)
    allow = 2 * kp * EPS * (np.abs(xi).astype(LD) @ np.abs(s0))
    assert (err <= allow).all(), "xs: err/allowed %s" % (err / np.maximum(allow, LD(1e-300))).astype(np.float64)
    return False


def check_g(st0, st, Gtri, Htri, dG, dH, kp, M=None, d=None):
    """the state after G against the state before it and the longdouble sums of the records.  The stop decision is
    taken from the rr the device stored (the rule tests of test_g_stop_rules give it exact operands)."""
    nrhs = st0.nrhs
    A, H = tri_sym(Gtri, kp, nrhs), tri_sym(Htri, kp, nrhs)
    sigma0 = np.nan_to_num(np.triu(_mat(st0, "sigma", kp)))
    r = ref_g(A, H, sigma0)
    rr, thr = _vec(st.rr), _vec(st0.thresh2)
    s0 = np.abs(sigma0).astype(LD)
    allow = 4 * kp * EPS * r["rr_mag"] + np.einsum("ic,ij,jc->c", s0, _tri_allow(dH, kp), s0)
    err = np.abs(rr[:nrhs].astype(LD) - r["rr"][:nrhs])
    ok = (err <= allow[:nrhs]) | (np.isnan(r["rr"][:nrhs]) & np.isnan(rr[:nrhs]))  # (a NaN norm is a NaN norm)
    assert ok.all(), "rr: err/allowed %s" % (err / allow[:nrhs]).astype(np.float64)
    exp = _copy(st0)
    exp.iters += 1
    exp.rr[:nrhs] = list(rr[:nrhs])
    met = [bool(rr[c] <= thr[c]) for c in range(nrhs)]
    outcome = "runs"
    if all(met):
        exp.status[:nrhs] = [CONVERGED] * nrhs
        exp.running, outcome = 0, "stop"
    elif exp.iters >= st0.maxit:
        exp.status[:nrhs] = [CONVERGED if m else MAXIT for m in met]
        exp.running, outcome = 0, "stop"
    elif r["bad"]:
        exp.status[:nrhs] = [BREAKDOWN] * nrhs
        exp.running, outcome = 0, "bad"
    else:
        for name in ("sigma", "zeta", "zinv"):
            _set_block(exp, name, _mat(st, name, kp))
    assert bytes(exp) == bytes(st), "G changed %s" % _diff(exp, st)
    if outcome != "runs":
        return outcome
    zeta, zinv, sigma = _mat(st, "zeta", kp), _mat(st, "zinv", kp), _mat(st, "sigma", kp)
    M = np.asarray(A, np.float64) if M is None else M
    d = np.ones(kp) if d is None else np.abs(d)
    _check_factor(zeta, zinv, A, _tri_allow(dG, kp), kp, M, d, "G")
    assert not np.tril(sigma, -1).any()
    err = np.abs(sigma.astype(LD) - zeta.astype(LD) @ sigma0.astype(LD))
    allow = 2 * kp * EPS * (np.abs(zeta).astype(LD) @ s0)
    assert (err <= allow).all(), "sigma: err/allowed %s" % (err / np.maximum(allow, LD(1e-300))).astype(np.float64)
    return outcome


def check_verify(st0, st, sums, kp, nrec):
    """VERIFY: true_relres = sqrt(sum / bb) -- the sum within (S), halved by the root, one rounding each for the
    quotient and the root: (chain + 1) eps relative --, CONVERGED -> MAXIT where it misses tol or is NaN"""
    exp = _copy(st0)
    for c in range(st0.nrhs):
        if not st0.bb[c] > 0.0:
            continue
        tr = st.true_relres[c]
        exp.true_relres[c] = tr
        with np.errstate(invalid="ignore"):
            ref = np.sqrt(sums[c] / LD(st0.bb[c]))
        if np.isnan(ref):
            assert np.isnan(tr)
        else:
            assert abs(LD(tr) - ref) <= (sum_chain(nrec, kp) + 1) * EPS * ref, (c, tr, float(ref))
        if st0.status[c] == CONVERGED and not tr <= st0.tol:
            exp.status[c] = MAXIT
    assert bytes(exp) == bytes(st), "VERIFY changed %s" % _diff(exp, st)


# ------------------------------------------------------------------ A. k_bcg_small on synthetic records
def _loop_state(rng, kp, nrhs=None, **kw):
    """a block in its loop: xi and xs full, zeta, zinv and sigma upper triangles, NaN wherever no rule reads"""
    nrhs = kp if nrhs is None else nrhs
    args = dict(xi=_embed(_rand(rng, kp, kp)), xs=_embed(_rand(rng, kp, kp)), zeta=_embed(_upper(rng, kp), True),
                zinv=_embed(_upper(rng, kp), True), sigma=_embed(_upper(rng, kp), True),
                rr=np.abs(_rand(rng, BS)), bb=np.abs(_rand(rng, BS)), thresh2=np.abs(_rand(rng, BS)),
                true_relres=np.full(BS, -1.0), tol=1e-8, min_pivot=0.5)
    args.update(kw)
    return _state(nrhs, **args)


def _run_small(dev, kp, phase, st0, buf, nrec, **kw):
    assert buf.shape[0] >= nrec and buf.shape[1] == small_width(phase, kp)
    dst, drec = dev.put_state(st0), dev.put(buf)
    dev.small(kp, phase, dst, drec, nrec, **kw)
    st = dev.get_state(dst)
    assert _same(dev.get(drec, buf.shape), buf), "k_bcg_small wrote into its records"
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
@pytest.mark.parametrize("phase", [START, GAMMA, G, VERIFY], ids=["START", "GAMMA", "G", "VERIFY"])
def test_small_record_sums(hip, phase, kp):
    """small_sum_records at every record count around its two loops (4 and 16 loads in flight, the switch at 4 NR) and
    a ragged last trip, NaN behind the last record.  The sums are seen where the kernel copies or uses them exactly --
    bb after START, rr after G with sigma = I (every other term of sigma_c^T H sigma_c is an exact zero),
    true_relres after VERIFY with bb = 1 -- within (S); elsewhere through the identities of the phase with (S)
    added."""
    T, W = tri_of(kp), small_width(phase, kp)
    for nrec in _nrecords(W):
        rng = np.random.default_rng(1000 * phase + 10 * kp + 100003 * nrec)
        A, M, d = _gram(rng, kp, scaled=False)
        with _device(hip) as dev:
            if phase == START:
                buf, sums, allow = _records(rng, nrec, W, _tri(A))
                st = _run_small(dev, kp, START, _state(running=0), buf, nrec, nrhs=kp, tol=1e-8, maxit=100)
                assert not check_start(st, sums[:T], allow[:T], sums[T:], allow[T:], kp, kp, 1e-8, 100), nrec
            elif phase == GAMMA:
                buf, sums, allow = _records(rng, nrec, W, _tri(A))
                st0 = _loop_state(rng, kp)
                st = _run_small(dev, kp, GAMMA, st0, buf, nrec)
                assert not check_gamma(st0, st, sums, allow, kp), nrec
            elif phase == G:
                buf, sums, allow = _records(rng, nrec, W, _tri(A))
                st0 = _loop_state(rng, kp, sigma=_embed(np.eye(kp), True), thresh2=np.full(BS, -np.inf))
                st = _run_small(dev, kp, G, st0, buf, nrec)
                assert check_g(st0, st, sums[:T], sums[T:], allow[:T], allow[T:], kp) == "runs", nrec
                diag = [i * kp - i * (i - 1) // 2 for i in range(kp)]
                err = np.abs(_vec(st.rr)[:kp].astype(LD) - sums[T:][diag])
                assert (err <= allow[T:][diag]).all(), (nrec, (err / allow[T:][diag]).astype(np.float64))
            else:
                buf, sums, allow = _records(rng, nrec, W)
                buf[:nrec] = np.abs(buf[:nrec])
                sums = buf[:nrec].astype(LD).sum(axis=0)
                st0 = _loop_state(rng, kp, bb=np.ones(BS), tol=np.inf, running=0,
                                  status=[CONVERGED] * BS)
                st = _run_small(dev, kp, VERIFY, st0, buf, nrec)
                check_verify(st0, st, sums, kp, nrec)
                assert all(st.true_relres[c] > 0 for c in range(kp))


def _one_record(kp, Atri, bb=None):
    """one record of START (or of GAMMA where bb is None), NaN behind it"""
    row = np.asarray(Atri, np.float64) if bb is None else np.concatenate([Atri, bb])
    buf = np.full((1 + PAD, row.size), np.nan)
    buf[0] = row
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("kp,nrhs", [(2, 2), (4, 4), (8, 8), (4, 3), (8, 5), (8, 7)])
def test_start(hip, kp, nrhs):
    """START writes the whole state from one exact record: sigma = zeta = L^T with (C) and (F), zinv with (I), bb, rr,
    thresh2 = tol^2 bb to the bit, min_pivot, the counters, tol, true_relres = -1.  With nrhs < kp the record holds
    what a packed block gives (zero off-diagonal entries on the padding) and NaN where the rule must not look (the
    padding's diagonal and its b.b): the identity on the padding and beyond kp, CONVERGED, zero bb and thresh2 there.
    maxit = 0: MAXIT and running = 0, the factor all the same.  The incoming state is garbage with running = 0."""
    rng = np.random.default_rng(2000 + 10 * kp + nrhs)
    T = tri_of(kp)
    A, M, d = _gram(rng, kp)
    pad = np.arange(kp) >= nrhs
    A[pad, :] = 0.0
    A[:, pad] = 0.0
    A[pad, pad] = np.nan
    bbv = np.where(pad, np.nan, np.abs(_rand(rng, kp)))
    buf = _one_record(kp, _tri(A), bbv)
    none = np.zeros(T + kp, LD)
    for tol, maxit in ((1e-10, 500), (3e-7, 0)):
        with _device(hip) as dev:
            st = _run_small(dev, kp, START, _state(running=0, rank_bad=1, nrhs=1, iters=9), buf, 1,
                            nrhs=nrhs, tol=tol, maxit=maxit)
        assert not check_start(st, buf[0, :T].astype(LD), none[:T], buf[0, T:].astype(LD), none[T:], kp, nrhs, tol, maxit)
        assert _same(_vec(st.bb)[:nrhs], bbv[:nrhs])  # one record: a copy
        assert st.running == (1 if maxit else 0) and st.status[0] == (RUNNING if maxit else MAXIT)


@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
def test_start_rank_rule_at_its_floor(hip, kp):
    """The unit-diagonal Gram matrix given exactly (test_pivot_floor_inputs_in_exact_arithmetic): with c = 1 - 2^-32
    the last pivot is 4.7e-10, the block runs and min_pivot is 1 - c^2 within (S) of that one subtraction,
    2 eps (1 + c^2); with c = 1 - 2^-36 it is 2.9e-11: BREAKDOWN on every column, rank_bad, running = 0 and the
    identity in sigma, zeta and zinv.  The same for a zero diagonal entry (0 / 0) and for an infinite record."""
    T = tri_of(kp)
    none = np.zeros(T + kp, LD)

    def run(rec):
        buf = _one_record(kp, rec[:T], rec[T:])
        with _device(hip) as dev:
            return _run_small(dev, kp, START, _state(running=1), buf, 1, nrhs=kp, tol=1e-9, maxit=50), buf
    rec, c = _floor_case(kp, 32)
    st, buf = run(rec)
    assert not check_start(st, buf[0, :T].astype(LD), none, buf[0, T:].astype(LD), none, kp, kp, 1e-9, 50,
                           piv_allow=2 * EPS * (1 + float(c) ** 2))
    assert 4.6e-10 < st.min_pivot < 4.7e-10 and st.running == 1 and st.rank_bad == 0
    bad = [_floor_case(kp, 36)[0]]
    zero = rec.copy()
    zero[0] = 0.0
    inf = rec.copy()
    inf[1] = np.inf
    bad += [zero, inf]
    if kp > 2:  # a zero diagonal entry that is not the first pivot
        z2 = rec.copy()
        z2[T - 1] = 0.0
        bad.append(z2)
    for r in bad:
        st, buf = run(r)
        with np.errstate(all="ignore"):
            assert check_start(st, buf[0, :T].astype(LD), none, buf[0, T:].astype(LD), none, kp, kp, 1e-9, 50)
        assert st.status[:] == [BREAKDOWN] * kp + [CONVERGED] * (BS - kp)
        assert (st.rank_bad, st.running) == (1, 0) and not st.min_pivot > FLOOR
        for name in ("sigma", "zeta", "zinv"):
            assert _same(_mat(st, name), np.eye(BS)), name


@pytest.mark.gpu
@pytest.mark.parametrize("kp,nrhs", [(2, 2), (4, 4), (8, 8), (4, 3), (8, 5)])
def test_gamma(hip, kp, nrhs):
    """GAMMA from one exact record: xi against Gamma^-1 (F), symmetric to the bit, xs = xi sigma with the sigma in the
    state (S), nspmm + 1, nothing else.  An indefinite and a NaN Gamma: BREAKDOWN on the nrhs columns only, running =
    0, xi and xs keep their bytes, nspmm still counts."""
    rng = np.random.default_rng(3000 + 10 * kp + nrhs)
    A, M, d = _gram(rng, kp)
    pad = np.arange(kp) >= nrhs
    A[pad, :] = 0.0
    A[:, pad] = 0.0
    M = np.where(np.outer(pad, np.ones(kp, bool)) | np.outer(np.ones(kp, bool), pad), np.eye(kp), M)
    d = np.where(pad, 1.0, d)
    A[pad, pad] = np.nan  # the rule puts 1 there
    none = np.zeros(tri_of(kp), LD)
    st0 = _loop_state(rng, kp, nrhs)
    with _device(hip) as dev:
        buf = _one_record(kp, _tri(A))
        st = _run_small(dev, kp, GAMMA, st0, buf, 1)
        assert not check_gamma(st0, st, buf[0].astype(LD), none, kp, M, d)
        assert st.nspmm == st0.nspmm + 1 and st.running == 1
        indef = np.nan_to_num(A).copy()
        indef[0, 0] = -indef[0, 0]
        nan = np.nan_to_num(A).copy()
        nan[0, nrhs - 1] = nan[nrhs - 1, 0] = np.nan
        last = np.nan_to_num(A).copy()
        last[nrhs - 1, nrhs - 1] = 0.0  # a pivot that is zero, not negative
        for B in (indef, nan, last):
            buf = _one_record(kp, _tri(B))
            st = _run_small(dev, kp, GAMMA, st0, buf, 1)
            assert check_gamma(st0, st, buf[0].astype(LD), none, kp)
            assert st.status[:] == [BREAKDOWN] * nrhs + [CONVERGED] * (BS - nrhs)
            assert (st.running, st.nspmm) == (0, st0.nspmm + 1)
            assert _same(_mat(st, "xi"), _mat(st0, "xi")) and _same(_mat(st, "xs"), _mat(st0, "xs"))


@pytest.mark.gpu
@pytest.mark.parametrize("kp,nrhs", [(2, 2), (4, 4), (8, 8), (4, 3), (8, 7)])
def test_g(hip, kp, nrhs):
    """G from one exact record: rr_c = sigma_c^T H sigma_c with the OLD sigma (S), zeta = L^T (C)(F), zinv (I),
    sigma = zeta sigma (S), iters + 1, nothing else.  A G that is not positive: BREAKDOWN."""
    rng = np.random.default_rng(4000 + 10 * kp + nrhs)
    T = tri_of(kp)
    A, M, d = _gram(rng, kp)
    pad = np.arange(kp) >= nrhs
    both = np.outer(pad, np.ones(kp, bool)) | np.outer(np.ones(kp, bool), pad)
    A[both] = 0.0
    M = np.where(both, np.eye(kp), M)
    d = np.where(pad, 1.0, d)
    H = _rand(rng, kp, kp)
    H = np.triu(H) + np.triu(H, 1).T
    H[both] = 0.0
    A[pad, pad] = np.nan
    H[pad, pad] = np.nan
    sig = _upper(rng, kp)
    sig[both] = np.eye(kp)[both]
    none = np.zeros(T, LD)
    st0 = _loop_state(rng, kp, nrhs, sigma=_embed(sig, True), thresh2=np.full(BS, -np.inf))
    with _device(hip) as dev:
        buf = _one_record(kp, np.concatenate([_tri(A), _tri(H)]))
        st = _run_small(dev, kp, G, st0, buf, 1)
        assert check_g(st0, st, buf[0, :T].astype(LD), buf[0, T:].astype(LD), none, none, kp, M, d) == "runs"
        assert st.iters == st0.iters + 1 and st.running == 1 and st.status[:] == st0.status[:]
        assert not _same(_mat(st, "sigma", kp), _mat(st0, "sigma", kp))
        neg = np.nan_to_num(A).copy()
        neg[nrhs - 1, nrhs - 1] = -neg[nrhs - 1, nrhs - 1]
        nan = np.nan_to_num(A).copy()
        nan[0, 0] = np.nan
        for B in (neg, nan):
            buf = _one_record(kp, np.concatenate([_tri(B), _tri(H)]))
            st = _run_small(dev, kp, G, st0, buf, 1)
            assert check_g(st0, st, buf[0, :T].astype(LD), buf[0, T:].astype(LD), none, none, kp) == "bad"
            assert st.status[:] == [BREAKDOWN] * nrhs + [CONVERGED] * (BS - nrhs) and st.running == 0
            for name in ("sigma", "zeta", "zinv"):
                assert _same(_mat(st, name), _mat(st0, name)), name


@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
def test_g_stop_rules(hip, kp):
    """The stop test with exact operands: sigma = I, so rr_c = H_cc to the bit, H_cc and thresh2 powers of two.  All
    columns <= their threshold, one of them equal: CONVERGED.  One column above at iters + 1 == maxit: that one MAXIT,
    the others -- one of them at equality -- CONVERGED.  The same column above with iterations left: the block runs
    on.  On either stop sigma, zeta and zinv keep their bytes and rr is written."""
    rng = np.random.default_rng(5000 + kp)
    T = tri_of(kp)
    A, M, d = _gram(rng, kp, scaled=False)
    hd = 2.0 ** -np.arange(20, 20 + kp)
    thr = np.full(BS, np.nan)
    thr[:kp] = 2 * hd
    thr[0] = hd[0]  # equality counts
    H = np.diag(hd)

    def run(dev, thresh2, iters, maxit, Hm=H):
        st0 = _loop_state(rng, kp, sigma=_embed(np.eye(kp), True), thresh2=thresh2, iters=iters, maxit=maxit)
        buf = _one_record(kp, np.concatenate([_tri(A), _tri(Hm)]))
        st = _run_small(dev, kp, G, st0, buf, 1)
        out = check_g(st0, st, buf[0, :T].astype(LD), buf[0, T:].astype(LD), np.zeros(T, LD), np.zeros(T, LD), kp)
        assert np.array_equal(_vec(st.rr)[:kp], np.diag(Hm), equal_nan=True) and st.iters == iters + 1
        return st0, st, out
    with _device(hip) as dev:
        st0, st, out = run(dev, thr, 5, 1000)
        assert out == "stop" and st.status[:kp] == [CONVERGED] * kp and st.running == 0
        above = thr.copy()
        above[kp - 1] = hd[kp - 1] / 2
        st0, st, out = run(dev, above, 5, 6)
        assert out == "stop" and st.status[:kp] == [CONVERGED] * (kp - 1) + [MAXIT] and st.running == 0
        st0, st, out = run(dev, above, 5, 7)
        assert out == "runs" and st.status[:kp] == [RUNNING] * kp and st.running == 1
        # a NaN norm is not <=: it never converges, and at maxit it is MAXIT
        Hn = H.copy()
        Hn[kp - 1, kp - 1] = np.nan  # (the last column's: no other column's chain meets it)
        st0, st, out = run(dev, thr, 5, 6, Hn)
        assert out == "stop" and st.status[:kp] == [CONVERGED] * (kp - 1) + [MAXIT]
        st0, st, out = run(dev, thr, 5, 7, Hn)
        assert out == "runs" and st.running == 1


@pytest.mark.gpu
@pytest.mark.parametrize("kp,nrhs", [(2, 2), (4, 3), (8, 8)])
def test_verify(hip, kp, nrhs):
    """VERIFY from three records: true_relres = sqrt(sum / bb); a CONVERGED column becomes MAXIT where it exceeds tol
    and where the sum is NaN; a column with bb = 0 and every other status are untouched, and so is the padding."""
    rng = np.random.default_rng(6000 + 10 * kp + nrhs)
    tol = 1e-6
    bb = np.abs(_rand(rng, BS))
    want = np.array([0.5 * tol, 2 * tol] * 4)[:kp]  # alternately inside and outside the tolerance
    buf, _, _ = _records(rng, 3, kp)
    buf[:3] = np.abs(buf[:3])
    buf[:3] *= (want ** 2 * bb[:kp] / buf[:3].sum(axis=0))[None, :]
    for case in ("converged", "other", "nan", "bb0"):
        b2, status = buf.copy(), [CONVERGED] * nrhs
        bbc = bb.copy()
        if case == "other":
            status = ([MAXIT, BREAKDOWN, RUNNING] * 3)[:nrhs]
        if case == "nan":
            b2[1, 0] = np.nan
        if case == "bb0":
            bbc[nrhs - 1] = 0.0
        st0 = _loop_state(rng, kp, nrhs, bb=bbc, tol=tol, running=0, status=status + [CONVERGED] * (BS - nrhs))
        with _device(hip) as dev:
            st = _run_small(dev, kp, VERIFY, st0, b2, 3)
        with np.errstate(invalid="ignore"):
            sums = b2[:3].astype(LD).sum(axis=0)
        check_verify(st0, st, sums, kp, 3)
        if case == "converged":
            assert st.status[:nrhs] == ([CONVERGED, MAXIT] * 4)[:nrhs]
        if case == "other":
            assert st.status[:nrhs] == status
        if case == "nan":
            assert st.status[0] == MAXIT and np.isnan(st.true_relres[0])
        if case == "bb0":
            assert st.true_relres[nrhs - 1] == -1.0 and st.status[nrhs - 1] == CONVERGED


# ------------------------------------------------------------------ B. the streaming passes
def _block(rng, n, kp):
    """n rows of kp values and PAD rows of slack behind them"""
    a = np.full((n + PAD, kp), SLACK)
    a[:n] = _rand(rng, n, kp)
    return a


def _pass_state(rng, kp, **kw):
    """the small matrices a pass reads: xi, xs full, zeta, zinv upper with different values in mirrored positions (the
    lower triangle holds NaN, so a transposed index shows), sigma -- which no pass reads -- NaN"""
    return _loop_state(rng, kp, sigma=np.full(BS * BS, np.nan), **kw)


def _dvec(rng, n, mode):
    """-> (the array or None, the constant, D^-1 as longdouble per row)"""
    if mode == "array":
        a = _rand(rng, n)
        return a, float("nan"), a.astype(LD)
    dc = -0.37
    return None, dc, np.full(n, dc, LD)


def _by_wg(v, g):
    """the sums of a per-row quantity over the rows each of g workgroups owns under the grid stride"""
    per = g * WG
    trips = -(-v.size // per)
    buf = np.zeros(trips * per, LD)
    buf[:v.size] = v
    return buf.reshape(trips, g, WG).sum(axis=(0, 2))


def _check_pass_records(rec, terms, n, g, what):
    """every record of a streaming pass against the longdouble sums of its own rows; terms: one per-row vector per
    component, in the record's order (an iterator: a wide block's 72 vectors are not held together).  The buffer behind
    record g is untouched (NaN)."""
    L = _ceil(n, g * WG) + 6 + 2
    assert np.isnan(rec[g:]).all(), what + ": wrote behind its records"
    k = -1
    for k, t in enumerate(terms):
        ref, mag = _by_wg(t, g), _by_wg(np.abs(t), g)
        err = np.abs(rec[:g, k].astype(LD) - ref)
        allow = 2 * L * EPS * mag
        assert (err <= allow).all(), "%s: component %d of record %s, err/allowed %.3g" % (
            what, k, np.flatnonzero(~(err <= allow))[:4], float((err / np.maximum(allow, LD(1e-300))).max()))
    assert k + 1 == rec.shape[1], what + ": the record's width"


def _gram_terms(a, z, d=None):
    """per-row terms of the upper triangle of A^T (D) Z, row by row"""
    kp = a.shape[1]
    for r in range(kp):
        for c in range(r, kp):
            yield (a[:, r] * z[:, c]) if d is None else (d * a[:, r] * z[:, c])


def _check_rows(got, ref, mag, L, what):
    allow = 2 * L * EPS * mag
    err = np.abs(got.astype(LD) - ref)
    ok = err <= allow
    assert ok.all(), "%s wrong at %s, err/allowed %.3g" % (
        what, np.argwhere(~ok)[:4].tolist(), float((err / np.maximum(allow, LD(1e-300))).max()))


def _upper_of(st, name, kp):
    return np.nan_to_num(np.triu(_mat(st, name, kp))).astype(LD)


def check_init(kp, n, b, dld, rec, nrec):
    assert nrec == pass_grid(n)
    bl = b[:n].astype(LD)
    terms = itertools.chain(_gram_terms(bl, bl, dld), (bl[:, c] * bl[:, c] for c in range(kp)))
    _check_pass_records(rec, terms, n, nrec, "init")


def check_start_vectors(kp, n, st, b, dld, w, p, x, z=None, what="start"):
    """W = B zinv, P = D^-1 W (one rounding on the W the device stored) or Z zinv, X = 0; the slack is the caller's"""
    zinv = _upper_of(st, "zinv", kp)
    bl = b[:n].astype(LD)
    _check_rows(w[:n], bl @ zinv, np.abs(bl) @ np.abs(zinv), kp, what + ": W")
    if z is None:
        pref = dld[:, None] * w[:n].astype(LD)
        _check_rows(p[:n], pref, np.abs(pref), 1, what + ": P")
    else:
        zl = z[:n].astype(LD)
        _check_rows(p[:n], zl @ zinv, np.abs(zl) @ np.abs(zinv), kp, what + ": P")
    assert not _bits(x[:n]).any(), what + ": X is not +0"
    for name, v in (("W", w), ("P", p), ("X", x)):
        assert (v[n:] == SLACK).all(), "%s: wrote behind row n of %s" % (what, name)


def check_pass_a(kp, n, st, w0, q, p, x0, w1, x1, what="pass A"):
    """X += P xs and W~ = W - Q xi against the values the operands held before"""
    xs, xi = _mat(st, "xs", kp).astype(LD), _mat(st, "xi", kp).astype(LD)
    pl, ql = p[:n].astype(LD), q[:n].astype(LD)
    _check_rows(x1[:n], x0[:n].astype(LD) + pl @ xs, np.abs(x0[:n]).astype(LD) + np.abs(pl) @ np.abs(xs), kp, what + ": X")
    _check_rows(w1[:n], w0[:n].astype(LD) - ql @ xi, np.abs(w0[:n]).astype(LD) + np.abs(ql) @ np.abs(xi), kp, what + ": W~")
    assert (w1[n:] == SLACK).all() and (x1[n:] == SLACK).all(), what + ": wrote behind row n"


def check_pass_b(kp, n, st, wt, p0, w1, p1, dld=None, z=None, what="pass B"):
    """W = W~ zinv ; P = D^-1 W (the W the device stored) + P zeta^T, or Z~ zinv + P zeta^T"""
    zinv, zeta = _upper_of(st, "zinv", kp), _upper_of(st, "zeta", kp)
    wl, pl = wt[:n].astype(LD), p0[:n].astype(LD)
    _check_rows(w1[:n], wl @ zinv, np.abs(wl) @ np.abs(zinv), kp, what + ": W")
    if z is None:
        first = dld[:, None] * w1[:n].astype(LD)
        fmag = np.abs(first)
    else:
        zl = z[:n].astype(LD)
        first, fmag = zl @ zinv, np.abs(zl) @ np.abs(zinv)
    _check_rows(p1[:n], first + pl @ zeta.T, fmag + np.abs(pl) @ np.abs(zeta).T, kp + 1, what + ": P")
    assert (w1[n:] == SLACK).all() and (p1[n:] == SLACK).all(), what + ": wrote behind row n"


def _rec_buf(dev, g, W):
    buf = np.full((g + PAD, W), np.nan)
    return dev.put(buf), buf.shape


def _passes_case(hip, kernel, kp, n):
    T = tri_of(kp)
    for mode in ("array", "constant"):
        if mode == "constant" and kernel in ("m_pass_a", "m_start", "m_pass_b"):
            continue  # (no diagonal among their arguments)
        rng = np.random.default_rng(7000 + 13 * n + kp + (mode == "array"))
        dinv, dc, dld = _dvec(rng, n, mode)
        st0 = _pass_state(rng, kp)
        g = pass_grid(n)
        assert 1 <= g <= PASS_CAP and n < 2 ** 31 // kp
        with _device(hip) as dev:
            dd = dev.put(dinv) if dinv is not None else None
            dst = dev.put_state(st0)
            b, w, q, p, x, z = (_block(rng, n, kp) for _ in range(6))
            shape = b.shape
            db, dw, dq, dp, dx, dz = (dev.put(v) for v in (b, w, q, p, x, z))
            if kernel == "init":
                drec, rs = _rec_buf(dev, g, T + kp)
                nrec = dev.init(kp, n, db, dd, dc, drec)
                check_init(kp, n, b, dld, dev.get(drec, rs), nrec)
                assert _same(dev.get(db, shape), b)
            elif kernel == "start":
                dev.start(kp, n, db, dd, dc, dw, dp, dx, dst)
                check_start_vectors(kp, n, st0, b, dld, dev.get(dw, shape), dev.get(dp, shape), dev.get(dx, shape))
                assert _same(dev.get(db, shape), b)
            elif kernel == "pass_a":
                drec, rs = _rec_buf(dev, g, 2 * T)
                nrec = dev.pass_a(kp, n, dw, dq, dp, dx, dd, dc, dst, drec)
                w1, x1 = dev.get(dw, shape), dev.get(dx, shape)
                check_pass_a(kp, n, st0, w, q, p, x, w1, x1)
                assert nrec == g
                wl = w1[:n].astype(LD)
                _check_pass_records(dev.get(drec, rs), itertools.chain(_gram_terms(wl, wl, dld), _gram_terms(wl, wl)),
                                    n, g, "pass A")
                assert _same(dev.get(dq, shape), q) and _same(dev.get(dp, shape), p)
            elif kernel == "pass_b":
                dev.pass_b(kp, n, dw, dp, dd, dc, dst)
                check_pass_b(kp, n, st0, w, p, dev.get(dw, shape), dev.get(dp, shape), dld=dld)
            elif kernel == "m_pass_a":
                dev.m_pass_a(kp, n, dw, dq, dp, dx, dst)
                check_pass_a(kp, n, st0, w, q, p, x, dev.get(dw, shape), dev.get(dx, shape), "m pass A")
                assert _same(dev.get(dq, shape), q) and _same(dev.get(dp, shape), p)
            elif kernel == "m_gram":
                wl, zl = w[:n].astype(LD), z[:n].astype(LD)
                if mode == "array":  # the start form: A^T Z, then a_c . a_c
                    drec, rs = _rec_buf(dev, g, T + kp)
                    nrec = dev.m_gram(kp, 1, n, dw, dz, drec, None)
                    terms = itertools.chain(_gram_terms(wl, zl), (wl[:, c] * wl[:, c] for c in range(kp)))
                else:                # the loop form: A^T Z, then A^T A
                    drec, rs = _rec_buf(dev, g, 2 * T)
                    nrec = dev.m_gram(kp, 0, n, dw, dz, drec, dst)
                    terms = itertools.chain(_gram_terms(wl, zl), _gram_terms(wl, wl))
                assert nrec == g
                _check_pass_records(dev.get(drec, rs), terms, n, g, "m gram")
                assert _same(dev.get(dw, shape), w) and _same(dev.get(dz, shape), z)
            elif kernel == "m_start":
                dev.m_start(kp, n, db, dz, dw, dp, dx, dst)
                check_start_vectors(kp, n, st0, b, None, dev.get(dw, shape), dev.get(dp, shape), dev.get(dx, shape),
                                    z=z, what="m start")
                assert _same(dev.get(db, shape), b) and _same(dev.get(dz, shape), z)
            elif kernel == "m_pass_b":
                dev.m_pass_b(kp, n, dw, dz, dp, dst)
                check_pass_b(kp, n, st0, w, p, dev.get(dw, shape), dev.get(dp, shape), z=z, what="m pass B")
                assert _same(dev.get(dz, shape), z)
            assert bytes(dev.get_state(dst)) == bytes(st0), kernel + " wrote the state"


PASSES = ["init", "start", "pass_a", "pass_b", "m_pass_a", "m_gram", "m_start", "m_pass_b"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kp", KPS)
@pytest.mark.parametrize("kernel", PASSES)
def test_streaming_pass(hip, kernel, kp, n):
    """Each streaming launcher alone: one row, two, one workgroup short of full, full and one over, and the two sizes
    between which pass_grid changes its rule (65536: one row per lane; 65537: the grid stays at 256 and a lane takes a
    second trip).  The diagonal as an array and as NULL with the constant.  Vectors element by element (S), in-place
    operands against what they held, the slack behind row n, nrecords, and every record against the rows its workgroup
    owns."""
    _passes_case(hip, kernel, kp, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kp", [2, 8])
@pytest.mark.parametrize("kernel", PASSES)
def test_streaming_pass_beyond_the_grid_cap(hip, kernel, kp):
    """512 workgroups and a ragged fifth trip"""
    _passes_case(hip, kernel, kp, N_CAPPED)


# ------------------------------------------------------------------ C. the row kernels with a dealt triangle
def _row_matrix(rng, n, L):
    """an unsymmetric CSR matrix whose rows have 3 L + 1, 0, 1, L - 1, L and L + 1 entries in turn (columns drawn with
    repetition: the kernels take entries as they are stored)"""
    lens = np.array([3 * L + 1, 0, 1, L - 1, L, L + 1])[np.arange(n) % 6]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(offs[-1])
    cols = rng.integers(0, n, size=max(nnz, 1)).astype(np.int32)
    vals = _rand(rng, max(nnz, 1))
    assert offs.size == n + 1 and cols.min() >= 0 and cols.max() < n
    return offs, cols, vals


def _csr_product(csr, n, X):
    """(S X, |S| |X|) in longdouble, and per row the chain ceil(entries / lanes) is the caller's"""
    offs, cols, vals = csr
    nnz = int(offs[n])
    rows = np.repeat(np.arange(n), np.diff(offs[:n + 1]))
    prod = vals[:nnz, None].astype(LD) * X[cols[:nnz]].astype(LD)
    Y, mag = np.zeros((n, X.shape[1]), LD), np.zeros((n, X.shape[1]), LD)
    np.add.at(Y, rows, prod)
    np.add.at(mag, rows, np.abs(prod))
    return Y, mag


def check_row_product(csr, n, L, X, Y, what):
    """Y = S X by the row rule: a lane's ceil(entries / L) fused steps and the log2 L steps of the butterfly"""
    ref, mag = _csr_product(csr, n, X[:n])
    chain = -(-np.diff(csr[0][:n + 1]) // L) + int(math.log2(L))
    allow = 2 * chain[:, None] * EPS * mag
    err = np.abs(Y[:n].astype(LD) - ref)
    assert (err <= allow).all(), "%s wrong at %s" % (what, np.argwhere(~(err <= allow))[:4].tolist())
    assert (Y[n:] == SLACK).all(), what + ": wrote behind row n"


def check_row_records(rec, g, n, L, tris, what):
    """the longdouble sum of a row kernel's records against the upper triangles tris = [(U, V), ...] of U^T V; NaN
    prefill: a workgroup without rows must have stored its zeros.  The chain: a lane's trips, the butterfly of the
    dealt triangle over the 64 / L lanes that hold the same entries, the four waves."""
    chain = rows_per_wg(n, g, L) // (WG // L) + int(math.log2(64 // L)) + 2
    assert np.isfinite(rec[:g]).all(), what + ": a record was not stored"
    assert np.isnan(rec[g:]).all(), what + ": wrote behind its records"
    got = rec[:g].astype(LD).sum(axis=0)
    k = 0
    for U, V in tris:
        for t in _gram_terms(U[:n].astype(LD), V[:n].astype(LD)):
            allow = 2 * chain * EPS * np.abs(t).sum()
            assert abs(got[k] - t.sum()) <= allow, "%s: component %d, err/allowed %.3g" % (
                what, k, float(abs(got[k] - t.sum()) / allow))
            k += 1
    assert k == rec.shape[1]


def _row_case(hip, kernel, kp, L, n):
    rng = np.random.default_rng(8000 + 1000 * L + 10 * kp + n)
    T = tri_of(kp)
    csr = _row_matrix(rng, n, L)
    g = spmm_grid(n, L)
    W = T if kernel == "spmm" else 2 * T
    st0 = _pass_state(rng, kp)
    x, wt = _block(rng, n, kp), _block(rng, n, kp)
    y = np.full((n + PAD, kp), SLACK)
    assert 8 <= g <= MAX_PARTIALS and g % NXCD == 0
    with _device(hip) as dev:
        assert int(dev.k.lsb_k_spmm_grid(n, L)) == g
        dcsr = (dev.put(csr[0], np.int32), dev.put(csr[1], np.int32), dev.put(csr[2]))
        dx, dwt, dy, dy2, dst = dev.put(x), dev.put(wt), dev.put(y), dev.put(y), dev.put_state(st0)
        drec, rs = _rec_buf(dev, g, W)
        dpart = dev.put(np.full((g + PAD, kp), np.nan))
        assert dev.spmm_csr(kp, n, dcsr, L, dx, dy2, dpart) == g
        if kernel == "spmm":
            nrec = dev.spmm(kp, n, dcsr, L, dx, dy, drec, dst)
        else:
            nrec = dev.gt_gram(kp, n, dcsr, L, dx, dwt, dy, drec, dst)
        assert nrec == g
        y1, rec = dev.get(dy, y.shape), dev.get(drec, rs)
        assert _same(y1, dev.get(dy2, y.shape)), "not the bits of lsb_k_spmm_csr"
        assert _same(dev.get(dx, x.shape), x) and _same(dev.get(dwt, wt.shape), wt)
        assert bytes(dev.get_state(dst)) == bytes(st0)
    check_row_product(csr, n, L, x, y1, kernel)
    check_row_records(rec, g, n, L, [(x, y1)] if kernel == "spmm" else [(wt, y1), (wt, wt)], kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
@pytest.mark.parametrize("L", LANES)
@pytest.mark.parametrize("kernel", ["spmm", "gt_gram"])
def test_row_kernel(hip, kernel, L, kp):
    """k_bcg_spmm and k_bcgm_gt_gram at every lane count and width on one row and on 33: the product bit for bit that
    of lsb_k_spmm_csr and within (S) of longdouble, the summed records against P^T Q (or W~^T Z and W~^T W~) -- the
    operator is unsymmetric, so a transposed entry shows --, nrecords == lsb_k_spmm_grid."""
    for n in (1, 33):
        _row_case(hip, kernel, kp, L, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["spmm", "gt_gram"])
@pytest.mark.parametrize("L,kp", [(64, 2), (64, 4), (64, 8), (2, 8)])
def test_row_kernel_two_trips(hip, kernel, L, kp):
    """n just above 2048 * 256 / L: the grid is at its cap and every workgroup takes a second trip over its rows"""
    _row_case(hip, kernel, kp, L, MAX_PARTIALS * (WG // L) + (5 if L == 64 else 3))


# ------------------------------------------------------------------ D. the gate
@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
def test_gate(hip, kp):
    """running = 0: the SpMM, gt_gram, both pass A, both pass B, the loop form of m_gram, GAMMA and G write nothing --
    state, vectors and records keep their bytes.  START, both start kernels, init and m_gram's start form are not gated
    by design and do write."""
    n, L = 1025, 8
    rng = np.random.default_rng(9000 + kp)
    T = tri_of(kp)
    csr = _row_matrix(rng, n, L)
    g = max(spmm_grid(n, L), pass_grid(n))
    A, M, d = _gram(rng, kp)
    st0 = _loop_state(rng, kp, running=0, sigma=_embed(_upper(rng, kp), True))
    vecs = [_block(rng, n, kp) for _ in range(6)]
    rec = np.full((g + PAD, 2 * T), np.nan)
    rec[0] = np.concatenate([_tri(A), _tri(A)])
    with _device(hip) as dev:
        dcsr = (dev.put(csr[0], np.int32), dev.put(csr[1], np.int32), dev.put(csr[2]))
        db, dw, dq, dp, dx, dz = (dev.put(v) for v in vecs)
        dd, dst, drec = dev.put(_rand(rng, n)), dev.put_state(st0), dev.put(rec)

        def unchanged(i):
            for k, (dv, v) in enumerate(zip((db, dw, dq, dp, dx, dz), vecs)):
                assert _same(dev.get(dv, v.shape), v), (i, k)
            assert _same(dev.get(drec, rec.shape), rec), i
            assert bytes(dev.get_state(dst)) == bytes(st0), i
        launches = [
            lambda: dev.spmm(kp, n, dcsr, L, dp, dq, drec, dst),
            lambda: dev.gt_gram(kp, n, dcsr, L, dq, dw, dz, drec, dst),
            lambda: dev.pass_a(kp, n, dw, dq, dp, dx, dd, 0.5, dst, drec),
            lambda: dev.pass_a(kp, n, dw, dq, dp, dx, None, 0.5, dst, drec),
            lambda: dev.m_pass_a(kp, n, dw, dq, dp, dx, dst),
            lambda: dev.pass_b(kp, n, dw, dp, dd, 0.5, dst),
            lambda: dev.m_pass_b(kp, n, dw, dz, dp, dst),
            lambda: dev.m_gram(kp, 0, n, dw, dz, drec, dst),
            lambda: dev.small(kp, GAMMA, dst, drec, 1),
            lambda: dev.small(kp, G, dst, drec, 1),
        ]
        for i, launch in enumerate(launches):
            launch()
            unchanged(i)
        # not gated: each writes with the same stopped state on the device
        dev.start(kp, n, db, dd, 0.5, dw, dp, dx, dst)
        assert not dev.get(dx, vecs[4].shape)[:n].any() and not _same(dev.get(dw, vecs[1].shape), vecs[1])
        dev.write(dx, vecs[4])
        dev.m_start(kp, n, db, dz, dw, dp, dx, dst)
        assert not dev.get(dx, vecs[4].shape)[:n].any()
        assert dev.init(kp, n, db, dd, 0.5, drec) == pass_grid(n)
        assert np.isfinite(dev.get(drec, rec.shape).ravel()[:pass_grid(n) * (T + kp)]).all()
        dev.write(drec, rec)
        assert dev.m_gram(kp, 1, n, dw, dz, drec, dst) == pass_grid(n)
        assert np.isfinite(dev.get(drec, rec.shape).ravel()[:pass_grid(n) * (T + kp)]).all()
        assert bytes(dev.get_state(dst)) == bytes(st0)
        dev.write(drec, rec)
        dev.small(kp, START, dst, drec, 1, nrhs=kp, tol=1e-8, maxit=10)
        st = dev.get_state(dst)
        assert (st.running, st.iters, st.maxit, st.nspmm) == (1, 0, 10, 0)


# ------------------------------------------------------------------ E. one iteration in driver order
def _invariants(S, B, dinv, W, sigma, X):
    """(max |W^T D^-1 W - I|, max over the columns of ||W sigma_c - (b_c - S x_c)|| / ||b_c||) in longdouble"""
    Wl = W.astype(LD)
    orth = np.abs(Wl.T @ (LD(dinv) * Wl) - np.eye(W.shape[1])).max()
    SX, _ = _csr_product((S.indptr, S.indices, S.data), S.shape[0], X)
    R = B.astype(LD) - SX
    dif = Wl @ np.triu(sigma).astype(LD) - R
    res = (np.sqrt((dif * dif).sum(axis=0)) / np.sqrt((B.astype(LD) ** 2).sum(axis=0))).max()
    return float(orth), float(res)


def _driver_order(hip, kp, m_form):
    """init / START / start and three iterations, launcher by launcher; after every launch the restatement is applied to
    what the device held before it.  -> (X after each iteration, the invariants after each iteration)"""
    from test_block_cg import LAP, columns8
    from test_mrhs import _lap2d
    S = _lap2d(*LAP).tocsr()
    n, L, dc, T = S.shape[0], 4, 0.25, tri_of(kp)
    assert (S.diagonal() == 4.0).all()
    B = columns8(S)[:, :kp]
    csr = (S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))
    dld = np.full(n, dc, LD)
    shape = (n + PAD, kp)
    b = np.full(shape, SLACK)
    b[:n] = B
    gs, gp = spmm_grid(n, L), pass_grid(n)
    none = np.zeros(T, LD)
    out_x, out_inv = [], []
    with _device(hip) as dev:
        dcsr = (dev.put(csr[0], np.int32), dev.put(csr[1], np.int32), dev.put(csr[2]))
        db = dev.put(b)
        dw, dp, dq, dx, dz = (dev.put(np.full(shape, SLACK)) for _ in range(5))
        dst = dev.put_state(_state(running=0))
        drs, rss = _rec_buf(dev, gs, T)
        drp, rsp = _rec_buf(dev, gp, 2 * T)
        nan_pass = np.full(rsp, np.nan)

        def put_z(src):  # the "operator": Z = D^-1 (.) formed on the host, exact for D^-1 = 1/4
            v = dev.get(src, shape)
            v[:n] *= dc
            dev.write(dz, v)
            return v
        # the start
        if m_form:
            z = put_z(db)
            nrec = dev.m_gram(kp, 1, n, db, dz, drp, dst)
            bl, zl = b[:n].astype(LD), z[:n].astype(LD)
            rec = dev.get(drp, rsp).reshape(-1)[:(gp + PAD) * (T + kp)].reshape(gp + PAD, T + kp)
            assert nrec == gp
            _check_pass_records(rec[:gp + 1], list(_gram_terms(bl, zl)) + [bl[:, c] * bl[:, c] for c in range(kp)],
                                n, gp, "m gram, start")
        else:
            nrec = dev.init(kp, n, db, None, dc, drp)
            rec = dev.get(drp, rsp).reshape(-1)[:(gp + PAD) * (T + kp)].reshape(gp + PAD, T + kp)
            check_init(kp, n, b, dld, rec[:gp + 1], nrec)
        sums = rec[:gp].astype(LD).sum(axis=0)
        dev.small(kp, START, dst, drp, nrec, nrhs=kp, tol=1e-10, maxit=1000)
        st = dev.get_state(dst)
        allow = 2 * sum_chain(nrec, T + kp) * EPS * np.abs(rec[:gp]).astype(LD).sum(axis=0)
        assert not check_start(st, sums[:T], allow[:T], sums[T:], allow[T:], kp, kp, 1e-10, 1000)
        if m_form:
            dev.m_start(kp, n, db, dz, dw, dp, dx, dst)
        else:
            dev.start(kp, n, db, None, dc, dw, dp, dx, dst)
        w, p, x = dev.get(dw, shape), dev.get(dp, shape), dev.get(dx, shape)
        check_start_vectors(kp, n, st, b, dld, w, p, x, z=z if m_form else None)
        for it in range(3):
            # Q = S P and the records of P^T Q
            assert dev.spmm(kp, n, dcsr, L, dp, dq, drs, dst) == gs
            q, rec = dev.get(dq, shape), dev.get(drs, rss)
            check_row_product(csr, n, L, p, q, "spmm")
            check_row_records(rec, gs, n, L, [(p, q)], "spmm")
            assert _same(dev.get(dp, shape), p)
            # GAMMA
            st0 = st
            dev.small(kp, GAMMA, dst, drs, gs)
            st = dev.get_state(dst)
            allow = 2 * sum_chain(gs, T) * EPS * np.abs(rec[:gs]).astype(LD).sum(axis=0)
            assert not check_gamma(st0, st, rec[:gs].astype(LD).sum(axis=0), allow, kp)
            # pass A
            dev.write(drp, nan_pass)
            if m_form:
                dev.m_pass_a(kp, n, dw, dq, dp, dx, dst)
            else:
                assert dev.pass_a(kp, n, dw, dq, dp, dx, None, dc, dst, drp) == gp
            w1, x1 = dev.get(dw, shape), dev.get(dx, shape)
            check_pass_a(kp, n, st, w, q, p, x, w1, x1)
            x_allow = 2 * kp * EPS * (np.abs(x[:n]).astype(LD) + np.abs(p[:n]).astype(LD) @ np.abs(_mat(st, "xs", kp)).astype(LD))
            wl = w1[:n].astype(LD)
            if m_form:
                z = put_z(dw)
                assert dev.m_gram(kp, 0, n, dw, dz, drp, dst) == gp
                terms = list(_gram_terms(wl, z[:n].astype(LD))) + list(_gram_terms(wl, wl))
            else:
                terms = list(_gram_terms(wl, wl, dld)) + list(_gram_terms(wl, wl))
            rec = dev.get(drp, rsp)
            _check_pass_records(rec, terms, n, gp, "the records of G and H")
            w, x = w1, x1
            # G
            st0 = st
            dev.small(kp, G, dst, drp, gp)
            st = dev.get_state(dst)
            sums = rec[:gp].astype(LD).sum(axis=0)
            allow = 2 * sum_chain(gp, 2 * T) * EPS * np.abs(rec[:gp]).astype(LD).sum(axis=0)
            assert check_g(st0, st, sums[:T], sums[T:], allow[:T], allow[T:], kp) == "runs"
            # pass B
            if m_form:
                dev.m_pass_b(kp, n, dw, dz, dp, dst)
            else:
                dev.pass_b(kp, n, dw, dp, None, dc, dst)
            w1, p1 = dev.get(dw, shape), dev.get(dp, shape)
            check_pass_b(kp, n, st, w, p, w1, p1, dld=dld, z=z if m_form else None)
            w, p = w1, p1
            assert _same(dev.get(dx, shape), x) and _same(dev.get(db, shape), b)
            assert (st.iters, st.nspmm, st.running) == (it + 1, it + 1, 1)
            out_x.append((x[:n].copy(), x_allow))
            out_inv.append(_invariants(S, B, dc, w[:n], _mat(st, "sigma", kp), x[:n]))
    return out_x, out_inv


@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
def test_three_iterations_in_driver_order(hip, kp):
    """The 40 x 30 Laplacian under its diagonal (D^-1 = 1/4, passed as the constant; no operator preconditioner),
    columns8: init, START, start, then three times SpMM, GAMMA, pass A, G, pass B, each launch judged alone.  After
    each iteration the two identities no end-to-end test can see, W^T D^-1 W = I and W sigma = B - S X column by column
    (relative to ||b_c||), may be off by 8 times what the plain-float64 block_pcg is off at the same step on the same
    input (the summation orders differ).

    Measured on an MI355X, block_pcg / the kernels, over iterations 1 .. 3 and the three widths: W^T D^-1 W - I
    3.5e-16 .. 9.2e-15 / 1.4e-16 .. 6.9e-16 (the kernels' ratio to block_pcg at most 0.51); W sigma - (B - S X)
    3.4e-15 .. 9.2e-15 / 3.5e-15 .. 1.7e-14 (at most 1.85, at 8 columns in the third iteration)."""
    from test_block_cg import LAP, block_pcg, columns8
    from test_mrhs import _lap2d
    S = _lap2d(*LAP).tocsr()
    B = columns8(S)[:, :kp]
    trace = []
    block_pcg(S, B, 1e-10, maxit=4, trace=trace)
    _, inv = _driver_order(hip, kp, False)
    for it in range(3):
        t = trace[it + 1]
        ref = _invariants(S, B, 0.25, t["W"], t["sigma"], t["X"])
        print("kp %d iteration %d: W^T D^-1 W - I  block_pcg %.3g kernels %.3g ; W sigma - (B - S X)  block_pcg %.3g "
              "kernels %.3g" % (kp, it + 1, ref[0], inv[it][0], ref[1], inv[it][1]))
        assert inv[it][0] <= 8 * ref[0] and inv[it][1] <= 8 * ref[1]


@pytest.mark.gpu
@pytest.mark.parametrize("kp", KPS)
def test_three_iterations_through_the_m_kernels(hip, kp):
    """The same sequence through k_bcgm_gram (start and loop form), k_bcgm_start, k_bcgm_pass_a and k_bcgm_pass_b with
    Z = D^-1 W formed on the host as the "operator".  D^-1 = 1/4 scales exactly, so every operand of the two runs
    agrees to the bit and X may differ by the rounding of its own update alone: the allowance (S) of pass A's X,
    summed over the iterations."""
    xd, _ = _driver_order(hip, kp, False)
    xm, _ = _driver_order(hip, kp, True)
    allow = 0
    for it in range(3):
        x, x_allow = xd[it]
        allow = allow + x_allow
        err = np.abs(xm[it][0].astype(LD) - x.astype(LD))
        assert (err <= allow).all(), "iteration %d: X differs at %s" % (it + 1, np.argwhere(~(err <= allow))[:4].tolist())
