"""Thin Python handles over the C-ABI (include/lsbench.h, include/lsbench_hip.h).

Names follow the reference's C API (lsbench_matrix_read, lsbench_bench, ...;
reference: src/lsbench.h:32-40) so that tests read like a driver program.
Nothing is computed here: every method is one call into liblsbench_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _ptr(a):
    """Device or host address of a torch tensor / numpy array / int."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)


class Matrix:
    """Owner of a `struct csr *` allocated by the library."""

    def __init__(self, handle):
        if not handle:
            raise L.LsbenchHipError("NULL struct csr")
        self._h = handle

    @classmethod
    def from_arrays(cls, offs, cols, vals, base=0):
        """Wrap numpy arrays as a struct csr (arrays are kept alive by self)."""
        self = cls.__new__(cls)
        self._offs = np.ascontiguousarray(offs, dtype=np.uint32)
        self._cols = np.ascontiguousarray(cols, dtype=np.uint32)
        self._vals = np.ascontiguousarray(vals, dtype=np.float64)
        s = L.CsrStruct(len(self._offs) - 1, base,
                        self._offs.ctypes.data_as(C.POINTER(C.c_uint)),
                        self._cols.ctypes.data_as(C.POINTER(C.c_uint)),
                        self._vals.ctypes.data_as(C.POINTER(C.c_double)))
        self._own = s
        self._h = C.pointer(s)
        return self

    @property
    def ptr(self):
        return self._h

    @property
    def nrows(self):
        return int(self._h.contents.nrows)

    @property
    def base(self):
        return int(self._h.contents.base)

    @property
    def nnz(self):
        return int(self._h.contents.offs[self.nrows])

    @property
    def offs(self):
        return np.ctypeslib.as_array(self._h.contents.offs, shape=(self.nrows + 1,))

    @property
    def cols(self):
        return np.ctypeslib.as_array(self._h.contents.cols, shape=(max(self.nnz, 1),))[:self.nnz]

    @property
    def vals(self):
        return np.ctypeslib.as_array(self._h.contents.vals, shape=(max(self.nnz, 1),))[:self.nnz]

    def free(self):
        if getattr(self, "_own", None) is None and self._h:
            L.load().lsb_csr_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def lsbench_matrix_read(path):
    return Matrix(L.load().lsbench_matrix_read(str(path).encode()))


def lsbench_matrix_synth(spec, r0=0, r1=0):
    n = C.c_uint()
    h = L.load().lsbench_matrix_synth(spec.encode(), r0, r1, C.byref(n))
    if not h:
        raise L.LsbenchHipError("bad synthetic spec %r" % spec)
    m = Matrix(h)
    m.n_global = n.value
    return m


def lsb_csr_symmetrize_upper(A):
    return Matrix(L.load().lsb_csr_symmetrize_upper(A.ptr))


def lsb_csr_copy_base0(A):
    return Matrix(L.load().lsb_csr_copy_base0(A.ptr))


def lsb_csr_row_slice(A, r0, r1):
    return Matrix(L.load().lsb_csr_row_slice(A.ptr, r0, r1))


def lsb_csr_partition_rows(A, nparts):
    b = (C.c_uint * (nparts + 1))()
    L.check(L.load().lsb_csr_partition_rows(A.ptr, nparts, b), "partition_rows")
    return np.array(b[:], dtype=np.int64)


def lsb_csr_row_blocks(A, cap):
    p = C.POINTER(C.c_uint)()
    nb = L.load().lsb_csr_row_blocks(A.ptr, cap, C.byref(p))
    out = np.ctypeslib.as_array(p, shape=(nb + 1,)).copy()
    C.CDLL(None).free(p)
    return out


def lsb_csr_block_lanes(A, rowblk):
    rb = np.ascontiguousarray(rowblk, dtype=np.uint32)
    out = np.zeros(len(rb) - 1, np.uint8)
    L.load().lsb_csr_block_lanes(A.ptr, rb.ctypes.data_as(C.POINTER(C.c_uint)), len(rb) - 1,
                                 out.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return out


def lsb_csr_sellize(A):
    """(sptr, cols, vals) of the sliced-ELL copy, as numpy arrays (copies)."""
    lib = L.load()
    p = lib.lsb_csr_sellize(A.ptr)
    if not p:
        raise L.LsbenchHipError("sliced-ELL copy does not fit 32-bit offsets")
    S = p.contents
    sptr = np.ctypeslib.as_array(S.sptr, (S.nslice + 1,)).copy()
    cols = np.ctypeslib.as_array(S.cols, (S.stored,)).copy()
    vals = np.ctypeslib.as_array(S.vals, (S.stored,)).copy()
    assert int(lib.lsb_csr_sell_stored(A.ptr)) == int(S.stored) == int(sptr[-1])
    lib.lsb_sell_free(p)
    return sptr, cols, vals


def lsb_csr_sellize16(A, row_begin=0):
    """(sptr, codes, sbase, vals) of the 16-bit sliced-ELL copy, or None when
    the operator cannot be encoded."""
    lib = L.load()
    p = lib.lsb_csr_sellize16(A.ptr, row_begin)
    if not p:
        return None
    S = p.contents
    sptr = np.ctypeslib.as_array(S.sptr, (S.nslice + 1,)).copy()
    nq = S.stored // L.SELL_ROWS
    codes = np.ctypeslib.as_array(S.codes, (max(S.ncode_slots, 1) * L.SELL_ROWS,)).copy()[
        :S.ncode_slots * L.SELL_ROWS]
    vals = np.ctypeslib.as_array(S.vals, (max(S.stored, 1),)).copy()[:S.stored]
    sbase = np.ctypeslib.as_array(S.sbase, (2 * nq + 2,)).copy()[:2 * nq].reshape(nq, 2)
    lib.lsb_sell_free(p)
    return sptr, codes, sbase, vals


def lsb_gmg_detect(A):
    """lsb_gmg_detect: (0, {"dim", "n": (nx, ny, nz), "c"}) for a constant-coefficient grid operator, else (the number
    of the rule it breaks, None)."""
    g = L.GmgGrid()
    rc = int(L.load().lsb_gmg_detect(A.ptr, C.byref(g)))
    return (rc, None) if rc else (0, {"dim": int(g.dim), "n": tuple(int(v) for v in g.n), "c": float(g.c)})


def lsb_gmg_plan(dims, coarse=256, max_levels=20, c=1.0):
    """lsb_gmg_plan for the grid dims = (nx, ny[, nz]): the levels as a list of ((n_d), (delta_d)), each of len(dims)
    entries; None where the coarsest level would be too large (-1)."""
    dim = len(dims)
    g = L.GmgGrid(dim, (C.c_uint * 3)(*(list(dims) + [1] * (3 - dim))), c)
    lv = (L.GmgLevel * L.GMG_MAX_LEVELS)()
    rc = int(L.load().lsb_gmg_plan(C.byref(g), coarse, max_levels, lv, L.GMG_MAX_LEVELS))
    if rc == -1:
        return None
    if rc < 1:
        raise L.LsbenchHipError("lsb_gmg_plan: bad argument (rc=%d)" % rc)
    return [(tuple(int(v) for v in lv[l].n[:dim]), tuple(float(v) for v in lv[l].delta[:dim])) for l in range(rc)]


def lsb_amg_colour(A):
    """(colour of every row as int32, number of colours) by the greedy rule of lsb_amg_colour."""
    nc = C.c_uint()
    p = L.load().lsb_amg_colour(A.ptr, C.byref(nc))
    if not p:
        raise L.LsbenchHipError("lsb_amg_colour failed")
    col = np.ctypeslib.as_array(p, shape=(max(A.nrows, 1),))[:A.nrows].astype(np.int32, copy=True)
    L.libc_free(p)
    return col, int(nc.value)


def lsb_csr_mcgs(A, colour, ncolours):
    """The colour-sorted copy of A (struct lsb_mcgs) as a dict of numpy arrays: cbeg, rowid, offs, cols, vals;
    None where lsb_csr_mcgs refuses the colouring."""
    col = np.ascontiguousarray(colour, np.int32)
    p = L.load().lsb_csr_mcgs(A.ptr, col.ctypes.data_as(C.POINTER(C.c_int)), ncolours)
    if not p:
        return None
    m = p.contents

    def arr(q, cnt, dt):
        return np.ctypeslib.as_array(q, shape=(max(cnt, 1),))[:cnt].astype(dt, copy=True)
    offs = arr(m.offs, m.n + 1, np.uint32)
    out = {"cbeg": arr(m.cbeg, m.ncolours + 1, np.uint32), "rowid": arr(m.rowid, m.n, np.uint32), "offs": offs,
           "cols": arr(m.cols, int(offs[-1]), np.uint32), "vals": arr(m.vals, int(offs[-1]), np.float64)}
    L.load().lsb_mcgs_free(p)
    return out


def lsb_mcgs_check(A, colour, copy):
    """lsb_mcgs_check of a colouring and a copy given as lsb_csr_mcgs returns it: (0, "") or (rule, its text)."""
    col = np.ascontiguousarray(colour, np.int32)
    keep = {k: np.ascontiguousarray(copy[k], np.float64 if k == "vals" else np.uint32)
            for k in ("cbeg", "rowid", "offs", "cols", "vals")}
    u = C.POINTER(C.c_uint)
    m = L.Mcgs(A.nrows, len(keep["cbeg"]) - 1, keep["cbeg"].ctypes.data_as(u), keep["rowid"].ctypes.data_as(u),
               keep["offs"].ctypes.data_as(u), keep["cols"].ctypes.data_as(u),
               keep["vals"].ctypes.data_as(C.POINTER(C.c_double)))
    why = C.create_string_buffer(512)
    rc = L.load().lsb_mcgs_check(A.ptr, col.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m), why, len(why))
    return int(rc), why.value.decode()


def lsb_csr_rcm(A):
    perm = np.zeros(A.nrows, np.uint32)
    L.check(L.load().lsb_csr_rcm(A.ptr, perm.ctypes.data_as(C.POINTER(C.c_uint))), "rcm")
    return perm


def lsb_csr_nd(A, budget=None):
    """The nested-dissection ordering of lsb_csr_nd, perm[new] = old.  With a budget: (perm or None, the lower bound
    of the entries of W this ordering cannot avoid) -- None where the bound exceeds the budget."""
    perm = np.zeros(max(A.nrows, 1), np.uint32)
    p = perm.ctypes.data_as(C.POINTER(C.c_uint))
    if budget is None:
        L.check(L.load().lsb_csr_nd(A.ptr, p), "lsb_csr_nd")
        return perm[:A.nrows]
    lower = C.c_ulonglong()
    rc = L.load().lsb_csr_nd_bounded(A.ptr, p, budget, C.byref(lower))
    if rc not in (0, 3):
        L.check(rc, "lsb_csr_nd_bounded")
    return (perm[:A.nrows] if rc == 0 else None), int(lower.value)


def lsb_csr_skyline_count(A, perm):
    """(entries of W = L^-1 under perm: the sum of the depths in the elimination tree, the tree's height)."""
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    h = C.c_uint()
    cnt = L.load().lsb_csr_skyline_count(A.ptr, perm.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(h))
    return int(cnt), int(h.value)


def lsb_csr_skyline_inverse(A, perm):
    """The skyline inverse factor (struct lsb_skyinv) as a dict of numpy arrays -- n, perm, first, woff, vals, parent,
    run_end -- or the reason it was refused as an int: 1 not positive definite, 2 over the budget, 3 memory."""
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    why = C.c_int()
    p = L.load().lsb_csr_skyline_inverse(A.ptr, perm.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(why))
    if not p:
        return int(why.value)
    w = p.contents
    n = int(w.n)

    def arr(q, cnt, dt):
        return np.ctypeslib.as_array(q, shape=(max(cnt, 1),))[:cnt].astype(dt, copy=True)
    woff = arr(w.woff, n + 1, np.uint64)
    out = {"n": n, "perm": arr(w.perm, n, np.uint32), "first": arr(w.first, n, np.uint32), "woff": woff,
           "vals": arr(w.vals, int(woff[-1]), np.float64), "parent": arr(w.parent, n, np.uint32),
           "run_end": arr(w.run_end, n, np.uint32)}
    L.load().lsb_skyinv_free(p)
    return out


def lsb_csr_tiered_count(A, perm, tiers):
    """(entries of the W_tt, entries of the coupling C, height of the whole tree) under perm in `tiers` tiers
    (1 .. DIRECT_MAX_TIERS), symbolic; None where the library refuses the arguments."""
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    w, c, h = C.c_ulonglong(), C.c_ulonglong(), C.c_uint()
    rc = L.load().lsb_csr_tiered_count(A.ptr, perm.ctypes.data_as(C.POINTER(C.c_uint)), tiers, C.byref(w), C.byref(c),
                                       C.byref(h))
    return (int(w.value), int(c.value), int(h.value)) if rc == 0 else None


def lsb_csr_tiered_inverse(A, perm, tiers):
    """The tiered inverse factor (struct lsb_tierinv) as a dict of numpy arrays -- n, ntier, lo (ntier + 1), the
    skyline arrays of lsb_csr_skyline_inverse, C as coffs / ccols / cvals (row i of the new numbering at
    coffs[i - lo[1]]) and C^T as toffs / tcols / tvals (tier t's lo[t] + 1 offsets one after another) -- or the reason
    it was refused as an int.  tiers = 0: the fewest that fit the budget."""
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    why = C.c_int()
    p = L.load().lsb_csr_tiered_inverse(A.ptr, perm.ctypes.data_as(C.POINTER(C.c_uint)), tiers, C.byref(why))
    if not p:
        return int(why.value)
    w = p.contents
    n, ntier = int(w.n), int(w.ntier)

    def arr(q, cnt, dt):
        return np.ctypeslib.as_array(q, shape=(max(cnt, 1),))[:cnt].astype(dt, copy=True)
    lo = np.array(list(w.lo)[:ntier + 1], np.int64)
    woff = arr(w.woff, n + 1, np.uint64)
    coffs = arr(w.coffs, n - int(lo[min(1, ntier)]) + 1, np.uint32)
    toffs = arr(w.toffs, int((lo[1:ntier] + 1).sum()), np.uint32)
    nc = int(coffs[-1])
    out = {"n": n, "ntier": ntier, "lo": lo, "perm": arr(w.perm, n, np.uint32), "first": arr(w.first, n, np.uint32),
           "woff": woff, "vals": arr(w.vals, int(woff[-1]), np.float64), "parent": arr(w.parent, n, np.uint32),
           "run_end": arr(w.run_end, n, np.uint32), "coffs": coffs, "ccols": arr(w.ccols, nc, np.uint32),
           "cvals": arr(w.cvals, nc, np.float64), "toffs": toffs, "tcols": arr(w.tcols, nc, np.uint32),
           "tvals": arr(w.tvals, nc, np.float64)}
    L.load().lsb_tierinv_free(p)
    return out


def lsb_csr_permute_sym(A, perm):
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    return Matrix(L.load().lsb_csr_permute_sym(A.ptr, perm.ctypes.data_as(C.POINTER(C.c_uint))))


def lsb_csr_bandwidth(A):
    return int(L.load().lsb_csr_bandwidth(A.ptr))


def lsb_csr_col_hull(A):
    lo, hi = C.c_uint(), C.c_uint()
    L.load().lsb_csr_col_hull(A.ptr, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def lsb_plan_exchange(me, hull):
    """hull: (nall, 4) array of {row_begin, nrows, col_lo, col_hi}.
    Returns (recvs, sends) as lists of (peer, offset, count)."""
    hull = np.ascontiguousarray(hull, dtype=np.uint32)
    nall = hull.shape[0]
    recv, send = (L.Xfer * nall)(), (L.Xfer * nall)()
    nr, ns = C.c_int(), C.c_int()
    L.load().lsb_plan_exchange(me, nall, hull.ctypes.data_as(C.POINTER(C.c_uint)),
                               recv, C.byref(nr), send, C.byref(ns))
    f = lambda a, n: [(a[i].peer, a[i].offset, a[i].count) for i in range(n)]
    return f(recv, nr.value), f(send, ns.value)


def default_opts(**kw):
    o = L.Opts()
    L.load().lsb_hip_opts_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def hip_cdna4_init():
    return L.load().hip_cdna4_init()


def hip_cdna4_finalize():
    return L.load().hip_cdna4_finalize()


def hip_cdna4_bench(A, r=None, trials=1, matrix_name="(memory)", opts=None):
    """The drop-in entry point, called the way lsbench_bench calls a backend
    (reference: src/lsbench.c:156-187): x = zeros, r_i = i unless given.
    Returns x (numpy)."""
    lib = L.load()
    m = A.nrows
    x = np.zeros(m, np.float64)
    r = np.arange(m, dtype=np.float64) if r is None else np.ascontiguousarray(r, np.float64)
    if opts is not None:
        lib.lsb_hip_set_opts(C.byref(opts))
    cb = L.LsbenchStruct(matrix_name.encode(), L.SOLVER_HIP, 0, 0, 0, trials)
    rc = lib.hip_cdna4_bench(x.ctypes.data_as(C.POINTER(C.c_double)), A.ptr,
                             r.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cb))
    L.check(rc, "hip_cdna4_bench")
    return x


def last_result():
    r = L.Result()
    L.load().lsb_hip_last_result(C.byref(r))
    return r


class Solver:
    """lsb_hip_solver handle: operator resident in HBM."""

    def __init__(self, A, opts=None, row_begin=None, n_global=None):
        lib = L.load()
        self.opts = opts if opts is not None else default_opts()
        if row_begin is None:
            h = lib.lsb_hip_solver_create(A.ptr, C.byref(self.opts))
        else:
            h = lib.lsb_hip_solver_create_dist(A.ptr, row_begin, n_global, C.byref(self.opts))
        if not h:
            raise L.LsbenchHipError("lsb_hip_solver_create failed: backend not "
                                    "initialised (no GPU?) -- there is no CPU path")
        self._adopt(h)

    def _adopt(self, h):
        lib = L.load()
        self._h = h
        self.n_local = lib.lsb_hip_solver_nrows_local(h)
        self.n_global = lib.lsb_hip_solver_nrows_global(h)
        self.nnz_local = lib.lsb_hip_solver_nnz_local(h)

    @classmethod
    def create_direct(cls, A, opts, tiers=0):
        """A direct solver (opts.krylov = KRYLOV_DIRECT) whose inverse factor is kept in `tiers` tiers: 1 is
        Solver(A, opts), 0 takes the fewest tiers that fit the entry budget.  See lsb_hip_solver_create_direct."""
        self = cls.__new__(cls)
        self.opts = opts
        h = L.load().lsb_hip_solver_create_direct(A.ptr, C.byref(opts), tiers)
        if not h:
            raise L.LsbenchHipError("lsb_hip_solver_create_direct failed: backend not initialised (no GPU?), "
                                    "opts.krylov is not KRYLOV_DIRECT, or tiers is out of 0 .. %d"
                                    % L.DIRECT_MAX_TIERS)
        self._adopt(h)
        return self

    def direct_tier_info(self):
        """(tiers, entries of the W_tt, entries of the coupling, rows per tier, launches per round) of a direct solver;
        None for any other."""
        nt, w, c, lp = C.c_uint(), C.c_ulonglong(), C.c_ulonglong(), C.c_uint()
        rows = (C.c_uint * L.DIRECT_MAX_TIERS)()
        rc = L.load().lsb_hip_solver_direct_tier_info(self._h, C.byref(nt), C.byref(w), C.byref(c), rows, C.byref(lp))
        return (int(nt.value), int(w.value), int(c.value), list(rows)[:nt.value], int(lp.value)) if rc == 0 else None

    def solve(self, b, x0=None):
        """x0: an initial guess (n_local); None solves from zero."""
        b = np.ascontiguousarray(b, np.float64)
        res = L.Result()
        if x0 is None:
            x = np.empty(self.n_local, np.float64)
            L.check(L.load().lsb_hip_solver_solve(self._h, b.ctypes.data, x.ctypes.data,
                                                  C.byref(res)), "solve")
            return x, res
        x = np.array(x0, dtype=np.float64, order="C")
        if x.shape != (self.n_local,):
            raise ValueError("solve: x0 must hold n_local values")
        L.check(L.load().lsb_hip_solver_solve_x0(self._h, b.ctypes.data, x.ctypes.data,
                                                 C.byref(res)), "solve_x0")
        return x, res

    def solve_dev(self, d_b, d_x, warm=False):
        """warm: d_x holds the initial guess on entry."""
        res = L.Result()
        lib = L.load()
        if warm:
            L.check(lib.lsb_hip_solver_solve_x0_dev(self._h, _ptr(d_b), _ptr(d_x), C.byref(res)), "solve_x0_dev")
        else:
            L.check(lib.lsb_hip_solver_solve_dev(self._h, _ptr(d_b), _ptr(d_x), C.byref(res)), "solve_dev")
        return res

    def start_relres(self, nrhs=1):
        """||b_c - S x0_c|| / ||b_c|| of the nrhs columns of the last solve, which must have been a warm-started
        one of that many columns (0 where b_c = 0)."""
        out = (C.c_double * max(nrhs, 1))()
        L.check(L.load().lsb_hip_solver_start_relres(self._h, nrhs, out), "start_relres")
        return np.array(out[:nrhs])

    def seq_begin(self, depth):
        """Successive right-hand sides: keep a basis of up to `depth` (1 .. SEQ_MAX_DEPTH) earlier solutions on the
        device and empty it; 0 frees it.  Raises on a solver the projection does not serve (shards, GMRES,
        BiCGSTAB)."""
        L.check(L.load().lsb_hip_solver_seq_begin(self._h, depth), "seq_begin")

    def solve_seq(self, b):
        """One solve of a sequence, from the projection of b on the basis (an empty basis: solve(b)).  Returns
        (x, result); the basis takes what was solved for."""
        b = np.ascontiguousarray(b, np.float64)
        if b.shape != (self.n_local,):
            raise ValueError("solve_seq: b must hold n_local values")
        x = np.empty(self.n_local, np.float64)
        res = L.Result()
        L.check(L.load().lsb_hip_solver_solve_seq(self._h, b.ctypes.data, x.ctypes.data, C.byref(res)), "solve_seq")
        return x, res

    def solve_seq_dev(self, d_b, d_x):
        res = L.Result()
        L.check(L.load().lsb_hip_solver_solve_seq_dev(self._h, _ptr(d_b), _ptr(d_x), C.byref(res)), "solve_seq_dev")
        return res

    @property
    def seq_info(self):
        """(depth, pairs held, restarts since seq_begin, device bytes held); all 0 without a basis."""
        d, h, r, by = C.c_uint(), C.c_uint(), C.c_uint(), C.c_ulonglong()
        L.check(L.load().lsb_hip_solver_seq_info(self._h, C.byref(d), C.byref(h), C.byref(r), C.byref(by)),
                "seq_info")
        return d.value, h.value, r.value, int(by.value)

    def seq_basis_dev(self, k, d_xk, d_sxk):
        """Pair k < held, (x~_k, S x~_k), into two device vectors of n_local doubles in the caller's numbering."""
        L.check(L.load().lsb_hip_solver_seq_basis_dev(self._h, k, _ptr(d_xk), _ptr(d_sxk)), "seq_basis_dev")

    @property
    def seq_last_us(self):
        """(projection, update): device microseconds of the last solve_seq's two parts, 0 where it had none.  The
        events are recorded only once this was asked: the first look behind a seq_begin turns them on, answers 0, 0."""
        p, u = C.c_double(), C.c_double()
        L.check(L.load().lsb_hip_solver_seq_last_us(self._h, C.byref(p), C.byref(u)), "seq_last_us")
        return p.value, u.value

    def spmv_dev(self, d_x, d_y):
        L.check(L.load().lsb_hip_solver_spmv_dev(self._h, _ptr(d_x), _ptr(d_y)), "spmv_dev")

    @staticmethod
    def _block(t, what):
        """(pointer, nrhs, ld) of a 2-D torch tensor of shape (nrhs, ld'): one row per column of the block"""
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError("%s: a 2-D tensor (nrhs, ld) with unit stride along its rows is needed" % what)
        return _ptr(t), int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

    def spmm_dev(self, d_X, d_Y):
        """Y = Op X for the nrhs columns held as the ROWS of two 2-D device tensors (ld = stride(0))."""
        px, k, ldx = self._block(d_X, "spmm_dev")
        py, ky, ldy = self._block(d_Y, "spmm_dev")
        if k != ky:
            raise ValueError("spmm_dev: X and Y hold different numbers of columns")
        L.check(L.load().lsb_hip_solver_spmm_dev(self._h, k, px, ldx, py, ldy), "spmm_dev")

    def solve_multi_dev(self, d_B, d_X, warm=False):
        """x_c = S^-1 b_c for the nrhs columns held as the ROWS of two 2-D device tensors; returns the list of
        their Results.  warm: the rows of d_X hold the columns' initial guesses on entry."""
        pb, k, ldb = self._block(d_B, "solve_multi_dev")
        px, kx, ldx = self._block(d_X, "solve_multi_dev")
        if k != kx:
            raise ValueError("solve_multi_dev: B and X hold different numbers of columns")
        res = (L.Result * max(k, 1))()
        lib = L.load()
        if warm:
            L.check(lib.lsb_hip_solver_solve_multi_x0_dev(self._h, k, pb, ldb, px, ldx, res), "solve_multi_x0_dev")
        else:
            L.check(lib.lsb_hip_solver_solve_multi_dev(self._h, k, pb, ldb, px, ldx, res), "solve_multi_dev")
        return list(res)[:k]

    def solve_multi(self, B):
        """B: numpy (n_local, nrhs) of any order.  Returns (X of the same shape, [Result, ...])."""
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.n_local:
            raise ValueError("solve_multi: B must be (n_local, nrhs)")
        k = B.shape[1]
        X = np.empty((self.n_local, k), np.float64, order="F")
        res = (L.Result * max(k, 1))()
        ld = max(self.n_local, 1)
        L.check(L.load().lsb_hip_solver_solve_multi(self._h, k, B.ctypes.data, ld, X.ctypes.data, ld, res),
                "solve_multi")
        return X, list(res)[:k]

    def multi_iteration_bytes(self, nrhs):
        """Bytes one iteration of a batch of nrhs right-hand sides must move (see lsbench_hip.h); 0 where
        solve_multi does not apply."""
        return int(L.load().lsb_hip_solver_multi_iteration_bytes(self._h, nrhs))

    def solve_block_dev(self, d_B, d_X, precond=False):
        """Block-CG proper: x_c = S^-1 b_c for the 2 .. 8 columns held as the ROWS of two 2-D device tensors, searched
        in ONE Krylov space; returns the list of their Results (the same iteration count in each).  A rank-deficient
        block (rc 3) leaves d_X untouched and returns every status BREAKDOWN; a solver the block form does not serve
        raises.  precond: lsb_hip_solver_solve_block_precond_dev, which also serves AMG and FSAI (fsai_blocks)
        solvers and forwards a diagonal one here."""
        pb, k, ldb = self._block(d_B, "solve_block_dev")
        px, kx, ldx = self._block(d_X, "solve_block_dev")
        if k != kx:
            raise ValueError("solve_block_dev: B and X hold different numbers of columns")
        res = (L.Result * max(k, 1))()
        lib = L.load()
        fn = lib.lsb_hip_solver_solve_block_precond_dev if precond else lib.lsb_hip_solver_solve_block_dev
        rc = fn(self._h, k, pb, ldb, px, ldx, res)
        if rc != 3:
            L.check(rc, "solve_block_dev")
        return list(res)[:k]

    def solve_block(self, B, precond=False):
        """B: numpy (n_local, nrhs) of any order, 2 <= nrhs <= 8.  Returns (X of the same shape, [Result, ...]); a
        rank-deficient block (rc 3) returns X unwritten and every status BREAKDOWN.  precond: as solve_block_dev's."""
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.n_local:
            raise ValueError("solve_block: B must be (n_local, nrhs)")
        k = B.shape[1]
        X = np.empty((self.n_local, k), np.float64, order="F")
        res = (L.Result * max(k, 1))()
        ld = max(self.n_local, 1)
        lib = L.load()
        fn = lib.lsb_hip_solver_solve_block_precond if precond else lib.lsb_hip_solver_solve_block
        rc = fn(self._h, k, B.ctypes.data, ld, X.ctypes.data, ld, res)
        if rc != 3:
            L.check(rc, "solve_block")
        return X, list(res)[:k]

    def block_iteration_bytes(self, nrhs):
        """Bytes one iteration of a block of nrhs right-hand sides must move (see lsbench_hip.h); 0 where the block
        form is not served."""
        return int(L.load().lsb_hip_solver_block_iteration_bytes(self._h, nrhs))

    def block_precond_iteration_bytes(self, nrhs):
        """Bytes one iteration of solve_block(precond=True) must move (see lsbench_hip.h); 0 under AMG and where
        nothing is served."""
        return int(L.load().lsb_hip_solver_block_precond_iteration_bytes(self._h, nrhs))

    def block_norms(self, nrhs):
        """(rr, bb): the recurrence's ||r_c||^2 and ||b_c||^2 out of the device state of the last block solved."""
        rr, bb = (C.c_double * 8)(), (C.c_double * 8)()
        L.check(L.load().lsb_hip_solver_block_norms(self._h, nrhs, rr, bb), "block_norms")
        return np.array(rr[:nrhs]), np.array(bb[:nrhs])

    def spmv_inner_dev(self, d_x, d_y, d_dot=None):
        """y = the product the Krylov loop issues (fp32 matrix values under PREC_MIXED, where spmv_dev
        stays exact); d_dot (one shard only): the launch's fused x.y."""
        L.check(L.load().lsb_hip_solver_spmv_inner_dev(self._h, _ptr(d_x), _ptr(d_y), _ptr(d_dot)),
                "spmv_inner_dev")

    def precond_dev(self, d_r, d_z):
        """z = M^-1 r once with the solver's preconditioner (device buffers, n_local each)."""
        L.check(L.load().lsb_hip_solver_precond_dev(self._h, _ptr(d_r), _ptr(d_z)), "precond_dev")

    def precond_padded_dev(self, d_r, d_z):
        """For tests, GMG solvers only: z = M^-1 r in the solver's own numbering (n_local + padded rows each; the pad
        rows of r are 0)."""
        L.check(L.load().lsb_hip_solver_precond_padded_dev(self._h, _ptr(d_r), _ptr(d_z)), "precond_padded_dev")

    def precond_multi_dev(self, d_R, d_Z):
        """Z = M^-1 R (AMG: one V-cycle per column; FSAI with opts.fsai_blocks: G^T (G r)) for the nrhs columns held
        as the ROWS of two 2-D device tensors (ld = stride(0)); under AMG a column of Z has the bits of precond_dev
        on that column alone."""
        pr, k, ldr = self._block(d_R, "precond_multi_dev")
        pz, kz, ldz = self._block(d_Z, "precond_multi_dev")
        if k != kz:
            raise ValueError("precond_multi_dev: R and Z hold different numbers of columns")
        L.check(L.load().lsb_hip_solver_precond_multi_dev(self._h, k, pr, ldr, pz, ldz), "precond_multi_dev")

    @property
    def fsai_nnz(self):
        """(entries of G, entries of G^T) of an FSAI-preconditioned solver; None for any other."""
        g, gt = C.c_ulonglong(), C.c_ulonglong()
        rc = L.load().lsb_hip_solver_fsai_nnz(self._h, C.byref(g), C.byref(gt))
        if rc == 2:
            return None
        L.check(rc, "fsai_nnz")
        return int(g.value), int(gt.value)

    @property
    def amg_info(self):
        """(levels, levels in the one-launch tail) of an AMG-preconditioned solver."""
        lv, tl = C.c_uint(), C.c_uint()
        L.check(L.load().lsb_hip_solver_amg_info(self._h, C.byref(lv), C.byref(tl)), "amg_info")
        return lv.value, tl.value

    @property
    def amg_precision(self):
        """AMG_PREC_FP64 or AMG_PREC_FP32, the precision of the V-cycle; None for a solver without AMG."""
        rc = L.load().lsb_hip_solver_amg_precision(self._h)
        return None if rc == 2 else rc

    @property
    def amg_cycle_bytes(self):
        """Bytes one application of the AMG V-cycle must move (0 without AMG)."""
        return int(L.load().lsb_hip_solver_amg_cycle_bytes(self._h))

    @property
    def gmg_info(self):
        """(levels, (nx, ny, nz), pitch of the fine level's lines) of a GMG-preconditioned solver; None for any
        other."""
        lv, dims, pitch = C.c_uint(), (C.c_uint * 3)(), C.c_uint()
        rc = L.load().lsb_hip_solver_gmg_info(self._h, C.byref(lv), dims, C.byref(pitch))
        if rc == 2:
            return None
        L.check(rc, "gmg_info")
        return int(lv.value), tuple(int(v) for v in dims), int(pitch.value)

    def gmg_level(self, level):
        """((n_d), (delta_d)), three entries each, of one level of a GMG-preconditioned solver; None for a level out
        of range or another preconditioner."""
        n, delta = (C.c_uint * 3)(), (C.c_double * 3)()
        rc = L.load().lsb_hip_solver_gmg_level(self._h, level, n, delta)
        if rc == 2:
            return None
        L.check(rc, "gmg_level")
        return tuple(int(v) for v in n), tuple(float(v) for v in delta)

    @property
    def gmg_cycle_bytes(self):
        """Bytes one application of the geometric V-cycle must move (0 without it)."""
        return int(L.load().lsb_hip_solver_gmg_cycle_bytes(self._h))

    @property
    def direct_info(self):
        """(entries of W, height of the elimination tree, bytes the two products of a round stream) of a direct
        solver (KRYLOV_DIRECT); None for any other."""
        e, h, by = C.c_ulonglong(), C.c_uint(), C.c_ulonglong()
        rc = L.load().lsb_hip_solver_direct_info(self._h, C.byref(e), C.byref(h), C.byref(by))
        return None if rc == 2 else (int(e.value), int(h.value), int(by.value))

    def solve_direct_multi_dev(self, d_B, d_X):
        """A direct solver (KRYLOV_DIRECT) on a block: x_c = S^-1 b_c for the nrhs columns held as the ROWS of two 2-D
        device tensors, W streamed once per product for a block of columns; returns the list of their Results.  A
        column has the bits of solve_dev on that column alone.  Any other solver raises."""
        pb, k, ldb = self._block(d_B, "solve_direct_multi_dev")
        px, kx, ldx = self._block(d_X, "solve_direct_multi_dev")
        if k != kx:
            raise ValueError("solve_direct_multi_dev: B and X hold different numbers of columns")
        res = (L.Result * max(k, 1))()
        L.check(L.load().lsb_hip_solver_solve_direct_multi_dev(self._h, k, pb, ldb, px, ldx, res),
                "solve_direct_multi_dev")
        return list(res)[:k]

    def solve_direct_multi(self, B):
        """B: numpy (n_local, nrhs) of any order.  Returns (X of the same shape, [Result, ...])."""
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.n_local:
            raise ValueError("solve_direct_multi: B must be (n_local, nrhs)")
        k = B.shape[1]
        X = np.empty((self.n_local, k), np.float64, order="F")
        res = (L.Result * max(k, 1))()
        ld = max(self.n_local, 1)
        L.check(L.load().lsb_hip_solver_solve_direct_multi(self._h, k, B.ctypes.data, ld, X.ctypes.data, ld, res),
                "solve_direct_multi")
        return X, list(res)[:k]

    def direct_apply_multi_dev(self, d_R, d_Z):
        """Z_c = P^T W^T W P R_c once for the nrhs columns held as the ROWS of two 2-D device tensors: a column of Z
        has the bits of precond_dev on that column alone."""
        pr, k, ldr = self._block(d_R, "direct_apply_multi_dev")
        pz, kz, ldz = self._block(d_Z, "direct_apply_multi_dev")
        if k != kz:
            raise ValueError("direct_apply_multi_dev: R and Z hold different numbers of columns")
        L.check(L.load().lsb_hip_solver_direct_apply_multi_dev(self._h, k, pr, ldr, pz, ldz), "direct_apply_multi_dev")

    def direct_multi_round_bytes(self, nrhs):
        """Bytes one round of a block of nrhs right-hand sides streams on a direct solver (see lsbench_hip.h); 0 for
        any other solver."""
        return int(L.load().lsb_hip_solver_direct_multi_round_bytes(self._h, nrhs))

    def solve_direct_tier_multi_dev(self, d_B, d_X):
        """solve_direct_multi_dev on every direct solver, one with a tiered factor (create_direct) included: the
        tiers' launches run on the block, every entry of the factor and of its coupling loaded once per product for
        all columns.  A column has the bits of solve_dev on that column alone on the same solver.  A single skyline is
        forwarded to solve_direct_multi_dev.  Any solver that is not direct raises."""
        pb, k, ldb = self._block(d_B, "solve_direct_tier_multi_dev")
        px, kx, ldx = self._block(d_X, "solve_direct_tier_multi_dev")
        if k != kx:
            raise ValueError("solve_direct_tier_multi_dev: B and X hold different numbers of columns")
        res = (L.Result * max(k, 1))()
        L.check(L.load().lsb_hip_solver_solve_direct_tier_multi_dev(self._h, k, pb, ldb, px, ldx, res),
                "solve_direct_tier_multi_dev")
        return list(res)[:k]

    def solve_direct_tier_multi(self, B):
        """B: numpy (n_local, nrhs) of any order.  Returns (X of the same shape, [Result, ...])."""
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.n_local:
            raise ValueError("solve_direct_tier_multi: B must be (n_local, nrhs)")
        k = B.shape[1]
        X = np.empty((self.n_local, k), np.float64, order="F")
        res = (L.Result * max(k, 1))()
        ld = max(self.n_local, 1)
        L.check(L.load().lsb_hip_solver_solve_direct_tier_multi(self._h, k, B.ctypes.data, ld, X.ctypes.data, ld, res),
                "solve_direct_tier_multi")
        return X, list(res)[:k]

    def direct_tier_apply_multi_dev(self, d_R, d_Z):
        """One application of the factor, tiered or not, to the nrhs columns held as the ROWS of two 2-D device
        tensors: a column of Z has the bits of precond_dev on that column alone."""
        pr, k, ldr = self._block(d_R, "direct_tier_apply_multi_dev")
        pz, kz, ldz = self._block(d_Z, "direct_tier_apply_multi_dev")
        if k != kz:
            raise ValueError("direct_tier_apply_multi_dev: R and Z hold different numbers of columns")
        L.check(L.load().lsb_hip_solver_direct_tier_apply_multi_dev(self._h, k, pr, ldr, pz, ldz),
                "direct_tier_apply_multi_dev")

    def direct_tier_multi_round_bytes(self, nrhs):
        """Bytes one round of a block of nrhs right-hand sides streams on a direct solver, tiered or not (see
        lsbench_hip.h); at nrhs = 1 direct_info's figure; 0 for any other solver."""
        return int(L.load().lsb_hip_solver_direct_tier_multi_round_bytes(self._h, nrhs))

    def amg_solve_multi_dev(self, d_B, d_X):
        """AMG as the solver (KRYLOV_RICHARDSON, PRECOND_AMG) on a block: stationary V-cycle iterations from x0 = 0 for
        the nrhs columns held as the ROWS of two 2-D device tensors, the hierarchy streamed once per cycle for a block
        of columns; returns the list of their Results.  A column's x, iters, status and relres do not depend on the
        block it runs in.  A solver that is not served raises."""
        pb, k, ldb = self._block(d_B, "amg_solve_multi_dev")
        px, kx, ldx = self._block(d_X, "amg_solve_multi_dev")
        if k != kx:
            raise ValueError("amg_solve_multi_dev: B and X hold different numbers of columns")
        res = (L.Result * max(k, 1))()
        L.check(L.load().lsb_hip_solver_amg_solve_multi_dev(self._h, k, pb, ldb, px, ldx, res), "amg_solve_multi_dev")
        return list(res)[:k]

    def amg_solve_multi(self, B):
        """B: numpy (n_local, nrhs) of any order.  Returns (X of the same shape, [Result, ...])."""
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.n_local:
            raise ValueError("amg_solve_multi: B must be (n_local, nrhs)")
        k = B.shape[1]
        X = np.empty((self.n_local, k), np.float64, order="F")
        res = (L.Result * max(k, 1))()
        ld = max(self.n_local, 1)
        L.check(L.load().lsb_hip_solver_amg_solve_multi(self._h, k, B.ctypes.data, ld, X.ctypes.data, ld, res),
                "amg_solve_multi")
        return X, list(res)[:k]

    def amg_cycle_multi_dev(self, d_R, d_Z):
        """Z = M^-1 R, one V-cycle per column in the precision the solver cycles in, for the nrhs columns held as the
        ROWS of two 2-D device tensors: a column of Z has the bits of precond_dev on that column alone."""
        pr, k, ldr = self._block(d_R, "amg_cycle_multi_dev")
        pz, kz, ldz = self._block(d_Z, "amg_cycle_multi_dev")
        if k != kz:
            raise ValueError("amg_cycle_multi_dev: R and Z hold different numbers of columns")
        L.check(L.load().lsb_hip_solver_amg_cycle_multi_dev(self._h, k, pr, ldr, pz, ldz), "amg_cycle_multi_dev")

    def amg_solve_multi_bytes(self, nrhs):
        """Bytes one cycle of amg_solve_multi on a block of nrhs right-hand sides must move (see lsbench_hip.h); 0 for
        a solver that is not served."""
        return int(L.load().lsb_hip_solver_amg_solve_multi_bytes(self._h, nrhs))

    def amg_cheb_interval(self, level):
        """(lo, hi) of D^-1 A the Chebyshev smoother of an AMG level was built on; None where the level is not
        smoothed by one (the coarsest level, an l1-Jacobi solver, another preconditioner)."""
        lo, hi = C.c_double(), C.c_double()
        rc = L.load().lsb_hip_solver_amg_cheb_interval(self._h, level, C.byref(lo), C.byref(hi))
        if rc == 2:
            return None
        L.check(rc, "amg_cheb_interval")
        return lo.value, hi.value

    def amg_colours(self, level):
        """Colours of the multicolour Gauss-Seidel sweeps of an AMG level; 0 for a level whose colouring exceeds the
        cap and which keeps l1-Jacobi; None for the coarsest level, a level out of range and a solver of another
        smoother or preconditioner."""
        nc = C.c_uint()
        rc = L.load().lsb_hip_solver_amg_colours(self._h, level, C.byref(nc))
        if rc == 2:
            return None
        L.check(rc, "amg_colours")
        return int(nc.value)

    @property
    def cheb_interval(self):
        """(lmin, lmax) of D^-1 S the Chebyshev preconditioner's polynomial was built on."""
        lo, hi = C.c_double(), C.c_double()
        L.check(L.load().lsb_hip_solver_cheb_interval(self._h, C.byref(lo), C.byref(hi)), "cheb_interval")
        return lo.value, hi.value

    def time_spmv(self, warm=5, reps=50):
        ms = C.c_double()
        L.check(L.load().lsb_hip_solver_time_spmv(self._h, warm, reps, C.byref(ms)),
                "time_spmv")
        return ms.value

    def jacobi_sweep_dev(self, w, d_b, d_x):
        L.check(L.load().lsb_hip_solver_jacobi_sweep_dev(self._h, w, _ptr(d_b), _ptr(d_x)),
                "jacobi_sweep_dev")

    @property
    def nblocks(self):
        return L.load().lsb_hip_solver_nblocks(self._h)

    @property
    def spmv_variant(self):
        return L.load().lsb_hip_solver_spmv_variant(self._h)

    @property
    def spmv_flags(self):
        return L.load().lsb_hip_solver_spmv_flags(self._h)

    @property
    def spmv_grid(self):
        return L.load().lsb_hip_solver_spmv_grid(self._h)

    @property
    def padded(self):
        """Pad rows of a line-padded 2-D grid inside the solver (0: none)."""
        return int(L.load().lsb_hip_solver_padded(self._h))

    @property
    def slab_mask(self):
        """Vectors inside the first shard's slab: bit 0 r, 1 the gather vector, 2 the second direction
        buffer, 3 / 4 the x / b of a padded or re-ordered solver."""
        return int(L.load().lsb_hip_solver_slab_mask(self._h))

    @property
    def spmv_col_slices(self):
        """Slices shard 0's z-column plan walks in columns (k_spmv_tmpl_col); 0 = no plan."""
        return int(L.load().lsb_hip_solver_spmv_col_slices(self._h))

    @property
    def spmv_period(self):
        return L.load().lsb_hip_solver_spmv_period(self._h)

    @property
    def sell_value_slots(self):
        """(slots that keep their 128 values, all slots) of the 16-bit sliced-ELL form in use,
        (0, 0) for every other form."""
        import ctypes as C
        k, t = C.c_uint(0), C.c_uint(0)
        L.load().lsb_hip_solver_sell_value_slots(self._h, C.byref(k), C.byref(t))
        return int(k.value), int(t.value)

    @property
    def spmv_layout_bytes(self):
        """Bytes one launch of the SpMV form in use must move: its matrix-side arrays as
        stored + x once + y once (0 for the multi-pass forms)."""
        return int(L.load().lsb_hip_solver_spmv_layout_bytes(self._h))

    @property
    def iteration_bytes(self):
        """Bytes one Krylov iteration must move (SpMV layout + the sweeps' vector passes); 0 where
        the iteration has another shape (see lsbench_hip.h)."""
        return int(L.load().lsb_hip_solver_iteration_bytes(self._h))

    @property
    def single_reduction(self):
        """True where the PCG iteration runs in its single-reduction form (see lsbench_hip.h)."""
        return bool(L.load().lsb_hip_solver_single_reduction(self._h))

    @property
    def fused_p(self):
        """0 / 1 / 2: the direction update rides in the next SpMV launch (see lsbench_hip.h)."""
        return int(L.load().lsb_hip_solver_fused_p(self._h))

    @property
    def blas1_nt(self):
        """mask of the sweeps' nontemporal operands (see lsbench_hip.h)"""
        return int(L.load().lsb_hip_solver_blas1_nt(self._h))

    @property
    def comm_plan(self):
        """The exchange plan of this process's first shard (see lsbench_hip.h)."""
        p = (C.c_ulonglong * 8)()
        L.load().lsb_hip_solver_comm_plan(self._h, p)
        us = (C.c_double * 2)()
        L.load().lsb_hip_solver_overlap(self._h, us)
        return {"rccl_ranks": int(p[0]), "recv_peers": int(p[1]), "send_peers": int(p[2]),
                "bytes_recv_per_exchange": int(p[3]), "bytes_sent_per_exchange": int(p[4]),
                "pattern": "all-gather" if p[5] else "halos (point-to-point)",
                "shards_in_process": int(p[6]), "overlap": bool(p[7]),
                # opts.overlap = -1: both forms of the sharded SpMV timed on this communicator at creation
                "overlap_timed_us": {"plain": us[0], "split": us[1]} if us[0] > 0 else None}

    @property
    def comm(self):
        """(mode, p2p_us, rccl_us): mode 0 = one shard, 1 = RCCL / device copies,
        2 = direct xGMI stores for the all-reduces, 3 = and for the halos; the
        two times are the creation-time self-test's cost of one exchange +
        all-reduce each way (0 when it did not run)."""
        a, b = C.c_double(), C.c_double()
        m = L.load().lsb_hip_solver_comm(self._h, C.byref(a), C.byref(b))
        return m, a.value, b.value

    @property
    def overlaps(self):
        """True when the halo exchange runs behind the interior rows."""
        return bool(L.load().lsb_hip_solver_overlaps(self._h))

    def destroy(self):
        if self._h:
            L.load().lsb_hip_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
