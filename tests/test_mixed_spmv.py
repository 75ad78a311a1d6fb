"""The fp32-valued SpMV kernels (opts.precision = LSB_PREC_MIXED: the inner CG multiplies by
S~ = fp32(S)) element by element against S~ -- at the kernel level through lsb_hip_spmv_csr_f64 with
LSB_SP_F32 and a float32 value array, at the solver level through lsb_hip_solver_spmv_inner_dev, the
product the Krylov loop really issues (spmv_dev stays the exact fp64 one).  A refined solve cannot
see an inner operator that is slightly wrong: the refinement recomputes b - S x in fp64 and only takes
more corrections.

Reference: S~ = vals.astype(float32).astype(float64) (the rounding of the upload), y_ref a numpy
longdouble row sum over S~.  Bound: test_gpu_parity._check_spmv's, |y - y_ref|_i <= 4 eps max(nnz_i, 1)
sum_j |a~_ij x_j| -- an fp32 value converts to fp64 exactly and every product and sum is fp64, so the
fp64 bound applies unchanged.  Fused dot: |dot - x.y_ref| <= 1e-12 sum |x_i y_i|.
"""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import EPS, GAMMA, _dev, _edge_matrix

F32 = 32                       # LSB_SP_F32
BLOCK_NNZ = 2048               # LSB_BLOCK_NNZ
_cache = {}


# ---------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------
def _third(hip, spec):
    """a constant-coefficient grid with every value divided by 3: constants that are no fp32 numbers"""
    A = hip.lsbench_matrix_synth(spec)
    return hip.Matrix.from_arrays(A.offs.copy(), A.cols.copy(), A.vals / 3.0)


def _vary(hip, nx, ny):
    """5-point grid, diagonal 4, +-nx = -1, the (i, i + 1) weights -(0.25 + 0.5 U[0, 1)) set symmetrically:
    SPD by dominance (3.5 < 4); the +-1 slots keep their values inside shaped templates"""
    import scipy.sparse as sp
    n = nx * ny
    w = -(0.25 + 0.5 * np.random.default_rng(nx + ny).random(n - 1))
    w[np.arange(1, n) % nx == 0] = 0.0                                   # no +-1 across a line end
    M = sp.diags([-np.ones(n - nx), w, 4.0 * np.ones(n), w, -np.ones(n - nx)], [-nx, -1, 0, 1, nx], format="csr")
    M.eliminate_zeros()
    M.sort_indices()
    return hip.Matrix.from_arrays(M.indptr, M.indices, M.data)


def _op(hip, name, matrix_path=None):
    """(Matrix, columns, declared fp32-exact) by name, built once"""
    if name not in _cache:
        exact = False
        ncol = None
        if name in ("xn3b_A_18", "tj7a_A_18"):
            A = hip.lsb_csr_symmetrize_upper(hip.lsbench_matrix_read(matrix_path(name)))
        elif name == "edge":
            A, ncol = _edge_matrix(hip)
        elif name.startswith("third:"):
            A = _third(hip, name[6:])
        elif name.startswith("vary:"):
            A = _vary(hip, *[int(v) for v in name[5:].split("x")])
        else:
            A = hip.lsbench_matrix_synth(name)
            exact = "coef" not in name and not name.startswith("powerlaw")   # the Laplacians' -1, 4, 6
        _cache[name] = (A, ncol if ncol else A.nrows, exact)
    return _cache[name]


GENERAL = "lap2d:nx=411,ny=203,coef=1"
POWERLAW = "powerlaw:n=40000,gamma=%r,max=4096,seed=3" % GAMMA          # longest row 4068 > 2048
POWERLAW_SELL = "powerlaw:n=20000,gamma=%r,max=512,seed=3" % GAMMA      # (a sliced-ELL copy pads every slice to its longest row)
POWERLAW_SELL16 = "powerlaw:n=20000,gamma=%r,max=200,seed=3" % GAMMA
FILES = ["xn3b_A_18", "tj7a_A_18"]
TINY = ["lap2d:nx=1,ny=1", "lap2d:nx=129,ny=1"]                          # fp32-exact: one row, a slice and a row
THIRD = ["third:lap2d:nx=411,ny=203", "third:lap2d:nx=8192,ny=40", "third:lap3d:nx=128,ny=64,nz=21",
         "third:lap3d:nx=64,ny=64,nz=40"]
VARY = ["vary:411x203", "vary:8192x40"]
KERNEL_OPS = [GENERAL, POWERLAW] + FILES + ["edge"] + TINY
ALL_OPS = KERNEL_OPS + [POWERLAW_SELL, POWERLAW_SELL16] + THIRD + VARY + ["third:lap2d:nx=640,ny=100", "vary:640x100"]


# ---------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------
def _rowsum_ld(offs, cols, vals, x):
    """numpy longdouble row sums of vals[k] x[cols[k]]"""
    offs = np.asarray(offs, np.int64)
    prod = np.asarray(vals, np.longdouble) * np.asarray(x, np.longdouble)[np.asarray(cols, np.int64)]
    y = np.zeros(len(offs) - 1, np.longdouble)
    full = np.flatnonzero(np.diff(offs) > 0)
    if len(full):
        y[full] = np.add.reduceat(prod, offs[:-1][full])               # (empty rows have no entries: skipped)
    return y


def _reference(A, x):
    """S~ (as fp64), y_ref = S~ x in longdouble, the bound of _check_spmv on S~"""
    offs, cols = A.offs.astype(np.int64), A.cols.astype(np.int64)
    vt = A.vals.astype(np.float32).astype(np.float64)
    y_ref = _rowsum_ld(offs, cols, vt, x)
    bound = 4 * EPS * np.maximum(np.diff(offs), 1) * O.spmv(A.offs, A.cols, np.abs(vt), np.abs(x))
    return vt, y_ref, bound


def _check(y, y_ref, bound, what, worst=None):
    assert not np.isnan(y).any(), what
    err = np.abs(y.astype(np.longdouble) - y_ref).astype(np.float64)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    print("worst error / bound %-60s %.3f" % (what, ratio))
    if worst is not None:
        worst[0] = max(worst[0], ratio)
    over = np.flatnonzero(err > bound)
    assert not len(over), "%s: %d rows beyond the bound, first %d: error %.3e, bound %.3e" % (
        what, len(over), over[0], err[over[0]], bound[over[0]])


def _check_dot(dot, x, y_ref, what):
    xy = np.asarray(x[:len(y_ref)], np.longdouble) * y_ref
    assert abs(dot - float(xy.sum())) <= 1e-12 * max(float(np.abs(xy).sum()), 1e-300), what


# ---------------------------------------------------------------------------------------------------
# CPU: the reference and the inputs
# ---------------------------------------------------------------------------------------------------
def test_longdouble_reference_agrees_with_the_oracle(matrix_path):
    import lsbench_amd as hip
    assert np.finfo(np.longdouble).eps < EPS / 1000                      # x87 extended: 64-bit mantissa
    for name in ALL_OPS:
        A, ncol, _ = _op(hip, name, matrix_path)
        x = np.random.default_rng(1).standard_normal(ncol)
        vt, y_ref, bound = _reference(A, x)
        yo = O.spmv(A.offs, A.cols, vt, x)
        assert np.all(np.abs(yo - y_ref) <= 0.25 * bound), name
        assert np.all(y_ref[np.diff(A.offs.astype(np.int64)) == 0] == 0)


def test_unrounded_values_break_the_bound(matrix_path):
    """a condition on the inputs: wherever an operator is not declared fp32-exact, S x with the fp64 values
    is outside the bound around S~ x in more than half of the rows that hold an entry (an empty row is 0
    either way: the edge matrix has 8 of 16) -- a kernel that ignored fp32 would fail on every one of them"""
    import lsbench_amd as hip
    for name in ALL_OPS:
        A, ncol, exact = _op(hip, name, matrix_path)
        x = np.random.default_rng(2).standard_normal(ncol)
        vt, y_ref, bound = _reference(A, x)
        if exact:
            assert np.array_equal(vt, A.vals), name
            continue
        broken = int((np.abs(_rowsum_ld(A.offs, A.cols, A.vals, x) - y_ref) > bound).sum())
        filled = int((np.diff(A.offs.astype(np.int64)) > 0).sum())
        share = float((vt == A.vals).mean())
        print("%-50s fp32-exact values %5.1f %%, rows outside the bound with fp64 values %d of %d" % (
            name, 100 * share, broken, filled))
        assert 2 * broken > filled, name
        if name.startswith("vary"):
            assert 0.5 < share < 0.7                                     # the -1 and 4 of the grid are fp32 numbers
        elif name not in FILES and name != "edge" and "lap3d" not in name:   # (6 / 3 = 2: the 7-point diagonal stays exact)
            assert share < 0.01, name


def _layout(hip, name, period=0, kmax=8):
    """what the host builders make of the operator: kind-1 slots inside shaped templates, masks, untemplated
    slices that hold constant slots, slices inside a z-column plan"""
    lib = hip._lib.load()
    A = _op(hip, name)[0]
    H = lib.lsb_csr_sellize16(A.ptr, 0)
    V = lib.lsb_sell16_value_slots(H)
    T = lib.lsb_sell16_templates(H, V)
    out = dict(kind1=0, masks=0, untemplated_const=0, untemplated=0, in_cols=0, kept=int(V.contents.nval_slots))
    if T:
        t, ns = T.contents, T.contents.nslice
        tid = np.ctypeslib.as_array(t.tid, (ns,))
        for k in np.unique(tid[tid != 255]):
            q = t.t[int(k)]
            cnt = int((tid == k).sum())
            out["kind1"] += cnt * sum(1 for j in range(q.nslots) if q.kind[j] == 1 and q.shaped)
        out["masks"] = int(t.nmask)
        sp = np.ctypeslib.as_array(H.contents.sptr, (ns + 1,)) // hip.SELL_ROWS
        rec = np.ctypeslib.as_array(V.contents.slots, (V.contents.nslots * 4,)).reshape(-1, 4)
        for sl in np.flatnonzero(tid == 255):
            out["untemplated"] += 1
            out["untemplated_const"] += bool((rec[sp[sl]:sp[sl + 1], 2] < 0).any())
        if period:
            Cp = lib.lsb_sell_tmpl_columns(T, period, kmax)
            if Cp:
                out["in_cols"] = int(Cp.contents.in_cols)
                lib.lsb_tmpl_cols_free(Cp)
        lib.lsb_sell_tmpls_free(T)
    lib.lsb_sell_vc_free(V), lib.lsb_sell_free(H)
    return out


def test_operators_reach_the_paths_they_are_there_for(matrix_path):
    import lsbench_amd as hip
    for name in (POWERLAW, "edge"):                                      # the workgroup-per-row path
        assert np.diff(_op(hip, name, matrix_path)[0].offs.astype(np.int64)).max() > BLOCK_NNZ
    E = _op(hip, "edge")[0]
    assert (np.diff(E.offs.astype(np.int64)) == 0).sum() == 8
    for name, period in (("third:lap2d:nx=411,ny=203", 0), ("third:lap2d:nx=8192,ny=40", 64), ("third:lap2d:nx=640,ny=100", 0),
                         ("third:lap3d:nx=128,ny=64,nz=21", 64), ("third:lap3d:nx=64,ny=64,nz=40", 32)):
        lay = _layout(hip, name, period)
        print(name, lay)
        assert lay["kept"] == 0 or "lap3d" in name or lay["kind1"] == 0, name   # every value a constant or a mask
        assert lay["masks"] > 0 or "8192" in name, name                 # (whole-slice lines end on slice ends: no mask)
        assert lay["untemplated_const"] > 0, name                        # the slot-by-slot fall-back on constants
        assert (lay["in_cols"] > 0) == bool(period), name
    for name, period in (("vary:411x203", 0), ("vary:8192x40", 64), ("vary:640x100", 0)):
        lay = _layout(hip, name, period)
        print(name, lay)
        assert lay["kind1"] > 0 and lay["untemplated"] > 0 and lay["untemplated_const"] > 0, name
        assert lay["in_cols"] == 0, name                                 # a column's slots are constants or masks: no plan
    assert _layout(hip, GENERAL)["kept"] > 0 and _layout(hip, GENERAL)["kind1"] == 0   # general values: no template


# ---------------------------------------------------------------------------------------------------
# GPU, kernel level: lsb_hip_spmv_csr_f64 with LSB_SP_F32 and a float32 value array
# ---------------------------------------------------------------------------------------------------
def _launch(hip, variant, n, offs, cols, vals32, rowblk, blklanes, nblk, mean, flags, x, with_dot):
    import torch
    lib = hip._lib.load()
    assert vals32.dtype == torch.float32
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    w = torch.zeros(lib.lsb_hip_partials_capacity(), dtype=torch.float64, device="cuda:0")
    dot = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.lsb_hip_spmv_csr_f64(variant, n, p(offs), p(cols), p(vals32), p(rowblk), p(blklanes), nblk, mean,
                                  flags | F32, p(x), y.data_ptr(), p(x) if with_dot else None,
                                  dot.data_ptr() if with_dot else None, w.data_ptr(), lib.lsb_hip_stream())
    assert rc == 0
    lib.lsb_hip_sync()
    return y.cpu().numpy(), dot.item()


def _csr_f32(hip, A, x, variant, mean, flags, lanes, with_dot):
    rb = hip.lsb_csr_row_blocks(A, BLOCK_NNZ)
    bl = hip.lsb_csr_block_lanes(A, rb)
    return _launch(hip, variant, A.nrows, _dev(A.offs, np.int32), _dev(A.cols, np.int32), _dev(A.vals, np.float32),
                   _dev(rb, np.int32), _dev(bl) if lanes else None, len(rb) - 1, mean, flags, _dev(x), with_dot)


def _sell_f32(hip, A, x, flags, with_dot):
    sptr, cols, vals = hip.lsb_csr_sellize(A)
    pad = hip.SELL_ROWS                       # the kernel may read one slice row past the end
    return _launch(hip, hip.SPMV_SELL, A.nrows, _dev(sptr.astype(np.int32)),
                   _dev(np.concatenate([cols, np.zeros(pad, np.int32)])),
                   _dev(np.concatenate([vals, np.zeros(pad)]), np.float32), None, None, len(sptr) - 1, 0, flags,
                   _dev(x), with_dot)


def _sell16_f32(hip, A, x, flags, with_dot):
    out = hip.lsb_csr_sellize16(A)
    if out is None:
        return None
    sptr, codes, sbase, vals = out
    pad = hip.SELL_ROWS
    return _launch(hip, hip.SPMV_SELL, A.nrows, _dev(sptr.astype(np.int32)),
                   _dev(np.concatenate([codes, np.zeros(pad, np.int16)])),
                   _dev(np.concatenate([vals, np.zeros(pad)]), np.float32),
                   _dev(np.concatenate([sbase.ravel(), np.zeros(2, np.int32)])), None, len(sptr) - 1, 0,
                   flags | hip.SPMV_FLAG_C16, _dev(x), with_dot)


def _kernel_cases(hip, names, matrix_path, seed, run, what):
    """run(A, x, with_dot) -> (y, dot) or None on every operator, with and without the fused dot: the bound,
    the dot, exact zeros on empty rows.  Returns the operators that ran."""
    done, worst = [], [0.0]
    for name in names:
        A, ncol, _ = _op(hip, name, matrix_path)
        x = np.random.default_rng(seed).standard_normal(ncol)
        _, y_ref, bound = _reference(A, x)
        empty = np.diff(A.offs.astype(np.int64)) == 0
        for with_dot in (True, False):
            out = run(A, x, with_dot)
            if out is None:
                break
            _check(out[0], y_ref, bound, "%s %s dot=%d" % (what, name, with_dot), worst)
            assert np.all(out[0][empty] == 0) and not np.signbit(out[0][empty]).any(), name
            if with_dot:
                _check_dot(out[1], x, y_ref, name)
        else:
            done.append(name)
    print("WORST %-40s %.3f" % (what, worst[0]))
    return done


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [True, False])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_adaptive_f32_kernel(hip, flags, lanes, matrix_path):
    """k_spmv_adaptive<.., float>, its four flavours, lanes per block given or not; the power-law and edge operators
    hold rows beyond LSB_BLOCK_NNZ (the workgroup-per-row path)"""
    done = _kernel_cases(hip, KERNEL_OPS, matrix_path, 10 + flags,
                         lambda A, x, d: _csr_f32(hip, A, x, hip.SPMV_ADAPTIVE, 0, flags, lanes, d),
                         "adaptive<float> flags=%d lanes=%d" % (flags, lanes))
    assert done == KERNEL_OPS


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [2, 4, 8, 16, 32, 64])
def test_subwave_f32_kernel(hip, mean, matrix_path):
    """k_spmv_subwave<2..64, float>"""
    done = _kernel_cases(hip, KERNEL_OPS, matrix_path, 20 + mean,
                         lambda A, x, d: _csr_f32(hip, A, x, hip.SPMV_SUBWAVE, mean, 0, True, d),
                         "subwave<%d, float>" % mean)
    assert done == KERNEL_OPS


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 2])
def test_sell_f32_kernel(hip, flags, matrix_path):
    """k_spmv_sell<.., float> (32-bit columns); the power-law operator with rows of at most 512 entries, as in
    test_sell.py: a sliced-ELL copy pads every slice to its longest row"""
    names = [GENERAL, POWERLAW_SELL] + FILES + ["edge"] + TINY
    done = _kernel_cases(hip, names, matrix_path, 30 + flags, lambda A, x, d: _sell_f32(hip, A, x, flags, d),
                         "sell<float> flags=%d" % flags)
    assert done == names


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 2])
def test_sell16_f32_kernel(hip, flags, matrix_path):
    """k_spmv_sell16<.., float> (16-bit codes, every value stored).  Square operators only: the entry point
    gives the kernel xlen = n (the edge matrix gathers from 6000 columns into 16 rows); an operator the
    codes cannot hold has no such copy."""
    names = [GENERAL, POWERLAW_SELL16] + FILES + TINY + THIRD[:1] + VARY[:1]
    done = _kernel_cases(hip, names, matrix_path, 40 + flags, lambda A, x, d: _sell16_f32(hip, A, x, flags, d),
                         "sell16<float> flags=%d" % flags)
    assert done == names


# ---------------------------------------------------------------------------------------------------
# GPU, solver level: lsb_hip_solver_spmv_inner_dev
# ---------------------------------------------------------------------------------------------------
def _forms(hip):
    """(name, spmv_variant, spmv_tune, environment)"""
    S = hip.SPMV_SELL
    return [("subwave", hip.SPMV_SUBWAVE, -1, {}), ("adaptive", hip.SPMV_ADAPTIVE, -1, {}),
            ("sell32", S, 2, {}), ("sell16", S, 6, {}), ("sell16-all-values", S, 6, {"LSBENCH_HIP_NO_VCONST": "1"}),
            ("tmpl", S, 6 | 64, {}), ("tmpl-defer", S, 6 | 64 | 128, {}),
            ("col-3", S, 6 | 64 | 256, {"LSBENCH_HIP_COL_K": "3"}), ("col-8", S, 6 | 64 | 256, {"LSBENCH_HIP_COL_K": "8"})]


BASIC = {"subwave", "adaptive", "sell32", "sell16", "sell16-all-values"}
ENV = ("LSBENCH_HIP_NO_VCONST", "LSBENCH_HIP_COL_K", "LSBENCH_HIP_PAD_LINES")


def _case(hip, name):
    """the operator, S~ as an operator of its own, x, y_ref, the bound"""
    key = ("case", name)
    if key not in _cache:
        A = _op(hip, name)[0]
        x = np.random.default_rng(len(name)).standard_normal(A.nrows)
        vt, y_ref, bound = _reference(A, x)
        At = hip.Matrix.from_arrays(A.offs.copy(), A.cols.copy(), vt)
        _cache[key] = (A, At, x, y_ref, bound)
    return _cache[key]


def _inner(s, d_x, n, with_dot):
    import torch
    d_y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    d_dot = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda:0") if with_dot else None
    s.spmv_inner_dev(d_x, d_y, d_dot)
    return d_y.cpu().numpy(), (d_dot.item() if with_dot else None)


def _run_forms(hip, monkeypatch, name, forms, worst, nvirt=1, overlap=0, comm=0, **kw):
    """every form of `forms` on the operator, as a mixed-precision solver and as an fp64 solver on S~; returns
    the forms that ran (a form the solver reports as absent for this operator is left out)"""
    import torch
    A, At, x, y_ref, bound = _case(hip, name)
    d_x = torch.from_numpy(x).to("cuda:0")
    ran, bytes16 = set(), None
    for form, variant, tune, env in forms:
        for k in ENV[:2]:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        what = "%s %s nvirt=%d overlap=%d comm=%d %s" % (form, name, nvirt, overlap, comm, kw or "")
        out = {}
        for prec, M in ((hip.PREC_MIXED, A), (hip.PREC_FP64, At)):
            s = hip.Solver(M, hip.default_opts(op_mode=hip.OP_RAW, precision=prec, use_graph=0, spmv_variant=variant,
                                               spmv_tune=tune, nvirt=nvirt, overlap=overlap, comm=comm, **kw))
            # the form, as the solver reports it
            assert s.spmv_variant == variant, what
            split = bool(s.overlaps)
            if variant == hip.SPMV_SELL:
                assert s.spmv_flags == tune and split == bool(overlap), what
                kept, total = s.sell_value_slots
                if form == "sell32":
                    assert total == 0, what
                elif not kw.get("reorder"):
                    assert total > 0 and (form != "sell16-all-values" or kept == total), what
                lb = s.spmv_layout_bytes
                if form == "sell16":
                    bytes16 = lb
                absent = (form.startswith("tmpl") and lb == bytes16) or (form.startswith("col") and not s.spmv_col_slices)
                if absent:
                    s.destroy()
                    break
            elif variant == hip.SPMV_ADAPTIVE:
                assert split == bool(overlap), what
            else:
                assert not split, what                                   # the sub-wavefront form has no split
            one = nvirt == 1
            y, dot = _inner(s, d_x, A.nrows, one)
            y2, dot2 = _inner(s, d_x, A.nrows, one)
            assert np.array_equal(y, y2) and dot == dot2, what          # run to run: the same bits
            if prec == hip.PREC_FP64:                                    # fp64: the inner product IS the exact one
                d_y = torch.full((A.nrows,), float("nan"), dtype=torch.float64, device="cuda:0")
                s.spmv_dev(d_x, d_y)
                assert np.array_equal(d_y.cpu().numpy(), y), what + " (fp64: spmv_dev against spmv_inner_dev)"
            s.destroy()
            _check(y, y_ref, bound, what + (" mixed" if prec == hip.PREC_MIXED else " fp64 on S~"), worst.setdefault(form, [0.0]))
            if one:
                _check_dot(dot, x, y_ref, what)
            out[prec] = y
        else:
            # lossless layouts, the same products in the same order: fp32 values or S~ in fp64, the same bits
            diff = np.flatnonzero(out[hip.PREC_MIXED] != out[hip.PREC_FP64])
            assert not len(diff), "%s: %d rows differ in bits from the fp64 solver on S~, first %d" % (what, len(diff), diff[0])
            ran.add(form)
    for k in ENV[:2]:
        monkeypatch.delenv(k, raising=False)
    return ran


def _expected(name, nvirt):
    want = set(BASIC)
    if nvirt == 1 and (name.startswith("third") or name.startswith("vary")):
        want |= {"tmpl", "tmpl-defer"}
        if name.startswith("third") and ("8192" in name or "lap3d" in name):
            want |= {"col-3", "col-8"}
    return want


SHARDS = [(1, 0, 0)] + [(nv, ov, cm) for nv in (2, 3) for ov in (0, 1) for cm in (1, 2)]
SOLVER_OPS = [GENERAL] + THIRD + VARY


@pytest.mark.gpu
@pytest.mark.parametrize("nvirt,overlap,comm", SHARDS)
@pytest.mark.parametrize("name", SOLVER_OPS)
def test_inner_product_of_a_mixed_solver_is_fp32_of_s(hip, monkeypatch, name, nvirt, overlap, comm):
    """Every SpMV form a mixed-precision solver can run, forced as in test_sell.py, over one shard and over 2 and
    3 row-range shards (cut inside a grid line or plane), behind the exchange and split around it, over device
    copies and the direct path: y = S~ x inside the bound, the fused dot on one shard, the same bits run to run,
    and the bits of an fp64 solver built on S~ in the same form (for which spmv_inner_dev and spmv_dev agree
    bit for bit, split launches included).  Worst error / bound per form: DESIGN.md, mixed-precision section."""
    worst = {}
    ran = _run_forms(hip, monkeypatch, name, _forms(hip), worst, nvirt, overlap, comm)
    for form in sorted(worst):
        print("WORST %-20s %-40s %.3f" % (form, name, worst[form][0]))
    print("RAN %s nvirt=%d overlap=%d comm=%d: %s" % (name, nvirt, overlap, comm, sorted(ran)))
    assert ran >= _expected(name, nvirt), sorted(_expected(name, nvirt) - ran)


@pytest.mark.gpu
def test_inner_product_of_a_reordered_and_of_a_line_padded_solver(hip, monkeypatch):
    """the gather / scatter of spmv_dev: rows renumbered by reverse Cuthill-McKee (reorder = 1), grid lines
    padded to whole slices (LSBENCH_HIP_PAD_LINES=1: the padded copy has a z-column plan along y)"""
    worst = {}
    forms = [f for f in _forms(hip) if f[0] in ("subwave", "adaptive", "sell32", "sell16")]
    for nvirt, overlap, comm in ((1, 0, 0), (3, 1, 1)):
        ran = _run_forms(hip, monkeypatch, GENERAL, forms, worst, nvirt, overlap, comm, reorder=1)
        assert ran == {f[0] for f in forms}
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1")
    name = "third:lap2d:nx=2050,ny=61"
    s = hip.Solver(_op(hip, name)[0], hip.default_opts(op_mode=hip.OP_RAW, precision=hip.PREC_MIXED, use_graph=0))
    assert s.padded > 0
    s.destroy()
    forms = [f for f in _forms(hip) if f[0] in ("adaptive", "sell16", "tmpl", "tmpl-defer", "col-8")]
    for nvirt, overlap, comm in ((1, 0, 0), (3, 1, 1)):
        ran = _run_forms(hip, monkeypatch, name, forms, worst, nvirt, overlap, comm)
        assert ran >= {f[0] for f in forms} - ({"col-8"} if nvirt > 1 else set())   # (a third of 61 lines may hold no plan)
    for form in sorted(worst):
        print("WORST %-20s %-40s %.3f" % (form, "re-ordered / line-padded", worst[form][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["MIXED", "FP64"])
def test_a_solve_after_the_inner_product_is_a_fresh_solvers_solve(hip, monkeypatch, precision):
    """spmv_inner_dev writes the gather vector, q, the dot partials and clears the device status: nothing a
    solve does not set itself -- x, iterations, corrections and residual of a fresh solver, bit for bit"""
    import torch
    monkeypatch.setenv("LSBENCH_HIP_COL_K", "8")
    S, AD = hip.SPMV_SELL, hip.SPMV_ADAPTIVE
    for name, kw in (("third:lap2d:nx=411,ny=203", dict(spmv_variant=S, spmv_tune=6 | 64)),
                     ("third:lap2d:nx=8192,ny=40", dict(spmv_variant=S, spmv_tune=6 | 64 | 256)),
                     ("vary:411x203", dict(spmv_variant=AD, nvirt=3, overlap=1, comm=1)),
                     ("vary:411x203", dict(spmv_variant=S, spmv_tune=6 | 64, nvirt=2, overlap=1, comm=2))):
        A, At, x, y_ref, bound = _case(hip, name)
        b = O.rhs(A.nrows)
        got = []
        for touch in (0, 1):
            s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, precision=getattr(hip, "PREC_" + precision), tol=1e-10,
                                               use_graph=0, **kw))
            if touch:
                _inner(s, torch.from_numpy(x).to("cuda:0"), A.nrows, kw.get("nvirt", 1) == 1)
            xs, r = s.solve(b)
            s.destroy()
            assert r.status == hip.STATUS_CONVERGED, (name, kw)
            got.append((xs, int(r.iters), int(r.corrections), r.relres))
        assert np.array_equal(got[0][0], got[1][0]) and got[0][1:] == got[1][1:], (name, kw)


@pytest.mark.gpu
def test_inner_product_refusals(hip):
    import torch
    lib = hip._lib.load()
    A = _op(hip, GENERAL)[0]
    d = torch.zeros(A.nrows, dtype=torch.float64, device="cuda:0")
    one = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, precision=hip.PREC_MIXED))
    assert lib.lsb_hip_solver_spmv_inner_dev(None, d.data_ptr(), d.data_ptr(), None) == 2
    assert lib.lsb_hip_solver_spmv_inner_dev(s._h, None, d.data_ptr(), None) == 2
    assert lib.lsb_hip_solver_spmv_inner_dev(s._h, d.data_ptr(), None, None) == 2
    y = torch.zeros_like(d)
    assert lib.lsb_hip_solver_spmv_inner_dev(s._h, d.data_ptr(), y.data_ptr(), one.data_ptr()) == 0
    s.destroy()
    s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, precision=hip.PREC_MIXED, nvirt=2, comm=1))
    assert lib.lsb_hip_solver_spmv_inner_dev(s._h, d.data_ptr(), y.data_ptr(), one.data_ptr()) == 2   # a dot over shards
    assert lib.lsb_hip_solver_spmv_inner_dev(s._h, d.data_ptr(), y.data_ptr(), None) == 0
    s.destroy()
