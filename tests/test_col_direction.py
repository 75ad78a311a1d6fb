"""Walk directions of the z-column plan (include/lsbench_hip.h, struct lsb_tmpl_cols.down): where a
z-group and its neighbours go through the chip in one turn of the workgroups, the z-groups of odd
index are walked from their top plane down, so that two neighbouring columns ask for the plane they
share at the same step.  The items are the same either way; every row's products keep their order,
so y, q, p' and x come out the same bits -- only the dot partials add their terms in another order."""
import ctypes as C

import numpy as np
import pytest

import lsbench_amd as la
from oracle import oracle as O

TURN = {1: 4 * 1280 // 8, 2: 4 * 768 // 8}   # LSB_TMPL_COL_TURN(nfar): items an XCD takes per turn


def _zgroup(s, period, kmax, ns):
    npl = -(-ns // period)
    ng = -(-npl // kmax)
    z = s // period
    return ((z + 1) * ng - 1) // npl


def _plan(lib, P, period, kmax):
    H = lib.lsb_csr_sellize16(P, 0)
    V = lib.lsb_sell16_value_slots(H)
    T = lib.lsb_sell16_templates(H, V)
    assert T
    return H, V, T, lib.lsb_sell_tmpl_columns(T, period, kmax)


@pytest.mark.parametrize("kmax", [3, 5, 8])
def test_directions_alternate_by_z_group_on_a_padded_2d_grid(kmax):
    lib = la._lib.load()
    why = C.create_string_buffer(256)
    for ny in (60, 63):                                         # z-groups of equal and of unequal length
        A = la.lsbench_matrix_synth("lap2d:nx=1000,ny=%d" % ny)
        nx, nxp = C.c_uint(0), C.c_uint(0)
        mp = C.POINTER(C.c_int)()
        P = lib.lsb_csr_pad_lines(A.ptr, 128, C.byref(nx), C.byref(nxp), C.byref(mp))
        assert P and nxp.value == 1024
        period = 8                                              # a grid line = 8 slices
        H, V, T, Cp = _plan(lib, P, period, kmax)
        assert Cp and T.contents.nfar == 1 and 2 * period <= TURN[1]
        c = Cp.contents
        ns = T.contents.nslice
        assert lib.lsb_tmpl_cols_check(T, Cp, why, 256) == 0, why.value
        assert c.down                                           # the deal allows it: alternation on
        it = np.ctypeslib.as_array(c.item, (4 * c.nitem,)).reshape(-1, 4)
        bits = np.ctypeslib.as_array(c.down, ((c.nitem + 31) // 32,))
        down = np.array([(int(bits[i // 32]) >> (i % 32)) & 1 for i in range(c.nitem)])
        zg = np.array([_zgroup(int(s), period, kmax, ns) for s in it[:, 0]])
        runs = it[:, 1] & 0x7fffffff
        # odd z-groups walk down -- columns of >= 3 slices: the PCG kernels take shorter items slice by slice,
        # upward, and a run's first p.q (the z-column SpMV) must add its terms in their order
        assert np.array_equal(down, (zg & 1) * (runs >= 3))
        assert down.any() and not down.all()
        # the items are those of an upward plan: item[0] the lowest slice, item[1] & 0x7fffffff the length
        assert np.all(it[:, 0] // period * period + it[:, 0] % period == it[:, 0])
        # a flipped direction is caught, on a column and on a single slice alike
        for i in (int(np.argmax(runs >= 3)), int(np.argmin(runs))):
            keep = int(bits[i // 32])
            c.down[i // 32] = keep ^ (1 << (i % 32))
            assert lib.lsb_tmpl_cols_check(T, Cp, why, 256) == 13 and b"walk" in why.value
            c.down[i // 32] = keep
        assert lib.lsb_tmpl_cols_check(T, Cp, why, 256) == 0
        lib.lsb_tmpl_cols_free(Cp), lib.lsb_sell_tmpls_free(T), lib.lsb_sell_vc_free(V), lib.lsb_sell_free(H)
        la._lib.libc_free(mp)
        lib.lsb_csr_free(P)


def test_no_directions_where_a_z_group_spans_turns():
    """a 3-D grid whose plane is 200 slices (two far slots: 384 items per XCD and turn) keeps today's
    upward plan, like config 4's 1250-slice planes; a small plane alternates"""
    lib = la._lib.load()
    why = C.create_string_buffer(256)
    for spec, period, alt in (("lap3d:nx=128,ny=200,nz=21", 200, False), ("lap3d:nx=128,ny=64,nz=21", 64, True)):
        A = la.lsbench_matrix_synth(spec)
        H, V, T, Cp = _plan(lib, A.ptr, period, 4)
        assert Cp and T.contents.nfar == 2
        assert (2 * period <= TURN[2]) == alt
        assert bool(Cp.contents.down) == alt
        assert lib.lsb_tmpl_cols_check(T, Cp, why, 256) == 0, why.value
        if not alt:                                            # bits on a plan the deal does not allow: refused
            nw = (Cp.contents.nitem + 31) // 32
            buf = (C.c_uint * nw)()
            Cp.contents.down = C.cast(buf, C.POINTER(C.c_uint))
            assert lib.lsb_tmpl_cols_check(T, Cp, why, 256) == 13
            Cp.contents.down = C.POINTER(C.c_uint)()
        lib.lsb_tmpl_cols_free(Cp), lib.lsb_sell_tmpls_free(T), lib.lsb_sell_vc_free(V), lib.lsb_sell_free(H)


@pytest.mark.gpu
@pytest.mark.parametrize("spec,kmax", [("lap2d:nx=1000,ny=60", 5),    # 12 z-groups of 5 lines
                                       ("lap2d:nx=1000,ny=63", 5),    # 13 of 4 and 5
                                       ("lap2d:nx=1000,ny=77", 3),    # 26 of 2 and 3
                                       ("lap2d:nx=2050,ny=61", 4)])   # 17 slices a line, 16 z-groups
def test_two_launch_iteration_on_alternating_columns(hip, monkeypatch, spec, kmax):
    """padded 2-D grids (LSBENCH_HIP_PAD_LINES=1) walked with alternating directions: the z-column SpMV
    gives y bit for bit as k_spmv_tmpl; the two-launch iteration (fused_p = 2) matches the oracle's
    PCG, repeats bit for bit, and runs cut by maxit 1..8 agree with the three-launch form to rounding
    (the same iteration count and status; x of the very same iterates up to the dots' order)"""
    import torch
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1")
    monkeypatch.setenv("LSBENCH_HIP_COL_K", str(kmax))
    A = hip.lsbench_matrix_synth(spec)
    b = O.rhs(A.nrows)
    xs = np.sin(np.arange(A.nrows, dtype=np.float64))
    xo, ito, relo, sto = O.pcg_jacobi(A.offs, A.cols, A.vals, b, 1e-10)
    ys = {}
    for name, tune in (("tmpl", 6 | 64), ("col", 6 | 64 | 256)):
        s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, spmv_variant=hip.SPMV_SELL, tol=1e-10,
                                           spmv_tune=tune, use_graph=0))
        assert s.padded and s.spmv_flags == tune and s.spmv_col_slices > 0    # the plan exists either way
        d_y = torch.full((A.nrows,), float("nan"), dtype=torch.float64, device="cuda:0")
        s.spmv_dev(torch.from_numpy(xs).to("cuda:0"), d_y)
        ys[name] = d_y.cpu().numpy()
        if name == "col":
            assert s.fused_p == 2
            x, r = s.solve(b)
            x2, r2 = s.solve(b)
            assert np.array_equal(x, x2) and r.iters == r2.iters and r.relres == r2.relres
            assert r.status == hip.STATUS_CONVERGED and abs(int(r.iters) - ito) <= 2
            assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
        s.destroy()
    assert np.array_equal(ys["tmpl"], ys["col"])
    for maxit in range(1, 9):
        got = {}
        for fused in (1, 0):
            if fused:
                monkeypatch.delenv("LSBENCH_HIP_NO_FUSE_PX", raising=False)
            else:
                monkeypatch.setenv("LSBENCH_HIP_NO_FUSE_PX", "1")
            s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, spmv_variant=hip.SPMV_SELL, tol=1e-10,
                                               spmv_tune=6 | 64 | 256, use_graph=maxit % 2, maxit=maxit))
            assert s.fused_p == (2 if fused else 0)
            x, r = s.solve(b)
            x2, r2 = s.solve(b)
            assert np.array_equal(x, x2) and r.iters == r2.iters
            s.destroy()
            assert r.status == hip.STATUS_MAXIT and r.iters == maxit
            got[fused] = x
        assert np.linalg.norm(got[1] - got[0]) <= 1e-12 * np.linalg.norm(got[0]), maxit
