"""The fixed cost of the two-launch PCG iteration's launches (k_pcg_col_px + k_pcg_col_r): their streamed results
written through the L2 (slice_store16: one buffer resource per slice and store, in both walk directions, p' and x
of k_pcg_col_px and r' of k_pcg_col_r), and the partial sums of the launch before asked for in one batch
(wg_sum_parts: the terms in wg_sum_partials' order, so the same bits).  Neither may change a bit of any row, nor the
order of a dot's terms: the checks are test_col_cache.py's, on shapes where a store's slice address or a batch of
records can go wrong -- bands of 3 to 14 groups of four against one, two and three workgroups per XCD (spmv_grid 8,
16, 24: 8 to 24 partial records, far short of one batch of 1280, and a last group that is not full where the band's
item count is no multiple of 4), fewer groups than workgroups (spmv_grid 0, the resident grid: 1280 or 768 records,
one whole batch or three fifths of one, and a run's first sums from the init sweep's grid), columns of 4 and 5
slices walked up and down, 17 slices a line, and two far slots per side."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

TUNE = 6 | 64 | 256                                    # 16-bit codes, templates, the z-column walk

# (operator, column length (0: the default), spmv_grid): groups of four per XCD band, from the plan builder
CASES = [("lap2d:nx=1000,ny=60", 5, 16),               # G = 5,3,3,3,3,3,3,5: two workgroups per XCD, odd group counts
         ("lap2d:nx=1000,ny=60", 5, 8),                # one workgroup per XCD walks every group
         ("lap2d:nx=1000,ny=60", 5, 24),               # three: G = 5 leaves two groups over, G = 3 none
         ("lap2d:nx=1000,ny=60", 5, 0),                # the resident grid: fewer groups than workgroups
         ("lap2d:nx=1000,ny=63", 5, 16),               # G = 6,3,4,4,4,3,4,5; bands of 23, 13, 14 items: a last group
         ("lap2d:nx=1000,ny=63", 5, 24),               # that is not full, first in the reversed launch
         ("lap2d:nx=2050,ny=61", 4, 16),               # G = 14,9,9,9,8,10,8,13, 17 slices a line
         ("lap2d:nx=2050,ny=61", 4, 24),
         ("lap3d:nx=128,ny=64,nz=21", 0, 8),           # two far slots per side, unpadded
         ("lap3d:nx=128,ny=64,nz=21", 0, 16)]


@functools.lru_cache(maxsize=None)
def _reference(spec):
    """the operator, b and the oracle's Jacobi-PCG solve at 1e-10: computed once per shape, never changed"""
    import lsbench_amd as la
    A = la.lsbench_matrix_synth(spec)
    b = O.rhs(A.nrows)
    xo, ito, relo, sto = O.pcg_jacobi(A.offs, A.cols, A.vals, b, 1e-10)
    xo.setflags(write=False), b.setflags(write=False)
    return A, b, xo, ito


def _env(monkeypatch, kmax):
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "1")
    if kmax:
        monkeypatch.setenv("LSBENCH_HIP_COL_K", str(kmax))
    else:
        monkeypatch.delenv("LSBENCH_HIP_COL_K", raising=False)


def _opts(hip, grid, **kw):
    return hip.default_opts(op_mode=hip.OP_RAW, spmv_variant=hip.SPMV_SELL, tol=1e-10, spmv_tune=TUNE,
                            spmv_grid=grid, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("spec,kmax,grid", CASES)
def test_two_launch_form_solves_and_repeats(hip, monkeypatch, spec, kmax, grid):
    _env(monkeypatch, kmax)
    A, b, xo, ito = _reference(spec)
    s = hip.Solver(A, _opts(hip, grid, use_graph=0))
    assert s.fused_p == 2
    if grid:
        assert s.spmv_grid == grid
    x, r = s.solve(b)
    x2, r2 = s.solve(b)
    s.destroy()
    assert np.array_equal(x, x2) and r.iters == r2.iters and r.relres == r2.relres
    assert r.status == hip.STATUS_CONVERGED and abs(int(r.iters) - ito) <= 2
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)


@pytest.mark.gpu
@pytest.mark.parametrize("spec,kmax,grid", CASES)
def test_two_launch_form_agrees_with_three_launches_cut_by_maxit(hip, monkeypatch, spec, kmax, grid):
    """the same iterates up to the order of the dots' terms: 1e-12, the same count and status; the odd cuts
    replay a captured graph"""
    _env(monkeypatch, kmax)
    A, b, xo, ito = _reference(spec)
    for maxit in range(1, 9):
        got = {}
        for fused in (1, 0):
            if fused:
                monkeypatch.delenv("LSBENCH_HIP_NO_FUSE_PX", raising=False)
            else:
                monkeypatch.setenv("LSBENCH_HIP_NO_FUSE_PX", "1")
            s = hip.Solver(A, _opts(hip, grid, use_graph=maxit % 2, maxit=maxit))
            assert s.fused_p == (2 if fused else 0)
            x, r = s.solve(b)
            x2, r2 = s.solve(b)
            s.destroy()
            assert np.array_equal(x, x2) and r.iters == r2.iters
            assert r.status == hip.STATUS_MAXIT and r.iters == maxit
            got[fused] = x
        assert np.linalg.norm(got[1] - got[0]) <= 1e-12 * np.linalg.norm(got[0]), maxit
