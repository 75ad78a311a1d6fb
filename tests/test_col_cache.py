"""The two-launch PCG iteration's vectors in one slab, and k_pcg_col_r walking each XCD's band of the
z-column plan from its END (rev = 1: every launch of an iteration starts on the lines the launch before
touched last).  The reversed turn loop takes group G - 1 - j where the ascending one takes j, with
G = ceil(items of the band / 4): the shapes below are where that can go wrong -- few groups per XCD, G no
multiple of the grid, a band whose item count is no multiple of 4, more turns than one (spmv_grid 8 and 16:
one and two workgroups per XCD) and fewer groups than workgroups (spmv_grid 0, the resident grid).  Every
row's r' keeps its bits; only the order of a thread's terms of (r.z, r.r) follows the turns, so the checks
are those of test_col_direction.py: the oracle's PCG, bit-identical repeats, and runs cut by maxit against
the three-launch form."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
TUNE = 6 | 64 | 256                                    # 16-bit codes, templates, the z-column walk

PADDED = [("lap2d:nx=1000,ny=60", 5),                   # 12 z-groups of 5 lines
          ("lap2d:nx=1000,ny=63", 5),                   # 13 of 4 and 5
          ("lap2d:nx=1000,ny=77", 3),                   # 26 of 2 and 3
          ("lap2d:nx=2050,ny=61", 4)]                   # 17 slices a line, 16 z-groups
SHAPES = PADDED + [("lap3d:nx=128,ny=64,nz=21", 0)]     # two far slots per side, unpadded (0: the default column length)
GRIDS = [8, 16, 0]


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
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("spec,kmax", SHAPES)
def test_reversed_r_launch_solves_and_repeats(hip, monkeypatch, spec, kmax, grid):
    _env(monkeypatch, kmax)
    A, b, xo, ito = _reference(spec)
    padded = (spec, kmax) in PADDED
    s = hip.Solver(A, _opts(hip, grid, use_graph=0))
    assert s.fused_p == 2 and bool(s.padded) == padded
    if grid:
        assert s.spmv_grid == grid
    # the slab: r, both direction buffers, and a padded solver's x (b too) in shard 0's one allocation
    assert s.slab_mask & 0b111 == 0b111
    if padded:
        assert s.slab_mask & 0b1111 == 0b1111 and s.slab_mask & 0b10000
    x, r = s.solve(b)
    x2, r2 = s.solve(b)
    s.destroy()
    assert np.array_equal(x, x2) and r.iters == r2.iters and r.relres == r2.relres
    assert r.status == hip.STATUS_CONVERGED and abs(int(r.iters) - ito) <= 2
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("spec,kmax", SHAPES)
def test_reversed_r_launch_agrees_with_three_launches_cut_by_maxit(hip, monkeypatch, spec, kmax, grid):
    """the same iterates up to the order of the dots' terms: 1e-12, the same count and status"""
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


@pytest.mark.gpu
def test_unpadded_one_shard_jacobi_solver_has_its_directions_in_the_slab(hip, monkeypatch):
    """whatever form it runs: the second direction buffer is counted and carved at upload"""
    monkeypatch.setenv("LSBENCH_HIP_PAD_LINES", "0")
    A, b, xo, ito = _reference("lap2d:nx=1000,ny=60")
    s = hip.Solver(A, hip.default_opts(op_mode=hip.OP_RAW, tol=1e-10))
    assert not s.padded and s.slab_mask & 0b111 == 0b111 and not s.slab_mask & 0b11000
    x, r = s.solve(b)
    s.destroy()
    assert r.status == hip.STATUS_CONVERGED and np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_two_launch_kernels_keep_their_registers(tmp_path):
    """the kernels that ship (k_pcg_col_r with its turn order as an argument): no scratch; one far slot per
    side <= 96 VGPRs and five waves per SIMD, two far slots three"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_kernels.hip"), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    info, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            info[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            info[name][m.group(1).strip()] = int(m.group(2))
    ks = {k: v for k, v in info.items() if "k_pcg_col_r" in k or "k_pcg_col_px" in k}
    assert sum("k_pcg_col_r" in k for k in ks) == 2 and sum("k_pcg_col_px" in k for k in ks) >= 4
    for k, v in ks.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
        if re.search(r"ILi1E", k):                      # NF = 1
            assert v["VGPRs"] <= 96 and v["Occupancy"] >= 5, (k, v)
        else:
            assert v["Occupancy"] >= 3, (k, v)
