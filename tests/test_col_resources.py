"""Compile-time guard for the two-launch PCG iteration's kernels (no GPU needed: hipcc cross-compiles
gfx950).  k_pcg_col_px and k_pcg_col_r are launched with every workgroup resident
(LSB_TMPL_COL_GRID: 1280 with one far slot per side, 768 with two = 5 and 3 workgroups of four
waves per CU on 256 CUs), and the plan's walk directions are dealt against that grid.  A kernel
that needs more registers than that occupancy allows leaves part of the grid for a second wave
(k_pcg_col_px<1, 3, true> once needed 102 VGPRs: four workgroups per CU, the last fifth of the
grid ran behind the rest), and a spill costs far more.  Both directions of the column walk are
compiled into these kernels, so their register counts are watched here."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
CUS = 256
GRID = {1: 1280, 2: 768}   # LSB_TMPL_COL_GRID(nfar), include/lsbench_hip.h


def _resources(tmp_path):
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
    return info


def _grid_cap(src, launcher):
    """the resident grid a launcher caps its launch at, read from its source"""
    body = src[src.index("void " + launcher + "("):]
    body = body[:body.index("\n}\n")]
    return body


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_two_launch_kernels_fit_their_resident_grid(tmp_path):
    info = _resources(tmp_path)
    px = {k: v for k, v in info.items() if "k_pcg_col_px" in k}
    colr = {k: v for k, v in info.items() if "k_pcg_col_r" in k}
    assert len(px) == 4 and len(colr) == 2      # {1, 2} far slots x {with, without x}; {1, 2} far slots
    for k, v in list(px.items()) + list(colr.items()):
        nf = 1 if re.search(r"ILi1E", k) else 2
        grid = GRID[nf] if "k_pcg_col_px" in k else GRID[1]
        per_cu = grid // CUS                     # workgroups of 4 waves = waves per SIMD
        assert v["ScratchSize"] == 0, (k, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)
        assert v["Occupancy"] >= per_cu, (k, v)  # every workgroup of the grid resident at once
        assert v["VGPRs"] <= 512 // per_cu // 8 * 8, (k, v)
        assert v["LDS Size"] * per_cu <= 160 * 1024, (k, v)
        assert v["LDS Size"] <= 16 * 1024 + 256, (k, v)   # the partial sums' reduction; nothing else staged
    # the z-column SpMV shares the walk: registers only, nothing promoted to LDS
    for k, v in info.items():
        if "k_spmv_tmpl_col" in k:
            assert v["ScratchSize"] == 0 and v["LDS Size"] <= 192 and v["Occupancy"] >= 5, (k, v)


def test_launch_bounds_and_header_grid_caps_agree():
    """the occupancy the kernels promise the compiler is the one their launchers cap the grid at: both
    launchers take the cap from LSB_TMPL_COL_GRID, which the header pins to GRID, and spell no grid of
    their own"""
    with open(os.path.join(CSRC, "hip_kernels.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "include", "lsbench_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"#define LSB_TMPL_COL_GRID\(nfar\) \(\(nfar\) >= 2 \? (\d+)u : (\d+)u\)", hdr)
    assert m and (int(m.group(2)), int(m.group(1))) == (GRID[1], GRID[2])
    m = re.search(r"__launch_bounds__\(WG, NF == 2 \? (\d) : (\d)\) void k_pcg_col_px\(", src)
    assert m and int(m.group(1)) * CUS == GRID[2] and int(m.group(2)) * CUS == GRID[1]
    m = re.search(r"__launch_bounds__\(WG, (\d)\) void k_pcg_col_r\(", src)
    assert m and int(m.group(1)) * CUS == GRID[1]
    assert "LSB_TMPL_COL_GRID(nfar)" in _grid_cap(src, "lsb_k_pcg_col_px")
    assert "LSB_TMPL_COL_GRID(1)" in _grid_cap(src, "lsb_k_pcg_col_r")   # pinned to GRID[1] above
    for launcher in ("lsb_k_pcg_col_px", "lsb_k_pcg_col_r"):
        assert not re.search(r"\b(%d|%d)u?\b" % (GRID[1], GRID[2]), _grid_cap(src, launcher)), launcher
