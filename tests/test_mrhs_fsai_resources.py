"""Compile-time guard for the two row kernels of FSAI on blocks of right-hand sides (no GPU needed: hipcc
cross-compiles gfx950), in the manner of test_mrhs_amg_resources.py: nothing in hip_mrhs_fsai.hip spills and the file
holds the expected instantiations -- 6 lane counts x 3 widths of k_mrhs_fsai_xr_gr and of k_mrhs_fsai_gt_dots -- and
nothing else.  It has no streaming kernel: the sweeps around the two launches are hip_mrhs.hip's and are held to 64
VGPRs at occupancy 8 there.  It looks at these resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
LANES, WIDTHS = (2, 4, 8, 16, 32, 64), (2, 4, 8)
KERNELS = ("k_mrhs_fsai_xr_gr", "k_mrhs_fsai_gt_dots")

# The row kernels as found: kernel -> width -> ((VGPRs for L = 2, 4, 8, 16, 32, 64), (waves per SIMD likewise)).
# Recorded and printed beside what the compiler reports now, not a target: a lane of k_mrhs_fsai_xr_gr keeps up to 2 KP
# gathered operands (q and r of row `col`) and KP sums in flight, k_mrhs_fsai_gt_dots KP gathered operands, KP sums and
# the 2 KP running sums of its record.  Whether fewer registers would pay has not been measured.
FOUND = {
    "k_mrhs_fsai_xr_gr": {2: ((32, 34, 34, 36, 36, 38), (8, 8, 8, 8, 8, 8)),
                          4: ((44, 46, 46, 44, 44, 46), (8, 8, 8, 8, 8, 8)),
                          8: ((64, 64, 64, 66, 66, 68), (8, 8, 8, 7, 7, 7))},
    "k_mrhs_fsai_gt_dots": {2: ((36, 36, 38, 38, 40, 40), (8, 8, 8, 8, 8, 8)),
                            4: ((56, 56, 58, 58, 60, 60), (8, 8, 8, 8, 8, 8)),
                            8: ((90, 90, 92, 92, 94, 94), (5, 5, 5, 5, 5, 5))},
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_mrhs_fsai_kernels_have_no_spills_and_the_expected_instantiations(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_mrhs_fsai.hip"), "-o", str(tmp_path / "hip_mrhs_fsai.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    info, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            assert name not in info, name
            info[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            info[name][m.group(1).strip()] = int(m.group(2))
    rows = {}
    for k, v in info.items():
        m = re.search(r"(k_mrhs_fsai_xr_gr|k_mrhs_fsai_gt_dots)ILi(\d+)ELi(\d+)E", k)
        assert m, k  # nothing else lives in the file
        rows[(m.group(1), int(m.group(2)), int(m.group(3)))] = (v["VGPRs"], v["Occupancy"])
    assert len(info) == 36
    assert sorted(rows) == sorted((kn, L, kp) for kn in KERNELS for L in LANES for kp in WIDTHS)  # 18 each
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    print("row kernels, (kernel, KP): recorded (VGPRs L = 2 .. 64), (occupancy) | now")
    for kn in KERNELS:
        for kp in WIDTHS:
            now = (tuple(rows[(kn, L, kp)][0] for L in LANES), tuple(rows[(kn, L, kp)][1] for L in LANES))
            print("  ", kn, kp, FOUND[kn][kp], "|", now)
