"""Compile-time guard for the kernels of the AMG V-cycle's Chebyshev smoother (no GPU needed: hipcc cross-compiles
gfx950), in the manner of test_mrhs_amg_resources.py: nothing in hip_amg_cheb.hip and none of the new kernels of
hip_amg.hip spills, the element-wise first step is within 64 VGPRs, and the expected instantiations are there.  It
looks at these resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
LANES, WIDTHS = (2, 4, 8, 16, 32, 64), (2, 4, 8)

# The row kernels as found: form -> width -> ((VGPRs from L = 2 to L = 64), (waves per SIMD likewise)); width 1 is
# the single-column k_amg_cheb of hip_amg.hip.  Recorded and printed beside what the compiler reports now, not a
# target and not tuned: a step keeps what hip_mrhs_amg.hip's sweep keeps plus the direction pair and the two
# coefficients (4-6 registers more than its 32-38 / 40-46 / 56-62); the step with records runs once per
# iteration, on the fine level, as the sweep with records does (42-52 / 60-70 / 92-104 there).
FOUND = {
    "step": {1: ((22, 26), (8, 8)), 2: ((32, 38), (8, 8)), 4: ((44, 49), (8, 8)), 8: ((60, 65), (8, 7))},
    "step + records": {2: ((44, 54), (8, 8)), 4: ((63, 74), (8, 6)), 8: ((100, 110), (4, 4))},
    "first step": {1: ((12, 12), (8, 8)), 2: ((16, 16), (8, 8)), 4: ((14, 14), (8, 8)), 8: ((14, 14), (8, 8))},
}


def _resources(hipcc, src, tmp_path):
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, src), "-o",
                        str(tmp_path / (src + ".o")), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
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
    return info


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_cheb_kernels_have_no_spills_and_the_first_step_is_light(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    blocks = _resources(hipcc, "hip_amg_cheb.hip", tmp_path)
    single = {k: v for k, v in _resources(hipcc, "hip_amg.hip", tmp_path).items() if "k_amg_cheb" in k}
    # blocks: 6 lane counts x 3 widths, with and without records; one first step per width; nothing else in the file
    assert len([k for k in blocks if "k_amg_cheb_mI" in k]) == 36 and len([k for k in blocks if "k_amg_cheb_first_mI" in k]) == 3
    assert len(blocks) == 39, sorted(blocks)
    # single column: one step per lane count and the first step
    assert len([k for k in single if "k_amg_chebI" in k]) == 6 and len([k for k in single if "k_amg_cheb_first" in k]) == 1
    assert len(single) == 7, sorted(single)
    rows = {}
    for k, v in list(blocks.items()) + list(single.items()):
        assert v["ScratchSize"] == 0, (k, v)
        m = re.search(r"k_amg_cheb_mILi(\d+)ELi(\d+)ELb([01])E", k)
        if m:
            rows[("step",) + tuple(int(g) for g in m.groups())] = (v["VGPRs"], v["Occupancy"])
        m = re.search(r"k_amg_chebILi(\d+)E", k)
        if m:
            rows[("step", int(m.group(1)), 1, 0)] = (v["VGPRs"], v["Occupancy"])
        if "k_amg_cheb_first" in k:
            assert v["VGPRs"] <= 64, (k, v)
            m = re.search(r"k_amg_cheb_first_mILi(\d+)E", k)
            rows[("first", int(m.group(1)) if m else 1)] = (v["VGPRs"], v["Occupancy"])
    assert sorted(k for k in rows if k[0] == "step") == sorted(
        [("step", L, kp, rec) for L in LANES for kp in WIDTHS for rec in (0, 1)] + [("step", L, 1, 0) for L in LANES])
    assert sorted(k for k in rows if k[0] == "first") == [("first", w) for w in (1,) + WIDTHS]
    print("recorded:", FOUND)
    print("now, (step, L, KP, REC) or (first, KP) -> (VGPRs, occupancy):")
    for k in sorted(rows):
        print("  ", k, rows[k])
