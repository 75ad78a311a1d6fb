"""Compile-time guard for the kernels of the geometric V-cycle (no GPU needed: hipcc cross-compiles gfx950), in the
manner of test_amg_cheb_resources.py: nothing in hip_gmg.hip spills, the expected instantiations -- DIM 2 and 3 of
each of the six kernels -- are there and no others, and the tile of the fused way up is the LDS the file says.  It
looks at these resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
KERNELS = ("k_gmg_first", "k_gmg_sweep", "k_gmg_restrict", "k_gmg_prolong", "k_gmg_down", "k_gmg_up")

# As found: kernel -> ((VGPRs at DIM 2, DIM 3), (waves per SIMD likewise)).  Recorded and printed beside what the
# compiler reports now, not a target and not tuned.  The two kernels that form 3^dim residuals per lane are the heavy
# ones: in 3-D the restriction loop is kept rolled to a line of three residuals at a time.
FOUND = {
    "k_gmg_first": ((13, 13), (8, 8)), "k_gmg_sweep": ((20, 28), (8, 8)), "k_gmg_restrict": ((64, 91), (8, 5)),
    "k_gmg_prolong": ((24, 36), (8, 8)), "k_gmg_down": ((76, 133), (6, 3)), "k_gmg_up": ((30, 44), (8, 8)),
}
# the tile of k_gmg_up and its one-point halo, in doubles: 66 x 10 (2-D), 34 x 6 x 6 (3-D)
LDS = {"k_gmg_up": (66 * 10 * 8, 34 * 6 * 6 * 8)}


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
def test_gmg_kernels_have_no_spills_and_the_expected_instantiations(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_gmg.hip", tmp_path)
    rows = {}
    for k, v in info.items():
        m = re.search(r"\d+(k_gmg_[a-z]+)ILi(\d)E", k)
        assert m, "a kernel the file is not meant to hold: " + k
        assert v["ScratchSize"] == 0, (k, v)
        rows[(m.group(1), int(m.group(2)))] = v
    assert sorted(rows) == sorted((name, dim) for name in KERNELS for dim in (2, 3)) and len(info) == 12
    for name in KERNELS:
        for at, dim in enumerate((2, 3)):
            assert rows[(name, dim)]["LDS Size"] == LDS.get(name, (0, 0))[at], (name, dim, rows[(name, dim)])
    print("recorded:", FOUND)
    print("now, (kernel, DIM) -> (VGPRs, waves per SIMD, LDS bytes per workgroup):")
    for k in sorted(rows):
        print("  ", k, (rows[k]["VGPRs"], rows[k]["Occupancy"], rows[k]["LDS Size"]))
