"""Compile-time guard for the kernels of the multicolour Gauss-Seidel smoother (hip_amg_mcgs.hip; no GPU needed: hipcc
cross-compiles gfx950), in the manner of test_amg_f32_resources.py: nothing spills, the expected instantiations are
there and nothing else is.  It looks at these resource numbers only."""
import os
import re
import shutil

import pytest

import lsbench_amd as la
from test_amg_cheb_resources import _resources

assert la.AMG_SMOOTH_MCGS == 2
LANES = (2, 4, 8, 16, 32, 64)

# kernel -> (VGPRs from L = 2 to L = 64, waves per SIMD likewise) as found; recorded and printed beside what the
# compiler reports now, not a target and not tuned: every kernel at the full 8 waves per SIMD.
FOUND = {
    "mcgs (fp64)": ((22, 26), (8, 8)),
    "mcgs32 (float result, or float and fp64)": ((18, 24), (8, 8)),
    "first / first32": ((8, 10), (8, 8)),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_mcgs_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_amg_mcgs.hip", tmp_path)
    rows = {}
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
        for stem, pat in (("mcgs", r"k_amg_mcgsILi(\d+)E"), ("first", r"k_amg_mcgs_first(?!I)"),
                          ("mcgs32", r"k_amg32_mcgsILi(\d+)ELb([01])E"), ("first32", r"k_amg32_mcgs_firstILb([01])E")):
            m = re.search(pat, k)
            if m:
                key = (stem,) + tuple(int(g) for g in m.groups())
                assert key not in rows, key
                rows[key] = (v["VGPRs"], v["Occupancy"])
                break
        else:
            raise AssertionError("a kernel nobody expected: " + k)
    # a colour step per lane count in fp64; in fp32 with the float result alone and with the fp64 z beside it; the
    # first launch in fp64, and in fp32 from a float b or from the caller's fp64 r
    expected = [("mcgs", L) for L in LANES] + [("first",)] + [("mcgs32", L, o) for L in LANES for o in (0, 1)] + \
               [("first32", 0), ("first32", 1)]
    assert sorted(rows) == sorted(expected)
    assert len(info) == len(expected) == 21
    print("recorded:", FOUND)
    print("now, (kernel, template arguments) -> (VGPRs, occupancy):")
    for k in sorted(rows):
        print("  ", k, rows[k])
