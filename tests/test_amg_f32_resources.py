"""Compile-time guard for the kernels of the fp32 AMG V-cycle (hip_amg_f32.hip; no GPU needed: hipcc cross-compiles
gfx950), in the manner of test_amg_cheb_resources.py: nothing spills, the expected instantiations are there and
nothing else is.  It looks at these resource numbers only."""
import os
import re
import shutil

import pytest

from test_amg_cheb_resources import _resources

LANES = (2, 4, 8, 16, 32, 64)
SWEEP, RESID, SPMV, ADDP = 1, 2, 3, 4

# kernel -> (VGPRs from L = 2 to L = 64, waves per SIMD likewise) as found; recorded and printed beside what the
# compiler reports now, not a target and not tuned: every kernel at the full 8 waves per SIMD.
FOUND = {
    "csr (any mode, fp32 or fp64 result)": ((20, 24), (8, 8)),
    "cheb (fp32 or fp64 result)": ((20, 24), (8, 8)),
    "dense": ((17, 23), (8, 8)),
    "first / cheb_first": ((9, 11), (8, 8)),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_f32_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_amg_f32.hip", tmp_path)
    rows = {}
    for k, v in info.items():
        assert "k_amg32_" in k, k
        assert v["ScratchSize"] == 0, (k, v)
        for stem, pat in (("csr", r"k_amg32_csrILi(\d+)ELi(\d+)ELb([01])E"), ("first", r"k_amg32_firstILb([01])E"),
                          ("cheb", r"k_amg32_chebILi(\d+)ELb([01])E"), ("cheb_first", r"k_amg32_cheb_firstILb([01])E"),
                          ("dense", r"k_amg32_denseILi(\d+)ELb([01])ELb([01])E")):
            m = re.search(pat, k)
            if m:
                key = (stem,) + tuple(int(g) for g in m.groups())
                assert key not in rows, key
                rows[key] = (v["VGPRs"], v["Occupancy"])
                break
        else:
            raise AssertionError("a kernel nobody expected: " + k)
    # the four modes on floats and the sweep that writes the fp64 z; a first step per end; the Chebyshev step with
    # either result; the coarse solve on floats and, for a one-level hierarchy, from the fp64 r to the fp64 z
    expected = [("csr", L, m, 0) for L in LANES for m in (SWEEP, RESID, SPMV, ADDP)] + \
               [("csr", L, SWEEP, 1) for L in LANES] + [("first", 0), ("first", 1)] + \
               [("cheb", L, o) for L in LANES for o in (0, 1)] + [("cheb_first", 0), ("cheb_first", 1)] + \
               [("dense", L, e, e) for L in LANES for e in (0, 1)]
    assert sorted(rows) == sorted(expected)
    assert len(info) == len(expected) == 58
    print("recorded:", FOUND)
    print("now, (kernel, template arguments) -> (VGPRs, occupancy):")
    for k in sorted(rows):
        print("  ", k, rows[k])
