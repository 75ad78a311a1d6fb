"""Compile-time guard for the kernels every round of the direct solver shares (hip_direct.hip: the state, the residual
and the step; no GPU needed: hipcc cross-compiles gfx950), in the manner of test_richardson_resources.py: nothing spills, the expected kernels are there and nothing else is, and
the LDS a launch can ask for stays inside a compute unit's 160 KB.  It looks at these resource numbers only."""
import os
import shutil

import pytest

from test_amg_cheb_resources import _resources

RESID = "_Z11k_dir_residILi%dEEvjPKiS1_PKdS3_S3_PdS4_PK13lsb_pcg_state"
EXPECTED = ["_Z10k_dir_stepP13lsb_pcg_statePKdj", "_Z16k_dir_init_stateP13lsb_pcg_statedi"] + \
    [RESID % L for L in (2, 4, 8, 16, 32, 64)]

# kernel -> (VGPRs, waves per SIMD, static LDS bytes) as found; recorded and printed beside what the compiler reports
# now, not a target and not tuned.  The products, and the dynamic LDS of their staged windows, are hip_direct_t.hip's:
# test_direct_tiers_resources.py
FOUND = {
    "k_dir_resid, 2 .. 64 lanes per row": ((28, 8, 64), (30, 8, 64), (32, 8, 64), (34, 8, 64), (36, 8, 64),
                                           (38, 8, 64)),
    "k_dir_step / k_dir_init_state": ((17, 8, 64), (8, 8, 0)),
}
LDS_PER_CU = 160 * 1024


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_direct_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_direct.hip", tmp_path)
    for k, v in info.items():
        assert "k_dir_" in k, k
        assert v["ScratchSize"] == 0, (k, v)
    assert sorted(info) == sorted(EXPECTED)
    print("recorded:", FOUND)
    print("now, kernel -> (VGPRs, occupancy, static LDS bytes):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"], info[k]["LDS Size"]))
        assert info[k]["LDS Size"] <= LDS_PER_CU, k
