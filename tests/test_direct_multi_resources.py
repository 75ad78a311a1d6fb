"""Compile-time guard for the kernels every round of the direct solver on blocks of right-hand sides shares
(hip_direct_m.hip: the state, the residual and the step; no GPU needed: hipcc cross-compiles gfx950), in the manner of
test_direct_resources.py: nothing spills, the expected kernels are there and nothing else is, and every launch stays
inside the 64 KB it gets without asking for more.  The products, and the dynamic LDS of their staged windows, are
hip_direct_tm.hip's: test_direct_tier_multi_resources.py.  It looks at these resource numbers only; VGPRs and occupancy are printed and recorded, not targeted."""
import os
import shutil

import pytest

from test_amg_cheb_resources import _resources

WIDTHS, LANES = (2, 4, 8), (2, 4, 8, 16, 32, 64)
STATE = "PK14lsb_mrhs_state"
RESID = "_Z13k_dir_resid_mILi%dELi%dEEvjPKiS1_PKdS3_S3_PdS4_" + STATE
STEP = "_Z12k_dir_step_mILi%dEEvP14lsb_mrhs_statePKdj"
EXPECTED = ["_Z18k_dir_init_state_mP14lsb_mrhs_statejdi"] + [RESID % (L, k) for k in WIDTHS for L in LANES] + \
    [STEP % k for k in WIDTHS]

# kernel -> (VGPRs, waves per SIMD, static LDS bytes) per width 2, 4, 8 as found; recorded and printed beside what the
# compiler reports now, not a target and not tuned
FOUND = {
    "k_dir_resid_m, 2 and 64 lanes per row": (((36, 8, 128), (46, 8, 128)), ((54, 8, 256), (64, 8, 256)),
                                              ((86, 5, 512), (96, 5, 512))),
    "k_dir_step_m": ((38, 8, 128), (70, 7, 256), (134, 3, 512)),
    "k_dir_init_state_m": (18, 8, 0),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_direct_multi_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_direct_m.hip", tmp_path)
    for k, v in info.items():
        assert "k_dir_" in k and "_m" in k, k
        assert v["ScratchSize"] == 0, (k, v)
    assert sorted(info) == sorted(EXPECTED)
    print("recorded:", FOUND)
    print("now, kernel -> (VGPRs, occupancy, static LDS bytes):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"], info[k]["LDS Size"]))
        assert info[k]["LDS Size"] <= 64 * 1024, k  # every launch stays inside the 64 KB it gets without asking
