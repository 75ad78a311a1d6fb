"""Compile-time guard for the kernels of the direct solver on blocks of right-hand sides (hip_direct_m.hip; no GPU
needed: hipcc cross-compiles gfx950), in the manner of test_direct_resources.py: nothing spills, the expected kernels
are there and nothing else is, and k_dir_rows_m's staged window at the cap stays inside the 64 KB a launch gets without
asking for more.  It looks at these resource numbers only; VGPRs and occupancy are printed and recorded, not targeted."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_amg_cheb_resources import _resources

WIDTHS, LANES = (2, 4, 8), (2, 4, 8, 16, 32, 64)
STATE = "PK14lsb_mrhs_state"
ROWS = "_Z12k_dir_rows_mILi%dEEvPKdPKyPKjS5_S5_S5_S5_jS1_S1_Pd" + STATE
COLS = "_Z12k_dir_cols_mILi%dELi%dEEvjPKdPKyPKjS5_S5_S5_S1_Pd" + STATE
RESID = "_Z13k_dir_resid_mILi%dELi%dEEvjPKiS1_PKdS3_S3_PdS4_" + STATE
STEP = "_Z12k_dir_step_mILi%dEEvP14lsb_mrhs_statePKdj"
FLIGHT = {2: 8, 4: 4, 8: 4}  # rows in flight per wavefront of k_dir_cols_m (dirm_flight)
EXPECTED = ["_Z18k_dir_init_state_mP14lsb_mrhs_statejdi"] + [ROWS % k for k in WIDTHS] + \
    [COLS % (k, FLIGHT[k]) for k in WIDTHS] + [RESID % (L, k) for k in WIDTHS for L in LANES] + \
    [STEP % k for k in WIDTHS]

# kernel -> (VGPRs, waves per SIMD, static LDS bytes) per width 2, 4, 8 as found; recorded and printed beside what the
# compiler reports now, not a target and not tuned.  k_dir_rows_m adds its window of P V as dynamic LDS: DIR_LDS_CAP
# doubles at the most, whatever the width (DIR_LDS_CAP / kp rows of kp doubles)
FOUND = {
    "k_dir_rows_m": ((38, 8, 0), (36, 8, 0), (60, 8, 0)),
    "k_dir_cols_m": ((68, 7, 16384), (68, 7, 32768), (76, 6, 65536)),
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
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_direct_drv.c")) as f:
        cap = int(re.search(r"#define DIR_LDS_CAP (\d+)u", f.read()).group(1))
    print("recorded:", FOUND)
    print("now, kernel -> (VGPRs, occupancy, static LDS bytes):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"], info[k]["LDS Size"]))
        # every launch stays inside the 64 KB it gets without asking: the staged window at the cap is cap / kp rows of
        # kp doubles, and k_dir_cols_m's sixteen partial sums of 64 columns are 8 KB per column of the block
        dynamic = 8 * cap if "k_dir_rows_m" in k else 0
        assert info[k]["LDS Size"] + dynamic <= 64 * 1024, k
    for kp in WIDTHS:
        assert (cap // kp) * kp * 8 + info[ROWS % kp]["LDS Size"] <= 64 * 1024
        assert info[COLS % (kp, FLIGHT[kp])]["LDS Size"] == 16 * 64 * 8 * kp
