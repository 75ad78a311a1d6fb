"""Compile-time guard for the kernels of the stationary V-cycle iteration (hip_rich.hip; no GPU needed: hipcc
cross-compiles gfx950), in the manner of test_amg_f32_resources.py: nothing spills, the expected kernels are there and
nothing else is.  It looks at these resource numbers only."""
import os
import shutil

import pytest

from test_amg_cheb_resources import _resources

# the sweeps in their 16-byte (Lb1) and 8-byte (Lb0) instantiation, the three one-workgroup state kernels
EXPECTED = ["_Z11k_rich_initILb0EEvjPKdPdS2_S2_", "_Z11k_rich_initILb1EEvjPKdPdS2_S2_",
            "_Z13k_rich_updateILb0EEvjPKdS1_PdS2_PK13lsb_pcg_stateS2_",
            "_Z13k_rich_updateILb1EEvjPKdS1_PdS2_PK13lsb_pcg_stateS2_",
            "_Z14k_rich_restartILb0EEvjPKdS1_PdS2_", "_Z14k_rich_restartILb1EEvjPKdS1_PdS2_",
            "_Z11k_rich_stepP13lsb_pcg_statePKdj", "_Z17k_rich_init_stateP13lsb_pcg_statePKdjdi",
            "_Z20k_rich_restart_stateP13lsb_pcg_statePKdji"]

# kernel -> (VGPRs, waves per SIMD) as found; recorded and printed beside what the compiler reports now, not a
# target and not tuned
FOUND = {
    "k_rich_init (8-byte, 16-byte)": ((22, 8), (22, 8)),
    "k_rich_update (8-byte, 16-byte)": ((34, 8), (34, 8)),
    "k_rich_restart (8-byte, 16-byte)": ((22, 8), (22, 8)),
    "k_rich_step / k_rich_init_state / k_rich_restart_state": ((9, 8), (11, 8), (12, 8)),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_rich_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_rich.hip", tmp_path)
    for k, v in info.items():
        assert "k_rich_" in k, k
        assert v["ScratchSize"] == 0, (k, v)
    assert sorted(info) == sorted(EXPECTED)
    print("recorded:", FOUND)
    print("now, kernel -> (VGPRs, occupancy):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"]))
