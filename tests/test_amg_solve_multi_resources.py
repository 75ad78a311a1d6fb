"""Compile-time guard for the kernels of AMG as the solver on blocks of right-hand sides (hip_rich_m.hip: the iteration;
hip_amg_f32_m.hip: the fp32 V-cycle on blocks; no GPU needed: hipcc cross-compiles gfx950), in the manner of
test_direct_multi_resources.py: nothing spills, the expected kernels are there and nothing else is.  VGPRs, occupancy
and LDS are printed and recorded, not targeted."""
import os
import re
import shutil

import pytest

from test_amg_cheb_resources import _resources

WIDTHS, LANES = (2, 4, 8), (2, 4, 8, 16, 32, 64)
SWEEP, RESID, SPMV, ADDP = 1, 2, 3, 4  # LSB_AMG_* (lsb_impl.h)
CST, ST = "PK14lsb_mrhs_state", "P14lsb_mrhs_state"

RICH = [f for k in WIDTHS for f in (
    "_Z12k_richm_initILi%dEEvjPKdPdS2_S2_" % k,
    "_Z18k_richm_init_stateILi%dEEv" % k + ST + "PKdjdi",
    "_Z14k_richm_updateILi%dEEvjPKdS1_PdS2_" % k + CST + "S2_",
    "_Z12k_richm_stepILi%dEEv" % k + ST + "PKdj",
    "_Z15k_richm_restartILi%dEEvjPKdS1_Pd" % k + CST + "S2_",
    "_Z21k_richm_restart_stateILi%dEEv" % k + ST + "PKdji")]

# k_amg32_csr_m<L, KP, MODE, OUT64>: the four modes, and the sweep once more with the fp64 store of the fine level's
# last step; k_amg32_first_m<KP, IN64>; k_amg32_dense_m<L, KP, IN64, OUT64>: between float blocks, or from R to Z
CSR = r"_Z13k_amg32_csr_mILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EEvjPKiPKyPKfS5_S5_PfPd" + CST
FIRST = r"_Z15k_amg32_first_mILi(\d+)ELb([01])EEvjPKvPKfPfS4_" + CST
DENSE = r"_Z15k_amg32_dense_mILi(\d+)ELi(\d+)ELb([01])ELb([01])EEvjPKfPKvPv" + CST

# kernel -> (VGPRs, waves per SIMD, static LDS bytes) per width 2, 4, 8 as found when the kernels were written;
# recorded and printed beside what the compiler reports now, not a target and not tuned
FOUND = {
    "iteration": {
        "k_richm_init": ((28, 8, 64), (40, 8, 128), (64, 8, 256)),
        "k_richm_init_state": ((18, 8, 64), (35, 8, 128), (46, 8, 256)),
        "k_richm_update": ((36, 8, 64), (40, 8, 128), (48, 8, 256)),
        "k_richm_step": ((17, 8, 64), (33, 8, 128), (65, 7, 256)),
        "k_richm_restart": ((26, 8, 64), (33, 8, 128), (41, 8, 256)),
        "k_richm_restart_state": ((22, 8, 64), (38, 8, 128), (70, 7, 256)),
    },
    # (VGPRs, waves per SIMD) at 2 and at 64 lanes per row; no LDS anywhere
    "fp32 cycle": {
        "k_amg32_csr_m, the sweep": (((22, 8), (26, 8)), ((30, 8), (34, 8)), ((46, 8), (50, 8))),
        "k_amg32_csr_m, residual / restriction / prolongation": (((20, 8), (26, 8)), ((24, 8), (30, 8)),
                                                                 ((34, 8), (38, 8))),
        "k_amg32_dense_m, between float blocks": (((20, 8), (26, 8)), ((24, 8), (30, 8)), ((34, 8), (38, 8))),
        "k_amg32_dense_m, from R to Z": (((22, 8), (28, 8)), ((28, 8), (34, 8)), ((40, 8), (46, 8))),
        "k_amg32_first_m, from a float block and from R": (((12, 8), (11, 8)), ((14, 8), (15, 8)), ((18, 8), (23, 8))),
    },
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_iteration_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_rich_m.hip", tmp_path)
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    assert sorted(info) == sorted(RICH)
    print("recorded:", FOUND.get("iteration"))
    print("now, kernel -> (VGPRs, occupancy, static LDS bytes):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"], info[k]["LDS Size"]))
        assert info[k]["LDS Size"] == 4 * 8 * int(re.search(r"ILi(\d)E", k).group(1))  # sred: 4 KP doubles


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_fp32_block_cycle_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_amg_f32_m.hip", tmp_path)
    csr, first, dense = set(), set(), set()
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] == 0, (k, v)
        for pat, into in ((CSR, csr), (FIRST, first), (DENSE, dense)):
            m = re.fullmatch(pat, k)
            if m:
                into.add(tuple(int(g) for g in m.groups()))
    assert len(csr) + len(first) + len(dense) == len(info), sorted(info)
    assert csr == {(L, k, mode, 0) for L in LANES for k in WIDTHS for mode in (SWEEP, RESID, SPMV, ADDP)} | \
        {(L, k, SWEEP, 1) for L in LANES for k in WIDTHS}
    assert first == {(k, i) for k in WIDTHS for i in (0, 1)}
    assert dense == {(L, k, e, e) for L in LANES for k in WIDTHS for e in (0, 1)}
    print("recorded:", FOUND.get("fp32 cycle"))
    print("now, kernel -> (VGPRs, occupancy):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"]))
