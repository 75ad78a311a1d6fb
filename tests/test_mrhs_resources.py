"""Compile-time guard for the kernels of several right-hand sides (no GPU needed: hipcc cross-compiles gfx950),
in the manner of test_bicgstab_resources.py: nothing in hip_mrhs.hip spills, the sweeps of an iteration -- in
both forms, z = dinv .* r and z as a block of its own (Lb0 / Lb1 of the two update kernels) -- and the streaming
kernels around them are within 64 VGPRs at occupancy 8 -- what the PCG sweeps are held to -- and the file holds
the expected instantiations and nothing else."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")

# k_spmm_csr<L, KP, false> (the iteration's product) as found: (VGPRs, waves per SIMD).  Recorded, not a target:
# a lane keeps KP accumulators, the KP dot partials of its workgroup's rows and KP gathered operands in flight,
# all fp64 -- 6 KP registers before any addressing, so the 8-column form is past the 64 registers of occupancy 8;
# the kernel gathers (latency bound), and whether fewer registers and more waves would pay has not been
# measured.  The residual form <L, KP, true> of opts.verify carries KP error terms more (48-52 / 76-80 /
# 100-130 registers, occupancy 8 / 6 / 3-4) and runs once per verify round.
SPMM_FOUND = {(2, 2): (28, 8), (4, 2): (30, 8), (8, 2): (30, 8), (16, 2): (32, 8), (32, 2): (32, 8), (64, 2): (34, 8),
              (2, 4): (44, 8), (4, 4): (44, 8), (8, 4): (46, 8), (16, 4): (46, 8), (32, 4): (48, 8), (64, 4): (48, 8),
              (2, 8): (76, 6), (4, 8): (76, 6), (8, 8): (78, 6), (16, 8): (78, 6), (32, 8): (80, 6), (64, 8): (80, 6)}
# the streaming sweeps, held to 64 VGPRs at occupancy 8: those of the diagonal preconditioners and those with z as
# a block of its own (the last four stems and the Lb1 forms of the two update kernels)
SWEEPS = ("k_mrhs_initI", "k_mrhs_update_xrI", "k_mrhs_update_pI", "k_mrhs_restartI", "k_amg_mrhs_initI",
          "k_amg_dot2_mI", "k_amg_mrhs_restart_rI", "k_amg_mrhs_restart_pI")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_mrhs_kernels_have_no_spills_and_the_sweeps_full_occupancy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_mrhs.hip"), "-o", str(tmp_path / "hip_mrhs.o"),
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
    # one per batch width of the sweeps and the state kernels -- 3 widths x {dinv, z block} of the two update sweeps
    # and 3 x {records, records and p = z} of the two-block record kernel --, 6 lane counts x 3 widths x {product,
    # residual} of the SpMM, pack / unpack
    for stem, count in (("k_mrhs_initI", 3), ("k_mrhs_init_stateI", 3), ("k_mrhs_update_xrI", 6),
                        ("k_mrhs_update_pI", 6), ("k_mrhs_restartI", 3), ("k_mrhs_restart_stateI", 3),
                        ("k_amg_mrhs_initI", 3), ("k_amg_dot2_mI", 6), ("k_amg_mrhs_restart_rI", 3),
                        ("k_amg_mrhs_restart_pI", 3), ("k_spmm_csrI", 36), ("k_mrhs_pack", 1), ("k_mrhs_unpack", 1)):
        assert len([k for k in info if stem in k]) == count, (stem, sorted(info))
    for stem in ("k_mrhs_update_xrI", "k_mrhs_update_pI", "k_amg_dot2_mI"):  # both forms at every width
        assert sorted(re.search(r"ILi(\d)ELb([01])E", k).groups() for k in info if stem in k) == \
            sorted((str(kp), z) for kp in (2, 4, 8) for z in "01"), (stem, sorted(info))
    assert len(info) == 77  # nothing else lives in the file
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    sweeps = [k for k in info if any(stem in k for stem in SWEEPS)]
    assert len(sweeps) == 33
    for k in sweeps:
        assert info[k]["VGPRs"] <= 64 and info[k]["Occupancy"] == 8, (k, info[k])
    spmm = {}
    for k, v in info.items():
        m = re.search(r"k_spmm_csrILi(\d+)ELi(\d+)ELb([01])E", k)
        if m:
            spmm[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = (v["VGPRs"], v["Occupancy"])
    assert sorted(spmm) == sorted((L, kp, res) for (L, kp) in SPMM_FOUND for res in (0, 1))
    print("k_spmm_csr<L, KP> (VGPRs, occupancy):", spmm, "recorded:", SPMM_FOUND)
