"""Compile-time guard for the kernels of several right-hand sides under AMG (no GPU needed: hipcc cross-compiles
gfx950), in the manner of test_mrhs_resources.py: nothing in hip_mrhs_amg.hip spills, its streaming kernel is
within 64 VGPRs at occupancy 8 -- what the PCG sweeps are held to; the PCG sweeps around the cycle live in
hip_mrhs.hip and are held to the same there -- and the file holds the expected instantiations and nothing else.
It looks at these resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
LANES, WIDTHS = (2, 4, 8, 16, 32, 64), (2, 4, 8)
# (MODE, REC) of k_amg_csr_m: LSB_AMG_SWEEP = 1 with and without the record epilogue, RESID = 2, SPMV = 3, ADDP = 4
FORMS = ((1, 0), (1, 1), (2, 0), (3, 0), (4, 0))
STREAMS = ("k_amg_first_mI",)

# The row kernels as found: form -> width -> ((VGPRs from L = 2 to L = 64), (waves per SIMD likewise)).  Recorded and
# printed beside what the compiler reports now, not a target: a lane keeps KP accumulators and KP gathered operands
# in flight as k_spmm_csr does (28-34 / 44-48 / 76-80 registers there), the sweep with records 2 KP running sums
# more -- at 8 columns that form is past the 64 registers of occupancy 8; it runs once per iteration, on the fine
# level, and whether fewer registers would pay there has not been measured.
FOUND = {
    "sweep": {2: ((32, 38), (8, 8)), 4: ((40, 46), (8, 8)), 8: ((56, 62), (8, 8))},
    "sweep + records": {2: ((42, 52), (8, 8)), 4: ((60, 70), (8, 7)), 8: ((92, 104), (5, 4))},
    "residual, restriction": {2: ((24, 28), (8, 8)), 4: ((34, 40), (8, 8)), 8: ((50, 56), (8, 8))},
    "prolongation": {2: ((24, 28), (8, 8)), 4: ((34, 40), (8, 8)), 8: ((56, 62), (8, 8))},
    "dense": {2: ((26, 30), (8, 8)), 4: ((34, 40), (8, 8)), 8: ((50, 56), (8, 8))},
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_mrhs_amg_kernels_have_no_spills_and_the_sweeps_full_occupancy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_mrhs_amg.hip"), "-o", str(tmp_path / "hip_mrhs_amg.o"),
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
    # 6 lane counts x 3 widths x 5 forms of the row kernel, 6 x 3 of the dense one, one per width of every stream
    for stem, count in (("k_amg_csr_mI", 90), ("k_amg_dense_mI", 18)) + tuple((s, 3) for s in STREAMS):
        assert len([k for k in info if stem in k]) == count, (stem, sorted(info))
    assert len(info) == 90 + 18 + 3 * len(STREAMS)  # nothing else lives in the file
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in info.items():
        if any(stem in k for stem in STREAMS):
            assert v["VGPRs"] <= 64 and v["Occupancy"] == 8, (k, v)
    rows = {}
    for k, v in info.items():
        m = re.search(r"k_amg_csr_mILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", k)
        if m:
            rows[("csr",) + tuple(int(g) for g in m.groups())] = (v["VGPRs"], v["Occupancy"])
        m = re.search(r"k_amg_dense_mILi(\d+)ELi(\d+)E", k)
        if m:
            rows[("dense",) + tuple(int(g) for g in m.groups())] = (v["VGPRs"], v["Occupancy"])
    assert sorted(k for k in rows if k[0] == "csr") == sorted(("csr", L, kp, mode, rec) for L in LANES for kp in WIDTHS
                                                             for (mode, rec) in FORMS)
    assert sorted(k for k in rows if k[0] == "dense") == sorted(("dense", L, kp) for L in LANES for kp in WIDTHS)
    print("recorded:", FOUND)
    print("row kernels now, (kernel, L, KP[, MODE, REC]) -> (VGPRs, occupancy):")
    for k in sorted(rows):
        print("  ", k, rows[k])
