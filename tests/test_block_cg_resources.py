"""Compile-time guard for the kernels of block-CG proper (no GPU needed: hipcc cross-compiles gfx950), in the manner of
test_mrhs_fsai_resources.py: nothing in hip_bcg.hip spills and the file holds the expected instantiations -- the SpMM
at 6 lane counts x 3 widths, the four streaming launches at 3 widths, the single-workgroup launch at 3 widths x 4
phases -- and nothing else.  It looks at these resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
LANES, WIDTHS, PHASES = (2, 4, 8, 16, 32, 64), (2, 4, 8), (0, 1, 2, 3)
STREAMING = ("k_bcg_init", "k_bcg_start", "k_bcg_pass_a", "k_bcg_pass_b")

# As found: (VGPRs, waves per SIMD).  Recorded and printed beside what the compiler reports now, not a target.  A lane
# of the streaming launches owns whole rows: at 8 columns k_bcg_pass_a keeps the 36 + 36 running sums of its two Gram
# triangles beside a row of W, Q, P and X, which is the register file of one wave per SIMD; k_bcg_init (once per
# solve) keeps 36 + 8.  Whether fewer registers would pay has not been measured.
FOUND_SPMM = {2: ((30, 28, 30, 30, 32, 32), (8, 8, 8, 8, 8, 8)),  # L = 2, 4, 8, 16, 32, 64
              4: ((46, 42, 42, 40, 42, 42), (8, 8, 8, 8, 8, 8)),
              8: ((96, 78, 73, 70, 69, 68), (5, 6, 6, 7, 7, 7))}
FOUND = {"k_bcg_init": {2: (28, 8), 4: (64, 8), 8: (180, 2)},
         "k_bcg_start": {2: (24, 8), 4: (36, 8), 8: (66, 7)},
         "k_bcg_pass_a": {2: (44, 8), 4: (86, 5), 8: (256, 1)},
         "k_bcg_pass_b": {2: (28, 8), 4: (40, 8), 8: (66, 7)}}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_block_cg_kernels_have_no_spills_and_the_expected_instantiations(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_bcg.hip"), "-o", str(tmp_path / "hip_bcg.o"),
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
    rows = {}
    for k, v in info.items():
        m = re.search(r"\d+(k_bcg_spmm|k_bcg_small)ILi(\d+)ELi(\d+)E", k) or \
            re.search(r"\d+(k_bcg_init|k_bcg_start|k_bcg_pass_a|k_bcg_pass_b)ILi(\d+)E()", k)
        assert m, k  # nothing else lives in the file
        key = (m.group(1), int(m.group(2))) + ((int(m.group(3)),) if m.group(3) else ())
        rows[key] = (v["VGPRs"], v["Occupancy"])
    want = [("k_bcg_spmm", L, kp) for L in LANES for kp in WIDTHS] + \
           [("k_bcg_small", kp, ph) for kp in WIDTHS for ph in PHASES] + [(kn, kp) for kn in STREAMING for kp in WIDTHS]
    assert len(info) == len(want) == 42
    assert sorted(rows, key=repr) == sorted(want, key=repr)
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    print("k_bcg_spmm, KP: recorded (VGPRs L = 2 .. 64), (occupancy) | now")
    for kp in WIDTHS:
        now = (tuple(rows[("k_bcg_spmm", L, kp)][0] for L in LANES), tuple(rows[("k_bcg_spmm", L, kp)][1] for L in LANES))
        print("  ", kp, FOUND_SPMM[kp], "|", now)
    print("streaming launches, (kernel, KP): recorded (VGPRs, occupancy) | now")
    for kn in STREAMING:
        for kp in WIDTHS:
            print("  ", kn, kp, FOUND[kn][kp], "|", rows[(kn, kp)])
    print("k_bcg_small, (KP, phase): (VGPRs, occupancy) now")
    for kp in WIDTHS:
        print("  ", kp, [rows[("k_bcg_small", kp, ph)] for ph in PHASES])
