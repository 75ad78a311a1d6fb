"""Compile-time guard for the kernels of block-CG under FSAI and AMG (no GPU needed: hipcc cross-compiles gfx950), in the
manner of test_block_cg_resources.py: nothing in hip_bcg_m.hip spills and the file holds the expected instantiations --
k_bcgm_gt_gram at 6 lane counts x 3 widths, k_bcgm_gram at 3 widths x 2 (the loop's and the start's), the other three
streaming launches at 3 widths -- and nothing else.  It looks at these resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
LANES, WIDTHS = (2, 4, 8, 16, 32, 64), (2, 4, 8)
STREAMING = ("k_bcgm_pass_a", "k_bcgm_start", "k_bcgm_pass_b")

# As found: (VGPRs, waves per SIMD).  Recorded and printed beside what the compiler reports now, not a target.  At 8
# columns the loop's k_bcgm_gram keeps the 36 + 36 running sums of its two triangles beside a row of W~ and of Z~: the
# register file of one wave per SIMD, as k_bcg_pass_a; k_bcgm_gt_gram deals those sums over the L lanes of a row.
FOUND_GT_GRAM = {2: ((34, 30, 32, 32, 34, 34), (8, 8, 8, 8, 8, 8)),  # L = 2, 4, 8, 16, 32, 64
                 4: ((56, 48, 46, 42, 44, 44), (8, 8, 8, 8, 8, 8)),
                 8: ((146, 96, 83, 75, 73, 70), (3, 5, 5, 6, 6, 7))}
FOUND_GRAM = {(2, 0): (30, 8), (2, 1): (28, 8), (4, 0): (82, 5), (4, 1): (62, 8), (8, 0): (256, 1), (8, 1): (178, 2)}
FOUND = {"k_bcgm_pass_a": {2: (28, 8), 4: (40, 8), 8: (75, 6)},
         "k_bcgm_start": {2: (28, 8), 4: (44, 8), 8: (76, 6)},
         "k_bcgm_pass_b": {2: (28, 8), 4: (48, 8), 8: (88, 5)}}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_block_cg_precond_kernels_have_no_spills_and_the_expected_instantiations(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_bcg_m.hip"), "-o", str(tmp_path / "hip_bcg_m.o"),
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
        m = re.search(r"\d+(k_bcgm_gt_gram)ILi(\d+)ELi(\d+)E", k) or re.search(r"\d+(k_bcgm_gram)ILi(\d+)ELb([01])E", k) or \
            re.search(r"\d+(k_bcgm_pass_a|k_bcgm_start|k_bcgm_pass_b)ILi(\d+)E()", k)
        assert m, k  # nothing else lives in the file
        key = (m.group(1), int(m.group(2))) + ((int(m.group(3)),) if m.group(3) else ())
        rows[key] = (v["VGPRs"], v["Occupancy"])
    want = [("k_bcgm_gt_gram", L, kp) for L in LANES for kp in WIDTHS] + \
           [("k_bcgm_gram", kp, st) for kp in WIDTHS for st in (0, 1)] + [(kn, kp) for kn in STREAMING for kp in WIDTHS]
    assert len(info) == len(want) == 33
    assert sorted(rows, key=repr) == sorted(want, key=repr)
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    print("k_bcgm_gt_gram, KP: recorded (VGPRs L = 2 .. 64), (occupancy) | now")
    for kp in WIDTHS:
        now = (tuple(rows[("k_bcgm_gt_gram", L, kp)][0] for L in LANES),
               tuple(rows[("k_bcgm_gt_gram", L, kp)][1] for L in LANES))
        print("  ", kp, FOUND_GT_GRAM[kp], "|", now)
    print("k_bcgm_gram, (KP, START): recorded (VGPRs, occupancy) | now")
    for kp in WIDTHS:
        for st in (0, 1):
            print("  ", kp, st, FOUND_GRAM[(kp, st)], "|", rows[("k_bcgm_gram", kp, st)])
    print("streaming launches, (kernel, KP): recorded (VGPRs, occupancy) | now")
    for kn in STREAMING:
        for kp in WIDTHS:
            print("  ", kn, kp, FOUND[kn][kp], "|", rows[(kn, kp)])
