"""Compile-time guard for the kernels of the projection onto earlier solutions (hip_seq.hip; no GPU needed: hipcc
cross-compiles gfx950), in the manner of test_amg_mcgs_resources.py: no kernel uses scratch, the expected
instantiations are there and nothing else is.  It looks at these resource numbers only."""
import os
import re
import shutil

import pytest

import lsbench_amd as la
from test_amg_cheb_resources import _resources

MS = tuple(range(1, la.SEQ_MAX_DEPTH + 1))

# kernel -> (VGPRs from m = 1 to m = 16, waves per SIMD likewise) as found; recorded and printed beside what the
# compiler reports now, not a target and not tuned.  The registers are what holding a turn's loads of every stream
# in flight costs: k_seq_orth<16> keeps 34 16-byte loads per lane outstanding and runs two waves per SIMD.
FOUND = {
    "dots": ((16, 106), (8, 4)),
    "combine": ((12, 70), (8, 7)),
    "orth": ((32, 182), (8, 2)),
    "store": ((50, 50), (8, 8)),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_seq_kernels_have_no_scratch_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = _resources(hipcc, "hip_seq.hip", tmp_path)
    rows = {}
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
        for stem, pat in (("dots", r"k_seq_dotsILi(\d+)EE"), ("combine", r"k_seq_combineILi(\d+)EE"),
                          ("orth", r"k_seq_orthILi(\d+)EE"), ("store", r"k_seq_store(?!I)")):
            m = re.search(pat, k)
            if m:
                key = (stem,) + tuple(int(g) for g in m.groups())
                assert key not in rows, key
                rows[key] = (v["VGPRs"], v["Occupancy"])
                break
        else:
            raise AssertionError("a kernel nobody expected: " + k)
    # every sweep over the basis once per number of vectors, and the store
    expected = [(stem, m) for stem in ("dots", "combine", "orth") for m in MS] + [("store",)]
    assert sorted(rows) == sorted(expected)
    assert len(info) == len(expected) == 49
    # the widest instantiation holds its loads and its accumulators in registers: under the 256 that leave two
    # waves per SIMD
    assert max(v for v, _ in rows.values()) <= 256
    print("recorded:", FOUND)
    print("now, (kernel, template arguments) -> (VGPRs, occupancy):")
    for k in sorted(rows):
        print("  ", k, rows[k])
