"""Compile-time guard for the kernels of the direct solver on a tiered factor (hip_direct_t.hip; no GPU needed: hipcc
cross-compiles gfx950), in the manner of test_direct_resources.py: nothing spills, the expected kernels are there and
nothing else is, and the LDS a launch can ask for stays inside the 64 KB a launch gets without asking for more.  It
looks at these resource numbers only."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_amg_cheb_resources import _resources

EXPECTED = ["k_dirt_rows<true>", "k_dirt_rows<false>", "k_dirt_cols", "k_dirt_fwd", "k_dirt_bwd"]

# kernel -> (VGPRs, waves per SIMD, static LDS bytes) as found; recorded and printed beside what the compiler reports
# now, not a target and not tuned.  k_dirt_rows adds its window as dynamic LDS: DIR_LDS_CAP doubles at the most
FOUND = {
    "k_dirt_rows<true>": (32, 8, 0),
    "k_dirt_rows<false>": (32, 8, 0),
    "k_dirt_cols": (55, 8, 8192),
    "k_dirt_fwd": (18, 8, 0),
    "k_dirt_bwd": (20, 8, 0),
}


def _name(mangled):
    """k_dirt_rows<true> from _Z11k_dirt_rowsILb1EEv..., k_dirt_cols from _Z11k_dirt_colsjjj..."""
    m = re.match(r"_Z(\d+)", mangled)
    assert m, mangled
    name, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    return name + ("<true>" if rest.startswith("ILb1E") else "<false>" if rest.startswith("ILb0E") else "")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_tiered_direct_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = {_name(k): v for k, v in _resources(hipcc, "hip_direct_t.hip", tmp_path).items()}
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    assert sorted(info) == sorted(EXPECTED)
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_direct_drv.c")) as f:
        cap = int(re.search(r"#define DIR_LDS_CAP (\d+)u", f.read()).group(1))
    print("recorded:", FOUND)
    print("now, kernel -> (VGPRs, occupancy, static LDS bytes):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"], info[k]["LDS Size"]))
        dynamic = 8 * cap if "k_dirt_rows" in k else 0
        assert info[k]["LDS Size"] + dynamic <= 64 * 1024, k
