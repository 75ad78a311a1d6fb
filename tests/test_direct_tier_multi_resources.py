"""Compile-time guard for the kernels of the direct solver on a tiered factor on blocks of right-hand sides
(hip_direct_tm.hip; no GPU needed: hipcc cross-compiles gfx950), in the manner of test_direct_tiers_resources.py:
nothing spills, the expected kernels are there and nothing else is, and the LDS a launch can ask for stays inside the
64 KB a launch gets without asking for more.  It looks at these resource numbers only; VGPRs and occupancy are printed
and recorded, not targeted."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_amg_cheb_resources import _resources

WIDTHS = (2, 4, 8)
FLIGHT = {2: 8, 4: 4, 8: 4}  # rows in flight per wavefront of k_dirt_cols_m (dirtm_flight)
EXPECTED = ["k_dirt_rows_m<%d, true>" % k for k in WIDTHS] + ["k_dirt_rows_m<%d, false>" % k for k in WIDTHS] + \
    ["k_dirt_cols_m<%d, %d>" % (k, FLIGHT[k]) for k in WIDTHS] + ["k_dirt_fwd_m<%d>" % k for k in WIDTHS] + \
    ["k_dirt_bwd_m<%d>" % k for k in WIDTHS]

# kernel -> (VGPRs, waves per SIMD, static LDS bytes) per width 2, 4, 8 as found; recorded and printed beside what the
# compiler reports now, not a target and not tuned.  k_dirt_rows_m adds its window as dynamic LDS: DIR_LDS_CAP doubles
# at the most, whatever the width (DIR_LDS_CAP / kp rows of kp doubles)
FOUND = {
    "k_dirt_rows_m<KP, true>": ((38, 8, 0), (36, 8, 0), (60, 8, 0)),
    "k_dirt_rows_m<KP, false>": ((38, 8, 0), (36, 8, 0), (60, 8, 0)),
    "k_dirt_cols_m": ((54, 8, 16384), (54, 8, 32768), (76, 6, 65536)),
    "k_dirt_fwd_m": ((16, 8, 0), (26, 8, 0), (42, 8, 0)),
    "k_dirt_bwd_m": ((18, 8, 0), (28, 8, 0), (44, 8, 0)),
}


def _name(mangled):
    """k_dirt_rows_m<2, true> from _Z13k_dirt_rows_mILi2ELb1EEv..., k_dirt_cols_m<8, 4> from ...ILi8ELi4EEv..."""
    m = re.match(r"_Z(\d+)", mangled)
    assert m, mangled
    name, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    assert t, mangled
    args = [("true" if v == "1" else "false") if k == "b" else v for k, v in re.findall(r"L([ib])(\d+)E", t.group(1))]
    return "%s<%s>" % (name, ", ".join(args))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_tiered_direct_block_kernels_have_no_spills_and_are_the_expected_set(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    info = {_name(k): v for k, v in _resources(hipcc, "hip_direct_tm.hip", tmp_path).items()}
    for k, v in info.items():
        assert v["ScratchSize"] == 0, (k, v)
    assert sorted(info) == sorted(EXPECTED)
    with open(os.path.join(ROOT, "lsbench_amd", "csrc", "hip_direct_drv.c")) as f:
        cap = int(re.search(r"#define DIR_LDS_CAP (\d+)u", f.read()).group(1))
    print("recorded:", FOUND)
    print("now, kernel -> (VGPRs, occupancy, static LDS bytes):")
    for k in sorted(info):
        print("  ", k, (info[k]["VGPRs"], info[k]["Occupancy"], info[k]["LDS Size"]))
        # every launch stays inside the 64 KB it gets without asking: the staged window at the cap is cap / kp rows of
        # kp doubles, and k_dirt_cols_m's sixteen partial sums of 64 columns are 8 KB per column of the block
        dynamic = 8 * cap if "k_dirt_rows_m" in k else 0
        assert info[k]["LDS Size"] + dynamic <= 64 * 1024, k
    for kp in WIDTHS:
        for perm in ("true", "false"):
            assert (cap // kp) * kp * 8 + info["k_dirt_rows_m<%d, %s>" % (kp, perm)]["LDS Size"] <= 64 * 1024
        assert info["k_dirt_cols_m<%d, %d>" % (kp, FLIGHT[kp])]["LDS Size"] == 16 * 64 * 8 * kp
