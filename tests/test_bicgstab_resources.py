"""Compile-time guard for the BiCGSTAB sweeps (no GPU needed: hipcc cross-compiles gfx950), in the manner
of test_build_resources.py: every k_bcg_* kernel without scratch, within 64 VGPRs, at occupancy 8 -- what the
PCG sweeps are held to."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not installed")
def test_bicgstab_sweeps_have_no_spills_and_full_occupancy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                        os.path.join(CSRC, "hip_bicgstab.hip"), "-o", str(tmp_path / "hip_bicgstab.o"),
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
    bcg = {k: v for k, v in info.items() if "k_bcg_" in k}
    # the four sweeps of an iteration, the init and the restart in their 16-byte and 8-byte forms + the two
    # one-workgroup state kernels
    for stem, count in (("k_bcg_sI", 2), ("k_bcg_ttI", 2), ("k_bcg_xrI", 2), ("k_bcg_pI", 2), ("k_bcg_initI", 2),
                        ("k_bcg_restartI", 2), ("k_bcg_init_state", 1), ("k_bcg_restart_state", 1)):
        assert len([k for k in bcg if stem in k]) == count, (stem, sorted(bcg))
    assert len(bcg) == 14 and len(info) == 14  # nothing else lives in the file
    for k, v in bcg.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] <= 64, (k, v)
        assert v["Occupancy"] == 8, (k, v)
