"""The host side of the tiered direct solver (lsb_direct.c: ordering, symbolic count, tiered factor) under ASan + UBSan,
as a stand-alone program (tests/asan_direct_tiers.c) on the CPU: the two reference matrices with long coupling rows,
a 2-D and a 3-D grid whose tiers end off every multiple of 64, the matrix without edges (the tiers collapse), the
indefinite 2 x 2 (refused in every tier count), a path of three rows (a tier of one row) and one row on its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsbench_amd", "csrc")
CASES = ["xn3b_A_18", "tj7a_A_12", "synth:lap2d:nx=24,ny=20", "synth:lap3d:nx=9,ny=8,nz=7", "I1_05x05", "A0_02x02",
         "synth:lap2d:nx=3,ny=1"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_tiered_factor_under_asan_ubsan(tmp_path, matrix_path):
    exe = str(tmp_path / "asan_direct_tiers")
    r = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-fopenmp",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "asan_direct_tiers.c"),
                        os.path.join(CSRC, "lsb_direct.c"), os.path.join(CSRC, "lsb_operator.c"),
                        os.path.join(CSRC, "lsb_synth.c"), os.path.join(CSRC, "lsb_matrix.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args = [c if c.startswith("synth:") else matrix_path(c) for c in CASES]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", OMP_NUM_THREADS="4")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("ok ") == len(CASES) + 1 and "FAILED" not in r.stdout
    assert r.stdout.count("refused") == 1  # the indefinite one alone
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
