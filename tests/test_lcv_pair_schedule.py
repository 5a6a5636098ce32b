"""The pair schedule of the single-precision likelihood evaluation of one-row fit workgroups (csrc/nbp_lcv_pairs.h), enumerated
on the host for every N from 2 to 320 by a stand-alone C++ program (lcv_pair_schedule_check.cpp): every unordered pair of points
in full chunks is visited exactly once, every pair with the partial chunk once from each side, no point meets itself, and
every travelling partner sum ends in the LDS entry of its own point, one writer per entry."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "incrementalinference.jl_amd", "csrc")


def test_every_pair_once_and_every_partner_sum_home(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "lcv_pair_schedule_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "lcv_pair_schedule_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok: 193 sizes" in out.stdout
