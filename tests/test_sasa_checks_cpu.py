"""The argument rules of the SASA entry points (rustsasa_amd/csrc/sasa_checks.h), exercised by a stand-alone program
(tests/c/sasa_checks_test.cpp) that the host compiler builds with the address and undefined-behaviour sanitizers.  No
GPU, no library: the header is plain host C++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sasa_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sasa_checks_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "rustsasa_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "sasa_checks_test.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "sasa checks ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
