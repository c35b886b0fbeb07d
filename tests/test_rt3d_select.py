"""Which RTCSM3D kernel the host selects for a brick, a window and a cap
(cartographer-1_amd/csrc/rt3d_select.h), checked at its thresholds by a
stand-alone program under AddressSanitizer and UBSan. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rt3d_select_test.cc")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "rt3d_select_test")


def test_kernel_choice_at_its_thresholds():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rt3d select OK" in out.stdout
