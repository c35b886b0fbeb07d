"""The v4/v5 search kernel's interleaved work queues: the host's schedule
builder (cartographer-1_amd/csrc/csm_schedule.h) and the slot decode the
kernel's claim runs (csm_device.h DecodeSlot), exercised together by a
stand-alone program under AddressSanitizer and UBSan. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "schedule_test.cc")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "schedule_test")


def test_every_pair_chunk_once_and_empty_slots_as_reported():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schedule OK" in out.stdout
