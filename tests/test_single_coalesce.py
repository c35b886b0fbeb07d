"""The leader/follower protocol that coalesces concurrent single Match /
MatchFullSubmap calls (cartographer-1_amd/csrc/single_coalesce.h) and the host
worker pool (host_pool.h), run by a stand-alone program with a fake batch
search: once under AddressSanitizer and UBSan, once under ThreadSanitizer.
CPU only.

ThreadSanitizer comes from the ROCm toolchain's clang++, the compiler hipcc
drives: g++ 11's libtsan does not model the pthread_cond_clockwait behind
wait_until(steady_clock) and reports a double lock that is not there."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "single_coalesce_test.cc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"]
TSAN = ["-fsanitize=thread"]
PROBE = "#include <thread>\nint main() { std::thread([] {}).join(); }\n"


def _run(compiler, sanitize, name):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call([compiler] + FLAGS + sanitize + [SRC, "-o", exe])
    # The program's own watchdog ends it after 120 s; it runs in 3 to 5 s.
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "single coalesce OK" in out.stdout


def _rocm_clangxx():
    """clang++ of the toolchain whose hipcc the library's Makefile uses."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    hipconfig = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "hipconfig")
    try:
        llvm = subprocess.run([hipconfig, "--hipclangpath"], capture_output=True, text=True,
                              timeout=60).stdout.strip()
    except OSError:
        llvm = ""  # no toolchain: the probe says so
    return os.path.join(llvm, "clang++")


def _probe(compiler, sanitize):
    """Why a trivial threaded program does not build or start with these
    flags (no runtime, or an address-space layout it refuses); None if it runs."""
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(BUILD, "sanitizer_probe.cc")
    exe = os.path.join(BUILD, "sanitizer_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    try:
        out = subprocess.run([compiler] + FLAGS + sanitize + [src, "-o", exe],
                             capture_output=True, text=True, timeout=120)
        if out.returncode == 0:
            out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    except OSError as e:
        return f"{compiler}: {e}"
    return None if out.returncode == 0 else (out.stdout + out.stderr).strip() or f"exit {out.returncode}"


def test_protocol_under_asan_ubsan():
    _run("g++", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
         "single_coalesce_test_asan")


def test_protocol_under_tsan():
    clangxx = _rocm_clangxx()
    why = _probe(clangxx, TSAN)
    if why is not None:
        pytest.skip("ThreadSanitizer probe: " + why)
    _run(clangxx, TSAN, "single_coalesce_test_tsan")
