"""Host sanitizer runs of the engine's owners and staging threads, as stand-alone programs (their own
main, no GPU): tests/asan/buffers_driver.cpp under AddressSanitizer + UBSan with leak detection --
Buf / Handle of sds_amd/csrc/sdsj_buffers.h with a counting allocator that fails a chosen allocation
(frees equal successful allocations, nothing is freed twice, a failed buffer is empty) and the staging
layout (16-byte aligned, ordered, disjoint regions) -- and tests/asan/stage_pool_driver.cpp under
ThreadSanitizer: 200 parallel_for calls on sds_amd/csrc/sdsj_stage_pool.h, then its destruction."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sds_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build_and_run(driver, sanitize, env):
    exe = os.path.join(tempfile.mkdtemp(), "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Werror", "-I", CSRC,
                        os.path.join(HERE, "asan", driver), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok", r.stdout[-2000:]


def test_buffers_and_layout_under_asan_and_ubsan():
    _build_and_run("buffers_driver.cpp", "address,undefined",
                   {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1"})


def test_stage_pool_under_tsan():
    _build_and_run("stage_pool_driver.cpp", "thread", {"TSAN_OPTIONS": "halt_on_error=1:exitcode=66"})
