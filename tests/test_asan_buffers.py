"""Host sanitizer runs of the engine's owners and staging threads, as stand-alone programs (their own
main, no GPU): tests/asan/buffers_driver.cpp under AddressSanitizer + UBSan with leak detection --
Buf / Handle of sds_amd/csrc/sdsj_buffers.h with a counting allocator that fails a chosen allocation
(frees equal successful allocations, nothing is freed twice, a failed buffer is empty) and the staging
layout (16-byte aligned, ordered, disjoint regions) -- and tests/asan/stage_pool_driver.cpp under
ThreadSanitizer: 200 parallel_for calls on sds_amd/csrc/sdsj_stage_pool.h, then its destruction."""
import os
import shutil
import subprocess

import pytest

from tests import asan_harness as H

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build_and_run(driver, sanitize, env):
    exe = H.build(driver, sanitize, ("-pthread", "-Wall", "-Werror", "-I", H.CSRC))
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok", r.stdout[-2000:]


def test_buffers_and_layout_under_asan_and_ubsan():
    _build_and_run("buffers_driver.cpp", "address,undefined", H.ASAN_UBSAN)


def test_stage_pool_under_tsan():
    _build_and_run("stage_pool_driver.cpp", "thread", {"TSAN_OPTIONS": "halt_on_error=1:exitcode=66"})
