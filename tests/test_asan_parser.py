"""Host AddressSanitizer + UBSan build of the shared JPEG header parser (SURVEY.md §5 "race
detection / sanitizers": the reference has none; the parser in sds_amd/csrc/sdsj_common.h runs on the
host in sdsj_probe and on the device in k_parse).  Every G1/G5 golden JPEG, truncated at every byte
of its headers and with bytes of its headers overwritten, goes through the sanitized parser; the
build aborts on any out-of-bounds read or undefined behaviour.  Statuses must equal the product
library's sdsj_probe (same parser, no sanitizer) where it is loadable."""
import os
import shutil
import struct
import subprocess
import tempfile

import pytest

from tests.parser_inputs import inputs as _inputs

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "asan", "parse_driver.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_parser_under_asan_and_ubsan():
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "parse_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "..", "include"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    inputs = _inputs()
    blob = os.path.join(d, "inputs.bin")
    with open(blob, "wb") as f:
        for x in inputs:
            f.write(struct.pack("<I", len(x)))
            f.write(x)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, blob], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [list(map(int, l.split())) for l in r.stdout.splitlines()]
    assert len(rows) == len(inputs)
    assert all(row[0] != 99 for row in rows)
    try:
        from sds_amd import _lib
        _lib.load()
    except Exception:  # noqa: BLE001  (the product library is not built: statuses are checked above only)
        return
    for x, row in zip(inputs, rows):
        st, info = _lib.probe(x)
        assert st == row[0], (len(x), st, row[0])
        if st == 0:
            assert (info.width, info.height, info.ncomp) == tuple(row[1:4])
