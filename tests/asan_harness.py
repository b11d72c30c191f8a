"""What the host sanitizer tests (test_asan_*.py) share: building a stand-alone driver of tests/asan/ with g++ under
a sanitizer, and running one over length-prefixed input records.  Every driver is a program with its own main; nothing
here is loaded into Python."""
import os
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(HERE, "..", "include")
CSRC = os.path.join(HERE, "..", "sds_amd", "csrc")

ASAN_UBSAN = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1"}


def build(driver, sanitize, extra_flags=()):
    """tests/asan/<driver> compiled with -fsanitize=<sanitize> into a fresh directory; returns the program's path."""
    exe = os.path.join(tempfile.mkdtemp(), os.path.splitext(driver)[0])
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *extra_flags, os.path.join(HERE, "asan", driver), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_records(exe, inputs, env, timeout=600):
    """Writes `inputs` (bytes each) as u32 length + bytes records, runs `exe` on the file with `env` added to the
    environment; the program must exit 0 and print one row of integers per record, which are returned."""
    blob = os.path.join(os.path.dirname(exe), "inputs.bin")
    with open(blob, "wb") as f:
        for x in inputs:
            f.write(struct.pack("<I", len(x)))
            f.write(x)
    r = subprocess.run([exe, blob], capture_output=True, text=True, env=dict(os.environ, **env), timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [list(map(int, l.split())) for l in r.stdout.splitlines()]
    assert len(rows) == len(inputs)
    return rows
