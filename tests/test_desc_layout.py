"""The ctypes mirror of ``sdsj::ImgDesc`` (tests/gpu_debug.py) against the struct itself.

A few-line host program, generated from the mirror's own field lists, is compiled against
sds_amd/csrc/sdsj_common.h and prints ``sizeof`` of the struct and ``offsetof`` / ``sizeof`` of every
field the mirror names; the test compares them with ctypes.  A field added to the struct without the
mirror changes ``sizeof(sdsj::ImgDesc)`` (or moves a later field) and fails here, on the CPU, instead of
in ``gpu_debug.snapshot`` on the first GPU run that needs it."""
import ctypes
import os
import shutil
import subprocess
import tempfile

from tests.gpu_debug import CompDescC, ImgDescC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _program(pairs) -> str:
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "sdsj_common.h"', "int main() {"]
    for cname, mirror in pairs:
        lines.append(f'  printf("{cname} sizeof %zu 0\\n", sizeof(sdsj::{cname}));')
        for name, _ in mirror._fields_:
            lines.append(f'  printf("{cname} {name} %zu %zu\\n", offsetof(sdsj::{cname}, {name}), '
                         f"sizeof(((sdsj::{cname}*)0)->{name}));")
    lines += ["  return 0;", "}"]
    return "\n".join(lines) + "\n"


def test_imgdesc_mirror_matches_the_struct():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to check the descriptor mirror"
    pairs = [("CompDesc", CompDescC), ("ImgDesc", ImgDescC)]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write(_program(pairs))
        r = subprocess.run([cxx, "-std=c++17", "-I", os.path.join(REPO, "include"),
                            "-I", os.path.join(REPO, "sds_amd", "csrc"), src, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]  # (a field the mirror names but the struct lacks fails here)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        cname, name, a, b = line.split()
        got[(cname, name)] = (int(a), int(b))
    for cname, mirror in pairs:
        assert got[(cname, "sizeof")][0] == ctypes.sizeof(mirror), \
            f"sizeof(sdsj::{cname}) = {got[(cname, 'sizeof')][0]}, the mirror has {ctypes.sizeof(mirror)}"
        for name, ctype in mirror._fields_:
            fd = getattr(mirror, name)
            assert got[(cname, name)] == (fd.offset, fd.size), \
                f"{cname}.{name}: struct (offset, size) {got[(cname, name)]}, mirror {(fd.offset, fd.size)}"
            assert fd.size == ctypes.sizeof(ctype)
