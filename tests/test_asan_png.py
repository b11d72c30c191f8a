"""Host AddressSanitizer + UBSan run of the shared PNG core (sds_amd/csrc/sdsj_png.h), the functions
that take every correctness and bounds decision of k_png_inflate / k_png_unfilter.  A stand-alone
program (tests/asan/png_driver.cpp, its own main) decodes the whole synthetic corpus, every truncation
of the small cases, seeded single-byte overwrites and the hand-made invalid streams with a serial
decoder built from those functions.  It must exit cleanly; a status of OK is allowed only where PIL
decodes the same bytes without raising, and then the RGB must equal PIL's."""
import shutil

import numpy as np
import pytest

from tests import asan_harness as H
from tests import png_synth as S


def fnv1a64(b: bytes) -> int:
    # vectorised over the prefix products is not possible for FNV; the corpus is small enough
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _inputs():
    native = S.group_types() + S.group_deflate() + S.group_sizes()
    damaged = S.group_damage()
    out = [(n, d, True) for n, d in native] + [(n, d, False) for n, d in damaged]
    small = [d for n, d in native if len(d) < 400][:12] + [S.make(13, 7, 3, "mixP"), S.make(5, 3, 6, "mixA", text=True)]
    for k, d in enumerate(small):
        for cut in range(len(d)):
            out.append((f"cut{k}_{cut}", d[:cut], False))
    rng = np.random.default_rng(17)
    pool = [d for n, d in native if len(d) < 3000]
    for k in range(400):
        b = bytearray(pool[int(rng.integers(0, len(pool)))])
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((f"mut{k}", bytes(b), False))
    out += [("empty", b"", False), ("sig_only", S.SIG, False), ("jpeg", b"\xff\xd8\xff\xe0" + bytes(30), False)]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_png_core_under_asan_and_ubsan():
    exe = H.build("png_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    inputs = _inputs()
    rows = H.run_records(exe, [x for _, x, _ in inputs], H.ASAN_UBSAN)
    n_ok = 0
    for (name, data, must), (st, w, h, hsh) in zip(inputs, rows):
        if must:
            assert st == 0, (name, st)
        if st == 0:
            kind, ref = S.pil_outcome(data)
            assert kind == "ok", (name, ref)
            assert ref.shape == (h, w, 3), name
            assert fnv1a64(ref.tobytes()) == hsh, name
            n_ok += 1
    assert n_ok >= sum(1 for _, _, m in inputs if m)
