"""Host AddressSanitizer + UBSan run of the shared WebP core (sds_amd/csrc/sdsj_webp.h), the functions that
take every correctness and bounds decision of k_parse's WebP branch, k_webp_decode, k_webp_inverse and k_webp_rgb.
A stand-alone program (tests/asan/webp_driver.cpp, its own main) decodes the three fixture groups, every truncation
of the small files, seeded single-byte overwrites and a few foreign inputs with a serial decoder built from those
functions.  It must exit cleanly; the native group must decode to the expected pixels; for every other input a
status of OK is allowed only where PIL decodes the same bytes without raising, and then the RGB must equal PIL's.
This is where bit-exactness against libwebp is established before any GPU run."""
import shutil

import numpy as np
import pytest

from tests import asan_harness as H
from tests import webp_synth as S
from tests.test_asan_png import fnv1a64


def _inputs():
    native = S.native()
    out = [(n, d, r) for n, d, r in native] + [(n, d, None) for n, d in S.refused() + S.damaged()]
    for k, d in enumerate(d for _, d, _ in native if len(d) < 400):
        for cut in range(len(d)):
            out.append((f"cut{k}_{cut}", d[:cut], None))
    rng = np.random.default_rng(29)
    pool = [d for _, d, _ in native if len(d) < 3000]
    for k in range(400):
        b = bytearray(pool[int(rng.integers(0, len(pool)))])
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((f"mut{k}", bytes(b), None))
    out += [("empty", b"", None), ("sig_only", b"RIFF\x04\0\0\0WEBP", None), ("wave", b"RIFF\x20\0\0\0WAVEfmt " + bytes(24), None),
            ("jpeg", b"\xff\xd8\xff\xe0" + bytes(30), None)]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_webp_core_under_asan_and_ubsan():
    exe = H.build("webp_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    inputs = _inputs()
    rows = H.run_records(exe, [x for _, x, _ in inputs], H.ASAN_UBSAN)
    n_ok = 0
    for (name, data, must), (st, w, h, hsh, _) in zip(inputs, rows):
        if must is not None:
            assert st == 0 and (h, w) == must.shape[:2], (name, st)
            assert fnv1a64(must.tobytes()) == hsh, name
            n_ok += 1
        elif st == 0:
            kind, ref = S.pil_outcome(data)
            assert kind == "ok", (name, ref)
            assert ref.shape == (h, w, 3), name
            assert fnv1a64(ref.tobytes()) == hsh, name
            n_ok += 1
    assert n_ok >= sum(1 for _, _, m in inputs if m is not None)
