"""Host AddressSanitizer + UBSan run of the shared GIF core (sds_amd/csrc/sdsj_gif.h), the functions that
take every correctness and bounds decision of k_parse's GIF branch, k_gif_lzw and k_gif_rgb.  A stand-alone
program (tests/asan/gif_driver.cpp, its own main) decodes the three fixture groups, every truncation of the
small files, seeded single-byte overwrites and a few foreign inputs with a serial decoder built from those
functions.  It must exit cleanly; the native group must decode; a status of OK is allowed only where PIL
decodes the same bytes without raising, and then the RGB must equal PIL's."""
import shutil

import numpy as np
import pytest

from tests import asan_harness as H
from tests import gif_synth as S
from tests.test_asan_png import fnv1a64


def _inputs():
    native = S.native()
    out = [(n, d, True) for n, d in native] + [(n, d, False) for n, d in S.refused() + S.damaged()]
    for k, d in enumerate(d for _, d in native if len(d) < 400):
        for cut in range(len(d)):
            out.append((f"cut{k}_{cut}", d[:cut], False))
    rng = np.random.default_rng(23)
    pool = [d for _, d in native if len(d) < 3000]
    for k in range(400):
        b = bytearray(pool[int(rng.integers(0, len(pool)))])
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((f"mut{k}", bytes(b), False))
    out += [("empty", b"", False), ("sig_only", b"GIF89a", False), ("jpeg", b"\xff\xd8\xff\xe0" + bytes(30), False)]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_gif_core_under_asan_and_ubsan():
    exe = H.build("gif_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
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
