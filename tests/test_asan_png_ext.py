"""Host AddressSanitizer + UBSan run of the shared PNG core under the full format mask (SDSJ_FORMAT_PNG |
SDSJ_FORMAT_PNG_EXT): png_parse with the mask, png_layout, the 64-bit png_recon and png_rgb_ext, the
functions that take every correctness and bounds decision of k_png_inflate / k_png_unfilter_ext.  A
stand-alone program (tests/asan/png_ext_driver.cpp, its own main) decodes the ext corpus, every truncation
of its small cases, seeded single-byte overwrites and the damaged inputs with a serial decoder built from
those functions.  It must exit cleanly; every corpus case must decode, and a status of OK is allowed only
where PIL decodes the same bytes without raising, and then the RGB must equal PIL's."""
import shutil

import numpy as np
import pytest

from tests import asan_harness as H
from tests import png_ext_synth as E
from tests import png_synth as S
from tests.test_asan_png import fnv1a64


def _inputs():
    native = E.group_all()
    damaged = S.group_damage() + E.group_ext_damage()
    out = [(n, d, True) for n, d in native] + [(n, d, False) for n, d in damaged]
    # one small case per kind: Adam7 8-bit RGB, 1-bit gray, 2-bit palette Adam7, RGBA 16 Adam7, an ancillary chunk
    small = [E.make(5, 7, 2, 8, 1, "mixP")[0], E.make(13, 7, 0, 1, 0, "mixA")[0], E.make(9, 9, 3, 2, 1, "mixU", plte_n=3)[0],
             E.make(5, 7, 6, 16, 1, "all4")[0], E.with_chunk(*E.ANCILLARY[0])]
    for k, d in enumerate(small):
        for cut in range(len(d)):
            out.append((f"cut{k}_{cut}", d[:cut], False))
    rng = np.random.default_rng(23)
    pool = [d for n, d in native if len(d) < 3000]
    for k in range(400):
        b = bytearray(pool[int(rng.integers(0, len(pool)))])
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((f"mut{k}", bytes(b), False))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_png_ext_core_under_asan_and_ubsan():
    exe = H.build("png_ext_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
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
