"""Host AddressSanitizer + UBSan run of the shared TIFF core (sds_amd/csrc/sdsj_tiff.h), the functions that take
every correctness and bounds decision of k_parse's TIFF branch, k_tiff_copy, k_tiff_lzw, k_tiff_inflate and
k_tiff_rgb.  A stand-alone program (tests/asan/tiff_driver.cpp, its own main) decodes the three fixture groups, every
truncation of the files under 400 bytes, 400 seeded single-byte overwrites and a few foreign inputs with a serial
decoder built from those functions.  It must exit cleanly; the native group must decode to the expected pixels; for
every other input a status of OK is allowed only where PIL decodes the same bytes without raising, and then the RGB
must equal PIL's.  This is where bit-exactness against PIL / libtiff is established before any GPU run."""
import shutil

import numpy as np
import pytest

from tests import asan_harness as H
from tests import tiff_synth as S
from tests.test_asan_png import fnv1a64


def _inputs():
    native = S.native()
    out = [(n, d, r) for n, d, r in native] + [(n, d, None) for n, d in S.refused() + S.damaged()]
    small = [d for _, d, _ in native if len(d) < 400]
    assert len(small) >= 4
    for k, d in enumerate(small):
        for cut in range(len(d)):
            out.append((f"cut{k}_{cut}", d[:cut], None))
    rng = np.random.default_rng(31)
    pool = [d for _, d, _ in native if len(d) < 3000]
    for k in range(400):
        b = bytearray(pool[int(rng.integers(0, len(pool)))])
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((f"mut{k}", bytes(b), None))
    out += [("empty", b"", None), ("sig_only_ii", b"II*\0", None), ("sig_only_mm", b"MM\0*\0\0\0\x08", None),
            ("ifd_at_end", b"II*\0\x08\0\0\0", None), ("png", b"\x89PNG\r\n\x1a\n" + bytes(30), None),
            ("jpeg", b"\xff\xd8\xff\xe0" + bytes(30), None)]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tiff_core_under_asan_and_ubsan():
    exe = H.build("tiff_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    inputs = _inputs()
    rows = H.run_records(exe, [x for _, x, _ in inputs], H.ASAN_UBSAN)
    assert len(rows) == len(inputs)
    n_ok = 0
    for (name, data, must), (st, w, h, hsh) in zip(inputs, rows):
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


# tags the parse names, tags it lets pass, and tags libtiff knows that it does not
_TAGS = (254, 255, 256, 257, 258, 259, 262, 263, 266, 269, 270, 273, 274, 277, 278, 279, 280, 281, 282, 283, 284, 296, 297, 301,
         305, 306, 315, 317, 318, 319, 320, 332, 333, 334, 336, 337, 338, 339, 340, 341, 700, 34675, 65000)


def _entry_mutations(d):
    """Every IFD entry of `d` with its tag renumbered (to each of _TAGS between its neighbours, so the order stays),
    its type, its count, its value field, and type and count together replaced."""
    import struct
    bo = "<" if d[:2] == b"II" else ">"
    ifd = struct.unpack(bo + "I", d[4:8])[0]
    n = struct.unpack(bo + "H", d[ifd:ifd + 2])[0]
    out = []
    for k in range(n):
        e = ifd + 2 + 12 * k
        tag, ty, cnt = struct.unpack(bo + "HHI", d[e:e + 8])
        lo = struct.unpack(bo + "H", d[e - 12:e - 10])[0] if k else 0
        hi = struct.unpack(bo + "H", d[e + 12:e + 14])[0] if k < n - 1 else 65536
        out += [d[:e] + struct.pack(bo + "H", t) + d[e + 2:] for t in _TAGS if lo < t < hi and t != tag]
        out += [d[:e + 2] + struct.pack(bo + "H", t) + d[e + 4:] for t in range(1, 14) if t != ty]
        out += [d[:e + 4] + struct.pack(bo + "I", c) + d[e + 8:] for c in (0, 1, 2, 3, 4, 5, 8, 20, 768) if c != cnt]
        out += [d[:e + 8] + struct.pack(bo + "I", v) + d[e + 12:] for v in (0, 1, 2, 3, 4, 7, 8, 255, 65535)]
        out += [d[:e + 2] + struct.pack(bo + "HI", t, c) + d[e + 8:] for t in (1, 3, 4) for c in (1, 2, 3, 4)]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_directory_entries_changed_one_field_at_a_time():
    """libtiff reads the whole directory of a compressed file and fails on entries whose type or count it rejects, also
    of tags that never reach the pixels.  Every entry of eight fixtures (each compression, an extra sample, a ColorMap,
    SampleFormat, the passive tags, both byte orders) with one field changed: SDSJ_OK only where PIL opens the file, to
    the same pixels."""
    nat = dict((n, d) for n, d, _ in S.native())
    inputs = []
    for name in ("rgb_lzw", "rgba_deflate", "p_packbits", "la_none", "cmyk_deflate_pred", "sample_format_each", "passive_tags",
                 "strips40_packbits"):
        inputs += _entry_mutations(nat[name])
    assert len(inputs) > 4000
    rows = H.run_records(H.build("tiff_driver.cpp", "address,undefined", ("-I", H.INCLUDE)), inputs, H.ASAN_UBSAN)
    n_ok = 0
    for data, (st, w, h, hsh) in zip(inputs, rows):
        if st == 0:
            kind, ref = S.pil_outcome(data)
            assert kind == "ok" and ref.shape == (h, w, 3), (kind, ref)
            assert fnv1a64(ref.tobytes()) == hsh
            n_ok += 1
    assert n_ok > 100  # (harmless changes -- a resolution's value, a description's length -- still decode)
