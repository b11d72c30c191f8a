"""Host AddressSanitizer + UBSan run of the shared PNG core under SDSJ_FORMAT_PNG_META: png_parse with the mask,
png_meta_check, the count-only inflate and the walk over the chunks after the image data -- the functions that take
every decision of k_parse and k_png_meta.  A stand-alone program (tests/asan/png_meta_driver.cpp, its own main) runs
them over the corpus of tests/png_meta_synth.py, the anchors, the truncations of small cases at every byte of their
chunk regions and the single-byte mutations.  It must exit cleanly; every corpus case must be accepted; a status of
OK is allowed only where PIL decodes the same bytes; and the library's probe gives the same statuses."""
import shutil

import pytest

from tests import asan_harness as H
from tests import png_meta_synth as M
from tests import png_synth as S


def _inputs():
    out = [(n, d, True) for n, d in M.corpus()] + [(a[0], a[1], False) for a in M.anchors()]
    out.append(("realistic", M.realistic(), False))
    out += [(n, d, False) for n, d in M.mutations()]
    z = S.zstream(b"compressed text " * 9)
    small = [M.rgb53([(b"iCCP", M.iccp(z)), (b"iTXt", M.itxt(z, comp=1))], [(b"zTXt", M.ztxt(z)), (b"tEXt", b"k\0v")], idat_sizes=[7]),
             M.meta_file(1, 1, 3)]
    for k, d in enumerate(small):
        first_idat = d.index(b"IDAT") - 4
        last_idat = d.rindex(b"IDAT") - 4
        # every byte of the chunks before the first IDAT (and its header), and of everything after the last one
        for cut in list(range(8, first_idat + 13)) + list(range(last_idat, len(d))):
            out.append((f"cut{k}_{cut}", d[:cut], False))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_png_meta_core_under_asan_and_ubsan():
    exe = H.build("png_meta_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    inputs = _inputs()
    rows = H.run_records(exe, [x for _, x, _ in inputs], H.ASAN_UBSAN)
    from sds_amd import _lib as L
    n_ok = 0
    for (name, data, must), (st19, st23, w, h) in zip(inputs, rows):
        if must:
            assert st19 == 0 and st23 == 0, (name, st19, st23)
        if st19 == 0:
            assert st23 == 0, name  # (the wider mask accepts no less)
        if st23 == 0:
            assert S.pil_outcome(data)[0] == "ok", name
            n_ok += 1
        assert L.png_probe(data, 19)[0] == st19 and L.png_probe(data, 23)[0] == st23, name
    assert n_ok >= sum(1 for _, _, m in inputs if m)
