"""SDSJ_FORMAT_PNG_META ("png-meta") on the host, no GPU: the mask rules, sdsj_png_probe_formats and
sdsj_plan_need_formats on files with iCCP, zTXt and iTXt chunks and with chunks after the image data, against PIL
on the same bytes.

The anchors (tests/png_meta_synth.py) are the outcomes observed with Pillow 12.2.0.  The rule is one-sided: SDSJ_OK
only where PIL decodes the bytes without raising.  PIL also accepts compressed chunks whose zlib stream is broken
or cut (it swallows zlib.error) and a profile of exactly 1,048,576 bytes; the rule hands those over, and the
anchors say so (native = False, PIL "ok").

Without the bit the probe stops at the first IDAT, as it always has: for a file whose only metadata follows the
image data it still reports SDSJ_OK under mask 3, and the refusal comes from the decode (png_tail_ok,
tests/test_gpu_png_meta.py::test_mask_off).  Every anchor with its metadata before the image data is
SDSJ_UNSUPPORTED under mask 3."""
import ctypes

import pytest

from tests import png_meta_synth as M
from tests import png_synth as S

OP = (32, 32, 1, 1, 0, 0)


def _lib():
    from sds_amd import _lib
    _lib.load()
    return _lib


def _need(L, data, mask):
    op = L.SdsjOp(*OP)
    need = ctypes.c_int64(-1)
    st = L.load().sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need))
    return st, need.value


def test_format_names_and_values():
    L = _lib()
    assert L.FORMAT_PNG_META == 16 and L.FORMATS["png-meta"] == 18
    assert L.format_mask(("jpeg", "png-meta")) == 19 and L.format_mask("png-meta") == 18
    assert L.format_mask(("jpeg", "png-ext", "png-meta")) == 23 and L.format_mask(("png-ext", "png-meta")) == 22
    assert L.format_mask(("jpeg", "png", "png-meta")) == 19
    assert L.format_mask(("jpeg", "png-ext")) == 7 and L.format_mask(None) == 1
    with pytest.raises(ValueError):
        L.format_mask(("jpeg", "png_meta"))


def test_mask_validity():
    L = _lib()
    data = M.rgb53()
    for mask in (16, 17, 8, 15, 20, 21, 32, 51):
        assert _need(L, data, mask)[0] == L.EINVAL, mask
    for mask in (18, 19, 22, 23):
        st, need = _need(L, data, mask)
        assert st == L.OK and need > 0 and need % 256 == 0, mask
        assert L.png_probe(data, mask)[0] == L.OK
    info = L.SdsjPngInfo()
    lib = L.load()
    for mask in (16, 17):  # (the probe wants SDSJ_FORMAT_PNG, as before)
        assert lib.sdsj_png_probe_formats(data, len(data), mask, ctypes.byref(info)) == L.EINVAL


ANCHORS = M.anchors()


@pytest.mark.parametrize("name,data,pil,native", ANCHORS, ids=[a[0] for a in ANCHORS])
def test_anchor(name, data, pil, native):
    """PIL's outcome is the recorded one; native acceptance and hand-over under the mask; the mask without the bit."""
    L = _lib()
    kind, ref = S.pil_outcome(data)
    assert kind == pil, ref
    mask = M.mask_for(name)
    st, info = L.png_probe(data, mask)
    assert (info.width, info.height) == (5, 3)
    if pil == "err":
        assert st != L.OK and info.supported == 0
    assert st == (L.OK if native else L.UNSUPPORTED) and info.supported == int(native)
    assert _need(L, data, mask)[0] == st
    # without the bit: the parent's answer -- the chunks before the image data refuse the file, the probe never
    # looked behind the first IDAT
    st3 = L.png_probe(data, 3)[0]
    assert st3 == L.png_probe(data)[0]
    if name.startswith("post_"):
        assert st3 == L.OK
    else:
        assert st3 == L.UNSUPPORTED
    assert L.png_probe(data, 7)[0] == st3


def test_tIME_after_the_image_data_needs_png_ext_too():
    L = _lib()
    data = dict((a[0], a[1]) for a in ANCHORS)["post_time_ext"]
    assert L.png_probe(data, 23)[0] == L.OK and L.png_probe(data, 19)[0] == L.UNSUPPORTED


def test_realistic_file():
    L = _lib()
    data = M.realistic()
    assert all(t in data for t in (b"iCCP", b"iTXt", b"tEXt", b"tIME"))
    assert S.pil_outcome(data)[0] == "ok"
    st, info = L.png_probe(data, 23)
    assert st == L.OK and (info.width, info.height, info.supported) == (53, 37, 1)
    assert _need(L, data, 23)[0] == L.OK
    assert L.png_probe(data, 19)[0] == L.UNSUPPORTED  # (the tIME)
    for mask in (3, 7):
        assert L.png_probe(data, mask)[0] == L.UNSUPPORTED and _need(L, data, mask) == (L.UNSUPPORTED, 0)


def test_corpus_is_native_and_mutations_never_beat_pil():
    """Every chunk form of the corpus is accepted on both sides of the image data; over the corpus, the anchors and
    the single-byte mutations of the chunk payloads, SDSJ_OK implies that PIL decodes the file; planning agrees."""
    L = _lib()
    corpus, muts = M.corpus(), M.mutations()
    assert len(muts) >= 200
    for name, data in corpus:
        assert L.png_probe(data, 19)[0] == L.OK, name
        if name.endswith("_pre"):
            assert L.png_probe(data, 3)[0] == L.UNSUPPORTED or name == "text_pre", name
    n_ok = n_refused = 0
    for name, data in corpus + muts + [(a[0], a[1]) for a in ANCHORS]:
        for mask in (19, 23):
            st = L.png_probe(data, mask)[0]
            assert _need(L, data, mask)[0] == st, (name, mask)
            if st == L.OK:
                assert S.pil_outcome(data)[0] == "ok", (name, mask)
                n_ok += 1
            else:
                n_refused += 1
    assert n_ok > 100 and n_refused > 50  # (both branches ran)


def test_structure_cases_the_rule_refuses():
    L = _lib()
    z = S.zstream(b"text")
    cases = {
        "ztxt_method1": [(b"zTXt", M.ztxt(z, method=1))],
        "ztxt_empty_stream": [(b"zTXt", b"k\0\0")],           # PIL: zlib gives nothing, accepted; the size rule: no stream
        "iccp_method_missing": [(b"iCCP", b"icc\0")],
        "iccp_preset_dictionary": [(b"iCCP", M.iccp(b"\x78\x20" + z[2:]))],
        "text_too_long": [(b"tEXt", b"k\0" + b"v" * 65536)],
    }
    for name, pre in cases.items():
        for data in (M.rgb53(pre), M.rgb53(post=pre)):
            st = L.png_probe(data, 23)[0]
            assert st == L.UNSUPPORTED, name
    # a bad CRC before the image data is an error in PIL and here; after it nobody looks
    bad = M.rgb53([(b"iCCP", M.iccp(z))], bad_crc="iCCP")
    assert L.png_probe(bad, 19)[0] == L.CORRUPT and S.pil_outcome(bad)[0] == "err"
    late = M.rgb53(post=[(b"iCCP", M.iccp(z))], bad_crc="iCCP")
    assert L.png_probe(late, 19)[0] == L.OK and S.pil_outcome(late)[0] == "ok"


def test_tail_walk_edges():
    """IDAT after another chunk, APNG chunks, critical and non-letter types, PLTE / IHDR, a payload that leaves the
    input, IEND with a payload: PIL decides.  The input ending after a CRC or inside the next header: accepted, as PIL
    stops on the short read."""
    L = _lib()
    good = M.rgb53(post=[(b"tEXt", b"k\0v")])
    assert L.png_probe(good, 19)[0] == L.OK
    iend = good.rindex(b"IEND") - 4
    for cut in range(iend, len(good) + 1):  # the last chunk cut anywhere
        data = good[:cut]
        st = L.png_probe(data, 19)[0]
        assert st == L.OK, cut
        assert S.pil_outcome(data)[0] == "ok", cut
    text = good.rindex(b"tEXt") - 4
    for cut in range(text + 8, iend - 4):  # the tEXt payload leaves the input
        st = L.png_probe(good[:cut], 19)[0]
        assert st == L.UNSUPPORTED, cut
    z = S.zstream(S.rgb_raw(5, 3, sched="mixP"))
    for post in ([(b"tEXt", b"k\0v"), (b"IDAT", b"")], [(b"fcTL", bytes(26))], [(b"fdAT", bytes(8))], [(b"acTL", bytes(8))],
                 [(b"ABCD", b"x")], [(b"ab{d", b"x")], [(b"PLTE", bytes(3))], [(b"IHDR", bytes(13))], [(b"tIME", M.TIME)]):
        data = S.write_png(5, 3, 2, z, post=post)
        assert L.png_probe(data, 19)[0] == L.UNSUPPORTED, post
    data = S.write_png(5, 3, 2, z, iend=False) + S.chunk(b"IEND", b"x")
    assert L.png_probe(data, 19)[0] == L.UNSUPPORTED
    # IDAT chunks the zlib stream does not need are skipped, as without the bit
    data = S.write_png(5, 3, 2, z, post=[(b"IDAT", b"extra"), (b"tEXt", b"k\0v")])
    assert L.png_probe(data, 19)[0] == L.OK and S.pil_outcome(data)[0] == "ok"
