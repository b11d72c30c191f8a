"""The host side of the opt-in "gif" format (no GPU): the mask, sdsj_gif_probe against PIL and the writer's
own parameters on the three fixture groups, sdsj_plan_need_formats, and sdsj_probe on the same bytes,
which still reports UNSUPPORTED (GIF stays off by default)."""
import ctypes
import io
import struct

import numpy as np
import pytest
from PIL import Image

from tests import gif_synth as S


def _lib():
    from sds_amd import _lib
    _lib.load()
    return _lib


def test_format_names_and_masks():
    L = _lib()
    assert L.FORMATS["gif"] == 256 == L.FORMAT_GIF
    assert L.format_mask(("gif",)) == 256
    assert L.format_mask(("jpeg", "gif")) == 257
    assert L.format_mask(("jpeg", "png", "gif")) == 259
    assert L.format_mask(("gif", "png-ext", "jpeg-scans")) == 256 | 2 | 4 | 1 | 128
    assert L.format_mask(None) == 1
    with pytest.raises(ValueError):
        L.format_mask(("gif89",))


def test_probe_native_files_against_pil():
    L = _lib()
    for name, data in S.native():
        st, info = L.gif_probe(data)
        assert st == L.OK and info.supported == 1, name
        im = Image.open(io.BytesIO(data))
        assert (info.width, info.height) == im.size, name
        assert 0 < info.frame_w and info.frame_x + info.frame_w <= info.width, name
        assert 0 < info.frame_h and info.frame_y + info.frame_h <= info.height, name
        assert 2 <= info.min_code_size <= 8, name
        # the effective table: without one (a grey ramp counts as none) PIL's loaded image is mode L
        im.load()
        assert (info.table_entries == 0) == (im.im.mode == "L"), (name, im.im.mode)


def test_probe_fields_follow_the_writer():
    L = _lib()
    t16 = S.colour_table(16, 1)
    sub = S.indices(5, 4, 16, 4)
    st, info = L.gif_probe(S.write_gif((20, 10), sub, gct=S.colour_table(256), lct=t16, frame_xy=(3, 2), interlace=True,
                                       min_code=4, exts=[S.comment(), S.gce(7)]))
    assert st == L.OK
    assert (info.width, info.height, info.frame_x, info.frame_y, info.frame_w, info.frame_h) == (20, 10, 3, 2, 5, 4)
    assert (info.interlace, info.table_entries, info.min_code_size, info.supported) == (1, 16, 4, 1)
    st, info = L.gif_probe(S.write_gif((20, 10), sub, gct=S.colour_table(256), lct=S.grey_table(16), min_code=4))
    assert (st, info.table_entries, info.interlace) == (L.OK, 256, 0)  # (a local ramp leaves the global table in force)
    st, info = L.gif_probe(S.write_gif((20, 10), sub, gct=S.grey_table(256), lct=S.grey_table(16), min_code=4))
    assert (st, info.table_entries) == (L.OK, 0)
    st, info = L.gif_probe(S.write_gif((20, 10), sub, min_code=4, version=b"87a"))
    assert (st, info.table_entries) == (L.OK, 0)


def test_probe_refused_and_damaged_files():
    L = _lib()
    for name, data in S.refused():
        st, info = L.gif_probe(data)
        assert st == L.UNSUPPORTED and info.supported == 0, name
        assert (info.width, info.height) == struct.unpack("<HH", data[6:10]), name
    for name, data in S.damaged():
        st, info = L.gif_probe(data)
        # the header gives away only some of them; the LZW data is the device's to judge
        assert st == (L.CORRUPT if name.endswith("_hdr") else L.OK), name
        assert info.supported == (st == L.OK), name


def test_probe_header_cut_at_every_byte_and_unknown_blocks():
    L = _lib()
    exts = [S.netscape(), S.gce(1), S.comment(), S.plain_text()]
    kw = dict(gct=S.colour_table(4, 2), lct=S.colour_table(8, 3), min_code=3)
    data = S.write_gif((9, 5), S.indices(9, 5, 4, 2), exts=exts, **kw)
    # screen, 4-entry global table, extensions, descriptor, 8-entry local table, the code size byte
    first_data = 13 + 12 + sum(map(len, exts)) + 10 + 24 + 1
    assert L.gif_probe(data)[0] == L.OK
    for cut in range(first_data):
        st, _ = L.gif_probe(data[:cut])
        assert st in (L.UNSUPPORTED, L.CORRUPT), cut
    assert L.gif_probe(data[:first_data])[0] == L.OK  # (the data itself is not the probe's business)
    unknown = S.write_gif((9, 5), S.indices(9, 5, 4, 2), exts=[b"\x21\x77" + S.sub_blocks(b"x")], **kw)
    assert L.gif_probe(unknown)[0] == L.UNSUPPORTED
    intro = bytearray(data)
    intro[13 + 12] = 0x3F  # the first block introducer after the 4-entry global table
    assert L.gif_probe(bytes(intro))[0] == L.UNSUPPORTED
    st, _ = L.gif_probe(b"\x89PNG\r\n\x1a\n" + bytes(40))
    assert st == L.UNSUPPORTED
    info = L.SdsjGifInfo()
    assert L.load().sdsj_gif_probe(None, 0, ctypes.byref(info)) == L.EINVAL


def test_plan_need_formats_sizes_gif_only_under_the_bit():
    L = _lib()
    lib = L.load()
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    need = ctypes.c_int64(-1)
    for name, data in S.native():
        st, info = L.gif_probe(data)
        for mask in (256, 257, 259):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.OK, name
            assert need.value % 256 == 0 and need.value >= info.width * info.height, name
        for mask in (1, 3, 1 | 2 | 4 | 16 | 64 | 128):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.UNSUPPORTED
            assert need.value == 0, name
        assert lib.sdsj_plan_need(data, len(data), ctypes.byref(op), ctypes.byref(need)) == L.UNSUPPORTED
    for name, data in S.refused():
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), 257, ctypes.byref(need)) == L.UNSUPPORTED, name
    data = S.native()[0][1]
    for mask in (0, 8, 32, 256 | 8, 256 | 32, 256 | 4, 256 | 16, 256 | 64, 256 | 128, 512, 1024):
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.EINVAL, mask
    # a JPEG under a mask that also names GIF is sized as before
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG")
    a, b = ctypes.c_int64(), ctypes.c_int64()
    jpg = buf.getvalue()
    assert lib.sdsj_plan_need_formats(jpg, len(jpg), ctypes.byref(op), 1, ctypes.byref(a)) == L.OK
    assert lib.sdsj_plan_need_formats(jpg, len(jpg), ctypes.byref(op), 257, ctypes.byref(b)) == L.OK
    assert a.value == b.value > 0


def test_sdsj_probe_still_reports_gif_unsupported():
    L = _lib()
    for name, data in S.native()[:6] + S.refused() + S.damaged():
        st, info = L.probe(data)
        assert st == L.UNSUPPORTED and info.supported == 0, name
        st, info = L.png_probe(data)
        assert st == L.UNSUPPORTED, name
