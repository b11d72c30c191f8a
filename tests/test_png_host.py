"""sdsj_png_probe (host header parse, no GPU) against PIL: size, mode <-> colour type and `supported`
for every colour type and depth, interlaced files, APNG, a header cut at every byte and the CRC
cases; sdsj_probe on the same bytes still reports UNSUPPORTED (PNG stays off by default)."""
import io
import struct
import zlib

import pytest
from PIL import Image

from tests import png_synth as S

SUBSET_TYPES = (0, 2, 3, 4, 6)
LEGAL = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16),
         (6, 8), (6, 16)]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# PIL's modes of 8-bit and narrower files (PngImagePlugin._MODES)
MODES = {(0, 1): "1", (0, 2): "L", (0, 4): "L", (0, 8): "L", (2, 8): "RGB", (3, 1): "P", (3, 2): "P", (3, 4): "P",
         (3, 8): "P", (4, 8): "LA", (6, 8): "RGBA"}


def _lib():
    from sds_amd import _lib
    _lib.load()
    return _lib


def _file(ct, depth, w=13, h=7, interlace=0, **kw):
    rowbytes = (w * CHANNELS[ct] * depth + 7) // 8
    raw = b"".join(b"\0" + bytes([(17 * y + 3) & 255] * rowbytes) for y in range(h))
    plte = bytes(range(48)) if ct == 3 else None
    return S.write_png(w, h, ct, zlib.compress(raw), depth=depth, interlace=interlace, plte=plte, **kw)


@pytest.mark.parametrize("ct,depth", LEGAL)
def test_probe_every_colour_type_and_depth(ct, depth):
    L = _lib()
    data = _file(ct, depth)
    st, info = L.png_probe(data)
    im = Image.open(io.BytesIO(data))
    assert (info.width, info.height) == im.size
    assert (info.bit_depth, info.color_type, info.interlace) == (depth, ct, 0)
    if (ct, depth) in MODES:
        assert im.mode == MODES[(ct, depth)]
    want = depth == 8 and ct in SUBSET_TYPES
    assert info.supported == int(want)
    assert st == (L.OK if want else L.UNSUPPORTED)
    assert L.probe(data)[0] == L.UNSUPPORTED


def test_probe_interlaced_and_apng_are_unsupported():
    L = _lib()
    data = _file(2, 8, interlace=1)
    st, info = L.png_probe(data)
    assert Image.open(io.BytesIO(data)).size == (info.width, info.height)
    assert (st, info.supported, info.interlace) == (L.UNSUPPORTED, 0, 1)
    data = _file(2, 8, pre=[(b"acTL", struct.pack(">II", 1, 0))])
    st, info = L.png_probe(data)
    assert (st, info.supported) == (L.UNSUPPORTED, 0)
    assert (info.width, info.height) == (13, 7)
    for d in (data, _file(2, 8, interlace=1)):
        assert L.probe(d)[0] == L.UNSUPPORTED


def test_probe_header_cut_at_every_byte():
    """Up to the first IDAT's header every cut leaves an unreadable file: never `supported`, and PIL
    fails to open it too.  From there on the header is whole."""
    L = _lib()
    data = S.make(13, 7, 3, "mixP", trns=True, text=True)
    first_idat = data.index(b"IDAT") - 4
    for cut in range(len(data)):
        st, info = L.png_probe(data[:cut])
        if cut < first_idat + 12:  # (the probe wants the IDAT's length and type and four more bytes)
            assert st != L.OK and info.supported == 0, cut
            if cut < first_idat + 8:
                with pytest.raises(Exception):
                    Image.open(io.BytesIO(data[:cut]))
        else:
            assert st == L.OK and info.supported == 1, cut
        assert L.probe(data[:cut])[0] == L.UNSUPPORTED


@pytest.mark.parametrize("which", ["IHDR", "PLTE", "tRNS", "tEXt"])
def test_probe_crc_before_idat_is_checked(which):
    L = _lib()
    pre = [(b"tRNS", b"\0\1\2"), (b"tEXt", b"k\0v")]
    z = zlib.compress(b"".join(b"\0" + bytes(13) for _ in range(7)))
    good = S.write_png(13, 7, 3, z, plte=bytes(30), pre=pre)
    bad = S.write_png(13, 7, 3, z, plte=bytes(30), pre=pre, bad_crc=which)
    assert L.png_probe(good)[0] == L.OK
    Image.open(io.BytesIO(good))
    st, info = L.png_probe(bad)
    assert st == L.CORRUPT and info.supported == 0
    with pytest.raises(Exception):
        Image.open(io.BytesIO(bad))


@pytest.mark.parametrize("which", ["IDAT", "IEND"])
def test_probe_crc_of_idat_and_iend_is_not_its_business(which):
    L = _lib()
    data = S.make(13, 7, 2, "mixP", bad_crc=which)
    st, info = L.png_probe(data)
    assert st == L.OK and info.supported == 1
    assert S.pil_outcome(data)[0] == "ok"


def test_probe_arguments_and_other_formats():
    L = _lib()
    assert L.png_probe(b"")[0] == L.UNSUPPORTED
    assert L.png_probe(b"\xff\xd8\xff\xe0" + bytes(20))[0] == L.UNSUPPORTED
    assert L.png_probe(S.SIG)[0] == L.CORRUPT
    assert L.load().sdsj_png_probe(None, 0, None) == L.EINVAL


def test_plan_need_formats_sizes_png_only_when_enabled():
    import ctypes
    L = _lib()
    lib = L.load()
    data = S.make(67, 5, 6, "mixA")
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    need = ctypes.c_int64(-1)
    assert lib.sdsj_plan_need(data, len(data), ctypes.byref(op), ctypes.byref(need)) == L.UNSUPPORTED
    assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), L.FORMAT_JPEG, ctypes.byref(need)) == L.UNSUPPORTED
    assert need.value == 0
    mask = L.FORMAT_JPEG | L.FORMAT_PNG
    assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.OK
    assert need.value >= 5 * (1 + 67 * 4) and need.value % 256 == 0
    assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), 0, ctypes.byref(need)) == L.EINVAL


def test_counter_and_stage_names():
    L = _lib()
    lib = L.load()
    assert L.NUM_COUNTERS == 11 and lib.sdsj_counter_name(10) == b"png"
    names = [lib.sdsj_stage_name(k).decode() for k in range(16)]
    assert names[:13] == ["parse", "plan", "unstuff", "prog", "entspec", "entsync", "entwrite", "idct", "color",
                          "coeffs", "hpass", "vpass", "resample"]
    assert names[13:] == ["png_inflate", "png_unfilter", ""]
