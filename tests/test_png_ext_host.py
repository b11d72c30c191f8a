"""The wider PNG subset (SDSJ_FORMAT_PNG_EXT, "png-ext") on the host, no GPU: sdsj_png_probe_formats against
sdsj_png_probe for every legal (colour type, depth) pair with and without interlace, the mask rules, host
planning of an Adam7 16-bit file, and the ancillary chunks before the image data against PIL."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

from tests import png_ext_synth as E
from tests import png_synth as S
from tests.test_png_host import LEGAL, _file


def _lib():
    from sds_amd import _lib
    _lib.load()
    return _lib


def _info(i):
    return (i.width, i.height, i.bit_depth, i.color_type, i.interlace, i.supported)


def test_format_names():
    L = _lib()
    assert (L.FORMAT_JPEG, L.FORMAT_PNG, L.FORMAT_PNG_EXT) == (1, 2, 4)
    assert L.format_mask(("jpeg", "png-ext")) == 7 and L.format_mask("png-ext") == 6
    assert L.format_mask(("jpeg", "png")) == 3 and L.format_mask(None) == 1
    with pytest.raises(ValueError):
        L.format_mask(("jpeg", "png_ext"))


@pytest.mark.parametrize("interlace", [0, 1])
@pytest.mark.parametrize("ct,depth", LEGAL)
def test_probe_formats_every_colour_type_and_depth(ct, depth, interlace):
    L = _lib()
    data = E.make(13, 7, ct, depth, interlace, "mixP", plte_n=2 if ct == 3 else None)[0]
    Image.open(io.BytesIO(data)).convert("RGB")
    full = L.FORMAT_JPEG | L.FORMAT_PNG | L.FORMAT_PNG_EXT
    st, info = L.png_probe(data, full)
    assert st == L.OK and _info(info) == (13, 7, depth, ct, interlace, 1)
    assert L.png_probe(data, L.FORMAT_PNG | L.FORMAT_PNG_EXT)[0] == L.OK
    # without the bit: exactly sdsj_png_probe, which is what it was
    st0, info0 = L.png_probe(data)
    base = depth == 8 and not interlace
    assert st0 == (L.OK if base else L.UNSUPPORTED) and _info(info0) == (13, 7, depth, ct, interlace, int(base))
    for mask in (L.FORMAT_JPEG | L.FORMAT_PNG, L.FORMAT_PNG):
        st1, info1 = L.png_probe(data, mask)
        assert (st1, _info(info1)) == (st0, _info(info0))
    # the zero-filled files of tests/test_png_host.py too
    data = _file(ct, depth, interlace=0)
    assert L.png_probe(data, full)[0] == L.OK


def test_the_bit_alone_is_invalid():
    L = _lib()
    lib = L.load()
    data = E.make(13, 7, 2, 8, 1)[0]
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    need = ctypes.c_int64(-1)
    for mask in (L.FORMAT_PNG_EXT, L.FORMAT_JPEG | L.FORMAT_PNG_EXT, 8, 15):
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.EINVAL
    info = L.SdsjPngInfo()
    assert lib.sdsj_png_probe_formats(data, len(data), L.FORMAT_PNG_EXT, ctypes.byref(info)) == L.EINVAL
    assert lib.sdsj_png_probe_formats(data, len(data), L.FORMAT_JPEG, ctypes.byref(info)) == L.EINVAL
    assert lib.sdsj_png_probe_formats(None, 0, 7, None) == L.EINVAL
    # (sdsj_engine_set_formats needs a live engine: tests/test_gpu_png_ext.py)


def test_plan_need_formats_sizes_an_adam7_rgba16_file():
    L = _lib()
    lib = L.load()
    data = E.make(67, 5, 6, 16, 1, "mixA")[0]
    layout = E.layout_bytes(67, 5, 6, 16, 1)
    assert layout == sum(ph * (1 + pw * 8) for *_, pw, ph in E.passes(67, 5, 1)) > 5 * (1 + 67 * 8)
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    need = ctypes.c_int64(-1)
    full = L.FORMAT_JPEG | L.FORMAT_PNG | L.FORMAT_PNG_EXT
    assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), full, ctypes.byref(need)) == L.OK
    assert need.value >= layout and need.value % 256 == 0
    assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), L.FORMAT_JPEG | L.FORMAT_PNG,
                                      ctypes.byref(need)) == L.UNSUPPORTED
    assert need.value == 0


def test_layout_of_the_synthetic_writer_is_the_specification():
    """Empty passes contribute nothing: 1 x 1 is one pass of one row, 3 x 2 has passes 1, 4, 6 and 7."""
    assert E.layout_bytes(1, 1, 2, 8, 1) == 1 + 3
    assert [(p[0], p[1]) for p in E.passes(3, 2, 1)] == [(0, 0), (2, 0), (1, 0), (0, 1)]
    assert E.layout_bytes(13, 7, 0, 1, 0) == 7 * (1 + 2)


@pytest.mark.parametrize("tag,payload", E.ANCILLARY, ids=[t.decode() for t, _ in E.ANCILLARY])
def test_ancillary_chunks_without_a_handler_are_accepted(tag, payload):
    L = _lib()
    full = L.FORMAT_JPEG | L.FORMAT_PNG | L.FORMAT_PNG_EXT
    good, bad = E.with_chunk(tag, payload), E.with_chunk(tag, payload, bad_crc=True)
    assert L.png_probe(good, full)[0] == L.OK
    assert S.pil_outcome(good)[0] == "ok"
    st, info = L.png_probe(bad, full)
    assert st == L.CORRUPT and info.supported == 0
    assert S.pil_outcome(bad)[0] == "err"
    assert L.png_probe(good)[0] == L.UNSUPPORTED  # the base subset still hands them over


@pytest.mark.parametrize("tag,payload", E.REFUSED, ids=[t.decode() for t, _ in E.REFUSED])
def test_chunks_with_a_handler_and_critical_chunks_stay_with_pil(tag, payload):
    L = _lib()
    st, info = L.png_probe(E.with_chunk(tag, payload), L.FORMAT_JPEG | L.FORMAT_PNG | L.FORMAT_PNG_EXT)
    assert st == L.UNSUPPORTED and info.supported == 0


def test_a_chunk_type_that_is_not_four_letters_stays_with_pil():
    L = _lib()
    data = E.with_chunk(b"ab{d", b"x")  # bit 5 of the first byte is set, but PIL's is_cid refuses the type
    assert S.pil_outcome(data)[0] == "err"
    assert L.png_probe(data, 7)[0] == L.UNSUPPORTED


def test_synthetic_samples_decode_to_the_reference_semantics():
    """The writer against PIL, so that the GPU tests' files mean what their names say: gray 1 / 2 / 4 scaled,
    palette looked up (black beyond a short PLTE), gray 16 clipped to 255, the high byte of the other 16-bit
    types, Adam7 placing every pixel, garbage padding ignored."""
    for (w, h, ct, depth, lace, kw) in [(13, 7, 0, 1, 1, {}), (67, 5, 0, 2, 0, {}), (9, 9, 0, 4, 1, dict(garbage=True)),
                                        (13, 7, 3, 2, 1, dict(plte_n=3)), (13, 7, 3, 4, 0, dict(plte_n=10)),
                                        (13, 7, 0, 16, 1, {}), (5, 7, 2, 16, 0, {}), (3, 2, 4, 16, 1, {}),
                                        (13, 7, 6, 16, 1, {}), (9, 9, 6, 8, 1, {}), (1, 3, 2, 8, 1, {})]:
        data, samples, plte = E.make(w, h, ct, depth, lace, "mixP", **kw)
        np.testing.assert_array_equal(S.pil_rgb(data), E.expected_rgb(samples, ct, depth, plte), err_msg=str((w, h, ct, depth, lace)))
    g16 = E.samples_for(13, 7, 0, 16)
    assert {0, 255, 256, 65535} <= set(g16.reshape(-1).tolist())
