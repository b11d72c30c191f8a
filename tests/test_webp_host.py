"""The host side of the opt-in "webp" format (no GPU): the mask, sdsj_webp_probe on the three fixture groups and
the committed Pillow files, sdsj_plan_need_formats (validity of masks, the documented scratch bound, nothing
without the bit), and the writer of tests/webp_synth.py pinned to libwebp through PIL."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image, features

from tests import webp_synth as S


def _lib():
    from sds_amd import _lib
    _lib.load()
    return _lib


def test_format_names_and_masks():
    L = _lib()
    assert L.FORMATS["webp"] == 4096 == L.FORMAT_WEBP
    assert L.format_mask(("webp",)) == 4096
    assert L.format_mask(("jpeg", "webp")) == 4097
    assert L.format_mask(("jpeg", "png", "gif", "webp")) == 4096 | 256 | 2 | 1
    assert L.format_mask(("webp", "png-ext", "jpeg-scans")) == 4096 | 2 | 4 | 1 | 128
    assert L.format_mask(("webp", "jpeg-cmyk-prog")) == 4096 | 1 | 512 | 1024
    assert L.format_mask(None) == 1
    with pytest.raises(ValueError):
        L.format_mask(("webp-lossy",))
    assert L.WEBP_SIGNATURE(S.native()[0][1]) and not L.WEBP_SIGNATURE(b"RIFF\0\0\0\0WAVEfmt ")


def test_mask_validity_through_plan_need_formats():
    L = _lib()
    lib = L.load()
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    need = ctypes.c_int64(-1)
    data = S.native()[0][1]
    for mask in (4096, 4097, 4096 | 256, 4096 | 2 | 4 | 16):
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.OK, mask
        assert need.value > 0
    for mask in (4096 | 4, 4096 | 64, 4096 | 8, 4096 | 32, 4096 | 2048, 2048, 8192, 4096 | 8192):
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.EINVAL, mask


def test_probe_native_files():
    L = _lib()
    for name, data, ref in S.native():
        st, info = L.webp_probe(data)
        assert st == L.OK and info.supported == 1 and info.lossless == 1, name
        assert (info.height, info.width) == ref.shape[:2], name
        assert info.extended == (data[12:16] == b"VP8X"), name
    alpha = dict((n, d) for n, d, _ in S.native())
    assert L.webp_probe(alpha["alpha_values"])[1].has_alpha == 1
    assert L.webp_probe(alpha["plain_lz"])[1].has_alpha == 0
    assert L.webp_probe(alpha["pillow_rgba_exact"])[1].has_alpha == 1
    info = L.SdsjWebpInfo()
    assert L.load().sdsj_webp_probe(None, 0, ctypes.byref(info)) == L.EINVAL


def test_probe_refused_and_damaged_files():
    L = _lib()
    sizes = {"lossy": (16, 8, 0), "lossy_alpha": (16, 8, 0), "animated_flag": (37, 29, 0), "canvas_differs": (37, 29, 1),
             "version_1": (37, 29, 1)}
    for name, data in S.refused():
        st, info = L.webp_probe(data)
        # (more groups than the path keeps tables for is the device's verdict)
        assert st == (L.OK if name.endswith("_dev") else L.UNSUPPORTED), name
        assert info.supported == (st == L.OK), name
        if name in sizes:
            assert (info.width, info.height, info.lossless) == sizes[name], name
    for name, data in S.damaged():
        st, info = L.webp_probe(data)
        # the container gives away only some of them; the prefix-coded data is the device's to judge
        assert st == (L.CORRUPT if name.endswith("_hdr") else L.OK), name
        assert info.supported == (st == L.OK), name


def test_probe_cut_at_every_byte_of_a_vp8x_file():
    L = _lib()
    data = dict((n, d) for n, d, _ in S.native())["vp8x_xmp_unknown_odd"]
    assert L.webp_probe(data)[0] == L.OK
    for cut in range(len(data)):
        st, _ = L.webp_probe(data[:cut])
        assert st in (L.UNSUPPORTED, L.CORRUPT), cut
    for other in (b"\x89PNG\r\n\x1a\n" + bytes(40), b"GIF89a" + bytes(40), b"RIFF" + bytes(4) + b"WAVE" + bytes(40)):
        assert L.webp_probe(other)[0] == L.UNSUPPORTED


def test_plan_need_is_the_documented_bound_and_only_under_the_bit():
    """The bytes of a sample are known from width and height alone: 256 (state) + 4 per pixel + three sub-images of
    ceil(w / 4) x ceil(h / 4) words + 2,048 (colour table) + (256 + 1) groups of prefix-code tables of 8,992 bytes,
    each part rounded up to 256.  They take the place a PNG's raw bytes take in the plan, so the need is that of an
    RGB PNG of the same size with h * (1 + 3 * w) raw bytes exchanged for the bound."""
    from tests import png_synth
    L = _lib()
    lib = L.load()
    need, png_need = ctypes.c_int64(-1), ctypes.c_int64(-1)
    up = lambda v: (v + 255) // 256 * 256
    for name, data, ref in S.native():
        h, w = ref.shape[:2]
        bound = 256 + up(4 * w * h) + 3 * up(4 * ((w + 3) // 4) * ((h + 3) // 4)) + 2048 + up((S.MAX_GROUPS + 1) * 8992)
        op = L.SdsjOp(32, 32, 1, 1, 0, 0)
        png = png_synth.make(w, h, 2, seed=1)
        assert lib.sdsj_plan_need_formats(png, len(png), ctypes.byref(op), 2, ctypes.byref(png_need)) == L.OK
        for mask in (4096, 4097, 4096 | 256 | 2):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.OK, name
            assert need.value > 0 and need.value % 256 == 0
            assert need.value - up(bound + 64) == png_need.value - up(h * (1 + 3 * w) + 64), name
        for mask in (1, 3, 256, 1 | 2 | 4 | 16 | 64 | 128 | 256 | 512 | 1024):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.UNSUPPORTED
            assert need.value == 0, name
        assert lib.sdsj_plan_need(data, len(data), ctypes.byref(op), ctypes.byref(need)) == L.UNSUPPORTED
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    for name, data in S.refused() + S.damaged():
        for mask in (1, 3, 256 | 1):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.UNSUPPORTED, name
            assert need.value == 0, name
        st = lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), 4097, ctypes.byref(need))
        assert st == L.webp_probe(data)[0], name
    # a JPEG under a mask that also names WebP is sized as before
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG")
    a, b = ctypes.c_int64(), ctypes.c_int64()
    jpg = buf.getvalue()
    assert lib.sdsj_plan_need_formats(jpg, len(jpg), ctypes.byref(op), 1, ctypes.byref(a)) == L.OK
    assert lib.sdsj_plan_need_formats(jpg, len(jpg), ctypes.byref(op), 4097, ctypes.byref(b)) == L.OK
    assert a.value == b.value > 0


def test_other_probes_still_report_webp_unsupported():
    L = _lib()
    for name, data in [(n, d) for n, d, _ in S.native()[:6]] + S.refused() + S.damaged():
        st, info = L.probe(data)
        assert st == L.UNSUPPORTED and info.supported == 0, name
        assert L.png_probe(data)[0] == L.UNSUPPORTED, name
        assert L.gif_probe(data)[0] == L.UNSUPPORTED, name


# what libwebp must refuse for the statuses of damaged() to mirror it
PIL_RAISES = ("riff_size_past_input_hdr", "chunk_size_past_riff_hdr", "cut_in_first_transform", "cut_in_transforms",
              "cut_in_codes", "cut_in_pixels", "cut_last_bytes", "cut_in_colour_table", "over_subscribed_code",
              "incomplete_code", "copy_before_first_pixel", "copy_past_last_pixel", "repeated_transform", "cache_bits_12",
              "two_image_chunks_hdr", "bad_signature_byte_hdr")


@pytest.mark.skipif(not features.check("webp"), reason="this Pillow has no WebP")
def test_the_writer_is_pinned_to_libwebp():
    """PIL decodes every native() file (the committed Pillow files among them) to the expected array -- so predictor
    modes 14 and 15, an index beyond the colour table, the 120 short distance codes and the border rules are what
    libwebp does --, and raises on the damaged files whose status claims that it does."""
    nat = S.native()
    assert 60 <= len(nat) and max(r.shape[0] * r.shape[1] for _, _, r in nat) == 320 * 240
    for name, data, ref in nat:
        kind, got = S.pil_outcome(data)
        assert kind == "ok", (name, got)
        np.testing.assert_array_equal(got, ref, err_msg=name)
    for e in S.pillow_manifest():  # the committed files are what Pillow writes from the manifest's arrays
        assert Image.open(S.GOLDEN + "/" + e["file"]).size == (e["width"], e["height"])
    dam = dict(S.damaged())
    assert set(PIL_RAISES) <= set(dam)
    for name in PIL_RAISES:
        kind, got = S.pil_outcome(dam[name])
        assert kind == "err" and got is OSError, (name, kind)
    for name, data in S.refused():  # (PIL decides: either is fine, but it must not crash)
        S.pil_outcome(data)
