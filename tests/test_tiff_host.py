"""The host side of the opt-in "tiff" format (no GPU): the writer of tests/tiff_synth.py pinned to PIL (its raw
decoder and libtiff), what PIL settled about doubtful files (the facts the opening comment of sdsj_tiff.h lists),
sdsj_tiff_probe on the three fixture groups, the mask, and sdsj_plan_need_formats."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image, features

from tests import tiff_synth as S

needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="this Pillow has no libtiff")


def _lib():
    from sds_amd import _lib
    _lib.load()
    return _lib


# -- the writer and the reference -----------------------------------------------------------------------------
@needs_libtiff
def test_the_writer_is_pinned_to_pil():
    """PIL decodes every native() file to the pixels it was written from: so photometric 0 inverts, the ColorMap's
    high byte is the colour, an extra sample is dropped, CMYK is cmyk2rgb, LZW needs no end code, the PackBits no-op
    is skipped and strips may lie in any order."""
    nat = S.native()
    assert len(nat) >= 90 and max(r.shape[0] * r.shape[1] for _, _, r in nat) == 320 * 240
    for name, data, ref in nat:
        kind, got = S.pil_outcome(data)
        assert kind == "ok", (name, got)
        np.testing.assert_array_equal(got, ref, err_msg=name)
    for e in S.pillow_manifest():
        assert Image.open(S.GOLDEN + "/" + e["file"]).size == (e["width"], e["height"])
    assert len(S.pillow_manifest()) >= 5


@needs_libtiff
def test_this_pillow_writes_every_mode_and_compression_to_the_expected_pixels():
    files = S.pillow_files()
    assert len(files) == len(S.PIL_MODES) * len(S.PIL_COMPS)
    for name, data, ref in files:
        kind, got = S.pil_outcome(data)
        assert kind == "ok", name
        np.testing.assert_array_equal(got, ref, err_msg=name)


def test_the_sixteen_to_eight_bit_rule_and_photometric_0():
    pix = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    cm = np.stack([np.arange(256) * 257, np.arange(256) * 256 + 255, (np.arange(256) * 256 + 128) % 65536]).astype(np.uint16)
    kind, got = S.pil_outcome(S.tiff(pix, 3, S.NONE, cmap=cm))
    assert kind == "ok"
    idx = pix[:, :, 0].astype(np.int64)
    np.testing.assert_array_equal(got[:, :, 0], idx)          # 257 i >> 8 = i
    np.testing.assert_array_equal(got[:, :, 1], idx)          # (256 i + 255) >> 8 = i: truncated, not rounded
    np.testing.assert_array_equal(got[:, :, 2], idx)          # (256 i + 128) >> 8 = i
    kind, got = S.pil_outcome(S.tiff(pix, 0, S.NONE))
    assert kind == "ok"
    np.testing.assert_array_equal(got[:, :, 1], 255 - idx)


# what PIL does with the doubtful files (the kind of each outcome in this Pillow / libtiff): the statuses of
# damaged() claim "raises" for the first group only
PIL_RAISES = ("ifd_past_file_hdr", "ifd_cut_hdr", "strip_offset_past_file_hdr", "strip_arrays_differ_hdr", "too_few_strips_hdr",
              "missing_byte_counts_hdr", "missing_offsets_hdr", "colour_map_absent_hdr", "zero_width_hdr", "rows_per_strip_0_hdr",
              "bits_count_differs_hdr", "lzw_eoi_early", "lzw_cut", "lzw_code_above_next", "lzw_first_code_no_clear",
              "lzw_string_after_clear", "deflate_adler_wrong", "deflate_cut", "deflate_too_few_bytes", "deflate_bad_header",
              "packbits_short", "packbits_literal_cut",
              "rows_per_strip_80000000_lzw_hdr", "rows_per_strip_80000001_lzw_hdr", "rows_per_strip_fffffffe_lzw_hdr",
              "rows_per_strip_80000000_packbits_hdr", "min_sample_value_rational_hdr", "max_sample_value_rational_hdr",
              "smin_sample_value_ascii_hdr", "smax_sample_value_ascii_hdr",
              "sample_format_count_2_packbits_hdr", "sample_format_count_2_lzw_hdr", "sample_format_count_2_deflate_hdr")
PIL_OPENS = ("strip_count_past_file_hdr", "unsorted_tags_hdr", "colour_map_short_hdr", "value_offset_past_file_hdr",
             "uncompressed_strip_short_hdr", "deflate_cut_before_adler", "deflate_too_many_bytes", "packbits_run_past_strip",
             "duplicate_tags_hdr", "rows_per_strip_80000000_none_hdr", "resolution_as_long_hdr", "page_number_hdr",
             "sample_format_count_2_none_hdr")


@needs_libtiff
def test_what_pil_settles_about_damaged_files():
    dam = dict(S.damaged())
    assert set(PIL_RAISES) | set(PIL_OPENS) == set(dam)
    for name in PIL_RAISES:
        kind, got = S.pil_outcome(dam[name])
        assert kind == "err" and issubclass(got, (OSError, ValueError, SyntaxError)), (name, kind, got)
    for name in PIL_OPENS:  # (refused here all the same: PIL decides at run time)
        assert S.pil_outcome(dam[name])[0] == "ok", name
    for name, data in S.refused():  # (either is fine, but it must not crash)
        S.pil_outcome(data)


# refused files PIL must raise on for the refusal to be needed at all (the others it may open, differently)
PIL_REFUSES = ("grey0_unassociated_alpha", "grey0_unspecified_extra", "grey1_unspecified_extra_deflate", "grey1_unspecified_extra",
               "two_extra_samples", "rgb_as_two_samples", "mask", "bigtiff")


@needs_libtiff
def test_pil_opens_a_grey_file_with_an_extra_sample_only_as_la():
    """Photometric 1 with ExtraSamples 2 is the one 8-bit grey-plus-extra key of PIL's table of modes: the other three
    combinations raise, compressed or not, while RGB opens with an extra sample of either kind."""
    ref = dict(S.refused())
    for name in PIL_REFUSES:
        kind, got = S.pil_outcome(ref[name])
        assert kind == "err", name
    for name in PIL_REFUSES[:4]:
        from PIL import UnidentifiedImageError
        assert S.pil_outcome(ref[name])[1] is UnidentifiedImageError, name
    nat = dict((n, d) for n, d, _ in S.native())
    for name in ("la_none", "la_deflate", "rgbx_lzw", "rgba_packbits"):
        assert S.pil_outcome(nat[name])[0] == "ok", name


@needs_libtiff
def test_orientation_is_applied_at_open():
    data = dict(S.refused())["orientation_6"]
    assert Image.open(io.BytesIO(data)).size == (5, 7)  # written as 7 x 5


# -- the probe ------------------------------------------------------------------------------------------------
def test_probe_native_files():
    L = _lib()
    for name, data, ref in S.native():
        st, info = L.tiff_probe(data)
        assert st == L.OK and info.supported == 1, name
        assert (info.height, info.width) == ref.shape[:2], name
        assert 1 <= info.strips <= info.height and info.rows_per_strip * info.strips >= info.height, name
    by = dict((n, d) for n, d, _ in S.native())
    i = L.tiff_probe(by["cmyk_lzw_pred"])[1]
    assert (i.samples, i.photometric, i.codec, i.predictor, i.rows_per_strip, i.strips) == (4, 5, 3, 2, 9, 8)
    i = L.tiff_probe(by["rps_max_none"])[1]
    assert (i.samples, i.photometric, i.codec, i.predictor, i.rows_per_strip, i.strips) == (3, 2, 1, 1, 7, 1)
    i = L.tiff_probe(by["rps_absent_deflate"])[1]
    assert (i.codec, i.rows_per_strip, i.strips) == (4, 7, 1)
    i = L.tiff_probe(by["rps1_packbits"])[1]
    assert (i.codec, i.rows_per_strip, i.strips) == (2, 1, 7)
    info = L.SdsjTiffInfo()
    assert L.load().sdsj_tiff_probe(None, 0, ctypes.byref(info)) == L.EINVAL


def test_probe_refused_and_damaged_files():
    L = _lib()
    for name, data in S.refused():
        st, info = L.tiff_probe(data)
        assert st == L.UNSUPPORTED and info.supported == 0, name
    assert L.tiff_probe(dict(S.refused())["orientation_6"])[1].width == 7  # (the size is filled all the same)
    for name, data in S.damaged():
        st, info = L.tiff_probe(data)
        # the directory gives away only some of them; the strips' data is the device's to judge
        assert st == (L.CORRUPT if name.endswith("_hdr") else L.OK), name
        assert info.supported == (st == L.OK), name


def test_probe_cut_at_every_byte_and_foreign_inputs():
    L = _lib()
    for name in ("two_strips_short_inline", "one_pixel", "rps3_lzw"):
        data = dict((n, d) for n, d, _ in S.native())[name]
        assert L.tiff_probe(data)[0] == L.OK
        for cut in range(len(data)):
            st, _ = L.tiff_probe(data[:cut])
            assert st in (L.UNSUPPORTED, L.CORRUPT), (name, cut)
    for other in (b"\x89PNG\r\n\x1a\n" + bytes(40), b"GIF89a" + bytes(40), b"RIFF" + bytes(4) + b"WEBP" + bytes(40), b"II" + bytes(40)):
        assert L.tiff_probe(other)[0] == L.UNSUPPORTED


def test_offsets_and_counts_are_checked_without_overflow():
    """An entry count of 2^32 - 1 RATIONALs, a value offset of 2^32 - 1, a strip of 2^32 - 1 bytes."""
    L = _lib()
    p = S.picture(8, 4, 1)
    for data in (S.tiff(p, 2, S.NONE, tags=[(273, S.LONG, [0xFFFFFFFF])]), S.tiff(p, 2, S.LZW, tags=[(279, S.LONG, [0xFFFFFFFF])])):
        assert L.tiff_probe(data)[0] == L.CORRUPT
    good = S.tiff(p, 2, S.NONE)
    ifd = struct.unpack("<I", good[4:8])[0]
    for k in range(struct.unpack("<H", good[ifd:ifd + 2])[0]):
        e = ifd + 2 + 12 * k
        if struct.unpack("<H", good[e:e + 2])[0] == 282:  # XResolution: one RATIONAL behind an offset
            huge = good[:e + 4] + struct.pack("<II", 0xFFFFFFFF, 0xFFFFFFF0) + good[e + 12:]
            assert L.tiff_probe(huge)[0] == L.CORRUPT
            break
    else:
        raise AssertionError("no XResolution entry")
    many = good[:ifd] + struct.pack("<H", 0xFFFF) + good[ifd + 2:]
    assert L.tiff_probe(many)[0] in (L.UNSUPPORTED, L.CORRUPT)


# -- masks -------------------------------------------------------------------------------------------------------
def test_format_names_and_masks():
    L = _lib()
    assert L.FORMATS["tiff"] == 16384 == L.FORMAT_TIFF
    assert L.format_mask(("tiff",)) == 16384
    assert L.format_mask(("jpeg", "tiff")) == 16385
    assert L.format_mask(("jpeg", "png", "gif", "webp", "tiff")) == 16384 | 4096 | 256 | 2 | 1
    assert L.format_mask(("tiff", "png-ext", "jpeg-scans")) == 16384 | 2 | 4 | 1 | 128
    assert L.format_mask(("tiff", "jpeg-cmyk-prog")) == 16384 | 1 | 512 | 1024
    assert L.format_mask(None) == 1
    with pytest.raises(ValueError):
        L.format_mask(("bigtiff",))
    assert L.TIFF_SIGNATURE(S.native()[0][1]) and L.TIFF_SIGNATURE(S.native()[1][1]) and not L.TIFF_SIGNATURE(b"II+\0" + bytes(12))


VALID_OTHERS = (1, 2, 3, 256, 4096, 1 | 64, 1 | 128, 1 | 512, 1 | 512 | 1024, 2 | 4, 2 | 16, 2 | 4 | 16, 4096 | 256 | 2 | 1,
                1 | 2 | 4 | 16 | 64 | 128 | 256 | 512 | 1024 | 4096)


def test_mask_validity_through_plan_need_formats():
    L = _lib()
    lib = L.load()
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    need = ctypes.c_int64(-1)
    data = S.native()[0][1]
    for mask in (16384,) + tuple(16384 | m for m in VALID_OTHERS):
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.OK, mask
        assert need.value > 0
    for bad in (8, 32, 2048, 8192):
        for mask in (bad, 16384 | bad, 16385 | bad):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.EINVAL, mask
    for mask in (16384 | 4, 16384 | 64, 16384 | 16, 16384 | 1024, 32768, 16384 | 32768):
        assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.EINVAL, mask


def test_plan_need_is_the_documented_bound_and_only_under_the_bit():
    """The decoded strips take height x width x samples bytes where a PNG's raw bytes stand in the plan, so the need
    is that of an RGB PNG of the same size with h * (1 + 3 * w) raw bytes exchanged for them."""
    from tests import png_synth
    L = _lib()
    lib = L.load()
    need, png_need = ctypes.c_int64(-1), ctypes.c_int64(-1)
    up = lambda v: (v + 255) // 256 * 256
    for name, data, ref in S.native():
        h, w = ref.shape[:2]
        spp = L.tiff_probe(data)[1].samples
        op = L.SdsjOp(32, 32, 1, 1, 0, 0)
        png = png_synth.make(w, h, 2, seed=1)
        assert lib.sdsj_plan_need_formats(png, len(png), ctypes.byref(op), 2, ctypes.byref(png_need)) == L.OK
        for mask in (16384, 16385, 16384 | 4096 | 256 | 2):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.OK, name
            assert need.value > 0 and need.value % 256 == 0
            assert need.value - up(h * w * spp + 64) == png_need.value - up(h * (1 + 3 * w) + 64), name
        for mask in (1, 3, 256, 4096, 1 | 2 | 4 | 16 | 64 | 128 | 256 | 512 | 1024 | 4096):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.UNSUPPORTED
            assert need.value == 0, name
        assert lib.sdsj_plan_need(data, len(data), ctypes.byref(op), ctypes.byref(need)) == L.UNSUPPORTED
    op = L.SdsjOp(32, 32, 1, 1, 0, 0)
    for name, data in S.refused() + S.damaged():
        for mask in (1, 3, 4096 | 1):
            assert lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need)) == L.UNSUPPORTED, name
            assert need.value == 0, name
        st = lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), 16385, ctypes.byref(need))
        assert st == L.tiff_probe(data)[0], name
    # a JPEG under a mask that also names TIFF is sized as before
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG")
    a, b = ctypes.c_int64(), ctypes.c_int64()
    jpg = buf.getvalue()
    assert lib.sdsj_plan_need_formats(jpg, len(jpg), ctypes.byref(op), 1, ctypes.byref(a)) == L.OK
    assert lib.sdsj_plan_need_formats(jpg, len(jpg), ctypes.byref(op), 16385, ctypes.byref(b)) == L.OK
    assert a.value == b.value > 0


def test_other_probes_still_report_tiff_unsupported():
    L = _lib()
    for name, data in [(n, d) for n, d, _ in S.native()[:6]] + S.refused() + S.damaged():
        st, info = L.probe(data)
        assert st == L.UNSUPPORTED and info.supported == 0, name
        assert L.png_probe(data)[0] == L.UNSUPPORTED, name
        assert L.gif_probe(data)[0] == L.UNSUPPORTED, name
        assert L.webp_probe(data)[0] == L.UNSUPPORTED, name


# -- the writer's own codecs ----------------------------------------------------------------------------------------
def test_the_fixtures_cover_what_they_claim():
    by = dict((n, d) for n, d, _ in S.native())
    # stored, fixed and dynamic Deflate blocks (BTYPE of the first block: bits 1..2 of the byte after the zlib header)
    strip = lambda name: S.deflate(S.picture(64, 30, 5, noise=2)[:10].tobytes(), *{"0": (0,), "1": (1,), "f": (6, zlib.Z_FIXED)}[name])
    assert (strip("0")[2] >> 1) & 3 == 0 and (strip("f")[2] >> 1) & 3 == 1 and (strip("1")[2] >> 1) & 3 == 2
    # the noisy strip passes every code width and the table reset
    raw = S.noisy(64, 30, 9).tobytes()
    assert len(raw) == 5760 and len(S.lzw(raw)) * 8 > 9 * (4094 - 258 + 2)
    # PackBits run lengths at their limits
    pb = S.packbits(S.runs_image()[0].tobytes(), 259)
    assert pb[0] == 257 - 128 and pb[2] == 257 - 2 and pb[4] == 127 and pb[4 + 129] == 0
    assert len(by["rps_max_none"]) > 0 and len(S.refused()) >= 20 and len(S.damaged()) >= 25
