"""ctypes binding of the C-ABI in include/sdsj.h (the in-tree ``sds_amd/lib/libsdsj.so``).

This is the binding a maintainer would add to sds.  ``torch`` is imported
first so that the process holds exactly one HIP runtime: the library's ``libamdhip64.so.7``
dependency then resolves to the copy torch already loaded (same SONAME as /opt/rocm's).

There is no CPU fallback: if the library is missing or cannot be loaded, every entry point
raises ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDSJ_LIBRARY: an alternative in-tree build (kernel experiments under tools/); default = the product
LIB_PATH = os.environ.get("SDSJ_LIBRARY") or os.path.join(_HERE, "lib", "libsdsj.so")

SDSJ_ABI_VERSION = 2
OK, EINVAL, UNSUPPORTED, CORRUPT, ENOMEM, EHIP, ECAPACITY = 0, -1, -2, -3, -4, -5, -6
STATUS_NAMES = {OK: "OK", EINVAL: "EINVAL", UNSUPPORTED: "UNSUPPORTED", CORRUPT: "CORRUPT", ENOMEM: "ENOMEM",
                EHIP: "EHIP", ECAPACITY: "ECAPACITY"}
FILTERS = {"box": 0, "bilinear": 1, "hamming": 2, "bicubic": 3, "lanczos": 4, "nearest": 5}
DTYPE_U8, DTYPE_F32 = 0, 1
LAYOUT_CHW, LAYOUT_HWC = 0, 1

# Every symbol include/sdsj.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "sdsj_abi_version", "sdsj_probe", "sdsj_engine_create", "sdsj_engine_destroy", "sdsj_decode_resize_batch",
    "sdsj_decode_resize_batch_device", "sdsj_engine_set_timing", "sdsj_engine_stage_times", "sdsj_last_error",
    "sdsj_stage_name", "sdsj_engine_debug_buffers", "sdsj_resize_frames_device", "sdsj_submit_batch",
    "sdsj_submit_files", "sdsj_wait_batch", "sdsj_engine_counters", "sdsj_counter_name", "sdsj_engine_set_lanes",
    "sdsj_engine_reserve", "sdsj_plan_need", "sdsj_service_serve", "sdsj_engine_set_formats", "sdsj_png_probe",
    "sdsj_plan_need_formats", "sdsj_png_probe_formats", "sdsj_probe_formats", "sdsj_engine_set_hints",
    "sdsj_engine_clear_hints", "sdsj_engine_hint_counters", "sdsj_hint_counter_name", "sdsj_gif_probe",
    "sdsj_webp_probe", "sdsj_tiff_probe",
]
NUM_COUNTERS = 11  # SDSJ_NUM_COUNTERS
NUM_HINT_COUNTERS = 4  # SDSJ_NUM_HINT_COUNTERS (the entry-point store's: sdsj_engine_hint_counters)
FORMAT_JPEG, FORMAT_PNG, FORMAT_PNG_EXT, FORMAT_PNG_META, FORMAT_JPEG_EXT = 1, 2, 4, 16, 64  # SDSJ_FORMAT_*
FORMAT_JPEG_SCANS = 128
FORMAT_GIF = 256
FORMAT_JPEG_CMYK = 512
FORMAT_JPEG_CMYK_PROG = 1024
FORMAT_WEBP = 4096  # (2048 is no format)
FORMAT_TIFF = 16384  # (nor is 8192)
# "png-ext": PNG with the wider subset (Adam7, depths 1 / 2 / 4 / 16, more ancillary chunks); the bit is
# valid only together with PNG, so the name carries both
# "png-meta": PNG files as converters and editors write them (iCCP, zTXt, iTXt, chunks after the image data);
# likewise valid only together with PNG, and combinable with "png-ext"
# "jpeg-ext": JPEG with the wider three-component subset (upsampling ratios of 3 and 4 such as 4:1:1 and 4:1:0,
# RGB-coded files); the bit is valid only together with JPEG, so the name carries both
# "jpeg-scans": multi-scan sequential JPEG (SOF0 / SOF1 frames whose components arrive in more than one scan, as
# jpegtran -scans writes them); likewise valid only together with JPEG, and combinable with "jpeg-ext"
# "jpeg-cmyk": four-component sequential JPEG (Adobe CMYK and YCCK files); likewise valid only together with JPEG, and
# combinable with every other name (components in several scans need "jpeg-scans" too, ratios of 3 and 4 "jpeg-ext")
# "jpeg-cmyk-prog": progressive (SOF2) four-component JPEG, as Pillow writes a CMYK image with progressive=True; the bit is
# valid only together with JPEG and JPEG_CMYK, so the name carries all three, and combines with every other name
# "gif": the first frame of a GIF87a / GIF89a file; a base format of its own, valid alone and with every other name
# "webp": lossless WebP (VP8L, bare or in a VP8X container); a base format of its own as well
# "tiff": classic TIFF in strips, 8 bits per sample (none / PackBits / LZW / Deflate); a base format of its own too
FORMATS = {"jpeg": FORMAT_JPEG, "png": FORMAT_PNG, "png-ext": FORMAT_PNG | FORMAT_PNG_EXT,
           "png-meta": FORMAT_PNG | FORMAT_PNG_META, "jpeg-ext": FORMAT_JPEG | FORMAT_JPEG_EXT,
           "jpeg-scans": FORMAT_JPEG | FORMAT_JPEG_SCANS, "gif": FORMAT_GIF, "webp": FORMAT_WEBP, "tiff": FORMAT_TIFF,
           "jpeg-cmyk": FORMAT_JPEG | FORMAT_JPEG_CMYK,
           "jpeg-cmyk-prog": FORMAT_JPEG | FORMAT_JPEG_CMYK | FORMAT_JPEG_CMYK_PROG}
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
GIF_SIGNATURES = (b"GIF87a", b"GIF89a")


def WEBP_SIGNATURE(data) -> bool:
    """RIFF at bytes 0..3 and WEBP at bytes 8..11."""
    return data[:4] == b"RIFF" and data[8:12] == b"WEBP"


def TIFF_SIGNATURE(data) -> bool:
    """II*\0 or MM\0* (classic TIFF; BigTIFF is not sized natively)."""
    return data[:4] in (b"II*\x00", b"MM\x00*")


def format_mask(formats) -> int:
    """SDSJ_FORMAT_* mask of a tuple of "jpeg" / "jpeg-ext" / "jpeg-scans" / "jpeg-cmyk" / "jpeg-cmyk-prog" / "png" /
    "png-ext" / "png-meta" / "gif" / "webp" / "tiff" (None: JPEG only, the engine's default).  "jpeg-ext", "jpeg-scans" and "jpeg-cmyk"
    include "jpeg", and "jpeg-cmyk-prog" includes "jpeg-cmyk" (so ("jpeg-cmyk-prog",) is 1537), as "png-ext" and
    "png-meta" include "png"; "gif", "webp" and "tiff" stand alone or beside any of them."""
    if formats is None:
        return FORMAT_JPEG
    if isinstance(formats, str):
        formats = (formats,)
    mask = 0
    for f in formats:
        if f not in FORMATS:
            raise ValueError(f"unknown format {f!r}: expected a tuple of {sorted(FORMATS)}")
        mask |= FORMATS[f]
    if not mask:
        raise ValueError("formats must name at least one of " + ", ".join(sorted(FORMATS)))
    return mask
SLOTS = 2  # SDSJ_SLOTS: batches in flight on the asynchronous host path


class NativeLibraryError(RuntimeError):
    pass


class SdsjInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32),
                ("h_samp", ctypes.c_int32 * 3), ("v_samp", ctypes.c_int32 * 3),
                ("restart_interval", ctypes.c_int32), ("supported", ctypes.c_int32),
                ("entropy_offset", ctypes.c_int64)]


class SdsjPngInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bit_depth", ctypes.c_int32),
                ("color_type", ctypes.c_int32), ("interlace", ctypes.c_int32), ("supported", ctypes.c_int32)]


class SdsjGifInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("frame_x", ctypes.c_int32),
                ("frame_y", ctypes.c_int32), ("frame_w", ctypes.c_int32), ("frame_h", ctypes.c_int32),
                ("interlace", ctypes.c_int32), ("table_entries", ctypes.c_int32), ("min_code_size", ctypes.c_int32),
                ("supported", ctypes.c_int32)]


class SdsjWebpInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("has_alpha", ctypes.c_int32),
                ("lossless", ctypes.c_int32), ("extended", ctypes.c_int32), ("supported", ctypes.c_int32)]


class SdsjTiffInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("photometric", ctypes.c_int32), ("codec", ctypes.c_int32), ("predictor", ctypes.c_int32),
                ("rows_per_strip", ctypes.c_int32), ("strips", ctypes.c_int32), ("supported", ctypes.c_int32)]


class SdsjCfg(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("max_batch", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64)]


class SdsjOp(ctypes.Structure):
    _fields_ = [("out_h", ctypes.c_int32), ("out_w", ctypes.c_int32), ("crop_before_resize", ctypes.c_int32),
                ("filter", ctypes.c_int32), ("out_dtype", ctypes.c_int32), ("layout", ctypes.c_int32)]


class SdsjServiceCfg(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("device", ctypes.c_int32), ("engines", ctypes.c_int32),
                ("max_batch", ctypes.c_int32), ("listen_fd", ctypes.c_int32), ("parent_pid", ctypes.c_int32)]


_lib = None
_lock = threading.Lock()


def load() -> ctypes.CDLL:
    """Loads libsdsj.so (raises NativeLibraryError if it is absent or broken)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} is missing: build the MI355X extension first "
                "(python -m sds_amd.build, or __graft_entry__.build()). There is no CPU fallback.")
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
        lib.sdsj_abi_version.restype = ctypes.c_int
        lib.sdsj_probe.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjInfo)]
        lib.sdsj_probe_formats.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.POINTER(SdsjInfo)]
        lib.sdsj_engine_create.argtypes = [ctypes.c_int, ctypes.POINTER(SdsjCfg), ctypes.POINTER(vp)]
        lib.sdsj_engine_destroy.argtypes = [vp]
        lib.sdsj_decode_resize_batch.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                                 ctypes.POINTER(sz), ctypes.POINTER(SdsjOp), vp, vp,
                                                 ctypes.POINTER(i32), vp]
        lib.sdsj_decode_resize_batch_device.argtypes = [vp, ctypes.c_int, vp, sz, vp, vp, ctypes.POINTER(SdsjOp), vp, vp,
                                                        vp, vp]
        lib.sdsj_resize_frames_device.argtypes = [vp, ctypes.c_int, vp, i32, i32, i64, ctypes.POINTER(SdsjOp), vp, vp,
                                                  vp, vp]
        lib.sdsj_submit_batch.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                          ctypes.POINTER(sz), ctypes.POINTER(SdsjOp), vp, vp, vp]
        lib.sdsj_submit_files.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                          ctypes.POINTER(SdsjOp), vp, vp, vp]
        lib.sdsj_wait_batch.argtypes = [vp, ctypes.c_int, ctypes.POINTER(i32)]
        lib.sdsj_engine_set_timing.argtypes = [vp, ctypes.c_int]
        lib.sdsj_engine_stage_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int)]
        lib.sdsj_last_error.argtypes = [vp]
        lib.sdsj_last_error.restype = ctypes.c_char_p
        lib.sdsj_stage_name.argtypes = [ctypes.c_int]
        lib.sdsj_stage_name.restype = ctypes.c_char_p
        lib.sdsj_engine_debug_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                  ctypes.POINTER(i64), ctypes.POINTER(i64)]
        lib.sdsj_engine_counters.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int]
        lib.sdsj_counter_name.argtypes = [ctypes.c_int]
        lib.sdsj_counter_name.restype = ctypes.c_char_p
        lib.sdsj_engine_set_lanes.argtypes = [vp, ctypes.c_int]
        lib.sdsj_engine_set_hints.argtypes = [vp, i64]
        lib.sdsj_engine_clear_hints.argtypes = [vp]
        lib.sdsj_engine_hint_counters.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int]
        lib.sdsj_hint_counter_name.argtypes = [ctypes.c_int]
        lib.sdsj_hint_counter_name.restype = ctypes.c_char_p
        lib.sdsj_engine_reserve.argtypes = [vp, i64]
        lib.sdsj_plan_need.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjOp), ctypes.POINTER(i64)]
        lib.sdsj_service_serve.argtypes = [ctypes.POINTER(SdsjServiceCfg)]
        lib.sdsj_engine_set_formats.argtypes = [vp, ctypes.c_int]
        lib.sdsj_png_probe.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjPngInfo)]
        lib.sdsj_png_probe_formats.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.POINTER(SdsjPngInfo)]
        lib.sdsj_gif_probe.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjGifInfo)]
        lib.sdsj_webp_probe.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjWebpInfo)]
        lib.sdsj_tiff_probe.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjTiffInfo)]
        lib.sdsj_plan_need_formats.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(SdsjOp), ctypes.c_int,
                                               ctypes.POINTER(i64)]
        for name in EXPORTS:
            getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        if lib.sdsj_abi_version() != SDSJ_ABI_VERSION:
            raise NativeLibraryError(f"ABI version mismatch: {lib.sdsj_abi_version()} != {SDSJ_ABI_VERSION}")
        _lib = lib
        return lib


def probe(jpg: bytes, mask=None) -> tuple[int, SdsjInfo]:
    """``mask``: the SDSJ_FORMAT_* mask the sample will be decoded under (sdsj_probe_formats: with
    FORMAT_JPEG_EXT the wider JPEG subset is supported, with FORMAT_JPEG_SCANS multi-scan sequential files, with FORMAT_JPEG_CMYK four-component ones, with FORMAT_JPEG_CMYK_PROG progressive ones too); None: the
    default subset (sdsj_probe)."""
    info = SdsjInfo()
    if mask is None:
        st = load().sdsj_probe(jpg, len(jpg), ctypes.byref(info))
    else:
        st = load().sdsj_probe_formats(jpg, len(jpg), int(mask), ctypes.byref(info))
    return st, info


def png_probe(png: bytes, formats=None) -> tuple[int, SdsjPngInfo]:
    """``formats``: the SDSJ_FORMAT_* mask the sample will be decoded under (sdsj_png_probe_formats); None: the
    base PNG subset (sdsj_png_probe)."""
    info = SdsjPngInfo()
    if formats is None:
        st = load().sdsj_png_probe(png, len(png), ctypes.byref(info))
    else:
        st = load().sdsj_png_probe_formats(png, len(png), int(formats), ctypes.byref(info))
    return st, info


def gif_probe(gif: bytes) -> tuple[int, SdsjGifInfo]:
    """sdsj_gif_probe: the screen, the first frame's rectangle and the status the sample gets under "gif" before its
    LZW data is decoded."""
    info = SdsjGifInfo()
    st = load().sdsj_gif_probe(gif, len(gif), ctypes.byref(info))
    return st, info


def webp_probe(webp: bytes) -> tuple[int, SdsjWebpInfo]:
    """sdsj_webp_probe: the size (of a lossy file too), whether the file is lossless and extended, and the status the
    sample gets under "webp" before its prefix-coded data is decoded."""
    info = SdsjWebpInfo()
    st = load().sdsj_webp_probe(webp, len(webp), ctypes.byref(info))
    return st, info


def tiff_probe(tiff: bytes) -> tuple[int, SdsjTiffInfo]:
    """sdsj_tiff_probe: the size, the layout of a supported file, and the status the sample gets under "tiff" before
    its strips are decoded."""
    info = SdsjTiffInfo()
    st = load().sdsj_tiff_probe(tiff, len(tiff), ctypes.byref(info))
    return st, info
