"""TIFF files for the tests of the opt-in "tiff" format, written from the pixels that must come out -- a writer of
its own (IFD, strips, PackBits, LZW, horizontal differencing; Deflate through zlib), so the expectation never comes
from the code under test.  tests/test_tiff_host.py pins the writer to PIL (its raw decoder and libtiff), the
reference.

  native()    (name, bytes, expected RGB): files of the subset, every one of which must decode natively
  refused()   (name, bytes): valid files outside the subset, one per refusal (SDSJ_UNSUPPORTED from the parse)
  damaged()   (name, bytes): malformed or doubtful files (SDSJ_CORRUPT, from the parse -- names ending in _hdr --
              or from the strip kernels)
  pillow_files() / pillow_manifest(): files Pillow writes of every accepted mode x compression; a handful of them
              are committed under tests/golden/tiff/ with a manifest of sizes and RGB hashes."""
import functools
import hashlib
import io
import json
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff")

BYTE, ASCII, SHORT, LONG, RATIONAL = 1, 2, 3, 4, 5
_SIZE = {BYTE: 1, ASCII: 1, SHORT: 2, LONG: 4, RATIONAL: 8, 7: 1, 16: 8}
NONE, LZW, DEFLATE, ADOBE_DEFLATE, PACKBITS = 1, 5, 32946, 8, 32773


# -- codecs ------------------------------------------------------------------------------------------------
def packbits(data: bytes, row: int) -> bytes:
    """PackBits row by row (a run never crosses a row): replicate runs of 2..128, literal runs of 1..128."""
    out = bytearray()
    for r0 in range(0, len(data), row):
        line = data[r0:r0 + row]
        i = 0
        lit = bytearray()

        def flush():
            for k in range(0, len(lit), 128):
                out.append(len(lit[k:k + 128]) - 1)
                out.extend(lit[k:k + 128])
            lit.clear()
        while i < len(line):
            j = i
            while j < len(line) and line[j] == line[i] and j - i < 128:
                j += 1
            if j - i >= 2:
                flush()
                out.append(257 - (j - i))
                out.append(line[i])
            else:
                lit.append(line[i])
            i = j
        flush()
    return bytes(out)


class _MsbBits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, bits):
        self.acc = (self.acc << bits) | code
        self.n += bits
        while self.n >= 8:
            self.out.append((self.acc >> (self.n - 8)) & 255)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def lzw(data: bytes, eoi=True, clear_first=True) -> bytes:
    """TIFF LZW: MSB first, 9..12 bits with the early change, clear 256 at the start and when entry 4093 has been
    made, end-of-information 257."""
    w = _MsbBits()
    bits, nxt, table = 9, 258, {}
    if clear_first:
        w.put(256, 9)
    cur = b""
    for b in data:
        s = cur + bytes([b])
        if len(s) == 1 or s in table:
            cur = s
            continue
        w.put(cur[0] if len(cur) == 1 else table[cur], bits)
        table[s] = nxt
        nxt += 1
        if nxt == 4094:
            w.put(256, bits)
            bits, nxt, table = 9, 258, {}
        elif nxt > (1 << bits) - 1:
            bits += 1
        cur = bytes([b])
    if cur:
        w.put(cur[0] if len(cur) == 1 else table[cur], bits)
        nxt += 1  # (the decoder makes its entry for this code before it reads the next one)
        if nxt > (1 << bits) - 1 and bits < 12:
            bits += 1
    if eoi:
        w.put(257, bits)
    return w.done()


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def difference(rows: np.ndarray) -> np.ndarray:
    """Predictor 2 on an array [rows, width, samples]: each sample minus the one a pixel to its left, modulo 256."""
    out = rows.copy()
    out[:, 1:] = rows[:, 1:] - rows[:, :-1]
    return out


# -- the writer ----------------------------------------------------------------------------------------------
def tiff(pix, photo, comp=NONE, *, bo="<", ifd_first=False, rps=None, rps_tag=True, predictor=1, strips=LONG,
         extra=None, cmap=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, tags=(), drop=(), edit=None, unsorted=False,
         encode=None, more_tags=True, pad_strips=0, reverse_file_order=False):
    """One classic TIFF of the samples `pix` [height, width, samples] (uint8) as stored.  `rps`: rows per strip
    (default: all rows); rps_tag=False leaves the tag out.  `strips`: the type of StripOffsets / StripByteCounts.
    `tags`: (tag, type, values) added or replacing; `drop`: tags left out; `unsorted`: the first entry moved to the
    end.  `encode(raw, row_bytes)` replaces the strip codec; `edit(datas, counts)` returns the strips' bytes and the
    StripByteCounts to store (the offsets follow the bytes as stored).  `pad_strips`: bytes between strips;
    `reverse_file_order`: the last strip first in the file."""
    pix = np.ascontiguousarray(pix, np.uint8)
    if pix.ndim == 2:
        pix = pix[:, :, None]
    h, w, spp = pix.shape
    rps_eff = h if rps is None else rps
    src = difference(pix) if predictor == 2 else pix
    raw, datas = [], []
    for y in range(0, h, rps_eff):
        raw.append(src[y:y + rps_eff].tobytes())
    for r in raw:
        if encode is not None:
            datas.append(encode(r, w * spp))
        elif comp == NONE:
            datas.append(r)
        elif comp == PACKBITS:
            datas.append(packbits(r, w * spp))
        elif comp == LZW:
            datas.append(lzw(r))
        else:
            datas.append(deflate(r, level, strategy))
    counts = [len(d) for d in datas]
    if edit is not None:
        datas, counts = edit(datas, counts)
    e = {256: (SHORT if w < 65536 else LONG, [w]), 257: (SHORT if h < 65536 else LONG, [h]), 258: (SHORT, [8] * spp),
         259: (SHORT, [comp]), 262: (SHORT, [photo]), 277: (SHORT, [spp]), 284: (SHORT, [1])}
    if more_tags:
        e[282] = (RATIONAL, [(72, 1)])
        e[283] = (RATIONAL, [(72, 1)])
        e[296] = (SHORT, [2])
        e[305] = (ASCII, b"tiff_synth\0")
    if rps_tag:
        e[278] = (strips, [rps_eff])
    if predictor != 1:
        e[317] = (SHORT, [predictor])
    if extra is not None:
        e[338] = (SHORT, list(extra))
    if cmap is not None:
        e[320] = (SHORT, [int(v) for v in np.asarray(cmap).reshape(-1)])
    e[273] = (strips, [0] * len(datas))
    e[279] = (strips, counts)
    for t, ty, vals in tags:
        e[t] = (ty, vals)
    for t in drop:
        e.pop(t, None)
    order = sorted(e)
    if unsorted:
        order = order[1:] + order[:1]

    def pack_vals(ty, vals):
        if ty == ASCII or isinstance(vals, (bytes, bytearray)):
            return bytes(vals)
        if ty == RATIONAL:
            return b"".join(struct.pack(bo + "II", *v) for v in vals)
        return struct.pack(bo + {BYTE: "B", SHORT: "H", LONG: "I", 16: "Q"}[ty] * len(vals), *vals)

    def layout(offsets):
        """(ifd bytes with its out-of-line values, given the IFD's own position), as a function of its position."""
        def at(pos):
            ee = dict(e)
            if 273 in ee and 273 not in [t for t, _, _ in tags]:
                ee[273] = (ee[273][0], offsets)
            body = struct.pack(bo + "H", len(order))
            tail = b""
            tail_pos = pos + 2 + 12 * len(order) + 4
            for t in order:
                ty, vals = ee[t]
                data = pack_vals(ty, vals)
                cnt = len(data) // _SIZE[ty]
                if len(data) <= 4:
                    field = data + bytes(4 - len(data))
                else:
                    if (tail_pos + len(tail)) & 1:
                        tail += b"\0"
                    field = struct.pack(bo + "I", tail_pos + len(tail))
                    tail += data
                body += struct.pack(bo + "HHI", t, ty, cnt) + field
            return body + struct.pack(bo + "I", 0) + tail
        return at

    head = (b"II" if bo == "<" else b"MM") + struct.pack(bo + "H", 42)
    file_order = list(range(len(datas)))
    if reverse_file_order:
        file_order.reverse()
    if ifd_first:
        ifd_len = len(layout([0] * len(datas))(8))
        p = 8 + ifd_len + (ifd_len & 1)
        offsets = [0] * len(datas)
        blob = b""
        for k in file_order:
            offsets[k] = p + len(blob)
            blob += datas[k] + bytes(pad_strips)
        ifd = layout(offsets)(8)
        return head + struct.pack(bo + "I", 8) + ifd + bytes(p - 8 - len(ifd)) + blob
    offsets = [0] * len(datas)
    blob = b""
    for k in file_order:
        offsets[k] = 8 + len(blob)
        blob += datas[k] + bytes(pad_strips)
    if len(blob) & 1:
        blob += b"\0"
    pos = 8 + len(blob)
    return head + struct.pack(bo + "I", pos) + blob + layout(offsets)(pos)


# -- expectations ---------------------------------------------------------------------------------------------
def rgb_of(pix, photo, cmap=None):
    """convert("RGB") of the stored samples: photometric 0 inverted, 1 replicated, 2 as it is, 3 through the colour
    map's high bytes, 5 as Convert.c cmyk2rgb; an extra sample is dropped."""
    pix = np.asarray(pix, np.uint8)
    if pix.ndim == 2:
        pix = pix[:, :, None]
    if photo in (0, 1):
        g = pix[:, :, 0]
        g = 255 - g if photo == 0 else g
        return np.stack([g, g, g], 2)
    if photo == 2:
        return pix[:, :, :3].copy()
    if photo == 3:
        cm = (np.asarray(cmap, np.uint32).reshape(3, 256) >> 8).astype(np.uint8)
        return np.stack([cm[0][pix[:, :, 0]], cm[1][pix[:, :, 0]], cm[2][pix[:, :, 0]]], 2)
    if photo == 5:
        c = pix[:, :, :3].astype(np.int32)
        k = pix[:, :, 3:4].astype(np.int32)
        return (((255 - c) * (255 - k) + 127) // 255).astype(np.uint8)
    raise ValueError(photo)


def pil_outcome(data):
    from PIL import Image
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return "ok", np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    except Exception as e:  # noqa: BLE001 -- the kind of outcome is what is compared
        return "err", type(e)


def picture(w, h, seed, samples=3, noise=0):
    """A smooth picture with some texture (so LZW and Deflate find matches), optionally noisy."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, samples), np.int32)
    for c in range(samples):
        out[:, :, c] = (x * (3 + c) + y * (5 - c) + 40 * c + 7 * seed) % 256
        out[:, :, c] = (out[:, :, c] // 8) * 8
    if noise:
        out += rng.integers(-noise, noise + 1, out.shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def noisy(w, h, seed, samples=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, samples), dtype=np.uint8)


def colour_map(seed):
    """3 x 256 SHORTs whose low bytes are not zero (so the 16-to-8-bit rule shows)."""
    return np.random.default_rng(seed).integers(0, 65536, (3, 256)).astype(np.uint16)


def runs_image():
    """PackBits run lengths at their limits, one row each (width 259, grey): a replicate run of 128 then one of 2
    then a lone literal and 128 different bytes (a literal run of 128 after one of 1 is what the encoder makes of
    129 different bytes)."""
    w = 128 + 2 + 129
    row0 = [7] * 128 + [9] * 2 + [(3 * i + 1) % 256 for i in range(129)]
    row1 = [(5 * i + 2) % 256 for i in range(128)] + [4] * 2 + [8] * 128 + [1]
    row2 = [200] * w
    a = np.array([row0, row1, row2, row1, row0], np.uint8)
    assert a.shape == (5, w)
    return a[:, :, None]


# -- fixture groups ----------------------------------------------------------------------------------------------
COMPS = (("none", NONE), ("packbits", PACKBITS), ("lzw", LZW), ("deflate", ADOBE_DEFLATE))
MODES = (("l", 1, 1, None), ("l0", 0, 1, None), ("p", 3, 1, None), ("rgb", 2, 3, None), ("rgba", 2, 4, (2,)),
         ("rgbx", 2, 4, (0,)), ("la", 1, 2, (2,)), ("cmyk", 5, 4, None))


@functools.lru_cache(maxsize=None)
def native():
    out = []

    def add(name, pix, photo, comp, cmap=None, **kw):
        out.append((name, tiff(pix, photo, comp, cmap=cmap, **kw), rgb_of(pix, photo, cmap)))

    # every mode x compression, 50 x 37 (no multiple of 64 or 4), three strips with a short last one
    for k, (mn, photo, spp, extra) in enumerate(MODES):
        pix = picture(50, 37, k, spp, noise=6)
        cmap = colour_map(k) if photo == 3 else None
        for j, (cn, comp) in enumerate(COMPS):
            add(f"{mn}_{cn}", pix, photo, comp, cmap=cmap, extra=extra, rps=16, bo="<>"[(k + j) & 1], ifd_first=bool(j & 1))
    # predictor 2 for LZW and Deflate, every sample count
    for k, (mn, photo, spp, extra) in enumerate(MODES):
        pix = picture(33, 70, 20 + k, spp, noise=3)
        cmap = colour_map(k) if photo == 3 else None
        for cn, comp in COMPS[2:]:
            add(f"{mn}_{cn}_pred", pix, photo, comp, cmap=cmap, extra=extra, rps=9, predictor=2, bo="<>"[k & 1])
    # rows per strip: 1, 3 on a height of 7, the height, above it, absent; SHORT and LONG arrays, inline and by offset
    pix7 = picture(13, 7, 3)
    for cn, comp in COMPS:
        add(f"rps1_{cn}", pix7, 2, comp, rps=1, strips=SHORT)
        add(f"rps3_{cn}", pix7, 2, comp, rps=3, strips=SHORT, bo=">")
        add(f"rps7_{cn}", pix7, 2, comp, rps=7, strips=LONG, bo=">")
        add(f"rps_above_{cn}", pix7, 2, comp, rps=7, tags=[(278, LONG, [4000])])
        add(f"rps_max_{cn}", pix7, 2, comp, rps=7, tags=[(278, LONG, [0xFFFFFFFF])], ifd_first=True)
        add(f"rps_absent_{cn}", pix7, 2, comp, rps=7, rps_tag=False, more_tags=False)
    # more strips than the strip kernels' grid has rows (16): their stride loop takes a second and a third strip
    pix40 = picture(11, 40, 6, noise=5)
    for cn, comp in COMPS:
        add(f"strips40_{cn}", pix40, 2, comp, rps=1, strips=SHORT, predictor=2 if comp in (LZW, ADOBE_DEFLATE) else 1)
    add("two_strips_short_inline", picture(9, 4, 1, 1), 1, NONE, rps=2, strips=SHORT, bo=">")  # two SHORTs fit the entry
    add("one_pixel", picture(1, 1, 1), 2, LZW)
    add("one_column", picture(1, 40, 2), 2, ADOBE_DEFLATE, rps=7, predictor=2)
    add("one_row", picture(300, 1, 3, 1), 1, PACKBITS)
    # Deflate: stored, fixed and dynamic blocks; the old compression number
    big = picture(64, 30, 5, noise=2)
    add("deflate_level0", big, 2, ADOBE_DEFLATE, level=0, rps=10)
    add("deflate_level1", big, 2, ADOBE_DEFLATE, level=1, rps=10)
    add("deflate_level9", big, 2, ADOBE_DEFLATE, level=9, rps=10, predictor=2)
    add("deflate_fixed", big, 2, ADOBE_DEFLATE, strategy=zlib.Z_FIXED, rps=10)
    add("deflate_32946", big, 2, DEFLATE, rps=10, bo=">")
    # LZW: one noisy strip of 5,760 bytes passes 9 -> 10 -> 11 -> 12 bits and the table reset; a flat one makes
    # long strings (the entry that is its own prefix)
    add("lzw_noisy_one_strip", noisy(64, 30, 9), 2, LZW)
    add("lzw_noisy_pred", noisy(64, 30, 10), 2, LZW, predictor=2, bo=">")
    add("lzw_flat", np.full((30, 64, 3), 77, np.uint8), 2, LZW, rps=8)
    add("lzw_no_eoi", picture(20, 9, 4), 2, LZW, encode=lambda r, row: lzw(r, eoi=False))
    add("lzw_bytes_after_eoi", picture(20, 9, 4), 2, LZW, encode=lambda r, row: lzw(r) + b"\x55\xaa\x55")
    # PackBits: runs of 1, 2 and 128; the no-op byte between runs
    add("packbits_runs", runs_image(), 1, PACKBITS, rps=2)
    add("packbits_noop", picture(16, 6, 2, 1), 1, PACKBITS, rps=3,
        encode=lambda r, row: b"\x80" + packbits(r, row)[:2] + b"\x80\x80" + packbits(r, row)[2:] + b"\x80")
    # PackBits runs that cross rows inside their strip (the strip coded as one long row; the flat rows make such runs)
    flat = np.repeat(np.arange(6, dtype=np.uint8)[:, None] // 3 * 9, 20, 1)[:, :, None]
    add("packbits_runs_cross_rows", flat, 1, PACKBITS, rps=6, encode=lambda r, row: packbits(r, len(r)))
    add("packbits_literals_cross_rows", picture(13, 6, 8, 1, noise=9), 1, PACKBITS, rps=3, encode=lambda r, row: packbits(r, len(r)))
    # RowsPerStrip of 0x7FFFFFFF: the largest value libtiff takes besides 0xFFFFFFFF
    add("rps_7fffffff_lzw", pix7, 2, LZW, rps=7, tags=[(278, LONG, [0x7FFFFFFF])])
    # the passive tags this path lets through, each as libtiff wants it
    add("passive_tags", picture(10, 10, 2), 2, LZW, rps=4, tags=[(254, LONG, [0]), (270, ASCII, b"a picture\0"), (271, ASCII, b"m\0"),
        (272, ASCII, b"model\0"), (306, ASCII, b"2026:10:21 12:00:00\0"), (315, ASCII, b"nobody\0"), (65535, SHORT, [1, 2])])
    # SampleFormat, one value for all samples and one each
    add("sample_format_one", picture(12, 9, 3, 4), 2, ADOBE_DEFLATE, rps=4, extra=(2,), tags=[(339, SHORT, [1])])
    add("sample_format_each", picture(12, 9, 4), 2, LZW, rps=4, tags=[(339, SHORT, [1, 1, 1])])
    add("sample_format_each_packbits", picture(12, 9, 5), 2, PACKBITS, rps=5, tags=[(339, SHORT, [1, 1, 1])], bo=">")
    # strips out of order in the file, with gaps between them
    add("strips_reversed_in_file", picture(21, 12, 6), 2, LZW, rps=4, reverse_file_order=True, pad_strips=3)
    add("strips_gaps_none", picture(21, 12, 7), 2, NONE, rps=5, reverse_file_order=True, pad_strips=2, ifd_first=True)
    # a second IFD and unknown tags are ignored
    add("private_tags", picture(10, 10, 1), 2, ADOBE_DEFLATE, tags=[(700, BYTE, b"<x/>"), (34675, 7, b"icc?" * 40), (65000, LONG, [1, 2, 3])])
    # the largest image
    add("large_rgb_lzw", picture(320, 240, 11, noise=1), 2, LZW, rps=34, predictor=2)
    add("large_cmyk_deflate", picture(320, 240, 12, 4), 5, ADOBE_DEFLATE, rps=25)
    add("large_p_packbits", picture(320, 240, 13, 1), 3, PACKBITS, rps=204, cmap=colour_map(5))
    for e in pillow_manifest():
        with open(os.path.join(GOLDEN, e["file"]), "rb") as f:
            data = f.read()
        out.append(("pillow_" + e["file"].split(".")[0], data, _pillow_pixels(e)))
    return out


@functools.lru_cache(maxsize=None)
def refused():
    p3, p1, p4 = picture(20, 11, 1), picture(20, 11, 1, 1), picture(20, 11, 1, 4)
    big = tiff(p3, 2, LZW)
    big = big[:2] + struct.pack("<H", 43) + big[4:]
    return [
        ("bigtiff", big),
        ("tiles", tiff(p3, 2, NONE, tags=[(322, SHORT, [16]), (323, SHORT, [16]), (324, LONG, [8]), (325, LONG, [768])], drop=(273, 279, 278))),
        ("planar_2", tiff(p3, 2, NONE, tags=[(284, SHORT, [2])])),
        ("bits_1", tiff(p1, 1, NONE, tags=[(258, SHORT, [1])])),
        ("bits_2", tiff(p1, 1, NONE, tags=[(258, SHORT, [2])])),
        ("bits_4", tiff(p1, 3, NONE, tags=[(258, SHORT, [4])], cmap=colour_map(1))),
        ("bits_16", tiff(np.repeat(p1, 2, 1), 1, NONE, tags=[(258, SHORT, [16]), (256, SHORT, [20])])),
        ("bits_32_float", tiff(np.repeat(p1, 4, 1), 1, NONE, tags=[(258, SHORT, [32]), (256, SHORT, [20]), (339, SHORT, [3])])),
        ("sample_format_2", tiff(p1, 1, NONE, tags=[(339, SHORT, [2])])),
        ("associated_alpha", tiff(p4, 2, LZW, extra=(1,))),
        ("two_extra_samples", tiff(picture(20, 11, 1, 5), 2, LZW, extra=(0, 2))),
        ("grey0_unassociated_alpha", tiff(picture(20, 11, 1, 2), 0, LZW, extra=(2,))),
        ("grey0_unspecified_extra", tiff(picture(20, 11, 1, 2), 0, NONE, extra=(0,))),
        ("grey1_unspecified_extra_deflate", tiff(picture(20, 11, 1, 2), 1, ADOBE_DEFLATE, extra=(0,))),
        ("grey1_unspecified_extra", tiff(picture(20, 11, 1, 2), 1, NONE, extra=(0,))),
        ("four_samples_no_extra_tag", tiff(p4, 2, LZW)),
        ("ycbcr", tiff(p3, 6, NONE)),
        ("cielab", tiff(p3, 8, NONE)),
        ("mask", tiff(p1, 4, NONE)),
        ("jpeg_compression", tiff(p3, 2, NONE, tags=[(259, SHORT, [7])])),
        ("ccitt_compression", tiff(p1, 0, NONE, tags=[(259, SHORT, [4]), (258, SHORT, [1])])),
        ("zstd_compression", tiff(p3, 2, NONE, tags=[(259, SHORT, [50000])])),
        ("predictor_3", tiff(p3, 2, LZW, tags=[(317, SHORT, [3])])),
        ("predictor_2_packbits", tiff(p3, 2, PACKBITS, tags=[(317, SHORT, [2])])),
        ("fill_order_2", tiff(p3, 2, LZW, tags=[(266, SHORT, [2])])),
        ("orientation_6", tiff(picture(7, 5, 1), 2, LZW, tags=[(274, SHORT, [6])])),
        ("orientation_3", tiff(p3, 2, NONE, tags=[(274, SHORT, [3])])),
        ("old_style_lzw", tiff(p3, 2, LZW, encode=lambda r, row: b"\x00\x01" + lzw(r)[2:])),
        ("cmyk_five_samples", tiff(picture(20, 11, 1, 5), 5, LZW, extra=(0,))),
        ("rgb_as_two_samples", tiff(picture(20, 11, 1, 2), 2, NONE)),
    ]


def _lzw_codes(codes):
    """A strip from explicit (code, bits) pairs."""
    w = _MsbBits()
    for c, b in codes:
        w.put(c, b)
    return w.done()


@functools.lru_cache(maxsize=None)
def damaged():
    p3, p1 = picture(20, 11, 2), picture(20, 11, 2, 1)
    good_lzw = tiff(p3, 2, LZW, rps=4)
    out = []

    def add(name, data):
        out.append((name, data))

    def cut(d, k):
        return lambda datas, counts: ([x[:k] if i == d else x for i, x in enumerate(datas)], [min(c, k) if i == d else c for i, c in enumerate(counts)])

    def count_only(d, delta):
        return lambda datas, counts: (datas, [c + delta if i == d else c for i, c in enumerate(counts)])

    def swap(d, new):
        return lambda datas, counts: ([new(x) if i == d else x for i, x in enumerate(datas)],
                                      [len(new(datas[i])) if i == d else c for i, c in enumerate(counts)])

    # the parse's own findings (names ending in _hdr)
    add("ifd_past_file_hdr", good_lzw[:4] + struct.pack("<I", len(good_lzw) + 10) + good_lzw[8:])
    add("ifd_cut_hdr", good_lzw[:-30])
    add("strip_offset_past_file_hdr", tiff(p3, 2, LZW, rps=4, tags=[(273, LONG, [8, 1 << 30, 40])]))
    add("strip_count_past_file_hdr", tiff(p3, 2, NONE, rps=4, edit=count_only(2, 5000)))
    add("strip_arrays_differ_hdr", tiff(p3, 2, LZW, rps=4, tags=[(279, LONG, [10, 10])]))
    add("too_few_strips_hdr", tiff(p3, 2, LZW, rps=4, tags=[(278, SHORT, [3])]))
    add("missing_byte_counts_hdr", tiff(p3, 2, LZW, rps=4, drop=(279,)))
    add("missing_offsets_hdr", tiff(p3, 2, LZW, rps=4, drop=(273,)))
    add("duplicate_tags_hdr", _duplicate_entry(tiff(p3, 2, LZW, rps=4, more_tags=False), 277))
    for v in (0x80000000, 0x80000001, 0xFFFFFFFE):
        add(f"rows_per_strip_{v:x}_lzw_hdr", tiff(p3, 2, LZW, tags=[(278, LONG, [v])]))
    add("rows_per_strip_80000000_packbits_hdr", tiff(p3, 2, PACKBITS, tags=[(278, LONG, [0x80000000])]))
    add("rows_per_strip_80000000_none_hdr", tiff(p3, 2, NONE, tags=[(278, LONG, [0x80000000])]))
    # tags libtiff knows, with a type it rejects; a tag outside the list this path lets through
    add("min_sample_value_rational_hdr", tiff(p3, 2, LZW, tags=[(280, RATIONAL, [(1, 1)])]))
    add("max_sample_value_rational_hdr", tiff(p3, 2, LZW, tags=[(281, RATIONAL, [(1, 1)])]))
    add("smin_sample_value_ascii_hdr", tiff(p3, 2, LZW, tags=[(340, ASCII, b"abc\0")]))
    add("smax_sample_value_ascii_hdr", tiff(p3, 2, ADOBE_DEFLATE, tags=[(341, ASCII, b"abc\0")]))
    add("resolution_as_long_hdr", tiff(p3, 2, LZW, tags=[(282, LONG, [72])]))
    add("page_number_hdr", tiff(p3, 2, LZW, tags=[(297, SHORT, [0, 1])]))
    for cn, comp in COMPS:  # (two values for three samples: libtiff fails the directory of a compressed file)
        add(f"sample_format_count_2_{cn}_hdr", tiff(p3, 2, comp, rps=4, tags=[(339, SHORT, [1, 1])]))
    add("unsorted_tags_hdr", tiff(p3, 2, LZW, rps=4, unsorted=True))
    add("colour_map_short_hdr", tiff(p1, 3, LZW, tags=[(320, SHORT, [0] * 96)]))
    add("colour_map_absent_hdr", tiff(p1, 3, LZW))
    add("zero_width_hdr", tiff(p3, 2, NONE, tags=[(256, SHORT, [0])]))
    add("rows_per_strip_0_hdr", tiff(p3, 2, NONE, tags=[(278, SHORT, [0])]))
    add("bits_count_differs_hdr", tiff(p3, 2, NONE, tags=[(258, SHORT, [8, 8])]))
    add("value_offset_past_file_hdr", _with_entry_offset(tiff(p3, 2, NONE), 305, 1 << 29))
    add("uncompressed_strip_short_hdr", tiff(p3, 2, NONE, rps=4, edit=count_only(1, -7)))
    # the strip kernels' findings
    add("lzw_eoi_early", tiff(p3, 2, LZW, rps=4, encode=lambda r, row: lzw(r[:-9])))
    add("lzw_cut", tiff(p3, 2, LZW, rps=4, edit=cut(1, 20)))
    add("lzw_code_above_next", tiff(p3, 2, LZW, encode=lambda r, row: _lzw_codes([(256, 9), (65, 9), (300, 9), (257, 9)])))
    add("lzw_first_code_no_clear", tiff(p3, 2, LZW, rps=4, encode=lambda r, row: lzw(r, clear_first=False)))
    add("lzw_string_after_clear", tiff(p3, 2, LZW, encode=lambda r, row: _lzw_codes([(256, 9), (258, 9), (257, 9)])))
    add("deflate_adler_wrong", tiff(p3, 2, ADOBE_DEFLATE, rps=4, edit=swap(2, lambda x: x[:-1] + bytes([x[-1] ^ 1]))))
    add("deflate_cut_before_adler", tiff(p3, 2, ADOBE_DEFLATE, rps=4, edit=cut(0, len(deflate(p3[:4].tobytes())) - 4)))
    add("deflate_cut", tiff(p3, 2, ADOBE_DEFLATE, rps=4, edit=cut(1, 12)))
    add("deflate_too_many_bytes", tiff(p3, 2, ADOBE_DEFLATE, rps=4, encode=lambda r, row: deflate(r + b"extra")))
    add("deflate_too_few_bytes", tiff(p3, 2, ADOBE_DEFLATE, rps=4, encode=lambda r, row: deflate(r[:-3])))
    add("deflate_bad_header", tiff(p3, 2, ADOBE_DEFLATE, rps=4, edit=swap(0, lambda x: b"\x78\x9d" + x[2:])))
    add("packbits_short", tiff(p3, 2, PACKBITS, rps=4, edit=cut(1, 9)))
    add("packbits_run_past_strip", tiff(p1, 1, PACKBITS, rps=4, encode=lambda r, row: packbits(r[:-2], row) + b"\xfb\x05"))
    add("packbits_literal_cut", tiff(p1, 1, PACKBITS, rps=4, encode=lambda r, row: packbits(r[:-4], row) + b"\x03\x01\x02"))
    return out


def _duplicate_entry(data, tag):
    """The little-endian file `data` (its IFD and values at the end) with entry `tag` twice in a row: the IFD is
    rewritten at the end of the file with the values' offsets kept."""
    ifd = struct.unpack("<I", data[4:8])[0]
    n = struct.unpack("<H", data[ifd:ifd + 2])[0]
    ents = [data[ifd + 2 + 12 * k:ifd + 14 + 12 * k] for k in range(n)]
    k = [struct.unpack("<H", e[:2])[0] for e in ents].index(tag)
    ents.insert(k, ents[k])
    pos = len(data) + (len(data) & 1)
    return (data[:4] + struct.pack("<I", pos) + data[8:] + bytes(len(data) & 1) + struct.pack("<H", n + 1) + b"".join(ents) +
            struct.pack("<I", 0))


def _with_entry_offset(data, tag, off):
    """The little-endian file `data` with the value field of entry `tag` replaced by `off`."""
    ifd = struct.unpack("<I", data[4:8])[0]
    n = struct.unpack("<H", data[ifd:ifd + 2])[0]
    for k in range(n):
        p = ifd + 2 + 12 * k
        if struct.unpack("<H", data[p:p + 2])[0] == tag:
            return data[:p + 2] + struct.pack("<HI", ASCII, 64) + struct.pack("<I", off) + data[p + 12:]
    raise KeyError(tag)


# -- Pillow-written files -------------------------------------------------------------------------------------
PIL_COMPS = ("raw", "packbits", "tiff_lzw", "tiff_adobe_deflate")
PIL_MODES = ("L", "P", "RGB", "RGBA", "LA", "CMYK")


def _pillow_image(mode, w, h, seed):
    from PIL import Image
    n = {"L": 1, "P": 1, "RGB": 3, "RGBA": 4, "LA": 2, "CMYK": 4}[mode]
    a = picture(w, h, seed, n, noise=4)
    if mode == "P":
        im = Image.fromarray(a[:, :, 0], "P")
        im.putpalette(np.random.default_rng(seed).integers(0, 256, 768, dtype=np.uint8).tobytes())
        return im
    return Image.fromarray(a[:, :, 0] if n == 1 else a, mode)


def pillow_files(w=50, h=37):
    """(name, bytes, expected RGB) of every accepted mode x compression as this Pillow writes them; the expectation
    is the array the file was written from, through rgb_of (P: through the palette that was put)."""
    out = []
    for k, mode in enumerate(PIL_MODES):
        im = _pillow_image(mode, w, h, 40 + k)
        if mode == "P":
            pal = np.asarray(im.getpalette(), np.uint8).reshape(-1, 3)
            ref = pal[np.asarray(im)]
        else:
            photo = {"L": 1, "RGB": 2, "RGBA": 2, "LA": 1, "CMYK": 5}[mode]
            ref = rgb_of(np.asarray(im), photo)
        for comp in PIL_COMPS:
            b = io.BytesIO()
            im.save(b, "TIFF", compression=comp)
            out.append((f"{mode.lower()}_{comp}", b.getvalue(), ref))
    return out


def pillow_manifest():
    p = os.path.join(GOLDEN, "manifest.json")
    if not os.path.exists(p):
        return []
    with open(p) as f:
        return json.load(f)


def _pillow_pixels(e):
    """The committed file's expected RGB: regenerated from the manifest's recipe, and checked against its hash."""
    ref = dict((n, r) for n, _, r in _pillow_refs(e["width"], e["height"]))[e["file"].split(".")[0]]
    assert hashlib.sha256(ref.tobytes()).hexdigest() == e["rgb_sha256"], e["file"]
    return ref


@functools.lru_cache(maxsize=None)
def _pillow_refs(w, h):
    return pillow_files(w, h)


def write_golden(names=("rgb_tiff_lzw", "rgba_tiff_adobe_deflate", "p_packbits", "cmyk_tiff_lzw", "la_raw", "l_tiff_adobe_deflate")):
    """Writes the committed handful (run once by hand: python -c "from tests import tiff_synth as S; S.write_golden()")."""
    os.makedirs(GOLDEN, exist_ok=True)
    man = []
    for n, d, r in pillow_files():
        if n in names:
            with open(os.path.join(GOLDEN, n + ".tif"), "wb") as f:
                f.write(d)
            man.append({"file": n + ".tif", "width": r.shape[1], "height": r.shape[0], "bytes": len(d),
                        "rgb_sha256": hashlib.sha256(r.tobytes()).hexdigest()})
    with open(os.path.join(GOLDEN, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1)
