"""Synthetic GIF files for the GIF tests (test infrastructure, no product code).

An LZW writer that tracks the decoder's code width itself, with a chosen minimum code size, clears every N
codes, two clears in a row, no leading clear, a deferred clear (a full table is kept and 12-bit codes go on),
no end code, extra codes after the last pixel, a stop after some pixels and explicit code lists; a container
writer with a chosen version, global and local table, frame rectangle, interlace, leading extensions, sub-block
size, trailer and second frame.  native() / refused() / damaged() are the fixture groups of the tests.
"""
from __future__ import annotations

import io
import struct

import numpy as np


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):  # k bits of v, least significant first
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


class _Width:
    """The decoder's view of the stream: the width of the next code, as GifDecode.c and sdsj_gif.h keep it."""

    def __init__(self, min_code, bits):
        self.mc, self.bits = min_code, bits
        self.clear = 1 << min_code
        self.reset()

    def reset(self):
        self.next, self.size, self.last = self.clear + 2, self.mc + 1, -1

    def emit(self, code):
        self.bits.put(code, self.size)
        if code == self.clear:
            self.reset()
        elif code == self.clear + 1:
            pass
        elif self.last < 0:
            self.last = code
        else:
            if self.next < 4096:
                if self.next == (1 << self.size) - 1 and self.size < 12:
                    self.size += 1
                self.next += 1
            self.last = code


def pack_codes(codes, min_code) -> bytes:
    """An explicit code list as LZW data bytes (widths as the decoder will read them)."""
    b = _Bits()
    w = _Width(min_code, b)
    for c in codes:
        w.emit(c)
    return b.done()


def lzw(indices, min_code, *, clear_every=None, double_clear=False, leading_clear=True, deferred_clear=False,
        end_code=True, extra_codes=0, stop_after=None) -> bytes:
    """LZW data bytes of `indices` (values below 1 << min_code).  stop_after: only that many pixels are coded."""
    data = [int(v) for v in np.asarray(indices).reshape(-1)]
    if stop_after is not None:
        data = data[:stop_after]
    clear, end = 1 << min_code, (1 << min_code) + 1
    b = _Bits()
    w = _Width(min_code, b)
    table, nxt, ncodes = {}, clear + 2, 0

    def do_clear():
        nonlocal table, nxt
        w.emit(clear)
        if double_clear:
            w.emit(clear)
        table, nxt = {}, clear + 2

    if leading_clear:
        w.emit(clear)
    cur = None  # the current string: a tuple key into `table`, or a 1-tuple literal
    for v in data:
        if cur is None:
            cur = (v,)
            continue
        key = cur + (v,)
        if key in table:
            cur = key
            continue
        w.emit(table[cur] if len(cur) > 1 else cur[0])
        ncodes += 1
        if nxt < 4096:
            table[key] = nxt
            nxt += 1
        cur = (v,)
        if clear_every and ncodes % clear_every == 0:
            do_clear()
        elif nxt == 4096 and not deferred_clear:
            do_clear()
    if cur is not None:
        w.emit(table[cur] if len(cur) > 1 else cur[0])
    for _ in range(extra_codes):
        w.emit(0)
    if end_code:
        w.emit(end)
    return b.done()


def sub_blocks(data: bytes, size=255, terminator=True) -> bytes:
    out = bytearray()
    for p in range(0, len(data), size):
        piece = data[p:p + size]
        out.append(len(piece))
        out += piece
    if terminator:
        out.append(0)
    return bytes(out)


def gce(transparent=None, delay=0) -> bytes:
    flags = 1 if transparent is not None else 0
    return b"\x21\xf9\x04" + bytes([flags]) + struct.pack("<H", delay) + bytes([transparent or 0]) + b"\x00"


def comment(text=b"made by gif_synth") -> bytes:
    return b"\x21\xfe" + sub_blocks(text, 7)


def netscape(loops=0) -> bytes:
    return b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loops) + b"\x00"


def plain_text() -> bytes:
    return b"\x21\x01\x0c" + struct.pack("<HHHHBBBB", 0, 0, 8, 8, 8, 8, 1, 0) + sub_blocks(b"hello")


def interlace_rows(h):
    return [r for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for r in range(start, h, step)]


def colour_table(n, seed=0) -> bytes:
    rng = np.random.default_rng(1000 + seed)
    t = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    t[0] = (7, 130, 250)  # (never the identity ramp)
    return t.tobytes()


def grey_table(n) -> bytes:
    return bytes(v for i in range(n) for v in (i, i, i))


def _table_flags(t):
    n = len(t) // 3
    assert len(t) % 3 == 0 and n in (2, 4, 8, 16, 32, 64, 128, 256)
    return 0x80 | (n.bit_length() - 2)


def write_gif(screen, idx, *, version=b"89a", gct=None, lct=None, frame_xy=(0, 0), interlace=False, exts=(),
              trailer=True, second_frame=False, min_code=8, block=255, data=None, background=0, **lzw_kw) -> bytes:
    """idx: [fh, fw] indices of the first frame; data: LZW bytes to use instead of coding idx."""
    idx = np.asarray(idx, np.uint8)
    fh, fw = idx.shape
    out = bytearray(b"GIF" + version)
    out += struct.pack("<HHBBB", screen[0], screen[1], _table_flags(gct) | 0x70 if gct else 0x70, background, 0)
    if gct:
        out += gct
    for e in exts:
        out += e
    desc = struct.pack("<HHHHB", frame_xy[0], frame_xy[1], fw, fh,
                       (0x40 if interlace else 0) | (_table_flags(lct) if lct else 0))
    rows = idx[interlace_rows(fh)] if interlace else idx
    body = data if data is not None else lzw(rows, min_code, **lzw_kw)
    out += b"," + desc + (lct or b"") + bytes([min_code]) + sub_blocks(body, block)
    if second_frame:
        out += gce(delay=5) + b"," + struct.pack("<HHHHB", 0, 0, 1, 1, 0) + bytes([min_code])
        out += sub_blocks(lzw([1], min_code))
    if trailer:
        out += b";"
    return bytes(out)


def indices(w, h, ncolors, seed=0, smooth=True) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, ncolors, (h, w), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    v = (x * 3 + y * 5 + rng.integers(0, 3, (h, w))) // 4
    return (v % ncolors).astype(np.uint8)


def pil_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_outcome(data: bytes):
    """("ok", pixels) or ("err", exception type) of the reference decode."""
    try:
        return "ok", pil_rgb(data)
    except Exception as e:  # noqa: BLE001
        return "err", type(e)


def _pil_gif(w, h, seed=0, frames=1, **kw) -> bytes:
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    ims = []
    for f in range(frames):
        a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y + 40 * f) % 256)], -1)
        a = np.clip(a + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
        ims.append(Image.fromarray(a, "RGB"))
    buf = io.BytesIO()
    if frames > 1:
        ims[0].save(buf, "GIF", save_all=True, append_images=ims[1:], duration=40, **kw)
    else:
        ims[0].save(buf, "GIF", **kw)
    return buf.getvalue()


_cache: dict = {}


def native():
    """Files the GPU path must decode itself; PIL decodes each without raising (asserted here)."""
    if "native" in _cache:
        return _cache["native"]
    out = []
    t256, t16, t4 = colour_table(256), colour_table(16, 1), colour_table(4, 2)

    def add(name, data):
        kind, ref = pil_outcome(data)
        assert kind == "ok", (name, ref)
        out.append((name, data))

    for w, h in ((1, 1), (5, 9), (50, 37), (33, 70)):
        for lace in (False, True):
            add(f"size_{w}x{h}_{'lace' if lace else 'plain'}",
                write_gif((w, h), indices(w, h, 256, w + h), gct=t256, interlace=lace))
    for h in (1, 2, 3, 4, 5):
        add(f"lace_h{h}", write_gif((11, h), indices(11, h, 256, h), gct=t256, interlace=True))
    for mc, t in ((2, t4), (4, t16), (8, t256)):
        add(f"code{mc}", write_gif((50, 37), indices(50, 37, len(t) // 3, mc), gct=t, min_code=mc))
    add("one_index_320x240", write_gif((320, 240), np.full((240, 320), 3, np.uint8), gct=t256))
    rnd = indices(128, 96, 256, 5, smooth=False)
    add("random_clear_on_full", write_gif((128, 96), rnd, gct=t256))
    add("random_deferred_clear", write_gif((128, 96), rnd, gct=t256, deferred_clear=True))
    base = indices(50, 37, 256, 9)
    add("clear_every_5", write_gif((50, 37), base, gct=t256, clear_every=5))
    add("double_clear", write_gif((50, 37), base, gct=t256, clear_every=40, double_clear=True))
    add("no_leading_clear", write_gif((50, 37), base, gct=t256, leading_clear=False))
    add("blocks_of_1", write_gif((50, 37), base, gct=t256, block=1))
    add("blocks_of_7", write_gif((50, 37), base, gct=t256, block=7))
    add("no_end_code", write_gif((50, 37), base, gct=t256, end_code=False))
    add("extra_codes", write_gif((50, 37), base, gct=t256, extra_codes=9))
    add("no_trailer", write_gif((50, 37), base, gct=t256, trailer=False))
    add("local_table_only", write_gif((50, 37), base, lct=t256))
    add("both_tables", write_gif((50, 37), base, gct=colour_table(256, 7), lct=t256))
    add("no_table", write_gif((50, 37), base))
    add("grey_table_256", write_gif((50, 37), base, gct=grey_table(256)))
    add("grey_table_4_beyond", write_gif((50, 37), base, gct=grey_table(4)))
    add("local_grey_over_global_colour", write_gif((50, 37), base, gct=t256, lct=grey_table(256)))
    add("colour_table_4_beyond", write_gif((50, 37), indices(50, 37, 16, 3), gct=t4))
    sub = indices(5, 4, 16, 4) + 1
    add("frame_sub", write_gif((20, 10), sub, gct=t256, frame_xy=(3, 2)))
    add("frame_sub_transparent7", write_gif((20, 10), sub, gct=t256, frame_xy=(3, 2), exts=[gce(7)]))
    add("frame_sub_edges", write_gif((20, 10), sub, gct=t256, frame_xy=(15, 6)))
    add("frame_sub_lace", write_gif((20, 10), sub, gct=t256, frame_xy=(3, 2), interlace=True))
    add("ext_gce", write_gif((50, 37), base, gct=t256, exts=[gce()]))
    add("ext_gce_transparent", write_gif((50, 37), base, gct=t256, exts=[gce(2)]))
    add("ext_comment", write_gif((50, 37), base, gct=t256, exts=[comment()]))
    add("ext_netscape", write_gif((50, 37), base, gct=t256, exts=[netscape()]))
    add("ext_plain_text", write_gif((50, 37), base, gct=t256, exts=[plain_text()]))
    add("ext_all", write_gif((50, 37), base, gct=t256, exts=[netscape(), comment(), plain_text(), gce(5)]))
    add("gif87a", write_gif((50, 37), base, gct=t256, version=b"87a"))
    add("second_frame", write_gif((50, 37), base, gct=t256, second_frame=True))
    add("pillow_64x48", _pil_gif(64, 48, 1))
    add("pillow_320x240", _pil_gif(320, 240, 2))
    add("pillow_optimize", _pil_gif(64, 48, 3, optimize=True))
    add("pillow_two_frames", _pil_gif(50, 37, 4, frames=2))
    _cache["native"] = out
    return out


def refused():
    """Valid files outside the subset: SDSJ_UNSUPPORTED from the header."""
    t = colour_table(256)
    base = indices(10, 6, 4, 1)
    out = [("frame_beyond_screen", write_gif((8, 8), base, gct=t, frame_xy=(4, 4), min_code=2))]
    for mc in (0, 1, 9, 12):
        out.append((f"code_size_{mc}", write_gif((10, 6), base, gct=t, min_code=mc, data=lzw(base, 2))))
    out.append(("trailer_only", b"GIF89a" + struct.pack("<HHBBB", 10, 6, 0x70, 0, 0) + b";"))
    return out


def damaged():
    """Files PIL refuses or this path is not sure about; the names of those the header alone gives away
    (SDSJ_CORRUPT from the probe) end in "_hdr"."""
    t = colour_table(256)
    base = indices(50, 37, 256, 9)
    good = write_gif((50, 37), base, gct=t)
    small = indices(10, 6, 4, 1)

    def codes(cs):
        return write_gif((10, 6), small, gct=t, min_code=2, data=pack_codes(cs, 2))

    pil = bytearray(_pil_gif(64, 48, 1))
    pil[len(pil) // 2] ^= 0x5A
    cut = good[:len(good) - 300]
    body = sub_blocks(lzw(base, 8))
    past = good[:len(good) - len(body) - 1] + body[:600]  # (the third sub-block of 255 bytes is cut short)
    return [
        ("cut_inside_data", cut),
        ("end_code_halfway", write_gif((50, 37), base, gct=t, stop_after=900)),
        ("chain_ends_halfway", write_gif((50, 37), base, gct=t, stop_after=900, end_code=False)),
        ("code_above_next", codes([4, 0, 1, 9, 0, 0, 5])),
        ("first_code_not_literal", codes([4, 6, 0, 0, 5])),
        ("sub_block_past_input", past),
        ("pillow_flipped_byte", bytes(pil)),
        ("zero_width_screen_hdr", write_gif((0, 37), base, gct=t)),
        ("zero_height_frame_hdr", write_gif((50, 37), np.zeros((0, 50), np.uint8), gct=t, data=lzw([0], 8))),
    ]
