"""Synthetic PNG files for the PNG tests (test infrastructure, no product code).

A PNG writer with a chosen colour type, per-row filter schedule (real filtering, so PIL decodes
meaningful images), caller-supplied zlib stream, IDAT split sizes (0-length chunks included), extra
chunks and a selectable CRC to damage; a fixed-Huffman deflate emitter that takes explicit literals
and (length, distance) pairs (zlib never emits distance 32768); zlib-made streams for the rest.
"""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PIL_MODE = {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}


def chunk(tag: bytes, data: bytes, bad_crc: bool = False) -> bytes:
    crc = zlib.crc32(tag + data) & 0xFFFFFFFF
    if bad_crc:
        crc ^= 0x00010000
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", crc)


def ihdr(w, h, ctype, depth=8, interlace=0) -> bytes:
    return struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)


def scanlines(pix: np.ndarray, bpp: int, schedule) -> bytes:
    """Filtered scanlines of pix [h, w * bpp] uint8; schedule[y] = filter type of row y (a type above 4
    writes the row unfiltered under that byte)."""
    h, n = pix.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    z = np.zeros(bpp, np.int32)
    for y in range(h):
        cur = pix[y].astype(np.int32)
        ft = int(schedule[y])
        a = np.concatenate([z, cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        c = np.concatenate([z, prev[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        if ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) >> 1
        elif ft == 4:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        else:
            pred = np.zeros(n, np.int32)
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def schedule(kind, h):
    """'all0'..'all4', or 'mixP' / 'mixA' / 'mixU': row i -> i mod 5 with the first row Paeth / Average / Up."""
    if kind.startswith("all"):
        return [int(kind[3])] * h
    s = [i % 5 for i in range(h)]
    s[0] = {"P": 4, "A": 3, "U": 2}[kind[3]]
    return s


def split_idat(z: bytes, sizes) -> list[bytes]:
    """z cut into pieces of the given sizes, cycled (a 0 gives an empty chunk); the rest in one piece."""
    if not sizes:
        return [z]
    out, p, k = [], 0, 0
    while p < len(z):
        s = sizes[k % len(sizes)]
        k += 1
        out.append(z[p:p + s])
        p += s
    return out or [b""]


def write_png(w, h, ctype, z: bytes, *, depth=8, interlace=0, plte: bytes | None = None, pre=(), post=(), idat_sizes=None,
              bad_crc: str | None = None, iend=True) -> bytes:
    """pre / post: (tag, data) chunks before the first / after the last IDAT; bad_crc: the chunk type whose
    CRC is damaged (the first IDAT for b'IDAT')."""
    bad = bad_crc.encode() if isinstance(bad_crc, str) else bad_crc
    out = [SIG, chunk(b"IHDR", ihdr(w, h, ctype, depth, interlace), bad == b"IHDR")]
    if plte is not None:
        out.append(chunk(b"PLTE", plte, bad == b"PLTE"))
    for tag, data in pre:
        out.append(chunk(tag, data, bad == tag))
    for k, piece in enumerate(split_idat(z, idat_sizes)):
        out.append(chunk(b"IDAT", piece, bad == b"IDAT" and k == 0))
    for tag, data in post:
        out.append(chunk(tag, data, bad == tag))
    if iend:
        out.append(chunk(b"IEND", b"", bad == b"IEND"))
    return b"".join(out)


# ---------------------------------------------------------------------------------------------
# deflate streams
# ---------------------------------------------------------------------------------------------
def zstream(raw: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, piece=None, flush=None) -> bytes:
    """zlib stream of raw; piece / flush: a flush of that mode after every `piece` input bytes."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if piece is None:
        return co.compress(raw) + co.flush()
    out = bytearray()
    for p in range(0, len(raw), piece):
        out += co.compress(raw[p:p + piece])
        out += co.flush(flush)
    return bytes(out + co.flush())


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, k):  # k bits of v, least significant first
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, k):  # a Huffman code: most significant bit first
        self.put(int(format(v, f"0{k}b")[::-1], 2), k)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _fixed_sym(bw, s):
    if s < 144:
        bw.code(0x30 + s, 8)
    elif s < 256:
        bw.code(0x190 + s - 144, 9)
    elif s < 280:
        bw.code(s - 256, 7)
    else:
        bw.code(0xC0 + s - 280, 8)


def fixed_deflate(ops) -> bytes:
    """One final fixed-Huffman block of ops: ints are literals, (length, distance) pairs are matches.  Nothing
    is validated: a distance before the start of the output is emitted as asked."""
    bw = _Bits()
    bw.put(1, 1)
    bw.put(1, 2)
    for op in ops:
        if isinstance(op, tuple):
            ln, dist = op
            k = 28 if ln == 258 else max(i for i in range(28) if _LBASE[i] <= ln)
            _fixed_sym(bw, 257 + k)
            bw.put(ln - _LBASE[k], _LEXT[k])
            j = max(i for i in range(30) if _DBASE[i] <= dist)
            bw.code(j, 5)
            bw.put(dist - _DBASE[j], _DEXT[j])
        else:
            _fixed_sym(bw, int(op))
    _fixed_sym(bw, 256)
    return bw.done()


def run_ops(ops) -> bytes:
    out = bytearray()
    for op in ops:
        if isinstance(op, tuple):
            ln, dist = op
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out.append(op)
    return bytes(out)


def match_ops(raw: bytes, dist: int, first_len: int = 258):
    """raw as literals and matches at `dist` wherever at least 3 bytes repeat with that period (the first
    match at most first_len long, the others up to 258)."""
    ops, p, cap = [], 0, first_len
    while p < len(raw):
        ln = 0
        if p >= dist:
            while ln < cap and p + ln < len(raw) and raw[p + ln] == raw[p + ln - dist]:
                ln += 1
        if ln >= 3:
            ops.append((ln, dist))
            p += ln
            cap = 258
        else:
            ops.append(raw[p])
            p += 1
    assert run_ops(ops) == raw
    return ops


def zwrap(deflate: bytes, raw: bytes, adler_xor=0) -> bytes:
    return b"\x78\x01" + deflate + struct.pack(">I", (zlib.adler32(raw) & 0xFFFFFFFF) ^ adler_xor)


# ---------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------
def pixels(w, h, ctype, seed=0, ncolors=256) -> np.ndarray:
    """[h, w * bpp] uint8: smooth gradients plus noise (so every filter type predicts something)."""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h)
    bpp = BPP[ctype]
    if ctype == 3:
        return rng.integers(0, ncolors, (h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = [(xx * 3 + yy * 5 + k * 40 + rng.integers(0, 24, (h, w))) & 255 for k in range(bpp)]
    return np.stack(ch, axis=-1).astype(np.uint8).reshape(h, w * bpp)


def make(w, h, ctype, sched="mixP", *, seed=0, level=6, plte_n=256, trns=False, text=False, **kw) -> bytes:
    pix = pixels(w, h, ctype, seed)
    raw = scanlines(pix, BPP[ctype], schedule(sched, h) if isinstance(sched, str) else sched)
    plte = None
    if ctype == 3:
        rng = np.random.default_rng(seed + 11)
        plte = rng.integers(0, 256, plte_n * 3, dtype=np.uint8).tobytes()
    pre = []
    if trns:
        pre.append((b"tRNS", {0: b"\0\x10", 2: b"\0\x10\0\x20\0\x30", 3: bytes(range(0, 200, 10))}.get(ctype, b"\x00")))
    if text:
        pre.append((b"tEXt", b"Comment\0synthetic"))
    kw.setdefault("pre", pre)
    return write_png(w, h, ctype, kw.pop("z", None) or zstream(raw, level), plte=plte, **kw)


def rgb_raw(w, h, seed=0, sched="all0"):
    return scanlines(pixels(w, h, 2, seed), 3, schedule(sched, h))


def pil_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_outcome(data: bytes):
    """("ok", pixels) or ("err", exception type) of the reference decode."""
    try:
        return "ok", pil_rgb(data)
    except Exception as e:  # noqa: BLE001
        return "err", type(e)


SIZES = [(1, 1), (13, 7), (67, 5), (64, 65), (200, 129)]
SCHEDULES = ["all0", "all1", "all2", "all3", "all4", "mixP", "mixA", "mixU"]


def group_types():
    """Group 1: colour types x sizes x filter schedules, palette cases (short PLTE, tRNS)."""
    out = []
    for ct in (0, 2, 3, 4, 6):
        for (w, h) in SIZES:
            for s in SCHEDULES:
                out.append((f"t{ct}_{w}x{h}_{s}", make(w, h, ct, s, seed=ct)))
    out.append(("pal_short_plte", make(67, 5, 3, "mixP", plte_n=40)))
    out.append(("pal_trns", make(13, 7, 3, "mixA", trns=True)))
    out.append(("gray_trns_text", make(13, 7, 0, "mixU", trns=True, text=True)))
    out.append(("rgb_trns", make(13, 7, 2, "mixP", trns=True)))
    return out


def fib_raw():
    """59 x 100 RGB scanlines whose byte frequencies are Fibonacci weighted (zlib's length-limited code
    reaches 15 bits)."""
    f, syms = [1, 1], []
    while len(f) < 21:
        f.append(f[-1] + f[-2])
    for k, n in enumerate(f[1:21]):
        syms += [k + 1] * n
    rng = np.random.default_rng(3)
    arr = np.array(syms, np.uint8)
    rng.shuffle(arr)
    pix = arr[:59 * 3 * 100].reshape(100, 177)
    return scanlines(pix, 3, [0] * 100)


def group_deflate():
    """Group 2: deflate structure on RGB 8-bit."""
    out = []

    def rgb(name, w, h, z, **kw):
        out.append((name, write_png(w, h, 2, z, **kw)))

    raw = rgb_raw(150, 160)  # 72,160 bytes: level 0 writes a 65,535-byte stored block
    rgb("stored", 150, 160, zstream(raw, 0))
    raw = rgb_raw(64, 65)
    rgb("stored_sync", 64, 65, zstream(raw, 0, piece=5000, flush=zlib.Z_SYNC_FLUSH))
    rgb("fixed", 64, 65, zstream(rgb_raw(64, 65, sched="mixP"), 6, zlib.Z_FIXED))
    rgb("level9", 200, 129, zstream(rgb_raw(200, 129, sched="mixA"), 9))
    rgb("full_flush", 64, 65, zstream(rgb_raw(64, 65, sched="mixP"), 6, piece=1000, flush=zlib.Z_FULL_FLUSH))
    rgb("sync_flush", 64, 65, zstream(rgb_raw(64, 65, sched="mixU"), 6, piece=1000, flush=zlib.Z_SYNC_FLUSH))
    # hand-emitted: dist = 1, len = 258 runs (flat rows)
    pix = np.repeat(np.arange(40, dtype=np.uint8)[:, None], 173 * 3, axis=1)
    raw = scanlines(pix, 3, [0] * 40)
    ops = match_ops(raw, 1)
    assert (258, 1) in ops
    rgb("runs_d1", 173, 40, zwrap(fixed_deflate(ops), raw))
    for d in (2, 3, 4):  # overlapped copies: period-d rows
        pix = np.tile(np.arange(7, 7 + d, dtype=np.uint8), (9, 120 * 3 // d + 1))[:, :120 * 3] + np.arange(9, dtype=np.uint8)[:, None]
        raw = scanlines(pix, 3, [0] * 9)
        ops = match_ops(raw, d)
        assert any(isinstance(o, tuple) and o[0] > d for o in ops)
        rgb(f"overlap_d{d}", 120, 9, zwrap(fixed_deflate(ops), raw))
    # distance 32768 and a 3-byte match at it: 256 x 43 inflates to 33,067 bytes
    b = bytearray(rgb_raw(256, 43, seed=5))
    b[32768:] = b[0:len(b) - 32768]
    raw = bytes(b)
    ops = match_ops(raw, 32768, first_len=3)
    assert (3, 32768) in ops
    rgb("dist32768", 256, 43, zwrap(fixed_deflate(ops), raw))
    # a match that spans a row boundary and a filter byte: every row repeats the first
    pix = np.tile(pixels(50, 1, 2, 9), (12, 1))
    raw = scanlines(pix, 3, [0] * 12)
    ops = match_ops(raw, 151)
    assert any(isinstance(o, tuple) and o[0] > 151 for o in ops)
    rgb("match_rows", 50, 12, zwrap(fixed_deflate(ops), raw))
    rgb("fib15", 59, 100, zstream(fib_raw(), 9, zlib.Z_HUFFMAN_ONLY))
    rgb("no_dist", 67, 5, zstream(rgb_raw(67, 5, sched="mixP"), 6, zlib.Z_HUFFMAN_ONLY))
    z = zstream(rgb_raw(13, 7, sched="mixP"), 6)
    rgb("idat_1", 13, 7, z, idat_sizes=[1])
    rgb("idat_7", 13, 7, z, idat_sizes=[7])
    rgb("idat_0", 13, 7, z, idat_sizes=[0, 5, 0, 0, 11])
    rgb("no_iend", 13, 7, z, iend=False)
    return out


def group_sizes():
    """Group 3: an incompressible and a flat 640 x 480."""
    rng = np.random.default_rng(1)
    noise = rng.integers(0, 256, (480, 640 * 3), dtype=np.uint8)
    flat = np.full((480, 640 * 3), 77, np.uint8)
    return [("noise640", write_png(640, 480, 2, zstream(scanlines(noise, 3, [0] * 480), 6))),
            ("flat640", write_png(640, 480, 2, zstream(scanlines(flat, 3, schedule("mixP", 480)), 6)))]


def group_damage():
    """Group 5: inputs outside the subset and damaged streams (each small)."""
    out = []
    w, h = 13, 7
    raw = rgb_raw(w, h, sched="mixP")
    z = zstream(raw, 6)
    good = write_png(w, h, 2, z)
    from PIL import Image

    def pil_png(mode, size=(13, 7), **kw):
        rng = np.random.default_rng(2)
        arr = rng.integers(0, 256, (size[1], size[0], len(Image.new(mode, (1, 1)).getbands())), dtype=np.uint8)
        im = Image.fromarray(arr.squeeze() if arr.shape[2] == 1 else arr, "L" if mode in ("1", "L") else mode)
        if mode == "1":
            im = im.convert("1")
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        return b.getvalue()

    out.append(("interlaced", write_png(8, 8, 2, zstream(b"\0" * 400, 6), interlace=1)))
    out.append(("depth16", write_png(w, h, 2, zstream(b"".join(b"\0" + bytes(w * 6) for _ in range(h)), 6), depth=16)))
    for dpt in (1, 2, 4):
        rb = (w * dpt + 7) // 8
        out.append((f"depth{dpt}", write_png(w, h, 0, zstream(b"".join(b"\0" + bytes([0x5A] * rb) for _ in range(h)), 6), depth=dpt)))
    out.append(("apng", write_png(w, h, 2, z, pre=[(b"acTL", struct.pack(">II", 1, 0))])))
    out.append(("bad_adler", write_png(w, h, 2, z[:-4] + struct.pack(">I", (zlib.adler32(raw) ^ 1) & 0xFFFFFFFF))))
    pal = make(w, h, 3, "mixP")
    out.append(("cut_ihdr", good[:20]))
    out.append(("cut_plte", pal[:pal.index(b"PLTE") + 40]))
    i0 = good.index(b"IDAT")
    out.append(("cut_idat", good[:i0 + 4 + len(z) // 2]))
    out.append(("cut_before_iend", good[:good.index(b"IEND") - 4]))
    out.append(("filter5", write_png(w, h, 2, zstream(scanlines(pixels(w, h, 2), 3, [0, 1, 5, 0, 0, 0, 0]), 6))))
    out.append(("dist_before_start", write_png(w, h, 2, zwrap(fixed_deflate([0, 1, 2, (10, 7)] + [0] * 300), raw))))
    out.append(("oversubscribed", write_png(w, h, 2, b"\x78\x01" + _dynamic_bad())))
    out.append(("block_type3", write_png(w, h, 2, b"\x78\x01\x07" + bytes(20))))
    out.append(("stored_len_mismatch", write_png(w, h, 2, b"\x78\x01\x01\x10\x00\x00\x00" + bytes(40))))
    out.append(("short_rows", write_png(w, h, 2, zstream(raw[:-40], 6))))
    out.append(("extra_rows", write_png(w, h, 2, zstream(raw + raw[:40], 6))))
    out.append(("after_zlib_end", write_png(w, h, 2, z + b"trailing bytes")))
    out.append(("bad_idat_crc", write_png(w, h, 2, z, bad_crc="IDAT")))
    out.append(("bad_ihdr_crc", write_png(w, h, 2, z, bad_crc="IHDR")))
    out.append(("bad_text_crc", write_png(w, h, 2, z, pre=[(b"tEXt", b"k\0v")], bad_crc="tEXt")))
    out.append(("bad_plte_crc", make(w, h, 3, "mixP", bad_crc="PLTE")))
    out.append(("chunk_after_idat", write_png(w, h, 2, z, post=[(b"tEXt", b"k\0v")])))
    out.append(("unknown_critical", write_png(w, h, 2, z, pre=[(b"ABCD", b"xyz")])))
    return out


def _dynamic_bad() -> bytes:
    """A dynamic block header whose code-length code is over-subscribed (19 codes of 1 bit)."""
    bw = _Bits()
    bw.put(1, 1)
    bw.put(2, 2)
    bw.put(0, 5)
    bw.put(0, 5)
    bw.put(15, 4)
    for _ in range(19):
        bw.put(1, 3)
    bw.put(0, 32)
    return bw.done() + bytes(16)
