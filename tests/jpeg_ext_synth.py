"""JPEG files of the opt-in "jpeg-ext" subset (test input generator): samplings with upsampling ratios of 3 and 4,
RGB-coded files, and the cases that stay refused.

Pillow's encoder writes neither 4:1:1 nor a subsampled first component, so the wide-ratio files are written here from
chosen quantised coefficients, as tests/golden/coefjpeg.py writes its files (whose Huffman tables, code assignment
and coefficient layout this module reuses): a baseline writer with an optional restart interval, component ids and
leading marker segments, and a progressive writer (spectral selection only: one interleaved DC scan, then one AC
1..63 scan per component over that component's own block raster, a plain EOB per block).  RGB-coded files come from
Pillow (keep_rgb=True), from an Adobe transform-0 marker spliced into a coefjpeg.write_jpeg file, and from component
ids 'R', 'G', 'B'.  The reference of every file is PIL itself (pil_rgb)."""
from __future__ import annotations

import functools
import io

import numpy as np

from tests.golden import coefjpeg as C

# (h, v) per component
SETS = {
    "411": ((4, 1), (1, 1), (1, 1)),
    "410": ((4, 2), (1, 1), (1, 1)),
    "1x4": ((1, 4), (1, 1), (1, 1)),
    "3x1": ((3, 1), (1, 1), (1, 1)),
    "2x3": ((2, 3), (1, 1), (1, 1)),
    "2x4": ((2, 4), (1, 1), (1, 1)),        # 10 blocks per MCU
    "mixed": ((4, 1), (2, 1), (1, 1)),      # Cb h2v1 fancy, Cr fourfold replication
    "lumasub": ((1, 1), (4, 1), (4, 1)),    # the first component is the subsampled one
    "cr42": ((1, 1), (1, 1), (4, 2)),       # 10 blocks per MCU
}
SIZES = [(1, 1), (5, 9), (50, 37), (33, 70)]  # (width, height); 5 x 9: downsampled widths <= 2
BIG = (320, 240)                              # several entropy subsequences
ADOBE0 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"  # APP14, transform 0
JFIF = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def pil_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_outcome(data: bytes):
    """("ok", pixels) or ("err", exception type) of the reference decode."""
    try:
        return "ok", pil_rgb(data)
    except Exception as e:  # noqa: BLE001
        return "err", type(e)


class _Bits:
    """MSB-first bit packer with FF00 stuffing (a byte at a time, unlike coefjpeg's per-bit writer)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value: int, nbits: int):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # pad with ones


def _geometry(w, h, samp):
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    return hmax, vmax, -(-w // (8 * hmax)), -(-h // (8 * vmax))


def random_blocks(w: int, h: int, samp, seed: int):
    """Per component [mcuy * v, mcux * h, 64] quantised coefficients in zigzag order: a DC random walk, a few
    low-frequency AC terms per block, every seventh block or so dense; and two quantisation tables."""
    rng = np.random.default_rng(seed)
    _, _, mcux, mcuy = _geometry(w, h, samp)
    blocks = []
    for hs, vs in samp:
        bh, bw = mcuy * vs, mcux * hs
        b = np.zeros((bh, bw, 64), np.int64)
        kind = rng.integers(0, 7, (bh, bw))
        for y in range(bh):
            for x in range(bw):
                if kind[y, x] == 0:
                    b[y, x, 1:] = rng.integers(-6, 7, 63)
                else:
                    k = rng.choice(np.arange(1, 30), int(rng.integers(0, 7)), replace=False)
                    b[y, x, k] = rng.integers(-40, 41, len(k))
        dc = np.clip(np.cumsum(rng.integers(-50, 51, bh * bw)), -700, 700)
        b[:, :, 0] = dc.reshape(bh, bw)
        blocks.append(b)
    q = {0: rng.integers(1, 12, 64), 1: rng.integers(1, 16, 64)}
    return blocks, q


def _tables():
    tabs = C._annex_k_tables()
    dc = [C._codes(*tabs[(0, t)]) for t in range(2)]
    ac = [C._codes(*tabs[(1, t)]) for t in range(2)]
    return tabs, dc, ac


def _marker(seg: bytearray, m: int, payload: bytes):
    seg.extend(bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + payload)


def _head(w, h, samp, qtables, sof, ids, lead, restart):
    """SOI, the leading segments, DQT, the frame header, the four Annex K tables, DRI."""
    tabs, _, _ = _tables()
    seg = bytearray(b"\xff\xd8") + lead
    for tq, q in qtables.items():
        _marker(seg, 0xDB, bytes([tq]) + bytes(int(v) for v in q))
    f = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(samp)])
    for ci, (hs, vs) in enumerate(samp):
        f += bytes([ids[ci], (hs << 4) | vs, 0 if ci == 0 else 1])
    _marker(seg, sof, f)
    for (tc, th), (bits, vals) in sorted(tabs.items()):
        if th < 2:
            _marker(seg, 0xC4, bytes([(tc << 4) | th] + bits + vals))
    if restart:
        _marker(seg, 0xDD, restart.to_bytes(2, "big"))
    return seg


def _put_dc(bw, codes, diff):
    s = C._category(diff)
    code, ln = codes[s]
    bw.put(code, ln)
    if s:
        bw.put(diff if diff > 0 else diff - 1 + (1 << s), s)


def _put_ac(bw, codes, blk):
    """AC 1..63 of one block: run/size symbols, ZRL, and a plain EOB unless coefficient 63 is coded."""
    run = 0
    last = max([k for k in range(1, 64) if blk[k] != 0], default=0)
    for k in range(1, last + 1):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*codes[0xF0])
            run -= 16
        s = C._category(v)
        bw.put(*codes[(run << 4) | s])
        bw.put(v if v > 0 else v - 1 + (1 << s), s)
        run = 0
    if last < 63:
        bw.put(*codes[0x00])


def write_baseline(w, h, samp, blocks, qtables, restart=0, ids=(1, 2, 3), lead=b"") -> bytes:
    """Baseline (SOF0) file of three components, one interleaved scan; restart: the restart interval in MCUs (0: none);
    ids: the component ids; lead: marker segments right after SOI (JFIF, Adobe)."""
    _, dc, ac = _tables()
    _, _, mcux, mcuy = _geometry(w, h, samp)
    seg = _head(w, h, samp, qtables, 0xC0, ids, lead, restart)
    sos = bytes([len(samp)])
    for ci in range(len(samp)):
        sos += bytes([ids[ci], 0x00 if ci == 0 else 0x11])
    _marker(seg, 0xDA, sos + bytes([0, 63, 0]))
    bw = _Bits()
    pred = [0] * len(samp)
    nmcu = mcux * mcuy
    for m in range(nmcu):
        if restart and m and m % restart == 0:
            bw.flush()
            bw.out.extend(bytes([0xFF, 0xD0 + (m // restart - 1) % 8]))
            pred = [0] * len(samp)
        my, mx = divmod(m, mcux)
        for ci, (hs, vs) in enumerate(samp):
            t = 0 if ci == 0 else 1
            for dy in range(vs):
                for dx in range(hs):
                    blk = blocks[ci][my * vs + dy, mx * hs + dx]
                    _put_dc(bw, dc[t], int(blk[0]) - pred[ci])
                    pred[ci] = int(blk[0])
                    _put_ac(bw, ac[t], blk)
    bw.flush()
    return bytes(seg + bw.out + b"\xff\xd9")


def write_progressive(w, h, samp, blocks, qtables, ids=(1, 2, 3), lead=b"", dc_only=False) -> bytes:
    """Progressive (SOF2) file, spectral selection only: one interleaved DC scan, then one AC 1..63 scan per component
    over that component's own ceil(dw / 8) x ceil(dh / 8) block raster (the AC terms of the MCU padding blocks are
    not coded).  dc_only: the file ends after the DC scan (EOI appended): the decoder smooths the blocks."""
    _, dc, ac = _tables()
    hmax, vmax, mcux, mcuy = _geometry(w, h, samp)
    seg = _head(w, h, samp, qtables, 0xC2, ids, lead, 0)
    sos = bytes([len(samp)])
    for ci in range(len(samp)):
        sos += bytes([ids[ci], 0x00 if ci == 0 else 0x10])
    _marker(seg, 0xDA, sos + bytes([0, 0, 0]))
    bw = _Bits()
    pred = [0] * len(samp)
    for my in range(mcuy):
        for mx in range(mcux):
            for ci, (hs, vs) in enumerate(samp):
                for dy in range(vs):
                    for dx in range(hs):
                        v = int(blocks[ci][my * vs + dy, mx * hs + dx, 0])
                        _put_dc(bw, dc[0 if ci == 0 else 1], v - pred[ci])
                        pred[ci] = v
    bw.flush()
    seg += bw.out
    for ci, (hs, vs) in enumerate(samp):
        if dc_only:
            break
        dw, dh = -(-w * hs // hmax), -(-h * vs // vmax)
        _marker(seg, 0xDA, bytes([1, ids[ci], 0x00 if ci == 0 else 0x01, 1, 63, 0]))
        bw = _Bits()
        for y in range(-(-dh // 8)):
            for x in range(-(-dw // 8)):
                _put_ac(bw, ac[0 if ci == 0 else 1], blocks[ci][y, x])
        bw.flush()
        seg += bw.out
    return bytes(seg + b"\xff\xd9")


def make(name: str, w: int, h: int, seed: int = 0, restart: int = 0, progressive: bool = False, **kw) -> bytes:
    samp = SETS[name]
    blocks, q = random_blocks(w, h, samp, seed)
    if progressive:
        return write_progressive(w, h, samp, blocks, q, **kw)
    return write_baseline(w, h, samp, blocks, q, restart=restart, **kw)


def splice(jpg: bytes, segments: bytes) -> bytes:
    """Marker segments inserted right after SOI."""
    assert jpg[:2] == b"\xff\xd8"
    return jpg[:2] + segments + jpg[2:]


def _coef_file(w, h, samp, seed):
    """A coefjpeg.write_jpeg file (no JFIF, no Adobe marker, component ids 1, 2, 3)."""
    blocks, q = random_blocks(w, h, samp, seed)
    return C.write_jpeg(w, h, [(hs, vs, 0 if ci == 0 else 1) for ci, (hs, vs) in enumerate(samp)], blocks, q)


def _pillow(w, h, seed, mode="RGB", **kw):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * (3 + c) + yy * (5 - c) + rng.integers(0, 24, (h, w))) % 256 for c in range(3)], -1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).convert(mode).save(buf, format="JPEG", **kw)
    return buf.getvalue()


S444 = ((1, 1), (1, 1), (1, 1))


@functools.lru_cache(maxsize=None)
def wide_baseline() -> tuple:
    """(name, bytes): every sampling set at every size, one 320 x 240 file, restart intervals of 1 and 3 MCUs on two sets."""
    out = []
    for si, name in enumerate(SETS):
        for (w, h) in SIZES:
            out.append((f"{name}-{w}x{h}", make(name, w, h, seed=10 * si + w)))
    out.append((f"411-{BIG[0]}x{BIG[1]}", make("411", *BIG, seed=99)))
    for name in ("410", "mixed"):
        for ri in (1, 3):
            out.append((f"{name}-50x37-dri{ri}", make(name, 50, 37, seed=7 + ri, restart=ri)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wide_progressive() -> tuple:
    out = []
    for name, (w, h) in (("411", (50, 37)), ("2x4", (33, 70)), ("mixed", (50, 37)), ("lumasub", (5, 9))):
        out.append((f"{name}-{w}x{h}-prog", make(name, w, h, seed=3, progressive=True)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rgb_coded() -> tuple:
    out = [("rgb-pillow", _pillow(50, 37, 1, keep_rgb=True, quality=90)),
           ("rgb-pillow-prog", _pillow(33, 70, 2, keep_rgb=True, quality=85, progressive=True)),
           # several entropy subsequences, all three components on one pair of Huffman tables (as Pillow writes them)
           (f"rgb-pillow-{BIG[0]}x{BIG[1]}", _pillow(*BIG, 9, keep_rgb=True, quality=92)),
           ("rgb-adobe0-444", splice(_coef_file(50, 37, S444, 4), ADOBE0)),
           ("rgb-adobe0-411", splice(_coef_file(50, 37, SETS["411"], 5), ADOBE0))]
    blocks, q = random_blocks(33, 70, S444, 6)
    out.append(("rgb-ids", write_baseline(33, 70, S444, blocks, q, ids=(82, 71, 66))))
    blocks, q = random_blocks(50, 37, SETS["411"], 7)
    out.append(("rgb-ids-411-dri", write_baseline(50, 37, SETS["411"], blocks, q, restart=2, ids=(82, 71, 66))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ext_fixtures() -> tuple:
    """Every file only the "jpeg-ext" mask decodes: UNSUPPORTED under the default mask, OK under it."""
    return wide_baseline() + wide_progressive() + rgb_coded()


@functools.lru_cache(maxsize=None)
def jfif_and_adobe0() -> bytes:
    """JFIF and an Adobe transform-0 marker: JFIF wins, YCbCr under either mask."""
    return splice(_coef_file(50, 37, S444, 8), JFIF + ADOBE0)


@functools.lru_cache(maxsize=None)
def refused() -> tuple:
    """Refused under either mask (Pillow raises OSError on the first two as well)."""
    return (("fractional", _coef_file(50, 37, ((3, 1), (2, 1), (1, 1)), 1)),
            ("luma4x4", _coef_file(50, 37, ((4, 4), (1, 1), (1, 1)), 2)),
            ("cmyk", _pillow(50, 37, 3, mode="CMYK", quality=90)))


@functools.lru_cache(maxsize=None)
def damaged() -> tuple:
    """Three damaged ext files: a truncated scan, a flipped byte in the entropy data, a progressive file cut after its
    DC scan (EOI appended: block smoothing)."""
    whole = make("411", 50, 37, seed=21)
    cut = whole[:len(whole) - (len(whole) - whole.rindex(b"\xff\xda")) // 2]
    b = bytearray(make("mixed", 50, 37, seed=22))
    p = bytes(b).rindex(b"\xff\xda") + 14 + 40
    b[p] ^= 0x5A
    if b[p] == 0xFF:
        b[p] = 0x7F
    return (("truncated-scan", cut), ("flipped-byte", bytes(b)),
            ("prog-dc-only", make("411", 50, 37, seed=23, progressive=True, dc_only=True)))


def header_mutations(files, seed: int = 5, overwrites: int = 24) -> list:
    """Each file truncated at every header byte (up to just past its first SOS) and with header bytes overwritten."""
    rng = np.random.default_rng(seed)
    out = []
    for jpg in files:
        end = jpg.index(b"\xff\xda") + 16
        out += [jpg[:k] for k in range(min(end, len(jpg)) + 1)]
        for _ in range(overwrites):
            b = bytearray(jpg)
            b[int(rng.integers(0, min(end, len(jpg))))] = int(rng.integers(0, 256))
            out.append(bytes(b))
    return out
