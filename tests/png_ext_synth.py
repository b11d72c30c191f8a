"""Synthetic PNG files of the wider subset (SDSJ_FORMAT_PNG_EXT): Adam7 interlace, bit depths 1, 2, 4 and
16, ancillary chunks before the image data.  Test infrastructure on top of tests/png_synth.py: samples
are packed most significant bit first below depth 8 and big-endian at depth 16, every non-empty Adam7
pass is filtered as an image of its own by S.scanlines under a real filter schedule, and S.write_png
writes the file.  Every case is small."""
from __future__ import annotations

import struct

import numpy as np

from tests import png_synth as S

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
PASS_SCHEDULES = ["mixP", "mixA", "mixU"]


def unit(ctype, depth) -> int:
    return max(1, CHANNELS[ctype] * depth // 8)


def passes(w, h, interlace):
    """(x start, y start, x step, y step, pass width, pass height) of the non-empty passes, in stream order."""
    if not interlace:
        return [(0, 0, 1, 1, w, h)]
    out = []
    for xs, ys, dx, dy in ADAM7:
        pw, ph = (w - xs + dx - 1) // dx if w > xs else 0, (h - ys + dy - 1) // dy if h > ys else 0
        if pw > 0 and ph > 0:
            out.append((xs, ys, dx, dy, pw, ph))
    return out


def layout_bytes(w, h, ctype, depth, interlace) -> int:
    bits = CHANNELS[ctype] * depth
    return sum(ph * (1 + (pw * bits + 7) // 8) for *_, pw, ph in passes(w, h, interlace))


def pack(samples: np.ndarray, depth: int, garbage=None) -> np.ndarray:
    """samples [h, n] (n = width x channels) -> the rows' bytes [h, ceil(n x depth / 8)] uint8.  garbage: a
    Generator that fills the padding bits of each row's last byte (zeros otherwise)."""
    h, n = samples.shape
    if depth == 8:
        return samples.astype(np.uint8)
    if depth == 16:
        return samples.astype(">u2").view(np.uint8).reshape(h, 2 * n)
    per = 8 // depth
    nb = (n + per - 1) // per
    padded = np.zeros((h, nb * per), np.uint16)
    padded[:, :n] = samples
    if garbage is not None and nb * per > n:
        padded[:, n:] = garbage.integers(0, 1 << depth, (h, nb * per - n))
    shifts = np.array([8 - depth * (k + 1) for k in range(per)], np.uint16)
    return (padded.reshape(h, nb, per) << shifts).sum(axis=2).astype(np.uint8)


def raw_stream(samples: np.ndarray, ctype, depth, interlace, sched, garbage=None) -> bytes:
    """The filtered scanlines of samples [h, w, channels]; sched: a schedule kind of S.schedule, or a list of
    kinds taken in turn by the non-empty passes."""
    h, w, ch = samples.shape
    kinds = [sched] if isinstance(sched, str) else list(sched)
    out = []
    for k, (xs, ys, dx, dy, pw, ph) in enumerate(passes(w, h, interlace)):
        sub = samples[ys::dy, xs::dx].reshape(ph, pw * ch)
        out.append(S.scanlines(pack(sub, depth, garbage), unit(ctype, depth), S.schedule(kinds[k % len(kinds)], ph)))
    return b"".join(out)


def samples_for(w, h, ctype, depth, seed=0) -> np.ndarray:
    """[h, w, channels] integer samples.  16-bit gray lies on both sides of 255 (PIL clips it there) and holds
    0, 255, 256 and 65535."""
    rng = np.random.default_rng(seed * 104729 + w * 131 + h * 7 + ctype * 17 + depth)
    ch = CHANNELS[ctype]
    if depth == 8:
        return S.pixels(w, h, ctype, seed).reshape(h, w, ch).astype(np.uint16)
    if depth == 16 and ctype == 0:
        v = rng.integers(0, 600, (h, w, 1)).astype(np.uint16)
        special = [65535, 0, 255, 256, 254, 257, 32768, 511]
        flat = v.reshape(-1)  # (a view)
        k = min(len(special), flat.size)
        flat[:k] = special[:k]
        return v
    return rng.integers(0, 1 << depth, (h, w, ch)).astype(np.uint16)


def expected_rgb(samples: np.ndarray, ctype, depth, plte: bytes | None) -> np.ndarray:
    """What convert("RGB") gives for the samples (the reference semantics of the wider subset)."""
    s = samples.astype(np.int64)
    if ctype == 3:
        pal = np.zeros((256, 3), np.uint8)
        p = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        pal[:len(p)] = p
        return pal[s[..., 0]]
    if depth == 16:
        col = np.minimum(s, 255) if ctype == 0 else s >> 8
    elif depth < 8:
        col = s * (255 // ((1 << depth) - 1))
    else:
        col = s
    col = col.astype(np.uint8)
    return np.repeat(col[..., :1], 3, axis=2) if ctype in (0, 4) else col[..., :3]


def make(w, h, ctype, depth, interlace, sched="mixP", *, seed=0, plte_n=None, pre=(), garbage=False, stream=None,
         level=6, **kw):
    """(file bytes, samples, PLTE bytes or None)."""
    samples = samples_for(w, h, ctype, depth, seed)
    plte = None
    if ctype == 3:
        n = (1 << depth) if plte_n is None else plte_n
        plte = np.random.default_rng(seed + 11).integers(0, 256, n * 3, dtype=np.uint8).tobytes()
    raw = raw_stream(samples, ctype, depth, interlace, sched, np.random.default_rng(seed + 5) if garbage else None)
    assert len(raw) == layout_bytes(w, h, ctype, depth, interlace)
    if stream is not None:
        raw = stream(raw)
    data = S.write_png(w, h, ctype, S.zstream(raw, level), depth=depth, interlace=interlace, plte=plte, pre=list(pre), **kw)
    return data, samples, plte


ADAM7_SIZES = [(1, 1), (1, 3), (3, 1), (2, 2), (4, 4), (5, 7), (8, 8), (9, 9), (13, 7), (67, 5), (64, 65), (200, 129),
               (9, 131)]


def group_adam7_8bit():
    """Adam7 at depth 8: all five colour types x sizes with empty passes (up to 4 columns or rows) and a second
    band of 64 rows in pass 6 (200 x 129) and pass 7 (9 x 131); the passes take mixP / mixA / mixU in turn."""
    out = []
    for ct in (0, 2, 3, 4, 6):
        for k, (w, h) in enumerate(ADAM7_SIZES):
            sched = PASS_SCHEDULES[k % 3:] + PASS_SCHEDULES[:k % 3]
            out.append((f"a7_t{ct}_{w}x{h}", make(w, h, ct, 8, 1, sched, seed=ct, plte_n=200 if ct == 3 else None)[0]))
    return out


LOW_WIDTHS, LOW_HEIGHTS = (1, 7, 8, 9, 13, 67), (1, 7, 65)


def group_low_depth():
    """Depths 1 / 2 / 4, gray and palette (every other palette case with a PLTE shorter than its indices),
    widths with partial and exact last bytes, non-interlaced and Adam7; the cases take S.SCHEDULES in turn, and
    one more has garbage padding bits."""
    out, k = [], 0
    for ct in (0, 3):
        for depth in (1, 2, 4):
            for w in LOW_WIDTHS:
                for h in LOW_HEIGHTS:
                    for lace in (0, 1):
                        sched = S.SCHEDULES[(k + k // 2) % len(S.SCHEDULES)]  # (every kind meets both layouts)
                        short = ct == 3 and (k // 2) % 2 == 1
                        plte_n = max(1, (1 << depth) * 5 // 8) if short else None
                        name = f"d{depth}_t{ct}_{w}x{h}_i{lace}_{sched}" + ("_short" if short else "")
                        out.append((name, make(w, h, ct, depth, lace, sched, seed=k, plte_n=plte_n)[0]))
                        k += 1
    for depth, lace in ((1, 0), (2, 1), (4, 0)):
        out.append((f"d{depth}_garbage_i{lace}", make(13, 7, 0, depth, lace, "mixP", seed=3, garbage=True)[0]))
    out.append(("d1_pal_garbage", make(13, 7, 3, 1, 1, "mixA", seed=4, garbage=True)[0]))
    return out


def group_depth16():
    """Depth 16: colour types 0, 2, 4, 6 (filter units 2, 6, 4, 8), all Paeth and mixA (Average first)."""
    out = []
    for ct in (0, 2, 4, 6):
        for (w, h) in ((1, 1), (13, 7), (64, 65)):
            for lace in (0, 1):
                for sched in ("all4", "mixA"):
                    out.append((f"d16_t{ct}_{w}x{h}_i{lace}_{sched}", make(w, h, ct, 16, lace, sched, seed=ct + 1)[0]))
    return out


ANCILLARY = [(b"tIME", struct.pack(">HBBBBB", 2024, 2, 29, 12, 30, 59)), (b"bKGD", b"\0\x10\0\x20\0\x30"),
             (b"sBIT", b"\x05\x06\x05"), (b"eXIf", b"MM\0\x2a\0\0\0\x08\0\0\0\0\0\0"), (b"prVt", b"private data")]
REFUSED = [(b"iCCP", b"icc\0\0" + S.zstream(b"\0" * 128)), (b"zTXt", b"k\0\0" + S.zstream(b"text")),
           (b"iTXt", b"k\0\0\0\0\0text"), (b"acTL", struct.pack(">II", 1, 0)), (b"ABCD", b"xyz")]


def with_chunk(tag, data, bad_crc=False, **kw):
    """A 13 x 7 RGB file with one chunk between IHDR and IDAT."""
    return make(13, 7, 2, 8, 0, "mixP", pre=[(tag, data)], bad_crc=tag if bad_crc else None, **kw)[0]


def group_chunks():
    out = [(f"chunk_{t.decode()}", with_chunk(t, d)) for t, d in ANCILLARY]
    out.append(("chunk_all", make(13, 7, 6, 16, 1, "mixA", pre=ANCILLARY)[0]))
    return out


def group_all():
    return group_adam7_8bit() + group_low_depth() + group_depth16() + group_chunks()


def group_ext_damage():
    """Damage only the wider subset has: an Adam7 stream one byte short, one row long, a filter byte 5 in pass
    3, a file cut inside pass 7's data."""
    w, h = 13, 7

    def lace(stream, **kw):
        return make(w, h, 2, 8, 1, "mixP", stream=stream, **kw)[0]

    ps = passes(w, h, 1)
    off3 = sum(ph * (1 + pw * 3) for *_, pw, ph in ps[:2])  # pass 3's first filter byte
    off7 = sum(ph * (1 + pw * 3) for *_, pw, ph in ps[:6])

    def filter5(raw):
        b = bytearray(raw)
        b[off3] = 5
        return bytes(b)

    out = [("a7_short_1", lace(lambda r: r[:-1])), ("a7_row_long", lace(lambda r: r + r[off7:off7 + 1 + ps[6][4] * 3])),
           ("a7_filter5_pass3", lace(filter5))]
    # level 0: stored blocks, so a cut of the file at a known stream position falls inside pass 7
    good = lace(None, level=0)
    i0 = good.index(b"IDAT") + 4
    out.append(("a7_cut_in_pass7", good[:i0 + 2 + 5 + off7 + 10]))
    out.append(("d16_short_1", make(w, h, 6, 16, 0, "mixA", stream=lambda r: r[:-1])[0]))
    out.append(("bad_tIME_crc", with_chunk(*ANCILLARY[0], bad_crc=True)))
    return out
