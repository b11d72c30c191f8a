"""Synthetic lossless WebP files for the WebP tests (test infrastructure, no product code).

A VP8L writer (RFC 9649) that takes the ARGB array that must come out, so the expected pixels are its input: the
four transforms in any order (every size_bits, every predictor mode forced or mixed per tile, colour tables of any
size with their pixel packing), simple and normal prefix codes (max_symbol, the repeat codes, codes of one symbol),
a colour cache, meta-prefix images, LZ77 copies through every kind of distance code or from an explicit token
list, and a RIFF container writer (bare, VP8X with ICCP / EXIF / XMP / unknown chunks, odd chunk sizes, trailing
bytes).  native() / refused() / damaged() are the fixture groups of the tests; pillow_files() are the files Pillow
wrote, committed under tests/golden/webp/ with their manifest.
"""
from __future__ import annotations

import heapq
import io
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webp")
MAX_GROUPS = 256  # kWebpMaxGroups

# (dx, dy) of the distance codes 1..120 (RFC 9649, 5.2.2); dist = dx + dy * xsize, at least 1
_PLANE = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0),
          (1, 3), (-1, 3), (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1),
          (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5),
          (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0),
          (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6),
          (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4),
          (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7),
          (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7),
          (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]


def plane_distance(code, xsize):
    """The pixel distance of distance code `code` (>= 1) in an image xsize wide."""
    if code > 120:
        return code - 120
    dx, dy = _PLANE[code - 1]
    return max(dx + dy * xsize, 1)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):  # k bits of v, least significant first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


# ------------------------------------------------------------------------------------------------
# prefix codes
# ------------------------------------------------------------------------------------------------
def huff_lengths(freq, limit):
    """Code lengths (a complete code, every length <= limit) for the symbols with freq > 0; {} for none."""
    syms = [s for s, f in enumerate(freq) if f > 0]
    if len(syms) <= 1:
        return {s: 1 for s in syms}
    f = {s: freq[s] for s in syms}
    while True:
        heap = [(f[s], s, None, None) for s in syms]
        heapq.heapify(heap)
        k = len(freq)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            heapq.heappush(heap, (a[0] + b[0], k, a, b))
            k += 1
        out = {}
        stack = [(heap[0], 0)]
        while stack:
            (w, s, l, r), d = stack.pop()
            if l is None:
                out[s] = d
            else:
                stack += [(l, d + 1), (r, d + 1)]
        if max(out.values()) <= limit:
            return out
        f = {s: (v + 1) // 2 for s, v in f.items()}


def canonical(lengths):
    """symbol -> (code, length), codes assigned by (length, symbol); a code of one symbol takes no bits."""
    used = sorted((l, s) for s, l in lengths.items() if l)
    if len(used) == 1:
        return {used[0][1]: (0, 0)}
    out, code, prev = {}, 0, 0
    for l, s in used:
        code <<= l - prev
        out[s] = (code, l)
        code += 1
        prev = l
    return out


def put_symbol(bits, enc, s):
    code, l = enc[s]
    for i in range(l - 1, -1, -1):  # the code's first bit is its most significant
        bits.put((code >> i) & 1, 1)


_CL_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def _cl_tokens(cl, repeat):
    """(token, extra value, extra bits) of a length sequence; 16 repeats the last non-zero length (8 at first)."""
    toks, i, prev = [], 0, 8
    n = len(cl)
    while i < n:
        v = cl[i]
        run = 1
        while i + run < n and cl[i + run] == v:
            run += 1
        if repeat and v == 0 and run >= 3:
            r = min(run, 138)
            toks.append((17, r - 3, 3) if r <= 10 else (18, r - 11, 7))
            i += r
        elif repeat and v and v == prev and run >= 3:
            r = min(run, 6)
            toks.append((16, r - 3, 2))
            i += r
        else:
            toks.append((v, 0, 0))
            if v:
                prev = v
            i += 1
    return toks


def write_code(bits, lengths, n, *, form="auto", repeat=True, max_symbol=False):
    """Writes the prefix code {symbol: length} of an alphabet of n symbols; returns symbol -> (code, length)."""
    used = sorted(s for s, l in lengths.items() if l)
    simple_ok = len(used) <= 2 and all(s < 256 and lengths[s] == 1 for s in used)
    if form in ("simple", "simple8") or (form == "auto" and simple_ok):
        assert simple_ok, lengths
        bits.put(1, 1)
        bits.put(len(used) - 1, 1)
        if used[0] < 2 and form != "simple8":
            bits.put(0, 1)
            bits.put(used[0], 1)
        else:
            bits.put(1, 1)
            bits.put(used[0], 8)
        if len(used) == 2:
            bits.put(used[1], 8)
        return canonical(lengths)
    cl = [lengths.get(s, 0) for s in range(n)]
    if max_symbol:
        while len(cl) > 1 and cl[-1] == 0:
            cl.pop()
    toks = _cl_tokens(cl, repeat)
    if max_symbol and len(toks) < 2:
        max_symbol = False
        toks = _cl_tokens([lengths.get(s, 0) for s in range(n)], repeat)
    freq = [0] * 19
    for t, _, _ in toks:
        freq[t] += 1
    cll = huff_lengths(freq, 7)
    cenc = canonical(cll)
    bits.put(0, 1)
    num = 19
    while num > 4 and cll.get(_CL_ORDER[num - 1], 0) == 0:
        num -= 1
    bits.put(num - 4, 4)
    for i in range(num):
        bits.put(cll.get(_CL_ORDER[i], 0), 3)
    if max_symbol:
        bits.put(1, 1)
        k = 0
        while (len(toks) - 2) >> (2 + 2 * k):
            k += 1
        bits.put(k, 3)
        bits.put(len(toks) - 2, 2 + 2 * k)
    else:
        bits.put(0, 1)
    for t, v, nb in toks:
        put_symbol(bits, cenc, t)
        bits.put(v, nb)
    return canonical(lengths)


def _prefix(v):
    """(symbol, extra bits, extra value) of a length or distance-code value v >= 1."""
    d = v - 1
    if d < 4:
        return d, 0, 0
    hb = d.bit_length() - 1
    return 2 * hb + ((d >> (hb - 1)) & 1), hb - 1, d & ((1 << (hb - 1)) - 1)


def _hash(v, bits):
    return ((0x1E35A7BD * int(v)) & 0xFFFFFFFF) >> (32 - bits)


def dist_code(dist, xsize):
    """The cheapest distance code of a pixel distance: a short one where (dx, dy) is on the map."""
    for c, (dx, dy) in enumerate(_PLANE):
        if dx + dy * xsize == dist and dist >= 1:
            return c + 1
    return dist + 120


def tokens_greedy(flat, xsize, max_len=4096, min_len=3):
    """Literals and copies (length, distance) over the pixel stream: runs, the row above, an earlier triple."""
    n = len(flat)
    flat = [int(v) for v in flat]
    toks, i, seen = [], 0, {}
    while i < n:
        best, bd = 0, 0
        cands = [1, xsize]
        key = tuple(flat[i:i + 3])
        if len(key) == 3 and key in seen:
            cands.append(i - seen[key])
        for d in cands:
            if d > i or d < 1:
                continue
            l = 0
            while i + l < n and l < max_len and flat[i + l] == flat[i + l - d]:
                l += 1
            if l > best:
                best, bd = l, d
        if best >= min_len:
            toks.append(("copy", best, dist_code(bd, xsize)))
            step = best
        else:
            toks.append(("lit", flat[i]))
            step = 1
        for j in range(i, min(i + step, n - 2)):
            seen[tuple(flat[j:j + 3])] = j
        i += step
    return toks


def encode_image(bits, img, *, main=False, cache_bits=0, lz="greedy", tokens=None, meta=None, code=None):
    """One entropy-coded image (h x w uint32 ARGB).  meta: (prefix_bits, h' x w' array of group numbers); code: options
    of write_code, or a function (group, j) -> options; tokens: an explicit list instead of the writer's own."""
    h, w = img.shape
    flat = img.reshape(-1)
    if tokens is None:
        tokens = [("lit", int(v)) for v in flat] if lz == "none" else tokens_greedy(flat, w)
    if cache_bits:
        bits.put(1, 1)
        bits.put(cache_bits, 4)
    else:
        bits.put(0, 1)
    groups = 1
    if main:
        if meta is None:
            bits.put(0, 1)
        else:
            pb, gimg = meta
            gimg = np.asarray(gimg, np.uint32)
            assert gimg.shape == ((h + (1 << pb) - 1) >> pb, (w + (1 << pb) - 1) >> pb)
            bits.put(1, 1)
            bits.put(pb - 2, 3)
            encode_image(bits, (gimg << 8) | np.uint32(0xFF000000))
            groups = int(gimg.max()) + 1
    # the colour cache, as the decoder keeps it: a literal that is in it becomes a cache token
    cache = [0] * (1 << cache_bits) if cache_bits else None
    out, pos = [], 0
    for t in tokens:
        g = 0 if meta is None else int(meta[1][(pos // w) >> meta[0]][(pos % w) >> meta[0]])
        if t[0] == "lit":
            v = t[1]
            if cache is not None and cache[_hash(v, cache_bits)] == v:
                out.append((g, "cache", _hash(v, cache_bits)))
            else:
                out.append((g, "lit", v))
            if cache is not None:
                cache[_hash(v, cache_bits)] = v
            pos += 1
        elif t[0] == "cache":
            out.append((g, "cache", t[1]))
            pos += 1
        else:
            out.append((g, "copy", t[1], t[2]))
            if cache is not None:
                for j in range(pos, min(pos + t[1], len(flat))):
                    cache[_hash(flat[j], cache_bits)] = int(flat[j])
            pos += t[1]
    sizes = [256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40]
    freq = [[[0] * n for n in sizes] for _ in range(groups)]
    for t in out:
        f = freq[t[0]]
        if t[1] == "lit":
            v = t[2]
            f[0][(v >> 8) & 255] += 1
            f[1][(v >> 16) & 255] += 1
            f[2][v & 255] += 1
            f[3][v >> 24] += 1
        elif t[1] == "cache":
            f[0][280 + t[2]] += 1
        else:
            f[0][256 + _prefix(t[2])[0]] += 1
            f[4][_prefix(t[3])[0]] += 1
    encs = []
    for g in range(groups):
        row = []
        for j in range(5):
            if not any(freq[g][j]):
                freq[g][j][0] = 1  # (an unused code still has to be a code)
            opts = code(g, j) if callable(code) else (code or {})
            row.append(write_code(bits, huff_lengths(freq[g][j], 15), sizes[j], **opts))
        encs.append(row)
    for t in out:
        e = encs[t[0]]
        if t[1] == "lit":
            v = t[2]
            put_symbol(bits, e[0], (v >> 8) & 255)
            put_symbol(bits, e[1], (v >> 16) & 255)
            put_symbol(bits, e[2], v & 255)
            put_symbol(bits, e[3], v >> 24)
        elif t[1] == "cache":
            put_symbol(bits, e[0], 280 + t[2])
        else:
            s, nb, ev = _prefix(t[2])
            put_symbol(bits, e[0], 256 + s)
            bits.put(ev, nb)
            s, nb, ev = _prefix(t[3])
            put_symbol(bits, e[4], s)
            bits.put(ev, nb)


# ------------------------------------------------------------------------------------------------
# transforms (forward)
# ------------------------------------------------------------------------------------------------
def _ch(a):
    a = np.asarray(a, np.uint32)
    return np.stack([(a >> s) & 255 for s in (24, 16, 8, 0)], -1).astype(np.int64)


def _un(c):
    c = (c & 255).astype(np.uint32)
    return (c[..., 0] << 24) | (c[..., 1] << 16) | (c[..., 2] << 8) | c[..., 3]


def _tile(v, bits, h, w):
    return np.repeat(np.repeat(np.asarray(v), 1 << bits, 0), 1 << bits, 1)[:h, :w]


def _sub_shape(h, w, bits):
    return (h + (1 << bits) - 1) >> bits, (w + (1 << bits) - 1) >> bits


def predict_all(img, modes):
    """The prediction of every pixel from the (final) image, `modes` per pixel, libwebp's border rules."""
    h, w = img.shape
    flat = np.concatenate([np.zeros(w + 1, np.uint32), img.reshape(-1)])
    n = h * w
    p = np.arange(n) + w + 1
    L, T, TL, TR = (_ch(flat[p - 1]), _ch(flat[p - w]), _ch(flat[p - w - 1]), _ch(flat[p - w + 1]))
    m = np.asarray(modes).reshape(-1).copy()
    ys, xs = np.divmod(np.arange(n), w)
    m[xs == 0] = 2
    m[ys == 0] = 1
    m[0] = 0
    a2 = lambda a, b: (a + b) >> 1
    sel = (np.abs(L - TL).sum(-1) - np.abs(T - TL).sum(-1) <= 0)[:, None]
    half = a2(L, T)
    d = half - TL
    black = np.broadcast_to(np.array([255, 0, 0, 0]), L.shape)
    cand = {0: black, 1: L, 2: T, 3: TR, 4: TL, 5: a2(a2(L, TR), T), 6: a2(L, TL), 7: a2(L, T), 8: a2(TL, T), 9: a2(T, TR),
            10: a2(a2(L, TL), a2(T, TR)), 11: np.where(sel, T, L), 12: np.clip(L + T - TL, 0, 255),
            13: np.clip(half + np.where(d < 0, -((-d) // 2), d // 2), 0, 255), 14: black, 15: black}
    out = np.zeros_like(L)
    for k, v in cand.items():
        out = np.where((m == k)[:, None], v, out)
    return out.reshape(h, w, 4)


def _ctd(t, c):
    t = np.asarray(t, np.int64)
    c = np.asarray(c, np.int64)
    t = np.where(t > 127, t - 256, t)
    c = np.where(c > 127, c - 256, c)
    return (t * c) >> 5


def forward(img, transforms, bits):
    """Applies the transforms in reading order to img (h x w uint32) and writes their headers and data; returns
    the image to code.  ("predictor", size_bits, modes per tile | int), ("cross", size_bits, (g2r, g2b, r2b) per
    tile | triple), ("green",), ("palette", table | None[, indices])."""
    cur = np.asarray(img, np.uint32)
    for t in transforms:
        h, w = cur.shape
        bits.put(1, 1)
        if t[0] == "predictor":
            sb = t[1]
            sh = _sub_shape(h, w, sb)
            modes = np.full(sh, t[2], np.uint32) if np.isscalar(t[2]) else np.asarray(t[2], np.uint32).reshape(sh)
            bits.put(0, 2)
            bits.put(sb - 2, 3)
            encode_image(bits, (modes << 8) | np.uint32(0xFF000000))
            cur = _un(_ch(cur) - predict_all(cur, _tile(modes, sb, h, w)))
        elif t[0] == "cross":
            sb = t[1]
            sh = _sub_shape(h, w, sb)
            k = np.broadcast_to(np.asarray(t[2], np.uint32), sh + (3,)) if np.ndim(t[2]) == 1 else np.asarray(t[2], np.uint32).reshape(sh + (3,))
            bits.put(1, 2)
            bits.put(sb - 2, 3)
            encode_image(bits, np.uint32(0xFF000000) | (k[..., 2] << 16) | (k[..., 1] << 8) | k[..., 0])
            c = _ch(cur)
            kk = [_tile(k[..., i], sb, h, w) for i in range(3)]
            c[..., 1], c[..., 3] = (c[..., 1] - _ctd(kk[0], c[..., 2]),
                                    c[..., 3] - _ctd(kk[1], c[..., 2]) - _ctd(kk[2], c[..., 1]))
            cur = _un(c)
        elif t[0] == "green":
            bits.put(2, 2)
            c = _ch(cur)
            c[..., 1] -= c[..., 2]
            c[..., 3] -= c[..., 2]
            cur = _un(c)
        else:
            table = np.asarray(sorted(set(int(v) for v in cur.reshape(-1))) if t[1] is None else t[1], np.uint32)
            n = len(table)
            assert 1 <= n <= 256
            if len(t) > 2:
                idx = np.asarray(t[2], np.int64)
            else:
                look = {int(v): i for i, v in enumerate(table)}
                idx = np.array([look[int(v)] for v in cur.reshape(-1)], np.int64).reshape(h, w)
            bits.put(3, 2)
            bits.put(n - 1, 8)
            tc = _ch(table)
            encode_image(bits, _un(np.concatenate([tc[:1], tc[1:] - tc[:-1]]))[None, :])
            pb = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            per, pw = 8 >> pb, (w + (1 << pb) - 1) >> pb
            packed = np.zeros((h, pw), np.int64)
            for x in range(w):
                packed[:, x >> pb] |= idx[:, x] << ((x & ((1 << pb) - 1)) * per)
            cur = (np.uint32(0xFF000000) | (packed.astype(np.uint32) << 8))
    bits.put(0, 1)
    return cur


def vp8l(img, *, transforms=(), alpha=None, version=0, **kw) -> bytes:
    """The VP8L payload that decodes to img (h x w uint32 ARGB); kw: encode_image's."""
    img = np.asarray(img, np.uint32)
    h, w = img.shape
    bits = _Bits()
    bits.put(0x2F, 8)
    bits.put(w - 1, 14)
    bits.put(h - 1, 14)
    bits.put(int(bool((img >> 24 != 255).any()) if alpha is None else alpha), 1)
    bits.put(version, 3)
    cur = forward(img, transforms, bits)
    encode_image(bits, cur, main=True, **kw)
    return bits.done()


def raw_vp8l(w, h, fn, alpha=0) -> bytes:
    """A payload whose bits after the header fn(bits) writes by hand."""
    bits = _Bits()
    bits.put(0x2F, 8)
    bits.put(w - 1, 14)
    bits.put(h - 1, 14)
    bits.put(alpha, 1)
    bits.put(0, 3)
    fn(bits)
    return bits.done()


# ------------------------------------------------------------------------------------------------
# container
# ------------------------------------------------------------------------------------------------
def chunk(tag: bytes, data: bytes, pad=True) -> bytes:
    return tag + struct.pack("<I", len(data)) + data + (b"\0" if pad and len(data) & 1 else b"")


def riff(body: bytes, size=None, trailing=b"") -> bytes:
    return b"RIFF" + struct.pack("<I", 4 + len(body) if size is None else size) + b"WEBP" + body + trailing


def vp8x(w, h, flags=0) -> bytes:
    return chunk(b"VP8X", bytes([flags, 0, 0, 0]) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3])


def webp(payload: bytes, **kw) -> bytes:
    return riff(chunk(b"VP8L", payload), **kw)


def webp_x(payload, w, h, before=(), after=(), flags=None, **kw) -> bytes:
    """A VP8X file: the flags follow the chunks unless given."""
    if flags is None:
        tags = [c[:4] for c in list(before) + list(after)]
        flags = (0x20 if b"ICCP" in tags else 0) | (0x08 if b"EXIF" in tags else 0) | (0x04 if b"XMP " in tags else 0)
        flags |= 0x10 if payload[4] & 0x10 else 0
    return riff(vp8x(w, h, flags) + b"".join(before) + chunk(b"VP8L", payload) + b"".join(after), **kw)


def argb(rgb, a=255):
    rgb = np.asarray(rgb, np.uint32)
    al = np.broadcast_to(np.asarray(a, np.uint32), rgb.shape[:2])
    return (al << 24) | (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]


def rgb_of(img):
    img = np.asarray(img, np.uint32)
    return np.stack([(img >> 16) & 255, (img >> 8) & 255, img & 255], -1).astype(np.uint8)


def picture(w, h, seed=0, noise=6):
    """A photo-like RGB array: smooth ramps and waves with a little noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 90 * np.sin(x / 9.0 + seed) + 30 * np.cos(y / 5.0), x * 200 // max(w - 1, 1) + y // 2,
                  (x + 2 * y + 40 * seed) % 256], -1)
    return np.clip(a + rng.integers(-noise, noise + 1, a.shape), 0, 255).astype(np.uint8)


def few_colours(w, h, n, seed=0):
    """(image, table) of n random colours in blocks and speckles."""
    rng = np.random.default_rng(seed)
    table = argb(rng.integers(0, 256, (n, 1, 3)))[:, 0]
    y, x = np.mgrid[0:h, 0:w]
    idx = ((x // 3 + y // 2) + rng.integers(0, 2, (h, w)) * rng.integers(0, n, (h, w))) % n
    return table[idx], table, idx


def pil_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_outcome(data: bytes):
    """("ok", pixels) or ("err", exception type) of the reference decode."""
    try:
        return "ok", pil_rgb(data)
    except Exception as e:  # noqa: BLE001
        return "err", type(e)


_cache: dict = {}


def native():
    """(name, bytes, expected RGB) of the files the GPU path must decode itself."""
    if "native" in _cache:
        return _cache["native"]
    out = []

    def add(name, img, data=None, expect=None, **kw):
        img = np.asarray(img, np.uint32)
        out.append((name, webp(vp8l(img, **kw)) if data is None else data, rgb_of(img) if expect is None else expect))

    rng = np.random.default_rng(7)
    base = argb(picture(37, 29, 1))
    add("plain_literals", base, lz="none")
    add("plain_lz", base)
    add("one_pixel", argb(picture(1, 1, 2)))
    add("alpha_values", argb(picture(37, 29, 1), rng.integers(0, 256, (29, 37))))
    add("alpha_bit_without_alpha", base, alpha=1)
    # widths for the packings and the 4-pixel tiles, heights for the band hand-over of the skewed wavefront
    for w in (1, 2, 3, 5, 7, 9, 15, 17):
        add(f"pred_w{w}", argb(picture(w, 11, w)), transforms=[("predictor", 2, rng.integers(0, 14, _sub_shape(11, w, 2)))])
    for h in (1, 63, 64, 65, 130):
        add(f"pred_h{h}", argb(picture(19, h, h)), transforms=[("predictor", 3, rng.integers(0, 14, _sub_shape(h, 19, 3)))])
    for m in range(16):
        add(f"pred_mode{m}", argb(picture(21, 13, m, noise=40)), transforms=[("predictor", 4, m)])
    for sb in range(2, 10):
        add(f"size_bits{sb}", argb(picture(33, 9, sb)),
            transforms=[("predictor", sb, rng.integers(0, 14, _sub_shape(9, 33, sb))),
                        ("cross", sb, rng.integers(0, 256, _sub_shape(9, 33, sb) + (3,)))])
    add("green_only", base, transforms=[("green",)])
    add("cross_only", base, transforms=[("cross", 2, rng.integers(0, 256, _sub_shape(29, 37, 2) + (3,)))])
    p = ("predictor", 2, rng.integers(0, 14, _sub_shape(29, 37, 2)))
    c = ("cross", 3, (250, 7, 130))
    g = ("green",)
    for k, order in enumerate(([p, c, g], [g, p, c], [c, g, p], [g, c, p], [p, g, c], [c, p, g])):
        add(f"order{k}", base, transforms=order)
    for n in (2, 4, 16, 17, 256):
        img, table, _ = few_colours(31 if n != 256 else 33, 10, n, n)
        add(f"palette{n}", img, transforms=[("palette", table)])
    # rows that pack into one word or less, and a predictor on a packed width of 1: the in-place unpack's tight shapes
    for w in (1, 2, 3, 5, 7, 9):
        for n in (2, 4, 16):
            img, table, _ = few_colours(w, 70, n, 10 * w + n)
            add(f"palette{n}_w{w}", img, transforms=[("palette", table)])
        img, table, _ = few_colours(w, 70, 4, w)
        add(f"palette4_w{w}_then_predictor", img, transforms=[("palette", table), ("predictor", 2, rng.integers(0, 14, _sub_shape(70, (w + 3) // 4, 2)))])
        add(f"predictor_then_palette_w{w}", img, transforms=[("predictor", 2, 1), ("palette", None)])
    img, table, _ = few_colours(31, 20, 4, 3)
    pp = ("predictor", 2, rng.integers(0, 14, _sub_shape(20, 8, 2)))  # (on the packed width: 31 pixels in 8 words)
    add("palette_then_predictor", img, transforms=[("palette", table), pp])
    add("palette_then_green_cross", img, transforms=[("palette", table), g, ("cross", 2, (3, 200, 90))])
    add("predictor0_then_palette", img, transforms=[("predictor", 2, 0), ("palette", None)])
    add("green_then_palette", img, transforms=[g, ("palette", None)])
    add("all_four", img, transforms=[("predictor", 3, 1), c, g, ("palette", None)])
    # an index at or beyond the table: 0x00000000 (libwebp zero-fills the expanded map)
    idx = rng.integers(0, 16, (10, 31))
    tab = argb(rng.integers(0, 256, (5, 1, 3)))[:, 0]
    full = np.concatenate([tab, np.zeros(11, np.uint32)])
    add("palette_index_beyond", full[idx], transforms=[("palette", tab, idx)], alpha=0)
    idx = rng.integers(0, 256, (10, 33))
    tab = argb(rng.integers(0, 256, (17, 1, 3)))[:, 0]
    add("palette17_index_beyond", np.concatenate([tab, np.zeros(239, np.uint32)])[idx], transforms=[("palette", tab, idx)], alpha=0)
    # prefix codes
    add("normal_codes_no_repeat", base, code=dict(form="normal", repeat=False))
    add("normal_codes_max_symbol", base, code=dict(form="normal", max_symbol=True))
    flat = argb(np.full((9, 12, 3), 77, np.uint8))
    add("single_symbol_simple", flat, lz="none")
    add("single_symbol_normal", flat, lz="none", code=dict(form="normal"))
    add("single_symbol_lz", flat)
    two = argb(np.where((np.arange(108).reshape(9, 12, 1) * 7 % 5) < 2, 0, 1).astype(np.uint8) * np.ones(3, np.uint8))
    add("simple_two_symbols", two, lz="none")
    ramp = argb(np.stack([np.arange(256).reshape(16, 16)] * 3, -1))
    add("all_lengths_8", ramp, lz="none", code=dict(form="normal"))  # (one code-length symbol: repeat 16 from the initial 8)
    # colour cache
    for cb in (1, 4, 11):
        img, _, _ = few_colours(40, 30, 9, cb)
        add(f"cache{cb}", img, cache_bits=cb)
        add(f"cache{cb}_literals", img, cache_bits=cb, lz="none")
    # a long copy over a small cache: the slots hold the last pixel of each hash, then cache tokens read them
    row = argb(rng.integers(0, 256, (1, 64, 3)))[0]
    last = int(row[-1])
    other = [int(v) for v in row if _hash(v, 1) != _hash(last, 1)][-1]
    tail = np.array([last, other] * 32, np.uint32)
    add("long_copy_small_cache", np.concatenate([np.tile(row, (9, 1)), tail[None, :]]), cache_bits=1)
    add("long_copy_cache3", np.concatenate([np.tile(row, (9, 1)), row[None, ::-1]]), cache_bits=3)
    # meta-prefix images
    big = argb(picture(45, 33, 5))
    add("meta_1_group", big, meta=(2, np.zeros(_sub_shape(33, 45, 2), np.int64)))
    add("meta_2_groups", big, meta=(3, np.indices(_sub_shape(33, 45, 3)).sum(0) % 2), cache_bits=5)
    add("meta_many_groups", big, meta=(3, np.arange(30).reshape(5, 6)))
    add("meta_bits9", big, meta=(9, np.zeros((1, 1), np.int64)))
    add("meta_max_groups", argb(picture(64, 64, 6)), meta=(2, np.arange(MAX_GROUPS).reshape(16, 16)), lz="none")
    # copies through each kind of distance code
    pat = argb(picture(24, 20, 9, noise=0))
    tiled = np.tile(pat[:10, :12], (2, 2))
    for code_ in (1, 2, 3, 4, 25, 60, 97, 120):
        dx, dy = _PLANE[code_ - 1]
        # pixels up to row 8 as literals, then every pixel a copy of length 1 through the short code
        src = argb(picture(24, 20, code_, noise=30)).reshape(-1).copy()
        toks = []
        for i in range(len(src)):
            d = plane_distance(code_, 24)
            if i >= 9 * 24 and i % 3 == 0:
                src[i] = src[i - d]
                toks.append(("copy", 1, code_))
            else:
                toks.append(("lit", int(src[i])))
        add(f"short_code{code_}", src.reshape(20, 24), tokens=toks)
    # in a 3-wide image (-3, 1) gives 0 and (-4, 1) gives -1: both below 1, so the distance is 1
    src = argb(picture(3, 30, 4, noise=30)).reshape(-1).copy()
    below = [_PLANE.index((-3, 1)) + 1, _PLANE.index((-4, 1)) + 1]
    toks = []
    for i in range(len(src)):
        if i > 10 and i % 4 == 0:
            src[i] = src[i - 1]
            toks.append(("copy", 1, below[(i // 4) & 1]))
        else:
            toks.append(("lit", int(src[i])))
    add("dist_below_1", src.reshape(30, 3), tokens=toks)
    run = np.concatenate([pat.reshape(-1)[:5], np.tile(pat.reshape(-1)[:5], 199)])[:24 * 40]
    add("long_overlapped_run", run.reshape(40, 24), tokens=[("lit", int(v)) for v in run[:5]] + [("copy", 24 * 40 - 5, 5 + 120)])
    add("tiled_lz", tiled)
    add("big_320x240", argb(picture(320, 240, 11)), transforms=[("predictor", 4, rng.integers(0, 14, _sub_shape(240, 320, 4))),
                                                                ("cross", 5, (5, 250, 9)), g], cache_bits=6,
        meta=(5, np.indices(_sub_shape(240, 320, 5)).sum(0) % 3))
    # containers
    pay = vp8l(base)
    icc, exif, xmp = chunk(b"ICCP", b"p" * 301), chunk(b"EXIF", b"Exif\0\0II*\0\x08\0\0\0\0\0"), chunk(b"XMP ", b"<x/>")
    add("vp8x_plain", base, data=webp_x(pay, 37, 29))
    add("vp8x_iccp_exif", base, data=webp_x(pay, 37, 29, before=[icc], after=[exif]))
    add("vp8x_xmp_unknown_odd", base, data=webp_x(pay, 37, 29, before=[icc, chunk(b"abcd", b"123")], after=[exif, xmp, chunk(b"zzzz", b"7")]))
    add("vp8x_flags_without_chunks", base, data=webp_x(pay, 37, 29, flags=0x2C))
    add("trailing_bytes", base, data=webp(pay, trailing=b"junk after the riff size"))
    add("vp8x_trailing_bytes", base, data=webp_x(pay, 37, 29, after=[exif], trailing=b"\0" * 9))
    odd = vp8l(base, lz="none")
    odd = odd if len(odd) & 1 else odd + b"\0"
    add("odd_payload", base, data=webp(odd))
    add("complete_code_4x4", np.zeros((4, 4), np.uint32), data=_hand_codes({0: 1, 1: 2, 2: 2}))
    for name, data, img in pillow_files():
        out.append((name, data, img))
    _cache["native"] = out
    return out


def pillow_manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def pillow_input(entry) -> np.ndarray:
    """The deterministic input array of a committed Pillow file (RGB, or RGBA with random alpha)."""
    w, h, seed = entry["width"], entry["height"], entry["seed"]
    if entry["kind"] == "four":
        a = rgb_of(few_colours(w, h, 4, seed)[0])
    else:
        a = picture(w, h, seed)
    if entry["mode"] == "RGBA":
        a = np.dstack([a, np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)])
    return a


def pillow_files():
    """(name, bytes, expected RGB) of the files Pillow wrote (tests/golden/webp/, written by make_pillow_files)."""
    out = []
    for e in pillow_manifest():
        with open(os.path.join(GOLDEN, e["file"]), "rb") as f:
            out.append(("pillow_" + e["file"][:-5], f.read(), pillow_input(e)[..., :3]))
    return out


def make_pillow_files():
    """Writes tests/golden/webp/ (run once, with a Pillow that has WebP): the manifest's save arguments."""
    from PIL import Image
    os.makedirs(GOLDEN, exist_ok=True)
    entries = []
    for file, w, h, seed, kind, mode, save in (
            ("m0.webp", 96, 64, 1, "picture", "RGB", dict(method=0)), ("m4.webp", 131, 67, 2, "picture", "RGB", dict(method=4)),
            ("m6.webp", 160, 120, 3, "picture", "RGB", dict(method=6, quality=100)),
            ("rgba_exact.webp", 101, 67, 4, "picture", "RGBA", dict(exact=True)),
            ("four.webp", 120, 90, 5, "four", "RGB", dict()),
            ("icc_exif.webp", 64, 48, 6, "picture", "RGB", dict(icc_profile="x" * 301, exif="Exif\0\0II*\0\x08\0\0\0\0\0"))):
        e = dict(file=file, width=w, height=h, seed=seed, kind=kind, mode=mode, save=save)
        buf = io.BytesIO()
        Image.fromarray(pillow_input(e), mode).save(buf, "WEBP", lossless=True,
                                                    **{k: v.encode("latin-1") if isinstance(v, str) else v for k, v in save.items()})
        with open(os.path.join(GOLDEN, file), "wb") as f:
            f.write(buf.getvalue())
        entries.append(e)
    with open(os.path.join(GOLDEN, "manifest.json"), "w") as f:
        json.dump(entries, f, indent=1)


def _lossy(alpha=False) -> bytes:
    """A lossy key frame's header is all the container walk reads: 16 x 8, no real data."""
    vp8 = chunk(b"VP8 ", bytes([0x10, 0x02, 0x00, 0x9D, 0x01, 0x2A, 16, 0, 8, 0]) + bytes(20))
    if not alpha:
        return riff(vp8)
    return riff(vp8x(16, 8, 0x10) + chunk(b"ALPH", bytes(9)) + vp8)


def refused():
    """(name, bytes) of valid files outside the subset: SDSJ_UNSUPPORTED, from the header unless the name ends in
    "_dev" (the device's verdict)."""
    base = argb(picture(37, 29, 1))
    pay = vp8l(base)
    anmf = chunk(b"ANMF", bytes(16) + chunk(b"VP8L", pay))
    return [
        ("lossy", _lossy()),
        ("lossy_alpha", _lossy(True)),
        ("animated_flag", riff(vp8x(37, 29, 0x02) + chunk(b"ANIM", bytes(6)) + anmf)),
        ("anim_chunk_without_flag", riff(vp8x(37, 29, 0) + chunk(b"ANIM", bytes(6)) + chunk(b"VP8L", pay))),
        ("canvas_differs", webp_x(pay, 40, 29)),
        ("version_1", webp(vp8l(base, version=1))),
        ("too_many_groups_dev", webp(vp8l(argb(picture(68, 68, 6)), meta=(2, np.arange(289).reshape(17, 17)), lz="none"))),
    ]


def _hand_codes(lengths_green) -> bytes:
    """A 4 x 4 file written by hand: no transform, cache or meta-prefix image; the green code from its lengths, the
    other four codes of one symbol; every pixel the green code's first symbol (0)."""
    def fn(b):
        b.put(0, 3)
        write_code(b, lengths_green, 280, form="normal")
        for _ in range(4):
            write_code(b, {0: 1}, 256, form="simple")
        b.put(0, 32)
    return webp(raw_vp8l(4, 4, fn))


def _resize(data: bytes, payload_len: int) -> bytes:
    """A bare file cut to payload_len bytes of VP8L payload, its chunk and RIFF sizes put right."""
    pay = data[20:20 + payload_len]
    return webp(pay)


def damaged():
    """(name, bytes) of files PIL refuses or this path is not sure about; the names of those the container gives
    away (SDSJ_CORRUPT from the probe) end in "_hdr"."""
    base = argb(picture(37, 29, 1))
    rng = np.random.default_rng(3)
    trans = [("predictor", 2, rng.integers(0, 14, _sub_shape(29, 37, 2))), ("cross", 2, (250, 7, 130)), ("green",)]
    good = webp(vp8l(base, transforms=trans, cache_bits=4, meta=(3, np.indices(_sub_shape(29, 37, 3)).sum(0) % 2)))
    n = len(good) - 20
    img4, tab4, _ = few_colours(31, 20, 4, 3)
    pal = webp(vp8l(img4, transforms=[("palette", tab4)]))

    return [
        ("riff_size_past_input_hdr", good[:len(good) - 7]),
        ("chunk_size_past_riff_hdr", good[:16] + struct.pack("<I", n + 40) + good[20:]),
        ("cut_in_first_transform", _resize(good, 9)),
        ("cut_in_transforms", _resize(good, 60)),
        ("cut_in_codes", _resize(good, n // 3)),
        ("cut_in_pixels", _resize(good, n - 40)),
        ("cut_last_bytes", _resize(good, n - 3)),
        ("cut_in_colour_table", _resize(pal, 12)),
        ("over_subscribed_code", _hand_codes({0: 1, 1: 1, 2: 1})),
        ("incomplete_code", _hand_codes({0: 1, 1: 2})),
        ("copy_before_first_pixel", webp(vp8l(base, tokens=[("copy", 5, 121)] + [("lit", int(v)) for v in base.reshape(-1)[5:]]))),
        ("copy_past_last_pixel", webp(vp8l(base, tokens=[("lit", int(v)) for v in base.reshape(-1)[:-3]] + [("copy", 9, 121)]))),
        ("repeated_transform", webp(vp8l(base, transforms=[("green",), ("cross", 2, (1, 2, 3)), ("green",)]))),
        ("cache_bits_12", webp(raw_vp8l(4, 4, lambda b: (b.put(0, 1), b.put(1, 1), b.put(12, 4), b.put(0, 64))))),
        ("vp8x_reserved_flag_hdr", webp_x(vp8l(base), 37, 29, flags=0x01)),
        ("two_image_chunks_hdr", riff(vp8x(37, 29) + chunk(b"VP8L", vp8l(base)) * 2)),
        ("bad_signature_byte_hdr", webp(b"\x2e" + vp8l(base)[1:])),
    ]
