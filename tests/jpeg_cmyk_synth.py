"""Four-component JPEG files of the opt-in "jpeg-cmyk" subset (test input generator): Adobe CMYK and YCCK, sequential,
in one interleaved scan or several, and the cases that stay refused.

Pillow writes a CMYK image as a four-component file with an Adobe marker (subsampling 0 / 1 / 2, optimised tables,
restart markers); everything else -- chosen sampling factors per component, component ids, the Adobe transform value, a
missing Adobe marker, JFIF beside it, SOF1, restart intervals, components spread over several scans -- is written here
from chosen quantised coefficients with the pieces of tests/jpeg_ext_synth.py (its header writer, bit packer, symbol
writers and random coefficients): write4 takes the scan grouping, so the same coefficients can be written as one
interleaved scan and as several.  The reference of every file is PIL itself (jpeg_ext_synth.pil_rgb)."""
from __future__ import annotations

import functools
import io

import numpy as np

from tests import jpeg_ext_synth as J
from tests.golden import coefjpeg as C

CMYK, CMYK_SCANS, CMYK_EXT = ("jpeg", "jpeg-cmyk"), ("jpeg", "jpeg-cmyk", "jpeg-scans"), ("jpeg", "jpeg-cmyk", "jpeg-ext")
SIZES = [(5, 9), (17, 23), (50, 37), (33, 70), (97, 65)]  # (width, height)
BIG = (320, 240)
S1 = ((1, 1), (1, 1), (1, 1), (1, 1))
S_PHOTOSHOP = ((2, 2), (1, 1), (1, 1), (2, 2))  # Y and K full, the chroma pair halved: 10 blocks per MCU
S_H2 = ((2, 1), (1, 1), (1, 1), (2, 1))
S_FIRST = ((2, 2), (1, 1), (1, 1), (1, 1))      # only the first component full (K fancy-upsampled)
S_411 = ((4, 1), (1, 1), (1, 1), (1, 1))        # ratio 4: "jpeg-ext" as well
IDS_CMYK, IDS_1234 = (67, 77, 89, 75), (1, 2, 3, 4)
ALL = ((0, 1, 2, 3),)
GROUPS = {"c-m-y-k": ((0,), (1,), (2,), (3,)), "cmy-k": ((0, 1, 2), (3,)), "k-cmy": ((3,), (0, 1, 2))}
JFIF = J.JFIF


def adobe(transform: int) -> bytes:
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


def write4(w, h, samp, blocks, q, groups=ALL, sof=0xC0, restart=0, ids=IDS_1234, lead=b"") -> bytes:
    """A sequential file of len(samp) components.  groups: per scan the frame indices of its components, in scan
    order (one group of all of them: a single interleaved scan).  restart: the restart interval in MCUs of every
    scan (a single-component scan's MCU is one block).  lead: marker segments right after SOI."""
    tabs, dc, ac = J._tables()
    hmax, vmax, mcux, mcuy = J._geometry(w, h, samp)
    seg = J._head(w, h, samp, q, sof, ids, lead, restart)
    for group in groups:
        sos = bytes([len(group)])
        for ci in group:
            sos += bytes([ids[ci], 0x00 if ci == 0 else 0x11])
        J._marker(seg, 0xDA, sos + bytes([0, 63, 0]))
        if len(group) == 1:
            ci = group[0]
            dw, dh = -(-w * samp[ci][0] // hmax), -(-h * samp[ci][1] // vmax)
            mcus = [[(ci, y, x)] for y in range(-(-dh // 8)) for x in range(-(-dw // 8))]
        else:
            mcus = [[(ci, my * samp[ci][1] + dy, mx * samp[ci][0] + dx)
                     for ci in group for dy in range(samp[ci][1]) for dx in range(samp[ci][0])]
                    for my in range(mcuy) for mx in range(mcux)]
        bw = J._Bits()
        pred = [0] * len(samp)
        for m, mcu in enumerate(mcus):
            if restart and m and m % restart == 0:
                bw.flush()
                bw.out.extend(bytes([0xFF, 0xD0 + (m // restart - 1) % 8]))
                pred = [0] * len(samp)
            for ci, y, x in mcu:
                t = 0 if ci == 0 else 1
                blk = blocks[ci][y, x]
                J._put_dc(bw, dc[t], int(blk[0]) - pred[ci])
                pred[ci] = int(blk[0])
                J._put_ac(bw, ac[t], blk)
        bw.flush()
        seg += bw.out
    return bytes(seg + b"\xff\xd9")


def pillow_cmyk(w, h, seed, **kw) -> bytes:
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * (3 + c) + yy * (5 - c) + rng.integers(0, 24, (h, w))) % 256 for c in range(4)], -1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a, "CMYK").save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _made(w, h, samp, seed, **kw):
    blocks, q = J.random_blocks(w, h, samp, seed)
    return write4(w, h, samp, blocks, q, **kw)


@functools.lru_cache(maxsize=None)
def pillow_files() -> tuple:
    """(name, bytes, formats, None): what Pillow writes for a CMYK image."""
    out = [("pil-ss0-17x23", pillow_cmyk(17, 23, 1, quality=90, subsampling=0)),
           ("pil-ss1-50x37", pillow_cmyk(50, 37, 2, quality=85, subsampling=1)),
           ("pil-ss2-33x70", pillow_cmyk(33, 70, 3, quality=88, subsampling=2)),
           ("pil-ss2-5x9", pillow_cmyk(5, 9, 4, quality=92, subsampling=2)),
           ("pil-opt-97x65", pillow_cmyk(97, 65, 5, quality=80, subsampling=2, optimize=True)),
           ("pil-rst-rows-50x37", pillow_cmyk(50, 37, 6, quality=85, subsampling=2, restart_marker_rows=1)),
           ("pil-rst-blocks-97x65", pillow_cmyk(97, 65, 7, quality=85, subsampling=0, restart_marker_blocks=1)),
           (f"pil-ss2-{BIG[0]}x{BIG[1]}", pillow_cmyk(*BIG, 8, quality=90, subsampling=2))]
    return tuple((n, d, CMYK, None) for n, d in out)


@functools.lru_cache(maxsize=None)
def writer_files() -> tuple:
    """(name, bytes, formats, None): single interleaved scans from the writer."""
    a0, a1, a2 = adobe(0), adobe(1), adobe(2)
    mcux97 = -(-97 // 16)
    out = [("cmyk-ids-cmyk-50x37", _made(50, 37, S1, 11, ids=IDS_CMYK, lead=a0)),
           ("cmyk-ids-1234-33x70", _made(33, 70, S1, 12, ids=IDS_1234, lead=a0)),
           ("cmyk-first-5x9", _made(5, 9, S_FIRST, 13, ids=IDS_CMYK, lead=a0)),
           ("cmyk-first-97x65", _made(97, 65, S_FIRST, 14, ids=IDS_1234, lead=a0)),
           ("ycck-444-17x23", _made(17, 23, S1, 15, lead=a2)),
           ("ycck-photoshop-50x37", _made(50, 37, S_PHOTOSHOP, 16, lead=a2)),
           ("ycck-photoshop-97x65", _made(97, 65, S_PHOTOSHOP, 17, ids=IDS_CMYK, lead=a2)),
           ("ycck-photoshop-5x9", _made(5, 9, S_PHOTOSHOP, 18, lead=a2)),
           ("ycck-h2-33x70", _made(33, 70, S_H2, 19, lead=a2)),
           ("cmyk-sof1-50x37", _made(50, 37, S1, 20, sof=0xC1, lead=a0)),
           ("ycck-sof1-photoshop-33x70", _made(33, 70, S_PHOTOSHOP, 21, sof=0xC1, lead=a2)),
           ("cmyk-dri1-50x37", _made(50, 37, S1, 22, restart=1, lead=a0)),
           ("ycck-dri-row-97x65", _made(97, 65, S_PHOTOSHOP, 23, restart=mcux97, lead=a2)),
           ("no-adobe-17x23", _made(17, 23, S1, 24, ids=IDS_CMYK)),
           ("no-adobe-photoshop-50x37", _made(50, 37, S_PHOTOSHOP, 25)),
           ("adobe1-33x70", _made(33, 70, S1, 26, lead=a1)),
           ("jfif-adobe2-50x37", _made(50, 37, S_H2, 27, lead=JFIF + a2))]
    return tuple((n, d, CMYK, None) for n, d in out)


@functools.lru_cache(maxsize=None)
def multiscan_files() -> tuple:
    """(name, bytes, formats, the same coefficients as one interleaved scan): components in several scans."""
    out = []
    cases = [("c-m-y-k", 50, 37, S1, adobe(0), 0), ("cmy-k", 33, 70, S_PHOTOSHOP, adobe(2), 0),
             ("k-cmy", 97, 65, S_FIRST, adobe(0), 0), ("c-m-y-k", 17, 23, S_PHOTOSHOP, adobe(2), 3),
             ("cmy-k", 5, 9, S_H2, adobe(2), 0)]
    for k, (g, w, h, samp, lead, ri) in enumerate(cases):
        blocks, q = J.random_blocks(w, h, samp, 40 + k)
        out.append((f"scans-{g}-{w}x{h}-dri{ri}", write4(w, h, samp, blocks, q, GROUPS[g], restart=ri, lead=lead),
                    CMYK_SCANS, write4(w, h, samp, blocks, q, lead=lead)))
    # EOI after three of four scans: the K plane decodes from zero coefficients
    blocks, q = J.random_blocks(50, 37, S_PHOTOSHOP, 49)
    zero_k = blocks[:3] + [np.zeros_like(blocks[3])]
    out.append(("scans-eoi-after-three", write4(50, 37, S_PHOTOSHOP, blocks, q, GROUPS["c-m-y-k"][:3], lead=adobe(2)),
                CMYK_SCANS, write4(50, 37, S_PHOTOSHOP, zero_k, q, lead=adobe(2))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ext_files() -> tuple:
    return (("cmyk-411-50x37", _made(50, 37, S_411, 51, lead=adobe(0)), CMYK_EXT, None),
            ("ycck-411-33x70", _made(33, 70, S_411, 52, lead=adobe(2)), CMYK_EXT, None))


@functools.lru_cache(maxsize=None)
def fixtures() -> tuple:
    """Every file the bit decodes: UNSUPPORTED without it, OK under the mask named with it."""
    return pillow_files() + writer_files() + multiscan_files() + ext_files()


N_FIXTURES = 8 + 17 + 6 + 2


@functools.lru_cache(maxsize=None)
def refused() -> tuple:
    """(name, bytes, gpu_formats under which it is still refused, PIL's outcome class "ok" / "err")."""
    multi = multiscan_files()[0][1]
    return (("progressive-pillow", pillow_cmyk(50, 37, 61, quality=85, progressive=True), CMYK_SCANS + ("jpeg-ext",), "ok"),
            ("sixteen-blocks", _made(50, 37, ((2, 2),) * 4, 62, lead=adobe(0)), CMYK_SCANS + ("jpeg-ext",), "err"),
            ("fractional", _made(50, 37, ((3, 1), (2, 1), (1, 1), (1, 1)), 63, lead=adobe(0)), CMYK_SCANS + ("jpeg-ext",), "err"),
            ("multiscan-without-scans", multi, CMYK, "ok"),
            ("ratio4-without-ext", ext_files()[0][1], CMYK, "ok"))


@functools.lru_cache(maxsize=None)
def damaged() -> tuple:
    """(name, bytes, PIL's outcome class): the scan cut in half (PIL raises OSError), the same with EOI appended (PIL
    decodes it), a flipped byte in the scan whose neighbours are not FF, and the AC table the scan uses made invalid
    (its code lengths oversubscribed: PIL raises)."""
    whole = _made(50, 37, S_PHOTOSHOP, 70, lead=adobe(2))
    sos = whole.rindex(b"\xff\xda")
    cut = whole[:len(whole) - (len(whole) - sos) // 2]
    if cut[-1] == 0xFF:
        cut = cut[:-1]
    b = bytearray(whole)
    p = sos + 12 + 40
    while 0xFF in (b[p - 1], b[p], b[p + 1]) or b[p] ^ 0x5A == 0xFF:
        p += 1
    b[p] ^= 0x5A
    bad = bytearray(whole)
    tabs, _, _ = J._tables()
    bits, vals = tabs[(1, 1)]
    at = whole.index(bytes([0xFF, 0xC4]) + (19 + len(vals)).to_bytes(2, "big") + bytes([0x11]))
    assert bad[at + 5] == 0 and bad[at + 20] > 3
    bad[at + 5] = 3   # three codes of length 1 ...
    bad[at + 20] -= 3  # ... taken from length 16: the segment's length still fits
    return (("truncated-scan", cut, "err"), ("truncated-scan-eoi", cut + b"\xff\xd9", "ok"),
            ("flipped-byte", bytes(b), "ok"), ("bad-dht", bytes(bad), "err"))


def ycck_file(data: bytes) -> bool:
    """libjpeg's default_decompress_parms for four components: YCCK when an Adobe marker has a transform other than 0."""
    p = data.find(b"\xff\xee\x00\x0eAdobe")
    return p >= 0 and data[p + 15] != 0


def as_transform0(data: bytes) -> bytes:
    """The same file with its Adobe transform byte set to 0: libjpeg then hands the planes over unconverted (CMYK),
    so PIL's CMYK-mode decode of it is 255 - the upsampled planes of the original."""
    p = data.find(b"\xff\xee\x00\x0eAdobe")
    assert p >= 0
    return data[:p + 15] + b"\x00" + data[p + 16:]


def cmyk_to_rgb(planes: np.ndarray, ycck: bool) -> np.ndarray:
    """The colour steps of k_cmyk on full-resolution samples [..., 4] as libjpeg hands them to Pillow before any
    conversion (uint8): ycck_cmyk_convert for YCCK, the inversion of Pillow's "CMYK;I" unpacker, Convert.c cmyk2rgb."""
    s = planes.astype(np.int64)
    c = s[..., :3].copy()
    if ycck:
        y, cb, cr = s[..., 0], s[..., 1] - 128, s[..., 2] - 128
        r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
        g = np.clip(y + ((-46802 * cr + (-22554 * cb + 32768)) >> 16), 0, 255)
        b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
        c = 255 - np.stack([r, g, b], -1)
    ink = 255 - c                # "CMYK;I"
    nk = s[..., 3:4]             # 255 - (255 - K)
    t = ink * nk + 128
    return np.clip(nk - (((t >> 8) + t) >> 8), 0, 255).astype(np.uint8)
