"""Progressive four-component JPEG files of the opt-in "jpeg-cmyk-prog" subset (test input generator): SOF2 CMYK and
YCCK, whole and cut short, and the cases that stay refused.

Pillow writes a CMYK image with progressive=True as a four-component SOF2 file of 18 scans (an interleaved DC scan with
Al = 1, per-component AC bands 1-5 and 6-63 with Al = 2, their refinements down to Al = 0, an interleaved DC
refinement); subsampling touches the first component only.  Their YCCK twins are the same bytes with another Adobe
transform value, or without the Adobe segment.  What Pillow cannot write -- chosen sampling factors per component (a
subsampled K, Photoshop's 2x2,1x1,1x1,2x2), DC scans over fewer than four components, free component ids, DRI -- comes
from write4p, a spectral-selection writer on the pieces of tests/jpeg_ext_synth.py and tests/jpeg_cmyk_synth.py: DC scans
code the differences only, an AC scan is the sequential run/size coding of its band with symbol 0x00 as end-of-block
(Ah = Al = 0).  Cut files end before scan j, or in the middle of a scan, with or without EOI: libjpeg smooths the
blocks of such a file in all four components.

Every fixture is (name, bytes, gpu_formats it needs, PIL's outcome class "ok" / "err"); the reference of every "ok"
file is PIL itself (jpeg_ext_synth.pil_rgb)."""
from __future__ import annotations

import functools

from tests import jpeg_cmyk_synth as S
from tests import jpeg_ext_synth as J

PROG, PROG_EXT = ("jpeg-cmyk-prog",), ("jpeg-cmyk-prog", "jpeg-ext")
MIXED = ("jpeg-cmyk-prog", "jpeg-ext", "jpeg-scans")  # 1537 + 64 + 128
PIL_SIZES = [(1, 1), (5, 9), (17, 23), (50, 37), (130, 70)]  # (width, height)
QUALITIES = (30, 85, 95)
S_KSUB = ((2, 1), (2, 1), (2, 1), (1, 1))  # K is the subsampled component
DC_ALL, DC_EACH, DC_3_1 = ((0, 1, 2, 3),), ((0,), (1,), (2,), (3,)), ((0, 1, 2), (3,))


# -- the writer ----------------------------------------------------------------------------------------------
def _put_band(bw, codes, blk, ss, se):
    """Coefficients ss..se of one block as an AC first scan codes them with Al = 0 and no EOB runs."""
    run = 0
    last = max([k for k in range(ss, se + 1) if blk[k] != 0], default=ss - 1)
    for k in range(ss, last + 1):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*codes[0xF0])
            run -= 16
        s = J.C._category(v)
        bw.put(*codes[(run << 4) | s])
        bw.put(v if v > 0 else v - 1 + (1 << s), s)
        run = 0
    if last < se:
        bw.put(*codes[0x00])


def write4p(w, h, samp, blocks, q, dc_groups=DC_ALL, bands=((1, 63),), restart=0, ids=S.IDS_1234, lead=b"") -> bytes:
    """A progressive (SOF2) file of len(samp) components, spectral selection only.  dc_groups: per DC scan the frame
    indices of its components; bands: the (Ss, Se) bands, each coded in one scan per component over that component's
    own block raster; restart: the restart interval in MCUs of every scan (a single-component scan's MCU is a block)."""
    _, dc, ac = J._tables()
    hmax, vmax, mcux, mcuy = J._geometry(w, h, samp)
    seg = J._head(w, h, samp, q, 0xC2, ids, lead, restart)

    def scan(sos, mcus, put):
        J._marker(seg, 0xDA, sos)
        bw = J._Bits()
        pred = [0] * len(samp)
        for m, mcu in enumerate(mcus):
            if restart and m and m % restart == 0:
                bw.flush()
                bw.out.extend(bytes([0xFF, 0xD0 + (m // restart - 1) % 8]))
                pred = [0] * len(samp)
            for ci, y, x in mcu:
                put(bw, ci, blocks[ci][y, x], pred)
        bw.flush()
        seg.extend(bw.out)

    def own_raster(ci):
        dw, dh = -(-w * samp[ci][0] // hmax), -(-h * samp[ci][1] // vmax)
        return [[(ci, y, x)] for y in range(-(-dh // 8)) for x in range(-(-dw // 8))]

    def put_dc(bw, ci, blk, pred):
        J._put_dc(bw, dc[0 if ci == 0 else 1], int(blk[0]) - pred[ci])
        pred[ci] = int(blk[0])

    for group in dc_groups:
        sos = bytes([len(group)])
        for ci in group:
            sos += bytes([ids[ci], 0x00 if ci == 0 else 0x10])
        if len(group) == 1:
            mcus = own_raster(group[0])
        else:
            mcus = [[(ci, my * samp[ci][1] + dy, mx * samp[ci][0] + dx)
                     for ci in group for dy in range(samp[ci][1]) for dx in range(samp[ci][0])]
                    for my in range(mcuy) for mx in range(mcux)]
        scan(sos + bytes([0, 0, 0]), mcus, put_dc)
    for ss, se in bands:
        for ci in range(len(samp)):
            t = 0 if ci == 0 else 1
            scan(bytes([1, ids[ci], t, ss, se, 0]), own_raster(ci),
                 lambda bw, ci, blk, pred, t=t, ss=ss, se=se: _put_band(bw, ac[t], blk, ss, se))
    return bytes(seg + b"\xff\xd9")


def _made(w, h, samp, seed, **kw):
    blocks, q = J.random_blocks(w, h, samp, seed)
    return write4p(w, h, samp, blocks, q, **kw)


# -- scans of a file -------------------------------------------------------------------------------------------
def scan_spans(data: bytes) -> list:
    """(start of the SOS marker, first byte of its entropy data, end of the entropy data) of every scan."""
    out, i = [], 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xD9:
            break
        ln = int.from_bytes(data[i + 2:i + 4], "big")
        if m != 0xDA:
            i += 2 + ln
            continue
        e = j = i + 2 + ln
        while not (data[j] == 0xFF and data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7):
            j += 1
        out.append((i, e, j))
        i = j
    return out


def cut_before_scan(data: bytes, j: int) -> bytes:
    """The file's first j scans, then EOI (whatever segments precede scan j + 1 are dropped with it)."""
    return data[:scan_spans(data)[j - 1][2]] + b"\xff\xd9"


def cut_mid_scan(data: bytes, j: int) -> bytes:
    """The file up to the middle of the entropy data of its scan j + 1 (not ending on FF); no EOI."""
    _, e, end = scan_spans(data)[j]
    k = e + (end - e) // 2
    while data[k - 1] == 0xFF:
        k -= 1
    assert k > e
    return data[:k]


def with_transform(data: bytes, transform: int) -> bytes:
    p = data.find(b"\xff\xee\x00\x0eAdobe")
    assert p >= 0
    return data[:p + 15] + bytes([transform]) + data[p + 16:]


def without_adobe(data: bytes) -> bytes:
    p = data.find(b"\xff\xee\x00\x0eAdobe")
    assert p >= 0
    return data[:p] + data[p + 16:]


# -- fixtures --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pillow_files() -> tuple:
    out = []
    for a, (w, h) in enumerate(PIL_SIZES):
        for ss in (0, 1, 2):
            qual = QUALITIES[(a + ss) % 3]  # (every subsampling meets every quality)
            out.append((f"pil-ss{ss}-q{qual}-{w}x{h}",
                        S.pillow_cmyk(w, h, 100 + 3 * a + ss, quality=qual, subsampling=ss, progressive=True)))
    out.append(("pil-rst-rows-50x37", S.pillow_cmyk(50, 37, 120, quality=85, subsampling=2, progressive=True,
                                                    restart_marker_rows=1)))
    out.append(("pil-rst-blocks-130x70", S.pillow_cmyk(130, 70, 121, quality=85, subsampling=0, progressive=True,
                                                       restart_marker_blocks=3)))
    return tuple((n, d, PROG, "ok") for n, d in out)


def _pil(name):
    return next(d for n, d, _, _ in pillow_files() if n == name)


CUT_SOURCES = ("pil-ss0-q30-50x37", "pil-ss2-q95-50x37")  # 4:4:4 and subsampling = 2
MID_SCANS = (2, 12)  # an AC first scan and a refinement scan


@functools.lru_cache(maxsize=None)
def ycck_files() -> tuple:
    out = [("ycck2-ss0-17x23", with_transform(_pil("pil-ss0-q95-17x23"), 2)),
           ("ycck2-ss1-50x37", with_transform(_pil("pil-ss1-q85-50x37"), 2)),
           ("ycck2-ss2-130x70", with_transform(_pil("pil-ss2-q30-130x70"), 2)),
           ("ycck1-ss2-50x37", with_transform(_pil("pil-ss2-q95-50x37"), 1)),
           ("no-adobe-ss1-17x23", without_adobe(_pil("pil-ss1-q30-17x23")))]
    return tuple((n, d, PROG, "ok") for n, d in out)


@functools.lru_cache(maxsize=None)
def writer_files() -> tuple:
    a0, a2 = S.adobe(0), S.adobe(2)
    out = [("w-photoshop-50x37", _made(50, 37, S.S_PHOTOSHOP, 201, lead=a2), PROG),
           ("w-photoshop-dc-each-5x9", _made(5, 9, S.S_PHOTOSHOP, 202, dc_groups=DC_EACH, lead=a2), PROG),
           ("w-ksub-dc-3-1-17x23", _made(17, 23, S_KSUB, 203, dc_groups=DC_3_1, lead=a0), PROG),
           ("w-ksub-50x37", _made(50, 37, S_KSUB, 204, lead=a2), PROG),
           ("w-ids-cmyk-no-adobe-17x23", _made(17, 23, S.S1, 205, ids=S.IDS_CMYK), PROG),
           ("w-ids-free-bands-50x37", _made(50, 37, S.S_H2, 206, ids=(9, 200, 3, 0), bands=((1, 5), (6, 63)), lead=a2), PROG),
           ("w-dri1-50x37", _made(50, 37, S.S1, 207, restart=1, lead=a0), PROG),
           ("w-dri3-first-17x23", _made(17, 23, S.S_FIRST, 208, restart=3, dc_groups=DC_3_1, lead=a0), PROG),
           ("w-dri3-photoshop-5x9", _made(5, 9, S.S_PHOTOSHOP, 209, restart=3, lead=a2), PROG),
           ("w-411-50x37", _made(50, 37, S.S_411, 210, lead=a0), PROG_EXT)]
    return tuple((n, d, fm, "ok") for n, d, fm in out)


@functools.lru_cache(maxsize=None)
def clean() -> tuple:
    """Every whole file the bit decodes: UNSUPPORTED without it, OK under the mask named with it."""
    return pillow_files() + ycck_files() + writer_files()


N_CLEAN = 17 + 5 + 10


@functools.lru_cache(maxsize=None)
def end_cuts() -> tuple:
    """The two cut sources ended before scan j + 1 with EOI, j = 1..17: PIL decodes all 34, smoothing the blocks."""
    out = []
    for src in CUT_SOURCES:
        data = _pil(src)
        assert len(scan_spans(data)) == 18, src
        out += [(f"{src}-first{j}", cut_before_scan(data, j), PROG, "ok") for j in range(1, 18)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mid_cuts_eoi() -> tuple:
    return tuple((f"{src}-mid{j}-eoi", cut_mid_scan(_pil(src), j) + b"\xff\xd9", PROG, "ok")
                 for src in CUT_SOURCES for j in MID_SCANS)


@functools.lru_cache(maxsize=None)
def mid_cuts() -> tuple:
    return tuple((f"{src}-mid{j}", cut_mid_scan(_pil(src), j), PROG, "err") for src in CUT_SOURCES for j in MID_SCANS)


@functools.lru_cache(maxsize=None)
def refused() -> tuple:
    """Refused under every mask, the full one included: sixteen blocks per MCU (SDSJ_CORRUPT), fractional ratios."""
    full = ("jpeg-cmyk-prog", "jpeg-ext", "jpeg-scans")
    return (("sixteen-blocks", _made(50, 37, ((2, 2),) * 4, 301, lead=S.adobe(0)), full, "err"),
            ("fractional", _made(50, 37, ((3, 1), (2, 1), (1, 1), (1, 1)), 302, lead=S.adobe(0)), full, "err"))


def fixtures() -> tuple:
    """Everything, for the host tests and the sanitizer driver."""
    return clean() + end_cuts() + mid_cuts_eoi() + mid_cuts() + refused()
