"""Multi-scan sequential JPEG files of the opt-in "jpeg-scans" subset (test input generator): SOF0 / SOF1 frames of
three components whose components arrive in more than one scan, and the cases that stay refused.

Pillow's encoder writes no such file, so they are written here from chosen quantised coefficients with the pieces of
tests/jpeg_ext_synth.py (its header writer, bit packer, symbol writers and random coefficients): write_multiscan
takes the scan grouping, the frame type, restart intervals, component ids, and marker segments / table
redefinitions between the scans.  A single-component scan codes that component's own ceil(dw / 8) x ceil(dh / 8)
block raster (jdinput.c per_scan_setup), an interleaved one the frame's MCUs.  The reference of every file is PIL
itself (jpeg_ext_synth.pil_rgb); for every clean fixture the same coefficients written as one interleaved scan
(jpeg_ext_synth.write_baseline) must give the same pixels as well."""
from __future__ import annotations

import functools

from tests import jpeg_ext_synth as J
from tests.golden import coefjpeg as C

SETS = {"444": ((1, 1), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "420": ((2, 2), (1, 1), (1, 1)),
        "411": J.SETS["411"]}  # (4:1:1 needs "jpeg-ext" as well)
SIZES = [(1, 1), (5, 9), (50, 37), (33, 70)]  # (width, height)
BIG = (320, 240)
GROUPS = {"y-cb-cr": ((0,), (1,), (2,)), "y-cbcr": ((0,), (1, 2)), "cr-y-cb": ((2,), (0,), (1,)),
          "ycb-cr": ((0, 1), (2,))}
SCANS, SCANS_EXT = ("jpeg", "jpeg-scans"), ("jpeg", "jpeg-scans", "jpeg-ext")


def dqt(tq: int, q) -> bytes:
    seg = bytearray()
    J._marker(seg, 0xDB, bytes([tq]) + bytes(int(v) for v in q))
    return bytes(seg)


def dri(restart: int) -> bytes:
    seg = bytearray()
    J._marker(seg, 0xDD, restart.to_bytes(2, "big"))
    return bytes(seg)


def dht(tc: int, th: int, bits, vals) -> bytes:
    seg = bytearray()
    J._marker(seg, 0xC4, bytes([(tc << 4) | th] + list(bits) + list(vals)))
    return bytes(seg)


def write_multiscan(w, h, samp, blocks, q, groups, sof=0xC0, restart=0, ids=(1, 2, 3), between=None, huff=None,
                    scan_params=None) -> bytes:
    """groups: per scan the frame indices of its components, in scan order.  sof: 0xC0 or 0xC1.  restart: the restart
    interval in MCUs of the scan (a single-component scan's MCU is one block), or one value per scan -- a DRI segment
    goes before every scan whose value differs from the one in force.  between: {scan index: marker segments written
    before that scan's SOS}.  huff: {scan index: {(tc, th): (bits, vals)}} -- tables redefined by a DHT before that
    scan and used from there on.  scan_params: {scan index: (Ss, Se, Ah << 4 | Al)} instead of (0, 63, 0)."""
    tabs, _, _ = J._tables()
    tabs = dict(tabs)
    hmax, vmax, mcux, mcuy = J._geometry(w, h, samp)
    ris = [restart] * len(groups) if isinstance(restart, int) else list(restart)
    seg = J._head(w, h, samp, q, sof, ids, b"", ris[0])
    in_force = ris[0]
    for k, group in enumerate(groups):
        seg += (between or {}).get(k, b"")
        for (tc, th), (bits, vals) in (huff or {}).get(k, {}).items():
            tabs[(tc, th)] = (bits, vals)
            seg += dht(tc, th, bits, vals)
        if ris[k] != in_force:
            seg += dri(ris[k])
            in_force = ris[k]
        dc = [C._codes(*tabs[(0, t)]) for t in range(2)]
        ac = [C._codes(*tabs[(1, t)]) for t in range(2)]
        sos = bytes([len(group)])
        for ci in group:
            sos += bytes([ids[ci], 0x00 if ci == 0 else 0x11])
        J._marker(seg, 0xDA, sos + bytes((scan_params or {}).get(k, (0, 63, 0))))
        # the scan's MCUs: each a list of (component, block row, block column)
        if len(group) == 1:
            ci = group[0]
            dw, dh = -(-w * samp[ci][0] // hmax), -(-h * samp[ci][1] // vmax)
            mcus = [[(ci, y, x)] for y in range(-(-dh // 8)) for x in range(-(-dw // 8))]
        else:
            mcus = [[(ci, my * samp[ci][1] + dy, mx * samp[ci][0] + dx)
                     for ci in group for dy in range(samp[ci][1]) for dx in range(samp[ci][0])]
                    for my in range(mcuy) for mx in range(mcux)]
        bw = J._Bits()
        pred = [0, 0, 0]
        for m, mcu in enumerate(mcus):
            if ris[k] and m and m % ris[k] == 0:
                bw.flush()
                bw.out.extend(bytes([0xFF, 0xD0 + (m // ris[k] - 1) % 8]))
                pred = [0, 0, 0]
            for ci, y, x in mcu:
                t = 0 if ci == 0 else 1
                blk = blocks[ci][y, x]
                J._put_dc(bw, dc[t], int(blk[0]) - pred[ci])
                pred[ci] = int(blk[0])
                J._put_ac(bw, ac[t], blk)
        bw.flush()
        seg += bw.out
    return bytes(seg + b"\xff\xd9")


def make(set_name, w, h, groups, seed=0, **kw):
    """(the multi-scan file, the same coefficients as one interleaved scan)"""
    samp = SETS[set_name]
    blocks, q = J.random_blocks(w, h, samp, seed)
    g = GROUPS[groups] if isinstance(groups, str) else groups
    single = J.write_baseline(w, h, samp, blocks, q, ids=kw.get("ids", (1, 2, 3)))
    return write_multiscan(w, h, samp, blocks, q, g, **kw), single


@functools.lru_cache(maxsize=None)
def clean() -> tuple:
    """(name, bytes, gpu_formats that admit it, the one-scan file of the same coefficients or None)."""
    out = []
    gnames = list(GROUPS)

    def add(set_name, w, h, gi, sof, ri, formats=SCANS, **kw):
        g = gnames[gi % 4]
        data, single = make(set_name, w, h, g, seed=len(out) + 1, sof=sof, restart=ri, **kw)
        name = f"{set_name}-{w}x{h}-{g}-sof{sof & 1}-dri{ri}" + ("-rgb" if "ids" in kw else "")
        out.append((name, data, formats, single))

    k = 0
    for set_name in ("444", "422", "420"):  # every set at every size, groupings / frame types / intervals in turn
        for (w, h) in SIZES:
            add(set_name, w, h, k, 0xC0 + (k & 1), 3 * ((k >> 1) & 1))
            k += 1
    for (w, h) in ((5, 9), (50, 37)):  # 4:2:0, where the Y scan's raster is smaller than the MCU-padded grid
        for gi in range(4):
            add("420", w, h, gi, 0xC1 - (gi & 1), 3 * (gi & 1) if (w, h) == (5, 9) else 3 * (1 - (gi & 1)))
    add("420", *BIG, 0, 0xC0, 0)  # the long scans
    add("422", *BIG, 1, 0xC1, 3)
    add("411", 50, 37, 0, 0xC0, 0, SCANS_EXT)  # both bits
    add("411", 33, 70, 3, 0xC1, 3, SCANS_EXT)
    add("444", 50, 37, 1, 0xC0, 0, SCANS_EXT, ids=(82, 71, 66))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def table_changes() -> tuple:
    """Tables redefined between the scans (name, bytes, formats, None): a DQT that redefines table 1 between the Cb
    and the Cr scan (the Cr plane dequantises with the new one: latch_quant_tables), a DHT that redefines AC table 1
    there (the Cr scan is coded with it), a restart interval that changes from scan to scan."""
    samp = SETS["420"]
    blocks, q = J.random_blocks(50, 37, samp, 77)
    g = GROUPS["y-cb-cr"]
    q2 = [min(255, int(v) * 3 + 1) for v in q[1]]
    tabs, _, _ = J._tables()
    return (("dqt-between", write_multiscan(50, 37, samp, blocks, q, g, between={2: dqt(1, q2)}), SCANS, None),
            ("dht-between", write_multiscan(50, 37, samp, blocks, q, g, huff={2: {(1, 1): tabs[(1, 0)]}}), SCANS, None),
            ("dri-between", write_multiscan(50, 37, samp, blocks, q, g, restart=(0, 2, 5)), SCANS, None))


@functools.lru_cache(maxsize=None)
def plain_of_table_changes() -> bytes:
    """The coefficients of table_changes() as one interleaved scan (the DHT and DRI files' pixels; not the DQT file's)."""
    samp = SETS["420"]
    blocks, q = J.random_blocks(50, 37, samp, 77)
    return J.write_baseline(50, 37, samp, blocks, q)


@functools.lru_cache(maxsize=None)
def early_eoi() -> tuple:
    """EOI after two of three scans: the Cr plane decodes from zero coefficients."""
    samp = SETS["420"]
    blocks, q = J.random_blocks(50, 37, samp, 78)
    return (("eoi-after-two", write_multiscan(50, 37, samp, blocks, q, ((0,), (1,))), SCANS, None),)


@functools.lru_cache(maxsize=None)
def fixtures() -> tuple:
    """Every file the bit decodes: UNSUPPORTED without it, OK under the mask named with it."""
    return clean() + table_changes() + early_eoi()


def _stuffed_file():
    """A file without restart intervals whose entropy data holds a stuffed zero (FF 00), and that pair's position."""
    for seed in range(40):
        data, _ = make("420", 50, 37, "y-cb-cr", seed=200 + seed)
        p = data.find(b"\xff\x00", data.index(b"\xff\xda"))
        if p > 0:
            return data, p
    raise AssertionError("no stuffed zero in 40 files")


@functools.lru_cache(maxsize=None)
def refused() -> tuple:
    """Non-OK under every mask: scan parameters that are not sequential ones (in the first scan, in a later one), a
    component scanned twice, and fill bytes before a stuffed zero in a scan without restart intervals."""
    samp = SETS["420"]
    blocks, q = J.random_blocks(50, 37, samp, 79)
    g = GROUPS["y-cb-cr"]
    data, p = _stuffed_file()
    return (("not-sequential-first", write_multiscan(50, 37, samp, blocks, q, g, scan_params={0: (0, 62, 0)})),
            ("not-sequential-later", write_multiscan(50, 37, samp, blocks, q, g, scan_params={2: (0, 63, 1)})),
            ("component-twice", write_multiscan(50, 37, samp, blocks, q, ((0,), (1,), (1,), (2,)))),
            ("fill-stuffed", data[:p] + b"\xff" + data[p:]))


@functools.lru_cache(maxsize=None)
def damaged() -> tuple:
    """The last scan cut in half (PIL raises OSError), the same with EOI appended (PIL decodes it), and a flipped byte
    in the first scan whose neighbours are not FF (no marker appears)."""
    whole, _ = make("420", 50, 37, "y-cb-cr", seed=90)
    last = whole.rindex(b"\xff\xda")
    cut = whole[:len(whole) - (len(whole) - last) // 2]
    if cut[-1] == 0xFF:
        cut = cut[:-1]
    b = bytearray(whole)
    p = whole.index(b"\xff\xda") + 10 + 40
    while 0xFF in (b[p - 1], b[p], b[p + 1]) or b[p] ^ 0x5A == 0xFF:
        p += 1
    b[p] ^= 0x5A
    return (("truncated-scan", cut), ("truncated-scan-eoi", cut + b"\xff\xd9"), ("flipped-byte", bytes(b)))
