"""The entropy / unstuff plan case table (test infrastructure; tests/test_entropy_cases_table.py proves on
the CPU that every case has the plan it is meant to have, tests/test_gpu_entropy_routes.py runs the cases on
the GPU, stage by stage against the oracle).

A *situation* is one edge of the front half of the pipeline (k_us_*, k_scanmap, k_entspec, k_entsync,
k_entwrite, the multi-hypothesis pass): a mode and the conditions an image's plan must meet there.  A *case* is
a named, deterministic JPEG and the situations it pins.  The modes: "alone", a host chunk of at most kSmallBatch
images (the latency plan: ImgDesc::lat), and "batch", inside a chunk of 40 images (the throughput plan).

Every threshold is one of the project's constants, read by name from sds_amd/csrc (``const``): none is
typed in here.  Conditions are (field, operator, value) triples over
  * the plan fields tests/asan/plan_driver.cpp prints (test_plan_host.ENT_FIELDS) and the route names,
  * what the restated unstuffing gives (test_entropy_cases_table.unstuff): nsub, first_at (the subsequence
    indices at which a restart segment begins), blocks_per_sub, bits_over_sub (ceil(unstuffed bits / sub_bits)),
  * run-time statistics only the device has (RUNTIME: sync_rounds, pad0), checked by the GPU test.
A value that is a string names another field or, for the "in" operator's left side, a set-valued field.

The sync-pressure situation -- more sync tasks in one round than max_tasks<kSyncThreads>() takes, "the rest are
picked up by the next round" -- is an inference, not a reading.  The device records only the number of rounds
and the task total over all rounds (pad0), and pad0 above the cap with two rounds or more does not show that any
single round passed it.  What makes it likely is the case's construction: the three components of a 4:4:4 scan
share one Huffman table pair, so nothing in the stream tells the MCU phase, the phase a subsequence guesses is
right for one in three, and about two thirds of the more than 257 entries disagree with their predecessor's
exit in the first round.  tools/sync_sim.c models neither the cap nor the device's warm-up and is not used as a
proof."""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass
from typing import Callable

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sds_amd", "csrc")
RUNTIME = ("sync_rounds", "pad0")
BATCH = 40  # the chunk a "batch" case runs in: more than kSmallBatch


@functools.lru_cache(maxsize=None)
def const(name: str, header: str = "sdsj_common.h") -> int:
    """A ``constexpr int`` (or the ``#define`` it takes its value from) of a source file, by name."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr int %s = ([A-Za-z_0-9]+);" % name, text) or re.search(r"#define %s (\w+)" % name, text)
    assert m, name
    return int(m.group(1)) if m.group(1).isdigit() else const(m.group(1), header)


def group_bytes(lat: bool) -> int:
    """Scan bytes one entropy workgroup takes before plan_image adds another: kDecodeThreads subsequences of
    kGroupBits (throughput plan: 262,144 bytes) or kLatSubBits (latency plan: 32,768 bytes)."""
    return const("kDecodeThreads") * const("kLatSubBits" if lat else "kGroupBits") // 8


def max_sync_tasks() -> int:
    """max_tasks<kSyncThreads>() of sdsj_entropy.hip: 4 x NT sync tasks per round."""
    text = open(os.path.join(CSRC, "sdsj_entropy.hip")).read()
    assert re.search(r"constexpr int max_tasks\(\) \{ return 4 \* NT; \}", text)
    return 4 * const("kSyncThreads", "sdsj_entropy.hip")


# -- situations --------------------------------------------------------------------------------------------
def _group_situations() -> dict:
    s = {}
    for lat, mode, tag, sub in ((False, "batch", "thr", "kGroupBits"), (True, "alone", "lat", "kLatSubBits")):
        gb, cap = group_bytes(lat), const("kMaxEntGroups")
        many = "kRtEnt11M"
        for rst, rtag in (((("nseg", ">", 1),), "rst"), ((("nseg", "==", 1),), "norst")):
            # one group and two on either side of kDecodeThreads x sub bits, within a tenth of it
            s[f"{tag}_g1_{rtag}"] = (mode, rst + (("ent_groups", "==", 1), ("entropy_len", ">", gb * 9 // 10),
                                                   ("ent", "==", "kRtEnt11")))
            s[f"{tag}_g2_{rtag}"] = (mode, rst + (("ent_groups", "==", 2), ("entropy_len", "<", gb * 11 // 10),
                                                   ("ent", "==", many)))
            # a group count that does not divide the subsequences: the last group's share is short
            s[f"{tag}_gmid_{rtag}"] = (mode, rst + (("ent_groups", ">=", 3), ("ent_groups", "<", cap),
                                                     ("nsub", "%!=0", "ent_groups"), ("ent", "==", many)))
            # the kMaxEntGroups cap: sub_bits grows instead
            s[f"{tag}_cap_{rtag}"] = (mode, rst + (("ent_groups", "==", cap), ("entropy_len", ">", cap * gb),
                                                    ("sub_bits", ">", const(sub)), ("ent", "==", many)))
    return s


SITUATIONS: dict[str, tuple] = {
    **_group_situations(),
    # groups planned from the raw scan length, subsequences laid over the unstuffed one
    "empty_share_batch": ("batch", (("entropy_len", ">", 2 * group_bytes(False)), ("nsub", "<", "ent_groups"))),
    "empty_share_alone": ("alone", (("nsub", "<", "ent_groups"),)),
    # more sync tasks than one round takes (max_tasks<kSyncThreads>()): see the module docstring on what is inferred
    "sync_pressure": ("batch", (("ent_groups", ">=", 2), ("entropy_len", ">", group_bytes(False)), ("nsub", ">", 257),
                                ("sync_rounds", ">=", 2), ("pad0", ">", max_sync_tasks()))),
    "sync_control_batch": ("batch", (("ent_groups", "==", 1), ("entropy_len", "<", group_bytes(True)))),
    "sync_control_alone": ("alone", (("ent_groups", "==", 1), ("entropy_len", "<", group_bytes(True)), ("mh", "==", 1))),
    "sync_pressure_mh": ("alone", (("mh", "==", 1), ("ent_groups", ">=", 2))),
    # the segmented scan's 64-wide chunks (kSyncThreads): a restart segment beginning at 63, 64, 65
    **{f"seg_first_{i}": ("batch", ((i, "in", "first_at"), (i - 1, "notin", "first_at"), ("nsub", ">", i + 1)))
       for i in (const("kSyncThreads", "sdsj_entropy.hip") + k for k in (-1, 0, 1))},
    "nseg_over_256": ("batch", (("nseg", ">", const("kDecodeThreads")), ("bits_over_sub", "<", "nseg"),
                                ("nsub", "==", "nseg"))),
    # records: far more block boundaries in a subsequence than kRecStore, and fewer than two
    "rec_many": ("batch", (("blocks_per_sub", ">", 4 * const("SDSJ_REC_STORE", "sdsj_entropy.hip")),
                           ("nsub", ">=", 2), ("sync_rounds", ">=", 1))),
    "rec_few": ("batch", (("sub_bits", "==", const("kMinSubBits")), ("blocks_per_sub", "<", 2), ("nsub", ">=", 2),
                          ("sync_rounds", ">=", 1))),
    # table slots x mode
    "ent10_multi_group": ("alone", (("ent", "==", "kRtEnt10"), ("ent_groups", ">=", 2), ("nseg", "==", 1))),
    "ent10_multi_group_batch": ("batch", (("ent", "==", "kRtEnt10"), ("ent_groups", ">=", 2), ("nseg", "==", 1))),
    "ent10_restart": ("batch", (("ent", "==", "kRtEnt10"), ("nseg", ">", 1))),
    "ent10_restart_alone": ("alone", (("ent", "==", "kRtEnt10"), ("nseg", ">", 1), ("mh", "==", 0))),
    "mh_on": ("alone", (("mh", "==", 1), ("nseg", "==", 1), ("nsub", ">=", 2))),
    "mh_off_restart": ("alone", (("mh", "==", 0), ("nseg", ">", 1), ("ent", "!=", "kRtEnt10"))),
    # unstuff: FF|00, FF|Dn, FF FF|Dn on a 32-byte thread boundary and an 8 KiB tile boundary of the scan
    "straddle_serial": ("batch", (("ntiles", "<=", const("kUsSerialTiles")), ("ntiles", ">=", 3), ("us", "==", "kRtUsSmall"))),
    "straddle_serial_size_tile_parallel": ("alone", (("ntiles", "<=", const("kUsSerialTiles")), ("us", "==", "kRtUsBig"))),
    "straddle_tile_parallel": ("batch", (("ntiles", ">", const("kUsSerialTiles")), ("us", "==", "kRtUsBig"))),
    "tiles_64": ("batch", (("ntiles", "==", const("kUsSerialTiles")), ("us", "==", "kRtUsSmall"),
                           ("entropy_len", "==", const("kUsSerialTiles") * const("kUsTileBytes")))),
    "tiles_65": ("batch", (("ntiles", "==", const("kUsSerialTiles") + 1), ("us", "==", "kRtUsBig"),
                           ("entropy_len", "==", const("kUsSerialTiles") * const("kUsTileBytes") + 1))),
    # the scan's start at every residue mod 16 (k_us_serial's realigned 16-byte loads)
    **{f"entropy_off_mod16_{r}": ("batch", (("entropy_off_mod16", "==", r), ("us", "==", "kRtUsSmall"))) for r in range(16)},
}

# Pinned next to an existing pixel check instead of a case of this table: the warm-up a lane gets
# (k_parse: kWarmBits for a lane of at least kWarmSmallLane images -- what the benchmark runs -- and
# kWarmBitsSmall below it).  {situation: (test file, test, the text of its descriptor assertion)}
REFERENCED = {
    "warm_bits_large_lane": ("tests/test_gpu_lanes.py", "test_lanes_equal_one_lane_and_oracle", 'r.ent["warm_bits"]'),
    "warm_bits_small_lane": ("tests/test_gpu_lanes.py", "test_lanes_equal_one_lane_and_oracle", 'r.ent["warm_small"]'),
}


OPS = {"==": lambda a, b: a == b, "!=": lambda a, b: a != b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b,
       "<": lambda a, b: a < b, "<=": lambda a, b: a <= b, "%!=0": lambda a, b: a % b != 0,
       "in": lambda a, b: a in b, "notin": lambda a, b: a not in b}


def check(props: dict, conds, runtime: bool, what: str = "") -> None:
    """Asserts the conditions over props; those on RUNTIME fields only when runtime (the GPU test)."""
    for f, op, v in conds:
        if (f in RUNTIME) != runtime:
            continue
        a = props[f] if isinstance(f, str) else f
        b = props[v] if isinstance(v, str) and v in props else v
        assert OPS[op](a, b), f"{what}: {f} ({a}) {op} {v} ({b if b is not v else ''}) does not hold"


# -- byte-level helpers --------------------------------------------------------------------------------------
def entropy_off(jpg: bytes) -> int:
    """The first byte after the first SOS segment (ImgDesc::entropy_off)."""
    i = 2
    while True:
        assert jpg[i] == 0xFF, i
        m, ln = jpg[i + 1], (jpg[i + 2] << 8) | jpg[i + 3]
        if m == 0xDA:
            return i + 2 + ln
        i += 2 + ln


def _next_rst(scan, pos: int) -> int:
    """Index of the FF of the first RSTn marker at or after pos."""
    while True:
        i = scan.find(b"\xff", pos)
        assert i >= 0 and i + 1 < len(scan), "no restart marker left"
        if 0xD0 <= scan[i + 1] <= 0xD7:
            return i
        pos = i + 2 if scan[i + 1] == 0 else i + 1


def rst_positions(jpg: bytes) -> list[int]:
    """File offsets of the FF of every RSTn marker in the scan."""
    off = entropy_off(jpg)
    scan, out, pos = jpg[off:], [], 0
    while True:
        i = scan.find(b"\xff", pos)
        if i < 0 or i + 1 >= len(scan):
            return out
        if 0xD0 <= scan[i + 1] <= 0xD7:
            out.append(off + i)
        elif scan[i + 1] not in (0, 0xFF):
            return out
        pos = i + 2 if scan[i + 1] != 0xFF else i + 1


def pad_restarts(jpg: bytes, fills: dict[int, int]) -> bytes:
    """The file with fills[k] fill bytes (FF) put in front of its k-th RSTn marker (ISO 10918-1 B.1.1.2: any
    marker may be preceded by fill bytes)."""
    pos = rst_positions(jpg)
    out, last = bytearray(), 0
    for k in sorted(fills):
        out += jpg[last:pos[k]] + b"\xff" * fills[k]
        last = pos[k]
    return bytes(out + jpg[last:])


def with_comment(jpg: bytes, extra: int) -> bytes:
    """The file with a COM segment of `extra` payload bytes after SOI: the scan starts 4 + extra bytes later."""
    return jpg[:2] + b"\xff\xfe" + (2 + extra).to_bytes(2, "big") + bytes(range(65, 65 + extra)) + jpg[2:]


STRADDLES = (("ff00", 32), ("rst", 32), ("fill_rst", 32), ("ff00", 8192), ("rst", 8192), ("fill_rst", 8192))


def straddle(jpg: bytes) -> tuple[bytes, tuple]:
    """Steers, with fill bytes in front of earlier RSTn markers, one FF|00, one FF|Dn and one FF FF|Dn of a
    restart-interval file so that the '|' falls on a multiple of 32 that is no multiple of 8192, and one of
    each on a multiple of 8192, counted from the scan's first byte.  Returns the file and ((kind, modulus,
    scan offset of the byte after the '|'), ...)."""
    assert const("kUsTileBytes") == 8192 and const("kUsTileBytes") // const("SDSJ_DECODE_THREADS") == 32
    off = entropy_off(jpg)
    scan, pos, found = bytearray(jpg[off:]), 0, []
    for kind, mod in STRADDLES:
        r1 = _next_rst(scan, pos)  # the marker that takes the fill bytes
        if kind == "ff00":
            x = scan.find(b"\xff\x00", r1 + 2) + 1
            assert x > 0
        else:
            t = _next_rst(scan, r1 + 2)
            if kind == "fill_rst":
                scan[t:t] = b"\xff"
                t += 1
            x = t + 1
        k = -x % mod
        if mod == 32 and (x + k) % 8192 == 0:
            k += 32
        scan[r1:r1] = b"\xff" * k
        found.append((kind, mod, x + k))
        pos = x + k + 1
    return jpg[:off] + bytes(scan), tuple(found)


# -- image builders (fixed seeds only) -------------------------------------------------------------------------
def noise(w: int, h: int, quality: int, samp: str, rst: int, seed: int, gray: bool = False) -> bytes:
    """PIL-encoded uniform noise; rst: MCUs per restart interval (0: none)."""
    from tests.golden.synth import encode_jpeg
    rng = np.random.default_rng(seed)
    kw = {"restart_marker_blocks": rst} if rst else {}
    if gray:
        return encode_jpeg(rng.integers(0, 256, (h, w), dtype=np.uint8), quality, **kw)
    return encode_jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality,
                       subsampling={"444": 0, "422": 1, "420": 2}[samp], **kw)


def varied(w: int, h: int, seed: int) -> bytes:
    """4:2:0 noise at quality 95 whose amplitude is drawn per 16 x 16 MCU, a restart interval of one MCU: the
    restart segments take one to three subsequences of kMinSubBits."""
    from tests.golden.synth import encode_jpeg
    rng = np.random.default_rng(seed)
    amp = np.kron(rng.random((-(-h // 16), -(-w // 16))), np.ones((16, 16)))[:h, :w, None]
    rgb = 128 + (rng.integers(0, 256, (h, w, 3)) - 128) * amp
    return encode_jpeg(rgb.astype(np.uint8), 95, subsampling=2, restart_marker_blocks=1)


def flat(w: int, h: int, rst: int, seed: int) -> bytes:
    """A nearly flat 4:2:0 image (blocks of a few bits each) with one pixel in 600 set apart, so that the
    stream is not periodic."""
    from tests.golden.synth import encode_jpeg
    rng = np.random.default_rng(seed)
    rgb = np.full((h, w, 3), 128, np.uint8)
    rgb[rng.random((h, w)) < 1 / 600] = (250, 30, 60)
    return encode_jpeg(rgb, 90, subsampling=2, **({"restart_marker_blocks": rst} if rst else {}))


S420 = [(2, 2, 0), (1, 1, 1), (1, 1, 1)]
S444 = [(1, 1, 0), (1, 1, 1), (1, 1, 1)]


def coef_blocks(seed: int, w: int, h: int, comps, nnz: int, amp: int):
    """Per component [bh, bw, 64] quantised coefficients (zigzag): about nnz AC terms in [-amp, amp] per
    block and a DC random walk."""
    rng = np.random.default_rng(seed)
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    blocks = []
    for hs, vs, _ in comps:
        bh, bw = mcuy * vs, mcux * hs
        b = np.zeros((bh, bw, 64), np.int64)
        b[..., 1:] = rng.integers(-amp, amp + 1, (bh, bw, 63)) * (rng.random((bh, bw, 63)) < nnz / 63)
        b[..., 0] = np.clip(np.cumsum(rng.integers(-40, 41, bh * bw)), -900, 900).reshape(bh, bw)
        blocks.append(b)
    return blocks


Q = {0: np.arange(2, 66), 1: np.arange(3, 67)}


def coef_jpeg(seed: int, w: int, h: int, comps, nnz: int, amp: int, huff, rst_rows: int = 0) -> bytes:
    """tests.golden.coefjpeg.write_jpeg of coef_blocks, with the chosen Huffman table ids.  rst_rows > 0: the
    same coefficients with a restart interval of rst_rows MCU rows -- each interval written as a scan of its
    own (the DC predictors start at zero and the last byte is padded with ones, as after RSTn) and joined
    with DRI / RSTn."""
    from tests.golden.coefjpeg import write_jpeg
    blocks = coef_blocks(seed, w, h, comps, nnz, amp)
    if not rst_rows:
        return write_jpeg(w, h, comps, blocks, Q, huff=huff)
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    head, scans = None, []
    for r0 in range(0, mcuy, rst_rows):
        r1 = min(r0 + rst_rows, mcuy)
        part = write_jpeg(w, (r1 - r0) * 8 * vmax, comps, [b[r0 * vs:r1 * vs] for b, (_, vs, _) in zip(blocks, comps)], Q,
                          huff=huff)
        off = entropy_off(part)
        if head is None:
            head = bytearray(part[:off])
        scans.append(part[off:-2])
    sof = head.index(b"\xff\xc0")
    head[sof + 5:sof + 7] = h.to_bytes(2, "big")
    sos = head.index(b"\xff\xda")
    head[sos:sos] = b"\xff\xdd\x00\x04" + (mcux * rst_rows).to_bytes(2, "big")
    body = b"".join(s + (bytes([0xFF, 0xD0 + k % 8]) if k + 1 < len(scans) else b"") for k, s in enumerate(scans))
    return bytes(head) + body + b"\xff\xd9"


def flat_coef(seed: int, w: int, h: int) -> bytes:
    """A flat 4:2:0 image written from coefficients, one table pair for all components: no AC term, and the DC
    of one block in 40 steps, so a block costs 6 bits (DC difference 0, end of block) -- about 170 block
    boundaries in a subsequence of kMinSubBits -- and nothing in the stream tells the MCU phase, while a phase
    taken wrong gives the steps to the wrong component."""
    from tests.golden.coefjpeg import write_jpeg
    rng = np.random.default_rng(seed)
    mcux, mcuy = -(-w // 16), -(-h // 16)
    blocks = []
    for hs, vs, _ in S420:
        b = np.zeros((mcuy * vs, mcux * hs, 64), np.int64)
        n = b.shape[0] * b.shape[1]
        b[..., 0] = np.cumsum(rng.integers(-20, 21, n) * (rng.random(n) < 1 / 40)).reshape(b.shape[:2])
        blocks.append(b)
    return write_jpeg(w, h, S420, blocks, Q, huff=[(0, 0), (0, 0), (0, 0)])


def fill_to(jpg: bytes, entropy_len: int, k: int = 5) -> bytes:
    """The restart-interval file with fill bytes in front of its k-th RSTn so that entropy_len (the bytes
    from the scan's first to the file's last) is the given one."""
    have = len(jpg) - entropy_off(jpg)
    assert have <= entropy_len
    return pad_restarts(jpg, {k: entropy_len - have})


# -- the table -------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    build: Callable[[], bytes]
    pins: tuple                 # situations (keys of SITUATIONS); a case runs in every mode one of them names
    big: bool = False           # may exceed 1 MP: no full-resolution output, coefficient blocks checked on a sample
    truncate: bool = False      # also run as a copy cut at 2/3 of the file
    group: str = ""             # "straddle": build returns (bytes, offsets); "padded": has an unpadded twin
    twin: Callable[[], bytes] | None = None   # the file PIL must decode to the same pixels

    @property
    def modes(self) -> tuple:
        return tuple(m for m in ("alone", "batch") if any(SITUATIONS[s][0] == m for s in self.pins))


_cache: dict = {}


def case_image(c: Case) -> bytes:
    """The case's JPEG, built once per process."""
    if c.name not in _cache:
        r = c.build()
        _cache[c.name] = r if isinstance(r, tuple) else (r, ())
    return _cache[c.name][0]


def case_offsets(c: Case) -> tuple:
    case_image(c)
    return _cache[c.name][1]


# Noise at quality 100, 4:4:4, costs 4.11 scan bytes a pixel: the sizes below put the scan just under / over
# kDecodeThreads x kLatSubBits / 8 = 32,768 bytes (88 x 88, 96 x 88), kDecodeThreads x kGroupBits / 8 = 262,144
# (248 x 256, 256 x 256), between 2 and 3 times that and over kMaxEntGroups x 32,768 (400 x 368), and over
# kMaxEntGroups x 262,144 (1024 x 1000: the smallest multiple-of-8 size that clears it with restart markers or
# without).  The restart interval of 7 MCUs leaves segments of about 1.3 KB.
_SIZES = {"a": (88, 88), "b": (96, 88), "c": (248, 256), "d": (256, 256), "e": (400, 368), "f": (1024, 1000)}
_NOISE_PINS = {
    "a": ("lat_g1",), "b": ("lat_g2",), "c": ("thr_g1", "lat_gmid"), "d": ("thr_g2",),
    "e": ("thr_gmid", "lat_cap"), "f": ("thr_cap",),
}


def _noise_case(key: str, rst: int) -> Case:
    w, h = _SIZES[key]
    tag = "rst" if rst else "norst"
    pins = tuple(f"{p}_{tag}" for p in _NOISE_PINS[key])
    return Case(f"noise_{key}_{w}x{h}_{tag}", lambda: noise(w, h, 100, "444", rst, 100 + ord(key)), pins,
                big=key == "f", truncate=(key, rst) == ("d", 7))


def _padded_420() -> bytes:
    return noise(32, 32, 90, "420", 1, 7)


def _sync_pressure(w: int, h: int) -> bytes:
    return coef_jpeg(11, w, h, S444, 40, 127, [(0, 0), (0, 0), (0, 0)])


SEG_SEEDS = {63: 1, 64: 3, 65: 5}  # seg_first_<index>: the seed of `varied`


def _table() -> list[Case]:
    t = [_noise_case(k, rst) for k in _SIZES for rst in (0, 7)]
    # 4 MCUs, a restart interval of one: 4 segments of a few dozen bytes; 350,000 fill bytes in front of each of
    # the 3 RSTn put the raw scan over 4 x 262,144 bytes: 5 groups (16 in latency mode) for 4 subsequences
    t.append(Case("empty_share_420", lambda: pad_restarts(_padded_420(), {0: 350000, 1: 350000, 2: 350000}),
                  ("empty_share_batch", "empty_share_alone"), truncate=True, group="padded", twin=_padded_420))
    # one table pair for all three components of a 4:4:4 scan: about 520 bits a block, 296 x 296 = 4,107 blocks
    t.append(Case("sync_pressure_444", lambda: _sync_pressure(296, 296), ("sync_pressure", "sync_pressure_mh"),
                  truncate=True))
    t.append(Case("sync_control_444", lambda: _sync_pressure(88, 80), ("sync_control_batch", "sync_control_alone")))
    # restart segments of one to three subsequences (`varied`, sub_bits = kMinSubBits): the first seeds of 1, 2, ..
    # with a segment that begins at the index and none at the index before it
    for idx, seed in SEG_SEEDS.items():
        t.append(Case(f"seg_first_{idx}", functools.partial(varied, 128, 128, seed), (f"seg_first_{idx}",)))
    t.append(Case("nseg_289", lambda: flat(272, 272, 1, 3), ("nseg_over_256",)))
    t.append(Case("rec_many_flat", lambda: flat_coef(5, 384, 384), ("rec_many",)))
    t.append(Case("rec_few_q100", lambda: noise(48, 48, 100, "444", 0, 9), ("rec_few",)))
    six = [(0, 0), (1, 1), (2, 2)]
    t.append(Case("six_slot_multi", lambda: coef_jpeg(21, 160, 160, S420, 30, 100, six), ("ent10_multi_group",)))
    t.append(Case("six_slot_multi_batch", lambda: coef_jpeg(22, 336, 336, S444, 30, 100, six), ("ent10_multi_group_batch",)))
    t.append(Case("six_slot_restart", lambda: coef_jpeg(21, 160, 160, S420, 30, 100, six, rst_rows=1),
                  ("ent10_restart", "ent10_restart_alone"), group="same_coef",
                  twin=lambda: coef_jpeg(21, 160, 160, S420, 30, 100, six)))
    t.append(Case("mh_on_420", lambda: coef_jpeg(31, 96, 80, S420, 12, 40, None), ("mh_on",)))
    t.append(Case("mh_off_420_restart", lambda: coef_jpeg(31, 96, 80, S420, 12, 40, None, rst_rows=1), ("mh_off_restart",),
                  group="same_coef", twin=lambda: coef_jpeg(31, 96, 80, S420, 12, 40, None)))
    t.append(Case("straddle_5_tiles", lambda: straddle(noise(96, 88, 100, "444", 7, 41)),
                  ("straddle_serial", "straddle_serial_size_tile_parallel"), group="straddle"))
    t.append(Case("straddle_over_64_tiles", lambda: straddle(noise(400, 360, 100, "444", 7, 42)),
                  ("straddle_tile_parallel",), group="straddle", truncate=False))
    full = const("kUsSerialTiles") * const("kUsTileBytes")
    t.append(Case("tiles_64_full", lambda: fill_to(noise(352, 352, 100, "444", 7, 43), full), ("tiles_64",)))
    t.append(Case("tiles_65_one_byte", lambda: fill_to(noise(352, 352, 100, "444", 7, 43), full + 1), ("tiles_65",)))
    for r in range(16):
        t.append(Case(f"entropy_off_{r}", functools.partial(_residue_image, r), (f"entropy_off_mod16_{r}",), group="residue"))
    return t


def _residue_base() -> bytes:
    return noise(40, 24, 95, "420", 0, 77)


def _residue_image(r: int) -> bytes:
    """The small image whose scan starts at a file offset of residue r mod 16."""
    base = _residue_base()
    return with_comment(base, (r - entropy_off(base) - 4) % 16)


CASES = _table()
