"""The resample route case table (test infrastructure; see tests/test_resample_routes_table.py for the
CPU proof of its coverage and tests/test_gpu_resample_routes.py for the GPU run).

One named case = image size, sampling, filter, crop mode, resolution, and the route plan_image /
image_routes (restated in tests/resample_plan.py) is meant to send it to.  Images are as small as the route
allows; only the multi-tile cases need a 200-700 pixel side (two 960-column-bound cases are wider, and
a few rows tall)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import resample_plan as P

SAMPLINGS = {"420": P.S420, "422": P.S422, "444": P.S444, "gray": P.GRAY, "440": P.S440}


@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    samp: str                 # key of SAMPLINGS
    res: tuple                # (out_h, out_w)
    route: str                # intended route (resample_plan.ROUTE_NAMES)
    filter: str = "bilinear"
    crop: bool = True
    multi: bool = False       # intended: more than one column tile (out_w > tile_w)
    group: str = ""           # "edge": crop box at a chroma block boundary; "span960": generic tile at kMaxSpan
    content: str = "synth"    # "synth": tests.golden.synth.synth_rgb; "noise": uniform noise

    @property
    def op(self) -> P.Op:
        return P.Op(self.res[0], self.res[1], self.crop, self.filter)

    def plan(self) -> P.Plan:
        return P.plan(self.w, self.h, SAMPLINGS[self.samp], self.op)


def _spec(lay: str, kt: int) -> str:
    return f"kRtF_{lay}_{kt}"


def _table() -> list[Case]:
    t: list[Case] = []
    small, wide, mid = (48, 64), (225, 300), (150, 200)
    for lay in ("420", "422", "444", "gray"):
        # -- specialised k_rs420<KT, LAY>, one column tile: bilinear scales <= 1, 1.56, 2.5, 3.6, 4.5
        for kt, (w, h) in zip(P.SPEC_TAPS, ((56, 40), (100, 80), (160, 130), (230, 180), (288, 216))):
            t.append(Case(f"{lay}_kt{kt}_single", w, h, lay, small, _spec(lay, kt)))
        # -- ... scales 2.5 and 4.5 fill 5 and 9 taps of the 7 and 11 (a window holds at most ceil(2 x support)
        # taps, one fewer than the kernel's count): 2.8 and 4.8 reach the 6th and the 10th
        t.append(Case(f"{lay}_kt7_wide_window", 180, 150, lay, small, _spec(lay, 7)))
        t.append(Case(f"{lay}_kt11_wide_window", 310, 240, lay, small, _spec(lay, 11)))
        # -- ... and more than one: out_w 300 > 256 for KT <= 7 (an 8-row ring holds 256-column tiles); a
        # vertical window of 9..16 rows caps the tile at kRingDW / 16 = 192 columns, so out_w 200 does for 9, 11
        t.append(Case(f"{lay}_kt3_multi", 200, 160, lay, wide, _spec(lay, 3), multi=True))
        t.append(Case(f"{lay}_kt5_multi", 480, 370, lay, wide, _spec(lay, 5), multi=True))
        t.append(Case(f"{lay}_kt7_multi", 200, 160, lay, wide, _spec(lay, 7), filter="lanczos", multi=True))
        t.append(Case(f"{lay}_kt9_multi", 240, 190, lay, mid, _spec(lay, 9), filter="lanczos", multi=True))
        t.append(Case(f"{lay}_kt11_multi", 320, 250, lay, mid, _spec(lay, 11), filter="lanczos", multi=True))
    # -- the other filters, every tap count at least once
    t += [
        Case("420_box_kt3", 100, 80, "420", small, _spec("420", 3), filter="box"),
        Case("gray_hamming_kt3", 56, 40, "gray", small, _spec("gray", 3), filter="hamming"),
        Case("420_bicubic_kt5", 56, 40, "420", small, _spec("420", 5), filter="bicubic"),
        Case("444_box_kt5", 160, 130, "444", small, _spec("444", 5), filter="box"),
        Case("422_bicubic_kt7", 80, 64, "422", small, _spec("422", 7), filter="bicubic"),
        Case("422_lanczos_kt7", 56, 40, "422", small, _spec("422", 7), filter="lanczos"),
        Case("444_bicubic_kt9", 100, 80, "444", small, _spec("444", 9), filter="bicubic"),
        Case("gray_lanczos_kt9", 80, 64, "gray", small, _spec("gray", 9), filter="lanczos"),
        Case("gray_lanczos_kt11", 100, 80, "gray", small, _spec("gray", 11), filter="lanczos"),
        Case("444_bicubic_kt11", 140, 110, "444", small, _spec("444", 11), filter="bicubic"),
        # bilinear multi-tile through the 192-column cap, and the 4:2:2 example at out_w 400
        Case("420_bilinear_kt9_multi", 700, 540, "420", mid, _spec("420", 9), multi=True),
        Case("422_kt5_multi_400", 600, 450, "422", (300, 400), _spec("422", 5), multi=True),
    ]
    # -- generic k_resample<KT>
    t += [
        Case("gen1_vertical_only", 64, 100, "420", small, "kRtGen1", crop=False),
        Case("gen1_identity", 64, 48, "422", small, "kRtGen1"),
        Case("gen1_crop_only", 64, 100, "444", small, "kRtGen1"),          # the crop has the output's size
        Case("gen3_440", 56, 40, "440", small, "kRtGen3"),
        Case("gen5_ksv_over_vtaps", 200, 400, "420", (100, 100), "kRtGen5", crop=False),
        Case("gen5_440", 100, 80, "440", small, "kRtGen5"),
        Case("gen7_horizontal_only", 180, 48, "444", small, "kRtGen7", crop=False),
        Case("gen9_chroma_dw2", 4, 16, "420", (4, 1), "kRtGen9", crop=False),
        Case("gen11_440", 154, 120, "440", (24, 32), "kRtGen11"),
        Case("gen0_15taps", 700, 200, "420", (100, 100), "kRtGen0", crop=False),
        Case("gen0_multi", 980, 60, "422", (30, 150), "kRtGen0", crop=False, multi=True),
        Case("gen5_multi_horizontal_only", 360, 50, "422", (50, 300), "kRtGen5", crop=False, multi=True),
        Case("gen9_span960_444_multi", 1896, 24, "444", (24, 512), "kRtGen9", crop=False, multi=True, group="span960"),
        Case("gen9_span960_440", 948, 32, "440", (16, 256), "kRtGen9", crop=False, group="span960"),
        Case("unfused_ksv19", 300, 900, "420", (100, 100), "kRtUnfused", crop=False),
    ]
    # -- crop boxes on, one before and one after a chroma block boundary (16 image columns / rows for a
    # 2x subsampled direction): a square target crops 128 x 96 to columns [16, 112), 126 to [15, 111),
    # 130 to [17, 113); the transposes move the rows
    for lay in ("420", "422", "440"):
        route = "kRtGen5" if lay == "440" else _spec(lay, 5)
        for w, h in ((126, 96), (128, 96), (130, 96), (96, 126), (96, 128), (96, 130)):
            t.append(Case(f"edge_{lay}_{w}x{h}", w, h, lay, (48, 48), route, group="edge", content="noise"))
    return t


CASES = _table()

# The 64-row-strip group: launch_resample takes strip_h = 64 for a lane of >= 512 images; out_h 65 is two
# strips (64 + 1), 130 three (64 + 64 + 2).  Distinct tiny images of every sampling, cycled to the batch.
STRIP_BATCH = 512
STRIP_OPS = (((65, 52), "bilinear"), ((130, 52), "bilinear"), ((65, 52), "lanczos"), ((130, 52), "lanczos"))
STRIP_IMAGES = [
    ("420", 100, 80), ("422", 90, 70), ("444", 77, 61), ("gray", 64, 48), ("440", 50, 80), ("420", 33, 47),
    ("422", 51, 38), ("444", 40, 100), ("gray", 99, 79), ("440", 96, 64), ("420", 70, 90), ("422", 100, 33),
]


def strip_cases() -> list[Case]:
    out = []
    for res, filt in STRIP_OPS:
        for samp, w, h in STRIP_IMAGES:
            c = Case(f"strip{res[0]}_{filt}_{samp}_{w}x{h}", w, h, samp, res, "", filter=filt)
            out.append(Case(c.name, w, h, samp, res, c.plan().route_name, filter=filt, multi=c.plan().multi_tile,
                            group="strip"))
    return out


# -- images ----------------------------------------------------------------------------------------------
def _coef_jpeg(w: int, h: int, comps, rng) -> bytes:
    """A baseline JPEG of the given (h, v) sampling from chosen coefficients (PIL's encoder writes no
    4:4:0): a DC random walk and a few low-frequency AC terms per block, as six_slot_jpegs."""
    from tests.golden.coefjpeg import write_jpeg
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    blocks = []
    for hs, vs in comps:
        bh, bw = mcuy * vs, mcux * hs
        b = np.zeros((bh, bw, 64), np.int64)
        for y in range(bh):
            for x in range(bw):
                k = rng.choice(np.arange(1, 30), int(rng.integers(0, 8)), replace=False)
                b[y, x, k] = rng.integers(-30, 31, len(k))
        b[:, :, 0] = np.clip(np.cumsum(rng.integers(-50, 51, (bh, bw)), axis=1), -900, 900)
        blocks.append(b)
    q = {0: rng.integers(2, 24, 64), 1: rng.integers(2, 40, 64)}
    return write_jpeg(w, h, [(hs, vs, 0 if ci == 0 else 1) for ci, (hs, vs) in enumerate(comps)], blocks, q)


@functools.lru_cache(maxsize=None)
def image(samp: str, w: int, h: int, content: str = "synth") -> bytes:
    """The JPEG of a case: deterministic in (sampling, size, content)."""
    import zlib
    from tests.golden.synth import encode_jpeg, synth_rgb
    rng = np.random.default_rng(zlib.crc32(f"{samp}:{w}x{h}:{content}".encode()))
    if samp == "440":
        return _coef_jpeg(w, h, SAMPLINGS[samp], rng)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if content == "noise" else synth_rgb(rng, w, h)
    if samp == "gray":
        from PIL import Image
        return encode_jpeg(np.array(Image.fromarray(rgb).convert("L")), 90)
    return encode_jpeg(rgb, 90, subsampling={"444": 0, "422": 1, "420": 2}[samp])


def case_image(c: Case) -> bytes:
    return image(c.samp, c.w, c.h, c.content)
