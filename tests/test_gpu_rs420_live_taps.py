"""The live taps of k_rs420 against the oracle, bit for bit.

A Pillow window holds at most ceil(2 x support) taps (tests/resample_plan.py window_counts), so a KT-tap kernel
(KT = 2 ceil(support) + 1) sees KT - 1 live taps when 2 x support > KT - 2 and KT - 2 otherwise -- never KT: the last
weight of each row of the table is padding.  k_rs420 therefore runs KT - 1 horizontal taps on a tile and KT - 1
vertical taps on a strip unless the bounds table shows a full window, and reads only the dwords the live bytes span.
SHAPES takes both live counts for every tap count, with a different ratio on each axis, and asserts them from the
restated planner: KT = 5 at the ratios 1.875 (VGA's: 2 x support = 3.75, four live taps), 1.4 (three) and 2.0
(2 x support = 4, still four); 2.2 is already KT = 7 with five, the first window past one dword.  The KT-tap branches
stay for a table with a fuller window, which Pillow's bounds do not produce.

Every case runs through all five filters back to back on one engine: BOX, BILINEAR and HAMMING (weights never
negative) and BICUBIC and LANCZOS (signed weights; at these shapes their wider windows also reach the other tap
counts and the generic kernel).

Contents: a synthetic gradient image and noise for every shape; all-255, all-0, and one-pixel checkerboards of
columns and of rows (the largest sums, and a dropped or doubled tap would show at once) at the VGA ratio and at an
11-tap one.  Windows clipped by the image's edges are in every case (asserted: the first and the last window are
shorter than the widest).  Geometry: out_w 300 (a second tile with its own byte shift and weights), 64-row strips at
out_h 65 and 130 whose first source row is no multiple of 4, odd crop offsets on either axis; uint8 / CHW /
unflipped and float LUT / HWC / flipped outputs; 4:2:0, 4:2:2, 4:4:4 and grayscale."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import gpu_debug  # noqa: E402
from tests import resample_plan as P  # noqa: E402
from tests.resample_cases import SAMPLINGS, image  # noqa: E402

FORMS = ((False, "chw", False), (True, "hwc", True))  # (normalize, layout, flip)
LAYS = ("420", "422", "444", "gray")
FILTERS = ("bilinear", "bicubic", "box", "lanczos", "hamming")  # non-negative and signed weights alternating

# name: (w, h, out_h, out_w, filter that pins the plan, KT, live taps H, live taps V); no crop, so the axes differ
SHAPES = {
    "kt3_live2_v3": (54, 67, 48, 60, "bilinear", 3, 2, 3),      # upscale 0.9; V 1.4
    "kt3_live1_box": (54, 60, 48, 60, "box", 3, 1, 2),           # BOX at scale <= 1: one tap; V 1.25
    "kt5_live4_vga": (105, 67, 48, 56, "bilinear", 5, 4, 3),     # 1.875 (VGA -> 256); V 1.4
    "kt5_live3": (84, 80, 40, 60, "bilinear", 5, 3, 4),          # 1.4; V 2.0
    "kt5_live4_support2": (100, 79, 36, 50, "bilinear", 5, 4, 5),  # 2.0: 2 x support = 4; V 2.19 (ksv 7)
    "kt7_live5": (110, 112, 40, 50, "bilinear", 7, 5, 6),        # 2.2: five taps, the first past one dword; V 2.8
    "kt7_live6": (140, 90, 64, 50, "bilinear", 7, 6, 3),         # 2.8; V 1.41
    "kt9_live7": (132, 152, 40, 40, "bilinear", 9, 7, 8),        # 3.3; V 3.8
    "kt9_live8": (152, 132, 40, 40, "bilinear", 9, 8, 7),        # 3.8: two whole dwords of taps; V 3.3
    "kt11_live9": (168, 192, 40, 40, "bilinear", 11, 9, 10),     # 4.2: one tap in the third dword; V 4.8
    "kt11_live10": (192, 168, 40, 40, "bilinear", 11, 10, 9),    # 4.8; V 4.2
    "kt5_two_tiles": (563, 75, 40, 300, "bilinear", 5, 4, 4),    # out_w 300: tiles of 256 and 44 columns
}
EXTREME_SHAPES = ("kt5_live4_vga", "kt11_live10")
EXTREMES = ("white", "black", "noise", "columns", "rows")
# (w, h, out_h, out_w, cx0, cy0) with crop: odd offsets, both at the VGA ratio 1.875
CROPS = {"odd_cx0": (152, 90, 48, 48, 31, 0), "odd_cy0": (90, 152, 48, 48, 0, 31)}
# 64-row strips (a lane of 512 images): (w, h, out_h, out_w), ratio 1.877 on both axes
STRIPS = {"strip65": (98, 122, 65, 52), "strip130": (98, 244, 130, 52)}
STRIP_BATCH = 512


@functools.lru_cache(maxsize=None)
def extreme_image(kind: str, lay: str, w: int, h: int) -> bytes:
    from PIL import Image
    from tests.golden.synth import encode_jpeg
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        rgb = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        v = {"white": np.full((h, w), 255), "black": np.zeros((h, w)), "columns": 255 * (x & 1), "rows": 255 * (y & 1)}[kind]
        rgb = np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2)
    if lay == "gray":
        return encode_jpeg(np.array(Image.fromarray(rgb).convert("L")), 100)
    return encode_jpeg(rgb, 100, subsampling={"444": 0, "422": 1, "420": 2}[lay])


class Rig:
    def __init__(self):
        from sds_amd.engine import JpegEngine
        self.engine = JpegEngine(max_batch=STRIP_BATCH)
        self.refs = {}

    def ref(self, jpg: bytes, res, crop, filt, form) -> np.ndarray:
        """The oracle's output, computed once per (image, op) and shared read-only."""
        key = (jpg, res, crop, filt)
        if key not in self.refs:
            r = O.pipeline(jpg, res, crop_before_resize=crop, filter=filt)
            r.setflags(write=False)
            self.refs[key] = r
        chw = self.refs[key]
        normalize, layout, flip = form
        if flip:
            chw = chw[:, :, ::-1]
        if normalize:
            chw = O.normalize_lut()[chw]
        return np.ascontiguousarray(chw.transpose(1, 2, 0) if layout == "hwc" else chw)

    def run(self, jpgs, res, crop, filt, form, uniq=None):
        """Decodes jpgs as one chunk and compares every output with the oracle; returns the chunk's descriptors."""
        normalize, layout, flip = form
        out, st = self.engine.decode_resize(jpgs, res, crop_before_resize=crop, filter=filt, normalize=normalize,
                                            layout=layout, flip=[flip] * len(jpgs))
        descs, _ = gpu_debug.snapshot(self.engine, len(jpgs))
        assert (st == 0).all(), st
        got = out.cpu().numpy()
        assert got.dtype == (np.float32 if normalize else np.uint8)
        for k, jpg in enumerate(jpgs):
            np.testing.assert_array_equal(got[k], self.ref(jpg, res, crop, filt, form), err_msg=f"image {k} {filt} {form}")
        return descs


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Rig()


def _check_plan(w, h, lay, res, crop, filt, kt, live_h, live_v, desc=None):
    p = P.plan(w, h, SAMPLINGS[lay], P.Op(res[0], res[1], crop, filt))
    assert (p.rs_fast, p.rs_lay, p.max_hc, p.max_vc) == (kt, LAYS.index(lay), live_h, live_v), (w, h, lay, res, filt, p)
    assert p.ksv <= kt or p.ksv <= P.rs_vtaps(kt)
    if desc is not None:
        assert (desc.status, desc.rs_fast, desc.rs_lay, desc.ksv, desc.tile_w) == (0, kt, p.rs_lay, p.ksv, p.tile_w)
    return p


def test_the_shapes_reach_the_intended_windows():
    """(no GPU work) Both live counts of every tap count, clipped windows at both ends, and the two tiles."""
    seen = set()
    for name, (w, h, oh, ow, filt, kt, lh, lv) in SHAPES.items():
        for lay in LAYS:
            p = _check_plan(w, h, lay, (oh, ow), False, filt, kt, lh, lv)
        sup = P.FILTER_SUPPORT[filt]
        for n_in, n_out in ((w, ow), (h, oh)):
            c = P.window_counts(n_in, n_out, sup)
            assert max(c) <= kt - 1 or n_in == h
            if max(c) > 1:
                assert c[0] < max(c) and c[-1] < max(c), name
        seen.add((kt, kt - lh))
        assert p.multi_tile == (name == "kt5_two_tiles")
    assert seen == {(kt, d) for kt in P.SPEC_TAPS for d in (1, 2)}
    for w, h, oh, ow, cx0, cy0 in CROPS.values():
        p = _check_plan(w, h, "420", (oh, ow), True, "bilinear", 5, 4, 4)
        assert (p.cx0, p.cy0) == (cx0, cy0) and (cx0 | cy0) & 1
    for w, h, oh, ow in STRIPS.values():
        _check_plan(w, h, "420", (oh, ow), True, "bilinear", 5, 4, 4)
        sup, scale = 1.0, h / oh
        first = int((64 + 0.5) * scale - sup * scale + 0.5)  # the second strip's first source row
        assert first % 4 != 0


@pytest.mark.parametrize("name", list(SHAPES), ids=list(SHAPES))
def test_shape_through_every_filter(rig, name):
    w, h, oh, ow, pin, kt, lh, lv = SHAPES[name]
    jpgs = [image(lay, w, h, content) for lay in LAYS for content in ("synth", "noise")]
    for form in FORMS:
        for filt in FILTERS:
            descs = rig.run(jpgs, (oh, ow), False, filt, form)
            if filt == pin:
                for k, d in enumerate(descs):
                    _check_plan(w, h, LAYS[k // 2], (oh, ow), False, filt, kt, lh, lv, d)


@pytest.mark.parametrize("name", EXTREME_SHAPES)
def test_extreme_pixels(rig, name):
    w, h, oh, ow, pin, kt, lh, lv = SHAPES[name]
    jpgs = [extreme_image(kind, lay, w, h) for lay in LAYS for kind in EXTREMES]
    white = O.pipeline(extreme_image("white", "444", w, h), (oh, ow), crop_before_resize=False, filter="bilinear")
    assert white.min() >= 254  # (the largest sums: every tap on 255 or next to it)
    for form in FORMS:
        for filt in FILTERS:
            descs = rig.run(jpgs, (oh, ow), False, filt, form)
            if filt == pin:
                assert all(d.rs_fast == kt for d in descs)


@pytest.mark.parametrize("name", list(CROPS), ids=list(CROPS))
def test_odd_crop_offsets(rig, name):
    w, h, oh, ow, cx0, cy0 = CROPS[name]
    jpgs = [image(lay, w, h, "noise") for lay in LAYS]
    for form in FORMS:
        for filt in FILTERS:
            descs = rig.run(jpgs, (oh, ow), True, filt, form)
            if filt == "bilinear":
                assert all((d.rs_fast, d.cx0, d.cy0) == (5, cx0, cy0) for d in descs)


@pytest.mark.parametrize("name", list(STRIPS), ids=list(STRIPS))
def test_64_row_strips(rig, name):
    """A lane of 512 images takes 64-row strips: out_h 65 and 130 are two and three of them, the later ones
    starting at a source row that is no multiple of the 4-row step."""
    w, h, oh, ow = STRIPS[name]
    four = [image(lay, w, h, "noise") for lay in LAYS]
    batch = [four[k % 4] for k in range(STRIP_BATCH)]
    rig.engine.set_lanes(1)  # one lane of 512: with 4 lanes each would hold 128 images and take 16-row strips
    try:
        assert P.strip_h(len(batch), lanes=1) == [P.K_MAX_STRIP]
        for form in FORMS:
            for filt in ("bilinear", "lanczos", "hamming"):
                descs = rig.run(batch, (oh, ow), True, filt, form)
                if filt == "bilinear":
                    assert all(d.rs_fast == 5 for d in descs)
    finally:
        rig.engine.set_lanes(4)
