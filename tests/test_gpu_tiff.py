"""The opt-in TIFF format on the GPU (gpu_formats "tiff": k_tiff_copy, k_tiff_lzw, k_tiff_inflate, k_tiff_rgb)
against the pixels the files were written from, bit for bit -- tests/tiff_synth.py takes the samples that must come
out, and tests/test_tiff_host.py pins that writer to PIL (its raw decoder and libtiff), the reference --, and, for
resized outputs, those pixels through the oracle's crop_box / resize exactly as tests/test_gpu_frames.py::_ref does.

Every native() fixture must be decoded natively: counters()["ok"] grows by their number and counters()["fallback"]
by zero, so the hand-over to PIL cannot hide a failure.  Without "tiff" the same files report UNSUPPORTED, and for
refused and damaged files the opt-in route must give the same tensor or the same exception type as the default
route on the same bytes."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (crop_box / resize only: the checker of the geometry)
from tests import gif_synth as G  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests import png_synth as S  # noqa: E402
from tests import tiff_synth as T  # noqa: E402
from tests import webp_synth as W  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402
from tests.test_gpu_jpeg_ext import _pillow_420  # noqa: E402

TIFF = ("jpeg", "tiff")


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def refs():
    """(name, bytes, expected pixels) of every native() fixture, the committed Pillow files among them."""
    return T.native()


# -- 1. the decode alone -------------------------------------------------------------------------------
def test_every_fixture_decodes_to_its_expected_pixels(engine, refs):
    from sds_amd.batched import GpuDecodeBatch
    assert len(refs) >= 90 and max(r.shape[0] * r.shape[1] for _, _, r in refs) == 320 * 240
    c0 = engine.counters()
    for (h, w), group in P.by_size(refs).items():
        batch = GpuDecodeBatch("tiff", (h, w), device="cuda", gpu_formats=TIFF, on_error="raise")(
            {"tiff": [d for _, d, _ in group], "name": [n for n, _, _ in group]})
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(group), 3, h, w)
        for k, (n, _, ref) in enumerate(group):
            np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=n)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == len(refs)
    assert c1["png"] - c0["png"] == 0  # (no counter of their own, and not PNG's)


# -- 2. geometry ---------------------------------------------------------------------------------------
# (20, 8): the crop of the 50 x 37 files starts off the left edge; (8, 20): that of the 33 x 70 files off the top
# edge and ends well above the bottom, so strips below it are decoded but never turned to RGB
GEO = [dict(res=(16, 20)), dict(res=(20, 8)), dict(res=(8, 20)), dict(res=(16, 20), flip=True),
       dict(res=(16, 20), normalize=True), dict(res=(16, 20), layout="hwc"),
       dict(res=(40, 90), filt="bicubic", crop=False)]


def _geo_samples(refs):
    """Eight files of two sizes: every compression, predictor 2 (whose rows are summed from their first pixel, left
    of the crop), a ColorMap, CMYK, an extra sample."""
    by = dict((n, (d, r)) for n, d, r in refs)
    return [by[n] for n in ("rgb_lzw", "p_packbits", "cmyk_deflate", "la_none",
                            "rgb_lzw_pred", "rgba_deflate_pred", "p_lzw_pred", "l0_deflate_pred")]


@pytest.fixture(scope="module")
def geo(refs):
    samples = _geo_samples(refs)
    return [d for d, _ in samples], [r for _, r in samples]


@pytest.mark.parametrize("cfg", GEO, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_resized_outputs_through_both_entry_points(engine, geo, cfg):
    """Eight samples on the host entry point: latency mode; the device-resident entry point plans them as a batch."""
    res, filt, crop = cfg["res"], cfg.get("filt", "bilinear"), cfg.get("crop", True)
    flip, normalize, layout = cfg.get("flip", False), cfg.get("normalize", False), cfg.get("layout", "chw")
    samples, pix = geo
    assert [p.shape[:2] for p in pix] == [(37, 50)] * 4 + [(70, 33)] * 4
    flips = [flip and k % 3 != 1 for k in range(len(samples))]
    ref = []
    for p, f in zip(pix, flips):
        chw = _ref(p, res, filt, crop=crop, flip=f, normalize=normalize)
        ref.append(chw.transpose(1, 2, 0) if layout == "hwc" else chw)
    if crop and res != (16, 20):  # (left, top) of the two sizes' crop boxes
        assert (O.crop_box(50, 37, *res)[0] > 0) if res == (20, 8) else (O.crop_box(33, 70, *res)[1] > 0)
    if crop and res == (8, 20):
        assert O.crop_box(33, 70, *res)[3] < 70 - 16  # the crop's last row: well above the image's
    kw = dict(filter=filt, crop_before_resize=crop, normalize=normalize, layout=layout, formats=TIFF)
    c0 = engine.counters()
    outs = {}
    out, st = engine.decode_resize(samples, res, flip=flips, **kw)
    outs["host"] = (out.cpu().numpy(), np.asarray(st))
    outs["device"] = P.decode_device(engine, samples, res, flip=flips, **kw)
    P.assert_rows_equal(outs, ref)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0 and c1["ok"] - c0["ok"] == 2 * len(samples)


# -- 3. lanes --------------------------------------------------------------------------------------------
def test_a_batch_of_several_lanes_mixing_jpeg_png_gif_webp_and_tiff(engine, refs):
    """512 samples (two kernel lanes of 256) under all five names: Pillow 4:2:0 files, which keep the fused kernels,
    PNGs, GIFs, WebPs and TIFFs, which share the unfused ones; every row equals its own reference."""
    res = (24, 32)
    sizes = [(64, 48), (50, 37), (33, 70), (96, 40), (17, 23), (80, 80)]
    jpgs = [_pillow_420(w, h, k) for k, (w, h) in enumerate(sizes)]
    pngs = [S.make(w, h, ct, seed=k) for k, ((w, h), ct) in enumerate(zip(sizes, (0, 2, 3, 4, 6, 2)))]
    gifs = [d for n, d in G.native()[:12]]
    webps = [(d, r) for n, d, r in W.native()[:12] if min(r.shape[:2]) >= 6]
    tiffs = [(d, r) for n, d, r in refs if min(r.shape[:2]) >= 6]
    distinct = ([(d, S.pil_rgb(d)) for d in jpgs + pngs] + [(d, G.pil_rgb(d)) for d in gifs if min(G.pil_rgb(d).shape[:2]) >= 6]
                + webps + tiffs)
    ref1 = [_ref(r, res) for _, r in distinct]
    order = np.random.default_rng(0).integers(0, len(distinct), 512)
    order[::3] = np.arange(len(order[::3])) % len(jpgs)
    order[1:3 * len(distinct):3] = np.arange(len(distinct))
    order = [int(o) for o in order]
    assert set(order) == set(range(len(distinct))) and len(tiffs) > 80 and len(webps) > 4
    samples = [distinct[o][0] for o in order]
    c0 = engine.counters()
    out, st = engine.decode_resize(samples, res, formats=("jpeg", "png", "gif", "webp", "tiff"))
    assert (np.asarray(st) == 0).all(), np.nonzero(np.asarray(st))[0][:8]
    out = out.cpu().numpy()
    for k, o in enumerate(order):
        np.testing.assert_array_equal(out[k], ref1[o], err_msg=f"row {k} (sample {o})")
    c1 = engine.counters()
    assert c1["ok"] - c0["ok"] == 512 and c1["fallback"] - c0["fallback"] == 0


# -- 4. off by default -----------------------------------------------------------------------------------
def test_nothing_moves_without_the_bit(engine, refs):
    files = [d for _, d, _ in refs]
    c0 = engine.counters()
    for fm in (None, ("jpeg",), ("jpeg", "png-ext", "png-meta", "gif", "webp", "jpeg-ext", "jpeg-scans", "jpeg-cmyk-prog")):
        _, st = engine.decode_resize(files, (16, 20), formats=fm)
        assert (np.asarray(st) == -2).all(), (fm, st)
    c1 = engine.counters()
    assert c1["ok"] == c0["ok"] and c1["unsupported"] - c0["unsupported"] == 3 * len(files)
    _, st = engine.decode_resize(files, (16, 20), formats=TIFF)  # the mask travels with the call ...
    assert (np.asarray(st) == 0).all()
    _, st = engine.decode_resize(files, (16, 20))  # ... and does not stay behind on the shared engine
    assert (np.asarray(st) == -2).all()
    _, st = engine.decode_resize(files[:4], (16, 20), formats=("tiff",))  # the bit alone is a mask
    assert (np.asarray(st) == 0).all()


# -- 5. damage and refusal ---------------------------------------------------------------------------------
DAMAGE = list(T.refused()) + list(T.damaged())


@pytest.mark.parametrize("name,data", DAMAGE, ids=[n for n, _ in DAMAGE])
def test_refused_and_damaged_files_equal_the_default_route(engine, name, data):
    good = T.tiff(T.picture(13, 7, 1), 2, T.LZW, rps=3, predictor=2)
    P.check_handover_and_damage(engine, data, TIFF, good)


def test_statuses_of_refused_and_damaged_files(engine):
    """The device's verdicts: UNSUPPORTED for every refused file, CORRUPT for every damaged one -- also where only
    one strip of several is damaged, whichever wavefront meets it."""
    _, st = engine.decode_resize([d for _, d in T.refused()], (16, 20), formats=TIFF)
    assert (np.asarray(st) == -2).all(), st
    _, st = engine.decode_resize([d for _, d in T.damaged()], (16, 20), formats=TIFF)
    assert (np.asarray(st) == -3).all(), st


# -- 6. the per-sample transform -----------------------------------------------------------------------------
def test_need_size_uses_the_tiff_probe(engine):
    """allow_vertical needs the image size before the decode: with "tiff" a 19 x 65 file is sized by sdsj_tiff_probe
    and decoded natively (no fallback)."""
    from sds_amd.presets import create_standard_image_pipeline
    data = T.tiff(T.picture(19, 65, 8), 2, T.ADOBE_DEFLATE, rps=16, predictor=2, bo=">")
    p = os.path.join(tempfile.mkdtemp(), "x.tif")
    with open(p, "wb") as f:
        f.write(data)
    c0 = engine.counters()
    kw = dict(device="cuda", service=None, resize_kwargs=dict(allow_vertical=True))
    a = P.run_transforms(create_standard_image_pipeline("tiff", (16, 32), gpu_formats=TIFF, **kw), {"tiff": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("tiff", (16, 32), **kw), {"tiff": p})["image"]
    assert tuple(a.shape) == tuple(b.shape) == (3, 32, 16)
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["ok"] - c0["ok"] == 1 and c1["fallback"] - c0["fallback"] == 0


# -- 7. mask validation ----------------------------------------------------------------------------------------
def test_masks_on_a_live_engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd import _lib as L
    from sds_amd.engine import JpegEngine
    eng = JpegEngine("cuda", max_batch=4)
    lib = L.load()
    for mask in (16384, 16385, 16384 | 4096 | 256, 16384 | 2 | 4 | 16):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.OK
    for mask in (16384 | 4, 16384 | 64, 16384 | 8, 16384 | 32, 16384 | 2048, 16384 | 8192, 8192):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.EINVAL
    assert lib.sdsj_engine_set_formats(eng._h, L.FORMAT_JPEG) == L.OK
