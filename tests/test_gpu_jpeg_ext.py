"""The opt-in wider JPEG subset on the GPU (gpu_formats "jpeg-ext": upsampling ratios of 3 and 4 through k_color's
int_upsample, RGB-coded files without the colour transform, baseline and progressive) against
np.asarray(PIL.Image.open(...).convert("RGB")), bit for bit -- the oracle does not restate these samplings, so PIL
is the reference, as for PNG -- and, for resized outputs, PIL's pixels through the oracle's crop_box / resize exactly
as tests/test_gpu_frames.py::_ref does.

Every ext fixture must be decoded natively: counters()["ok"] grows by their number and counters()["fallback"] by
zero, so the hand-over to PIL cannot hide a failure.  Without "jpeg-ext" the same files report UNSUPPORTED, and for
refused and damaged files the opt-in route must give the same tensor or the same exception type as the default
route on the same bytes."""
import io
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (crop_box / resize only: the checker of the geometry)
from tests import jpeg_ext_synth as J  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402

EXT = ("jpeg", "jpeg-ext")


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def refs():
    """(name, bytes, PIL's pixels) of every ext fixture, computed once."""
    return [(n, d, J.pil_rgb(d)) for n, d in J.ext_fixtures()]


# -- 1. the decode alone -------------------------------------------------------------------------------
def test_every_fixture_decodes_to_pils_pixels(engine, refs):
    from sds_amd.batched import GpuDecodeBatch
    assert len(refs) == 52
    c0 = engine.counters()
    for (h, w), group in P.by_size(refs).items():
        batch = GpuDecodeBatch("jpg", (h, w), device="cuda", gpu_formats=EXT, on_error="raise")(
            {"jpg": [d for _, d, _ in group], "name": [n for n, _, _ in group]})
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(group), 3, h, w)
        for k, (n, _, ref) in enumerate(group):
            np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=n)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == len(refs)


# -- 2. geometry ---------------------------------------------------------------------------------------
GEO_SETS = ("410", "2x3", "mixed", "lumasub")
# (20, 8): the crop of the 50 x 37 files starts off the left edge; (8, 20): that of the 33 x 70 files off the top edge
GEO = [dict(res=(16, 20)), dict(res=(20, 8)), dict(res=(8, 20)), dict(res=(16, 20), flip=True),
       dict(res=(16, 20), normalize=True), dict(res=(16, 20), layout="hwc"),
       dict(res=(40, 90), filt="bicubic", crop=False)]


@pytest.mark.parametrize("cfg", GEO, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_resized_outputs_through_both_entry_points(engine, refs, cfg):
    """Eight samples on the host entry point: latency mode; the device-resident entry point plans them as a batch."""
    res, filt, crop = cfg["res"], cfg.get("filt", "bilinear"), cfg.get("crop", True)
    flip, normalize, layout = cfg.get("flip", False), cfg.get("normalize", False), cfg.get("layout", "chw")
    by_name = {n: (d, r) for n, d, r in refs}
    names = [f"{s}-{w}x{h}" for s in GEO_SETS for (w, h) in ((50, 37), (33, 70))]
    samples = [by_name[n][0] for n in names]
    flips = [flip and k % 3 != 1 for k in range(len(names))]
    ref = []
    for n, f in zip(names, flips):
        chw = _ref(by_name[n][1], res, filt, crop=crop, flip=f, normalize=normalize)
        ref.append(chw.transpose(1, 2, 0) if layout == "hwc" else chw)
    if crop and res != (16, 20):  # (left, top) of the two sizes' crop boxes
        assert (O.crop_box(50, 37, *res)[0] > 0) if res == (20, 8) else (O.crop_box(33, 70, *res)[1] > 0)
    kw = dict(filter=filt, crop_before_resize=crop, normalize=normalize, layout=layout, formats=EXT)
    c0 = engine.counters()
    outs = {}
    out, st = engine.decode_resize(samples, res, flip=flips, **kw)
    outs["host"] = (out.cpu().numpy(), np.asarray(st))
    outs["device"] = P.decode_device(engine, samples, res, flip=flips, **kw)
    P.assert_rows_equal(outs, ref)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0 and c1["ok"] - c0["ok"] == 2 * len(samples)


# -- 3. lanes --------------------------------------------------------------------------------------------
def _pillow_420(w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * (2 + c) + yy * (7 - c) + rng.integers(0, 32, (h, w))) % 256 for c in range(3)], -1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=88, subsampling=2)
    return buf.getvalue()


def test_a_batch_of_several_lanes_mixing_420_and_ext(engine, refs):
    """512 samples (two kernel lanes of 256): Pillow 4:2:0 files, which keep the fused kernels, between ext files,
    which take the unfused ones; every row equals its own reference."""
    res = (24, 32)
    plain = [_pillow_420(w, h, k) for k, (w, h) in enumerate([(64, 48), (50, 37), (33, 70), (96, 40), (17, 23), (80, 80)])]
    ext = [(n, d, r) for n, d, r in refs if min(r.shape[:2]) >= 9 or "5x9" in n]
    distinct = [(d, J.pil_rgb(d)) for d in plain] + [(d, r) for _, d, r in ext]
    ref1 = [_ref(r, res) for _, r in distinct]
    # every distinct sample at least once, every third sample a 4:2:0 file, the rest drawn from all of them
    order = np.random.default_rng(0).integers(0, len(distinct), 512)
    order[::3] = np.arange(len(order[::3])) % len(plain)
    order[1:3 * len(distinct):3] = np.arange(len(distinct))
    order = [int(o) for o in order]
    assert set(order) == set(range(len(distinct))) and len(distinct) > len(plain) + 40
    samples = [distinct[o][0] for o in order]
    c0 = engine.counters()
    out, st = engine.decode_resize(samples, res, formats=EXT)
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
    for fm in (("jpeg",), None, ("jpeg", "png-ext", "png-meta")):
        _, st = engine.decode_resize(files, (16, 20), formats=fm)
        assert (np.asarray(st) == -2).all(), (fm, st)
    c1 = engine.counters()
    assert c1["ok"] == c0["ok"] and c1["unsupported"] - c0["unsupported"] == 3 * len(files)
    _, st = engine.decode_resize(files, (16, 20), formats=EXT)  # the mask travels with the call ...
    assert (np.asarray(st) == 0).all()
    _, st = engine.decode_resize(files, (16, 20))  # ... and does not stay behind on the shared engine
    assert (np.asarray(st) == -2).all()
    # the JFIF + Adobe transform 0 file is YCbCr under either mask
    both = J.jfif_and_adobe0()
    a, sa = engine.decode_resize([both], (37, 50))
    b, sb = engine.decode_resize([both], (37, 50), formats=EXT)
    assert sa[0] == 0 and sb[0] == 0
    np.testing.assert_array_equal(a[0].cpu().numpy(), J.pil_rgb(both).transpose(2, 0, 1))
    np.testing.assert_array_equal(b[0].cpu().numpy(), a[0].cpu().numpy())


def test_the_default_pipeline_gives_the_ext_pipelines_output(engine, refs):
    tmp = tempfile.mkdtemp()
    c0 = engine.counters()
    for k, (n, d, _) in enumerate(refs):
        p = os.path.join(tmp, f"{k}.jpg")
        with open(p, "wb") as f:
            f.write(d)
        a, b = P.pipeline_outcome(p, gpu_formats=EXT), P.pipeline_outcome(p)
        assert a[0] == "ok" and b[0] == "ok", (n, a, b)
        np.testing.assert_array_equal(a[1], b[1], err_msg=n)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == len(refs)  # (the default route's reruns on PIL; the ext route has none)


# -- 5. damage and refusal ---------------------------------------------------------------------------------
DAMAGE = list(J.refused()) + list(J.damaged())


@pytest.mark.parametrize("name,data", DAMAGE, ids=[n for n, _ in DAMAGE])
def test_refused_and_damaged_files_equal_the_default_route(engine, name, data):
    P.check_handover_and_damage(engine, data, EXT, J.make("411", 13, 7, seed=1))


# -- 6. the per-sample transform -----------------------------------------------------------------------------
def test_need_size_uses_the_probe_under_the_mask(engine):
    """allow_vertical needs the image size before the decode: with "jpeg-ext" a 4:1:0 file is sized by
    sdsj_probe_formats and decoded natively (no fallback)."""
    from sds_amd.presets import create_standard_image_pipeline
    data = dict(J.ext_fixtures())["410-33x70"]
    p = os.path.join(tempfile.mkdtemp(), "x.jpg")
    with open(p, "wb") as f:
        f.write(data)
    c0 = engine.counters()
    kw = dict(device="cuda", service=None, resize_kwargs=dict(allow_vertical=True))
    a = P.run_transforms(create_standard_image_pipeline("jpg", (16, 32), gpu_formats=EXT, **kw), {"jpg": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("jpg", (16, 32), **kw), {"jpg": p})["image"]
    assert tuple(a.shape) == tuple(b.shape) == (3, 32, 16)
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["ok"] - c0["ok"] == 1 and c1["fallback"] - c0["fallback"] == 0


# -- 7. mask validation ----------------------------------------------------------------------------------------
def test_the_bit_alone_is_refused_by_a_live_engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd import _lib as L
    from sds_amd.engine import JpegEngine
    eng = JpegEngine("cuda", max_batch=4)
    lib = L.load()
    for mask in (64, 66):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.EINVAL
    for mask in (65, 67):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.OK
    assert lib.sdsj_engine_set_formats(eng._h, L.FORMAT_JPEG) == L.OK
