"""Multi-scan sequential JPEG on the GPU (gpu_formats "jpeg-scans": k_scans walks every scan of a SOF0 / SOF1 file
whose components arrive in more than one scan) against np.asarray(PIL.Image.open(...).convert("RGB")), bit for bit,
and -- for every clean fixture -- against PIL's pixels of the same coefficients written as one interleaved scan; for
resized outputs, PIL's pixels through the oracle's crop_box / resize exactly as tests/test_gpu_frames.py::_ref does.

Every fixture must be decoded natively: counters()["ok"] grows by their number and counters()["fallback"] by zero, so
the hand-over to PIL cannot hide a failure.  Without "jpeg-scans" the same files report UNSUPPORTED, and for refused
and damaged files the opt-in route must give the same tensor or the same exception type as the default route on the
same bytes."""
import io
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import jpeg_ext_synth as J  # noqa: E402
from tests import jpeg_scans_synth as S  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402

SCANS = S.SCANS


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def refs():
    """(name, bytes, PIL's pixels, gpu_formats) of every fixture, computed once."""
    return [(n, d, J.pil_rgb(d), fm) for n, d, fm, _ in S.fixtures()]


def _under(refs, formats):
    return [(n, d, r) for n, d, r, fm in refs if fm == formats]


# -- 1. the decode alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("formats", [S.SCANS, S.SCANS_EXT], ids=["scans", "scans+ext"])
def test_every_fixture_decodes_to_pils_pixels(engine, refs, formats):
    from sds_amd.batched import GpuDecodeBatch
    cases = _under(refs, formats)
    assert len(cases) == (26 if formats == S.SCANS else 3)
    # the same coefficients as one interleaved scan, on PIL (the clean fixtures)
    singles = {n: J.pil_rgb(single) for n, _, _, single in S.clean()}
    c0 = engine.counters()
    for (h, w), group in P.by_size(cases).items():
        batch = GpuDecodeBatch("jpg", (h, w), device="cuda", gpu_formats=formats, on_error="raise")(
            {"jpg": [d for _, d, _ in group], "name": [n for n, _, _ in group]})
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(group), 3, h, w)
        for k, (n, _, ref) in enumerate(group):
            np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=n)
            if n in singles:
                np.testing.assert_array_equal(img[k], singles[n].transpose(2, 0, 1), err_msg=n + " (one scan)")
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == len(cases)
    assert c1["progressive"] == c0["progressive"]  # (the counter keeps counting SOF2 files only)


# -- 2. geometry ---------------------------------------------------------------------------------------
GEO = [dict(res=(16, 20)), dict(res=(16, 20), flip=True), dict(res=(16, 20), normalize=True),
       dict(res=(16, 20), layout="hwc"), dict(res=(40, 90), filt="bicubic", crop=False)]


@pytest.mark.parametrize("cfg", GEO, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_resized_outputs_through_both_entry_points(engine, refs, cfg):
    """Eight samples on the host entry point: latency mode; the device-resident entry point plans them as a batch."""
    res, filt, crop = cfg["res"], cfg.get("filt", "bilinear"), cfg.get("crop", True)
    flip, normalize, layout = cfg.get("flip", False), cfg.get("normalize", False), cfg.get("layout", "chw")
    picked = [(n, d, r) for n, d, r in _under(refs, SCANS) if r.shape[:2] in ((37, 50), (70, 33))][:8]
    assert len(picked) == 8 and len({r.shape for _, _, r in picked}) == 2
    samples = [d for _, d, _ in picked]
    flips = [flip and k % 3 != 1 for k in range(len(picked))]
    ref = []
    for (_, _, r), f in zip(picked, flips):
        chw = _ref(r, res, filt, crop=crop, flip=f, normalize=normalize)
        ref.append(chw.transpose(1, 2, 0) if layout == "hwc" else chw)
    kw = dict(filter=filt, crop_before_resize=crop, normalize=normalize, layout=layout, formats=SCANS)
    c0 = engine.counters()
    outs = {}
    out, st = engine.decode_resize(samples, res, flip=flips, **kw)
    outs["host"] = (out.cpu().numpy(), np.asarray(st))
    outs["device"] = P.decode_device(engine, samples, res, flip=flips, **kw)
    P.assert_rows_equal(outs, ref)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0 and c1["ok"] - c0["ok"] == 2 * len(samples)


# -- 3. lanes --------------------------------------------------------------------------------------------
def _pillow(w, h, seed, **kw):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * (2 + c) + yy * (7 - c) + rng.integers(0, 32, (h, w))) % 256 for c in range(3)], -1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=88, subsampling=2, **kw)
    return buf.getvalue()


def test_a_batch_of_several_lanes_mixing_420_progressive_and_multiscan(engine, refs):
    """512 samples (two kernel lanes of 256): Pillow 4:2:0 files (the baseline entropy kernels), Pillow progressive
    files (k_prog) and multi-scan files (k_scans) side by side; every row equals its own reference."""
    res = (24, 32)
    sizes = [(64, 48), (50, 37), (33, 70), (96, 40), (17, 23), (80, 80)]
    plain = [_pillow(w, h, k) for k, (w, h) in enumerate(sizes)] + \
        [_pillow(w, h, 10 + k, progressive=True) for k, (w, h) in enumerate(sizes)]
    multi = [(d, r) for _, d, r in _under(refs, SCANS) if r.shape[:2] != (1, 1)]  # (a 1 x 1 image has no 4:3 crop)
    distinct = [(d, J.pil_rgb(d)) for d in plain] + multi
    ref1 = [_ref(r, res) for _, r in distinct]
    # every distinct sample at least once, every third sample a Pillow file, the rest drawn from all of them
    order = np.random.default_rng(0).integers(0, len(distinct), 512)
    order[::3] = np.arange(len(order[::3])) % len(plain)
    order[1:3 * len(distinct):3] = np.arange(len(distinct))
    order = [int(o) for o in order]
    assert set(order) == set(range(len(distinct))) and len(distinct) == 12 + 23
    samples = [distinct[o][0] for o in order]
    c0 = engine.counters()
    out, st = engine.decode_resize(samples, res, formats=SCANS)
    assert (np.asarray(st) == 0).all(), np.nonzero(np.asarray(st))[0][:8]
    out = out.cpu().numpy()
    for k, o in enumerate(order):
        np.testing.assert_array_equal(out[k], ref1[o], err_msg=f"row {k} (sample {o})")
    c1 = engine.counters()
    assert c1["ok"] - c0["ok"] == 512 and c1["fallback"] - c0["fallback"] == 0
    assert c1["progressive"] - c0["progressive"] == sum(6 <= o < 12 for o in order)


# -- 4. off by default -----------------------------------------------------------------------------------
def test_nothing_moves_without_the_bit(engine, refs):
    files = [d for _, d, _, _ in refs]
    c0 = engine.counters()
    for fm in (None, ("jpeg",), ("jpeg", "jpeg-ext")):
        _, st = engine.decode_resize(files, (16, 20), formats=fm)
        assert (np.asarray(st) == -2).all(), (fm, st)
    c1 = engine.counters()
    assert c1["ok"] == c0["ok"] and c1["unsupported"] - c0["unsupported"] == 3 * len(files)
    _, st = engine.decode_resize(files, (16, 20), formats=S.SCANS_EXT)  # the mask travels with the call ...
    assert (np.asarray(st) == 0).all()
    _, st = engine.decode_resize(files, (16, 20))  # ... and does not stay behind on the shared engine
    assert (np.asarray(st) == -2).all()
    # the files that need "jpeg-ext" as well stay refused under "jpeg-scans" alone
    both = [d for _, d, _, fm in refs if fm == S.SCANS_EXT]
    _, st = engine.decode_resize(both, (16, 20), formats=SCANS)
    assert (np.asarray(st) == -2).all()
    # a one-scan file decodes to the same pixels under either mask
    single = S.clean()[10][3]
    a, sa = engine.decode_resize([single], (37, 50))
    b, sb = engine.decode_resize([single], (37, 50), formats=SCANS)
    assert sa[0] == 0 and sb[0] == 0
    np.testing.assert_array_equal(a[0].cpu().numpy(), J.pil_rgb(single).transpose(2, 0, 1))
    np.testing.assert_array_equal(b[0].cpu().numpy(), a[0].cpu().numpy())


# -- 5. damage and refusal ---------------------------------------------------------------------------------
DAMAGE = list(S.refused()) + list(S.damaged())


@pytest.mark.parametrize("name,data", DAMAGE, ids=[n for n, _ in DAMAGE])
def test_refused_and_damaged_files_equal_the_default_route(engine, name, data):
    P.check_handover_and_damage(engine, data, SCANS, S.make("420", 13, 7, "y-cbcr", seed=1)[0])
    _, st = engine.decode_resize([data], (16, 20), formats=SCANS)
    if (name, data) in S.refused() or name == "truncated-scan":
        assert st[0] != 0, name


def test_the_device_refuses_what_host_planning_refuses(engine):
    """scans_check (host planning, the probe) and k_scans state the rules of a scan each in its own form: file by
    file, the refused group's status from the device equals sdsj_plan_need_formats', and so does every fixture's."""
    import ctypes

    from sds_amd import _lib as L
    lib = L.load()
    files = [(n, d) for n, d in S.refused()] + [(n, d) for n, d, fm, _ in S.fixtures() if fm == SCANS]
    op = L.SdsjOp(16, 20, 1, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    host = []
    for _, d in files:
        need = ctypes.c_int64(-1)
        host.append(lib.sdsj_plan_need_formats(d, len(d), ctypes.byref(op), 129, ctypes.byref(need)))
    _, dev = P.decode_device(engine, [d for _, d in files], (16, 20), formats=SCANS)
    assert [int(s) for s in dev] == host, [(n, int(a), b) for (n, _), a, b in zip(files, dev, host) if int(a) != b]
    assert all(s != 0 for s in host[:len(S.refused())]) and all(s == 0 for s in host[len(S.refused()):])


@pytest.mark.parametrize("where", [0, 110, 219])
def test_a_refused_file_takes_no_scratch_from_its_batch(where):
    """A batch whose scratch exceeds the engine's 64 MiB floor on a fresh engine, so that the arena is sized to the
    byte from host planning (the host entry point) or from scratch_need (the device-resident one): 219 copies of the
    320 x 240 file and one file k_scans refuses only after k_plan has given it its share.  Every good row decodes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import JpegEngine
    good = next(d for n, d, _, _ in S.clean() if n.startswith("420-320x240"))
    ref = J.pil_rgb(good).transpose(2, 0, 1)
    bad = dict(S.refused())["component-twice"]
    samples = [good] * 219
    samples.insert(where, bad)
    assert JpegEngine.scratch_need(samples, (240, 320), formats=SCANS) > (64 << 20)
    for entry in ("host", "device"):
        eng = JpegEngine("cuda", max_batch=256)  # (fresh: no scratch yet)
        if entry == "host":
            out, st = eng.decode_resize(samples, (240, 320), formats=SCANS)
            out, st = out.cpu().numpy(), np.asarray(st)
        else:
            out, st = P.decode_device(eng, samples, (240, 320), formats=SCANS)
        assert st[where] == -2, (entry, st[where])
        good_rows = [k for k in range(220) if k != where]
        assert (st[good_rows] == 0).all(), (entry, np.nonzero(st)[0])
        for k in (good_rows[0], good_rows[109], good_rows[-1]):
            np.testing.assert_array_equal(out[k], ref, err_msg=f"{entry} row {k}")
        del eng


# -- 6. the per-sample transform -----------------------------------------------------------------------------
def test_need_size_uses_the_probe_under_the_mask(engine):
    """allow_vertical needs the image size before the decode: with "jpeg-scans" a multi-scan file is sized by
    sdsj_probe_formats and decoded natively (no fallback)."""
    from sds_amd.presets import create_standard_image_pipeline
    data = next(d for n, d, _, _ in S.clean() if n.startswith("420-33x70"))
    p = os.path.join(tempfile.mkdtemp(), "x.jpg")
    with open(p, "wb") as f:
        f.write(data)
    c0 = engine.counters()
    kw = dict(device="cuda", service=None, resize_kwargs=dict(allow_vertical=True))
    a = P.run_transforms(create_standard_image_pipeline("jpg", (16, 32), gpu_formats=SCANS, **kw), {"jpg": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("jpg", (16, 32), **kw), {"jpg": p})["image"]
    assert tuple(a.shape) == tuple(b.shape) == (3, 32, 16)
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["ok"] - c0["ok"] == 1 and c1["fallback"] - c0["fallback"] == 0
