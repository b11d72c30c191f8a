"""Four-component JPEG on the GPU (gpu_formats "jpeg-cmyk": k_scans walks the scan or scans of a sequential CMYK / YCCK
file, k_idct<4> and k_cmyk follow) against np.asarray(PIL.Image.open(...).convert("RGB")), bit for bit, and -- for the
multi-scan fixtures -- against PIL's pixels of the same coefficients written as one interleaved scan; for resized
outputs, PIL's pixels through the oracle's crop_box / resize exactly as tests/test_gpu_frames.py::_ref does.

Every fixture must be decoded natively: counters()["ok"] grows by their number and counters()["fallback"] by zero, so
the hand-over to PIL cannot hide a failure.  Without "jpeg-cmyk" the same files report UNSUPPORTED, and for refused
and damaged files the opt-in route must give the same tensor or the same exception type as the default route on the
same bytes.  (The device's status is compared with host planning's on the clean and the refused files; what is wrong
with a damaged file lies in its entropy data, which host planning does not decode.)"""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import gif_synth as GS  # noqa: E402
from tests import goldens as G  # noqa: E402
from tests import jpeg_cmyk_synth as S  # noqa: E402
from tests import jpeg_ext_synth as J  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests import png_synth as PS  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402
from tests.test_gpu_jpeg_ext import _pillow_420  # noqa: E402
from tests.test_gpu_jpeg_scans import GEO  # noqa: E402

CMYK = S.CMYK


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
def test_every_fixture_decodes_to_pils_pixels(engine, refs):
    from sds_amd.batched import GpuDecodeBatch
    assert len(refs) == S.N_FIXTURES == 33
    assert [len(_under(refs, fm)) for fm in (S.CMYK, S.CMYK_SCANS, S.CMYK_EXT)] == [25, 6, 2]
    assert max(r.shape[0] * r.shape[1] for _, _, r, _ in refs) == 320 * 240
    twins = {n: J.pil_rgb(t) for n, _, _, t in S.fixtures() if t is not None}
    assert len(twins) == 6
    c0 = engine.counters()
    for formats in (S.CMYK, S.CMYK_SCANS, S.CMYK_EXT):
        for (h, w), group in P.by_size(_under(refs, formats)).items():
            batch = GpuDecodeBatch("jpg", (h, w), device="cuda", gpu_formats=formats, on_error="raise")(
                {"jpg": [d for _, d, _ in group], "name": [n for n, _, _ in group]})
            img = batch["image"].cpu().numpy()
            assert img.shape == (len(group), 3, h, w)
            for k, (n, _, ref) in enumerate(group):
                np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=n)
                if n in twins:
                    np.testing.assert_array_equal(img[k], twins[n].transpose(2, 0, 1), err_msg=n + " (one scan)")
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == len(refs)
    assert c1["progressive"] == c0["progressive"]  # (the counter keeps counting SOF2 files only)


def test_the_g6_cmyk_file_decodes_to_the_goldens_outputs(engine):
    """jpeg_cmyk_48x32 of tests/golden/g6_fallback (the reference pipeline's outputs for it), decoded natively."""
    meta = G.load_json("g6_fallback.json")
    z = np.load(os.path.join(G.GOLDEN, "g6_fallback.npz"))
    data = z["jpeg_cmyk_48x32__bytes"].tobytes()
    c0 = engine.counters()
    seen = 0
    for vname, res, kw in meta["variants"]:
        if f"jpeg_cmyk_48x32__{vname}" not in z.files:  # (the float variants are stored as hashes only)
            continue
        rk = dict(kw.get("resize_kwargs", {}))
        out, st = engine.decode_resize([data], tuple(res), crop_before_resize=rk.get("crop_before_resize", True), formats=CMYK)
        assert st[0] == 0, vname
        np.testing.assert_array_equal(out[0].cpu().numpy(), z[f"jpeg_cmyk_48x32__{vname}"], err_msg=vname)
        seen += 1
    c1 = engine.counters()
    assert seen >= 2 and c1["ok"] - c0["ok"] == seen and c1["fallback"] - c0["fallback"] == 0


# -- 2. geometry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", GEO, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_resized_outputs_through_both_entry_points(engine, refs, cfg):
    """Eight samples on the host entry point: latency mode; the device-resident entry point plans them as a batch."""
    res, filt, crop = cfg["res"], cfg.get("filt", "bilinear"), cfg.get("crop", True)
    flip, normalize, layout = cfg.get("flip", False), cfg.get("normalize", False), cfg.get("layout", "chw")
    picked = [(n, d, r) for n, d, r in _under(refs, CMYK) if r.shape[:2] in ((37, 50), (70, 33))][:8]
    assert len(picked) == 8 and len({r.shape for _, _, r in picked}) == 2
    samples = [d for _, d, _ in picked]
    flips = [flip and k % 3 != 1 for k in range(len(picked))]
    ref = []
    for (_, _, r), f in zip(picked, flips):
        chw = _ref(r, res, filt, crop=crop, flip=f, normalize=normalize)
        ref.append(chw.transpose(1, 2, 0) if layout == "hwc" else chw)
    kw = dict(filter=filt, crop_before_resize=crop, normalize=normalize, layout=layout, formats=CMYK)
    c0 = engine.counters()
    outs = {}
    out, st = engine.decode_resize(samples, res, flip=flips, **kw)
    outs["host"] = (out.cpu().numpy(), np.asarray(st))
    outs["device"] = P.decode_device(engine, samples, res, flip=flips, **kw)
    P.assert_rows_equal(outs, ref)
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0 and c1["ok"] - c0["ok"] == 2 * len(samples)


# -- 3. lanes --------------------------------------------------------------------------------------------
def test_a_batch_of_several_lanes_mixing_420_png_gif_and_cmyk(engine, refs):
    """512 samples (two kernel lanes of 256) under ("jpeg", "png", "gif", "jpeg-cmyk"): Pillow 4:2:0 files, which keep
    the fused kernels, and PNGs, GIFs and CMYK / YCCK files, which share the unfused ones; every row equals its own
    reference."""
    res = (24, 32)
    sizes = [(64, 48), (50, 37), (33, 70), (96, 40), (17, 23), (80, 80)]
    jpgs = [_pillow_420(w, h, k) for k, (w, h) in enumerate(sizes)]
    pngs = [PS.make(w, h, ct, seed=k) for k, ((w, h), ct) in enumerate(zip(sizes, (0, 2, 3, 4, 6, 2)))]
    t = GS.colour_table(256, 11)
    gifs = [GS.write_gif((w, h), GS.indices(w, h, 256, 3 * w + h, smooth=False), gct=t, interlace=bool(k & 1))
            for k, (w, h) in enumerate(sizes[:4])]
    cmyk = [(d, r) for _, d, r in _under(refs, CMYK)]
    distinct = [(d, PS.pil_rgb(d)) for d in jpgs + pngs + gifs] + cmyk
    ref1 = [_ref(r, res) for _, r in distinct]
    order = np.random.default_rng(0).integers(0, len(distinct), 512)
    order[::3] = np.arange(len(order[::3])) % len(jpgs)
    order[1:3 * len(distinct):3] = np.arange(len(distinct))
    order = [int(o) for o in order]
    assert set(order) == set(range(len(distinct))) and len(distinct) == 16 + 25
    samples = [distinct[o][0] for o in order]
    c0 = engine.counters()
    out, st = engine.decode_resize(samples, res, formats=("jpeg", "png", "gif", "jpeg-cmyk"))
    assert (np.asarray(st) == 0).all(), np.nonzero(np.asarray(st))[0][:8]
    out = out.cpu().numpy()
    for k, o in enumerate(order):
        np.testing.assert_array_equal(out[k], ref1[o], err_msg=f"row {k} (sample {o})")
    c1 = engine.counters()
    assert c1["ok"] - c0["ok"] == 512 and c1["fallback"] - c0["fallback"] == 0


# -- 4. off by default -----------------------------------------------------------------------------------
def test_nothing_moves_without_the_bit(engine, refs):
    files = [d for _, d, _, _ in refs]
    c0 = engine.counters()
    for fm in (None, ("jpeg",), ("jpeg", "jpeg-ext", "jpeg-scans")):
        _, st = engine.decode_resize(files, (16, 20), formats=fm)
        assert (np.asarray(st) == -2).all(), (fm, st)
        _, st = P.decode_device(engine, files, (16, 20), formats=fm)
        assert (np.asarray(st) == -2).all(), (fm, st)
    c1 = engine.counters()
    assert c1["ok"] == c0["ok"] and c1["unsupported"] - c0["unsupported"] == 6 * len(files)
    _, st = engine.decode_resize(files, (16, 20), formats=S.CMYK_SCANS + ("jpeg-ext",))  # the mask travels with the call ...
    assert (np.asarray(st) == 0).all()
    _, st = engine.decode_resize(files, (16, 20))  # ... and does not stay behind on the shared engine
    assert (np.asarray(st) == -2).all()
    # the files that need a second bit stay refused under "jpeg-cmyk" alone
    both = [d for _, d, _, fm in refs if fm != CMYK]
    _, st = engine.decode_resize(both, (16, 20), formats=CMYK)
    assert len(both) == 8 and (np.asarray(st) == -2).all()


def test_the_per_sample_transform_without_the_bit_is_the_default_routes(engine, refs):
    """Without the name a CMYK file reruns on PIL as before; with it the same tensor comes from the native route."""
    from sds_amd.presets import create_standard_image_pipeline
    data = next(d for n, d, _, _ in refs if n == "ycck-photoshop-50x37")
    p = os.path.join(tempfile.mkdtemp(), "x.jpg")
    with open(p, "wb") as f:
        f.write(data)
    kw = dict(device="cuda", service=None)
    c0 = engine.counters()
    a = P.run_transforms(create_standard_image_pipeline("jpg", (16, 20), **kw), {"jpg": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("jpg", (16, 20), gpu_formats=CMYK, **kw), {"jpg": p})["image"]
    c2 = engine.counters()
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    np.testing.assert_array_equal(b.cpu().numpy(), _ref(J.pil_rgb(data), (16, 20)))
    assert c1["fallback"] - c0["fallback"] == 1 and c2["fallback"] == c1["fallback"] and c2["ok"] - c1["ok"] == 1


# -- 5. damage and refusal ---------------------------------------------------------------------------------
DAMAGE = [(n, d, fm) for n, d, fm, _ in S.refused()] + [(n, d, CMYK) for n, d, _ in S.damaged()]


@pytest.mark.parametrize("name,data,formats", DAMAGE, ids=[n for n, _, _ in DAMAGE])
def test_refused_and_damaged_files_equal_the_default_route(engine, name, data, formats):
    P.check_handover_and_damage(engine, data, formats, S.fixtures()[0][1])
    _, st = engine.decode_resize([data], (16, 20), formats=formats)
    if name in [n for n, _, _, _ in S.refused()] or name in ("truncated-scan", "bad-dht"):
        assert st[0] != 0, name


def test_the_device_refuses_what_host_planning_refuses(engine):
    """File by file, the refused group's status from the device equals sdsj_plan_need_formats', and so does every
    clean fixture's, each under its own mask."""
    import ctypes

    from sds_amd import _lib as L
    lib = L.load()
    files = [(n, d, fm) for n, d, fm, _ in S.refused()] + [(n, d, fm) for n, d, fm, _ in S.fixtures()]
    op = L.SdsjOp(16, 20, 1, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    host, dev = [], []
    for _, d, fm in files:
        need = ctypes.c_int64(-1)
        host.append(lib.sdsj_plan_need_formats(d, len(d), ctypes.byref(op), L.format_mask(fm), ctypes.byref(need)))
    for fm in sorted({fm for _, _, fm in files}):
        idx = [k for k, f in enumerate(files) if f[2] == fm]
        _, st = P.decode_device(engine, [files[k][1] for k in idx], (16, 20), formats=fm)
        dev += [(k, int(s)) for k, s in zip(idx, st)]
    dev = [s for _, s in sorted(dev)]
    assert dev == host, [(f[0], a, b) for f, a, b in zip(files, dev, host) if a != b]
    nref = len(S.refused())
    assert all(s != 0 for s in host[:nref]) and all(s == 0 for s in host[nref:])


@pytest.mark.parametrize("where", [0, 110, 219])
def test_a_refused_file_takes_no_scratch_from_its_batch(where):
    """A batch whose scratch exceeds the engine's 64 MiB floor on a fresh engine, so that the arena is sized to the
    byte from host planning (the host entry point) or from scratch_need (the device-resident one): 219 copies of the
    320 x 240 file and one file the header refuses.  Every good row decodes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import JpegEngine
    good = next(d for n, d, _, _ in S.fixtures() if n == "pil-ss2-320x240")
    ref = J.pil_rgb(good).transpose(2, 0, 1)
    bad = next(d for n, d, _, _ in S.refused() if n == "sixteen-blocks")
    samples = [good] * 219
    samples.insert(where, bad)
    assert JpegEngine.scratch_need(samples, (240, 320), formats=CMYK) > (64 << 20)
    for entry in ("host", "device"):
        eng = JpegEngine("cuda", max_batch=256)  # (fresh: no scratch yet)
        if entry == "host":
            out, st = eng.decode_resize(samples, (240, 320), formats=CMYK)
            out, st = out.cpu().numpy(), np.asarray(st)
        else:
            out, st = P.decode_device(eng, samples, (240, 320), formats=CMYK)
        assert st[where] == -3, (entry, st[where])
        good_rows = [k for k in range(220) if k != where]
        assert (st[good_rows] == 0).all(), (entry, np.nonzero(st)[0])
        for k in (good_rows[0], good_rows[109], good_rows[-1]):
            np.testing.assert_array_equal(out[k], ref, err_msg=f"{entry} row {k}")
        del eng
