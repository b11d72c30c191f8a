"""Progressive four-component JPEG on the GPU (gpu_formats "jpeg-cmyk-prog": k_prog4 walks every scan of a SOF2 CMYK /
YCCK file, k_prog4_dcs / k_prog4_smooth smooth the blocks of a file that ends early, k_idct<4> and k_cmyk follow) against
np.asarray(PIL.Image.open(...).convert("RGB")), bit for bit; for resized outputs, PIL's pixels through the oracle's
crop_box / resize exactly as tests/test_gpu_frames.py::_ref does.

Every clean and every cut fixture must be decoded natively: counters()["ok"] and ["progressive"] grow by their number and
["fallback"] by zero, so the hand-over to PIL cannot hide a failure.  Without the name the same files report UNSUPPORTED
(tests/test_gpu_jpeg_cmyk.py pins that for the masks that existed before), and for refused and truncated files the
opt-in route must give the same tensor or the same exception type as the default route on the same bytes."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import jpeg_cmyk_prog_synth as PS  # noqa: E402
from tests import jpeg_cmyk_synth as S  # noqa: E402
from tests import jpeg_ext_synth as J  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402
from tests.test_gpu_jpeg_ext import _pillow_420  # noqa: E402

RES = (16, 20)


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def refs():
    """(name, bytes, PIL's pixels, gpu_formats) of every clean fixture, computed once."""
    return [(n, d, J.pil_rgb(d), fm) for n, d, fm, _ in PS.clean()]


def _want(ref, res, crop):
    """_ref, or zeros where the centre crop is empty (the 1 x 1 file: the pipeline's output for an empty crop)."""
    if crop and (ref.shape[1], ref.shape[0]) != (res[1], res[0]):
        l, t, r, b = O.crop_box(ref.shape[1], ref.shape[0], res[0], res[1])
        if r <= l or b <= t:
            return np.zeros((3,) + tuple(res), np.uint8)
    return _ref(ref, res, crop=crop)


def _resized(engine, group, formats, c0_ok):
    """The group at RES with and without the centre crop, CHW and HWC; returns the number of samples decoded."""
    samples = [d for _, d, _ in group]
    seen = 0
    for crop, layout in ((True, "chw"), (False, "chw"), (True, "hwc")):
        out, st = engine.decode_resize(samples, RES, crop_before_resize=crop, layout=layout, formats=formats)
        assert (np.asarray(st) == 0).all(), (crop, layout, [n for (n, _, _), s in zip(group, st) if s != 0])
        out = out.cpu().numpy()
        for k, (n, _, ref) in enumerate(group):
            want = _want(ref, RES, crop)
            np.testing.assert_array_equal(out[k], want.transpose(1, 2, 0) if layout == "hwc" else want,
                                          err_msg=f"{n} crop={crop} {layout}")
        seen += len(samples)
    return seen


# -- 1. the clean fixtures ---------------------------------------------------------------------------------
def test_every_clean_fixture_decodes_to_pils_pixels(engine, refs):
    from sds_amd.batched import GpuDecodeBatch
    assert len(refs) == PS.N_CLEAN == 32
    assert max(r.shape[0] * r.shape[1] for _, _, r, _ in refs) == 130 * 70
    c0 = engine.counters()
    n = 0
    for formats in (PS.PROG, PS.PROG_EXT):
        under = [(nm, d, r) for nm, d, r, fm in refs if fm == formats]
        for (h, w), group in P.by_size(under).items():  # full resolution: the decode alone
            samples = [d for _, d, _ in group]
            batch = GpuDecodeBatch("jpg", (h, w), device="cuda", gpu_formats=formats, on_error="raise")({"jpg": samples})
            img = batch["image"].cpu().numpy()
            assert img.shape == (len(group), 3, h, w)
            out, st = engine.decode_resize(samples, (h, w), layout="hwc", formats=formats)
            assert (np.asarray(st) == 0).all()
            hwc = out.cpu().numpy()
            for k, (nm, _, ref) in enumerate(group):
                np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=nm)
                np.testing.assert_array_equal(hwc[k], ref, err_msg=nm + " hwc")
            n += 2 * len(group)
        n += _resized(engine, under, formats, c0)
    c1 = engine.counters()
    assert n == 5 * len(refs)
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == n
    assert c1["progressive"] - c0["progressive"] == n  # (SOF2 files: the counter counts them too)


# -- 2. files that end early: block smoothing of four components ----------------------------------------------
def test_files_cut_between_and_inside_scans_equal_pil(engine):
    """The 34 files cut before scan j + 1 and the four cut in the middle of a scan, all with EOI: libjpeg smooths
    the blocks of every component, K included, and uses the previous scan's bits in the iMCU rows past the data."""
    fx = PS.end_cuts() + PS.mid_cuts_eoi()
    assert len(fx) == 34 + 4
    group = [(n, d, J.pil_rgb(d)) for n, d, _, _ in fx]
    assert {r.shape for _, _, r in group} == {(37, 50, 3)}
    whole = {src: J.pil_rgb(PS._pil(src)) for src in PS.CUT_SOURCES}
    assert all(not np.array_equal(r, whole[n.rsplit("-", 1)[0]]) for n, _, r in group if "-first" in n)
    c0 = engine.counters()
    out, st = engine.decode_resize([d for _, d, _ in group], (37, 50), layout="hwc", formats=PS.PROG)
    assert (np.asarray(st) == 0).all(), [n for (n, _, _), s in zip(group, st) if s != 0]
    out = out.cpu().numpy()
    bad = [n for k, (n, _, ref) in enumerate(group) if not np.array_equal(out[k], ref)]
    assert not bad, bad
    out, st = P.decode_device(engine, [d for _, d, _ in group], (37, 50), formats=PS.PROG, layout="hwc")
    assert (st == 0).all()
    bad = [n for k, (n, _, ref) in enumerate(group) if not np.array_equal(out[k], ref)]
    assert not bad, bad
    c1 = engine.counters()
    assert c1["fallback"] - c0["fallback"] == 0 and c1["ok"] - c0["ok"] == 2 * len(group)
    assert c1["progressive"] - c0["progressive"] == 2 * len(group)


MID = [(n, d) for n, d, _, _ in PS.mid_cuts()]


@pytest.mark.parametrize("name,data", MID, ids=[n for n, _ in MID])
def test_a_file_that_ends_inside_a_scan_is_the_default_routes_error(engine, name, data):
    P.check_handover_and_damage(engine, data, PS.PROG, PS.clean()[0][1])
    _, st = engine.decode_resize([data], RES, formats=PS.PROG)
    assert st[0] != 0, name


# -- 3. a mixed batch ------------------------------------------------------------------------------------------
def test_a_mixed_batch_under_every_jpeg_bit(engine, refs):
    """Mask 1537 + 64 + 128: progressive CMYK / YCCK beside sequential CMYK in one scan and in several, baseline
    4:2:0, progressive three-component, gray and a refused file; each row equals its own reference."""
    prog4 = [d for n, d, _, _ in refs if n in ("pil-ss2-q95-50x37", "ycck2-ss1-50x37", "w-photoshop-50x37", "w-411-50x37",
                                              "w-dri3-first-17x23", "pil-rst-blocks-130x70")]
    cut = [PS.end_cuts()[4][1], PS.mid_cuts_eoi()[3][1]]
    seq4 = [S.pillow_files()[1][1], S.writer_files()[5][1]] + [S.multiscan_files()[k][1] for k in (0, 1)]
    plain = [_pillow_420(64, 48, 1), _pillow_420(50, 37, 2), J._pillow(50, 37, 3, progressive=True, quality=85),
             J._pillow(33, 70, 4, progressive=True, subsampling=2), J._pillow(50, 37, 5, mode="L"),
             J._pillow(17, 23, 6, mode="L", progressive=True)]
    refused = PS.refused()[1][1]
    assert len(prog4) == 6
    distinct = prog4 + cut + seq4 + plain
    ref1 = [_ref(J.pil_rgb(d), (24, 32)) for d in distinct]
    order = [int(o) for o in np.random.default_rng(0).permutation(np.arange(3 * len(distinct)) % len(distinct))]
    samples = [distinct[o] for o in order]
    samples.insert(7, refused)
    c0 = engine.counters()
    for entry in ("host", "device"):
        if entry == "host":
            out, st = engine.decode_resize(samples, (24, 32), formats=PS.MIXED)
            out, st = out.cpu().numpy(), np.asarray(st)
        else:
            out, st = P.decode_device(engine, samples, (24, 32), formats=PS.MIXED)
        assert st[7] == -2 and (np.delete(st, 7) == 0).all(), (entry, st)
        assert not out[7].any()
        for k, o in enumerate(order):
            np.testing.assert_array_equal(out[k + (k >= 7)], ref1[o], err_msg=f"{entry} row {k} (sample {o})")
    c1 = engine.counters()
    assert c1["ok"] - c0["ok"] == 2 * len(order) and c1["fallback"] - c0["fallback"] == 0
    assert c1["progressive"] - c0["progressive"] == 2 * 3 * (len(prog4) + len(cut) + 3)


# -- 4. refusal ------------------------------------------------------------------------------------------------
REFUSED = [(n, d, fm) for n, d, fm, _ in PS.refused()]


@pytest.mark.parametrize("name,data,formats", REFUSED, ids=[n for n, _, _ in REFUSED])
def test_refused_files_equal_the_default_route(engine, name, data, formats):
    P.check_handover_and_damage(engine, data, formats, PS.clean()[0][1])
    _, st = engine.decode_resize([data], RES, formats=formats)
    assert st[0] == (-3 if name == "sixteen-blocks" else -2), name


def test_the_device_refuses_what_host_planning_refuses(engine):
    """File by file, the device's status equals sdsj_plan_need_formats': the refused group, every clean fixture and
    every cut with EOI, each under its own mask and under "jpeg-cmyk-prog" alone."""
    from sds_amd import _lib as L
    lib = L.load()
    files = [(n, d, fm) for n, d, fm, _ in PS.refused() + PS.clean() + PS.end_cuts() + PS.mid_cuts_eoi()]
    files += [(n, d, PS.PROG) for n, d, fm, _ in PS.clean() if fm != PS.PROG]
    op = L.SdsjOp(RES[0], RES[1], 1, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    host, dev = [], []
    for _, d, fm in files:
        need = ctypes.c_int64(-1)
        host.append(lib.sdsj_plan_need_formats(d, len(d), ctypes.byref(op), L.format_mask(fm), ctypes.byref(need)))
    for fm in sorted({fm for _, _, fm in files}):
        idx = [k for k, f in enumerate(files) if f[2] == fm]
        _, st = P.decode_device(engine, [files[k][1] for k in idx], RES, formats=fm)
        dev += [(k, int(s)) for k, s in zip(idx, st)]
    dev = [s for _, s in sorted(dev)]
    assert dev == host, [(f[0], a, b) for f, a, b in zip(files, dev, host) if a != b]
    assert host[:2] == [-3, -2] and all(s == 0 for s in host[2:-1]) and host[-1] == -2


# -- 5. the engine's entry points ----------------------------------------------------------------------------
def test_set_formats_follows_the_mask_table():
    from sds_amd import _lib as L
    from sds_amd.engine import JpegEngine
    from tests.test_jpeg_cmyk_prog_host import INVALID, VALID
    eng = JpegEngine("cuda", max_batch=8)
    lib = L.load()
    for mask in INVALID:
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.EINVAL, mask
    for mask in VALID:
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.OK, mask
    assert lib.sdsj_engine_set_formats(eng._h, 1) == L.OK
    del eng


def test_the_device_entry_equals_the_host_entry(engine, refs):
    picked = [(n, d, r) for n, d, r, fm in refs if fm == PS.PROG and r.shape[:2] in ((37, 50), (23, 17))]
    assert len(picked) >= 8
    samples = [d for _, d, _ in picked]
    for res, kw in (((16, 20), {}), ((40, 90), dict(filter="bicubic", crop_before_resize=False)),
                    ((16, 20), dict(normalize=True))):
        ref = [_ref(r, res, kw.get("filter", "bilinear"), crop=kw.get("crop_before_resize", True),
                    normalize=kw.get("normalize", False)) for _, _, r in picked]
        out, st = engine.decode_resize(samples, res, formats=PS.PROG, **kw)
        outs = {"host": (out.cpu().numpy(), np.asarray(st)), "device": P.decode_device(engine, samples, res, formats=PS.PROG, **kw)}
        P.assert_rows_equal(outs, ref)


def test_the_transform_and_the_batch_decode_natively_only_under_the_name(engine, refs):
    """Under ("jpeg-cmyk-prog",) a progressive CMYK sample decodes natively (fallback +0); under ("jpeg-cmyk",) the
    same sample reruns on PIL (fallback +1); the pixels are equal."""
    from sds_amd.batched import GpuDecodeBatch
    from sds_amd.presets import create_standard_image_pipeline
    data = next(d for n, d, _, _ in refs if n == "pil-ss2-q95-50x37")
    want = _ref(J.pil_rgb(data), RES)
    p = os.path.join(tempfile.mkdtemp(), "x.jpg")
    with open(p, "wb") as f:
        f.write(data)
    kw = dict(device="cuda", service=None)
    c0 = engine.counters()
    a = P.run_transforms(create_standard_image_pipeline("jpg", RES, gpu_formats=PS.PROG, **kw), {"jpg": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("jpg", RES, gpu_formats=S.CMYK, **kw), {"jpg": p})["image"]
    c2 = engine.counters()
    np.testing.assert_array_equal(a.cpu().numpy(), want)
    np.testing.assert_array_equal(b.cpu().numpy(), want)
    assert c1["fallback"] == c0["fallback"] and c1["ok"] - c0["ok"] == 1 and c1["progressive"] - c0["progressive"] == 1
    # (the rerun: the device refuses the sample, PIL decodes it, the GPU resizes PIL's frame)
    assert c2["fallback"] - c1["fallback"] == 1 and c2["unsupported"] - c1["unsupported"] == 1
    assert c2["progressive"] == c1["progressive"] and c1["unsupported"] == c0["unsupported"]
    a = GpuDecodeBatch("jpg", RES, device="cuda", gpu_formats=PS.PROG)({"jpg": [data, data]})["image"]
    c3 = engine.counters()
    b = GpuDecodeBatch("jpg", RES, device="cuda", gpu_formats=S.CMYK)({"jpg": [data, data]})["image"]
    c4 = engine.counters()
    for row in list(a.cpu().numpy()) + list(b.cpu().numpy()):
        np.testing.assert_array_equal(row, want)
    assert c3["fallback"] == c2["fallback"] and c3["ok"] - c2["ok"] == 2 and c3["progressive"] - c2["progressive"] == 2
    assert c4["fallback"] - c3["fallback"] == 2 and c4["unsupported"] - c3["unsupported"] == 2
    assert c4["progressive"] == c3["progressive"] and c3["unsupported"] == c2["unsupported"]
