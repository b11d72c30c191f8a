"""The wider opt-in PNG subset on the GPU (gpu_formats "png-ext": k_png_inflate with the pass layout,
k_png_unfilter_ext) against np.asarray(PIL.Image.open(...).convert("RGB")) -- PNG is lossless, so PIL is the
reference -- and, for resized outputs, PIL's pixels through the oracle's crop_box / resize exactly as
tests/test_gpu_frames.py::_ref does, as tests/test_gpu_png.py compares the base subset.

Every sample of the Adam7, low-depth, 16-bit and ancillary-chunk groups must be decoded natively:
counters()["png"] grows by their number and counters()["fallback"] by zero, so the hand-over to PIL cannot
hide a failure.  Without "png-ext" the same files report UNSUPPORTED, and for damaged streams the opt-in
route must give the same tensor or the same exception type as the default route on the same bytes."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import goldens as G  # noqa: E402
from tests import png_ext_synth as E  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests import png_synth as S  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402

EXT = ("jpeg", "png-ext")
BOTH = ("jpeg", "png")


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def refs():
    """PIL's pixels of every native-group sample, computed once."""
    cases = {"adam7": E.group_adam7_8bit(), "low": E.group_low_depth(), "d16": E.group_depth16(), "chunks": E.group_chunks()}
    return {g: [(n, d, S.pil_rgb(d)) for n, d in c] for g, c in cases.items()}


def test_adam7_8bit_every_colour_type_and_size(engine, refs):
    assert len(refs["adam7"]) == 5 * len(E.ADAM7_SIZES)
    P.decode_group_natively(engine, refs["adam7"], EXT)


def test_depths_1_2_4_gray_and_palette(engine, refs):
    assert len(refs["low"]) == 2 * 3 * len(E.LOW_WIDTHS) * len(E.LOW_HEIGHTS) * 2 + 4
    P.decode_group_natively(engine, refs["low"], EXT)


def test_depth_16(engine, refs):
    assert len(refs["d16"]) == 4 * 3 * 2 * 2
    P.decode_group_natively(engine, refs["d16"], EXT)


def test_ancillary_chunks_before_the_image_data(engine, refs):
    assert len(refs["chunks"]) == len(E.ANCILLARY) + 1
    P.decode_group_natively(engine, refs["chunks"], EXT)


@pytest.mark.parametrize("res,filt,crop", [((24, 40), "bilinear", True), ((150, 90), "bicubic", False)])
def test_resized_outputs_join_the_resample_passes(engine, refs, res, filt, crop):
    """With the crop on, the crop of the taller cases starts inside the image and ends above its last row: the
    rows below are skipped in every pass."""
    cases = [c for g in ("adam7", "low", "d16", "chunks") for c in refs[g] if min(c[2].shape[:2]) >= 5]
    assert any(c[2].shape[0] > 100 for c in cases)
    c0 = engine.counters()
    out, status = engine.decode_resize([d for _, d, _ in cases], res, filter=filt, crop_before_resize=crop, formats=EXT)
    assert (status == 0).all(), [cases[i][0] for i in np.nonzero(status)[0]]
    out = out.cpu().numpy()
    for k, (n, _, ref) in enumerate(cases):
        np.testing.assert_array_equal(out[k], _ref(ref, res, filt, crop=crop), err_msg=n)
    c1 = engine.counters()
    assert c1["png"] - c0["png"] == len(cases) and c1["fallback"] - c0["fallback"] == 0


# -- entry points and mixing -------------------------------------------------------------------------
def _mixed():
    """16 samples: G2 JPEGs, PNGs of the base subset and of the wider one, interleaved."""
    _, jpgs = G.g2_jpegs()
    base = [S.make(67, 50, 2, "mixP", seed=1), S.make(64, 65, 3, "mixA", seed=2, plte_n=200), S.make(200, 129, 6, "mixU", seed=3),
            S.make(90, 120, 2, "all4", seed=4)]
    ext = [E.make(200, 129, 2, 8, 1, E.PASS_SCHEDULES, seed=1)[0], E.make(67, 65, 3, 4, 0, "mixP", seed=2, plte_n=11)[0],
           E.make(64, 65, 6, 16, 1, "mixA", seed=3)[0], E.make(131, 90, 0, 1, 1, "mixU", seed=4)[0],
           E.make(90, 131, 0, 16, 0, "all4", seed=5)[0], E.make(9, 131, 4, 8, 1, "mixP", seed=6)[0],
           E.make(67, 5, 3, 2, 1, "all3", seed=7)[0], E.make(48, 48, 2, 16, 1, "all4", seed=8, pre=E.ANCILLARY)[0]]
    samples = [jpgs[0], base[0], ext[0], ext[1], jpgs[1], base[1], ext[2], ext[3], jpgs[2], base[2], ext[4], ext[5],
               jpgs[3], base[3], ext[6], ext[7]]
    is_png = [s[:8] == S.SIG for s in samples]
    assert sum(is_png) == 12
    return samples, is_png


_MIXED_REFS = {}  # (the lanes parameter repeats the configuration: one reference)


def _mixed_ref(samples, is_png, res, filt, flips, normalize, layout):
    key = (res, filt, tuple(flips), normalize, layout)
    if key not in _MIXED_REFS:
        out = []
        for s, p, f in zip(samples, is_png, flips):
            chw = _ref(S.pil_rgb(s), res, filt, flip=f, normalize=normalize) if p else \
                O.pipeline(s, res, crop_before_resize=True, filter=filt, flip=f, normalize=normalize)
            out.append(chw.transpose(1, 2, 0) if layout == "hwc" else chw)
        _MIXED_REFS[key] = np.stack(out)
    return _MIXED_REFS[key]


@pytest.mark.parametrize("lanes", [1, 4])
def test_mixed_batch_through_every_entry_point(engine, lanes):
    res, filt, normalize, layout = (96, 64), "bicubic", True, "hwc"
    samples, is_png = _mixed()
    n = len(samples)
    flips = [bool(i % 3 != 1) for i in range(n)]
    ref = _mixed_ref(samples, is_png, res, filt, flips, normalize, layout)
    kw = dict(filter=filt, normalize=normalize, layout=layout, formats=EXT)
    engine.set_lanes(lanes)
    try:
        c0 = engine.counters()
        outs = {}
        out, st = engine.decode_resize(samples, res, flip=flips, **kw)
        outs["host"] = (out.cpu().numpy(), np.asarray(st))
        outs["device"] = P.decode_device(engine, samples, res, flip=flips, **kw)
        tmp = tempfile.mkdtemp()
        paths = []
        for i, s in enumerate(samples):
            paths.append(os.path.join(tmp, f"{i}.bin"))
            with open(paths[-1], "wb") as f:
                f.write(s)
        engine.submit(0, samples, res, flip=flips, **kw)
        engine.submit(1, paths, res, files=True, flip=flips, **kw)
        for slot, name in ((0, "submit0"), (1, "files1")):
            out, st = engine.wait(slot)
            outs[name] = (out.cpu().numpy(), np.asarray(st))
        P.assert_rows_equal(outs, ref)
        c1 = engine.counters()
        assert c1["png"] - c0["png"] == len(outs) * sum(is_png)
        assert c1["fallback"] - c0["fallback"] == 0
    finally:
        engine.set_lanes(4)


# -- off by default ------------------------------------------------------------------------------------
def test_the_wider_subset_is_off_by_default(engine):
    files = [E.make(13, 7, 2, 8, 1)[0], E.make(13, 7, 0, 4, 0)[0], E.make(13, 7, 6, 16, 0)[0], E.with_chunk(*E.ANCILLARY[0])]
    c0 = engine.counters()
    for fm in (BOTH, ("jpeg",), None):
        _, st = engine.decode_resize(files, (7, 13), formats=fm)
        assert (np.asarray(st) == -2).all(), (fm, st)
    c1 = engine.counters()
    assert c1["png"] == c0["png"] and c1["unsupported"] - c0["unsupported"] == 3 * len(files)
    out, st = engine.decode_resize(files, (7, 13), formats=EXT)  # the mask travels with the call ...
    assert (np.asarray(st) == 0).all()
    for k, f in enumerate(files):
        np.testing.assert_array_equal(out[k].cpu().numpy(), S.pil_rgb(f).transpose(2, 0, 1))
    assert engine.counters()["png"] - c1["png"] == len(files)
    _, st = engine.decode_resize(files, (7, 13), formats=BOTH)  # ... and does not stay behind on the shared engine
    assert (np.asarray(st) == -2).all()
    _, st = engine.decode_resize(files, (7, 13))
    assert (np.asarray(st) == -2).all()


def test_the_bit_alone_is_refused_by_a_live_engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd import _lib as L
    from sds_amd.engine import JpegEngine
    eng = JpegEngine("cuda", max_batch=4)
    lib = L.load()
    for mask in (L.FORMAT_PNG_EXT, L.FORMAT_JPEG | L.FORMAT_PNG_EXT, 8):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.EINVAL
    assert lib.sdsj_engine_set_formats(eng._h, L.FORMAT_JPEG | L.FORMAT_PNG | L.FORMAT_PNG_EXT) == L.OK
    assert lib.sdsj_engine_set_formats(eng._h, L.FORMAT_PNG | L.FORMAT_PNG_EXT) == L.OK
    assert lib.sdsj_engine_set_formats(eng._h, L.FORMAT_JPEG) == L.OK


def test_need_size_uses_the_probe_under_the_mask(engine):
    """allow_vertical needs the image size before the decode: with "png-ext" an interlaced file is sized by
    sdsj_png_probe_formats and decoded natively (no fallback)."""
    from sds_amd.presets import create_standard_image_pipeline
    data = E.make(40, 90, 6, 16, 1, "mixP")[0]
    p = os.path.join(tempfile.mkdtemp(), "x.png")
    with open(p, "wb") as f:
        f.write(data)
    c0 = engine.counters()
    kw = dict(device="cuda", service=None, resize_kwargs=dict(allow_vertical=True))
    a = P.run_transforms(create_standard_image_pipeline("png", (16, 32), gpu_formats=EXT, **kw), {"png": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("png", (16, 32), **kw), {"png": p})["image"]
    assert tuple(a.shape) == tuple(b.shape) and a.shape[0] == 3
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["png"] - c0["png"] == 1 and c1["fallback"] - c0["fallback"] == 0


# -- hand-over and damage ----------------------------------------------------------------------------
DAMAGE = S.group_damage() + E.group_ext_damage()


@pytest.mark.parametrize("name,data", DAMAGE, ids=[n for n, _ in DAMAGE])
def test_handover_and_damage_equal_the_default_route(engine, name, data):
    P.check_handover_and_damage(engine, data, EXT, E.make(13, 7, 2, 8, 1, "mixP")[0])


def test_damage_split_follows_pil(engine):
    """Which damaged inputs PIL accepts is asked of PIL here, not written down: every input it rejects is
    refused natively, and at least one accepted and one rejected input exist, so both branches ran.  The files
    of S.group_damage() that are merely outside the base subset (interlaced, depths 1 / 2 / 4 / 16) are now
    decoded natively wherever PIL accepts them."""
    kinds = {n: S.pil_outcome(d)[0] for n, d in DAMAGE}
    assert "ok" in kinds.values() and "err" in kinds.values()
    _, st = engine.decode_resize([d for _, d in DAMAGE], (16, 20), formats=EXT)
    for (n, _), s in zip(DAMAGE, st):
        if kinds[n] == "err":
            assert s != 0, n
        assert s in (0, -2, -3), (n, s)
    by_name = dict(zip([n for n, _ in DAMAGE], st))
    for n in ("depth16", "depth1", "depth2", "depth4"):
        assert kinds[n] == "ok" and by_name[n] == 0, n
