"""The opt-in native PNG path on the GPU (k_png_inflate, k_png_unfilter) against
np.asarray(PIL.Image.open(...).convert("RGB")) -- PNG is lossless, so PIL is the reference -- and, for
resized outputs, PIL's pixels through the oracle's crop_box / resize exactly as
tests/test_gpu_frames.py::_ref does.  A target equal to the image size compares the decode alone.

Every sample of the colour-type, deflate-structure, size and mixed-batch groups must be decoded
natively: counters()["png"] grows by their number and counters()["fallback"] by zero, so the hand-over
to PIL cannot hide a failure.  Outside the subset and for damaged streams the opt-in route must give
the same tensor or the same exception type as the default route on the same bytes."""
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import goldens as G  # noqa: E402
from tests import png_synth as S  # noqa: E402
from tests.test_gpu_frames import _ref  # noqa: E402

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
    cases = {"types": S.group_types(), "deflate": S.group_deflate(), "sizes": S.group_sizes()}
    return {g: [(n, d, S.pil_rgb(d)) for n, d in c] for g, c in cases.items()}


def _by_size(cases):
    out = {}
    for n, d, ref in cases:
        out.setdefault(ref.shape[:2], []).append((n, d, ref))
    return out


def _decode_group_natively(engine, cases):
    """The group through GpuDecodeBatch(gpu_formats=...) at each image's own size (the decode alone): pixels
    equal PIL's, every sample counted as native PNG, none as a PIL fallback."""
    from sds_amd.batched import GpuDecodeBatch
    c0 = engine.counters()
    total = 0
    for (h, w), group in _by_size(cases).items():
        batch = GpuDecodeBatch("png", (h, w), device="cuda", gpu_formats=BOTH, on_error="raise")(
            {"png": [d for _, d, _ in group], "name": [n for n, _, _ in group]})
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(group), 3, h, w)
        for k, (n, _, ref) in enumerate(group):
            np.testing.assert_array_equal(img[k], ref.transpose(2, 0, 1), err_msg=n)
        total += len(group)
    c1 = engine.counters()
    assert c1["png"] - c0["png"] == total
    assert c1["fallback"] - c0["fallback"] == 0
    assert c1["ok"] - c0["ok"] == total


def test_colour_types_sizes_and_filters(engine, refs):
    _decode_group_natively(engine, refs["types"])


def test_deflate_structure(engine, refs):
    _decode_group_natively(engine, refs["deflate"])


def test_incompressible_and_flat_640x480(engine, refs):
    _decode_group_natively(engine, refs["sizes"])


@pytest.mark.parametrize("res,filt,crop", [((24, 40), "bilinear", True), ((150, 90), "bicubic", False)])
def test_resized_outputs_join_the_resample_passes(engine, refs, res, filt, crop):
    cases = [c for c in refs["types"] + refs["deflate"] if min(c[2].shape[:2]) >= 5]
    c0 = engine.counters()
    out, status = engine.decode_resize([d for _, d, _ in cases], res, filter=filt, crop_before_resize=crop, formats=BOTH)
    assert (status == 0).all(), [cases[i][0] for i in np.nonzero(status)[0]]
    out = out.cpu().numpy()
    for k, (n, _, ref) in enumerate(cases):
        np.testing.assert_array_equal(out[k], _ref(ref, res, filt, crop=crop), err_msg=n)
    assert engine.counters()["png"] - c0["png"] == len(cases)


# -- entry points and mixing -------------------------------------------------------------------------
def _mixed():
    _, jpgs = G.g2_jpegs()
    pngs = [S.make(67, 50, 2, "mixP", seed=1), S.make(64, 65, 3, "mixA", seed=2, plte_n=200), S.make(200, 129, 6, "mixU", seed=3),
            S.make(90, 120, 2, "all4", seed=4), S.make(33, 77, 3, "all3", seed=5, trns=True), S.make(101, 40, 6, "mixP", seed=6),
            S.make(640, 480, 2, "mixP", seed=7), S.make(48, 48, 6, "all1", seed=8)]
    jp = [jpgs[k % len(jpgs)] for k in range(8)]
    samples = [x for pair in zip(jp, pngs) for x in pair]
    return samples, [i % 2 == 1 for i in range(16)]


_MIXED_REFS = {}  # (the lanes parameter repeats every configuration: one reference each)


def _mixed_ref(samples, is_png, res, filt, flips, normalize, layout):
    key = (res, filt, tuple(flips), normalize, layout)
    if key not in _MIXED_REFS:
        _MIXED_REFS[key] = _mixed_ref_once(samples, is_png, res, filt, flips, normalize, layout)
    return _MIXED_REFS[key]


def _mixed_ref_once(samples, is_png, res, filt, flips, normalize, layout):
    out = []
    for s, p, f in zip(samples, is_png, flips):
        chw = _ref(S.pil_rgb(s), res, filt, flip=f, normalize=normalize) if p else \
            O.pipeline(s, res, crop_before_resize=True, filter=filt, flip=f, normalize=normalize)
        out.append(chw.transpose(1, 2, 0) if layout == "hwc" else chw)
    return np.stack(out)


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("res,filt,normalize,layout,flipped", [((32, 32), "bilinear", False, "chw", False),
                                                                ((96, 64), "bicubic", True, "hwc", True)])
def test_mixed_batch_through_every_entry_point(engine, lanes, res, filt, normalize, layout, flipped):
    from sds_amd.engine import JpegEngine
    samples, is_png = _mixed()
    n = len(samples)
    flips = [bool(flipped and i % 3 != 1) for i in range(n)]
    ref = _mixed_ref(samples, is_png, res, filt, flips, normalize, layout)
    kw = dict(filter=filt, normalize=normalize, layout=layout, formats=BOTH)
    engine.set_lanes(lanes)
    try:
        c0 = engine.counters()
        outs = {}
        out, st = engine.decode_resize(samples, res, flip=flips, **kw)
        outs["host"] = (out.cpu().numpy(), np.asarray(st))
        lens = np.array([len(s) for s in samples], np.int32)
        offs = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 15) // 16 * 16)[:-1]]).astype(np.int64)
        blob = np.zeros(int(offs[-1] + lens[-1] + 16), np.uint8)
        for s, o in zip(samples, offs):
            blob[o:o + len(s)] = np.frombuffer(s, np.uint8)
        engine.reserve(JpegEngine.scratch_need(samples, res, filter=filt, normalize=normalize, layout=layout, formats=BOTH))
        out, st = engine.decode_resize_device(torch.from_numpy(blob).cuda(), torch.from_numpy(offs).cuda(),
                                              torch.from_numpy(lens).cuda(), res,
                                              flip=torch.tensor(flips, dtype=torch.uint8).cuda(), **kw)
        outs["device"] = (out.cpu().numpy(), st.cpu().numpy())
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
        engine.submit(1, samples, res, flip=flips, **kw)
        out, st = engine.wait(1)
        outs["submit1"] = (out.cpu().numpy(), np.asarray(st))
        for name, (o, st) in outs.items():
            assert (st == 0).all(), (name, st)
            for k in range(n):
                np.testing.assert_array_equal(o[k], ref[k], err_msg=f"{name} row {k}")
        c1 = engine.counters()
        assert c1["png"] - c0["png"] == len(outs) * sum(is_png)
        assert c1["fallback"] - c0["fallback"] == 0
    finally:
        engine.set_lanes(4)


# -- hand-over and damage ----------------------------------------------------------------------------
def _run(transforms, sample):
    for t in transforms:
        sample = t(sample)
    return sample


def _pipeline_outcome(path, **kw):
    from sds_amd.presets import create_standard_image_pipeline
    try:
        s = _run(create_standard_image_pipeline("png", (16, 20), device="cuda", service=None, **kw), {"png": path})
        return "ok", s["image"].cpu().contiguous().numpy()
    except Exception as e:  # noqa: BLE001 -- the exception type is what is compared
        return "err", type(e)


DAMAGE = S.group_damage()


@pytest.mark.parametrize("name,data", DAMAGE, ids=[n for n, _ in DAMAGE])
def test_handover_and_damage_equal_the_default_route(engine, name, data):
    from sds_amd.batched import GpuDecodeBatch
    p = os.path.join(tempfile.mkdtemp(), "x.png")
    with open(p, "wb") as f:
        f.write(data)
    a, b = _pipeline_outcome(p, gpu_formats=BOTH), _pipeline_outcome(p)
    assert a[0] == b[0], (a, b)
    if a[0] == "ok":
        np.testing.assert_array_equal(a[1], b[1])
    else:
        assert a[1] is b[1]
    good = S.make(13, 7, 2, "mixP")
    outs = []
    for fm in (BOTH, ("jpeg",)):
        try:
            r = GpuDecodeBatch("png", (16, 20), device="cuda", gpu_formats=fm, on_error="raise")({"png": [good, data, good]})
            outs.append(("ok", r["image"].cpu().numpy()))
        except Exception as e:  # noqa: BLE001
            outs.append(("err", type(e)))
    assert outs[0][0] == outs[1][0] == a[0]
    if outs[0][0] == "ok":
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
    else:
        assert outs[0][1] is outs[1][1]
    # engine level: status 0 only where PIL decodes the same bytes, and then to the same pixels
    kind, ref = S.pil_outcome(data)
    out, st = engine.decode_resize([data], (16, 20), formats=BOTH)
    if kind == "err":
        assert st[0] != 0
    if st[0] == 0:
        assert kind == "ok"
        np.testing.assert_array_equal(out[0].cpu().numpy(), _ref(ref, (16, 20)))


def test_damage_split_follows_pil(engine):
    """Which damaged inputs PIL accepts is asked of PIL here, not written down: every input it rejects is
    refused natively, and at least one accepted and one rejected input exist, so both branches ran."""
    kinds = {n: S.pil_outcome(d)[0] for n, d in DAMAGE}
    assert "ok" in kinds.values() and "err" in kinds.values()
    _, st = engine.decode_resize([d for _, d in DAMAGE], (16, 20), formats=BOTH)
    for (n, _), s in zip(DAMAGE, st):
        if kinds[n] == "err":
            assert s != 0, n
        assert s in (0, -2, -3), (n, s)


def test_default_is_off(engine):
    data = S.make(13, 7, 2, "mixP")
    c0 = engine.counters()
    _, st = engine.decode_resize([data], (7, 13))
    assert st[0] == -2
    _, st = engine.decode_resize([data], (7, 13), formats=("jpeg",))
    assert st[0] == -2
    c1 = engine.counters()
    assert c1["png"] == c0["png"] and c1["unsupported"] - c0["unsupported"] == 2
    _, st = engine.decode_resize([data], (7, 13), formats=BOTH)  # the mask travels with the call ...
    assert st[0] == 0
    _, st = engine.decode_resize([data], (7, 13))  # ... and does not stay behind on the shared engine
    assert st[0] == -2


def test_need_size_uses_the_png_probe(engine):
    """allow_vertical needs the image size before the decode: with PNG on it comes from sdsj_png_probe,
    and the sample is decoded natively (no fallback)."""
    from sds_amd.presets import create_standard_image_pipeline
    data = S.make(40, 90, 6, "mixP")
    p = os.path.join(tempfile.mkdtemp(), "x.png")
    with open(p, "wb") as f:
        f.write(data)
    c0 = engine.counters()
    kw = dict(device="cuda", service=None, resize_kwargs=dict(allow_vertical=True))
    a = _run(create_standard_image_pipeline("png", (16, 32), gpu_formats=BOTH, **kw), {"png": p})["image"]
    c1 = engine.counters()
    b = _run(create_standard_image_pipeline("png", (16, 32), **kw), {"png": p})["image"]
    assert tuple(a.shape) == tuple(b.shape) and a.shape[0] == 3
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["png"] - c0["png"] == 1 and c1["fallback"] - c0["fallback"] == 0
