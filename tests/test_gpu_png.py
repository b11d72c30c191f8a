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
from tests import png_gpu as P  # noqa: E402
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


def test_colour_types_sizes_and_filters(engine, refs):
    P.decode_group_natively(engine, refs["types"], BOTH)


def test_deflate_structure(engine, refs):
    P.decode_group_natively(engine, refs["deflate"], BOTH)


def test_incompressible_and_flat_640x480(engine, refs):
    P.decode_group_natively(engine, refs["sizes"], BOTH)


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
        engine.submit(1, samples, res, flip=flips, **kw)
        out, st = engine.wait(1)
        outs["submit1"] = (out.cpu().numpy(), np.asarray(st))
        P.assert_rows_equal(outs, ref)
        c1 = engine.counters()
        assert c1["png"] - c0["png"] == len(outs) * sum(is_png)
        assert c1["fallback"] - c0["fallback"] == 0
    finally:
        engine.set_lanes(4)


# -- hand-over and damage ----------------------------------------------------------------------------
DAMAGE = S.group_damage()


@pytest.mark.parametrize("name,data", DAMAGE, ids=[n for n, _ in DAMAGE])
def test_handover_and_damage_equal_the_default_route(engine, name, data):
    P.check_handover_and_damage(engine, data, BOTH, S.make(13, 7, 2, "mixP"))


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
    a = P.run_transforms(create_standard_image_pipeline("png", (16, 32), gpu_formats=BOTH, **kw), {"png": p})["image"]
    c1 = engine.counters()
    b = P.run_transforms(create_standard_image_pipeline("png", (16, 32), **kw), {"png": p})["image"]
    assert tuple(a.shape) == tuple(b.shape) and a.shape[0] == 3
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["png"] - c0["png"] == 1 and c1["fallback"] - c0["fallback"] == 0
