"""SDSJ_FORMAT_PNG_META on the GPU (gpu_formats "png-meta": k_png_meta between k_parse and k_plan, then
k_png_inflate_meta): files with an ICC profile, compressed and plain text chunks and chunks after the image data
decode natively to the pixels of np.asarray(PIL.Image.open(...).convert("RGB")); the statuses of both entry points
are the probe's; the size and budget limits are judged on the device; without the bit every such file reports
UNSUPPORTED; and the batched transform equals the default route sample for sample."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import goldens as G  # noqa: E402
from tests import png_gpu as P  # noqa: E402
from tests import png_meta_synth as M  # noqa: E402
from tests import png_synth as S  # noqa: E402

META = ("jpeg", "png-meta")
FULL = ("jpeg", "png-ext", "png-meta")
EXT = ("jpeg", "png-ext")


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def files():
    """(name, bytes, PIL's pixels) of the meta files, computed once."""
    return [(n, d, S.pil_rgb(d)) for n, d in M.meta_files()]


def _probe(samples, formats):
    from sds_amd import _lib as L
    mask = L.format_mask(formats)
    return np.array([L.png_probe(s, mask)[0] for s in samples])


def test_full_size_decode_equals_pil_on_both_entry_points(engine, files):
    assert len(files) == 2 * len(M.META_SIZES)
    c0 = engine.counters()
    runs = 0
    for name, data, ref in files:
        h, w = ref.shape[:2]
        out, st = engine.decode_resize([data], (h, w), layout="hwc", formats=META)
        assert list(st) == [0], name
        np.testing.assert_array_equal(out[0].cpu().numpy(), ref, err_msg=name)
        out, st = P.decode_device(engine, [data], (h, w), META, layout="hwc")
        assert list(st) == [0], name
        np.testing.assert_array_equal(out[0], ref, err_msg=name)
        runs += 2
    c1 = engine.counters()
    assert c1["png"] - c0["png"] == runs and c1["fallback"] - c0["fallback"] == 0


def test_adam7_16_bit_with_metadata_under_the_full_mask(engine):
    data = M.meta_adam7_16()
    ref = S.pil_rgb(data)
    c0 = engine.counters()
    for run in (lambda f: engine.decode_resize([data], (7, 13), layout="hwc", formats=f),
                lambda f: P.decode_device(engine, [data], (7, 13), f, layout="hwc")):
        out, st = run(FULL)
        assert list(np.asarray(st)) == [0]
        np.testing.assert_array_equal(np.asarray(out[0].cpu() if hasattr(out[0], "cpu") else out[0]), ref)
        for fm in (META, EXT):  # each bit alone refuses it: Adam7 and tIME, iCCP
            _, st = run(fm)
            assert list(np.asarray(st)) == [-2], fm
    assert engine.counters()["png"] - c0["png"] == 2


def test_mixed_batch_statuses_counter_and_mask_off(engine, files):
    """JPEG, plain PNG, meta files and files the rule hands over in one batch: the statuses of the host and the device
    entry point are the probe's, counters()["png"] counts exactly the native PNG samples, and under masks 7 and 3 every
    file with metadata reports UNSUPPORTED (test_mask_off)."""
    _, jpgs = G.g2_jpegs()
    anchors = {a[0]: a for a in M.anchors()}
    refused = [anchors[k][1] for k in ("iccp_1048577", "iccp_garbage", "post_trns_short", "post_time_ext", "iccp_method1")]
    plain = [S.make(67, 50, 2, "mixP", seed=1), S.make(64, 65, 3, "mixA", seed=2, plte_n=200)]
    meta = [d for _, d, _ in files]
    samples, kinds = [], []
    for k in range(max(len(meta), len(refused))):
        for kind, group in (("jpeg", jpgs[:2]), ("plain", plain), ("meta", meta), ("refused", refused)):
            if k < len(group):
                samples.append(group[k])
                kinds.append(kind)
    kinds = np.array(kinds)
    is_png = kinds != "jpeg"
    want = np.zeros(len(samples), np.int64)
    want[is_png] = _probe([s for s, p in zip(samples, is_png) if p], META)
    assert (want[kinds == "meta"] == 0).all() and (want[kinds == "refused"] == -2).all() and (want[kinds == "plain"] == 0).all()
    res = (32, 32)
    c0 = engine.counters()
    out_h, st_h = engine.decode_resize(samples, res, formats=META)
    out_d, st_d = P.decode_device(engine, samples, res, META)
    c1 = engine.counters()
    np.testing.assert_array_equal(np.asarray(st_h), want)
    np.testing.assert_array_equal(st_d, want)
    np.testing.assert_array_equal(out_h.cpu().numpy(), out_d)
    assert c1["png"] - c0["png"] == 2 * int(((want == 0) & is_png).sum())
    assert c1["unsupported"] - c0["unsupported"] == 2 * len(refused)
    # the bit off: the plain files still decode, to the same pixels; nothing with metadata does
    for fm in (EXT, ("jpeg", "png")):
        out_o, st_o = P.decode_device(engine, samples, res, fm)
        assert (st_o[(kinds == "meta") | (kinds == "refused")] == -2).all(), fm
        assert (st_o[(kinds == "plain") | (kinds == "jpeg")] == 0).all(), fm
        keep = st_o == 0
        np.testing.assert_array_equal(out_o[keep], out_d[keep])


def test_mask_off(engine, files):
    """The same files under mask 7: UNSUPPORTED, every one, on both entry points -- also those whose only metadata
    follows the image data (png_tail_ok's strict answer, which the probe does not give)."""
    late = [M.rgb53(post=[(b"tEXt", b"k\0v")]), M.rgb53(post=[(b"tIME", M.TIME)])]
    batch = [d for _, d, _ in files] + late
    c0 = engine.counters()
    _, st = engine.decode_resize(batch, (16, 16), formats=EXT)
    assert (np.asarray(st) == -2).all(), st
    _, st = P.decode_device(engine, batch, (16, 16), EXT)
    assert (st == -2).all(), st
    assert engine.counters()["png"] == c0["png"]
    _, st = P.decode_device(engine, late, (16, 16), FULL)
    assert (st == 0).all(), st


def test_size_and_budget_limits_on_the_device(engine):
    """1,048,575 against 1,048,577 inflated bytes and 63 against 65 text chunks, judged by k_png_meta: the statuses
    do not depend on host planning (the scratch is reserved from the plain file's need)."""
    from sds_amd.engine import JpegEngine
    anchors = {a[0]: a for a in M.anchors()}
    names = ["iccp_1048575", "iccp_1048577", "ztxt_x63", "ztxt_x65", "ztxt_1048577", "itxt_z_1048577", "ztxt_x33_x33",
             "post_ztxt_1048577", "iccp_1048576"]
    batch = [anchors[k][1] for k in names]
    want = [0 if anchors[k][3] else -2 for k in names]
    assert want == [0, -2, 0, -2, -2, -2, -2, -2, -2]
    for k in names:
        assert (S.pil_outcome(anchors[k][1])[0] == "ok") >= anchors[k][3]
    lens = np.array([len(s) for s in batch], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]]).astype(np.int64)  # (unaligned samples)
    blob = np.frombuffer(b"".join(batch), np.uint8).copy()
    engine.reserve(JpegEngine.scratch_need([M.rgb53()], (3, 5), formats=META) * len(batch))
    out, st = engine.decode_resize_device(torch.from_numpy(blob).cuda(), torch.from_numpy(offs).cuda(),
                                          torch.from_numpy(lens).cuda(), (3, 5), layout="hwc", formats=META)
    assert list(st.cpu().numpy()) == want
    ref = S.pil_rgb(batch[0])
    for k, w in enumerate(want):
        if w == 0:
            np.testing.assert_array_equal(out[k].cpu().numpy(), ref)


def test_batched_transform_equals_the_default_route(engine, files):
    from sds_amd.batched import GpuDecodeBatch
    batch = [d for _, d, _ in files] + [M.realistic(), M.anchors()[3][1]]  # (the garbage profile: handed over, PIL accepts)
    c0 = engine.counters()
    a = GpuDecodeBatch("png", (32, 32), device="cuda", gpu_formats=META, on_error="raise")({"png": batch})["image"]
    c1 = engine.counters()
    b = GpuDecodeBatch("png", (32, 32), device="cuda", on_error="raise")({"png": batch})["image"]
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert c1["png"] - c0["png"] == len(files) and c1["fallback"] - c0["fallback"] == 2  # (realistic has a tIME: mask 23)
    full = GpuDecodeBatch("png", (32, 32), device="cuda", gpu_formats=FULL, on_error="raise")({"png": batch})["image"]
    np.testing.assert_array_equal(full.cpu().numpy(), b.cpu().numpy())
    assert engine.counters()["png"] - c1["png"] == len(files) + 1
    bad = dict((x[0], x[1]) for x in M.anchors())["ztxt_1048577"]
    raised = []
    for fm in (META, ("jpeg",)):
        with pytest.raises(Exception) as e:
            GpuDecodeBatch("png", (32, 32), device="cuda", gpu_formats=fm, on_error="raise")({"png": [batch[0], bad]})
        raised.append(e.type)
    assert raised[0] is raised[1]


def test_set_formats_accepts_and_refuses_the_masks():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd import _lib as L
    from sds_amd.engine import JpegEngine
    eng = JpegEngine("cuda", max_batch=4)
    lib = L.load()
    for mask in (16, 17, 8, 15, 20, 21, 32):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.EINVAL, mask
    for mask in (18, 19, 22, 23, 1):
        assert lib.sdsj_engine_set_formats(eng._h, mask) == L.OK, mask
