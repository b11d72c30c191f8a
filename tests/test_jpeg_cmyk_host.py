"""The opt-in "jpeg-cmyk" mask on the host (no GPU): the bit's value and names, mask validity, the status of every
fixture of tests/jpeg_cmyk_synth.py without the bit and under it (sdsj_plan_need_formats, sdsj_probe_formats), the
references on PIL, the colour steps of k_cmyk restated in numpy against Pillow, the CMYK file of the g6 golden, and the
parser and planner under the masks in a stand-alone ASan + UBSan program (tests/asan/jpeg_cmyk_driver.cpp, its own
main; nothing sanitized is loaded into Python)."""
import ctypes
import io
import os
import shutil

import numpy as np
import pytest

from sds_amd import _lib as L
from tests import asan_harness as H
from tests import goldens as G
from tests import jpeg_cmyk_synth as S
from tests import jpeg_ext_synth as J


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _need(lib, data, mask, crop=1):
    op = L.SdsjOp(16, 20, crop, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    need = ctypes.c_int64(-1)
    st = lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need))
    return st, need.value


def test_values_and_names():
    assert L.FORMAT_JPEG_CMYK == 512
    assert L.FORMATS["jpeg-cmyk"] == 513
    assert L.format_mask(("jpeg-cmyk",)) == 513
    assert L.format_mask(("jpeg", "jpeg-cmyk")) == 513
    assert L.format_mask(("jpeg-cmyk", "jpeg-ext")) == 577
    assert L.format_mask(("jpeg-cmyk", "jpeg-scans")) == 641
    assert L.format_mask(("jpeg-cmyk", "jpeg-ext", "jpeg-scans")) == 705
    assert L.format_mask(("jpeg-cmyk", "gif")) == 769
    assert L.format_mask(("jpeg-cmyk", "gif", "jpeg-ext", "jpeg-scans")) == 513 + 64 + 128 + 256
    assert L.format_mask(S.CMYK) == 513 and L.format_mask(S.CMYK_SCANS) == 641 and L.format_mask(S.CMYK_EXT) == 577


def test_mask_validity(lib):
    data = S.fixtures()[0][1]
    # the bit without SDSJ_FORMAT_JPEG, alone or beside PNG / GIF bits; what was invalid before stays invalid
    for mask in (512, 514, 518, 530, 768, 512 + 64, 512 + 128, 128, 130, 8, 32, 192, 136, 161, 64, 66, 513 + 8, 513 + 32, 1024 + 1):
        assert _need(lib, data, mask)[0] == L.EINVAL, mask
    for mask in (513, 577, 641, 705, 515, 769, 513 + 2 + 4 + 16, 1023 - 8 - 32):
        assert _need(lib, data, mask)[0] == L.OK, mask
    info = L.SdsjInfo()
    assert lib.sdsj_probe_formats(data, len(data), 512, ctypes.byref(info)) == L.EINVAL


def test_status_of_every_fixture(lib):
    fx = S.fixtures()
    assert len(fx) == S.N_FIXTURES == 33
    for name, data, formats, _ in fx:
        ref = J.pil_rgb(data)  # (PIL decodes every fixture)
        own = L.format_mask(formats)
        for mask in (1, 65, 129, 193):  # nothing moves without the bit
            assert _need(lib, data, mask) == (L.UNSUPPORTED, 0), (name, mask)
            st, info = L.probe(data, mask)
            assert st == L.UNSUPPORTED and info.supported == 0, (name, mask)
        st, info = L.probe(data)  # sdsj_probe answers as before
        assert st == L.UNSUPPORTED and info.supported == 0, name
        for mask in (513, own, 705):
            want = L.OK if mask & own == own else L.UNSUPPORTED  # (a file that needs a second bit stays refused without it)
            st, need = _need(lib, data, mask)
            assert st == want and (need > 0) == (want == L.OK), (name, mask, st, need)
            st, info = L.probe(data, mask)
            assert st == want and info.supported == (want == L.OK), (name, mask)
            assert (info.height, info.width) == ref.shape[:2] and info.ncomp == 4, name
        assert _need(lib, data, own) == _need(lib, data, 705), name


def test_refused_and_damaged_statuses(lib):
    for name, data, formats, _ in S.refused():
        for mask in (1, 65, 129, 513, L.format_mask(formats)):
            st, need = _need(lib, data, mask)
            assert st in (L.UNSUPPORTED, L.CORRUPT) and need == 0, (name, mask, st)
            st2, info = L.probe(data, mask)
            assert st2 == st and info.supported == 0, (name, mask)
    by_name = {n: d for n, d, _, _ in S.refused()}
    assert _need(lib, by_name["sixteen-blocks"], 513)[0] == L.CORRUPT  # (as for three components: PIL raises)
    assert _need(lib, by_name["multiscan-without-scans"], 641)[0] == L.OK
    assert _need(lib, by_name["ratio4-without-ext"], 577)[0] == L.OK
    for name, data, _ in S.damaged():
        for mask in (1, 65, 129):
            assert _need(lib, data, mask) == (L.UNSUPPORTED, 0), (name, mask)
        st, need = _need(lib, data, 513)  # the header is whole: the scan is the device's to judge
        assert st == L.OK and need > 0, (name, st)


def test_the_references_hold():
    """PIL decodes every clean fixture, a multi-scan one to the pixels of its one-scan twin; each refused or damaged
    file has the PIL outcome its class claims."""
    twins = 0
    for name, data, _, twin in S.fixtures():
        kind, ref = J.pil_outcome(data)
        assert kind == "ok", name
        if twin is not None:
            np.testing.assert_array_equal(ref, J.pil_rgb(twin), err_msg=name)
            twins += 1
    assert twins == 6
    for name, data, _, cls in S.refused():
        kind, what = J.pil_outcome(data)
        assert kind == cls and (kind == "ok" or what is OSError), (name, kind, what)
    for name, data, cls in S.damaged():
        kind, what = J.pil_outcome(data)
        assert kind == cls and (kind == "ok" or what is OSError), (name, kind, what)
    assert [c for _, _, _, c in S.refused()] == ["ok", "err", "err", "ok", "ok"]
    assert [c for _, _, c in S.damaged()] == ["err", "ok", "ok", "err"]


def test_the_colour_steps_equal_pillows_over_every_pair():
    """Steps 3 and 4 (the inversion of "CMYK;I", cmyk2rgb): a four-layer JPEG sample s with K sample k reaches Pillow
    as the CMYK pixel (255 - s, ., ., 255 - k); all 65,536 pairs, in each of the three colour layers."""
    from PIL import Image
    s, k = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    for layer in range(3):
        raw = np.zeros((256, 256, 4), np.uint8)
        raw[..., layer] = s
        raw[..., (layer + 1) % 3] = 255 - s
        raw[..., 3] = k
        pil = np.asarray(Image.frombytes("CMYK", (256, 256), (255 - raw).tobytes()).convert("RGB"))
        np.testing.assert_array_equal(S.cmyk_to_rgb(raw, False), pil)


def test_the_colour_steps_equal_pils_decode_of_the_fixtures():
    """Steps 2 to 4 on the planes PIL itself decodes: with the Adobe transform byte set to 0 libjpeg converts
    nothing, so PIL's CMYK-mode decode of that file is 255 - the upsampled planes of the original; the restatement
    on them (ycck_cmyk_convert for the YCCK files) equals PIL's convert("RGB") of the original, bit for bit."""
    from PIL import Image
    ycck = 0
    for name, data, _, _ in S.fixtures():
        if b"Adobe" not in data:
            continue
        img = Image.open(io.BytesIO(S.as_transform0(data)))
        assert img.mode == "CMYK"
        raw = 255 - np.asarray(img)
        np.testing.assert_array_equal(S.cmyk_to_rgb(raw, S.ycck_file(data)), J.pil_rgb(data), err_msg=name)
        ycck += S.ycck_file(data)
    assert ycck >= 12
    # without an Adobe marker the file is CMYK: the same coefficients under an Adobe transform-0 marker
    blocks, q = J.random_blocks(17, 23, S.S1, 24)
    np.testing.assert_array_equal(J.pil_rgb(S.write4(17, 23, S.S1, blocks, q, ids=S.IDS_CMYK)),
                                  J.pil_rgb(S.write4(17, 23, S.S1, blocks, q, ids=S.IDS_CMYK, lead=S.adobe(0))))


def test_the_g6_cmyk_file_is_supported_under_the_mask(lib):
    z = np.load(os.path.join(G.GOLDEN, "g6_fallback.npz"))
    data = z["jpeg_cmyk_48x32__bytes"].tobytes()
    assert _need(lib, data, 1) == (L.UNSUPPORTED, 0)
    st, need = _need(lib, data, 513)
    assert st == L.OK and need > 0
    st, info = L.probe(data, 513)
    assert st == L.OK and info.supported == 1 and (info.width, info.height, info.ncomp) == (48, 32, 4)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_parser_and_planner_under_the_masks_under_asan_and_ubsan():
    fx = S.fixtures()
    whole = [d for _, d, _, _ in fx] + [d for _, d, _, _ in S.refused()] + [d for _, d, _ in S.damaged()]
    picks = {n: d for n, d, _, _ in fx}
    seeds = [picks[k] for k in ("pil-ss2-5x9", "ycck-photoshop-5x9", "no-adobe-17x23", "cmyk-dri1-50x37",
                                "scans-cmy-k-5x9-dri0", "scans-c-m-y-k-17x23-dri3", "cmyk-411-50x37")]
    # cuts all through the scans of one small multi-scan file (the marker walk meets every position), and byte damage
    small = picks["scans-cmy-k-5x9-dri0"]
    first = small.index(b"\xff\xda")
    rng = np.random.default_rng(3)
    walk = [small[:k] for k in range(first, len(small))]
    for _ in range(64):
        b = bytearray(small)
        b[int(rng.integers(first, len(small)))] = int(rng.choice([0xFF, 0x00, 0xDA, 0xD9, 0xC4, int(rng.integers(0, 256))]))
        walk.append(bytes(b))
    inputs = whole + J.header_mutations(seeds) + walk
    exe = H.build("jpeg_cmyk_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    rows = H.run_records(exe, inputs, H.ASAN_UBSAN)
    assert len(rows) == len(inputs)
    masks = (513, 577, 641, 705)
    for (name, _, formats, _), row in zip(fx, rows):
        own = L.format_mask(formats)
        for k, mask in enumerate(masks):
            st, need, prog, re = row[4 * k:4 * k + 4]
            if mask & own == own:
                assert st == 0 and need > 0 and prog == 2 and re == row[16], (name, mask, row)
            else:
                assert st == L.UNSUPPORTED and need == 0, (name, mask, row)
        assert row[17] == 4, (name, row)
    for row in rows:  # every sample of four components the planner accepts takes k_scans' route
        for k in range(4):
            if row[4 * k] == 0 and row[17] == 4:
                assert row[4 * k + 2] == 2 and row[4 * k + 3] == row[16], row
    try:
        lib = L.load()
    except Exception:  # noqa: BLE001  (the product library is not built: the sanitized run is the check)
        return
    for x, row in zip(inputs, rows):
        for k, mask in enumerate(masks):
            st, need = _need(lib, x, mask, crop=0)  # (the driver's op and masks)
            assert (st, need) == (row[4 * k], row[4 * k + 1]), (len(x), mask, st, need, row)
