"""The opt-in "jpeg-scans" mask on the host (no GPU): the bit's value and names, mask validity, the status of every
fixture of tests/jpeg_scans_synth.py without the bit and under it (sdsj_plan_need_formats, sdsj_probe_formats), the
refused group under every mask, and the parser and planner under the mask in a stand-alone ASan + UBSan program
(tests/asan/jpeg_scans_driver.cpp, its own main; nothing sanitized is loaded into Python).

PIL decodes every fixture, a clean one to the pixels of the same coefficients written as one interleaved scan."""
import ctypes
import shutil

import numpy as np
import pytest

from sds_amd import _lib as L
from tests import asan_harness as H
from tests import jpeg_ext_synth as J
from tests import jpeg_scans_synth as S


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _need(lib, data, mask, crop=1):
    op = L.SdsjOp(16, 20, crop, L.FILTERS["bilinear"], L.DTYPE_U8, L.LAYOUT_CHW)
    need = ctypes.c_int64(-1)
    st = lib.sdsj_plan_need_formats(data, len(data), ctypes.byref(op), mask, ctypes.byref(need))
    return st, need.value


def test_values_and_names():
    assert L.FORMAT_JPEG_SCANS == 128
    assert L.FORMATS["jpeg-scans"] == 129
    assert L.format_mask(("jpeg", "jpeg-scans")) == 129
    assert L.format_mask(("jpeg-scans", "jpeg-ext")) == 193
    assert L.format_mask(("jpeg-scans", "png-meta")) == 147
    assert L.format_mask(S.SCANS) == 129 and L.format_mask(S.SCANS_EXT) == 193


def test_mask_validity(lib):
    data = S.fixtures()[0][1]
    for mask in (128, 130, 8, 32, 192, 136, 161):
        assert _need(lib, data, mask)[0] == L.EINVAL, mask
    for mask in (129, 193, 131, 215):
        assert _need(lib, data, mask)[0] == L.OK, mask
    info = L.SdsjInfo()
    assert lib.sdsj_probe_formats(data, len(data), 128, ctypes.byref(info)) == L.EINVAL


def test_the_references_hold():
    """PIL gives a clean multi-scan file the pixels of its coefficients in one interleaved scan; the redefined
    quantisation table changes the pixels, the redefined Huffman table and the changed restart interval do not; a file
    that ends after two scans decodes."""
    assert len(S.clean()) == 25
    for n, d, _, single in S.clean():
        np.testing.assert_array_equal(J.pil_rgb(d), J.pil_rgb(single), err_msg=n)
    plain = J.pil_rgb(S.plain_of_table_changes())
    by_name = {n: J.pil_rgb(d) for n, d, _, _ in S.table_changes()}
    assert (by_name["dqt-between"] != plain).any()
    np.testing.assert_array_equal(by_name["dht-between"], plain)
    np.testing.assert_array_equal(by_name["dri-between"], plain)
    assert J.pil_outcome(S.early_eoi()[0][1])[0] == "ok"
    kinds = {n: J.pil_outcome(d) for n, d in S.damaged()}
    assert kinds["truncated-scan"] == ("err", OSError)
    assert kinds["truncated-scan-eoi"][0] == "ok" and kinds["flipped-byte"][0] == "ok"
    fill = dict(S.refused())["fill-stuffed"]
    assert fill.count(b"\xff\xff\x00") == 1


def test_status_of_every_fixture(lib):
    fx = S.fixtures()
    assert len(fx) == 29
    for name, data, formats, _ in fx:
        ref = J.pil_rgb(data)  # (PIL decodes every fixture)
        for mask in (L.FORMAT_JPEG, L.FORMAT_JPEG | L.FORMAT_JPEG_EXT):  # nothing moves without the bit
            assert _need(lib, data, mask) == (L.UNSUPPORTED, 0), (name, mask)
            assert L.probe(data, mask)[0] == L.UNSUPPORTED, (name, mask)
        mask = L.format_mask(formats)
        st, need = _need(lib, data, mask)
        assert st == L.OK and need > 0, (name, st, need)
        st, info = L.probe(data, mask)
        assert st == L.OK and info.supported == 1, name
        assert (info.height, info.width) == ref.shape[:2], name
        if formats == S.SCANS_EXT:  # ratios of 4 and RGB-coded files need "jpeg-ext" as well
            assert _need(lib, data, 129) == (L.UNSUPPORTED, 0), name
        else:
            assert _need(lib, data, 193) == (st, need), name
        st, info = L.probe(data)  # sdsj_probe answers as before
        assert st == L.UNSUPPORTED and info.supported == 0, name
        assert (info.height, info.width) == ref.shape[:2], name


def test_one_scan_files_plan_the_same_under_the_bit(lib):
    for name, _, formats, single in S.clean():
        base = L.FORMAT_JPEG | (L.FORMAT_JPEG_EXT if formats == S.SCANS_EXT else 0)
        a, b = _need(lib, single, base), _need(lib, single, base | L.FORMAT_JPEG_SCANS)
        assert a[0] == L.OK and a == b, name


def test_refused_under_every_mask(lib):
    """Without the bit the header refuses them (need 0).  Under it the refusal comes from the walk over the scans,
    which the device makes after it has planned the file's scratch: the status with the plan's need, that of the
    same header on a file the walk accepts."""
    accepted = _need(lib, S.make("420", 50, 37, "y-cb-cr", seed=79)[0], 129)
    assert accepted[0] == L.OK
    for name, data in S.refused():
        for mask in (1, 65, 129, 193):
            st, need = _need(lib, data, mask)
            assert st in (L.UNSUPPORTED, L.CORRUPT), (name, mask, st)
            assert need == (accepted[1] if mask & 128 else 0), (name, mask, need)
            st2, info = L.probe(data, mask)
            assert st2 == st and info.supported == 0, (name, mask)
    assert _need(lib, dict(S.refused())["fill-stuffed"], 129)[0] == L.CORRUPT


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_parser_and_planner_under_the_mask_under_asan_and_ubsan():
    fx = S.fixtures()
    whole = [d for _, d, _, _ in fx] + [d for _, d in S.refused()] + [d for _, d in S.damaged()]
    # header damage on one file of every kind (the truncations of all of them would only repeat the same headers)
    picks = {n: d for n, d, _, _ in fx}
    seeds = [picks[k] for k in ("420-5x9-ycb-cr-sof0-dri3", "422-33x70-ycb-cr-sof1-dri3", "411-50x37-y-cb-cr-sof0-dri0",
                                "444-50x37-y-cbcr-sof0-dri0-rgb", "dqt-between", "dri-between", "eoi-after-two")]
    # cuts all through the scans of one small file (the marker walk meets every position), and byte damage there
    small = picks["420-5x9-y-cb-cr-sof1-dri0"]
    first = small.index(b"\xff\xda")
    rng = np.random.default_rng(3)
    walk = [small[:k] for k in range(first, len(small))]
    for _ in range(64):
        b = bytearray(small)
        b[int(rng.integers(first, len(small)))] = int(rng.choice([0xFF, 0x00, 0xDA, 0xD9, 0xC4, int(rng.integers(0, 256))]))
        walk.append(bytes(b))
    inputs = whole + J.header_mutations(seeds) + walk
    exe = H.build("jpeg_scans_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    rows = H.run_records(exe, inputs, H.ASAN_UBSAN)
    assert len(rows) == len(inputs)
    for (name, _, _, _), row in zip(fx, rows):
        st, need, prog, re, scans = row[:5]
        assert st == 0 and need > 0 and prog == 2 and re == scans, (name, row)
    for (name, _), row in zip(S.refused(), rows[len(fx):]):
        assert row[0] in (L.UNSUPPORTED, L.CORRUPT) and row[1] > 0 and row[2] == 2 and row[3] == row[4], (name, row)
    for row in rows:  # every OK multi-scan sample, damaged ones included, takes k_scans' route
        if row[0] == 0:
            assert (row[2] == 2) == (row[3] == row[4]), row
    try:
        lib = L.load()
    except Exception:  # noqa: BLE001  (the product library is not built: the sanitized run is the check)
        return
    for x, row in zip(inputs, rows):
        st, need = _need(lib, x, 193, crop=0)  # (the driver's op and mask)
        assert (st, need) == (row[0], row[1]), (len(x), st, need, row)
