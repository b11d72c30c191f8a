"""Host AddressSanitizer + UBSan build of the shared JPEG header parser (SURVEY.md §5 "race
detection / sanitizers": the reference has none; the parser in sds_amd/csrc/sdsj_common.h runs on the
host in sdsj_probe and on the device in k_parse).  Every G1/G5 golden JPEG, truncated at every byte
of its headers and with bytes of its headers overwritten, goes through the sanitized parser; the
build aborts on any out-of-bounds read or undefined behaviour.  Statuses must equal the product
library's sdsj_probe (same parser, no sanitizer) where it is loadable."""
import shutil

import pytest

from tests import asan_harness as H
from tests.parser_inputs import inputs as _inputs


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_parser_under_asan_and_ubsan():
    exe = H.build("parse_driver.cpp", "address,undefined", ("-I", H.INCLUDE))
    inputs = _inputs()
    rows = H.run_records(exe, inputs, H.ASAN_UBSAN)
    assert all(row[0] != 99 for row in rows)
    try:
        from sds_amd import _lib
        _lib.load()
    except Exception:  # noqa: BLE001  (the product library is not built: statuses are checked above only)
        return
    for x, row in zip(inputs, rows):
        st, info = _lib.probe(x)
        assert st == row[0], (len(x), st, row[0])
        if st == 0:
            assert (info.width, info.height, info.ncomp) == tuple(row[1:4])
