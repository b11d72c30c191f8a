"""Host AddressSanitizer + UBSan run of the subsequence layout by subsequence and of the stored entries' safety
predicate (sds_amd/csrc/sdsj_common.h: sub_count, sub_total, sub_interval, sub_layout, hint_entry_safe) in a
stand-alone program, tests/asan/hint_layout_driver.cpp (its own main; nothing is loaded into Python).

k_enthint counts an image's subsequences with these functions and every lane of k_entwrite builds its own
subsequence with them on a hinted image, where no SubState is laid out any more; k_entspec still stores the layout
with ent_layout.  The driver holds the two to each other: seeded random interval tables of 1, 2, 3, 63, 64, 65,
255 and 256 intervals -- lengths of 0, below 0, and 1 bit short of, exactly and 1 bit over a multiple of sub_bits
where whole bytes allow it -- with nsub_cap below, at and above the natural count, every subsequence and the count
compared with a serial restatement of ent_layout.  Then the predicate at its edges: start_bit - 1, start_bit,
lim_bit + 2048, lim_bit + 2049, MCU block bpm - 1 and bpm."""
import os
import shutil
import subprocess

import pytest

from tests import asan_harness as H

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_layout_by_subsequence_equals_ent_layout_under_asan_and_ubsan():
    exe = H.build("hint_layout_driver.cpp", "address,undefined", ("-Wall", "-Werror", "-I", H.INCLUDE))
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **H.ASAN_UBSAN), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok", r.stdout[-2000:]
