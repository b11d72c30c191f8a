"""The write pass reads the entry-point store's records itself: a hit image has no SubState laid
out -- k_enthint only looks the record up, every lane of k_entwrite builds its own subsequence of the layout
(sdsj_common.h sub_layout; tests/test_hint_layout_host.py holds it to ent_layout on the CPU) and takes its packed
entry from the record, and its predecessor proves it against what it left in LDS.

Scaffolding as tests/test_gpu_hints.py (Blob, Rig, the oracle's results computed once): small generated images
through ``decode_resize_device`` over dirtied scratch, every status and pixel compared with the oracle by
``Rig.run`` whatever the store did.  Each test decodes the same device blob twice; the second call's counters say
that every served row was decoded from its record, and its coefficient blocks (tests/coef_compact.py) equal the
first call's."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import entropy_cases as E  # noqa: E402
from tests import gpu_debug  # noqa: E402
from tests.coef_compact import read_blocks  # noqa: E402
from tests.test_gpu_hints import HINT_KEYS, N, Blob, E_route11, Rig, oracle, small  # noqa: E402

K_SEG_EMPTY, K_SEG_INS = 1, 2  # sdsj_common.h kSegEmpty, kSegIns
ALL_HIT = lambda n: {"hint_hits": n, "hint_misses": 0, "hint_verify_failed": 0, "hint_stored": 0}  # noqa: E731


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Rig()


def looked_up(d) -> bool:
    """An image k_enthint looks up: the single-group plan of the 11-bit route outside latency mode."""
    return d.status == 0 and d.ent_groups == 1 and not d.lat and not d.mh and not d.progressive and E_route11(d)


def served(d) -> bool:
    """An image the store keeps a record of: looked up, and of at most kDecodeThreads subsequences."""
    return looked_up(d) and d.nsub <= E.const("SDSJ_DECODE_THREADS")


def seg_table(d, fetch):
    """(lo, hi, vend, flag) of the image's restart-interval table (sdsj_common.h seg_view)."""
    n = d.nseg
    t = fetch(d.off_seg, (4 * n + 2) * 4).view(np.int32)
    return t[:n], t[n + 1:2 * n + 1], t[2 * n + 2:3 * n + 2], t[3 * n + 2:4 * n + 2]


def coefs(rig, rows, which):
    """The coefficient blocks of the last call's images `which` (indices into its rows)."""
    descs, fetch = gpu_debug.snapshot(rig.engine, len(rows))
    return {k: read_blocks(descs[k], fetch)[0] for k in which}


def twice(rig, blob, want_served=None):
    """Two calls over the blob: the first records every served row, the second decodes each from its record, all
    proved, to the same coefficient blocks.  Returns both calls' descriptors."""
    rows = list(range(len(blob.files)))
    rig.engine.clear_hints()  # (an earlier test's blob may have stood at these addresses)
    _, _, d1, c1 = rig.run(blob)
    sv = [k for k, d in enumerate(d1) if served(d)]
    if want_served is not None:
        assert sv == list(want_served), sv
    assert c1["hint_stored"] == len(sv) and c1["hint_hits"] == 0, c1
    z1 = coefs(rig, rows, sv)
    _, _, d2, c2 = rig.run(blob)
    # (an image of more than kDecodeThreads subsequences is looked up and never recorded: a miss in every call)
    too_long = sum(1 for d in d1 if looked_up(d)) - len(sv)
    assert c2 == dict(ALL_HIT(len(sv)), hint_misses=too_long), c2
    z2 = coefs(rig, rows, sv)
    for k in sv:
        np.testing.assert_array_equal(z2[k], z1[k], err_msg=f"row {k}: coefficient blocks of the hit")
    assert [d.nsub for d in d2] == [d.nsub for d in d1]
    return d1, d2, sv


def test_every_single_group_case_of_the_table(rig):
    """Every case of tests/entropy_cases.py under 1 MP in one batch; the ones the store serves are chosen by the
    device's own descriptors, and must hold the three restart-boundary cases (an interval beginning at
    subsequence 63, 64 and 65) and a case without DRI."""
    cases = [c for c in E.CASES if not c.big]
    assert len(cases) <= 64
    blob = Blob([E.case_image(c) for c in cases])
    d1, _, sv = twice(rig, blob)
    names = {cases[k].name for k in sv}
    print("served:", sorted(names))
    assert {"seg_first_63", "seg_first_64", "seg_first_65"} <= names, names
    assert any(d1[k].nseg == 1 for k in sv), "no served case without DRI"
    for idx in (63, 64, 65):
        d = d1[next(k for k in sv if cases[k].name == f"seg_first_{idx}")]
        assert d.nseg > 1 and d.nsub > idx


def _empty_interval(jpg: bytes) -> bytes:
    """The restart-interval file with its second RSTn renumbered one ahead: libjpeg leaves it unread, decodes an
    empty interval, and takes it as the next interval's marker (jdmarker.c jpeg_resync_to_restart)."""
    p = E.rst_positions(jpg)[1]
    return jpg[:p + 1] + bytes([0xD0 + ((jpg[p + 1] - 0xD0 + 1) & 7)]) + jpg[p + 2:]


def test_other_mcu_shapes_and_an_empty_interval(rig):
    one_each = E.noise(64, 48, 75, "444", 1, 21)     # 48 intervals under kMinSubBits bits: one subsequence each
    empty = _empty_interval(small(22, rst=4))        # kSegEmpty
    gray, gray_rst = small(23, gray=True), small(24, gray=True, rst=2)
    shared = E.case_image(next(c for c in E.CASES if c.name == "sync_control_444"))
    files = [one_each, empty, gray, gray_rst, shared]
    assert oracle(empty)[0] == O.OK
    blob = Blob(files + [small(900 + k) for k in range(N - len(files))])
    d1, d2, _ = twice(rig, blob, want_served=range(N))
    assert d1[0].nseg == d1[0].nsub > 1
    _, fetch = gpu_debug.snapshot(rig.engine, N)
    lo, hi, _, flag = seg_table(d2[1], fetch)
    assert (flag & K_SEG_EMPTY).any() and (hi[(flag & K_SEG_EMPTY) != 0] == lo[(flag & K_SEG_EMPTY) != 0]).all()
    assert d1[2].ncomp == 1 and d1[2].bpm == 1 and d1[2].nseg == 1 and d1[3].bpm == 1 and d1[3].nseg > 1
    # the shared table pair: the sync pass had work, and the hit puts its statistics back
    assert d1[4].sync_rounds >= 1 and d1[4].pad0 >= 1
    assert (d2[4].sync_rounds, d2[4].pad0) == (d1[4].sync_rounds, d1[4].pad0)


W, H, RST_ROWS = 128, 96, 6  # 4:4:4: 16 x 12 MCUs, two restart intervals of 6 MCU rows


def _join(blocks) -> bytes:
    """tests.entropy_cases.coef_jpeg's restart-interval file, from given coefficient blocks."""
    from tests.golden.coefjpeg import write_jpeg
    mcux, mcuy = W // 8, H // 8
    head, scans = None, []
    for r0 in range(0, mcuy, RST_ROWS):
        part = write_jpeg(W, RST_ROWS * 8, E.S444, [b[r0:r0 + RST_ROWS] for b in blocks], E.Q)
        off = E.entropy_off(part)
        if head is None:
            head = bytearray(part[:off])
        scans.append(part[off:-2])
    sof = head.index(b"\xff\xc0")
    head[sof + 5:sof + 7] = H.to_bytes(2, "big")
    sos = head.index(b"\xff\xda")
    head[sos:sos] = b"\xff\xdd\x00\x04" + (mcux * RST_ROWS).to_bytes(2, "big")
    body = b"".join(s + (bytes([0xFF, 0xD0 + k % 8]) if k + 1 < len(scans) else b"") for k, s in enumerate(scans))
    return bytes(head) + body + b"\xff\xd9"


def _late_dc_pair():
    """Two restart-interval files from coefficients that differ in the lowest value bit of one DC difference, in the
    first MCU row of the last interval (every later block of the interval's component moves with it, so only that
    difference changes): same Huffman codes, same length, one byte apart.  The lanes after that block's in its
    interval hold its DC sum in their entries."""
    base = E.coef_blocks(33, W, H, E.S444, 12, 40)
    a = _join(base)
    bw = W // 8
    flat = base[0][..., 0].reshape(-1)
    for k in range(RST_ROWS * bw + 1, (RST_ROWS + 1) * bw):
        d = int(flat[k] - flat[k - 1])
        if abs(d) < 2 or d % 2:
            continue
        moved = flat.copy()
        moved[k:] += int(np.sign(d))
        blocks = [b.copy() for b in base]
        blocks[0][..., 0] = moved.reshape(base[0].shape[:2])
        b = _join(blocks)
        if len(b) == len(a) and sum(p != q for p, q in zip(a, b)) == 1:
            return a, b
    raise AssertionError("no such pair")


def test_refuted_without_a_laid_out_substate(rig):
    """A restart-interval row replaced in place by a copy that differs in one DC-difference bit of its last
    interval: the record's header still matches, the lanes after the change start from stale DC sums and the proof
    refutes them; the retry lays the image out, decodes the new bytes, and leaves vend / kSegIns as a fresh engine
    does; the third call hits."""
    a, b = _late_dc_pair()
    assert oracle(a)[0] == O.OK and oracle(b)[0] == O.OK and not np.array_equal(oracle(a)[1], oracle(b)[1])
    blob = Blob([a] + [small(950 + k) for k in range(N - 1)])
    rig.engine.clear_hints()
    _, _, d1, c = rig.run(blob)
    assert c["hint_stored"] == N and served(d1[0]) and d1[0].nseg == 2
    _, fetch = gpu_debug.snapshot(rig.engine, N)
    lo, hi, _, _ = seg_table(d1[0], fetch)
    assert (int(hi[1]) - int(lo[1])) * 8 > 2 * d1[0].sub_bits, "the last interval must hold lanes after the change"
    blob.put(0, b)
    _, _, d2, c = rig.run(blob)  # (statuses and pixels: the oracle's for the bytes now there)
    assert c["hint_verify_failed"] >= 1 and c["hint_hits"] == N - c["hint_verify_failed"] and c["hint_misses"] == 0, c
    assert c["hint_stored"] == c["hint_verify_failed"]
    _, fetch = gpu_debug.snapshot(rig.engine, N)
    _, _, vend, flag = (x.copy() for x in seg_table(d2[0], fetch))
    z2 = coefs(rig, range(N), [0])[0]
    fresh = Rig()
    _, _, df, _ = fresh.run(blob)
    _, ffetch = gpu_debug.snapshot(fresh.engine, N)
    _, _, fvend, fflag = seg_table(df[0], ffetch)
    np.testing.assert_array_equal(vend, fvend)
    np.testing.assert_array_equal(flag & K_SEG_INS, fflag & K_SEG_INS)
    np.testing.assert_array_equal(z2, coefs(fresh, range(N), [0])[0])
    _, _, _, c = rig.run(blob)
    assert c == ALL_HIT(N), c
    np.testing.assert_array_equal(coefs(rig, range(N), [0])[0], z2)


def test_the_same_row_in_two_lanes_and_twice_in_one():
    """512-image calls (four lanes): 16 rows stand at three positions each, one in the first lane and two in the
    last.  A later copy may find the record an earlier one is writing -- whole, torn (refuted by the write pass) or
    not yet there; every copy equals the oracle, and the next call decodes all 512 from records."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rig = Rig(max_batch=512)
    kinds = [small(500 + k) for k in range(8)]
    blob = Blob([kinds[k % 8] for k in range(480)])
    win = list(range(480)) + list(range(16)) + list(range(16))
    got, _, d, c = rig.run(blob, win)
    assert all(x.nsub >= 4 for x in d)
    assert c["hint_hits"] + c["hint_verify_failed"] <= 32 and c["hint_hits"] + c["hint_misses"] + c["hint_verify_failed"] == 512, c
    for k in range(16):
        np.testing.assert_array_equal(got[480 + k], got[k])
        np.testing.assert_array_equal(got[496 + k], got[k])
    got2, _, _, c = rig.run(blob, win)
    assert c == ALL_HIT(512), c
    np.testing.assert_array_equal(got2, got)
    assert set(HINT_KEYS) == set(c)
