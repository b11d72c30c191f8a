"""The compact coefficient format between k_entwrite<11> and k_idct (sdsj_common.h coef_compact): 64-byte main
slots of 8-bit AC coefficients with the DC in their first word, and a hi slot for the blocks that do not fit.
Calls of at most 32 images run in latency mode, which keeps int16 blocks: every case here also runs in a batch
of 40 (the throughput plan), where the compact format applies.

Inputs with exact quantised coefficients come from tests/golden/coefjpeg.py write_jpeg; every comparison is
bit-exact against the C oracle (the checker), as in test_gpu_parity.py.
"""
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import goldens as G  # noqa: E402
from tests.golden.coefjpeg import extreme_jpegs, six_slot_jpegs, write_jpeg  # noqa: E402

BOUNDARY = (127, -127, -128, 128, -129, 255, 256, 1023, -1023)
Q1 = {0: np.ones(64, np.int64)}
YUV420 = [(2, 2, 0), (1, 1, 1), (1, 1, 1)]


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import JpegEngine
    return JpegEngine(max_batch=64)


def _gray_block(pairs, dc=40) -> bytes:
    b = np.zeros((1, 1, 64), np.int64)
    b[0, 0, 0] = dc
    for k, v in pairs:
        b[0, 0, k] = v
    return write_jpeg(8, 8, [(1, 1, 0)], [b], Q1)


def _full_equals_oracle(engine, jpg, msg=""):
    ref = O.decode(jpg)
    got, st = engine.decode_resize([jpg], ref.shape[:2], layout="hwc")
    assert st[0] == 0, msg
    np.testing.assert_array_equal(got[0].cpu().numpy(), ref, err_msg=msg)


@pytest.mark.parametrize("where", ["ac1", "ac63", "ac62_ac63"])
def test_width_boundary_one_block(engine, where):
    """One-block gray images, quantisation table all 1, an AC value on either side of the 8-bit boundary (and
    at the ends of the 16-bit symbols' range) at the first position, the last, and the last two."""
    pos = {"ac1": (1,), "ac63": (63,), "ac62_ac63": (62, 63)}[where]
    jpgs = [_gray_block([(k, v) for k in pos]) for v in BOUNDARY]
    for v, j in zip(BOUNDARY, jpgs):
        _full_equals_oracle(engine, j, f"{where} = {v}")
    # the same images in one throughput-plan batch (more than kSmallBatch images)
    batch = (jpgs * 5)[:40]
    got, st = engine.decode_resize(batch, (8, 8))
    assert (st == 0).all(), st
    for k, j in enumerate(batch):
        np.testing.assert_array_equal(got[k].cpu().numpy(), O.pipeline(j, (8, 8)), err_msg=f"{where} image {k}")


@pytest.mark.parametrize("where", ["ac63_4bit", "dc_11bit", "ac63_hi63", "dc_11bit_wide_ac"])
def test_main_slot_word_boundaries_one_block(engine, where):
    """The main slot's first word holds 4 bits of AC 63 and 11 bits of DC: one-block gray images on either side
    of both edges.  ac63_4bit: AC 63 = 7 / -8 (symbols of 3 and 4 bits) / 8 / -9, alone and next to a narrow
    negative AC; dc_11bit: DC = 1023 / 1024 / -1024 / -1025 with narrow AC only (a block flagged by its DC
    alone zeroes its own hi slot); ac63_hi63: the widest AC 63 the Annex K tables can code (+-1023, category
    10: hi[0] = +-64; hi[63] only leaves zero beyond +-2047, which needs a category these tables do not
    have), next to a wide AC 62 and in a block wide at every position; dc_11bit_wide_ac: both kinds of flag
    in one block."""
    jpgs = []
    if where == "ac63_4bit":
        for v in (7, -7, -8, 8, -9, 15, -16):
            jpgs.append(_gray_block([(63, v)]))
            jpgs.append(_gray_block([(1, -5), (40, -127), (63, v)]))
    elif where == "dc_11bit":
        for dc in (1023, 1024, -1024, -1025, 2047, -2047):
            jpgs.append(_gray_block([(1, -3), (62, 100)], dc=dc))
            jpgs.append(_gray_block([], dc=dc))
    elif where == "ac63_hi63":
        for v in (1023, -1023, 512, -513):
            jpgs.append(_gray_block([(62, -v), (63, v)]))
            jpgs.append(_gray_block([(k, -v if k % 2 else v) for k in range(1, 64)]))
    else:
        for dc in (1024, -1025):
            jpgs.append(_gray_block([(5, 300), (63, -9)], dc=dc))
            jpgs.append(_gray_block([(5, -128), (63, 7)], dc=dc))
    for k, j in enumerate(jpgs):
        _full_equals_oracle(engine, j, f"{where} image {k}")
    batch = (jpgs * 6)[:40]  # the throughput plan; a narrow image after each flagged one in the same slots
    batch[1::2] = [_gray_block([(1, -2)])] * len(batch[1::2])
    got, st = engine.decode_resize(batch, (8, 8))
    assert (st == 0).all(), st
    for k, j in enumerate(batch):
        np.testing.assert_array_equal(got[k].cpu().numpy(), O.pipeline(j, (8, 8)), err_msg=f"{where} image {k}")


def test_width_boundary_one_mcu_420(engine):
    """A 16x16 4:2:0 image (one MCU, 6 blocks) with one wide coefficient in each component, next to narrow
    negative ones in the same blocks."""
    rng = np.random.default_rng(11)
    blocks = [np.zeros((2, 2, 64), np.int64), np.zeros((1, 1, 64), np.int64), np.zeros((1, 1, 64), np.int64)]
    for b in blocks:
        b[..., 1:20] = rng.integers(-127, 128, b[..., 1:20].shape)
        b[..., 0] = rng.integers(-200, 200, b[..., 0].shape)
    blocks[0][1, 0, 7] = 300
    blocks[1][0, 0, 63] = -513
    blocks[2][0, 0, 2] = 128
    q = {0: np.ones(64, np.int64), 1: np.ones(64, np.int64)}
    jpg = write_jpeg(16, 16, YUV420, blocks, q)
    _full_equals_oracle(engine, jpg)
    got, st = engine.decode_resize([jpg] * 40, (16, 16))  # the throughput plan: compact blocks
    assert (st == 0).all(), st
    ref = O.pipeline(jpg, (16, 16))
    for k in range(40):
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref, err_msg=f"image {k}")


def _mcu420_48x32(rng, dense_wide: bool):
    """48x32 4:2:0: 6 MCUs of 6 blocks = 36 blocks.  dense_wide: |AC| >= 256 at all 63 positions of every
    block; else narrow values (both signs) everywhere."""
    blocks = []
    for bh, bw in ((4, 6), (2, 3), (2, 3)):
        b = np.zeros((bh, bw, 64), np.int64)
        if dense_wide:
            b[..., 1:] = rng.integers(256, 1024, (bh, bw, 63)) * rng.choice([-1, 1], (bh, bw, 63))
        else:
            b[..., 1:] = rng.integers(-127, 128, (bh, bw, 63))
        b[..., 0] = rng.integers(-500, 500, (bh, bw))
        blocks.append(b)
    return blocks


def test_mixed_blocks_and_stale_hi_slots(engine):
    """Batch X (every block dense with |AC| >= 256: every hi slot written), then batch Y of the same geometry,
    narrow except AC63 = 300 in the first block, the last block and one chroma block: a flagged slot's other 62
    bytes are zeros and unflagged blocks ignore what X left in hi.  Then X again."""
    rng = np.random.default_rng(23)
    q = {0: np.ones(64, np.int64), 1: np.full(64, 2, np.int64)}
    xs, ys = [], []
    for _ in range(4):
        xs.append(write_jpeg(48, 32, YUV420, _mcu420_48x32(rng, True), q))
        by = _mcu420_48x32(rng, False)
        by[0][0, 0, 63] = 300   # the first block in decode order
        by[2][1, 2, 63] = 300   # the last one (Cr of the last MCU)
        by[1][0, 1, 63] = 300   # a chroma block in between
        ys.append(write_jpeg(48, 32, YUV420, by, q))
    refs = {j: O.pipeline(j, (32, 48)) for j in xs + ys}
    for name, four in (("X", xs), ("Y", ys), ("X again", xs)):
        batch = four * 10  # 40 images: the throughput plan, so the compact format
        got, st = engine.decode_resize(batch, (32, 48))
        assert (st == 0).all(), (name, st)
        for k, j in enumerate(batch):
            np.testing.assert_array_equal(got[k].cpu().numpy(), refs[j], err_msg=f"{name} image {k}")


def test_flush_of_more_than_16_blocks_per_wave(engine):
    """A PIL-encoded image whose entropy data gives >= 64 subsequences, so a wave of the write pass has 64
    decoding lanes and its flush takes more than one 16-block step: one-image calls (latency mode, the
    multi-hypothesis route) and a 40-image batch (throughput plan), bit-exact against the oracle."""
    from tests.golden.synth import encode_jpeg, synth_rgb
    from tests.gpu_debug import snapshot
    rng = np.random.default_rng(7)
    jpgs = [encode_jpeg(synth_rgb(rng, 160, 120), 95) for _ in range(4)]
    res = (96, 128)
    refs = [O.pipeline(j, res) for j in jpgs]
    for k, j in enumerate(jpgs[:2]):
        got, st = engine.decode_resize([j], res)
        assert st[0] == 0
        d, _ = snapshot(engine, 1)
        assert d[0].nsub >= 64, d[0].nsub
        np.testing.assert_array_equal(got[0].cpu().numpy(), refs[k], err_msg=f"single image {k}")
    batch = [jpgs[k % 4] for k in range(40)]
    got, st = engine.decode_resize(batch, res)
    assert (st == 0).all(), st
    d, _ = snapshot(engine, 40)
    assert all(x.nsub >= 64 for x in d), [x.nsub for x in d]
    for k in range(40):
        np.testing.assert_array_equal(got[k].cpu().numpy(), refs[k % 4], err_msg=f"batch image {k}")


def test_coefficient_level_both_widths_vs_oracle(engine):
    """The stored coefficients themselves, read back through tests/coef_compact.py from a 40-image batch (compact
    format): G2 image 0 (no flagged block) and the extreme-coefficient images (some flagged) equal the oracle's
    block for block.  The same images in one-image calls (latency mode: int16 blocks) read back equal too."""
    from tests.coef_compact import blocks_differing_from_oracle, is_compact, read_blocks
    from tests.gpu_debug import snapshot
    _, g2 = G.g2_jpegs()
    cases = [("g2[0]", g2[0])] + [(f"extreme[{k}]", j) for k, j in enumerate(extreme_jpegs(202, 8))]
    batch = [cases[k % len(cases)][1] for k in range(40)]
    _, st = engine.decode_resize(batch, (32, 32))
    assert (st == 0).all(), st
    d, fetch = snapshot(engine, 40)
    flagged_total = 0
    for k, (name, j) in enumerate(cases):
        assert is_compact(d[k]), name
        zz, flagged = read_blocks(d[k], fetch)
        assert blocks_differing_from_oracle(d[k], zz, j) == [0] * d[k].ncomp, name
        if name == "g2[0]":
            assert not flagged.any()
        else:
            flagged_total += int(flagged.sum())
    assert flagged_total > 0
    for name, j in cases[:3]:
        _, st = engine.decode_resize([j], (32, 32))
        assert st[0] == 0, name
        d, fetch = snapshot(engine, 1)
        assert not is_compact(d[0]), name
        zz, _ = read_blocks(d[0], fetch)
        assert blocks_differing_from_oracle(d[0], zz, j) == [0] * d[0].ncomp, name


def test_formats_side_by_side_in_one_batch(engine):
    """A 6-slot image (10-bit route, int16 blocks), a progressive image (k_prog, int16 blocks) and 4-slot
    baseline images (compact format) in one 40-image batch, bit-exact against the oracle."""
    from PIL import Image
    from tests.golden.synth import encode_jpeg, synth_rgb
    rng = np.random.default_rng(31)
    six = six_slot_jpegs(43, 2)
    buf = io.BytesIO()
    Image.fromarray(synth_rgb(rng, 160, 120)).save(buf, format="JPEG", quality=88, progressive=True)
    prog = buf.getvalue()
    base = [encode_jpeg(synth_rgb(rng, 160, 120), 90) for _ in range(4)] + extreme_jpegs(77, 4)
    jpgs = []
    for k in range(40):
        jpgs.append(six[k % 2] if k % 10 == 3 else prog if k % 10 == 6 else base[k % len(base)])
    res = (64, 80)
    got, st = engine.decode_resize(jpgs, res)
    assert (st == 0).all(), st
    refs = {}
    for k, j in enumerate(jpgs):
        if j not in refs:
            refs[j] = O.pipeline(j, res)
        np.testing.assert_array_equal(got[k].cpu().numpy(), refs[j], err_msg=f"image {k}")
