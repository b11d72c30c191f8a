"""Asynchronous host path: double-buffered pinned slots, bytes or files read
straight into pinned memory (sdsj_submit_batch / sdsj_submit_files / sdsj_wait_batch).  Results are
checked against the oracle (the CPU restatement pinned to the reference's goldens), status and
pixels; an unreadable file is a per-sample SDSJ_EINVAL.  Includes configs[4]'s shape on one GPU:
640x480 JPEG files -> pinned slot -> H2D -> decode + resize 512x512 -> D2H."""
import os
import tempfile

import numpy as np
import pytest

from oracle import oracle as O

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sds_amd.engine import JpegEngine
    return JpegEngine(max_batch=256)


def _batches():
    from tests.golden.synth import mutated_jpegs
    from tests.test_gpu_parity import _random_jpegs
    a = _random_jpegs(31, 40)
    return [a[:20], a[20:] + mutated_jpegs(31, 10), _random_jpegs(32, 33)]


_ORACLE = {}


def _check_vs_oracle(jpgs, out, st, res, flip=None, normalize=False, skip=()):
    from sds_amd import _lib
    from tests.golden.synth import has_fill_stuffing
    host = out.cpu().numpy()
    for i, j in enumerate(jpgs):
        if i in skip:
            continue
        key = (j, tuple(res), bool(flip[i]) if flip else False, normalize)
        if key not in _ORACLE:  # (computed once per sample and op, shared by the tests of this module)
            try:
                _ORACLE[key] = (O.pipeline(j, res, flip=key[2], normalize=normalize), _lib.OK)
            except O.OracleError as e:
                _ORACLE[key] = (None, e.status)
        ref, rst = _ORACLE[key]
        if rst == _lib.OK and has_fill_stuffing(j):  # (FF FF .. 00: reported CORRUPT, rerun on PIL)
            ref, rst = None, _lib.CORRUPT
        assert st[i] == rst, (i, st[i], rst)
        if ref is not None:
            np.testing.assert_array_equal(host[i], ref, err_msg=f"sample {i}")


def test_submit_wait_matches_oracle(engine):
    res = (48, 40)
    batches = _batches()[:2]
    flips = [[i % 3 == 0 for i in range(len(b))] for b in batches]
    for slot, batch in enumerate(batches):
        engine.submit(slot, batch, res, flip=flips[slot], normalize=True)
    for slot, batch in enumerate(batches):
        out, st = engine.wait(slot)
        _check_vs_oracle(batch, out, st, res, flip=flips[slot], normalize=True)


def test_decode_stream_of_files_with_a_missing_file(engine):
    d = tempfile.mkdtemp()
    batches, paths = _batches(), []
    for b, batch in enumerate(batches):
        ps = []
        for i, j in enumerate(batch):
            p = os.path.join(d, f"{b}_{i}.jpg")
            with open(p, "wb") as f:
                f.write(j)
            ps.append(p)
        paths.append(ps)
    paths[1][3] = os.path.join(d, "missing.jpg")
    from sds_amd import _lib
    before = engine.counters()
    got = list(engine.decode_stream(paths, (64, 64), files=True))
    after = engine.counters()
    assert len(got) == 3
    assert after["other"] == before["other"] + 1  # the unreadable file, counted as such
    # the missing file moves no other count: corrupt / unsupported grow by the returned statuses alone
    sts = np.concatenate([np.asarray(st) for _, st in got])
    assert after["corrupt"] - before["corrupt"] == int((sts == _lib.CORRUPT).sum())
    assert after["unsupported"] - before["unsupported"] == int((sts == _lib.UNSUPPORTED).sum())
    for b, (out, st) in enumerate(got):
        if b == 1:
            assert st[3] == _lib.EINVAL
        _check_vs_oracle(batches[b], out, st, (64, 64), skip=(3,) if b == 1 else ())


def test_resubmitting_a_busy_slot_waits_for_it(engine):
    a, b = _batches()[0], _batches()[2]
    out_a = engine.submit(0, a, (32, 32))
    out_b = engine.submit(0, b, (32, 32))  # the native side waits for batch a before restaging
    got_b, st_b = engine.wait(0)
    assert got_b is out_b
    _check_vs_oracle(a, out_a, np.zeros(len(a), np.int32), (32, 32))
    _check_vs_oracle(b, got_b, st_b, (32, 32))
    with pytest.raises(RuntimeError):
        engine.wait(0)


def test_config4_files_to_512_and_back_to_host_vs_oracle(engine):
    """configs[4] on one GPU: synthetic 640x480 q90 JPEG files (the downloader's local cache) -> pinned
    slot -> H2D -> decode + centre crop + resize 512x512 -> D2H into pinned host memory."""
    from tests.golden.synth import synth_jpegs
    jpgs = synth_jpegs(24, seed=4040)
    d = tempfile.mkdtemp()
    paths = []
    for i, j in enumerate(jpgs):
        p = os.path.join(d, f"{i}.jpg")
        with open(p, "wb") as f:
            f.write(j)
        paths.append(p)
    batches = [paths[:8], paths[8:16], paths[16:]]
    host = torch.empty((24, 3, 512, 512), dtype=torch.uint8).pin_memory()
    k = 0
    for out, st in engine.decode_stream(batches, (512, 512), files=True):
        assert (st == 0).all(), st
        host[k:k + len(st)].copy_(out, non_blocking=True)
        k += len(st)
    torch.cuda.synchronize()
    for i, j in enumerate(jpgs):
        np.testing.assert_array_equal(host[i].numpy(), O.pipeline(j, (512, 512)), err_msg=f"image {i}")


def test_sync_path_runs_more_samples_than_max_batch_in_chunks():
    """decode_resize of 40 samples on an engine of max_batch 16: chunks of 16, 16 and 8 through the one
    staging, statuses and pixels of every sample against the oracle."""
    from sds_amd.engine import JpegEngine
    from tests.golden.synth import mutated_jpegs
    from tests.test_gpu_parity import _random_jpegs
    jpgs = _random_jpegs(41, 30) + mutated_jpegs(41, 10)
    flip = [i % 3 == 1 for i in range(len(jpgs))]
    eng = JpegEngine(max_batch=16)
    out, st = eng.decode_resize(jpgs, (48, 40), flip=flip, normalize=True)
    assert len(st) == 40
    _check_vs_oracle(jpgs, out, st, (48, 40), flip=flip, normalize=True)
    eng.close()


def test_staging_regrowth_on_both_paths():
    """Small batch, then one well past the 1 MiB minimum staging size (the free-then-reallocate path),
    then the small batch again: through decode_resize, and through submit / wait on slot 0 then slot 1."""
    from sds_amd.engine import JpegEngine
    from tests.golden.synth import synth_jpegs
    small, large = synth_jpegs(4, seed=7, w=64, h=48), synth_jpegs(24, seed=8)
    assert sum(len(j) for j in large) > 3 << 19  # (1.5 x the 1 MiB first allocation)
    res = (48, 40)
    eng = JpegEngine(max_batch=64)
    for batch in (small, large, small):
        out, st = eng.decode_resize(batch, res)
        _check_vs_oracle(batch, out, st, res)
    for slot in (0, 1):
        for batch in (small, large, small):
            eng.submit(slot, batch, res)
            out, st = eng.wait(slot)
            _check_vs_oracle(batch, out, st, res)
    eng.close()


def test_empty_and_one_sample_submits(engine):
    from tests.golden.synth import synth_jpegs
    res = (32, 32)
    engine.submit(0, [], res)
    out, st = engine.wait(0)
    assert len(st) == 0 and out.shape[0] == 0
    one = synth_jpegs(1, seed=9, w=64, h=48)
    engine.submit(1, one, res)
    out, st = engine.wait(1)
    _check_vs_oracle(one, out, st, res)


def test_engine_lifetime_create_use_close_three_times_then_goldens():
    """Teardown is the owners' destructors: three engines each run the sync path, a slot and the frames
    path and are closed; a fourth then decodes the g2 goldens bit-exactly."""
    from sds_amd.engine import JpegEngine
    from tests import goldens as G
    from tests.golden.synth import synth_jpegs
    from tests.test_gpu_frames import _frames, _ref
    tiny, res = synth_jpegs(3, seed=10, w=64, h=48), (32, 32)
    fr = _frames(11, 2, 40, 30)
    for _ in range(3):
        eng = JpegEngine(max_batch=32)
        out, st = eng.decode_resize(tiny, res)
        _check_vs_oracle(tiny, out, st, res)
        eng.submit(0, tiny, res)
        out, st = eng.wait(0)
        _check_vs_oracle(tiny, out, st, res)
        out, st = eng.resize_frames(torch.from_numpy(fr).cuda(), (24, 20))
        assert (st == 0).all()
        for k in range(fr.shape[0]):
            np.testing.assert_array_equal(out[k].cpu().numpy(), _ref(fr[k], (24, 20)), err_msg=f"frame {k}")
        eng.close()
    eng = JpegEngine(max_batch=32)
    meta, jpgs = G.g2_jpegs()
    out, st = eng.decode_resize(jpgs, (256, 256))
    assert (st == 0).all(), st
    for k in range(len(jpgs)):
        assert G.sha(out[k].cpu().numpy()) == meta["images"][k]["u8_256_sha256"]
    eng.close()
