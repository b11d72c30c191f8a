"""The entry-point store of the device-resident path (include/sdsj.h sdsj_engine_set_hints).

A row decoded before is decoded again from its stored entry states, without the speculative and sync passes; the
write pass proves the states while it decodes and the call falls back to the full decode when it cannot.  So a
record may cost time and never a pixel: every test compares statuses and pixels with the oracle, whatever the
store did, and the counters say which path ran.

Every call is a chunk of 40 small images through ``decode_resize_device`` (the throughput plan; one test uses 512
so that four lanes run); the images are just large enough for at least four subsequences, which each test
asserts from the descriptors.  Between two calls over the same rows the engine decodes a batch of larger noise
images through the host path, so subsequence states and coefficient slots in scratch are stale."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from tests import entropy_cases as E  # noqa: E402
from tests import gpu_debug  # noqa: E402

RES = (48, 64)
N = E.BATCH
HINT_KEYS = ("hint_hits", "hint_misses", "hint_verify_failed", "hint_stored")
_refs: dict = {}


def oracle(jpg: bytes):
    """(status, pixels or None) of one file, computed once."""
    if jpg not in _refs:
        try:
            r = O.pipeline(jpg, RES)
            r.setflags(write=False)
            _refs[jpg] = (O.OK, r)
        except O.OracleError as e:
            _refs[jpg] = (e.status, None)
    return _refs[jpg]


def small(seed: int, **kw) -> bytes:
    return E.noise(64, 48, 90, kw.pop("samp", "420"), kw.pop("rst", 0), seed, **kw)


class Blob:
    """Samples in one device tensor at 16-byte-aligned offsets; ``put`` replaces one in place."""

    def __init__(self, files):
        self.files = list(files)
        self.offs, pos = [], 0
        for f in self.files:
            self.offs.append(pos)
            pos += -(-len(f) // 16) * 16
        host = np.zeros(pos + 16, np.uint8)
        for o, f in zip(self.offs, self.files):
            host[o:o + len(f)] = np.frombuffer(f, np.uint8)
        self.data = torch.from_numpy(host).cuda()

    def args(self, rows):
        return (self.data, torch.tensor([self.offs[r] for r in rows], dtype=torch.int64).cuda(),
                torch.tensor([len(self.files[r]) for r in rows], dtype=torch.int32).cuda())

    def put(self, row: int, f: bytes):
        assert len(f) == len(self.files[row])
        o = self.offs[row]
        self.data[o:o + len(f)] = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
        self.files[row] = f


class Rig:
    def __init__(self, **kw):
        from sds_amd.engine import JpegEngine
        from tests.golden.synth import encode_jpeg
        self.engine = JpegEngine(**{"max_batch": 256, **kw})
        rng = np.random.default_rng(2024)
        self.noise = [encode_jpeg(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), 95) for _ in range(2)] * 6

    def dirty(self):
        _, st = self.engine.decode_resize(self.noise, (32, 32))
        assert (st == 0).all()

    def run(self, blob: Blob, rows=None, check=True):
        """One device-resident call over the rows: (pixels, statuses, descriptors, what the store's counters
        grew by); statuses and pixels are compared with the oracle."""
        rows = list(range(len(blob.files))) if rows is None else list(rows)
        self.dirty()
        c0 = self.engine.counters()
        out, st = self.engine.decode_resize_device(*blob.args(rows), RES)
        descs, _ = gpu_debug.snapshot(self.engine, min(len(rows), self.engine.max_batch))
        c1 = self.engine.counters()
        got, st = out.cpu().numpy(), st.cpu().numpy()
        if check:
            for k, r in enumerate(rows):
                ost, ref = oracle(blob.files[r])
                assert int(st[k]) == ost, f"row {r}: status {int(st[k])} vs oracle {ost}"
                if ost == O.OK:
                    np.testing.assert_array_equal(got[k], ref, err_msg=f"row {r}")
        return got, st, descs, {k: c1[k] - c0[k] for k in HINT_KEYS}


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Rig()


def E_route11(d) -> bool:
    """At most 4 Huffman table slots (the 11-bit route): DC keys td, AC keys 4 | ta of the scan's components."""
    keys = set()
    for c in range(d.ncomp):
        keys |= {d.comp[c].td, 4 | d.comp[c].ta}
    return len(keys) <= 4


def test_same_blob_twice(rig):
    """Both calls equal the oracle; the second decodes every row from its record, all proved."""
    blob = Blob([small(100 + k) for k in range(N)])
    _, _, descs, c = rig.run(blob)
    assert all(d.nsub >= 4 and d.ent_groups == 1 for d in descs)
    assert c == {"hint_hits": 0, "hint_misses": N, "hint_verify_failed": 0, "hint_stored": N}
    _, _, descs2, c = rig.run(blob)
    assert c == {"hint_hits": N, "hint_misses": 0, "hint_verify_failed": 0, "hint_stored": 0}
    assert [d.nsub for d in descs2] == [d.nsub for d in descs]


def test_shared_table_444_restores_sync_statistics(rig):
    """The 4:4:4 scan whose components share one table pair (tests/entropy_cases.py sync_control_444): nothing in
    the stream tells the MCU phase, so the sync pass has work; a hit gives the same pixels and puts the stored
    sync_rounds / pad0 back into the descriptor."""
    case = next(c for c in E.CASES if c.name == "sync_control_444")
    blob = Blob([E.case_image(case)] * 3 + [small(200 + k) for k in range(N - 3)])
    _, _, d1, c = rig.run(blob)
    assert c["hint_stored"] == N and all(d.nsub >= 4 for d in d1)
    assert d1[0].sync_rounds >= 1 and d1[0].pad0 >= 1
    _, _, d2, c = rig.run(blob)
    assert c["hint_hits"] == N and c["hint_verify_failed"] == 0
    assert [(d.sync_rounds, d.pad0) for d in d2] == [(d.sync_rounds, d.pad0) for d in d1]


def test_restart_intervals_and_grayscale(rig):
    """Several exact entries per image (one per restart interval), intervals of one to three subsequences, and a
    single-component scan."""
    varied = next(c for c in E.CASES if c.name == "seg_first_64")
    rst_coef = next(c for c in E.CASES if c.name == "mh_off_420_restart")
    files = [E.case_image(varied), E.case_image(rst_coef), small(7, gray=True), small(8, gray=True, rst=2), small(9, rst=3)]
    blob = Blob(files + [small(300 + k) for k in range(N - len(files))])
    _, _, d1, c = rig.run(blob)
    assert c["hint_stored"] == N and all(d.nsub >= 4 for d in d1)
    assert d1[0].nseg > 1 and d1[1].nseg > 1 and d1[2].ncomp == 1 and d1[3].ncomp == 1 and d1[3].nseg > 1 and d1[4].nseg > 1
    _, _, _, c = rig.run(blob)
    assert c == {"hint_hits": N, "hint_misses": 0, "hint_verify_failed": 0, "hint_stored": 0}


def _coef_pair(kind: str):
    """Two 4:4:4 files written from coefficients that differ in one bit of the scan: the lowest value bit of one AC
    coefficient ("ac") or of one DC difference ("dc": every later block of the component moves with it, so only that
    difference changes), in a block a quarter of the way in.  Same Huffman codes, same length."""
    from tests.golden.coefjpeg import write_jpeg
    w, h = 96, 80
    base = E.coef_blocks(31, w, h, E.S444, 12, 40)
    a = write_jpeg(w, h, E.S444, base, E.Q)
    bw = base[0].shape[1]
    n = base[0].shape[0] * bw
    for k in range(n // 4, n // 2):
        blocks = [b.copy() for b in base]
        y, x = divmod(k, bw)
        if kind == "ac":
            nz = [p for p in range(1, 64) if abs(base[0][y, x, p]) >= 2 and base[0][y, x, p] % 2 == 0]
            if not nz:
                continue
            blocks[0][y, x, nz[0]] += int(np.sign(base[0][y, x, nz[0]]))
        else:
            flat = base[0][..., 0].reshape(-1)
            d = int(flat[k] - flat[k - 1])
            if abs(d) < 2 or d % 2:
                continue
            moved = flat.copy()
            moved[k:] += int(np.sign(d))
            blocks[0][..., 0] = moved.reshape(base[0].shape[:2])
        b = write_jpeg(w, h, E.S444, blocks, E.Q)
        if len(b) == len(a) and sum(p != q for p, q in zip(a, b)) == 1:
            return a, b
    raise AssertionError("no such pair")


def _flip_late(jpg: bytes) -> bytes:
    """One byte of the scan changed (five of its bits) at about 85 % of it, away from any FF."""
    off = E.entropy_off(jpg)
    i = off + (len(jpg) - off) * 85 // 100
    while 0xFF in jpg[i - 1:i + 2] or (jpg[i] ^ 0x5B) == 0xFF:
        i += 1
    return jpg[:i] + bytes([jpg[i] ^ 0x5B]) + jpg[i + 1:]


def test_content_replaced_in_place(rig):
    """The same addresses and lengths, other bytes: whatever the records say, statuses and pixels are those of the
    bytes now there, and the next call hits again."""
    longer, shorter = sorted((small(401), small(402)), key=len, reverse=True)
    ac0, ac1 = _coef_pair("ac")
    dc0, dc1 = _coef_pair("dc")
    late = small(403)
    files = [longer, late, ac0, dc0] + [small(410 + k) for k in range(N - 4)]
    blob = Blob(files)
    _, _, d1, c = rig.run(blob)
    assert c["hint_stored"] == N and all(d.nsub >= 4 for d in d1)
    # another image, padded to the length after its EOI; a byte flipped late in the scan; one AC value bit; one
    # bit of a DC difference
    blob.put(0, shorter + bytes(len(longer) - len(shorter)))
    blob.put(1, _flip_late(late))
    blob.put(2, ac1)
    blob.put(3, dc1)
    assert oracle(ac1)[0] == O.OK and oracle(dc1)[0] == O.OK
    assert not np.array_equal(oracle(dc0)[1], oracle(dc1)[1])
    _, st, _, c = rig.run(blob)
    print("replaced in place:", c, "statuses", st[:4])
    # the AC value bit leaves every entry state as it was: proved, decoded from the record.  The DC difference
    # cannot pass, the late flip fails in the lane it lands in or a later one; the other image has another
    # layout (a miss) or fails.  (A sample that does not decode is neither looked up nor recorded.)
    ok = int((st == 0).sum())
    assert c["hint_hits"] == N - 3, c
    assert c["hint_verify_failed"] + c["hint_misses"] == ok - (N - 3) and c["hint_verify_failed"] >= int(st[1] == 0) + 1, c
    assert c["hint_stored"] == ok - c["hint_hits"]
    _, st2, _, c = rig.run(blob)
    assert (st2 == st).all()
    assert c == {"hint_hits": ok, "hint_misses": 0, "hint_verify_failed": 0, "hint_stored": 0}, c


def test_same_offset_twice_and_overlapping_windows():
    """512-image calls (four lanes) whose row windows overlap, each holding some rows twice: lanes look records
    up while others write them."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rig = Rig(max_batch=512)
    kinds = [small(500 + k) for k in range(8)]
    blob = Blob([kinds[k % 8] for k in range(768)])
    win1 = list(range(496)) + list(range(16))       # rows 0..15 twice
    win2 = list(range(256, 752)) + list(range(256, 272))
    _, _, d, c = rig.run(blob, win1)
    # (a doubled row's second copy, in the last lane, may find the record the first lane is writing: whole, torn
    # -- refuted by the write pass -- or not yet there)
    assert all(x.nsub >= 4 for x in d) and c["hint_hits"] + c["hint_verify_failed"] <= 16, c
    _, _, _, c = rig.run(blob, win2)
    assert c == {"hint_hits": 256, "hint_misses": 256, "hint_verify_failed": 0, "hint_stored": 256}, c  # rows 256..495, 16 twice
    _, _, _, c = rig.run(blob, win2)
    assert c == {"hint_hits": 512, "hint_misses": 0, "hint_verify_failed": 0, "hint_stored": 0}, c
    _, _, _, c = rig.run(blob, win1)
    assert c["hint_hits"] == 512 and c["hint_verify_failed"] == 0, c


def test_store_smaller_than_the_rows_offered():
    """20 rows of store, 40 distinct rows: at most 20 records, at most 20 hits, everything exact."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rig = Rig(hint_rows=N // 2)
    blob = Blob([small(600 + k) for k in range(N)])
    _, _, _, c = rig.run(blob)
    assert c["hint_misses"] == N and 0 < c["hint_stored"] <= N // 2
    stored = c["hint_stored"]
    _, _, _, c = rig.run(blob)
    assert c["hint_hits"] == stored and c["hint_misses"] == N - stored and c["hint_verify_failed"] == 0
    assert c["hint_stored"] == 0
    rig.engine.clear_hints()
    _, _, _, c = rig.run(blob)
    assert c["hint_hits"] == 0 and c["hint_misses"] == N


def test_ineligible_samples_leave_no_record(rig):
    """Progressive, the 10-bit route and multi-group images through the device path, a latency-mode host call of 8
    images and a host call of 40: no lookup, no record, the same outputs."""
    from tests.golden.synth import encode_jpeg
    rng = np.random.default_rng(5)
    prog = encode_jpeg(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), 90, progressive=True)
    ten = E.case_image(next(c for c in E.CASES if c.name == "six_slot_restart"))
    multi = E.case_image(next(c for c in E.CASES if c.name == "noise_d_256x256_norst"))
    blob = Blob([prog, ten, multi] * 13 + [prog])
    for _ in range(2):
        _, _, d, c = rig.run(blob)
        assert c == dict.fromkeys(HINT_KEYS, 0), c
    assert d[0].progressive == 1 and not E_route11(d[1]) and d[2].ent_groups > 1
    files = [small(700 + k) for k in range(N)]
    for chunk in (files[:8], files):
        c0 = rig.engine.counters()
        for _ in range(2):
            out, st = rig.engine.decode_resize(chunk, RES)
            for k, f in enumerate(chunk):
                assert int(st[k]) == 0
                np.testing.assert_array_equal(out[k].cpu().numpy(), oracle(f)[1])
        c1 = rig.engine.counters()
        assert all(c1[k] == c0[k] for k in HINT_KEYS)


@pytest.mark.parametrize("how", ["hint_rows", "env"])
def test_store_off(rig, how):
    """hint_rows=0 and SDSJ_HINTS=0: counters stay zero, outputs identical to the enabled engine's."""
    blob = Blob([small(800 + k) for k in range(N)])
    want, st_want, _, _ = rig.run(blob)
    old = os.environ.get("SDSJ_HINTS")
    try:
        if how == "env":
            os.environ["SDSJ_HINTS"] = "0"
        off = Rig(**({"hint_rows": 0} if how == "hint_rows" else {}))
    finally:
        if how == "env":
            os.environ.pop("SDSJ_HINTS") if old is None else os.environ.__setitem__("SDSJ_HINTS", old)
    for _ in range(2):
        got, st, _, c = off.run(blob)
        assert c == dict.fromkeys(HINT_KEYS, 0), c
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(st, st_want)
