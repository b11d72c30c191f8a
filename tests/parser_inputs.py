"""Damaged JPEG inputs of the sanitized host drivers (test infrastructure, shared by
tests/test_asan_parser.py and tests/test_plan_host.py): every G1/G5 golden JPEG whole, truncated at every
byte of its headers and with bytes of its headers overwritten, and a few streams that are no JPEG."""
import base64
import functools

import numpy as np

from tests import goldens as G


@functools.lru_cache(maxsize=None)
def inputs() -> tuple:
    out = []
    rng = np.random.default_rng(5)
    for case, jpg, _ in G.g1():
        out.append(jpg)
    for c in G.load_json("g5_edge.json")["cases"]:
        out.append(base64.b64decode(c["jpg_b64"]))
    muts = []
    for jpg in out:
        from oracle import oracle as O  # locates the entropy segment only (test infrastructure)
        _, info = O.probe(jpg)
        hdr_end = int(info.entropy_offset) or min(len(jpg), 700)
        for k in range(0, hdr_end + 2):
            muts.append(jpg[:k])
        for _ in range(40):
            b = bytearray(jpg)
            p = int(rng.integers(0, hdr_end))
            b[p] = int(rng.integers(0, 256))
            muts.append(bytes(b))
    return tuple(out + muts + [b"", b"\x89PNG\r\n\x1a\n" + b"\x00" * 32, b"\xff\xd8", b"\xff\xd8\xff"])
