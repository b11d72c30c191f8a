"""Helpers to load the committed golden vectors (tests/golden/, made by make_golden.py)."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a) -> str:
    if isinstance(a, (bytes, bytearray)):
        return hashlib.sha256(a).hexdigest()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


PART_LIMIT = 900 << 10  # bytes per stored archive part (committed files stay under 1 MiB)


class NpzParts:
    """The arrays of one golden archive stored as ``<name>.0.npz``, ``<name>.1.npz``, ...: ``files`` and
    ``[key]`` as numpy's NpzFile has them."""

    def __init__(self, name: str):
        stem = os.path.join(GOLDEN, name)
        self._parts = []
        while os.path.exists(f"{stem}.{len(self._parts)}.npz"):
            self._parts.append(np.load(f"{stem}.{len(self._parts)}.npz"))
        if not self._parts:
            raise FileNotFoundError(f"{stem}.0.npz")
        self._where = {k: p for p in self._parts for k in p.files}
        self.files = list(self._where)

    def __getitem__(self, key: str):
        return self._where[key][key]


def load_npz(name: str) -> NpzParts:
    return NpzParts(name)


def save_npz(name: str, arrays: dict) -> list[str]:
    """Writes `arrays` as ``<name>.<k>.npz`` parts (compressed) of at most PART_LIMIT bytes each, arrays in
    the given order; returns the file names (the generators call this)."""
    import io
    parts, cur, size = [], {}, 0
    for k, a in arrays.items():
        buf = io.BytesIO()
        np.savez_compressed(buf, **{k: a})
        n = buf.getbuffer().nbytes
        if n > PART_LIMIT:
            raise ValueError(f"{k}: {n} bytes compressed, over the {PART_LIMIT}-byte part limit")
        if cur and size + n > PART_LIMIT:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += n
    parts.append(cur)
    names = []
    for i, p in enumerate(parts):
        names.append(f"{name}.{i}.npz")
        np.savez_compressed(os.path.join(GOLDEN, names[-1]), **p)
    return names


def g1():
    """Yields (case dict, jpg bytes, arrays dict) for each G1 case."""
    with open(os.path.join(GOLDEN, "g1_cases.json")) as f:
        cases = json.load(f)
    z = load_npz("g1_small")
    for c in cases:
        name = c["name"]
        jpg = z[f"{name}__jpg"].tobytes()
        arrs = {k[len(name) + 2:]: z[k] for k in z.files if k.startswith(name + "__")}
        yield c, jpg, arrs


def load_json(name: str):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def g2_jpegs():
    from tests.golden.synth import synth_jpegs
    meta = load_json("g2_synth.json")
    jpgs = synth_jpegs(len(meta["images"]), seed=meta["seed"], w=meta["w"], h=meta["h"], quality=meta["quality"])
    return meta, jpgs


def g3_jpegs():
    from tests.golden.synth import encode_jpeg, synth_rgb
    meta = load_json("g3_mixed.json")
    rng = np.random.default_rng(777)
    jpgs = [encode_jpeg(synth_rgb(rng, im["w"], im["h"]), 90) for im in meta["images"]]
    return meta, jpgs
