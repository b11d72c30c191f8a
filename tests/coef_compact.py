"""Coefficient blocks of a ``tests.gpu_debug.snapshot`` in either device format (test infrastructure).

Mirrors ``coef_compact`` / ``coef_dc_off`` / ``coef_hi_off`` of sds_amd/csrc/sdsj_common.h: baseline images
of at most 4 Huffman table slots keep 64-byte main slots (a word of flag, DC and AC 63 bits, then AC 1..62 as
bytes) and, per flagged block, an int16 DC and a hi slot; progressive images and the 10-bit entropy route keep
128-byte int16 blocks.  ``gpu_debug.stage_report`` reads the 128-byte format only; this module reads both into
``[N, 64]`` int16 in zigzag order.
"""
from __future__ import annotations

import numpy as np

from tests.golden.coefjpeg import ZIGZAG_TO_NATURAL


def _align(v: int, a: int = 256) -> int:
    return (v + a - 1) // a * a


def huff_slots(d) -> int:
    keys = set()
    for c in range(d.ncomp):
        keys.add(d.comp[c].td)
        keys.add(4 | d.comp[c].ta)
    return len(keys)


def is_compact(d) -> bool:
    return not d.progressive and not d.png and not d.lat and huff_slots(d) <= 4


def read_blocks(d, fetch):
    """(coefficients [N, 64] int16 in zigzag order and decode order, flagged [N] bool) of image ``d``."""
    n = int(d.total_blocks)
    if not is_compact(d):
        return fetch(d.off_coef, n * 128).view(np.int16).reshape(n, 64).copy(), np.zeros(n, bool)
    dc_off = _align(n * 64)
    hi_off = dc_off + _align(n * 2)
    main = fetch(d.off_coef, n * 64).reshape(n, 64)
    dc = fetch(d.off_coef + dc_off, n * 2).view(np.int16)
    hi = fetch(d.off_coef + hi_off, n * 64).reshape(n, 64)
    flagged = (main[:, 0] & 1) == 1
    word = main[:, :2].copy().view(np.uint16)[:, 0].astype(np.int32)  # flag | DC (11 bits) << 1 | AC 63 (4 bits) << 12
    sext = lambda v, bits: ((v & ((1 << bits) - 1)) ^ (1 << (bits - 1))) - (1 << (bits - 1))  # noqa: E731
    val = np.zeros((n, 64), np.int32)
    val[:, 0] = sext(word >> 1, 11)
    val[:, 1:63] = main[:, 2:64].view(np.int8)  # AC k's low byte at byte k + 1
    val[:, 63] = sext(word >> 12, 4)
    h = hi.view(np.int8).astype(np.int32)
    val[flagged, 1:63] += h[flagged, 1:63] << 8
    val[flagged, 63] += (h[flagged, 0] + (h[flagged, 63] << 8)) << 4  # (hi[0]: the low byte, sign-extended too)
    zz = val.astype(np.int16)  # (the 16-bit wrap)
    zz[flagged, 0] = dc[flagged]
    return zz, flagged


def blocks_differing_from_oracle(d, zz, jpg: bytes) -> list[int]:
    """Per component, how many of its blocks differ from the oracle's coefficients (as stage_report counts)."""
    from oracle import oracle as O
    coef = np.zeros_like(zz)
    coef[:, ZIGZAG_TO_NATURAL] = zz
    out = []
    for c in range(d.ncomp):
        ref = O.coefficients(jpg, c)  # [bh][bw][64], natural order
        got = np.zeros_like(ref)
        g = 0
        for m in range(d.mcux * d.mcuy):
            mx, my = m % d.mcux, m // d.mcux
            for b in range(d.bpm):
                cc = d.blk_comp[b]
                if d.ncomp == 1:
                    bx, by = mx, my
                else:
                    bx, by = mx * d.comp[cc].h + d.blk_dx[b], my * d.comp[cc].v + d.blk_dy[b]
                if cc == c:
                    got[by, bx] = coef[g]
                g += 1
        out.append(int((got != ref).any(-1).sum()))
    return out
