"""Synthetic PNG files for SDSJ_FORMAT_PNG_META ("png-meta"): iCCP, zTXt and iTXt chunks and chunks after the
image data.  Test infrastructure on top of tests/png_synth.py and tests/png_ext_synth.py.

ANCHORS are the outcomes observed with Pillow 12.2.0 on a 5 x 3 RGB file; every test that uses them asks PIL
again (S.pil_outcome), so the table cannot drift from the reference.  `native` is what the rule of
sds_amd/csrc/sdsj_png.h gives under mask 19 (JPEG | PNG | PNG_META; 23 where the name ends in _ext): True =
SDSJ_OK, False = handed to PIL.  PIL accepts three cases the rule hands over on purpose: the profile of
exactly 1,048,576 bytes, and the garbage and the truncated stream (zlib.error is swallowed there; the count-
only inflate accepts only streams that are well formed up to the end of a final block).

b"a" * 1,048,577 deflates to about 1 KB, so every case is cheap."""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np

from tests import png_ext_synth as E
from tests import png_synth as S

MIB = 1 << 20
TIME = struct.pack(">HBBBBB", 2024, 2, 29, 12, 30, 59)


def zbytes(n: int) -> bytes:
    return S.zstream(b"a" * n)


def iccp(z: bytes, name=b"icc", method=0) -> bytes:
    return name + b"\0" + bytes([method]) + z


def ztxt(z: bytes, key=b"Comment", method=0) -> bytes:
    return key + b"\0" + bytes([method]) + z


def itxt(text: bytes, key=b"XML:com.adobe.xmp", comp=0, method=0, lang=b"", tk=b"") -> bytes:
    return key + b"\0" + bytes([comp, method]) + lang + b"\0" + tk + b"\0" + text


def rgb53(pre=(), post=(), **kw) -> bytes:
    """The 5 x 3 RGB file of the anchors."""
    return S.make(5, 3, 2, "mixP", pre=list(pre), post=list(post), **kw)


def _anchors():
    z = zbytes(MIB - 1)
    big = zbytes(MIB + 1)
    garbage = bytes(np.random.default_rng(5).integers(0, 256, 300, dtype=np.uint8))
    many = lambda k: [(b"zTXt", ztxt(z, b"k%d" % i)) for i in range(k)]  # noqa: E731
    return [
        # name, file, PIL's outcome, native
        ("iccp_1048575", rgb53([(b"iCCP", iccp(z))]), "ok", True),
        ("iccp_1048576", rgb53([(b"iCCP", iccp(zbytes(MIB)))]), "ok", False),
        ("iccp_1048577", rgb53([(b"iCCP", iccp(big))]), "err", False),
        ("iccp_garbage", rgb53([(b"iCCP", iccp(garbage))]), "ok", False),
        ("iccp_cut9", rgb53([(b"iCCP", iccp(zbytes(5000)[:-9]))]), "ok", False),
        ("iccp_method1", rgb53([(b"iCCP", iccp(z, method=1))]), "err", False),
        ("iccp_no_nul", rgb53([(b"iCCP", b"icc")]), "err", False),
        ("iccp_empty", rgb53([(b"iCCP", b"")]), "err", False),
        ("ztxt_1048577", rgb53([(b"zTXt", ztxt(big))]), "err", False),
        ("itxt_z_1048577", rgb53([(b"iTXt", itxt(big, comp=1))]), "err", False),
        ("itxt_bad_utf8", rgb53([(b"iTXt", itxt(b"\xff\xfe\xfd"))]), "ok", True),
        ("ztxt_x63", rgb53(many(63)), "ok", True),
        ("ztxt_x65", rgb53(many(65)), "err", False),
        ("ztxt_x33_x33", rgb53(many(33), many(33)), "err", False),
        ("post_text_bad_crc", rgb53(post=[(b"tEXt", b"k\0v")], bad_crc="tEXt"), "ok", True),
        ("post_time_ext", rgb53(post=[(b"tIME", TIME)]), "ok", True),
        ("post_ztxt_1048577", rgb53(post=[(b"zTXt", ztxt(big))]), "err", False),
        ("post_iccp_1048577", rgb53(post=[(b"iCCP", iccp(big))]), "err", False),
        ("post_trns_short", rgb53(post=[(b"tRNS", b"\0\1")]), "err", False),
        ("post_gama_short", rgb53(post=[(b"gAMA", b"\0\1")]), "err", False),
        ("post_phys_short", rgb53(post=[(b"pHYs", b"\0\1\2")]), "err", False),
    ]


_CACHE: dict = {}


def anchors():
    if "anchors" not in _CACHE:
        _CACHE["anchors"] = _anchors()
    return _CACHE["anchors"]


def mask_for(name: str) -> int:
    return 23 if name.endswith("_ext") else 19


def realistic() -> bytes:
    """A file as an editor exports it: saved by PIL with an ICC profile of about 3 KB (arbitrary bytes: PIL does
    not parse them), a compressed iTXt XMP-like packet, a tEXt, and a tEXt and a tIME after the image data."""
    from PIL import Image
    from PIL.PngImagePlugin import PngInfo
    rng = np.random.default_rng(7)
    im = Image.fromarray(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "RGB")
    info = PngInfo()
    info.add_itxt("XML:com.adobe.xmp", "<x:xmpmeta>" + "".join(f"<rdf:li>{i}</rdf:li>" for i in range(300)) + "</x:xmpmeta>", zip=True)
    info.add_text("Software", "an editor")
    b = io.BytesIO()
    im.save(b, "PNG", icc_profile=rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), pnginfo=info)
    data = b.getvalue()
    k = data.rindex(b"IEND") - 4
    return data[:k] + S.chunk(b"tEXt", b"Comment\0after the data") + S.chunk(b"tIME", TIME) + data[k:]


# ---------------------------------------------------------------------------------------------
# the corpus: small files the rule accepts, one chunk form each
# ---------------------------------------------------------------------------------------------
def profile(n=3000, seed=3) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def corpus_chunks():
    """(name, tag, payload) of chunk forms PIL accepts and the rule accepts natively."""
    rnd = profile(70000)  # incompressible: several dynamic blocks, long codes
    return [
        ("iccp_small", b"iCCP", iccp(S.zstream(profile(200)))),
        ("iccp_stored", b"iCCP", iccp(S.zstream(profile(300), 0))),
        ("iccp_fixed", b"iCCP", iccp(S.zstream(b"profile " * 40, 6, zlib.Z_FIXED))),
        ("iccp_blocks", b"iCCP", iccp(S.zstream(rnd, 6, piece=9000, flush=zlib.Z_FULL_FLUSH))),
        ("iccp_noname", b"iCCP", iccp(S.zstream(b"x" * 50), name=b"")),
        ("ztxt", b"zTXt", ztxt(S.zstream(b"compressed text " * 9))),
        ("ztxt_no_nul", b"zTXt", b"keyonly"),
        ("ztxt_nul_last", b"zTXt", b"key\0"),
        ("ztxt_nokey", b"zTXt", ztxt(S.zstream(b"text"), key=b"")),
        ("itxt_plain", b"iTXt", itxt("grüße".encode(), key=b"Title", lang=b"de", tk=b"Titel")),
        ("itxt_z", b"iTXt", itxt(S.zstream(b"<xmp>" + b"packet " * 60 + b"</xmp>"), comp=1)),
        ("itxt_no_nul", b"iTXt", b"keyonly"),
        ("itxt_short", b"iTXt", b"key\0\1"),
        ("itxt_one_nul", b"iTXt", b"key\0\0\0lang-without-end"),
        ("itxt_method1", b"iTXt", itxt(b"whatever", comp=1, method=1)),
        ("itxt_z_garbage_flagless", b"iTXt", itxt(b"\x01\x02\x03", comp=0)),
        ("text", b"tEXt", b"Comment\0plain"),
    ]


def corpus():
    """(name, file): each chunk form before the image data and after it, 5 x 3 RGB."""
    out = []
    for name, tag, payload in corpus_chunks():
        out.append((name + "_pre", rgb53([(tag, payload)])))
        out.append((name + "_post", rgb53(post=[(tag, payload)], idat_sizes=[7])))
    return out


def mutations(per_chunk=12, seed=29):
    """Single-byte overwrites of the chunk payloads, the CRC recomputed (before the image data PIL checks it): each
    chunk form before and after the image data, plus the compressed streams at the size limit."""
    rng = np.random.default_rng(seed)
    forms = corpus_chunks() + [("iccp_1048575", b"iCCP", iccp(zbytes(MIB - 1))), ("ztxt_1048577", b"zTXt", ztxt(zbytes(MIB + 1))),
                               ("itxt_z_1048575", b"iTXt", itxt(zbytes(MIB - 1), comp=1))]
    out = []
    for name, tag, payload in forms:
        if not payload:
            continue
        for k in range(per_chunk):
            b = bytearray(payload)
            # half of the overwrites in the first 24 bytes (keyword, NULs, flags, zlib and block headers)
            hi = min(len(b), 24) if k % 2 == 0 else len(b)
            b[int(rng.integers(0, hi))] = int(rng.integers(0, 256))
            where = "pre" if k % 3 else "post"
            data = rgb53([(tag, bytes(b))]) if where == "pre" else rgb53(post=[(tag, bytes(b))])
            out.append((f"{name}_{where}_m{k}", data))
    return out


# ---------------------------------------------------------------------------------------------
# files for the GPU tests
# ---------------------------------------------------------------------------------------------
def assemble(w, h, ctype, z, *, plte=None, before_plte=(), pre=(), post=(), idat_sizes=None) -> bytes:
    """S.write_png with chunks before PLTE too."""
    out = [S.SIG, S.chunk(b"IHDR", S.ihdr(w, h, ctype))]
    out += [S.chunk(t, d) for t, d in before_plte]
    if plte is not None:
        out.append(S.chunk(b"PLTE", plte))
    out += [S.chunk(t, d) for t, d in pre]
    out += [S.chunk(b"IDAT", p) for p in S.split_idat(z, idat_sizes)]
    out += [S.chunk(t, d) for t, d in post]
    out.append(S.chunk(b"IEND", b""))
    return b"".join(out)


META_SIZES = [(1, 1), (13, 7), (67, 5), (64, 65)]


def meta_file(w, h, ctype, seed=0) -> bytes:
    """One image with a profile of about 3 KB before PLTE (before the image data for RGB), a compressed XMP-like
    iTXt, a zTXt and a tEXt between PLTE and IDAT, and a tEXt, a zTXt and a gAMA after an IDAT run split in
    pieces of 50 bytes."""
    pix = S.pixels(w, h, ctype, seed)
    raw = S.scanlines(pix, S.BPP[ctype], S.schedule("mixP", h))
    plte = np.random.default_rng(seed + 11).integers(0, 256, 200 * 3, dtype=np.uint8).tobytes() if ctype == 3 else None
    head = [(b"iCCP", iccp(S.zstream(profile(3000, seed))))]
    mid = [(b"iTXt", itxt(S.zstream(b"<x:xmpmeta>" + b"<rdf:li>item</rdf:li>" * 200 + b"</x:xmpmeta>"), comp=1)),
           (b"zTXt", ztxt(S.zstream(b"zipped " * 30))), (b"tEXt", b"Software\0synthetic")]
    post = [(b"tEXt", b"Comment\0after the data"), (b"zTXt", ztxt(S.zstream(b"late " * 20), b"Late")), (b"gAMA", struct.pack(">I", 45455))]
    return assemble(w, h, ctype, S.zstream(raw), plte=plte, before_plte=head, pre=mid, post=post, idat_sizes=[50])


def meta_files():
    """(name, file) for META_SIZES x colour types 2 and 3."""
    return [(f"meta_t{ct}_{w}x{h}", meta_file(w, h, ct, seed=ct + w)) for ct in (2, 3) for (w, h) in META_SIZES]


def meta_adam7_16() -> bytes:
    """An Adam7 RGBA 16-bit file with the same kinds of chunks and a tIME on both sides (mask 23)."""
    pre = [(b"iCCP", iccp(S.zstream(profile(3000)))), (b"tIME", TIME), (b"iTXt", itxt(S.zstream(b"packet " * 100), comp=1))]
    post = [(b"tEXt", b"Comment\0after"), (b"tIME", TIME)]
    return E.make(13, 7, 6, 16, 1, "mixA", pre=pre, post=post, idat_sizes=[40])[0]
