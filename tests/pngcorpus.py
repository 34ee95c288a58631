"""A small PNG writer with exact control over filters, zlib level / strategy and IDAT splitting, and the corpora the PNG
decoder tests use (tests/test_png_cpu.py, tests/test_gpu_png.py).  The expected pixels of every file are the writer's input."""
import random
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


def chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data) & 0xffffffff)


def compress(raw, level=6, strategy="default"):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, STRATEGIES[strategy])
    return c.compress(raw) + c.flush()


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, bpp, filters):
    """img: [H, row bytes] uint8 -> the filtered scanlines (filter byte + row) as bytes."""
    h, rb = img.shape
    out = bytearray()
    prev = np.zeros(rb, np.int32)
    for y in range(h):
        cur = img[y].astype(np.int32)
        f = filters[y]
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        upleft = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        left, upleft = left[:rb], upleft[:rb]
        if f == 0:
            v = cur
        elif f == 1:
            v = cur - left
        elif f == 2:
            v = cur - prev
        elif f == 3:
            v = cur - (left + prev) // 2
        else:
            v = cur - _paeth(left, prev, upleft)
        out.append(f)
        out += (v & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def write_png(pix, color_type, bit_depth=8, filters=None, level=6, strategy="default", split=None, seed=0,
              interlace=0, palette=None, zdata=None):
    """pix: [H, W] (gray), [H, W, 3] (RGB), [H, W, 4] (RGBA), [H, W, 2] (gray + alpha), uint8 or (16-bit) uint16.
    filters: an int 0-4 for every row, 'random', or None (0).  split: None (one IDAT), an int (chunk size) or 'random'."""
    pix = np.asarray(pix)
    h, w = pix.shape[:2]
    ch = 1 if pix.ndim == 2 else pix.shape[2]
    if bit_depth == 16:
        rows = pix.astype(">u2").reshape(h, w * ch).view(np.uint8).reshape(h, w * ch * 2)
    else:
        rows = pix.astype(np.uint8).reshape(h, w * ch)
    bpp = max(1, ch * bit_depth // 8)
    rng = random.Random(seed)
    if filters is None:
        filters = [0] * h
    elif filters == "random":
        filters = [rng.randrange(5) for _ in range(h)]
    elif isinstance(filters, int):
        filters = [filters] * h
    if zdata is None:
        zdata = compress(filter_rows(rows, bpp, filters), level, strategy)
    if split is None:
        parts = [zdata]
    else:
        parts, i = [], 0
        while i < len(zdata):
            n = split if isinstance(split, int) else rng.randrange(1, 5000)
            parts.append(zdata[i:i + n])
            i += n
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, color_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", palette)
    out += chunk(b"tEXt", b"Comment\x00pngcorpus")  # an ancillary chunk to skip
    for p in parts:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"")


def as_bgr8(pix):
    """What tum.load_frame's colour path (PIL convert('RGB') + RGB->BGR) gives for these pixels."""
    pix = np.asarray(pix, np.uint8)
    if pix.ndim == 2:
        return np.repeat(pix[..., None], 3, axis=2)
    if pix.shape[2] == 2:
        return np.repeat(pix[..., :1], 3, axis=2)
    return np.ascontiguousarray(pix[..., 2::-1])


def noisy_rgb(rng, h, w, sigma=6.0):
    """A smooth render plus sensor-like noise (camera images compress far worse than noise-free renders)."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(x / 37.0 + c) * np.cos(y / 23.0 - c) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, sigma, base.shape), 0, 255).astype(np.uint8)


def zlib_corpus():
    """(name, raw bytes, zlib stream) cases that stress the inflater."""
    rng = np.random.default_rng(7)
    cases = []
    geo = np.minimum(rng.geometric(0.35, 200000), 255).astype(np.uint8).tobytes()  # skewed: Huffman-only gives 15-bit codes
    cases.append(("huffman_only_geometric", geo, compress(geo, 9, "huffman")))
    period = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    rep = period * 4  # a level-9 stream of a 32768-byte period (zlib's encoder reaches back 32768 - 262 bytes at most)
    cases.append(("period_32768_l9", rep, compress(rep, 9)))
    cases.append(("dist_32768_len_258", period + period[:258 * 40], far_matches(period, 40)))
    runs = b"\x00" * 5000 + b"\x07" * 3000 + bytes(range(256)) * 4 + b"\xff" * 777
    cases.append(("distance_1_runs", runs, compress(runs, 6)))
    cases.append(("empty", b"", compress(b"", 6)))
    # empty stored blocks around data: a full flush writes an empty stored block
    c = zlib.compressobj(1)
    z = c.compress(b"abc" * 100) + c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(b"xyz" * 50) + c.flush()
    cases.append(("empty_stored_blocks", b"abc" * 100 + b"xyz" * 50, z))
    noise = rng.integers(0, 256, 100000, dtype=np.uint8).tobytes()
    text = b"".join(b"line %d of some text, with repeats %d\n" % (i, i % 17) for i in range(3000))
    for name, raw in (("noise", noise), ("text", text), ("geometric", geo[:50000])):
        for level in (0, 1, 6, 9):
            for strat in STRATEGIES:
                cases.append(("%s_l%d_%s" % (name, level, strat), raw, compress(raw, level, strat)))
    big_stored = rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()  # stored blocks > 64 KiB are split by zlib
    cases.append(("stored_200k", big_stored, compress(big_stored, 0)))
    return cases


def bad_streams():
    """(name, zlib stream, expected output length): inputs the inflater must reject."""
    raw = b"".join(b"row %d %s\n" % (i, b"x" * (i % 40)) for i in range(2000))
    good = compress(raw, 9)
    n = len(raw)
    out = []
    for cut in (0, 1, 2, 3, 10, len(good) // 2, len(good) - 5, len(good) - 1):
        out.append(("truncated_%d" % cut, good[:cut], n))
    # a flipped bit in a dynamic block header (byte 2 is the first block's header: BFINAL, BTYPE, HLIT, ...)
    for byte, bit in ((2, 3), (3, 0), (4, 5), (5, 2), (6, 7), (8, 1)):
        b = bytearray(good)
        b[byte] ^= 1 << bit
        out.append(("flip_%d_%d" % (byte, bit), bytes(b), n))
    # a distance before the start of the output: fixed block, literal 'a', then length 3 at distance 2
    bw = _BitWriter()
    bw.put(1, 1); bw.put(1, 2)
    bw.huff(0x30 + ord("a"), 8)
    bw.huff(0x01, 7)          # symbol 257 (length 3): code 0000001
    bw.huff(0x01, 5)          # distance symbol 1 (distance 2)
    bw.huff(0x00, 7)          # end of block
    body = bw.done()
    zh = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(b"aaa"))
    out.append(("distance_before_start", zh, 4))
    b = bytearray(good)
    b[-1] ^= 0x10
    out.append(("adler_mismatch", bytes(b), n))
    out.append(("fdict", b"\x78\x20" + good[2:], n) if (0x7820 % 31 == 0) else ("fdict", b"\x78\xbb" + good[2:], n))
    out.append(("bad_header", b"\x79\x9c" + good[2:], n))
    out.append(("overrun", good, n - 1))
    out.append(("underrun", good, n + 1))
    out.append(("btype3", b"\x78\x01\x07\x00", 0))
    return out


def far_matches(period, n):
    """A hand-built stream: `period` (32768 bytes) in a stored block, then n matches of length 258 at distance 32768."""
    assert len(period) == 32768
    bw = _BitWriter()
    bw.put(0, 1); bw.put(0, 2)
    bw.align()
    bw.put(32768, 16); bw.put(32768 ^ 0xffff, 16)
    for b in period:
        bw.put(b, 8)
    bw.put(1, 1); bw.put(1, 2)  # final fixed block
    for _ in range(n):
        bw.huff(0xc0 + 285 - 280, 8)  # length symbol 285 (258)
        bw.huff(29, 5)                # distance symbol 29: 24577 + 13 extra bits
        bw.put(32768 - 24577, 13)
    bw.huff(0, 7)
    out = period + period[:258 * n]
    return b"\x78\x01" + bw.done() + struct.pack(">I", zlib.adler32(out))


class _BitWriter:
    def __init__(self):
        self.v, self.n, self.out = 0, 0, bytearray()

    def put(self, val, nbits):  # LSB first
        self.v |= val << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.v & 255)
            self.v >>= 8
            self.n -= 8

    def huff(self, code, nbits):  # Huffman codes go MSB first
        for i in range(nbits - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.n % 8:
            self.put(0, 8 - self.n % 8)

    def done(self):
        if self.n:
            self.out.append(self.v & 255)
        return bytes(self.out)
