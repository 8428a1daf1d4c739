"""Deflate streams for the inflate tests (test support, not a test): the valid matrix and the corruption fuzz, built with Python's zlib from
fixed seeds.  The host twin (tests/test_inflate.py) and the device kernel (tests/test_inflate_gpu.py) get the same vectors."""
import os
import random
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_fixture as bf  # noqa: E402
import frontend_cases as fc  # noqa: E402

LEVELS = (0, 1, 6, 9)
STRATEGIES = dict(default=zlib.Z_DEFAULT_STRATEGY, fixed=zlib.Z_FIXED, huffman_only=zlib.Z_HUFFMAN_ONLY, rle=zlib.Z_RLE, filtered=zlib.Z_FILTERED)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def zlib_inflate(stream, cap):
    """zlib's verdict as hostsrc/host_bam.cpp asks for it: inflate(Z_FINISH), windowBits -15, room for cap bytes -> the bytes, or None
    when the stream does not end within them."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, cap + 1)
    except zlib.error:
        return None
    return out if d.eof and len(out) <= cap else None


def payloads():
    rng = random.Random(20240917)
    case = fc.synth(3, n_reads=400, ref_len=4000)
    bam = bf.Bam(case["sam"].decode(), [(case["ctg"], 4000)])
    records = b"".join(r.encode() for r in bam.records)[:65280]
    far = rng.randbytes(32768)
    return [("empty", b""), ("one_byte", b"Q"), ("zeros", bytes(65280)), ("random", rng.randbytes(65280)), ("distance_32768", far + far[:30000]),
            ("bam_records", records), ("sam_text", bam.canonical().encode()[:65280])]


def valid_matrix():
    """[(name, stream, payload)]: every payload at every level and strategy, streams with full flushes in the middle (several deflate blocks,
    an empty stored one among them), and a stream followed by garbage."""
    out = []
    pl = payloads()
    for name, data in pl:
        for level in LEVELS:
            for sname, strategy in STRATEGIES.items():
                out.append(("%s-l%d-%s" % (name, level, sname), deflate(data, level, strategy), data))
    for name, data in pl[2:]:
        for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
            out.append(("%s-l%d-flush" % (name, level), deflate(data, level, strategy, flush_at=len(data) // 3), data))
    rng = random.Random(7)
    for name, data in pl:
        out.append(("%s-garbage" % name, deflate(data) + rng.randbytes(37), data))
    return out


def corrupt_cases():
    """[(name, stream, cap)]: for small streams of each block type every single-bit flip of the first 64 bytes; for larger ones a few hundred
    seeded byte edits and truncations.  cap is the original payload's length + 1, as the BGZF reader gives it."""
    rng = random.Random(99)
    pl = dict(payloads())
    kinds = (("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("dynamic", 6, zlib.Z_DEFAULT_STRATEGY), ("huffman", 9, zlib.Z_HUFFMAN_ONLY))
    out = []
    small = (pl["one_byte"], pl["sam_text"][:700], pl["bam_records"][:1500], rng.randbytes(200))
    for kname, level, strategy in kinds:
        for k, data in enumerate(small):
            z = deflate(data, level, strategy)
            for bit in range(min(len(z), 64) * 8):
                y = bytearray(z)
                y[bit >> 3] ^= 1 << (bit & 7)
                out.append(("%s-small%d-bit%d" % (kname, k, bit), bytes(y), len(data) + 1))
    large = (pl["sam_text"][:20000], pl["bam_records"][:30000], pl["distance_32768"][:40000])
    for kname, level, strategy in kinds:
        for k, data in enumerate(large):
            z = deflate(data, level, strategy, flush_at=len(data) // 2 if k == 0 else None)
            for j in range(100):
                y = bytearray(z)
                for _ in range(rng.randint(1, 3)):
                    y[rng.randrange(len(y))] = rng.randrange(256)
                if rng.random() < 0.3:
                    y = y[:rng.randrange(len(y) + 1)]
                out.append(("%s-large%d-edit%d" % (kname, k, j), bytes(y), len(data) + 1))
    return out


def bgzf_block(stream, crc, isize):
    """a BGZF block around a raw deflate stream (at most 65510 bytes)"""
    assert len(stream) + 26 <= 65536
    return struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(stream) + 25) + stream + struct.pack("<II", crc & 0xffffffff, isize)


def status_cases():
    """[(name, block, expected status)]: a stream that ends with ISIZE - 1, ISIZE, ISIZE + 1 and ISIZE + 2 bytes, and a wrong CRC32."""
    data = dict(payloads())["sam_text"][:5000]
    z, crc = deflate(data), zlib.crc32(data)
    return [("isize-1", bgzf_block(z, crc, len(data) + 1), 2), ("isize", bgzf_block(z, crc, len(data)), 0), ("isize+1", bgzf_block(z, crc, len(data) - 1), 2),
            ("isize+2", bgzf_block(z, crc, len(data) - 2), 1), ("crc", bgzf_block(z, crc ^ 0x10000, len(data)), 3),
            ("empty", bgzf_block(deflate(b""), 0, 0), 0), ("empty+1", bgzf_block(deflate(b"x"), zlib.crc32(b"x"), 0), 2)]
