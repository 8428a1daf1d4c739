"""What tests/test_sort_bam.py and tests/test_sort_bam_gpu.py share (test support, not a test): the shuffled SAM that exercises every rule of
docs/sort_bam.md, the yardstick order (np.lexsort over the fixture's records, not the code under test), the header cases, the groups a
--memory gives restated, the key sets of the radix tests and a NumPy restatement of the tile-and-rank rule the device sorts by."""
import random
import struct
import zlib

import numpy as np

from bam_fixture import Bam
from index_bam_cases import _line

REFS = [("chr1", 5000000), ("chr2", 300000), ("chr3", 2500000)]      # 5 + 1 + 3 buckets, and the one of the reads without a reference
BUCKET_SHIFT = 20
PAYLOAD = 65280
WAYS = {"straddle": dict(block=300), "whole": dict(block=65280), "per_record": dict(per_record=True)}


def sam_text(seed=5):
    """About 300 records over three references, shuffled: runs of 20 records with one (tid, pos, strand); both strands at one position;
    unplaced records; placed unmapped mates; a record at pos 0; one record of more than 70 000 bytes."""
    rng = random.Random(seed)
    rows = []
    for k in range(150):
        ref = rng.choice(["chr1", "chr1", "chr2", "chr3"])
        length = dict(REFS)[ref]
        n = rng.randrange(60, 320)
        rows.append(_line("r%03d" % k, rng.choice([0, 16]), ref, rng.randrange(1, length - 400), "%dM" % n, n))
    for run, (ref, pos1, flag) in enumerate([("chr1", 1048577, 0), ("chr3", 2097000, 16), ("chr2", 77, 0)]):
        rows += [_line("run%d_%02d" % (run, k), flag, ref, pos1, "50M", 50) for k in range(20)]
    for k in range(12):                                                # both strands at one position, alternating in the input
        rows.append(_line("strand%02d" % k, 16 if k % 2 == 0 else 0, "chr1", 3000001, "80M", 80))
    rows += [_line("nowhere%02d" % k, rng.choice([4, 77, 141]), "*", 0, "*", 40 + k) for k in range(25)]
    rows += [_line("mate%02d" % k, rng.choice([69, 133, 117]), rng.choice(["chr1", "chr3"]), rng.randrange(1, 2000000), "*", 64) for k in range(20)]
    rows.append(_line("first", 0, "chr1", 1, "10M", 10))               # pos 0
    rows.append(_line("first_rev", 16, "chr1", 1, "10M", 10))
    rows.append(_line("long", 0, "chr3", 1200000, "50000M", 50000))    # 75 048 bytes
    rows.append(_line("past_the_end", 0, "chr2", 300000, "30M", 30))   # the last base of its reference
    rng.shuffle(rows)
    return "\n".join(rows) + "\n"


def bam(seed=5):
    return Bam(sam_text(seed), REFS, sort=False)


def order(records):
    """The yardstick: by (uint32 tid, pos + 1, reverse strand), the input order among equals."""
    tid = np.array([r.tid for r in records], dtype=np.int64) & 0xffffffff
    pos1 = np.array([r.pos + 1 for r in records], dtype=np.int64)
    reverse = np.array([r.flag >> 4 & 1 for r in records], dtype=np.int64)
    return np.lexsort((np.arange(len(records)), reverse, pos1, tid))


def sorted_records(b):
    return [b.records[i] for i in order(b.records)]


def expected_stream(b, header=None):
    """What the sorted file inflates to"""
    return (b.header() if header is None else header) + b"".join(r.encode() for r in sorted_records(b))


def keys_of(records):
    return np.array([((r.tid & 0xffffffff) << 32) | (((r.pos + 1) << 1) & 0xffffffff) | (r.flag >> 4 & 1) for r in records], dtype=np.uint64)


def read_bgzf(path):
    """-> (the payloads of the file's blocks, True when the last one is the empty EOF block), by Python's zlib"""
    data, at, out = open(path, "rb").read(), 0, []
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 14] == b"BC"
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        payload = zlib.decompress(data[at + 18:at + size - 8], -15)
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert isize == len(payload) and crc == zlib.crc32(payload) & 0xffffffff
        out.append(payload)
        at += size
    return out, bool(out) and out[-1] == b"" and data[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def inflated(path):
    return b"".join(read_bgzf(path)[0])


def bucket_bytes(b):
    """bytes of records per bucket of the histogram"""
    first, total = [], 0
    for _, length in b.refs:
        first.append(total)
        total += max(1, -(-length >> BUCKET_SHIFT))
    hist = [0] * (total + 1)
    for r in b.records:
        bucket = total if r.tid < 0 else first[r.tid] + (max(0, min(r.pos, b.refs[r.tid][1] - 1)) >> BUCKET_SHIFT)
        hist[bucket] += len(r.encode())
    return hist


def expected_groups(b, memory):
    """(groups, reads of the input) of a sort under --memory: one read when everything fits, else consecutive buckets greedily"""
    hist = bucket_bytes(b)
    if sum(hist) <= memory:
        return 1, 1
    assert max(hist) <= memory
    groups, at = 0, 0
    while at < len(hist):
        total = 0
        while at < len(hist) and total + hist[at] <= memory:
            total += hist[at]
            at += 1
        groups += 1
    return groups, 1 + groups


def bucket_bam():
    """Three records in every bucket of the histogram, in no order: under a --memory of the largest bucket no two buckets share a group"""
    rows = []
    for ref, length in REFS:
        for b in range(-(-length >> BUCKET_SHIFT)):
            rows += [_line("%s_%d_%d" % (ref, b, k), 16 * (k & 1), ref, min((b << BUCKET_SHIFT) + 1000 - 300 * k, length), "100M", 100) for k in range(3)]
    rows += [_line("nowhere_%d" % k, 4, "*", 0, "*", 100) for k in range(3)]
    random.Random(8).shuffle(rows)
    return Bam("\n".join(rows) + "\n", REFS, sort=False)


class HeaderBam(Bam):
    """A fixture BAM with a header text of the test's own"""

    def __init__(self, text, sam, refs):
        Bam.__init__(self, sam, refs, sort=False)
        self.text = text

    def header(self):
        out = b"BAM\1" + struct.pack("<I", len(self.text)) + self.text + struct.pack("<i", len(self.refs))
        for name, length in self.refs:
            out += struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", length)
        return out


SQ = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in REFS)
HEADER_CASES = {      # name: (text in, text out)
    "unsorted": (b"@HD\tVN:1.6\tSO:unsorted\n" + SQ, b"@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    "queryname": (b"@HD\tVN:1.5\tSO:queryname\tGO:query\tSS:queryname:natural\n" + SQ + b"@PG\tID:bwa\n",
                  b"@HD\tVN:1.5\tSO:coordinate\tGO:query\tSS:queryname:natural\n" + SQ + b"@PG\tID:bwa\n"),
    "no_so": (b"@HD\tVN:1.4\tGO:none\n" + SQ, b"@HD\tVN:1.4\tGO:none\tSO:coordinate\n" + SQ),
    "no_hd": (SQ + b"@PG\tID:minimap2\tCL:x SO:y\n", b"@HD\tVN:1.6\tSO:coordinate\n" + SQ + b"@PG\tID:minimap2\tCL:x SO:y\n"),
    "empty": (b"", b"@HD\tVN:1.6\tSO:coordinate\n"),
    "comment": (b"@HD\tVN:1.6\tSO:unknown\n" + SQ + b"@CO\tresorted, was SO:queryname\tSO:unsorted\n",
                b"@HD\tVN:1.6\tSO:coordinate\n" + SQ + b"@CO\tresorted, was SO:queryname\tSO:unsorted\n"),
}


# ---- the radix sort
def sizes_for(tile):
    return [0, 1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 17]


def key_sets(n, seed=0):
    """{name: uint64 keys [n]}"""
    rng = np.random.default_rng(1000 + seed + n)
    real = keys_of(bam().records)
    three = np.array([7 << 32 | 5, 3, 7 << 32 | 4], dtype=np.uint64)
    return {
        "random": rng.integers(0, 1 << 64, n, dtype=np.uint64),
        "three_values": three[rng.integers(0, 3, n)],
        "top_byte": (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00a5a5a5a5a5a5a5),
        "bit_0": rng.integers(0, 2, n, dtype=np.uint64) | np.uint64(0x1234567800000100),
        "all_equal": np.full(n, 0x0123456789abcdef, dtype=np.uint64),
        "bit_63": (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) | rng.integers(0, 1 << 20, n, dtype=np.uint64),
        "real": real[np.arange(n) % len(real)],
    }


def radix_restated(keys, tile, lanes=64):
    """The rule of csrc/bam_sort.hip restated: eight passes of eight bits, least significant first, a pass skipped when its digit is the same
    in every key.  A pass: per tile the digit counts, digit-major; their exclusive scan; every key goes to base[digit][tile] + rank, where
    rank counts the equal digits of the waves before its wave, of the rounds of 64 before its round within the wave, and of the lanes below
    its lane in the round.  -> (perm, passes run)"""
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    idx = np.arange(n, dtype=np.uint32)
    if n < 2:
        return idx, 0
    differing, passes = int(np.bitwise_or.reduce(keys ^ keys[0])), 0
    per_wave = tile // 4
    for p in range(8):
        if not differing >> (8 * p) & 0xff:
            continue
        passes += 1
        digit = ((keys >> np.uint64(8 * p)) & np.uint64(0xff)).astype(np.int64)
        n_tiles = -(-n // tile)
        hist = np.zeros((256, n_tiles), dtype=np.int64)
        np.add.at(hist, (digit, np.arange(n) // tile), 1)
        base = (np.cumsum(hist.ravel()) - hist.ravel()).reshape(256, n_tiles)
        out_keys, out_idx = np.empty_like(keys), np.empty_like(idx)
        for t in range(n_tiles):
            wave_count = np.zeros((4, 256), dtype=np.int64)
            rank = np.zeros(min(tile, n - t * tile), dtype=np.int64)
            for w in range(4):
                for at in range(t * tile + w * per_wave, min(t * tile + (w + 1) * per_wave, n), lanes):
                    d = digit[at:at + lanes]
                    below = np.array([np.count_nonzero(d[:k] == d[k]) for k in range(len(d))], dtype=np.int64)
                    rank[at - t * tile:at - t * tile + len(d)] = wave_count[w, d] + below
                    np.add.at(wave_count[w], d, 1)
            before = np.cumsum(wave_count, axis=0) - wave_count           # the waves in wave order
            lo, hi = t * tile, min((t + 1) * tile, n)
            wave_of = (np.arange(lo, hi) - lo) // per_wave
            dst = base[digit[lo:hi], t] + before[wave_of, digit[lo:hi]] + rank
            out_keys[dst], out_idx[dst] = keys[lo:hi], idx[lo:hi]
        keys, idx = out_keys, out_idx
    return idx, passes


# ---- the gather
def gather_case(seed=3):
    """-> (stream, starts, perm): records of 36, 37, 38, 39 bytes, of random lengths up to 9000 and one of more than 70 000, with noise in
    front of, between (none) and behind them; a random permutation"""
    rng = random.Random(seed)
    lengths = [36, 37, 38, 39] * 3 + [rng.randrange(36, 9001) for _ in range(60)] + [70001]
    rng.shuffle(lengths)
    out, starts = bytearray(rng.getrandbits(8) for _ in range(3)), []
    for size in lengths:
        starts.append(len(out))
        out += struct.pack("<I", size - 4) + bytes(rng.getrandbits(8) for _ in range(size - 4))
    out += bytes(rng.getrandbits(8) for _ in range(5))
    perm = list(range(len(lengths)))
    rng.shuffle(perm)
    return bytes(out), starts, perm
