"""What tests/test_index_bam.py and tests/test_index_bam_gpu.py share (test support, not a test): the small SAM whose .bai exercises every
rule of docs/index_bam.md, the four ways it is written, the malformed files, and the generated record streams of the framing tests."""
import random
import struct
import zlib

from bam_fixture import EOF_BLOCK, Bam

REFS = [("chr1", 70000000), ("chrEmpty", 5000), ("chr2", 200000)]
WAYS = {"whole": dict(block=65280), "straddle": dict(block=211), "per_record": dict(per_record=True), "no_eof": dict(eof=False)}


def _line(name, flag, ref, pos1, cigar, seq_len, mapq=60):
    return "\t".join([name, str(flag), ref, str(pos1), str(mapq), cigar, "*", "0", "0", "ACGT" * (seq_len // 4) + "A" * (seq_len % 4), "*"])


def sam_text():
    """Three contigs (one empty); bins of every level, one record crossing a 2^26 boundary (bin 0); a record over four 16 KiB windows; two
    records of bin 4681 with one of bin 585 between them (three chunks, not two); a placed unmapped mate; pos 0; unplaced reads; one record of
    65 536 CIGAR operations (stored as the placeholder)."""
    rows = [
        _line("first", 0, "chr1", 1, "10M", 10),                       # pos 0, bin 4681
        _line("same_bin", 16, "chr1", 100, "20M", 20),
        _line("x1", 0, "chr1", 16371, "5M", 5),                        # bin 4681 ...
        _line("y", 0, "chr1", 16381, "10M", 10),                       # ... 585 (crosses 16384) ...
        _line("x2", 0, "chr1", 16383, "2M", 2),                        # ... 4681 again
        _line("windows", 0, "chr1", 30001, "40000M", 40000),           # windows 1 .. 4
        _line("level3", 0, "chr1", 131001, "100M2D100M", 200),         # crosses 2^17: bin 73
        _line("level2", 0, "chr1", 1048501, "200M", 200),              # crosses 2^20: bin 9
        _line("mate", 69, "chr1", 2000001, "*", 30),                   # placed, unmapped: span 0
        _line("mapped_mate", 137, "chr1", 2000001, "30M", 30),
        _line("level1", 0, "chr1", 8388601, "20M", 20),                # crosses 2^23: bin 1
        _line("level0", 0, "chr1", 67108861, "5M3N2M5S", 12),          # crosses 2^26: bin 0
        _line("c2a", 0, "chr2", 11, "4S10M", 14),
        _line("long_cigar", 0, "chr2", 1001, "1M1I" * 32768, 65536),   # 65 536 operations: the placeholder, the real CIGAR in CG:B:I
        _line("c2b", 0, "chr2", 150001, "50=1X", 51),
        _line("nowhere1", 4, "*", 0, "*", 8),
        _line("nowhere2", 77, "*", 0, "*", 8),
    ]
    return "\n".join(rows) + "\n"


def bam():
    return Bam(sam_text(), REFS)


def write_ways(tmp, names=tuple(WAYS)):
    """-> {way: path}; each BAM with the fixture's own .bai next to it"""
    b, out = bam(), {}
    for way in names:
        out[way] = str(tmp / ("%s.bam" % way))
        b.write(out[way], **WAYS[way])
    return out


def write_records(path, refs, records, block=65280, eof=True):
    """A BAM of hand-made records (bytes, size word included), in the order given: what the fixture's sorting writer cannot make."""
    b = Bam("", refs)
    b.records = []

    class Raw(object):
        def __init__(self, data):
            self.data = data

        def encode(self):
            return self.data
    b.records = [Raw(r) for r in records]
    b.write(path, block=block, index=False, eof=eof)
    return path


def raw_record(tid, pos, cigar=((10, 0),), name=b"r", flag=0, l_seq=None, block_size=None):
    """One record, fields as given (nothing is checked: these are the malformed ones too)."""
    seq_len = sum(n for n, op in cigar if op in (0, 1, 4, 7, 8)) if l_seq is None else l_seq
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 60, 0, len(cigar), flag, seq_len, -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    body += b"\x11" * ((max(seq_len, 0) + 1) // 2) + b"\xff" * max(seq_len, 0)
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def synthetic_bam(path, n_reads=16000, seed=11):
    """A sorted BAM of Illumina-like reads from a seed, built with NumPy: 150 bp ('150M') and 101 bp ('60M2D41M') reads over two contigs, every
    hundredth one a placed unmapped mate, a few unplaced reads at the end; about 4 MB of records in BGZF blocks of 65 280 bytes.  No index."""
    import numpy as np
    rng = np.random.default_rng(seed)
    refs = [("chrA", 3000000), ("chrB", 1200000)]
    n_unplaced = 40
    tid = np.sort(rng.integers(0, 2, n_reads)).astype(np.int32)
    pos = rng.integers(0, 1000000, n_reads).astype(np.int32)
    order = np.lexsort((pos, tid))
    tid, pos = tid[order], pos[order]
    tid[n_reads - n_unplaced:], pos[n_reads - n_unplaced:] = -1, -1
    dtype = np.dtype([("bs", "<u4"), ("tid", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mq", "u1"), ("bin", "<u2"), ("nc", "<u2"), ("flag", "<u2"),
                      ("lseq", "<i4"), ("nt", "<i4"), ("np", "<i4"), ("tl", "<i4")])
    shapes = []
    for ops in ([(150, 0)], [(60, 0), (2, 2), (41, 0)]):
        qlen = sum(n for n, op in ops if op in (0, 1))
        cigar = np.array([n << 4 | op for n, op in ops], np.uint32).tobytes()
        body = 32 + 12 + len(cigar) + (qlen + 1) // 2 + qlen
        rec = np.zeros((n_reads, 4 + body), np.uint8)
        fixed = np.zeros(n_reads, dtype=dtype)
        fixed["bs"], fixed["tid"], fixed["pos"], fixed["lrn"], fixed["mq"], fixed["nc"], fixed["lseq"], fixed["nt"], fixed["np"] = body, tid, pos, 12, 60, len(ops), qlen, -1, -1
        fixed["flag"] = np.where(tid < 0, 4, np.where(np.arange(n_reads) % 100 == 99, 69, rng.integers(0, 2, n_reads) * 16))
        rec[:, :36] = fixed.view(np.uint8).reshape(n_reads, 36)
        rec[:, 36:47] = np.array([("r%010d" % i).encode() for i in range(n_reads)], dtype="S11").view(np.uint8).reshape(n_reads, 11)
        rec[:, 48:48 + len(cigar)] = np.frombuffer(cigar, np.uint8)
        rec[:, 48 + len(cigar):] = rng.integers(0, 256, (n_reads, body + 4 - 48 - len(cigar)), dtype=np.uint8)      # bases and qualities: noise
        shapes.append(rec)
    which = rng.integers(0, 2, n_reads)
    stream = Bam("", refs).header() + b"".join(shapes[which[i]][i].tobytes() for i in range(n_reads))
    out = bytearray()
    for a in range(0, len(stream), 65280):
        data = stream[a:a + 65280]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z = c.compress(data) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(z) + 25) + z + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))
    with open(path, "wb") as f:
        f.write(bytes(out) + EOF_BLOCK)
    return path, n_reads


# ---- the framing tests' streams: records of random bytes, so that false size words are everywhere
def record_stream(seed, lengths, n_records, entry=0, tail=b""):
    """-> (stream, starts): `entry` bytes of noise, n_records records of 4 + block_size bytes drawn from `lengths` (each >= 36), then `tail`"""
    rng = random.Random(seed)
    out, starts = bytearray(rng.getrandbits(8) for _ in range(entry)), []
    for _ in range(n_records):
        size = rng.choice(lengths)
        starts.append(len(out))
        out += struct.pack("<I", size - 4) + bytes(rng.getrandbits(8) for _ in range(size - 4))
    return bytes(out + tail), starts


def lengths_for(segment):
    return [36, 37, 63, 64, 65, segment - 4, segment, segment + 1, 5 * segment]


def frame_cases(segment):
    lengths = lengths_for(segment)
    for seed in range(6):
        for entry in (0, 1, 2, 3, segment // 2 + 1, segment - 1, segment - 2, segment - 3):
            yield "seed%d_entry%d" % (seed, entry), record_stream(1000 * segment + seed, lengths, 40, entry=entry), entry
    short = lengths_for(segment)[:5]
    yield "one_record", record_stream(1, short, 1), 0
    yield "empty", (b"", []), 0
    yield "block_size_31", record_stream(2, short, 9, tail=struct.pack("<I", 31) + bytes(40)), 0
    stream, starts = record_stream(3, short, 9)
    yield "one_byte_short", (stream[:-1], starts[:-1]), 0
    yield "size_word_cut", record_stream(4, short, 9, tail=b"\x40\0\0"), 0
    yield "huge_block_size", record_stream(5, short, 9, tail=struct.pack("<I", 0x80000000) + bytes(40)), 0


# ---- files an index build must refuse
REFS2 = [("a", 1 << 30), ("b", 100000)]


def malformed(tmp):
    """{name: (path, what the message says)}"""
    rec = raw_record
    good = [rec(0, 100), rec(0, 200), rec(0, 300), rec(1, 5), rec(-1, -1, cigar=(), flag=4, l_seq=4)]
    out = {}

    def case(name, records, pattern, **kw):
        out[name] = (write_records(str(tmp / (name + ".bam")), REFS2, records, **kw), pattern)
    case("swapped_records", [good[0], good[2], good[1], good[3]], r"record 2 \(0:200, virtual offset \d+\) comes after 0:300: the BAM is not sorted")
    case("swapped_contigs", [good[3], good[0]], r"record 1 \(0:100, .*comes after 1:5.*not sorted")
    case("mapped_after_unplaced", [good[0], good[4], good[3]], r"record 2 \(1:5, .*comes after -1:-1.*not sorted")
    case("beyond_2_29", [good[0], rec(0, (1 << 29) - 5, cigar=((10, 0),))], r"record 1 \(0:536870907, .*ends at 536870917, beyond 2\^29.*\.csi")
    lying = rec(0, 150)
    lying = lying[:20] + struct.pack("<i", 4000) + lying[24:]                      # l_seq says more than block_size holds
    case("fields_too_long", [good[0], lying], r"record 1 at virtual offset \d+ is malformed: fields longer than block_size")
    case("negative_l_seq", [good[0], rec(0, 150, l_seq=-3)], r"record 1 .*negative l_seq")
    case("unknown_reference", [good[0], rec(7, 150)], r"record 1 .*reference id not in the header")
    case("block_size_31", [good[0], rec(0, 150, block_size=31)], r"record at virtual offset \d+: block_size 31 < 32")
    whole = write_records(str(tmp / "whole.bam"), REFS2, [good[0]] * 60 + [good[3]] * 60 + [good[4]] * 9, block=300)
    data = open(whole, "rb").read()
    for name, keep, pattern in (("cut_mid_block", len(data) - 28 - 10, r"truncated BGZF block at compressed offset \d+"),):
        with open(str(tmp / (name + ".bam")), "wb") as f:
            f.write(data[:keep])
        out[name] = (str(tmp / (name + ".bam")), pattern)
    case("cut_mid_record", [good[0]] * 30 + [good[3][:-7]], r"the stream ends inside a record \(virtual offset \d+\)", eof=False)
    with open(str(tmp / "text.bam"), "wb") as f:
        f.write(b"@HD\tVN:1.6\n" * 20)
    out["not_bgzf"] = (str(tmp / "text.bam"), r"is not a BGZF-compressed BAM")
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = c.compress(b"#not a bam\n" * 9) + c.flush()
    with open(str(tmp / "vcf.bam"), "wb") as f:
        f.write(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(z) + 25) + z + struct.pack("<II", zlib.crc32(b"#not a bam\n" * 9), 99) + EOF_BLOCK)
    out["not_bam"] = (str(tmp / "vcf.bam"), r"BGZF but not BAM")
    return out
