#!/usr/bin/env python3
"""sort_bam, measured (a measurement for the record, not a gate; no test runs it).

Synthesises the BAMs of tools/gpu/bam_reader_bench.py from a seed -- Illumina-like reads (150 bp) and ONT-like reads (10 kb, CIGARs with
indels) --, shuffles their records, and sorts each with the host backend at 16 threads and the device backend in turn, --repeats times over,
alternating, so that no leg has the warm file cache to itself.  Every repeat is printed as one JSON line: seconds for the whole sort_bam
call (the reads of the input, batches, sort, gather, deflate, the write), MB of records per second, and whether the two files are the same
bytes.  docs/sort_bam.md says how a result is to be read: the device leg against the 16-thread host leg of the same build on the same box,
with the spread of the repeats as the margin.

    python tools/gpu/sort_bam_bench.py [--illumina N] [--ont N] [--repeats K] [--memory BYTES[K|M|G]] [--out DIR] [--quick]
"""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LEGS = (("host16", dict(backend="host", threads=16)), ("device", dict(backend="device")))


def shuffle_bam(path, out, seed):
    """The records of a BAM whose records all have one length (the synthetic ones), in a random order; blocks by zlib at level 1"""
    import bam_fixture as bf
    data, at, stream = open(path, "rb").read(), 0, bytearray()
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        stream += zlib.decompress(data[at + 18:at + size - 8], -15)
        at += size
    l_text, = struct.unpack_from("<I", stream, 4)
    n_ref, = struct.unpack_from("<i", stream, 8 + l_text)
    first = 12 + l_text
    for _ in range(n_ref):
        first += 8 + struct.unpack_from("<I", stream, first)[0]
    each = 4 + struct.unpack_from("<I", stream, first)[0]
    records = np.frombuffer(bytes(stream[first:]), dtype=np.uint8).reshape(-1, each)
    shuffled = bytes(stream[:first]) + records[np.random.default_rng(seed).permutation(len(records))].tobytes()
    with open(out, "wb") as f:
        for a in range(0, len(shuffled), 65280):
            piece = shuffled[a:a + 65280]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z = c.compress(piece) + c.flush()
            f.write(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(z) + 25) + z + struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece)))
        f.write(bf.EOF_BLOCK)
    return len(records)


def measure(shape, path, rec_bytes, repeats, out_dir, memory):
    from clair_amd import sort_bam
    files = {}
    for repeat in range(repeats):
        for leg, kw in LEGS:
            out = os.path.join(out_dir, "%s.%s.sorted.bam" % (shape, leg))
            t0 = time.perf_counter()
            r = sort_bam.sort_bam(path, out, force=True, memory=memory, **kw)
            dt = time.perf_counter() - t0
            files[leg] = open(out, "rb").read()
            print(json.dumps(dict(shape=shape, leg=leg, repeat=repeat, seconds=round(dt, 4), mb_per_s=round(rec_bytes / dt / 1e6, 1), records=r["records"],
                                  groups=r["groups"], input_reads=r["input_reads"], bytes_out=r["bytes_out"])), flush=True)
        print(json.dumps(dict(shape=shape, repeat=repeat, same_bytes=len(set(files.values())) == 1)), flush=True)


def main():
    import bam_reader_bench as brb
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--illumina", type=int, default=2000000, help="Illumina-like reads, default: %(default)s")
    ap.add_argument("--ont", type=int, default=50000, help="ONT-like reads, default: %(default)s")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--memory", type=str, default=None, help="sort_bam's --memory, default: its own")
    ap.add_argument("--quick", action="store_true", help="200 000 Illumina-like and 5 000 ONT-like reads")
    ap.add_argument("--out", type=str, default=None, help="directory for the synthetic BAMs and the sorted files, default: a new temporary one")
    args = ap.parse_args()
    if args.quick:
        args.illumina, args.ont = 200000, 5000
    if args.out is None:
        import tempfile
        args.out = tempfile.mkdtemp(prefix="sort_bam_bench_")
    os.makedirs(args.out, exist_ok=True)
    for shape, n, read_len, ref_len, ont in (("illumina", args.illumina, 150, 10000000, False), ("ont", args.ont, 10000, 20000000, True)):
        if n <= 0:
            continue
        path = os.path.join(args.out, "%s.bam" % shape)
        _, rec_bytes = brb.synth_bam(path, n, read_len, ref_len, 1, ont)
        os.remove(path + ".bai")
        shuffled = os.path.join(args.out, "%s.shuffled.bam" % shape)
        assert shuffle_bam(path, shuffled, 2) == n
        measure(shape, shuffled, rec_bytes, args.repeats, args.out, args.memory)


if __name__ == "__main__":
    main()
