#!/usr/bin/env python3
"""markdup_bam, measured (a measurement for the record, not a gate; no test runs it).

Synthesises the coordinate-sorted BAMs of tools/gpu/bam_reader_bench.py from a seed -- Illumina-like reads (150 bp) and ONT-like reads
(10 kb, CIGARs with indels); unpaired, so every record is a fragment and reads that share a start and a strand are duplicates -- and marks
each with the host backend at 16 threads and the device backend in turn, --repeats times over, alternating, so that no leg has the warm file
cache to itself.  Every repeat is printed as one JSON line: seconds for the whole markdup_bam call (both reads of the input, the summaries,
the resolution, the patch, deflate, the write), MB of records per second, the counts, and whether the two files are the same bytes.
docs/markdup_bam.md says how a result is to be read: the device leg against the 16-thread host leg of the same build on the same box, with
the spread of the repeats as the margin.

    python tools/gpu/markdup_bench.py [--illumina N] [--ont N] [--repeats K] [--remove_duplicates] [--out DIR] [--quick]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LEGS = (("host16", dict(backend="host", threads=16)), ("device", dict(backend="device")))


def measure(shape, path, rec_bytes, repeats, out_dir, remove):
    from clair_amd import markdup_bam
    files = {}
    for repeat in range(repeats):
        for leg, kw in LEGS:
            out = os.path.join(out_dir, "%s.%s.marked.bam" % (shape, leg))
            t0 = time.perf_counter()
            r = markdup_bam.markdup_bam(path, out, remove=remove, force=True, **kw)
            dt = time.perf_counter() - t0
            files[leg] = open(out, "rb").read()
            print(json.dumps(dict(shape=shape, leg=leg, repeat=repeat, seconds=round(dt, 4), mb_per_s=round(rec_bytes / dt / 1e6, 1), records=r["records"],
                                  examined=r["examined"], duplicates=r["duplicates"], written=r["written"], bytes_out=r["bytes_out"])), flush=True)
        print(json.dumps(dict(shape=shape, repeat=repeat, same_bytes=len(set(files.values())) == 1)), flush=True)


def main():
    import bam_reader_bench as brb
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--illumina", type=int, default=2000000, help="Illumina-like reads, default: %(default)s")
    ap.add_argument("--ont", type=int, default=50000, help="ONT-like reads, default: %(default)s")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--remove_duplicates", action="store_true", help="measure the removing mode")
    ap.add_argument("--quick", action="store_true", help="200 000 Illumina-like and 5 000 ONT-like reads")
    ap.add_argument("--out", type=str, default=None, help="directory for the synthetic BAMs and the marked files, default: a new temporary one")
    args = ap.parse_args()
    if args.quick:
        args.illumina, args.ont = 200000, 5000
    if args.out is None:
        import tempfile
        args.out = tempfile.mkdtemp(prefix="markdup_bench_")
    os.makedirs(args.out, exist_ok=True)
    for shape, n, read_len, ref_len, ont in (("illumina", args.illumina, 150, 10000000, False), ("ont", args.ont, 10000, 20000000, True)):
        if n <= 0:
            continue
        path = os.path.join(args.out, "%s.bam" % shape)
        _, rec_bytes = brb.synth_bam(path, n, read_len, ref_len, 1, ont)
        measure(shape, path, rec_bytes, args.repeats, args.out, args.remove_duplicates)


if __name__ == "__main__":
    main()
