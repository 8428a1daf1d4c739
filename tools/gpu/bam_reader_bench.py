#!/usr/bin/env python3
"""--bam_reader native, measured (a measurement for the record, not a gate).

Synthesises a sorted BAM + .bai from a seed at user-sized shapes -- Illumina-like reads (150 bp, one contig) and ONT-like reads
(10 kb, CIGARs with indels) -- and reports, as one JSON line per shape:
  inflate_walk     BGZF inflate + record walk (clair_host_bam_next) over the whole contig at 1, 4 and 16 threads: MB/s of records, records/s;
  add_bam          the device decode (clair_frontend_add_bam) of those records in 64 MB chunks: alignments/s, seconds;
  device_fe_bam    read + add_bam + candidates + windows, end to end from the file;
  device_fe_text   the same alignments as the canonical text, already in memory, through clair_frontend_add_text (no samtools process:
                   the text path's upper bound), + candidates + windows.
With --inflate the run measures the BGZF inflate legs instead (docs/bam_reader.md, "Device inflate"): per repeat, alternating, read + walk and
the end-to-end device front end from the file with the host inflate at --bam_threads (`host`), on the GPU (`device`), or host at 4 threads,
host at 16 and device in turn (`all`); every repeat is reported.  The inflate kernel's own time comes from
`rocprofv3 --kernel-trace --stats -- python tools/gpu/bam_reader_bench.py --quick --inflate device`.
The fe_bam_* kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu/bam_reader_bench.py --quick`.

    python tools/gpu/bam_reader_bench.py [--illumina N] [--ont N] [--out DIR]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synth_bam(path, n_reads, read_len, ref_len, seed, ont):
    """Records built with NumPy (no per-base Python): Illumina-like '150M'; ONT-like alternating M / I / D blocks."""
    import struct
    import bam_fixture as bf
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, ref_len - read_len - 64, n_reads)).astype(np.int32)
    if ont:
        pieces = []                                          # per read: 20 x (240M 5I 240M 5D), 80 operations, 9 700 bases
        for _ in range(20):
            pieces += [(240, 0), (5, 1), (240, 0), (5, 2)]
        ops = pieces
    else:
        ops = [(read_len, 0)]
    qlen = sum(n for n, op in ops if op in (0, 1))
    rlen = sum(n for n, op in ops if op in (0, 2))
    cigar = np.array([n << 4 | op for n, op in ops], np.uint32).tobytes()
    header = bf.Bam("", [("chrB", ref_len)]).header()
    name_len = 12
    seq_bytes = (qlen + 1) // 2
    body = 32 + name_len + len(cigar) + seq_bytes + qlen
    rec = np.zeros((n_reads, 4 + body), np.uint8)
    fixed = np.zeros(n_reads, dtype=np.dtype([("bs", "<u4"), ("tid", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mq", "u1"), ("bin", "<u2"),
                                              ("nc", "<u2"), ("flag", "<u2"), ("lseq", "<i4"), ("nt", "<i4"), ("np", "<i4"), ("tl", "<i4")]))
    fixed["bs"], fixed["tid"], fixed["pos"], fixed["lrn"], fixed["mq"] = body, 0, pos, name_len, 60
    fixed["bin"] = [bf.reg2bin(int(p), int(p) + rlen) for p in pos]
    fixed["nc"], fixed["flag"], fixed["lseq"], fixed["nt"], fixed["np"] = len(ops), rng.integers(0, 2, n_reads) * 16, qlen, -1, -1
    rec[:, :36] = fixed.view(np.uint8).reshape(n_reads, 36)
    names = np.array([("r%010d" % i).encode() for i in range(n_reads)], dtype="S11")
    rec[:, 36:36 + 11] = names.view(np.uint8).reshape(n_reads, 11)
    c0 = 36 + name_len
    rec[:, c0:c0 + len(cigar)] = np.frombuffer(cigar, np.uint8)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n_reads, seq_bytes * 2))]
    rec[:, c0 + len(cigar):c0 + len(cigar) + seq_bytes] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, c0 + len(cigar) + seq_bytes:] = 30
    stream = header + rec.tobytes()
    out = bytearray()
    starts = []
    for a in range(0, len(stream), 65280):
        data = stream[a:a + 65280]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z = c.compress(data) + c.flush()
        starts.append((a, len(out)))
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(z) + 25) + z + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))
    end = len(out)
    out += bf.EOF_BLOCK
    with open(path, "wb") as f:
        f.write(out)
    # .bai: one chunk in the bin of the whole contig, the linear index from the record starts (enough for a whole-contig query)
    first = len(header)
    block_of = lambda u: starts[min(u // 65280, len(starts) - 1)]
    voff = lambda u: (end << 16) if u >= len(stream) else (block_of(u)[1] << 16 | (u - block_of(u)[0]))
    lin = {}
    for k in range(0, n_reads, max(1, n_reads // 4096)):
        lin.setdefault(int(pos[k]) >> 14, voff(first + k * (4 + body)))
    n_intv = (ref_len >> 14) + 1
    vals, last = [], voff(first)
    for w in range(n_intv):
        last = lin.get(w, last)
        vals.append(last)
    bai = b"BAI\1" + struct.pack("<i", 1) + struct.pack("<i", 1) + struct.pack("<Ii", 0, 1) + struct.pack("<QQ", voff(first), voff(len(stream)))
    bai += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in vals)
    with open(path + ".bai", "wb") as f:
        f.write(bai)
    ref = "".join(np.array(list("ACGT"))[rng.integers(0, 4, ref_len)])
    return ref, len(stream) - len(header)


def measure_inflate(path, ref, rec_bytes, n_reads, legs, repeats):
    """legs: [(name, BamReader keywords)], run in turn `repeats` times: A B C A B C ..."""
    from clair_amd import _capi, _hostapi
    cap = 64 << 20
    buf, off = np.empty(cap + 16, np.uint8), _hostapi.bam_offsets_for(cap)
    out = dict(records=n_reads, record_mb=round(rec_bytes / 1e6, 1), legs={name: dict(read_walk=[], device_fe_bam=[]) for name, _ in legs})
    sums = {}
    for rep in range(repeats + 1):                           # repeat 0 warms up (module load, first allocations) and is not reported
        for name, kw in legs:
            r = _hostapi.BamReader(path, **kw)
            r.query("chrB")
            t0, n_bytes, crc = time.perf_counter(), 0, 0
            while True:
                n, k = r.readinto(buf, off, cap=cap)
                if not k:
                    break
                n_bytes += n
                if rep == 0:
                    crc = zlib.crc32(buf[:n], crc)
            dt = time.perf_counter() - t0
            r.close()
            f = _capi.Frontend(0, ref, 0, -64, len(ref) + 64)
            t1 = time.perf_counter()
            r = _hostapi.BamReader(path, **kw)
            r.query("chrB")
            f.bam_options(0)
            while True:
                n, k = r.readinto(buf, off, cap=cap)
                if not k:
                    break
                f.add_bam(buf, n, off, k)
            r.close()
            t_feed = time.perf_counter() - t1
            f.find_candidates(min_coverage=4, threshold=0.125)
            n_win = f.build_windows(min_coverage=0, drop_non_iupac_centre=True)
            total = time.perf_counter() - t1
            f.close()
            if rep == 0:
                sums[name] = (n_bytes, crc, n_win)
                continue
            out["legs"][name]["read_walk"].append(dict(seconds=round(dt, 3), mb_per_s=round(n_bytes / dt / 1e6, 1)))
            out["legs"][name]["device_fe_bam"].append(dict(seconds=round(total, 3), read_and_add_bam_seconds=round(t_feed, 3), windows=n_win))
    out["same_bytes"] = len(set(sums.values())) == 1
    return out


def measure(path, ref, rec_bytes, n_reads, quick):
    from clair_amd import _capi, _hostapi
    out = dict(records=n_reads, record_mb=round(rec_bytes / 1e6, 1))
    cap = 64 << 20
    buf = np.empty(cap + 16, np.uint8)
    off = _hostapi.bam_offsets_for(cap)
    walk = {}
    for threads in ((4,) if quick else (1, 4, 16)):
        r = _hostapi.BamReader(path, threads=threads)
        r.query("chrB")
        t0, n_rec, n_bytes = time.perf_counter(), 0, 0
        while True:
            n, k = r.readinto(buf, off, cap=cap)
            if not k:
                break
            n_rec += k
            n_bytes += n
        dt = time.perf_counter() - t0
        r.close()
        walk[str(threads)] = dict(seconds=round(dt, 3), mb_per_s=round(n_bytes / dt / 1e6, 1), records_per_s=round(n_rec / dt))
    out["inflate_walk"] = walk
    # device decode: chunks read first (host time excluded), then add_bam timed
    r = _hostapi.BamReader(path, threads=16)
    r.query("chrB")
    chunks, texts = [], []
    while True:
        n, k = r.readinto(buf, off, cap=cap)
        if not k:
            break
        chunks.append((buf[:n].copy(), off[:k].copy()))
        texts.append(r.render(buf, off, k))
    r.close()

    def run_fe(feed):
        f = _capi.Frontend(0, ref, 0, -64, len(ref) + 64)
        t0 = time.perf_counter()
        feed(f)
        t_feed = time.perf_counter() - t0
        f.find_candidates(min_coverage=4, threshold=0.125)
        n_win = f.build_windows(min_coverage=0, drop_non_iupac_centre=True)
        total = time.perf_counter() - t0
        reads = f.stats()["reads"]
        f.close()
        return t_feed, total, reads, n_win

    def feed_bam(f):
        f.bam_options(0)
        for data, offs in chunks:
            f.add_bam(data, len(data), offs, len(offs))

    def feed_text(f):
        f.text_options("chrB")
        for t in texts:
            f.add_text(t)

    run_fe(feed_bam)                                          # warm-up (module load, first allocations)
    t_feed, total, reads, n_win = run_fe(feed_bam)
    out["add_bam"] = dict(seconds=round(t_feed, 3), alignments_per_s=round(reads / t_feed), alignments=reads)
    t_feed_t, total_t, reads_t, n_win_t = run_fe(feed_text)
    out["device_fe_text"] = dict(seconds=round(total_t, 3), add_text_seconds=round(t_feed_t, 3), alignments=reads_t, windows=n_win_t,
                                 text_mb=round(sum(len(t) for t in texts) / 1e6, 1))

    def feed_file(f):
        r = _hostapi.BamReader(path, threads=4)
        r.query("chrB")
        f.bam_options(0)
        while True:
            n, k = r.readinto(buf, off, cap=cap)
            if not k:
                break
            f.add_bam(buf, n, off, k)
        r.close()
    t_feed_f, total_f, reads_f, n_win_f = run_fe(feed_file)
    out["device_fe_bam"] = dict(seconds=round(total_f, 3), read_and_add_bam_seconds=round(t_feed_f, 3), alignments=reads_f, windows=n_win_f,
                                bam_threads=4, pageable_buffer=True)
    out["same_windows"] = n_win == n_win_t == n_win_f and reads == reads_t == reads_f
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--illumina", type=int, default=2000000, help="Illumina-like 150 bp reads, default: %(default)s")
    p.add_argument("--ont", type=int, default=50000, help="ONT-like 10 kb reads, default: %(default)s")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--quick", action="store_true", help="small shapes, one thread count (the run under rocprofv3)")
    p.add_argument("--out", type=str, default=None, help="directory for the synthetic BAMs and results.json, default: a new temporary one")
    p.add_argument("--inflate", choices=("host", "device", "all"), default=None,
                   help="measure the BGZF inflate legs only: host (at --bam_threads), device, or all = host at 4 threads, host at 16, device in turn")
    p.add_argument("--bam_threads", type=int, default=4, help="threads of the host inflate leg, default: %(default)s")
    p.add_argument("--repeats", type=int, default=3, help="repeats of every inflate leg, default: %(default)s")
    a = p.parse_args()
    legs = dict(host=[("host_%d" % a.bam_threads, dict(threads=a.bam_threads))], device=[("device", dict(inflate="device"))],
                all=[("host_4", dict(threads=4)), ("host_16", dict(threads=16)), ("device", dict(inflate="device"))]).get(a.inflate)
    if a.out is None:
        import tempfile
        a.out = tempfile.mkdtemp(prefix="bam_reader_bench_")
    if a.quick:
        a.illumina, a.ont = 200000, 5000
    os.makedirs(a.out, exist_ok=True)
    results = []
    for name, n, read_len, ref_len, ont in (("illumina", a.illumina, 150, 10000000, False), ("ont", a.ont, 10000, 20000000, True)):
        if n <= 0:
            continue
        path = os.path.join(a.out, "%s.bam" % name)
        t0 = time.perf_counter()
        ref, rec_bytes = synth_bam(path, n, read_len, ref_len, a.seed, ont)
        res = dict(shape=name, synth_seconds=round(time.perf_counter() - t0, 1))
        res.update(measure_inflate(path, ref, rec_bytes, n, legs, a.repeats) if legs else measure(path, ref, rec_bytes, n, a.quick))
        print(json.dumps(res), flush=True)
        results.append(res)
        os.remove(path)
        os.remove(path + ".bai")
    print("results: %s" % os.path.join(a.out, "results.json"), file=sys.stderr)
    with open(os.path.join(a.out, "results.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
