"""index_bam: the .bai of a coordinate-sorted BAM, without samtools (docs/index_bam.md).

    python -m clair_amd.index_bam --bam_fn reads.bam [--bai_fn out.bai] [--backend auto|device|host] [--device N] [--bam_threads N] [--force]
    build_index(bam_fn, out_fn=None, backend="auto", device=0, threads=4, force=False) -> dict

The records are framed and their fields, bins, virtual offsets, runs and linear-index minima computed by a backend: the GPU
(clair_bamidx_*, csrc/bam_index.hip: the inflated bytes never leave the device) or its host twin (clair_host_bamidx_*,
hostsrc/host_bam_index.cpp), bit for bit the same.  Both run under one file driver (clair_host_bamidx_build), which hands back the runs
(tid, bin, begin, end) in file order, the linear index and the counts.  This module stitches them into the file:

    magic "BAI\\1", n_ref; per reference: n_bin, per bin (ascending): bin, n_chunk, the chunks in file order; n_intv, the 16 KiB windows.

A window no record touched takes the value of the window before it, 0 before the first (clair_amd/tabix.py's convention); n_intv is the last
touched window + 1; a reference without records has n_bin = 0 and n_intv = 0.  The pseudo-bin 37450 and the trailing n_no_coor, both optional
in the specification, are not written.  The file is written under a temporary name and renamed."""
import ctypes
import os
import struct
import sys
from argparse import ArgumentParser

import numpy as np

from clair_amd import _hostapi, bam_stage
from clair_amd._hostapi import BamError
from clair_amd.bam_stage import BATCH_BLOCKS

RUN_DTYPE = np.dtype([("tid", "<i4"), ("bin", "<u4"), ("beg", "<u8"), ("end", "<u8")])     # clair_bamidx_run_t
BACKEND_WORDS = 5                                # clair_bamidx_backend_t: ctx and four function pointers
FRAME_WORDS = 4                                  # clair_*bamidx_debug_frame's result
SEGMENT_MIN, SEGMENT_DEFAULT = 64, 8192          # clair_bix::SEG_MIN, SEG_DEFAULT (csrc/bam_index_core.h)
NO_OFFSET = np.uint64(0xffffffffffffffff)


class HostIndexer(bam_stage.HostBackend):
    """clair_host_bamidx_*: the host twin (hostsrc/host_bam_index.cpp)."""
    prefix, words = "bamidx", BACKEND_WORDS


class DeviceIndexer(bam_stage.DeviceBackend):
    """clair_bamidx_*: the device backend (csrc/bam_index.hip)."""
    prefix, words = "bamidx", BACKEND_WORDS

    def frame(self, stream, entry=0):
        """clair_bamidx_debug_frame -> (starts, tail, bad, sentinels intact)"""
        stream = np.ascontiguousarray(np.frombuffer(bytes(stream), dtype=np.uint8))
        starts, result = np.zeros(len(stream) // 36 + 2, dtype=np.int64), np.zeros(FRAME_WORDS, dtype=np.int64)
        self._check(self._lib.clair_bamidx_debug_frame(self._h, stream.ctypes.data, len(stream), int(entry), starts.ctypes.data, len(starts), result.ctypes.data))
        return starts[:result[0]].tolist(), int(result[1]), bool(result[2]), bool(result[3])

def host_frame(stream, entry=0, segment_bytes=0):
    """clair_host_bamidx_debug_frame -> (starts, tail, bad): segment_bytes 0 is the sequential walk, else the segmented rule restated."""
    lib = _hostapi.load()
    stream = np.ascontiguousarray(np.frombuffer(bytes(stream), dtype=np.uint8))
    starts, result = np.zeros(len(stream) // 36 + 2, dtype=np.int64), np.zeros(FRAME_WORDS, dtype=np.int64)
    if lib.clair_host_bamidx_debug_frame(stream.ctypes.data, len(stream), int(entry), int(segment_bytes), starts.ctypes.data, len(starts), result.ctypes.data) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    return starts[:result[0]].tolist(), int(result[1]), bool(result[2])


def scan(bam_fn, indexer):
    """clair_host_bamidx_build: the whole file through the indexer's backend -> (counts dict, runs, linear, first_window)."""
    lib = _hostapi.load()
    table = indexer.backend()
    res = ctypes.c_void_p()
    if lib.clair_host_bamidx_build(bam_fn.encode(), table, indexer.max_blocks, ctypes.byref(res)) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    try:
        info = np.zeros(6, dtype=np.int64)
        lib.clair_host_bamidx_result_info(res, info.ctypes.data)
        runs, linear = np.zeros(int(info[4]), dtype=RUN_DTYPE), np.zeros(int(info[5]), dtype=np.uint64)
        first_window = np.zeros(int(info[0]) + 1, dtype=np.int64)
        lib.clair_host_bamidx_result_copy(res, runs.ctypes.data, linear.ctypes.data, first_window.ctypes.data)
    finally:
        lib.clair_host_bamidx_result_free(res)
    counts = dict(references=int(info[0]), records=int(info[1]), mapped=int(info[2]), unplaced=int(info[3]), chunks=len(runs))
    return counts, runs, linear, first_window


def bai_bytes(n_ref, runs, linear, first_window):
    """The file, from the runs in file order and the linear index (all-ones: a window no record touched)."""
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    order = np.lexsort((np.arange(len(runs)), runs["bin"], runs["tid"]))          # by (tid, bin), file order within
    by = runs[order]
    edges = np.searchsorted(by["tid"], np.arange(n_ref + 1))
    for tid in range(n_ref):
        mine = by[edges[tid]:edges[tid + 1]]
        bins, first = np.unique(mine["bin"], return_index=True)
        out.append(struct.pack("<i", len(bins)))
        for k, b in enumerate(bins):
            chunks = mine[first[k]:first[k + 1] if k + 1 < len(bins) else len(mine)]
            out.append(struct.pack("<Ii", int(b), len(chunks)))
            pairs = np.empty((len(chunks), 2), dtype="<u8")
            pairs[:, 0], pairs[:, 1] = chunks["beg"], chunks["end"]
            out.append(pairs.tobytes())
        lin = linear[first_window[tid]:first_window[tid + 1]]
        touched = np.flatnonzero(lin != NO_OFFSET)
        n_intv = int(touched[-1]) + 1 if len(touched) else 0
        lin = lin[:n_intv]
        if n_intv:                                                                # an empty window: the value of the window before it
            src = np.maximum.accumulate(np.where(lin != NO_OFFSET, np.arange(n_intv), -1))
            lin = np.where(src >= 0, lin[np.maximum(src, 0)], np.uint64(0)).astype("<u8")
        out.append(struct.pack("<i", n_intv))
        out.append(lin.astype("<u8").tobytes())
    return b"".join(out)


def build_index(bam_fn, out_fn=None, backend="auto", device=0, threads=4, force=False, max_blocks=BATCH_BLOCKS, segment_bytes=None):
    """-> dict(references, records, mapped, unplaced, chunks, bytes, backend, path).  backend "auto": the device when one is present (a choice
    of convenience, not of measured speed: docs/index_bam.md), else the host.  segment_bytes None: the device's default segment, the host's
    sequential walk."""
    backend = bam_stage.resolve_backend(backend)
    bam_stage.check_threads(threads)
    if not os.path.isfile(bam_fn):
        raise BamError("%s: cannot open" % bam_fn)
    out_fn = out_fn or bam_fn + ".bai"
    if os.path.exists(out_fn) and not force:
        raise BamError("%s exists: --force overwrites it" % out_fn)
    if backend == "device":
        indexer = DeviceIndexer(device=device, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
    else:
        indexer = HostIndexer(threads=threads, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
    try:
        counts, runs, linear, first_window = scan(bam_fn, indexer)
    finally:
        indexer.close()
    data = bai_bytes(counts["references"], runs, linear, first_window)
    tmp = "%s.tmp.%d" % (out_fn, os.getpid())
    try:
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, out_fn)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    counts.update(bytes=len(data), backend=backend, path=out_fn)
    return counts


def build_parser():
    parser = ArgumentParser(description="Write the .bai index of a coordinate-sorted BAM, on the GPU or on the host, without samtools")
    add = parser.add_argument
    add('--bam_fn', type=str, required=True, help="coordinate-sorted BAM")
    add('--bai_fn', type=str, default=None, help="the index to write, default: <bam_fn>.bai")
    bam_stage.add_backend_arguments(parser, "framed and indexed", "BGZF inflate threads of --backend host", force_help="overwrite an existing index")
    return parser


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    try:
        r = build_index(args.bam_fn, args.bai_fn, backend=args.backend, device=args.device, threads=args.bam_threads, force=args.force)
    except BamError as e:
        print("[ERROR] index_bam: %s" % e, file=sys.stderr)
        sys.exit(1)
    print("[INFO] index_bam (%s): %s: %d references, %d records (%d mapped, %d unplaced), %d chunks, %d bytes"
          % (r["backend"], r["path"], r["references"], r["records"], r["mapped"], r["unplaced"], r["chunks"], r["bytes"]), file=sys.stderr)


if __name__ == "__main__":
    main()
