"""markdup_bam: duplicate reads flagged (0x400) or removed, without samtools or Picard (docs/markdup_bam.md).

    python -m clair_amd.markdup_bam --bam_fn in.bam --marked_fn out.bam [--remove_duplicates] [--backend auto|device|host] [--device N]
            [--bam_threads N] [--memory BYTES[K|M|G]] [--bgzf_deflate zlib|host|device] [--index] [--force] [--json_fn stats.json]
    markdup_bam(bam_fn, marked_fn, remove=False, backend="auto", device=0, threads=4, memory=None, deflate=None, index=False, force=False) -> dict

The input is read twice.  The first read keeps a 32-byte summary per record (its end: reference, unclipped 5' position and strand; the hash
of its name; its score; a few flag bits); the rule of csrc/markdup_core.h is resolved over the summaries alone; the second read sets or
clears bit 0x400 of every examined record where it lies and writes the records in the input's order (--remove_duplicates: without the flagged
ones).  Both reads and the resolution are computed by a backend: the GPU (clair_markdup_*, csrc/markdup.hip: the inflated bytes never leave
the device) or its host twin (clair_host_markdup_*, hostsrc/host_markdup.cpp), byte for byte the same.  Both run under one file driver
(clair_host_markdup_run).  The header goes through as it is: no @PG line, SO untouched."""
import ctypes
import json
import os
import sys
from argparse import ArgumentParser

import numpy as np

from clair_amd import _hostapi, bam_stage
from clair_amd._hostapi import BamError
from clair_amd.bam_stage import BATCH_BLOCKS

BACKEND_WORDS = 8                                # clair_markdup_backend_t: ctx and seven function pointers
STATS_WORDS = 9                                  # CLAIR_MARKDUP_STATS
SUMMARY = np.dtype([("end", "<u8"), ("hash", "<u8"), ("score", "<u4"), ("index", "<u4"), ("bits", "<u4"), ("pad", "<u4")])      # clair_markdup_summary_t
EXAMINED, PAIRABLE, READ2, REVERSE = 1, 2, 4, 8  # the summary's bits (csrc/markdup_core.h)
NO_END = 0xffffffffffffffff
STAT_NAMES = ("records", "examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "duplicates", "written")


def _stream_arguments(stream, starts):
    stream = np.ascontiguousarray(np.frombuffer(bytes(stream), dtype=np.uint8))
    return stream, np.ascontiguousarray(starts, dtype=np.int64)


class HostMarker(bam_stage.HostBackend):
    """clair_host_markdup_*: the host twin (hostsrc/host_markdup.cpp)."""
    prefix, words = "markdup", BACKEND_WORDS


def host_debug_summary(stream, starts, n_ref):
    """clair_host_markdup_debug_summary -> the summaries (SUMMARY) of the records at `starts` of a raw record stream"""
    lib = _hostapi.load()
    stream, starts = _stream_arguments(stream, starts)
    out = np.zeros(len(starts), dtype=SUMMARY)
    if lib.clair_host_markdup_debug_summary(stream.ctypes.data, len(stream), starts.ctypes.data, len(starts), int(n_ref), out.ctypes.data) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    return out


def host_debug_resolve(summaries):
    """clair_host_markdup_debug_resolve -> uint8 [n], 1: the rule flags the record"""
    lib = _hostapi.load()
    summaries = np.ascontiguousarray(summaries, dtype=SUMMARY)
    out = np.zeros(len(summaries), dtype=np.uint8)
    if lib.clair_host_markdup_debug_resolve(summaries.ctypes.data, len(summaries), out.ctypes.data) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    return out


class DeviceMarker(bam_stage.DeviceBackend):
    """clair_markdup_*: the device backend (csrc/markdup.hip)."""
    prefix, words = "markdup", BACKEND_WORDS

    def summary(self, stream, starts, n_ref):
        """clair_markdup_debug_summary -> SUMMARY [n]"""
        stream, starts = _stream_arguments(stream, starts)
        out = np.zeros(len(starts), dtype=SUMMARY)
        self._check(self._lib.clair_markdup_debug_summary(self._h, stream.ctypes.data, len(stream), starts.ctypes.data, len(starts), int(n_ref), out.ctypes.data))
        return out

    def resolve(self, summaries):
        """clair_markdup_debug_resolve -> uint8 [n]"""
        summaries = np.ascontiguousarray(summaries, dtype=SUMMARY)
        out = np.zeros(len(summaries), dtype=np.uint8)
        self._check(self._lib.clair_markdup_debug_resolve(self._h, summaries.ctypes.data, len(summaries), out.ctypes.data))
        return out

    def mark(self, stream, starts, summaries, duplicate, remove=False):
        """clair_markdup_debug_mark -> (the patched stream, the records written) as bytes (the guard regions around the device's stream and
        output are checked there)"""
        stream, starts = _stream_arguments(stream, starts)
        summaries, duplicate = np.ascontiguousarray(summaries, dtype=SUMMARY), np.ascontiguousarray(duplicate, dtype=np.uint8)
        if not len(starts) == len(summaries) == len(duplicate):
            raise BamError("mark: %d starts, %d summaries, %d bytes" % (len(starts), len(summaries), len(duplicate)))
        patched, out, n = np.zeros(len(stream), dtype=np.uint8), np.zeros(len(stream), dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.clair_markdup_debug_mark(self._h, stream.ctypes.data, len(stream), starts.ctypes.data, len(starts), summaries.ctypes.data,
                                                       duplicate.ctypes.data, int(bool(remove)), patched.ctypes.data, out.ctypes.data, ctypes.byref(n)))
        return patched.tobytes(), out[:n.value].tobytes()

def markdup_bam(bam_fn, marked_fn, remove=False, backend="auto", device=0, threads=4, memory=None, deflate=None, index=False, force=False,
                max_blocks=BATCH_BLOCKS, segment_bytes=None):
    """-> dict(records, examined, pairs, fragments, duplicate_pairs, duplicate_fragments, duplicates, written, bytes_in, bytes_out, backend,
    path).  backend "auto": the device when one is present (a choice of convenience, not of speed: docs/markdup_bam.md), else the
    host.  deflate None: the backend's own compressor.  segment_bytes None: the device's default segment, the host's sequential walk."""
    stats, head_bytes, backend = bam_stage.rewrite(
        bam_fn, marked_fn, host=HostMarker, device_backend=DeviceMarker, header_of=bytes, run_args=(int(bool(remove)),), stats_words=STATS_WORDS,
        device_needs="records", backend=backend, device=device, threads=threads, memory=memory, deflate=deflate, index=index, force=force,
        max_blocks=max_blocks, segment_bytes=segment_bytes)
    result = dict(zip(STAT_NAMES, (int(v) for v in stats[:8])))
    result.update(bytes_in=os.path.getsize(bam_fn), bytes_out=head_bytes + int(stats[8]), backend=backend, path=marked_fn)
    return result


def build_parser():
    parser = ArgumentParser(description="Flag or remove duplicate reads of a BAM, on the GPU or on the host, without samtools or Picard")
    add = parser.add_argument
    add('--bam_fn', type=str, required=True, help="the BAM to read, in any order")
    add('--marked_fn', type=str, required=True, help="the BAM to write: the input's records in the input's order")
    add('--remove_duplicates', action='store_true', help="drop the records the rule flags instead of writing them with 0x400")
    bam_stage.add_backend_arguments(parser, "framed, summarised, resolved and patched", "BGZF inflate and deflate threads on the host",
                                    speed="convenience, not speed: docs/markdup_bam.md",
                                    memory_help="most bytes of record summaries (32 a record), BYTES[K|M|G]; a larger file is refused, default: 8G",
                                    index_help="write <marked_fn>.bai as index_bam does, with the same backend (the input must be sorted by coordinate)")
    add('--json_fn', type=str, default=None, help="write the counts as JSON")
    return parser


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    try:
        r = markdup_bam(args.bam_fn, args.marked_fn, remove=args.remove_duplicates, backend=args.backend, device=args.device, threads=args.bam_threads,
                        memory=args.memory, deflate=args.bgzf_deflate, index=args.index, force=args.force)
    except BamError as e:
        print("[ERROR] markdup_bam: %s" % e, file=sys.stderr)
        sys.exit(1)
    if args.json_fn:
        with open(args.json_fn, "w") as f:
            json.dump(r, f, indent=1, sort_keys=True)
            f.write("\n")
    print("[INFO] markdup_bam (%s): %s: %d records, %d examined (%d pairs, %d fragments), %d duplicates (%d pairs, %d fragments), %d written, %d -> %d bytes"
          % (r["backend"], r["path"], r["records"], r["examined"], r["pairs"], r["fragments"], r["duplicates"], r["duplicate_pairs"], r["duplicate_fragments"],
             r["written"], r["bytes_in"], r["bytes_out"]), file=sys.stderr)


if __name__ == "__main__":
    main()
