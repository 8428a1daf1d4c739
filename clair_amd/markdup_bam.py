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

from clair_amd import _hostapi, bgzf
from clair_amd._hostapi import BamError
from clair_amd.sort_bam import BATCH_BLOCKS, DEFLATE_MODES, header_blocks, parse_memory

BACKEND_WORDS = 8                                # clair_markdup_backend_t: ctx and seven function pointers
STATS_WORDS = 9                                  # CLAIR_MARKDUP_STATS
SUMMARY = np.dtype([("end", "<u8"), ("hash", "<u8"), ("score", "<u4"), ("index", "<u4"), ("bits", "<u4"), ("pad", "<u4")])      # clair_markdup_summary_t
EXAMINED, PAIRABLE, READ2, REVERSE = 1, 2, 4, 8  # the summary's bits (csrc/markdup_core.h)
NO_END = 0xffffffffffffffff
STAT_NAMES = ("records", "examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "duplicates", "written")


def _stream_arguments(stream, starts):
    stream = np.ascontiguousarray(np.frombuffer(bytes(stream), dtype=np.uint8))
    return stream, np.ascontiguousarray(starts, dtype=np.int64)


class HostMarker(_hostapi.Handle):
    """clair_host_markdup_*: the host twin.  segment_bytes 0: records framed by the sequential walk; a power of two: by the segmented rule."""
    _error = BamError
    name = "host"

    def __init__(self, threads=4, max_blocks=BATCH_BLOCKS, segment_bytes=0):
        self._lib = _hostapi.load()
        out = self._own(self._lib.clair_host_markdup_destroy, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_markdup_create(int(threads), int(max_blocks), int(segment_bytes), out))

    def backend(self):
        table = (ctypes.c_void_p * BACKEND_WORDS)()
        self._check(self._lib.clair_host_markdup_backend(self._h, table))
        return table


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


class DeviceMarker(object):
    """clair_markdup_*: the device backend (csrc/markdup.hip)."""
    name = "device"

    def __init__(self, device=0, max_blocks=BATCH_BLOCKS, segment_bytes=0):
        from clair_amd import _capi
        try:
            self._lib = _capi.load()
        except _capi.EngineError as e:
            raise BamError(str(e))
        self._h = ctypes.c_void_p()
        if self._lib.clair_markdup_create(int(device), int(max_blocks), int(segment_bytes), ctypes.byref(self._h)) != 0:
            raise BamError("clair_markdup_create failed: %s" % self._lib.clair_markdup_last_error(None).decode())

    def _check(self, rc):
        if rc != 0:
            raise BamError(self._lib.clair_markdup_last_error(self._h).decode())

    def backend(self):
        table = (ctypes.c_void_p * BACKEND_WORDS)()
        self._check(self._lib.clair_markdup_backend(self._h, table))
        return table

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

    def close(self):
        if self._h:
            self._lib.clair_markdup_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def markdup_bam(bam_fn, marked_fn, remove=False, backend="auto", device=0, threads=4, memory=None, deflate=None, index=False, force=False,
                max_blocks=BATCH_BLOCKS, segment_bytes=None):
    """-> dict(records, examined, pairs, fragments, duplicate_pairs, duplicate_fragments, duplicates, written, bytes_in, bytes_out, backend,
    path).  backend "auto": the device when one is present (a choice of convenience, not of speed: docs/markdup_bam.md), else the
    host.  deflate None: the backend's own compressor.  segment_bytes None: the device's default segment, the host's sequential walk."""
    if backend not in ("auto", "device", "host"):
        raise BamError("--backend %s: auto, device or host" % backend)
    if deflate is not None and deflate not in bgzf.BACKENDS:
        raise BamError("--bgzf_deflate %s: %s" % (deflate, ", ".join(bgzf.BACKENDS)))
    if not isinstance(threads, int) or not 1 <= threads <= 16:
        raise BamError("--bam_threads %s: 1 .. 16" % threads)
    memory = parse_memory(memory)
    if not os.path.isfile(bam_fn):
        raise BamError("%s: cannot open" % bam_fn)
    if os.path.realpath(bam_fn) == os.path.realpath(marked_fn) or (os.path.exists(marked_fn) and os.path.samefile(bam_fn, marked_fn)):
        raise BamError("%s: the output is the input" % marked_fn)
    for fn in [marked_fn] + ([marked_fn + ".bai"] if index else []):
        if os.path.exists(fn) and not force:
            raise BamError("%s exists: --force overwrites it" % fn)
    if backend == "auto":
        backend = "host"
        try:
            from clair_amd import _capi
            if _capi.load().clair_device_count() > 0:
                backend = "device"
        except Exception:
            pass
    deflate = deflate or backend
    if deflate == "device" and backend != "device":
        raise BamError("--bgzf_deflate device compresses the device-resident records: it needs --backend device")
    lib = _hostapi.load()
    job = ctypes.c_void_p()
    if lib.clair_host_markdup_open(bam_fn.encode(), ctypes.byref(job)) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    tmp = "%s.tmp.%d" % (marked_fn, os.getpid())
    marker = None
    try:
        n = ctypes.c_int64()
        lib.clair_host_markdup_header(job, None, 0, ctypes.byref(n))
        raw = np.zeros(n.value, dtype=np.uint8)
        lib.clair_host_markdup_header(job, raw.ctypes.data, len(raw), ctypes.byref(n))
        if backend == "device":
            marker = DeviceMarker(device=device, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
        else:
            marker = HostMarker(threads=threads, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
        head = header_blocks(raw.tobytes(), deflate)
        with open(tmp, "wb") as f:
            f.write(head)
        stats = np.zeros(STATS_WORDS, dtype=np.int64)
        mode = DEFLATE_MODES["own" if deflate == backend else deflate]
        if lib.clair_host_markdup_run(job, marker.backend(), tmp.encode(), mode, memory, int(max_blocks), threads, int(bool(remove)), stats.ctypes.data) != 0:
            raise BamError(lib.clair_host_last_error().decode())
        os.replace(tmp, marked_fn)
    finally:
        lib.clair_host_markdup_close(job)
        if marker is not None:
            marker.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    result = dict(zip(STAT_NAMES, (int(v) for v in stats[:8])))
    result.update(bytes_in=os.path.getsize(bam_fn), bytes_out=len(head) + int(stats[8]), backend=backend, path=marked_fn)
    if index:
        from clair_amd import index_bam
        index_bam.build_index(marked_fn, backend=backend, device=device, threads=threads, force=force)
    return result


def build_parser():
    parser = ArgumentParser(description="Flag or remove duplicate reads of a BAM, on the GPU or on the host, without samtools or Picard")
    add = parser.add_argument
    add('--bam_fn', type=str, required=True, help="the BAM to read, in any order")
    add('--marked_fn', type=str, required=True, help="the BAM to write: the input's records in the input's order")
    add('--remove_duplicates', action='store_true', help="drop the records the rule flags instead of writing them with 0x400")
    add('--backend', type=str, default="auto", choices=("auto", "device", "host"),
        help="where records are framed, summarised, resolved and patched: the GPU, the host, or the GPU when one is present (convenience, not speed: docs/markdup_bam.md), default: %(default)s")
    add('--device', type=int, default=0, help="GPU of --backend device, default: %(default)s")
    add('--bam_threads', type=int, default=4, help="BGZF inflate and deflate threads on the host (1 .. 16), default: %(default)s")
    add('--memory', type=str, default=None, help="most bytes of record summaries (32 a record), BYTES[K|M|G]; a larger file is refused, default: 8G")
    add('--bgzf_deflate', type=str, default=None, choices=bgzf.BACKENDS, help="who compresses the output's blocks, default: the backend itself")
    add('--index', action='store_true', help="write <marked_fn>.bai as index_bam does, with the same backend (the input must be sorted by coordinate)")
    add('--force', action='store_true', help="overwrite an existing output")
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
