"""sort_bam: a BAM sorted by coordinate, without samtools (docs/sort_bam.md).

    python -m clair_amd.sort_bam --bam_fn in.bam --sorted_fn out.bam [--backend auto|device|host] [--device N] [--bam_threads N]
            [--memory BYTES[K|M|G]] [--bgzf_deflate zlib|host|device] [--index] [--force]
    sort_bam(bam_fn, sorted_fn, backend="auto", device=0, threads=4, memory=None, deflate=None, index=False, force=False) -> dict

Every record gets the key (uint32)tid << 32 | (uint32)(pos + 1) << 1 | reverse strand; records go out in the order of their keys, equal keys
in the order they came in.  The keys, the stable radix sort, the gather of the variable-length records and (--bgzf_deflate device) the BGZF
blocks are computed by a backend: the GPU (clair_bamsort_*, csrc/bam_sort.hip: the inflated bytes never leave the device) or its host twin
(clair_host_bamsort_*, hostsrc/host_bam_sort.cpp), byte for byte the same.  Both run under one file driver (clair_host_bamsort_run).  A file
whose records do not fit --memory is read once more per group of histogram buckets: no temporary files, no merge.  This module rewrites the
header (SO:coordinate), writes its blocks, lets the driver append the records' blocks and the EOF marker, and renames the file."""
import os
import struct
import sys
from argparse import ArgumentParser

import numpy as np

from clair_amd import _hostapi, bam_stage
from clair_amd._hostapi import BamError
from clair_amd.bam_stage import BATCH_BLOCKS, DEFLATE_MODES, PAYLOAD, header_blocks, parse_memory  # noqa: F401  (callers read them here)

BACKEND_WORDS = 8                                # clair_bamsort_backend_t: ctx and seven function pointers
STATS_WORDS = 7                                  # CLAIR_BAMSORT_STATS
RADIX_ITEMS = 8                                  # clair_bsort::RADIX_ITEMS (csrc/bam_sort_core.h)
RADIX_TILE = 256 * RADIX_ITEMS                   # keys per workgroup of a radix pass
HD_LINE = b"@HD\tVN:1.6\tSO:coordinate\n"


def sort_keys(tid, pos, flag):
    """The key of csrc/bam_sort_core.h over arrays."""
    tid, pos, flag = (np.asarray(a, dtype=np.int64) for a in (tid, pos, flag))
    return ((tid & 0xffffffff).astype(np.uint64) << np.uint64(32)) | ((((pos + 1) & 0xffffffff) << 1) & 0xffffffff).astype(np.uint64) | ((flag >> 4) & 1).astype(np.uint64)


def coordinate_header(raw):
    """The BAM header `raw` (magic, text, reference list) with SO:coordinate on the @HD line: an SO: value replaced, a missing one appended, a
    missing @HD line put in front; every other byte as it is."""
    l_text, = struct.unpack_from("<I", raw, 4)
    text, rest = raw[8:8 + l_text], raw[8 + l_text:]
    if text.startswith(b"@HD\t") or text.startswith(b"@HD\n") or text == b"@HD":
        end = text.find(b"\n")
        line, behind = (text, b"") if end < 0 else (text[:end], text[end:])
        fields = line.split(b"\t")
        if any(f.startswith(b"SO:") for f in fields[1:]):
            fields = [fields[0]] + [b"SO:coordinate" if f.startswith(b"SO:") else f for f in fields[1:]]
        else:
            cr = fields[-1].endswith(b"\r")
            fields = fields[:-1] + [fields[-1][:len(fields[-1]) - cr], b"SO:coordinate" + b"\r" * cr]
        text = b"\t".join(fields) + behind
    else:
        text = HD_LINE + text
    return raw[:4] + struct.pack("<I", len(text)) + text + rest


class HostSorter(bam_stage.HostBackend):
    """clair_host_bamsort_*: the host twin (hostsrc/host_bam_sort.cpp)."""
    prefix, words = "bamsort", BACKEND_WORDS


def _gather_arguments(stream, starts, perm):
    stream = np.ascontiguousarray(np.frombuffer(bytes(stream), dtype=np.uint8))
    starts, perm = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(perm, dtype=np.uint32)
    if len(starts) != len(perm):
        raise BamError("gather: %d starts, %d places" % (len(starts), len(perm)))
    total = sum(4 + struct.unpack_from("<I", stream, int(o))[0] for o in starts)
    return stream, starts, perm, np.zeros(total, dtype=np.uint8)


def host_debug_sort(keys):
    """clair_host_bamsort_debug_sort -> perm (uint32): the stable order of the keys"""
    lib = _hostapi.load()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    perm = np.zeros(len(keys), dtype=np.uint32)
    if lib.clair_host_bamsort_debug_sort(keys.ctypes.data, len(keys), perm.ctypes.data) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    return perm


def host_debug_gather(stream, starts, perm):
    """clair_host_bamsort_debug_gather -> the records at `starts` of the stream in the order perm, as bytes"""
    lib = _hostapi.load()
    stream, starts, perm, out = _gather_arguments(stream, starts, perm)
    if lib.clair_host_bamsort_debug_gather(stream.ctypes.data, len(stream), starts.ctypes.data, perm.ctypes.data, len(perm), out.ctypes.data, len(out)) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    return out.tobytes()


class DeviceSorter(bam_stage.DeviceBackend):
    """clair_bamsort_*: the device backend (csrc/bam_sort.hip)."""
    prefix, words = "bamsort", BACKEND_WORDS

    def sort(self, keys):
        """clair_bamsort_debug_sort -> perm (uint32)"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        perm = np.zeros(len(keys), dtype=np.uint32)
        self._check(self._lib.clair_bamsort_debug_sort(self._h, keys.ctypes.data, len(keys), perm.ctypes.data))
        return perm

    def gather(self, stream, starts, perm):
        """clair_bamsort_debug_gather -> bytes (the guard regions around the device's output are checked there)"""
        stream, starts, perm, out = _gather_arguments(stream, starts, perm)
        self._check(self._lib.clair_bamsort_debug_gather(self._h, stream.ctypes.data, len(stream), starts.ctypes.data, perm.ctypes.data, len(perm),
                                                         out.ctypes.data, len(out)))
        return out.tobytes()

def sort_bam(bam_fn, sorted_fn, backend="auto", device=0, threads=4, memory=None, deflate=None, index=False, force=False, max_blocks=BATCH_BLOCKS,
             segment_bytes=None):
    """-> dict(records, mapped, unplaced, groups, input_reads, already_sorted, bytes_in, bytes_out, backend, path).  backend "auto": the device
    when one is present (a choice of convenience, not of measured speed: docs/sort_bam.md), else the host.  deflate None: the backend's own
    compressor.  segment_bytes None: the device's default segment, the host's sequential walk."""
    stats, head_bytes, backend = bam_stage.rewrite(
        bam_fn, sorted_fn, host=HostSorter, device_backend=DeviceSorter, header_of=coordinate_header, run_args=(), stats_words=STATS_WORDS,
        device_needs="sorted records", backend=backend, device=device, threads=threads, memory=memory, deflate=deflate, index=index, force=force,
        max_blocks=max_blocks, segment_bytes=segment_bytes)
    return dict(records=int(stats[0]), mapped=int(stats[1]), unplaced=int(stats[2]), groups=int(stats[3]), input_reads=int(stats[4]),
                already_sorted=bool(stats[5]), bytes_in=os.path.getsize(bam_fn), bytes_out=head_bytes + int(stats[6]), backend=backend, path=sorted_fn)


def build_parser():
    parser = ArgumentParser(description="Sort a BAM by coordinate, on the GPU or on the host, without samtools")
    add = parser.add_argument
    add('--bam_fn', type=str, required=True, help="the BAM to sort, in any order")
    add('--sorted_fn', type=str, required=True, help="the coordinate-sorted BAM to write")
    bam_stage.add_backend_arguments(parser, "framed, sorted and gathered", "BGZF inflate and deflate threads on the host",
                                    memory_help="most record bytes held at once, BYTES[K|M|G]; a larger file is read once more per group, default: 8G",
                                    index_help="write <sorted_fn>.bai as index_bam does, with the same backend")
    return parser


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    try:
        r = sort_bam(args.bam_fn, args.sorted_fn, backend=args.backend, device=args.device, threads=args.bam_threads, memory=args.memory,
                     deflate=args.bgzf_deflate, index=args.index, force=args.force)
    except BamError as e:
        print("[ERROR] sort_bam: %s" % e, file=sys.stderr)
        sys.exit(1)
    print("[INFO] sort_bam (%s): %s: %d records (%d mapped, %d unplaced), %d group%s, %d read%s of the input%s, %d -> %d bytes"
          % (r["backend"], r["path"], r["records"], r["mapped"], r["unplaced"], r["groups"], "" if r["groups"] == 1 else "s", r["input_reads"],
             "" if r["input_reads"] == 1 else "s", " (it was sorted already)" if r["already_sorted"] else "", r["bytes_in"], r["bytes_out"]), file=sys.stderr)


if __name__ == "__main__":
    main()
