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
import ctypes
import os
import struct
import sys
from argparse import ArgumentParser

import numpy as np

from clair_amd import _hostapi, bgzf
from clair_amd._hostapi import BamError

BACKEND_WORDS = 8                                # clair_bamsort_backend_t: ctx and seven function pointers
BATCH_BLOCKS = 64                                # BGZF blocks per batch
STATS_WORDS = 7                                  # CLAIR_BAMSORT_STATS
MEMORY_DEFAULT = 8 << 30                         # record bytes held at once: a capacity, no measurement is behind it (docs/sort_bam.md)
RADIX_ITEMS = 8                                  # clair_bsort::RADIX_ITEMS (csrc/bam_sort_core.h)
RADIX_TILE = 256 * RADIX_ITEMS                   # keys per workgroup of a radix pass
PAYLOAD = bgzf.BLOCK_INPUT
HD_LINE = b"@HD\tVN:1.6\tSO:coordinate\n"
DEFLATE_MODES = {"own": 0, "zlib": 1, "host": 2}


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


def parse_memory(value):
    """BYTES[K|M|G] -> int"""
    if value is None:
        return MEMORY_DEFAULT
    if isinstance(value, (int, np.integer)):
        n = int(value)
    else:
        text = str(value).strip()
        shift = {"K": 10, "M": 20, "G": 30}.get(text[-1:].upper())
        try:
            n = int(text[:-1] if shift else text) << (shift or 0)
        except ValueError:
            raise BamError("--memory %s: BYTES, or BYTES with K, M or G behind" % value)
    if n < 1:
        raise BamError("--memory %s: at least one byte" % value)
    return n


class HostSorter(_hostapi.Handle):
    """clair_host_bamsort_*: the host twin.  segment_bytes 0: records framed by the sequential walk; a power of two: by the segmented rule."""
    _error = BamError
    name = "host"

    def __init__(self, threads=4, max_blocks=BATCH_BLOCKS, segment_bytes=0):
        self._lib = _hostapi.load()
        out = self._own(self._lib.clair_host_bamsort_destroy, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_bamsort_create(int(threads), int(max_blocks), int(segment_bytes), out))
        self.max_blocks = int(max_blocks)

    def backend(self):
        table = (ctypes.c_void_p * BACKEND_WORDS)()
        self._check(self._lib.clair_host_bamsort_backend(self._h, table))
        return table


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


class DeviceSorter(object):
    """clair_bamsort_*: the device backend (csrc/bam_sort.hip)."""
    name = "device"

    def __init__(self, device=0, max_blocks=BATCH_BLOCKS, segment_bytes=0):
        from clair_amd import _capi
        try:
            self._lib = _capi.load()
        except _capi.EngineError as e:
            raise BamError(str(e))
        self._h = ctypes.c_void_p()
        if self._lib.clair_bamsort_create(int(device), int(max_blocks), int(segment_bytes), ctypes.byref(self._h)) != 0:
            raise BamError("clair_bamsort_create failed: %s" % self._lib.clair_bamsort_last_error(None).decode())
        self.max_blocks = int(max_blocks)

    def _check(self, rc):
        if rc != 0:
            raise BamError(self._lib.clair_bamsort_last_error(self._h).decode())

    def backend(self):
        table = (ctypes.c_void_p * BACKEND_WORDS)()
        self._check(self._lib.clair_bamsort_backend(self._h, table))
        return table

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

    def close(self):
        if self._h:
            self._lib.clair_bamsort_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def header_blocks(data, deflate):
    """The header's bytes as BGZF blocks of their own.  zlib: Python's; host and device: the host twin of the device compressor, whose bytes
    are the device's (docs/merge_vcf.md): a few blocks of host work either way."""
    one = bgzf.zlib_block if deflate == "zlib" else _hostapi.deflate_bgzf
    return b"".join(one(data[k:k + PAYLOAD]) for k in range(0, len(data), PAYLOAD))


def sort_bam(bam_fn, sorted_fn, backend="auto", device=0, threads=4, memory=None, deflate=None, index=False, force=False, max_blocks=BATCH_BLOCKS,
             segment_bytes=None):
    """-> dict(records, mapped, unplaced, groups, input_reads, already_sorted, bytes_in, bytes_out, backend, path).  backend "auto": the device
    when one is present (a choice of convenience, not of measured speed: docs/sort_bam.md), else the host.  deflate None: the backend's own
    compressor.  segment_bytes None: the device's default segment, the host's sequential walk."""
    if backend not in ("auto", "device", "host"):
        raise BamError("--backend %s: auto, device or host" % backend)
    if deflate is not None and deflate not in bgzf.BACKENDS:
        raise BamError("--bgzf_deflate %s: %s" % (deflate, ", ".join(bgzf.BACKENDS)))
    if not isinstance(threads, int) or not 1 <= threads <= 16:
        raise BamError("--bam_threads %s: 1 .. 16" % threads)
    memory = parse_memory(memory)
    if not os.path.isfile(bam_fn):
        raise BamError("%s: cannot open" % bam_fn)
    if os.path.realpath(bam_fn) == os.path.realpath(sorted_fn) or (os.path.exists(sorted_fn) and os.path.samefile(bam_fn, sorted_fn)):
        raise BamError("%s: the output is the input" % sorted_fn)
    for fn in [sorted_fn] + ([sorted_fn + ".bai"] if index else []):
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
        raise BamError("--bgzf_deflate device compresses the device-resident sorted records: it needs --backend device")
    lib = _hostapi.load()
    job = ctypes.c_void_p()
    if lib.clair_host_bamsort_open(bam_fn.encode(), ctypes.byref(job)) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    tmp = "%s.tmp.%d" % (sorted_fn, os.getpid())
    sorter = None
    try:
        n = ctypes.c_int64()
        lib.clair_host_bamsort_header(job, None, 0, ctypes.byref(n))
        raw = np.zeros(n.value, dtype=np.uint8)
        lib.clair_host_bamsort_header(job, raw.ctypes.data, len(raw), ctypes.byref(n))
        if backend == "device":
            sorter = DeviceSorter(device=device, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
        else:
            sorter = HostSorter(threads=threads, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
        head = header_blocks(coordinate_header(raw.tobytes()), deflate)
        with open(tmp, "wb") as f:
            f.write(head)
        stats = np.zeros(STATS_WORDS, dtype=np.int64)
        mode = DEFLATE_MODES["own" if deflate == backend else deflate]
        if lib.clair_host_bamsort_run(job, sorter.backend(), tmp.encode(), mode, memory, int(max_blocks), threads, stats.ctypes.data) != 0:
            raise BamError(lib.clair_host_last_error().decode())
        os.replace(tmp, sorted_fn)
    finally:
        lib.clair_host_bamsort_close(job)
        if sorter is not None:
            sorter.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    result = dict(records=int(stats[0]), mapped=int(stats[1]), unplaced=int(stats[2]), groups=int(stats[3]), input_reads=int(stats[4]),
                  already_sorted=bool(stats[5]), bytes_in=os.path.getsize(bam_fn), bytes_out=len(head) + int(stats[6]), backend=backend, path=sorted_fn)
    if index:
        from clair_amd import index_bam
        index_bam.build_index(sorted_fn, backend=backend, device=device, threads=threads, force=force)
    return result


def build_parser():
    parser = ArgumentParser(description="Sort a BAM by coordinate, on the GPU or on the host, without samtools")
    add = parser.add_argument
    add('--bam_fn', type=str, required=True, help="the BAM to sort, in any order")
    add('--sorted_fn', type=str, required=True, help="the coordinate-sorted BAM to write")
    add('--backend', type=str, default="auto", choices=("auto", "device", "host"),
        help="where records are framed, sorted and gathered: the GPU, the host, or the GPU when one is present (convenience, not measured speed), default: %(default)s")
    add('--device', type=int, default=0, help="GPU of --backend device, default: %(default)s")
    add('--bam_threads', type=int, default=4, help="BGZF inflate and deflate threads on the host (1 .. 16), default: %(default)s")
    add('--memory', type=str, default=None, help="most record bytes held at once, BYTES[K|M|G]; a larger file is read once more per group, default: 8G")
    add('--bgzf_deflate', type=str, default=None, choices=bgzf.BACKENDS, help="who compresses the output's blocks, default: the backend itself")
    add('--index', action='store_true', help="write <sorted_fn>.bai as index_bam does, with the same backend")
    add('--force', action='store_true', help="overwrite an existing output")
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
