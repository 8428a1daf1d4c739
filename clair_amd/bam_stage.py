"""What index_bam, sort_bam and markdup_bam share (docs/index_bam.md, docs/sort_bam.md, docs/markdup_bam.md): the checks of their arguments,
the choice of the backend, the two kinds of backend handle, the options of their command lines, and -- for the two that rewrite a BAM --
the driver: the job opened (clair_host_bam_job_*), the header's blocks written to a temporary file, the stage's file driver
(clair_host_<prefix>_run) appending the records' blocks and the EOF marker, the file renamed, the index on request."""
import ctypes
import os

import numpy as np

from clair_amd import _hostapi, bgzf
from clair_amd._hostapi import BamError

BATCH_BLOCKS = 64                                # BGZF blocks per batch: 4 MiB of records at a time
MEMORY_DEFAULT = 8 << 30                         # bytes held at once: a capacity, no measurement is behind it (docs/sort_bam.md)
PAYLOAD = bgzf.BLOCK_INPUT
DEFLATE_MODES = {"own": 0, "zlib": 1, "host": 2}


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


def header_blocks(data, deflate):
    """The header's bytes as BGZF blocks of their own.  zlib: Python's; host and device: the host twin of the device compressor, whose bytes
    are the device's (docs/merge_vcf.md): a few blocks of host work either way."""
    one = bgzf.zlib_block if deflate == "zlib" else _hostapi.deflate_bgzf
    return b"".join(one(data[k:k + PAYLOAD]) for k in range(0, len(data), PAYLOAD))


def check_threads(threads):
    if not isinstance(threads, int) or not 1 <= threads <= 16:
        raise BamError("--bam_threads %s: 1 .. 16" % threads)


def resolve_backend(backend):
    """auto -> device when one is present, else host"""
    if backend not in ("auto", "device", "host"):
        raise BamError("--backend %s: auto, device or host" % backend)
    if backend == "auto":
        backend = "host"
        try:
            from clair_amd import _capi
            if _capi.load().clair_device_count() > 0:
                backend = "device"
        except Exception:
            pass
    return backend


def check_outputs(in_fn, out_fn, index, force):
    if not os.path.isfile(in_fn):
        raise BamError("%s: cannot open" % in_fn)
    if os.path.realpath(in_fn) == os.path.realpath(out_fn) or (os.path.exists(out_fn) and os.path.samefile(in_fn, out_fn)):
        raise BamError("%s: the output is the input" % out_fn)
    for fn in [out_fn] + ([out_fn + ".bai"] if index else []):
        if os.path.exists(fn) and not force:
            raise BamError("%s exists: --force overwrites it" % fn)


class Backend(_hostapi.Handle):
    """The handle of one backend of a stage: a subclass names the stage's prefix and the words of its backend table (ctx and the entry points)."""
    _error = BamError
    prefix, words, _symbol = None, 0, None

    def _fn(self, name):
        return getattr(self._lib, self._symbol % (self.prefix, name))

    def backend(self):
        table = (ctypes.c_void_p * self.words)()
        self._check(self._fn("backend")(self._h, table))
        return table


class HostBackend(Backend):
    """clair_host_<prefix>_*: a host twin.  segment_bytes 0: records framed by the sequential walk; a power of two: by the segmented rule."""
    name, _symbol = "host", "clair_host_%s_%s"

    def __init__(self, threads=4, max_blocks=BATCH_BLOCKS, segment_bytes=0):
        self._lib = _hostapi.load()
        out = self._own(self._fn("destroy"), self._lib.clair_host_last_error)
        self._check(self._fn("create")(int(threads), int(max_blocks), int(segment_bytes), out))
        self.max_blocks = int(max_blocks)


class DeviceBackend(Backend):
    """clair_<prefix>_*: a device backend (csrc/bam_index.hip, bam_sort.hip, markdup.hip)."""
    name, _symbol = "device", "clair_%s_%s"

    def __init__(self, device=0, max_blocks=BATCH_BLOCKS, segment_bytes=0):
        from clair_amd import _capi
        try:
            self._lib = _capi.load()
        except _capi.EngineError as e:
            raise BamError(str(e))
        out = self._own(self._fn("destroy"), lambda: self._fn("last_error")(self._h or None))
        self._check(self._fn("create")(int(device), int(max_blocks), int(segment_bytes), out), "clair_%s_create failed: " % self.prefix)
        self.max_blocks = int(max_blocks)


def rewrite(bam_fn, out_fn, *, host, device_backend, header_of, run_args, stats_words, device_needs, backend, device, threads, memory, deflate, index,
            force, max_blocks, segment_bytes):
    """The driver of a tool that rewrites a BAM -> (stats, bytes of the header's blocks, the backend's name).  host, device_backend: the
    stage's two backend classes; header_of: the header's bytes -> those to write; run_args: what clair_host_<prefix>_run takes between the
    threads and the stats; device_needs: what --bgzf_deflate device compresses, for the message."""
    backend = resolve_backend(backend)
    if deflate is not None and deflate not in bgzf.BACKENDS:
        raise BamError("--bgzf_deflate %s: %s" % (deflate, ", ".join(bgzf.BACKENDS)))
    check_threads(threads)
    memory = parse_memory(memory)
    check_outputs(bam_fn, out_fn, index, force)
    deflate = deflate or backend
    if deflate == "device" and backend != "device":
        raise BamError("--bgzf_deflate device compresses the device-resident %s: it needs --backend device" % device_needs)
    lib = _hostapi.load()
    job = ctypes.c_void_p()
    if lib.clair_host_bam_job_open(bam_fn.encode(), ctypes.byref(job)) != 0:
        raise BamError(lib.clair_host_last_error().decode())
    tmp = "%s.tmp.%d" % (out_fn, os.getpid())
    stage = None
    try:
        n = ctypes.c_int64()
        lib.clair_host_bam_job_header(job, None, 0, ctypes.byref(n))
        raw = np.zeros(n.value, dtype=np.uint8)
        lib.clair_host_bam_job_header(job, raw.ctypes.data, len(raw), ctypes.byref(n))
        if backend == "device":
            stage = device_backend(device=device, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
        else:
            stage = host(threads=threads, max_blocks=max_blocks, segment_bytes=segment_bytes or 0)
        head = header_blocks(header_of(raw.tobytes()), deflate)
        with open(tmp, "wb") as f:
            f.write(head)
        stats = np.zeros(stats_words, dtype=np.int64)
        mode = DEFLATE_MODES["own" if deflate == backend else deflate]
        run = getattr(lib, "clair_host_%s_run" % host.prefix)
        if run(job, stage.backend(), tmp.encode(), mode, memory, int(max_blocks), threads, *(tuple(run_args) + (stats.ctypes.data,))) != 0:
            raise BamError(lib.clair_host_last_error().decode())
        os.replace(tmp, out_fn)
    finally:
        lib.clair_host_bam_job_close(job)
        if stage is not None:
            stage.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    if index:
        from clair_amd import index_bam
        index_bam.build_index(out_fn, backend=backend, device=device, threads=threads, force=force)
    return stats, len(head), backend


def add_backend_arguments(parser, does, threads_help, speed="convenience, not measured speed", force_help="overwrite an existing output", memory_help=None,
                          index_help=None):
    """--backend, --device, --bam_threads, then (the tools that rewrite a BAM: memory_help, index_help) --memory, --bgzf_deflate, --index,
    and --force.  does: what a backend does to the records, for the help of --backend."""
    add = parser.add_argument
    add('--backend', type=str, default="auto", choices=("auto", "device", "host"),
        help="where records are %s: the GPU, the host, or the GPU when one is present (%s), default: %%(default)s" % (does, speed))
    add('--device', type=int, default=0, help="GPU of --backend device, default: %(default)s")
    add('--bam_threads', type=int, default=4, help="%s (1 .. 16), default: %%(default)s" % threads_help)
    if memory_help:
        add('--memory', type=str, default=None, help=memory_help)
        add('--bgzf_deflate', type=str, default=None, choices=bgzf.BACKENDS, help="who compresses the output's blocks, default: the backend itself")
        add('--index', action='store_true', help=index_help)
    add('--force', action='store_true', help=force_help)
