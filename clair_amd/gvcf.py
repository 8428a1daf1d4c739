"""gVCF output: the calls of a VCF plus reference-confidence blocks that tile everything in between, banded by genotype quality
(docs/gvcf.md).  The reference project writes no gVCF; the format is GATK's.

    python -m clair_amd.gvcf --bam_fn reads.bam --ref_fn ref.fa --ctgName chr20 [--ctgStart A --ctgEnd B] [--bed_fn r.bed]
                             --vcf_fn calls.vcf --gvcf_fn out.g.vcf [--backend device|host]

makes the gVCF for an existing call VCF; callVarBam --gvcf_fn writes it from the front end that is still alive when the calls are done.
The per-position rule (csrc/gvcf_core.h) runs over the candidate search's tallies: on the GPU (csrc/gvcf.hip, a segmented scan cuts the
bands into blocks) or in the host twin (hostsrc/host_gvcf.cpp); both give the same bytes.  Python computes the three integer costs from
--gvcf_error_rate once, builds the allowed set (region, bed, less the span of every call) and puts rows and blocks together."""
import ctypes
import logging
import math
import os
import sys
from argparse import ArgumentParser, Namespace
from time import time

import numpy as np

from . import _capi

BLOCK_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("min_dp", "<u4"), ("dp", "<u4"), ("gq", "<i4"), ("pl", "<i4", (3,))])   # clair_gvcf_block_t
assert BLOCK_DTYPE.itemsize == 40
SCAN_TILE = _capi.GVCF_SCAN_TILE             # positions one workgroup of the block scan takes
DEFAULT_ERROR_RATE = 0.1                     # a conservative, platform-neutral design default; not tuned (docs/gvcf.md)
DEFAULT_GQ_BANDS = list(range(1, 61)) + [70, 80, 90, 99]      # GATK's; 0 is implied
MAX_COST = (1 << 17) - 1
EXTRA_HEADER = ('##ALT=<ID=NON_REF,Description="Represents any possible alternative allele not already represented at this location by REF and ALT">\n'
                '##INFO=<ID=END,Number=1,Type=Integer,Description="Stop position of the interval">\n'
                '##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description="Minimum DP observed within the GVCF block">\n'
                '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Normalized, Phred-scaled likelihoods for genotypes as defined in the VCF specification">\n')


class GvcfArgumentError(ValueError):
    """A verdict of the host twin on an argument: the text clair_frontend_gvcf_blocks gives for the same argument."""


def costs_from(error_rate):
    """--gvcf_error_rate e -> (c_match, c_err, c_half) in 1/1024 phred: the only floating point of the stage."""
    e = float(error_rate)
    if not 0.0 < e < 1.0:
        raise ValueError("--gvcf_error_rate %r: a probability, 0 < e < 1" % error_rate)
    costs = tuple(int(round(-10.0 * math.log10(x) * 1024.0)) for x in (1.0 - e, e, 0.5))
    for name, c in zip(("c_match", "c_err", "c_half"), costs):
        if not 1 <= c <= MAX_COST:
            raise ValueError("--gvcf_error_rate %r: the cost %s = %d (1/1024 phred) is outside 1 .. %d" % (error_rate, name, c, MAX_COST))
    return costs


def parse_bands(text):
    """--gvcf_gq_bands "1,2,...,99" (or a list) -> the sorted lower bounds, 0 first"""
    if text is None:
        bounds = list(DEFAULT_GQ_BANDS)
    elif isinstance(text, str):
        try:
            bounds = [int(x) for x in text.replace(",", " ").split()]
        except ValueError:
            raise ValueError("--gvcf_gq_bands %r: integers separated by commas" % text)
    else:
        bounds = [int(x) for x in text]
    if any(not 0 <= b <= 99 for b in bounds) or any(b <= a for a, b in zip(bounds, bounds[1:])):
        raise ValueError("--gvcf_gq_bands: lower bounds in 0 .. 99, strictly ascending")
    return bounds if bounds and bounds[0] == 0 else [0] + bounds


def band_table(bounds):
    """lower bounds (0 first) -> uint8 [100]: the band of every GQ value"""
    return (np.searchsorted(np.asarray(bounds, dtype=np.int64), np.arange(100), side="right") - 1).astype(np.uint8)


def band_header(bounds):
    return "".join("##GVCFBlock%d-%d=minGQ=%d(inclusive),maxGQ=%d(exclusive)\n" % (a, b, a, b) for a, b in zip(bounds, bounds[1:] + [100]))


# ---- interval arithmetic (sorted, disjoint, half-open; NumPy throughout) ------------------------------------------------------------------
def _merge(st, en):
    st, en = np.asarray(st, dtype=np.int64), np.asarray(en, dtype=np.int64)
    keep = en > st
    st, en = st[keep], en[keep]
    if not len(st):
        return st, en
    order = np.argsort(st, kind="stable")
    st, en = st[order], np.maximum.accumulate(en[order])
    new = np.concatenate([[True], st[1:] > en[:-1]])
    return st[new], en[np.concatenate([new[1:], [True]])]


def _inside(st, en, p):
    if not len(st):
        return np.zeros(len(p), dtype=bool)
    i = np.searchsorted(st, p, side="right") - 1
    return (i >= 0) & (p < en[np.maximum(i, 0)])


def _combine(a, b, keep):
    cuts = np.unique(np.concatenate([a[0], a[1], b[0], b[1]]))
    if len(cuts) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    left = cuts[:-1]
    k = keep(_inside(a[0], a[1], left), _inside(b[0], b[1], left))
    return _merge(left[k], cuts[1:][k])


def allowed_intervals(span, table, bed, var_start, var_end):
    """span = (lo, hi) 0-based half-open: the region, or the contig; table: the span the tallies cover; bed = (starts, ends) merged, or None;
    var_*: [POS - 1, POS - 1 + len(REF)) of every row of the call VCF -> (starts, ends) of span & table & bed - rows, maximal runs."""
    lo, hi = max(span[0], table[0]), min(span[1], table[1])
    cur = _merge([lo], [hi])
    if bed is not None:
        cur = _combine(cur, _merge(bed[0], bed[1]), lambda x, y: x & y)
    if len(var_start):
        cur = _combine(cur, _merge(var_start, var_end), lambda x, y: x & ~y)
    return cur


# ---- the call VCF --------------------------------------------------------------------------------------------------------------------------
def read_call_vcf(path, ctg_name):
    """-> (header lines, rows of ctg_name as written, their 0-based POS int64, len(REF) int64)"""
    header, rows, pos, length = [], [], [], []
    import gzip
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        for line in f:
            if line.startswith("#"):
                header.append(line if line.endswith("\n") else line + "\n")
                continue
            col = line.split("\t", 5)
            if len(col) < 5:
                if line.strip():
                    sys.exit("[ERROR] %s: a row with fewer than five columns" % path)
                continue
            if col[0] != ctg_name:
                continue
            rows.append(line if line.endswith("\n") else line + "\n")
            pos.append(int(col[1]) - 1)
            length.append(max(len(col[3]), 1))
    return header, rows, np.array(pos, dtype=np.int64), np.array(length, dtype=np.int64)


def with_non_ref(row):
    """a variant row with <NON_REF> as one more alternate allele (the only allele of a --showRef row, whose ALT is '.')"""
    col = row.split("\t", 5)
    col[4] = "<NON_REF>" if col[4] in (".", "") else col[4] + ",<NON_REF>"
    return "\t".join(col)


# ---- the two backends ----------------------------------------------------------------------------------------------------------------------
class HostTallies(object):
    """The host twin's tables: what DeviceFrontEnd.feed() fills in place of a device front end (add_slab), through clair_host_gvcf_tally."""

    def __init__(self, lo, hi):
        self.lo, self.n = int(lo), int(hi) - int(lo)
        self.tallies = np.zeros((self.n, 7), dtype=np.uint32)
        self.anomalies = 0

    def add_arrays(self, reads, ops, op_elem, seq):
        from . import _hostapi
        reads, ops = np.ascontiguousarray(reads, dtype=_hostapi.READ_DTYPE), np.ascontiguousarray(ops, dtype=_hostapi.OP_DTYPE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self._tally(reads.ctypes.data, len(reads), ops.ctypes.data, len(ops), seq.ctypes.data, len(seq))

    def add_slab(self, packer):
        (r, o, _, q), st = packer.slab_pointers()
        if st["reads"] and st["ops"]:
            self._tally(r, st["reads"], o, st["ops"], q, st["seq_bytes"])
        packer.reset()

    def _tally(self, reads, n_reads, ops, n_ops, seq, seq_bytes):
        from . import _hostapi
        lib = _hostapi.load()
        bits = ctypes.c_uint32(0)
        if lib.clair_host_gvcf_tally(reads, n_reads, ops, n_ops, seq, seq_bytes, self.lo, self.n, self.tallies.ctypes.data, ctypes.byref(bits)):
            raise ValueError(lib.clair_host_last_error().decode())
        self.anomalies |= bits.value


def _ref_bytes(ref):
    return np.frombuffer(ref.encode("latin-1") if isinstance(ref, str) else bytes(ref), dtype=np.uint8)


def host_blocks(tallies, lo, ref, ref0, costs, band_of_gq, iv_start, iv_end, guard=0):
    """clair_host_gvcf_blocks -> records (BLOCK_DTYPE); guard as clair_amd._capi.Frontend.gvcf_blocks'"""
    from . import _hostapi
    lib = _hostapi.load()
    t = np.ascontiguousarray(tallies, dtype=np.uint32)
    r = _ref_bytes(ref)
    bands = np.ascontiguousarray(band_of_gq, dtype=np.uint8)
    st, en = np.ascontiguousarray(iv_start, dtype=np.int64), np.ascontiguousarray(iv_end, dtype=np.int64)
    if bands.shape != (100,) or st.shape != en.shape or st.ndim != 1:
        raise ValueError("host_blocks: a band table of 100 entries and two interval arrays of one length")
    n = ctypes.c_int64(0)

    def call(out, capacity):
        rc = lib.clair_host_gvcf_blocks(t.ctypes.data, int(lo), len(t), r.ctypes.data, len(r), int(ref0), int(costs[0]), int(costs[1]), int(costs[2]),
                                        bands.ctypes.data, st.ctypes.data, en.ctypes.data, len(st), None if out is None else out.ctypes.data, capacity,
                                        ctypes.byref(n))
        if rc:
            raise (GvcfArgumentError if rc == 2 else ValueError)(lib.clair_host_last_error().decode())
    call(None, 0)
    out = np.empty(n.value + int(guard), dtype=BLOCK_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    if n.value:
        call(out, n.value)
    return out if guard else out[:n.value]


def format_blocks(records, ctg_name, ref, ref0):
    """clair_host_gvcf_format -> (the rows as one bytes-like buffer, int64 offsets [n + 1] of the rows in it)"""
    from . import _hostapi
    lib = _hostapi.load()
    rec = np.ascontiguousarray(records, dtype=BLOCK_DTYPE)
    r = _ref_bytes(ref)
    n = len(rec)
    offsets = np.zeros(n + 1, dtype=np.int64)
    cap = n * (len(ctg_name.encode()) + 96) + 64
    while True:
        out = np.empty(cap, dtype=np.uint8)
        need = ctypes.c_int64(0)
        if lib.clair_host_gvcf_format(rec.ctypes.data, 0, n, ctg_name.encode(), r.ctypes.data, len(r), int(ref0), out.ctypes.data, cap, ctypes.byref(need),
                                      offsets.ctypes.data):
            raise ValueError(lib.clair_host_last_error().decode())
        if need.value <= cap:
            return memoryview(out)[:need.value], offsets
        cap = need.value


def device_or_host_blocks(frontend, twin, costs, band_of_gq, iv_start, iv_end):
    """The blocks from a device front end; where it refuses because the front end reported an anomaly bit (its tallies may be incomplete),
    twin() -- the host twin over the same alignments -- answers instead.  -> (records, "device" or "host")"""
    try:
        return frontend.gvcf_blocks(costs, band_of_gq, iv_start, iv_end), "device"
    except _capi.TalliesIncomplete as exc:
        logging.info("gvcf: %s" % exc)
        return twin(), "host"


# ---- the file ------------------------------------------------------------------------------------------------------------------------------
def gvcf_text_parts(header, rows, row_pos, records, ctg_name, ref, ref0, bounds, sample_name="SAMPLE"):
    """The gVCF as a list of bytes-like pieces: the call VCF's header with the gVCF lines, then rows and block rows interleaved by position
    (the split points by searchsorted over the block starts: no Python loop over blocks)."""
    extra = EXTRA_HEADER + band_header(bounds)
    head = [h for h in header if not h.startswith("#CHROM")]
    chrom = [h for h in header if h.startswith("#CHROM")]
    if not head:
        head = ["##fileformat=VCFv4.1\n"]
    if not chrom:
        chrom = ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % sample_name]
    parts = [("".join(head) + extra + chrom[0]).encode()]
    text, off = format_blocks(records, ctg_name, ref, ref0)
    n = len(records)
    prev = 0
    if len(rows):
        k = np.maximum.accumulate(np.searchsorted(records["start"], row_pos, side="left"))
        for row, ki in zip(rows, k.tolist()):
            if ki > prev:
                parts.append(text[off[prev]:off[ki]])
                prev = ki
            parts.append(with_non_ref(row).encode())
    if n > prev:
        parts.append(text[off[prev]:off[n]])
    return parts


def _front_end_args(opts):
    """what clair_amd.callVarBam.DeviceFrontEnd reads of its arguments, for a run that only feeds alignments"""
    keep = ("bam_fn", "ref_fn", "bed_fn", "ctgName", "ctgStart", "ctgEnd", "dcov", "samtools", "samtools_threads", "samtools_view_args", "view_readers",
            "bam_reader", "bam_threads", "bam_inflate", "device")
    defaults = dict(dcov=250, samtools="samtools", samtools_threads=0, samtools_view_args=None, view_readers=1, bam_reader="samtools", bam_threads=4,
                    bam_inflate="host", device=0, bed_fn=None)
    a = Namespace(**{k: getattr(opts, k, defaults.get(k)) for k in keep})
    a.vcf_fn, a.front_end, a.indel_lookup, a.subsample = None, "device", "pysam", None
    return a


def make_gvcf(opts, live=None):
    """opts: bam_fn, ref_fn, ctgName, ctgStart, ctgEnd, bed_fn, vcf_fn (the call VCF), gvcf_fn, backend, device, gvcf_error_rate, gvcf_gq_bands and
    the alignment-reading options of callVarBam.  live: a callVarBam.DeviceFrontEnd whose front end still holds the region's tallies (the BAM
    is then not read again).  -> dict(blocks, rows, backend, seconds)"""
    from . import callVarBam
    from ._hostapi import merged_bed
    t_start = time()
    costs = costs_from(DEFAULT_ERROR_RATE if opts.gvcf_error_rate is None else opts.gvcf_error_rate)
    bounds = parse_bands(opts.gvcf_gq_bands)
    bands = band_table(bounds)
    header, rows, row_pos, row_len = read_call_vcf(opts.vcf_fn, opts.ctgName)
    feeder = {}

    def feed_into(sink):
        """the region's alignments through DeviceFrontEnd's view and packer code -> the packer's statistics"""
        if not feeder:
            feeder["fe"] = callVarBam.DeviceFrontEnd(_front_end_args(opts), opts.device, pinned=None)
            feeder["region"] = feeder["fe"].tables(search=True)[5]
        return feeder["fe"].feed(sink, feeder["region"])[0]

    fe = live if live is not None and live.frontend is not None else None
    if fe is not None:
        info = fe.table_info
    else:
        feeder["fe"] = callVarBam.DeviceFrontEnd(_front_end_args(opts), opts.device, pinned=None)
        feeder["region"] = feeder["fe"].tables(search=True)[5]
        info = feeder["fe"].table_info
    seq, ref0, lo, hi = info["seq"], info["ref0"], info["lo"], info["hi"]
    have_range = opts.ctgStart is not None and opts.ctgEnd is not None
    span = (opts.ctgStart - 1, opts.ctgEnd) if have_range else (ref0, ref0 + len(seq))
    bs, be, n_bed = merged_bed(info["bed"])
    inside = (max(lo, ref0), min(hi, ref0 + len(seq)))          # the tables, and no position past the end of the contig (--ctgEnd may lie beyond it)
    st, en = allowed_intervals(span, inside, None if n_bed < 0 else (bs, be), row_pos, row_pos + row_len)

    def host():
        tallies = HostTallies(lo, hi)
        if feed_into(tallies)["evc_reads"] == 0:
            logging.info("gvcf: no alignment of %s passes the candidate search's filters: every block has GQ 0" % opts.bam_fn)
        return host_blocks(tallies.tallies, lo, seq, ref0, costs, bands, st, en)

    t_blocks = time()
    if fe is not None:
        records, backend = device_or_host_blocks(fe.frontend, host, costs, bands, st, en)
    elif opts.backend == "host":
        records, backend = host(), "host"
    else:
        f = _capi.Frontend(opts.device, seq, ref0, lo, hi)
        try:
            bits = feed_into(f)["anomalies"]
            if bits:        # what the host packer saw (unsorted input, ...) the device handle does not know of
                logging.info("gvcf: the packer reported anomaly bits 0x%x: the host twin runs" % bits)
                records, backend = host(), "host"
            else:
                records, backend = device_or_host_blocks(f, host, costs, bands, st, en)
        finally:
            f.close()
    t_blocks = time() - t_blocks
    parts = gvcf_text_parts(header, rows, row_pos, records, opts.ctgName, seq, ref0, bounds, getattr(opts, "sampleName", "SAMPLE"))
    with open(opts.gvcf_fn, "wb") as out:
        out.writelines(parts)
    seconds = time() - t_start
    logging.info("gvcf: %d blocks between %d rows -> %s (%s backend; blocks %.3f s, stage %.3f s)" % (len(records), len(rows), opts.gvcf_fn, backend, t_blocks, seconds))
    return dict(blocks=len(records), rows=len(rows), backend=backend, seconds=seconds)


def check_options(opts):
    """the two --gvcf_* options, checked before anything runs: exits with the message"""
    try:
        costs_from(DEFAULT_ERROR_RATE if opts.gvcf_error_rate is None else opts.gvcf_error_rate)
        parse_bands(opts.gvcf_gq_bands)
    except ValueError as exc:
        sys.exit("[ERROR] %s" % exc)


def after_calls(args, device_fe):
    """callVarBam --gvcf_fn, once the call VCF is closed: from the live front end, or (host front end, or the device one handed the region
    back) by the stand-alone path with the host backend, which reads the region once more."""
    opts = Namespace(**vars(args))
    opts.vcf_fn = args.call_fn
    live = device_fe if device_fe is not None and device_fe.frontend is not None else None
    opts.backend = "device" if live is not None else "host"
    return make_gvcf(opts, live=live)


def add_gvcf_options(add):
    add('--gvcf_error_rate', type=float, default=None,
        help="gVCF: the per-read error rate e of the reference-confidence model, default: %g (a conservative design default, not calibrated per platform)" % DEFAULT_ERROR_RATE)
    add('--gvcf_gq_bands', type=str, default=None,
        help="gVCF: lower bounds of the GQ bands, ascending, comma separated, in 0 .. 99 (0 is implied); default: GATK's 1,2,...,60,70,80,90,99")


def build_parser():
    parser = ArgumentParser(description="the gVCF of an existing call VCF: its rows plus reference-confidence blocks banded by GQ (docs/gvcf.md)")
    add = parser.add_argument
    add('--bam_fn', type=str, required=True, help="sorted alignments the calls were made from")
    add('--ref_fn', type=str, required=True, help="reference FASTA with its .fai")
    add('--ctgName', type=str, required=True, help="contig to process")
    add('--ctgStart', type=int, default=None, help="1-based first position of the region")
    add('--ctgEnd', type=int, default=None, help="1-based last position of the region (inclusive)")
    add('--bed_fn', type=str, default=None, help="restrict the blocks to these intervals (intersected with the region)")
    add('--vcf_fn', type=str, required=True, help="the call VCF (callVarBam --call_fn) of the same contig / region")
    add('--gvcf_fn', type=str, required=True, help="output gVCF")
    add('--backend', type=str, default="device", choices=("device", "host"), help="where the rule and the banding run: on the GPU or in the host twin (same bytes), default: %(default)s")
    add('--device', type=int, default=0, help="HIP device ordinal, default: %(default)s")
    add_gvcf_options(add)
    add('--sampleName', type=str, default="SAMPLE", help="sample column, used only when the call VCF has no header")
    add('--dcov', type=int, default=250, help="as callVarBam's (the pileup's cap; the tallies count every alignment the search accepts), default: %(default)s")
    add('--samtools', type=str, default="samtools", help="samtools executable")
    add('--samtools_threads', type=int, default=0, help="as callVarBam's")
    add('--samtools_view_args', type=str, default=None, help="as callVarBam's")
    add('--view_readers', type=int, default=1, help="as callVarBam's")
    add('--bam_reader', type=str, default="samtools", choices=("samtools", "native"), help="as callVarBam's: `samtools view` or the native BAM reader")
    add('--bam_threads', type=int, default=4, help="as callVarBam's")
    add('--bam_inflate', type=str, default="host", choices=("host", "device"), help="as callVarBam's")
    return parser


def main(argv=None):
    opts = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    for path in (opts.bam_fn, opts.ref_fn, opts.vcf_fn):
        if not os.path.isfile(path):
            sys.exit("[ERROR] file %s not found" % path)
    if opts.ctgStart is not None and opts.ctgEnd is not None and opts.ctgStart > opts.ctgEnd:
        opts.ctgStart = opts.ctgEnd = None              # as callVarBam reads such a pair
    if (opts.ctgStart is None) != (opts.ctgEnd is None):
        opts.ctgStart = opts.ctgEnd = None
    check_options(opts)
    try:
        make_gvcf(opts)
    except _capi.EngineError as exc:
        sys.exit("[ERROR] %s" % exc)


if __name__ == "__main__":
    main()
