"""BAM -> VCF for one contig / region: candidate extraction, pileup tensors, network, decode, in ONE process.

Host-side mirror of the reference's clair/callVarBam.py (same flags).  The reference wires three interpreters together with
text pipes (callVarBam.py:124-199): `pypy ExtractVariantCandidates | pypy CreateTensor | python call_var`, 2.3 KB of decimal
text per candidate on the second pipe.  Here the same three stages are native code in one process and hand each other
arrays:

    samtools view  -> clair_host_evc_*     -> candidate positions (int64)
    samtools view  -> clair_host_pileup_*  -> count windows int32 [n,33,8,4] + (position, refseq)
                   -> float32, channels 1..3 minus channel 0 (clair/utils.py:96-98), centre-base filter (:90-91)
                   -> HIP forward pass (libclair_amd.so) -> native decode -> VCF rows

The VCF is the one `extract_variant_candidates | create_tensor | call_var` produce through their text interfaces
(tests/test_pileup.py pins that), which in turn are pinned against the reference scripts.  Like the reference, alignments
are read twice (`samtools view` once per stage): the pileup needs the candidates ahead of the reads.

--front_end device (the default where it applies) moves both stages to the GPU (include/clair_amd.h: clair_frontend_*):

    samtools view  -> clair_host_sampack_* (ONE pass over the text) -> packed alignments, resident in HBM
                   -> per-position tables -> candidate filter -> windows int16 [n,33,8,4] that never leave the device
                   -> HIP forward pass + decode kernel -> call records -> VCF rows

Same candidates, same windows, same VCF (tests/test_frontend_gpu.py, tests/test_e2e_gpu.py); where the input leaves the regime
that formulation reproduces exactly (CLAIR_FE_* in include/clair_reads.h, a tuple budget that binds) the run falls back to the
host stages above and says so.

--bam_reader native reads the BAM without samtools (include/clair_host.h: clair_host_bam_*; docs/bam_reader.md): BGZF inflated on
--bam_threads host threads (or on the GPU, a wave per block: --bam_inflate device), the region's records found with the .bai, and with the device front end the binary records go to the GPU
as they are (clair_frontend_add_bam), which decodes them and applies the view's filter itself.  The host stages, and the device front
end's fall-back, read the text `samtools view` would have printed, rendered from the records; the reference slice comes from the .fai.
--subsample FRAC / --ensemble_subsample FRAC[:SEED] add what `samtools view -s` adds to that view, on the GPU or in the renderer: --bam_fn
at a fraction of its reads, as the BAM itself or as further sources of the ensemble across BAMs (docs/subsample.md).
"""
import logging
import os
import shlex
import sys
from argparse import ArgumentParser

import numpy as np

from . import call_var as cv
from . import create_tensor as ct
from . import extract_variant_candidates as evc
from . import param

IUPAC = frozenset("ACGTURYSWKMBDHVN")


def view_command(args, region):
    """`samtools view -F 2316 <bam> <region>` as the reference spawns it (CreateTensor.py:163-170), plus -@ N with --samtools_threads N
    (BGZF blocks inflated on N extra threads: the text that comes out is the same)."""
    threads = getattr(args, "samtools_threads", 0) or 0
    extra = getattr(args, "samtools_view_args", None) or ""
    return shlex.split("%s view %s%s-F %d %s %s" % (args.samtools, "-@ %d " % threads if threads > 0 else "", extra + " " if extra else "",
                                                  ct.SAMTOOLS_VIEW_FILTER_FLAG, args.bam_fn, region))


def split_region(region):
    """samtools' region syntax -> (ctg, start, end) 1-based inclusive, or (ctg, None, None) for a whole contig."""
    import re
    m = re.fullmatch(r"(.+):(\d+)-(\d+)", region)
    return (m.group(1), int(m.group(2)), int(m.group(3))) if m else (region, None, None)


def native_reader(args, region):
    """--bam_reader native: a clair_amd._hostapi.BamReader positioned on `region` (samtools' syntax).  What it cannot read ends the run."""
    from . import _hostapi
    ctg, lo, hi = split_region(region)
    try:
        reader = _hostapi.BamReader(args.bam_fn, threads=getattr(args, "bam_threads", 4), inflate=getattr(args, "bam_inflate", "host"),
                                    device=getattr(args, "device", 0))
        if not reader.info()["eof_block"]:
            logging.warning("[W::bgzf] %s: no BGZF EOF marker; the file may be truncated" % args.bam_fn)
        if not reader.query(ctg, lo, hi):
            logging.info("%s has no .bai index: reading it from the first record" % args.bam_fn)
        if subsample_of(args) is not None:              # for the text it renders: the host stages' and the device front end's hand-back
            frac, seed = subsample_of(args)
            reader.set_subsample(seed, frac)
    except _hostapi.BamError as exc:
        sys.exit("[ERROR] %s" % exc)
    return reader


class _NativeText(object):
    """What `samtools view -F 2316 <bam> <region>` prints, rendered from the BAM's records without samtools: read() / readinto() / abort() /
    finish() like _OnePipe."""

    def __init__(self, args, region):
        from . import _hostapi
        self.text = _hostapi.BamText(native_reader(args, region))

    def read(self, n):
        from . import _hostapi
        try:
            return self.text.read(n)
        except _hostapi.BamError as exc:
            sys.exit("[ERROR] %s" % exc)

    def readinto(self, mv):
        from . import _hostapi
        try:
            return self.text.readinto(mv)
        except _hostapi.BamError as exc:
            sys.exit("[ERROR] %s" % exc)

    def abort(self):
        self.text.abort()

    def finish(self):
        return self.text.finish()


def alignment_text(args, region):
    """The alignments of `region` as `samtools view -F 2316` text: from samtools (the default) or rendered natively (--bam_reader native)."""
    if native_input(args):
        return _NativeText(args, region)
    return _OnePipe(args, region)


def native_input(args):
    return getattr(args, "bam_reader", "samtools") == "native"


def native_lookup(args):
    return getattr(args, "indel_lookup", "pysam") == "native"


def subsample_of(args):
    """--subsample / --subsample_seed -> (fraction, seed) of the reads --bam_fn is read at, or None for all of them (docs/subsample.md)"""
    frac = getattr(args, "subsample", None)
    return None if frac is None else (float(frac), int(getattr(args, "subsample_seed", 0) or 0))


def check_subsample_fraction(flag, frac, seed):
    if not 0.0 < frac <= 1.0:                       # (NaN fails both)
        sys.exit("[ERROR] %s %r: a fraction of the reads, 0 < FRAC <= 1" % (flag, frac))
    if not 0 <= seed <= 0xffffffff:
        sys.exit("[ERROR] %s: seed %d: 0 .. 4294967295" % (flag, seed))


def check_subsample_flags(args):
    """--subsample, --subsample_seed, --ensemble_subsample: what they need; args.ensemble_subsample becomes [(fraction, seed), ...]."""
    seed = int(getattr(args, "subsample_seed", 0) or 0)
    virtual = []
    for text in getattr(args, "ensemble_subsample", None) or []:
        if isinstance(text, tuple):                 # normalised before
            virtual.append(text)
            continue
        frac, colon, own = text.partition(":")
        try:
            virtual.append((float(frac), int(own) if colon else seed))
        except ValueError:
            sys.exit("[ERROR] --ensemble_subsample %s: FRAC or FRAC:SEED, a fraction and an integer" % text)
        check_subsample_fraction("--ensemble_subsample %s" % text, *virtual[-1])
    args.ensemble_subsample = virtual or None
    if subsample_of(args) is not None:
        check_subsample_fraction("--subsample", *subsample_of(args))
    elif not virtual and not seed:
        return
    check_subsample_fraction("--subsample_seed", 1.0, seed)
    if not native_input(args):
        sys.exit("[ERROR] --subsample, --subsample_seed and --ensemble_subsample select reads in the native reader's view: add --bam_reader native "
                 "(for a single BAM, --samtools_view_args \"-s SEED.FRAC\" already hands the job to samtools)")
    if subsample_of(args) is not None and not native_lookup(args):
        sys.exit("[ERROR] --subsample with --indel_lookup pysam: pysam would look indels up in the whole file while the call is made from a "
                 "subset of its reads; --indel_lookup native answers from the alignments the front end kept: add it")


def reference_and_bed(args, search, not_loaded):
    """What both front ends start with: the reference slice of the region (widened by 1 Mbp: the two stages load the same one,
    ExtractVariantCandidates.py:228-236, CreateTensor.py:113-156) and, where candidates are searched for, the .fai looked for before it and the
    bed intervals of the contig after it.  not_loaded: the exit message for a slice that cannot be had (the stages word it differently).
    -> (sequence, its 0-based start, bed intervals or None)"""
    if search and not os.path.isfile("%s.fai" % args.ref_fn):
        sys.exit("Fasta index %s.fai doesn't exist." % args.ref_fn)
    seq, ref_start = ct.reference_sequence_from(args.samtools, args.ref_fn, args.ctgName, args.ctgStart, args.ctgEnd, native=native_input(args))
    if not seq:
        sys.exit(not_loaded)
    tree = evc.bed_regions_from(args.bed_fn) if search else None
    if tree is not None and args.ctgName not in tree:
        sys.exit("[ERROR] ctg_name(%s) not exists in bed file(%s)." % (args.ctgName, args.bed_fn))
    return seq, 0 if ref_start is None else ref_start - 1, None if tree is None else tree[args.ctgName]


def window_infos(ctg_name, centres, seqs):
    """[[ctg, pos, refseq], ...] of a batch of windows (centres int64 [n], seqs uint8 [n,34] NUL-terminated): in column form, without a Python
    string per window (tensor_binary.InfoTable), or the list itself for a contig name too long for that."""
    from .tensor_binary import MAX_CTG, InfoTable
    ctg, n = ctg_name.encode(), len(centres)
    if len(ctg) <= MAX_CTG:
        return InfoTable(np.full(n, ctg, dtype="S%d" % MAX_CTG), np.full(n, len(ctg), dtype=np.uint8), centres,
                         np.ascontiguousarray(seqs[:, :33]).view("S33").ravel(), (seqs[:, :33] != 0).sum(axis=1).astype(np.uint8))
    raw = seqs.tobytes()
    return [[ctg_name, str(c), raw[i * 34:i * 34 + 34].split(b"\0", 1)[0].decode("latin-1")] for i, c in enumerate(centres.tolist())]


def candidate_positions(args, quiet=False):
    """Stage 1.  -> int64 positions (1-based, ascending for sorted alignments)."""
    from . import _hostapi
    if args.vcf_fn is not None:
        return positions_from_vcf(args.vcf_fn, args.ctgName, args.ctgStart, args.ctgEnd)
    seq, ref0, bed = reference_and_bed(args, True, "[ERROR] Failed to load reference seqeunce from file (%s)." % args.ref_fn)
    have_range = args.ctgStart is not None and args.ctgEnd is not None
    finder = _hostapi.CandidateFinder(args.ctgName, seq, ref0, ctg_start=args.ctgStart if have_range else None,
                                      ctg_end=args.ctgEnd if have_range else None, bed=bed,
                                      min_coverage=int(args.minCoverage), threshold=args.threshold, min_mq=0)   # callVarBam.py:75: int() before it reaches the extractor
    # the search reads the alignments of the region its reference slice covers (ExtractVariantCandidates.py:228-240)
    view = alignment_text(args, evc.reference_region(args.ctgName, args.ctgStart if have_range else None, args.ctgEnd if have_range else None)[0])
    chunks = [finder.take_positions() for _ in _hostapi.feed_stream(finder, view.read, 1 << 22)]
    if view.finish() != 0:
        sys.exit("[ERROR] `samtools view` failed on %s" % args.bam_fn)
    if finder.reads == 0 and not quiet:
        print("No read has been process, either the genome region you specified has no read cover, or please check the correctness of your BAM input (%s)."
              % args.bam_fn, file=sys.stderr)
    return np.concatenate(chunks)


def positions_from_vcf(vcf_fn, ctg_name, ctg_start, ctg_end):
    """--vcf_fn: call only at the sites of a VCF.  The reference pipes dataPrepScripts/GetTruth.py into CreateTensor, which
    reads column 2 of its rows; this is that column, in GetTruth's order (GetTruth.py:75-134): every record of the contig inside
    the range, one row per run of equal positions (:127-133); a '*' alternate adds the base before the record -- first when
    '*' is one of the first two alternates, after it otherwise (:30-48), so the stream need not be sorted (the pileup handles that
    as the reference does)."""
    from .get_truth import expanded_records
    out = []
    for info in expanded_records(vcf_fn, ctg_name, ctg_start, ctg_end, get_base=None, with_genotype=False):
        site = int(info.position)
        if not out or out[-1] != site:
            out.append(site)
    return np.array(out, dtype=np.int64)


def tensor_batches(args, positions, batch_size, read_flank=(0, 0), progress=True):
    """Stage 2 as a generator of (X float32 [n,33,8,4], [[ctg, pos, refseq], ...]) -- what clair_amd.utils.tensor_generator_from
    yields for the text records of the same windows.  read_flank = (left, right) widens the region the ALIGNMENTS are taken from
    (not the candidates): a sub-range of a larger run needs the reads that touch only the flanks of its outermost windows."""
    from . import _hostapi
    seq, ref_start = ct.reference_sequence_from(args.samtools, args.ref_fn, args.ctgName, args.ctgStart, args.ctgEnd, native=native_input(args))
    if not seq:
        sys.exit("Failed to load reference seqeunce. Please check if the provided reference fasta %s and the ctgName %s are correct."
                 % (args.ref_fn, args.ctgName))
    have_range = args.ctgStart is not None and args.ctgEnd is not None
    if have_range:
        positions = positions[(positions >= args.ctgStart) & (positions <= args.ctgEnd)]
    builder = _hostapi.PileupBuilder(args.ctgName, seq, 0 if ref_start is None else ref_start - 1, positions,
                                     consider_left_edge=not args.stop_consider_left_edge, dcov=args.dcov, set_order=ct.set_order_of(getattr(args, "pypy", None)))
    region = "%s:%d-%d" % (args.ctgName, max(1, args.ctgStart - read_flank[0]), args.ctgEnd + read_flank[1]) if have_range else args.ctgName
    view = alignment_text(args, region)
    from .tensor_binary import _IUPAC_TABLE
    total = 0
    held = [[], [], []]                             # centres, refseq bytes [n,34], counts of windows not yet handed out
    held_n = 0

    def emit(centres, seqs, counts):
        nonlocal total
        total += len(centres)
        if progress:
            print("Processed %d tensors" % total, file=sys.stderr)
        infos = window_infos(args.ctgName, centres, seqs)
        x = _hostapi.counts_to_input(counts)              # the decode reads depth and allele support from the tensor
        # the GPU takes the raw counts (half the bytes on the host link) when they fit int16
        small = counts.astype(np.int16) if int(counts.max()) <= 32767 and int(counts.min()) >= -32768 else None
        return x, infos, small

    def drain(final):
        nonlocal held, held_n
        while builder.pending():
            centres, seqs, counts = builder.take_columns(batch_size)    # at most one batch per take: every copy below is O(batch)
            keep = _IUPAC_TABLE[seqs[:, 16]]                             # a refseq shorter than 17 has NUL there: not an IUPAC code
            if not keep.all():
                centres, seqs, counts = centres[keep], seqs[keep], counts[keep]
            for col, piece in zip(held, (centres, seqs, counts)):
                col.append(piece)
            held_n += len(centres)
            if held_n >= batch_size:
                cols = [np.concatenate(c) if len(c) > 1 else c[0] for c in held]
                held = [[c[batch_size:]] if held_n > batch_size else [] for c in cols]
                held_n -= batch_size
                yield emit(*(c[:batch_size] for c in cols))
        if final and held_n > 0:
            cols = [np.concatenate(c) if len(c) > 1 else c[0] for c in held]
            held, held_n = [[], [], []], 0
            yield emit(*cols)

    for last in _hostapi.feed_stream(builder, view.read, 1 << 22):
        for batch in drain(last):
            yield batch
    if view.finish() != 0:
        sys.exit("[ERROR] `samtools view` failed on %s" % args.bam_fn)


SLAB_BYTES = 64 << 20      # SEQ bytes per slab of packed alignments sent to the device (host packer)
TEXT_CHUNK = 64 << 20      # bytes of `samtools view` text handed to the device at a time (device parser; the page-locked buffer it is read into)
TABLE_MARGIN = 64          # positions the device tables extend beyond the region (a window reaches 17 beyond its centre)
FE_REASONS = ((1, "alignments not sorted by position"), (2, "a zero-length insertion/deletion"), (4, "an alignment spanning > 100 kb more than its bases"),
              (8, "a CIGAR longer than its SEQ"), (16, "a read base outside the IUPAC alphabet"), (32, "a reference base outside the IUPAC alphabet"),
              (64, "a count beyond int16"), (128, "the reference's budget of 5 M outstanding tuples would run out"), (256, "candidate sites not strictly ascending"),
              (512, "an alignment that begins with an insertion/deletion after another one at the same start position"))


class AlignmentStream(object):
    """The text of `samtools view <bam> ctg:a-b`, produced by K `samtools view` processes over K consecutive pieces of [a, b] at once
    (--view_readers K): BAM decoding is what the device front end waits for, and one samtools formats a few hundred MB of text per second.
    The pieces' outputs, taken in order, are the single stream's lines exactly once each, in its order, when the alignments every piece
    but the first prints that START before the piece are dropped: they overlap an earlier piece too and were printed there (sorted BAM:
    those lines are a prefix of the piece's output).  readinto() / close() like the single pipe's."""

    def __init__(self, args, ctg, first, last, readers):
        import queue
        import threading
        edges = [first + (last - first + 1) * k // readers for k in range(readers)] + [last + 1]
        self.starts = edges[:-1]
        self.procs = [ct.subprocess_popen(view_command(args, "%s:%d-%d" % (ctg, edges[k], edges[k + 1] - 1)), text=False) for k in range(readers)]
        self.queues = [queue.Queue(maxsize=16) for _ in range(readers)]          # 16 x 8 MB read ahead per piece
        self.stop = threading.Event()
        self.threads = [threading.Thread(target=self._drain, args=(k,), daemon=True) for k in range(readers)]
        for t in self.threads:
            t.start()
        self.piece, self.pending, self.dropping, self.carry = 0, b"", False, b""

    def _drain(self, k):
        import queue
        out = self.procs[k].stdout
        while not self.stop.is_set():
            chunk = out.read(1 << 23)
            while not self.stop.is_set():
                try:
                    self.queues[k].put(chunk, timeout=0.2)      # b"" = end of this piece
                    break
                except queue.Full:
                    continue
            if not chunk:
                return

    def _next_chunk(self):
        """-> bytes of the merged stream, b"" at its end"""
        while self.piece < len(self.procs):
            chunk = self.queues[self.piece].get()
            if not chunk:
                last, self.carry = self.carry, b""                   # a last line of the piece without its line end, still undecided
                keep = b""
                if last:
                    col = last.split(None, 4)
                    if not (self.piece > 0 and len(col) >= 4 and col[3].isdigit() and int(col[3]) < self.starts[self.piece]):
                        keep = last + b"\n"
                self.piece += 1
                self.dropping = True
                if keep:
                    return keep
                continue
            if self.piece > 0 and self.dropping:
                # the lines at the head of this piece that start before it: POS is the fourth column
                data, at, start = self.carry + chunk, 0, self.starts[self.piece]
                self.carry = b""
                while True:
                    nl = data.find(b"\n", at)
                    if nl < 0:
                        self.carry = data[at:]                        # no complete line yet
                        data = b""
                        break
                    col = data[at:nl].split(None, 4)
                    if len(col) >= 4 and col[0][:1] != b"@" and col[3].isdigit() and int(col[3]) < start:
                        at = nl + 1
                        continue
                    self.dropping = False
                    data = data[at:]
                    break
                if not data:
                    continue
                return data
            return chunk
        return b""

    def readinto(self, mv):
        if not self.pending:
            self.pending = self._next_chunk()
            if not self.pending:
                return 0
        n = min(len(mv), len(self.pending))
        mv[:n] = self.pending[:n]
        self.pending = self.pending[n:]
        return n

    def read(self, n):
        if not self.pending:
            self.pending = self._next_chunk()
        out, self.pending = self.pending[:n], self.pending[n:]
        return out

    def abort(self):
        """The consumer gave up: do not leave K samtools writing into full pipes."""
        self.stop.set()
        for p in self.procs:
            try:
                p.kill()
                p.stdout.close()
                p.wait()
            except OSError:
                pass

    def finish(self):
        """-> 0 when every samtools ended well"""
        self.stop.set()
        code = 0
        for p in self.procs:
            p.stdout.close()
            p.wait()
            code = code or p.returncode
        return code


class _OnePipe(object):
    def __init__(self, args, region):
        self.proc = ct.subprocess_popen(view_command(args, region), text=False)
        self.readinto, self.read = self.proc.stdout.readinto, self.proc.stdout.read

    def abort(self):
        try:
            self.proc.kill()
            self.proc.stdout.close()
            self.proc.wait()
        except OSError:
            pass

    def finish(self):
        self.proc.stdout.close()
        self.proc.wait()
        return self.proc.returncode


class _NativeBam(object):
    """--bam_reader native with the device front end: whole BAM records of `region` read into the page-locked buffer and decoded on the
    GPU (clair_frontend_add_bam), which applies the view's filter itself."""

    def __init__(self, args, region):
        self.args = args
        self.reader = native_reader(args, region)
        self.region = split_region(region)[1:]

    def feed(self, f, pack_kw, pinned):
        """pinned: nbytes -> page-locked uint8 array (DeviceFrontEnd's).  -> seconds spent in the device calls"""
        from time import time
        from . import _capi, _hostapi
        f.bam_options(self.reader.tid, region=None if self.region[0] is None else self.region, **pack_kw)
        if native_lookup(self.args):
            f.bam_lookup(True)
        if subsample_of(self.args) is not None:
            frac, seed = subsample_of(self.args)
            f.bam_subsample(seed, frac)
        buf = pinned(BAM_CHUNK + 16)
        offsets = _hostapi.bam_offsets_for(BAM_CHUNK)
        t_dev = 0.0
        while True:
            try:
                n_bytes, n_rec = self.reader.readinto(buf, offsets, cap=BAM_CHUNK)
            except _hostapi.BamError as exc:
                sys.exit("[ERROR] %s" % exc)
            if not n_rec:
                return t_dev
            t0 = time()
            try:
                f.add_bam(buf.ctypes.data, n_bytes, offsets, n_rec)
            except _capi.MalformedRecord as exc:
                why = str(exc)
                try:
                    self.reader.render(buf, offsets[exc.index:exc.index + 1], 1)
                except _hostapi.BamError as host:
                    why = str(host)
                sys.exit("[ERROR] %s: the record at BGZF virtual offset %d (compressed offset %d) is malformed: %s"
                         % (self.args.bam_fn, self.reader.voffset(exc.index), self.reader.voffset(exc.index) >> 16, why))
            t_dev += time() - t0

    def abort(self):
        self.reader.close()

    def finish(self):
        self.reader.close()
        return 0


BAM_CHUNK = 64 << 20       # bytes of whole BAM records handed to the device at a time (--bam_reader native; the page-locked buffer they are read into)


class DeviceFrontEnd(object):
    """Both pileup stages on the GPU for one contig / region.  run() -> number of windows, or None when the run has to take the host
    path (reason logged); batches() then yields what tensor_batches yields, with the counts as clair_amd._capi.DeviceWindows."""

    def __init__(self, args, device, pinned=None, candidate_step=None, window_kw=None):
        """pinned: nbytes -> page-locked uint8 array (Clair.pinned_buffer): the text is then read straight into it and parsed on the
        device; without it (or with CLAIR_AMD_FE_PACK=host) the host packer (clair_host_sampack_*) makes the slabs.
        candidate_step(frontend, bed intervals or None) -> number of candidates: fixes the candidate list in place of find_candidates
        (clair_amd.make_train_set samples it); window_kw: build_windows' drop rules where they are not the caller's (the same module)."""
        self.args, self.device, self.pinned = args, device, pinned
        self.candidate_step = candidate_step
        self.window_kw = dict(min_coverage=0, drop_non_iupac_centre=True) if window_kw is None else window_kw
        self.frontend = None
        self.n_windows = 0

    def close(self):
        if self.frontend is not None:
            self.frontend.close()
            self.frontend = None

    def _fallback(self, why):
        """The input is outside the regime the device formulation reproduces bit for bit (never: the device or the library is missing --
        that is an error).  --front_end device makes it an error too."""
        self.close()
        if self.args.front_end == "device":
            sys.exit("[ERROR] --front_end device: %s; the sequential host stages (--front_end host) reproduce the reference there" % why)
        logging.info("device front end not used (%s): running the candidate search and the pileup on the host" % why)
        return None

    def run(self):
        """-> number of windows, or None after a logged hand-back to the host stages.  Errors of the device library (out of memory, a lost
        device) end the run like the engine's do: a message and a non-zero exit."""
        from . import _capi
        try:
            return self._run()
        except _capi.MalformedText:
            raise
        except _capi.EngineError as exc:
            if "out of memory" in str(exc).lower():       # tables for the whole region + the resident text: too much for what is free on this GPU
                return self._fallback("not enough device memory for the region: %s" % exc)
            sys.exit("[ERROR] %s" % exc)

    def tables(self, search=True):
        """What a front end of this region is created over, and the region its alignments are read from -> (reference slice, its 0-based
        start, bed intervals or None, table span lo, hi, samtools' region).  search: candidates are searched for (the .fai and the bed file
        are then looked at, as the search looks at them)."""
        args = self.args
        have_range = args.ctgStart is not None and args.ctgEnd is not None
        seq, ref0, bed = reference_and_bed(args, search, "Failed to load reference seqeunce. Please check if the provided reference fasta %s "
                                           "and the ctgName %s are correct." % (args.ref_fn, args.ctgName))
        if have_range:
            lo, hi = args.ctgStart - 1 - TABLE_MARGIN, args.ctgEnd + TABLE_MARGIN
            # the candidate search reads the widened region, the pileup the plain one (callVarBam.py:124-199); an alignment can only
            # matter to a position of [ctgStart, ctgEnd] if it reaches within one base of it -- the packer marks which of the two
            # stages would have been given it
            region = "%s:%d-%d" % (args.ctgName, max(1, args.ctgStart - 2), args.ctgEnd + 2)
        else:
            lo, hi = ref0 - TABLE_MARGIN, ref0 + len(seq) + TABLE_MARGIN
            region = args.ctgName
        self.table_info = dict(seq=seq, ref0=ref0, bed=bed, lo=lo, hi=hi)
        return seq, ref0, bed, lo, hi, region

    def feed(self, f, region):
        """The alignments of `region` into f -- a clair_amd._capi.Frontend, or (without a page-locked buffer: through the host packer)
        anything with its add_slab(packer), which clair_amd.gvcf's host backend uses -> (the packer's statistics, start time, seconds
        packing on the host, seconds in the device calls)."""
        from . import _capi, _hostapi
        args = self.args
        have_range = args.ctgStart is not None and args.ctgEnd is not None
        pack_kw = dict(dcov=args.dcov, evc_min_mq=0, pile_min_mq=0, pile_region=(args.ctgStart, args.ctgEnd) if have_range else None)
        readers = max(1, int(getattr(args, "view_readers", 1) or 1))
        span = (max(1, args.ctgStart - 2), args.ctgEnd + 2) if have_range else (1, contig_length(args.ref_fn, args.ctgName) or 0)
        on_device = self.pinned is not None and os.environ.get("CLAIR_AMD_FE_PACK", "device") != "host"
        if native_input(args):
            # no samtools: the records themselves go to the GPU (or, for the host packer, the text they render to)
            view = _NativeBam(args, region) if on_device else _NativeText(args, region)
        elif readers > 1 and span[1] - span[0] + 1 >= 2 * readers:
            view = AlignmentStream(args, args.ctgName, span[0], span[1], readers)
        else:
            view = _OnePipe(args, region)
        from time import time
        t_start, t_pack, t_dev = time(), 0.0, 0.0
        try:
            if on_device and isinstance(view, _NativeBam):
                t_dev = view.feed(f, pack_kw, self.pinned)
                pst = f.text_stats()
            elif on_device:
                # the text goes to the GPU as it comes out of the pipe (read into a page-locked buffer, whole lines at a time) and is
                # parsed there: the host touches no byte of it but the last megabyte of each chunk, looking for the line end
                f.text_options(args.ctgName, **pack_kw)
                buf = self.pinned(TEXT_CHUNK + 16)
                mv = memoryview(buf)
                fill, eof = 0, False
                while not eof:
                    while fill < TEXT_CHUNK:
                        n = view.readinto(mv[fill:TEXT_CHUNK])
                        if not n:
                            eof = True
                            break
                        fill += n
                    cut = fill
                    if not eof:
                        cut, span = -1, 1 << 20
                        while cut < 0:
                            lo_ = max(0, fill - span)
                            k = bytes(mv[lo_:fill]).rfind(b"\n")
                            cut = lo_ + k + 1 if k >= 0 else -1
                            if lo_ == 0:
                                break
                            span *= 4
                        if cut <= 0:
                            sys.exit("[ERROR] an alignment line longer than %d bytes" % TEXT_CHUNK)
                    elif fill and buf[fill - 1] != 10:             # the stream ended without a line end
                        buf[fill] = 10
                        fill = cut = fill + 1
                    if cut:
                        t0 = time()
                        try:
                            f.add_text(buf.ctypes.data, cut)
                        except _capi.MalformedText:
                            _hostapi.SamPacker(args.ctgName, **pack_kw).feed(bytes(mv[:cut]), final=True)     # raises with the line and the column
                            raise
                        t_dev += time() - t0
                    buf[:fill - cut] = buf[cut:fill]
                    fill -= cut
                pst = f.text_stats()
            else:
                packer = _hostapi.SamPacker(args.ctgName, lookup=native_lookup(args) and native_input(args), **pack_kw)

                def read(n):                                   # packing time is the feed loop's less what it waits for here
                    nonlocal t_pack
                    t0 = time()
                    chunk = view.read(n)
                    t_pack -= time() - t0
                    return chunk
                t0 = time()
                for last in _hostapi.feed_stream(packer, read, 1 << 23):
                    t_pack += time() - t0
                    if last or packer.stats()["seq_bytes"] >= SLAB_BYTES:
                        t0 = time()
                        f.add_slab(packer)
                        t_dev += time() - t0
                    t0 = time()
                pst = packer.stats()
        except BaseException:
            view.abort()
            raise
        if view.finish() != 0:
            sys.exit("[ERROR] `samtools view` failed on %s" % args.bam_fn)
        self.view_kind = ("packing the text on the host %.2f s" % t_pack if t_pack else
                          ("BAM records decoded on the device" if isinstance(view, _NativeBam) else "text parsed on the device"))
        return pst, t_start, t_pack, t_dev

    def _run(self):
        from time import time
        from . import _capi
        args = self.args
        have_range = args.ctgStart is not None and args.ctgEnd is not None
        given = None
        if args.vcf_fn is not None:
            given = positions_from_vcf(args.vcf_fn, args.ctgName, args.ctgStart, args.ctgEnd)
            if have_range:
                given = given[(given >= args.ctgStart) & (given <= args.ctgEnd)]
            if len(given) > 1 and not (np.diff(given) > 0).all():
                return self._fallback(FE_REASONS[8][1])
        seq, ref0, bed, lo, hi, region = self.tables(given is None)
        f = self.frontend = _capi.Frontend(self.device, seq, ref0, lo, hi)
        pst, t_start, t_pack, t_dev = self.feed(f, region)
        t0 = time()
        if given is None:
            if pst["evc_reads"] == 0:
                print("No read has been process, either the genome region you specified has no read cover, or please check the correctness of your BAM input (%s)."
                      % args.bam_fn, file=sys.stderr)
            if self.candidate_step is not None:
                n_cand = self.candidate_step(f, bed)
            else:
                n_cand = f.find_candidates(min_coverage=int(args.minCoverage), threshold=args.threshold,     # callVarBam.py:75: int() before it reaches the extractor
                                           ctg_start=args.ctgStart if have_range else None, ctg_end=args.ctgEnd if have_range else None, bed=bed)
        else:
            f.set_candidates(given)
            n_cand = len(given)
        n = f.build_windows(consider_left_edge=not args.stop_consider_left_edge, **self.window_kw)
        bits = pst["anomalies"] | f.stats()["anomalies"]
        if not bits and f.budget_binds():
            bits = 128
        if bits:
            return self._fallback("; ".join(why for bit, why in FE_REASONS if bits & bit))
        t_dev += time() - t0
        logging.info("%d candidate sites" % n_cand)
        logging.info("device front end: %d alignments, %d windows in %.2f s (%s, device %.2f s, the rest waiting for %s)"
                     % (f.stats()["reads"], n, time() - t_start, self.view_kind, t_dev,
                        "the BAM reader" if native_input(args) else "`samtools view`"))
        self.n_windows = n
        return n

    def batches(self, batch_size, lean=True, progress=True):
        """(X float32 or None, infos, counts) per batch.  lean: nobody on the host reads the tensor (decode on the device, no BAM open):
        the counts stay in HBM (DeviceWindows) and X is None; otherwise both come back to the host, as from tensor_batches."""
        from . import _capi, _hostapi
        f = self.frontend
        total = 0
        for first in range(0, self.n_windows, batch_size):
            n = min(batch_size, self.n_windows - first)
            centres, seqs = f.window_info(first, n)
            total += n
            if progress:
                print("Processed %d tensors" % total, file=sys.stderr)
            infos = window_infos(self.args.ctgName, centres, seqs)
            if lean:
                yield None, infos, _capi.DeviceWindows(f, first, n)
            else:
                counts = f.window_counts(first, n)
                yield _hostapi.counts_to_input(counts.astype(np.int32)), infos, counts


WINDOW_FLANK = 33          # reads that touch only the flank of a sub-range's outermost windows (16 positions) must still be seen
MIN_SPAN_PER_WORKER = 50000


def contig_length(ref_fn, ctg_name):
    with open(ref_fn + ".fai") as f:
        for row in f:
            col = row.split("\t")
            if col[0] == ctg_name:
                return int(col[1])
    return None


def front_end_workers(args):
    """How many sub-ranges the two host stages are split into (--front_end_workers; default: by the CPUs this process may use)."""
    if args.vcf_fn is not None:
        return 1, None, None
    have_range = args.ctgStart is not None and args.ctgEnd is not None
    lo, hi = (args.ctgStart, args.ctgEnd) if have_range else (1, contig_length(args.ref_fn, args.ctgName) if os.path.isfile(args.ref_fn + ".fai") else None)
    if hi is None:
        return 1, None, None
    want = args.front_end_workers
    if want is None or want == 1:
        return 1, None, None        # the default is the single pass: see --front_end_workers for when the split run can differ from it
    if want <= 0:                   # 0 = by the CPUs this process may use
        want = max(1, min(8, ingest_cpus() // 2))
    want = max(1, min(want, (hi - lo + 1) // MIN_SPAN_PER_WORKER))
    return want, lo, hi


def ingest_cpus():
    """CPUs this process may use: affinity mask, capped by a cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def parallel_front_end(args, batch_size, workers, lo, hi):
    """Both host stages (candidate search, pileup windows) over `workers` consecutive sub-ranges of [lo, hi] at once, each on its
    own thread with its own `samtools view` streams (the native cores release the GIL) -- the reference's process-per-chunk
    fan-out (clair/callVarBamParallel.py:90-119) inside one process feeding one GPU.  Batches come out in position order: a
    sub-range's batches are consumed when every earlier sub-range is done (bounded queues hold the others back).  Candidates
    and windows are those of the unsplit run (a sub-range takes its alignments from WINDOW_FLANK positions beyond its INNER ends) as
    long as CreateTensor's tuple budget does not run out: each sub-range has its own, like each chunk of callVarBamParallel."""
    import copy
    import queue
    import threading
    edges = [lo + (hi - lo + 1) * k // workers for k in range(workers)] + [hi + 1]
    queues = [queue.Queue(maxsize=6) for _ in range(workers)]
    counts = [0] * workers
    stop = threading.Event()

    def put(q, item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                continue
        return False

    def work(k):
        sub = copy.copy(args)
        sub.ctgStart, sub.ctgEnd = edges[k], edges[k + 1] - 1
        try:
            positions = candidate_positions(sub, quiet=True)
            counts[k] = len(positions)
            # the run's own outer ends keep the reference's region semantics (alignments of exactly ctgStart-ctgEnd, CreateTensor.py);
            # on a whole contig they are the contig's ends
            flank = (WINDOW_FLANK if k > 0 else 0, WINDOW_FLANK if k + 1 < workers else 0)
            for batch in tensor_batches(sub, positions, batch_size, read_flank=flank, progress=False):
                if not put(queues[k], batch):
                    return
            put(queues[k], None)
        except BaseException:                       # sys.exit of a failing samtools included: handed to the consumer
            put(queues[k], sys.exc_info())

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(workers)]
    for t in threads:
        t.start()
    total = 0
    try:
        for k in range(workers):
            while True:
                item = queues[k].get()
                if item is None:
                    break
                if isinstance(item, tuple) and len(item) == 3 and isinstance(item[1], BaseException):
                    raise item[1].with_traceback(item[2])
                total += len(item[1])
                print("Processed %d tensors" % total, file=sys.stderr)
                yield item
        logging.info("%d candidate sites" % sum(counts))
    finally:
        stop.set()


def normalise(args):
    """The argument checks of callVarBam.py:62-101."""
    if args.ctgName is None:
        sys.exit("--ctgName must be specified. You can call variants on multiple chromosomes simultaneously.")
    for path, suffix in ((args.bam_fn, ""), (args.ref_fn, "")):
        if not os.path.isfile(path + suffix):
            sys.exit("[ERROR] file %s not found" % (path + suffix))
    if args.ctgStart is not None and args.ctgEnd is not None and int(args.ctgStart) > int(args.ctgEnd):
        args.ctgStart = args.ctgEnd = None          # callVarBam.py:97-101
    if (args.ctgStart is None) != (args.ctgEnd is None):
        args.ctgStart = args.ctgEnd = None
    if getattr(args, "bam_inflate", "host") == "device" and not native_input(args):
        sys.exit("[ERROR] --bam_inflate device inflates the BGZF blocks the native reader reads: add --bam_reader native")
    if native_input(args):
        for name, given in (("--samtools_view_args", args.samtools_view_args is not None), ("--samtools_threads", (args.samtools_threads or 0) > 0),
                            ("--view_readers", (args.view_readers or 1) > 1)):
            if given:
                sys.exit("[ERROR] %s configures `samtools view`, which --bam_reader native does not run: drop one of the two" % name)
        if not 1 <= args.bam_threads <= 16:
            sys.exit("[ERROR] --bam_threads %d: 1 .. 16" % args.bam_threads)
    cv.check_ensemble_flags(args)
    cv.check_overlap_flags(args)
    check_subsample_flags(args)
    check_site_flags(args)
    check_gvcf_flags(args)
    if native_lookup(args):
        if not native_input(args):
            sys.exit("[ERROR] --indel_lookup native answers from the alignments the native reader feeds the device front end: add --bam_reader native")
        if not wants_device_front_end(args):
            sys.exit("[ERROR] --indel_lookup native answers from the alignments resident on the GPU: it needs the device front end "
                     "(drop --front_end host / --front_end_workers)")
    return args


def check_gvcf_flags(args):
    """--gvcf_fn: what it cannot go with (docs/gvcf.md, "out of scope"), and its two options checked before the model is loaded."""
    if not getattr(args, "gvcf_fn", None):
        return
    for flag, given in (("--vcf_fn", args.vcf_fn is not None), ("--ensemble_bam_fn", bool(getattr(args, "ensemble_bam_fn", None))),
                        ("--ensemble_subsample", bool(getattr(args, "ensemble_subsample", None))), ("--output_for_ensemble", args.output_for_ensemble)):
        if given:
            sys.exit("[ERROR] --gvcf_fn tiles the region between the calls of one BAM's own candidate search with reference-confidence blocks; "
                     "with %s there is no such call set: drop one of the two" % flag)
    if args.call_fn is None:
        sys.exit("[ERROR] --gvcf_fn adds blocks to the rows of --call_fn: give --call_fn as well")
    from . import gvcf
    gvcf.check_options(args)


MAX_ENSEMBLE_BAMS = 7      # --ensemble_bam_fn: CLAIR_SITES_MAX_BAMS less --bam_fn


def site_sources(args):
    """The BAMs call_sites reads after --bam_fn, in order: the --ensemble_bam_fn files whole, then --bam_fn again at every --ensemble_subsample
    (normalised: (fraction, seed)) -> [(path, None or (fraction, seed)), ...]; empty for a run that is no ensemble across BAMs."""
    return ([(path, None) for path in getattr(args, "ensemble_bam_fn", None) or []]
            + [(args.bam_fn, virtual) for virtual in getattr(args, "ensemble_subsample", None) or []])


def check_site_flags(args):
    """--ensemble_bam_fn / --ensemble_subsample replace the text chain over several BAMs; what only makes sense with them, and what cannot go
    with them."""
    more = getattr(args, "ensemble_bam_fn", None) or []
    n_more = len(site_sources(args))
    if not n_more:
        if getattr(args, "minimum_count_to_output", 0):
            sys.exit("[ERROR] --minimum_count_to_output counts the (BAM, checkpoint) runs of a site across --ensemble_bam_fn BAMs: give --ensemble_bam_fn "
                     "(or --ensemble_subsample) as well")
        return
    if n_more > MAX_ENSEMBLE_BAMS:
        sys.exit("[ERROR] --ensemble_bam_fn and --ensemble_subsample: %d BAMs, at most %d" % (n_more, MAX_ENSEMBLE_BAMS))
    if args.output_for_ensemble:
        sys.exit("[ERROR] --ensemble_bam_fn merges and averages the BAMs' sites in this process; --output_for_ensemble writes one run's "
                 "probabilities for the `ensemble` submodule to average: use one of the two")
    if args.minimum_count_to_output < 0:
        sys.exit("[ERROR] --minimum_count_to_output %d: 0 or more" % args.minimum_count_to_output)
    if getattr(args, "overlap_filter", "off") != "off" and args.ensemble_order != "position":
        sys.exit("[ERROR] --overlap_filter walks rows sorted by position; --ensemble_bam_fn writes them in the text chain's order unless "
                 "--ensemble_order position is given: add it")
    if (args.front_end_workers or 1) != 1:
        sys.exit("[ERROR] --ensemble_bam_fn runs every BAM through the device front end or the single-pass host stages: drop --front_end_workers")
    for path in more:
        if not os.path.isfile(path):
            sys.exit("[ERROR] file %s not found" % path)


def load_model(args):
    from .model import Clair
    batch = args.batch_size or param.engineBatchSize
    try:
        m = Clair(device=args.device, max_batch=batch, n_slots=param.pipeline_slots())
        m.init()
        cv.restore_checkpoints(m, args)
    except Exception as exc:
        sys.exit("[ERROR] %s" % exc)
    return m


def wants_device_front_end(args):
    return args.front_end != "host" and front_end_workers(args)[0] == 1


def call_region(args, m, prepared=None):
    """One contig / region through an engine that is already up: front end, network, decode, VCF.  prepared: a DeviceFrontEnd whose run()
    has been called (clair_amd.callVarBamParallel --run reads the next regions' alignments while this one is called); it is closed here."""
    config = cv.OutputConfig(
        is_show_reference=False, is_debug=args.debug,
        is_haploid_precision_mode_enabled=args.haploid_precision,
        is_haploid_sensitive_mode_enabled=args.haploid_sensitive,
        is_output_for_ensemble=args.output_for_ensemble, quality_score_for_pass=args.qual)
    device_fe = prepared
    if native_lookup(args):
        # the tables come from the front end's slabs, which exist once it has run: the look-up asks for them through this handle
        def tables(positions, capacity):
            return device_fe.frontend.indel_table(positions, capacity)
        lookup = cv.IndelTableLookup(tables, args.ref_fn)
    else:
        lookup = cv.AlignmentLookup(args.bam_fn, args.ref_fn)
    decoder = cv.VariantDecoder(config, lookup, always_use_bam=args.pysam_for_all_indel_bases, arith=args.arith)
    writer = cv.writer_for(args)
    if site_sources(args):
        def first_front_end(fe):            # BAM 0's front end is this function's to close, like the single BAM's: the native look-up asks it
            nonlocal device_fe
            device_fe = fe
        try:
            call_sites(args, m, decoder, lookup, writer, prepared, first_front_end)
            if native_lookup(args):
                logging.info("indel look-up: %d positions in %d device calls (at most %d in one), lookup_over_depth %d, answered by the host twin %d"
                             % (lookup.positions, lookup.calls, lookup.largest_call, lookup.over_depth, lookup.handed_over))
        finally:
            if device_fe is not None:
                device_fe.close()
            writer.close()
            lookup.close()
        return
    try:
        batch = args.batch_size or param.engineBatchSize
        source = None
        workers, lo, hi = front_end_workers(args)
        if wants_device_front_end(args):
            # nobody on the host reads the tensors when the decode runs on the device and no BAM is consulted (cv.call_variants)
            lean = decoder.native_applies() and lookup.sam is None and os.environ.get("CLAIR_AMD_DEVICE_DECODE", "1") != "0"
            if device_fe is None:
                device_fe = DeviceFrontEnd(args, args.device, pinned=getattr(m, "pinned_buffer", None))
                device_fe.run()
            if device_fe.frontend is not None:
                def source(batch):
                    return device_fe.batches(batch, lean=lean)
        if source is None and workers > 1:
            def source(batch):
                return parallel_front_end(args, batch, workers, lo, hi)
        elif source is None:
            positions = candidate_positions(args)
            logging.info("%d candidate sites" % len(positions))

            def source(batch):
                return tensor_batches(args, positions, batch)
        if native_lookup(args) and (device_fe is None or device_fe.frontend is None):
            sys.exit("[ERROR] --indel_lookup native: the device front end handed this region to the host stages (see the message above), so no "
                     "alignments are resident on the GPU to look indels up in; --indel_lookup pysam works with every front end")
        cv.call_variants(args, m, decoder, writer, batch, generator=source(batch))
        if native_lookup(args):
            logging.info("indel look-up: %d positions in %d device calls (at most %d in one), lookup_over_depth %d, answered by the host twin %d"
                         % (lookup.positions, lookup.calls, lookup.largest_call, lookup.over_depth, lookup.handed_over))
        if getattr(args, "gvcf_fn", None):
            # the call VCF is finished first (the overlap filter included): its rows are what the blocks leave out.  The front end is still
            # alive, so the tallies of the region are in HBM and the BAM is not read again (docs/gvcf.md)
            from . import gvcf
            writer.close()
            gvcf.after_calls(args, device_fe)
    finally:
        if device_fe is not None:
            device_fe.close()
        writer.close()
        lookup.close()


def call_sites(args, m, decoder, lookup, writer, prepared=None, first_front_end=None):
    """--ensemble_bam_fn / --ensemble_subsample: one region from B BAMs (files, or --bam_fn at a fraction of its reads: docs/subsample.md)
    with the K checkpoints of the model, merged per site and averaged on the GPU (the site table,
    include/clair_amd.h: clair_sites_*; docs/ensemble.md).  Per BAM: the front end (on the device, or the host stages where it hands the
    region back), the table told of all the BAM's window positions at once, then the batches through submit_sites, as many in flight as the
    model has slots.  Then the table is finished and its output list decoded batch by batch into the existing decoder and writer.
    first_front_end(fe): told of BAM 0's device front end, which the caller closes after the last row is decoded (the native indel look-up
    asks it until then); every other BAM's is closed here when its windows have been consumed."""
    import copy
    from time import time
    from . import _capi, _hostapi
    t0 = time()
    batch = args.batch_size or param.engineBatchSize
    n_slots = max(1, int(getattr(m, "n_slots", 2)))
    # --bam_fn (at --subsample if given), the --ensemble_bam_fn files whole, then the virtual BAMs: --bam_fn at each --ensemble_subsample
    bams = [(args.bam_fn, subsample_of(args))] + site_sources(args)
    table = m.site_table()
    buffers = {}

    def pinned(nbytes):                            # one page-locked feed buffer for all the BAMs: a front end reads it only while it is fed
        if nbytes not in buffers:
            buffers[nbytes] = m.pinned_buffer(nbytes)
        return buffers[nbytes]
    try:
        for b, (bam, virtual) in enumerate(bams):
            sub = copy.copy(args)
            sub.bam_fn = bam
            sub.subsample, sub.subsample_seed = virtual if virtual is not None else (None, 0)
            if virtual is not None:
                bam = "%s at %g (seed %d)" % ((bam,) + virtual)
            if b > 0:
                sub.indel_lookup = "pysam"         # only BAM 0 is ever asked: the other front ends keep nothing for the look-up
            fe = None
            try:
                if wants_device_front_end(sub):
                    if b == 0 and prepared is not None:
                        fe = prepared
                    else:
                        fe = DeviceFrontEnd(sub, args.device, pinned=pinned if hasattr(m, "pinned_buffer") else None)
                        if b == 0 and first_front_end is not None:
                            first_front_end(fe)
                        fe.run()
                    if fe.frontend is None:
                        fe = None
                if b == 0 and native_lookup(args) and fe is None:
                    sys.exit("[ERROR] --indel_lookup native: the device front end handed this region to the host stages (see the message above), so no "
                             "alignments are resident on the GPU to look indels up in; --indel_lookup pysam works with every front end")
                if fe is not None:
                    f, n_windows = fe.frontend, fe.n_windows
                    centres, seqs = f.window_info(0, n_windows) if n_windows else (np.zeros(0, np.int64), np.zeros((0, 34), np.uint8))

                    def pieces():
                        for first in range(0, n_windows, batch):
                            n = min(batch, n_windows - first)
                            q = seqs[first:first + n]
                            yield first, _capi.DeviceWindows(f, first, n), True, np.stack([q[:, 16], np.minimum((q[:, :33] != 0).sum(axis=1), 255)], axis=1).astype(np.uint8), q
                else:
                    positions = candidate_positions(sub)
                    logging.info("%d candidate sites" % len(positions))
                    # the table wants every position of the BAM before its first batch: the batches are held, as int16 counts where they fit
                    held = [(infos, small if small is not None else x, small is not None) for x, infos, small in tensor_batches(sub, positions, batch)]
                    centres = np.array([int(info[1]) for infos, _, _ in held for info in infos], dtype=np.int64)

                    def pieces():
                        first = 0
                        for infos, windows, is_counts in held:
                            yield first, windows, is_counts, _hostapi.centre_bytes(infos), [info[2] for info in infos]
                            first += len(infos)
                n_new = table.begin_source(centres)
                logging.info("%s: %d windows, %d sites the earlier BAMs did not have" % (bam, len(centres), n_new))
                inflight = []
                try:
                    for k, (first, windows, is_counts, centre, seq) in enumerate(pieces()):
                        if len(inflight) == n_slots:
                            m.wait(inflight.pop(0))
                        m.submit_sites(k % n_slots, table, first, windows, centre, seq, counts=is_counts)
                        inflight.append(k % n_slots)
                finally:
                    failed = sys.exc_info()[0] is not None
                    for slot in inflight:
                        try:
                            m.wait(slot)
                        except Exception:
                            if not failed:
                                raise
            finally:
                if fe is not None and b > 0:
                    fe.close()
        n_out = table.finish(args.minimum_count_to_output, args.ensemble_order)
        logging.info("%d sites of %d BAMs x %d checkpoints to call" % (n_out, len(bams), getattr(m, "n_models", 1)))
        writer.write_header()
        logging.info("Calling variants ...")
        device_decode = decoder.native_applies() and os.environ.get("CLAIR_AMD_DEVICE_DECODE", "1") != "0"
        keep_probabilities = device_decode and lookup.sam is not None      # candidates that consult the BAM are decoded again from them
        inflight = []

        def retire():
            slot, first, n = inflight.pop(0)
            prediction = m.wait(slot)
            positions, _, seqs = table.info(first, n)
            infos = window_infos(args.ctgName, positions, seqs)
            if device_decode:
                calls, probabilities = prediction if keep_probabilities else (prediction, None)
                x = table.windows(first, n) if keep_probabilities else None
                writer.write_rows(decoder.decode_calls(x, infos, calls, probabilities))
            else:
                writer.write_rows(decoder.decode_batch(table.windows(first, n), infos, prediction))

        for k, first in enumerate(range(0, n_out, batch)):
            if len(inflight) == n_slots:
                retire()
            n = min(batch, n_out - first)
            m.submit_site_calls(k % n_slots, table, first, n, with_calls=device_decode, with_probabilities=keep_probabilities)
            inflight.append((k % n_slots, first, n))
        while inflight:
            retire()
        logging.info("Total time elapsed: %.2f s" % (time() - t0))
    finally:
        table.close()


def Run(args):
    normalise(args)
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    cv.ingest.setup_environment()
    if args.activation_only:
        cv.writer_for(args).close()
        return
    m = load_model(args)
    try:
        call_region(args, m)
    finally:
        m.close()


def build_parser():
    """Flag names and defaults of clair/callVarBam.py:237-322 (help texts are this build's), plus --batch_size / --device / --arith."""
    parser = ArgumentParser(description="BAM to VCF for one contig or region, in one process on one GPU")
    add = parser.add_argument
    add('--chkpnt_fn', type=str, default=None, help="model checkpoint prefix (.npz container or TensorFlow bundle)")
    add('--ref_fn', type=str, default="ref.fa", help="reference FASTA with its .fai")
    add('--bed_fn', type=str, default=None, help="restrict candidates to these intervals (intersected with the region)")
    add('--bam_fn', type=str, default="bam.bam", help="sorted alignments")
    add('--call_fn', type=str, default=None, help="output VCF")
    add('--vcf_fn', type=str, default=None, help="call only at the sites of this VCF instead of extracting candidates")
    add('--threshold', type=float, default=0.125, help="minimum allele frequency of a candidate site, default: %(default)s")
    add('--minCoverage', type=float, default=4, help="minimum depth of a candidate site, default: %(default)s")
    add('--qual', type=int, default=None, help="PASS / LowQual cut-off, optional")
    add('--sampleName', type=str, default="SAMPLE", help="sample column of the VCF")
    add('--ctgName', type=str, default=None, help="contig to process (required)")
    add('--ctgStart', type=int, default=None, help="1-based first position of the region")
    add('--ctgEnd', type=int, default=None, help="1-based last position of the region (inclusive)")
    add('--stop_consider_left_edge', action='store_true', help="open a window only for reads that cover its left edge")
    add('--dcov', type=int, default=250, help="at most this many reads per start position, default: %(default)s")
    add('--samtools', type=str, default="samtools", help="samtools executable")
    add('--pypy', type=str, default="pypy3", help="no stage of this pipeline runs under pypy; the name only selects whose set order the pileup follows where the reference's tuple budget binds (pypy*: insertion order, anything else: CPython's)")
    add('--threads', type=int, default=None, help="host threads, optional")
    add('--delay', type=int, default=10, help="ignored: there is no TensorFlow start-up thread storm to stagger")
    add('--debug', action='store_true', help="debug lines in the VCF body")
    add('--pysam_for_all_indel_bases', action='store_true', help="look every indel up in the BAM (needs pysam, or --indel_lookup native)")
    add('--haploid_precision', action='store_true', help="haploid calling: homozygous variants only")
    add('--haploid_sensitive', action='store_true', help="haploid calling: everything but multi-allelic variants")
    add('--activation_only', action='store_true', help="kept for flag compatibility (plotting is a dead path)")
    add('--max_plot', type=int, default=10, help="kept for flag compatibility")
    add('--log_path', type=str, nargs='?', default=None, help="kept for flag compatibility")
    add('-p', '--parallel_level', type=int, default=2, help="kept for flag compatibility")
    add('--fast_plotting', action='store_true', help="kept for flag compatibility")
    add('-w', '--workers', type=int, default=8, help="kept for flag compatibility")
    add('--output_for_ensemble', action='store_true', help="write probabilities for ensembling instead of a VCF")
    # additions of this implementation
    add('--batch_size', type=int, default=None, help="candidates per forward pass, default: %d" % param.engineBatchSize)
    add('--front_end_workers', type=int, default=None,
        help="run the candidate search and the pileup over this many consecutive sub-ranges at once (threads, one pair of samtools streams each; "
             "0 = half the usable CPUs, at most 8; at least 50 kb per sub-range).  Default 1: the single pass.  The split run yields the single "
             "pass's candidates and windows EXCEPT where CreateTensor's 5 M-tuple budget runs out (candidates every few bases at high depth): every "
             "sub-range has its own budget, as every chunk of callVarBamParallel has")
    add('--front_end', type=str, default="auto", choices=("auto", "device", "host"),
        help="where the candidate search and the pileup run: on the GPU (one pass over the alignments; auto = device, falling back to the host "
             "stages, with a message, where the device formulation does not reproduce the reference exactly) or on the host (two passes, the "
             "sequential code).  --front_end_workers > 1 implies host")
    add('--view_readers', type=int, default=1,
        help="with the front end on the device: read the alignments with this many `samtools view` processes at once, each over a consecutive piece "
             "of the region (same lines, same order as one)")
    add('--samtools_view_args', type=str, default=None,
        help="extra options for `samtools view`, e.g. \"--keep-tag NM\": nothing beyond SEQ is read from a line, and the tags of an ONT BAM (move "
             "tables) can be several times the size of the rest.  Write a value that is itself one option with `=`: --samtools_view_args=-x")
    add('--samtools_threads', type=int, default=0,
        help="extra decompression threads for `samtools view` (its -@): with the front end on the device the BAM decoder is what the run waits for")
    add('--bam_reader', type=str, default="samtools", choices=("samtools", "native"),
        help="how the alignments and the reference slice are read: `samtools view` / `samtools faidx` (default), or natively without samtools "
             "(BGZF BAM with a .bai or none; the records are decoded on the GPU with the device front end).  CRAM, .csi indexes and extra view "
             "options need samtools")
    add('--bam_threads', type=int, default=4, help="with --bam_reader native: threads that inflate BGZF blocks (1 .. 16), default: %(default)s")
    add('--bam_inflate', type=str, default="host", choices=("host", "device"),
        help="with --bam_reader native: where BGZF blocks are inflated: zlib on --bam_threads host threads (default), or on the GPU --device names, "
             "a wave per block (--bam_threads is then ignored)")
    add('--indel_lookup', type=str, default="pysam", choices=("pysam", "native"),
        help="who answers the decode's questions to the BAM (indels of 16 bases or more, the second allele of Ins/Ins calls, every indel with "
             "--pysam_for_all_indel_bases): pysam (default; every answer is empty where pysam is not installed), or native: the alignments the device "
             "front end keeps on the GPU (needs --bam_reader native; docs/indel_lookup.md)")
    add('--device', type=int, default=0, help="HIP device ordinal, default: %(default)s")
    add('--ensemble_chkpnt_fn', type=str, action='append', default=None, metavar="PREFIX",
        help="one more checkpoint to call with, repeatable (at most 7): the probabilities of --chkpnt_fn and of these are averaged on the GPU "
             "exactly as the reference's call_var --output_for_ensemble | ensemble | call_var --input_probabilities averages them")
    add('--ensemble_bam_fn', type=str, action='append', default=None, metavar="BAM",
        help="one more BAM of the same sample and region (e.g. a down-sampled one), repeatable (at most %d): every BAM is called with every "
             "checkpoint, the sites are merged and their probabilities averaged on the GPU exactly as `cat` of the runs' --output_for_ensemble "
             "rows | ensemble | call_var --input_probabilities does.  --bam_fn is BAM 0: window and reference of a site are those of the first "
             "BAM that has it, and the decode's questions to a BAM (pysam, --indel_lookup native) go to --bam_fn" % MAX_ENSEMBLE_BAMS)
    add('--subsample', type=float, default=None, metavar="FRAC",
        help="read --bam_fn at this fraction of its reads (0 < FRAC <= 1), chosen by read name as `samtools view -s` chooses them, in the native "
             "reader's view on the GPU: no down-sampled copy on disk (needs --bam_reader native and --indel_lookup native; docs/subsample.md)")
    add('--subsample_seed', type=int, default=0, metavar="INT",
        help="the 32-bit word the read name's hash is XORed with (0 .. 4294967295), default: %(default)s; with 0 the subset is the one "
             "`samtools view -s 0.FRAC` keeps, a non-zero seed is not scrambled as samtools scrambles it")
    add('--ensemble_subsample', type=str, action='append', default=None, metavar="FRAC[:SEED]",
        help="one more virtual BAM, repeatable: --bam_fn at this fraction (SEED: --subsample_seed unless given), called and averaged like an "
             "--ensemble_bam_fn file, after those; --bam_fn and all of both kinds: at most %d (needs --bam_reader native)" % (MAX_ENSEMBLE_BAMS + 1))
    add('--minimum_count_to_output', type=int, default=0,
        help="with --ensemble_bam_fn: call a site only when at least this many (BAM, checkpoint) runs produced it (the `ensemble` filter's "
             "option of the same name), default: %(default)s")
    add('--ensemble_order', type=str, default="chain", choices=("chain", "position"),
        help="with --ensemble_bam_fn: rows in the order the text chain yields (all sites of --bam_fn ascending, then those only later BAMs "
             "have, BAM by BAM), or sorted by position; default: %(default)s")
    add('--arith', type=str, default="legacy", choices=("legacy", "numpy2"),
        help="QUAL/AF arithmetic: float64 as under the reference's NumPy 1.x (legacy) or float32 (numpy2)")
    add('--overlap_filter', type=str, default="off", choices=("off", "host", "device"),
        help="pass the finished VCF through the overlap filter (python -m clair_amd.overlap_variant: of two calls one of whose deletion covers "
             "the other, the one with the higher QUAL stays), with its walk on the host or on the GPU --device names; default: %(default)s")
    add('--gvcf_fn', type=str, default=None, metavar="FILE",
        help="also write a gVCF: the rows of --call_fn plus reference-confidence blocks banded by GQ that tile the rest of the region, from the "
             "tallies the device front end still holds (docs/gvcf.md; not with --vcf_fn, --ensemble_bam_fn, --ensemble_subsample)")
    from .gvcf import add_gvcf_options
    add_gvcf_options(add)
    return parser


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        sys.exit(1)
    Run(parser.parse_args(argv))


if __name__ == "__main__":
    main()
