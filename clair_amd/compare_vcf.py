"""compare_vcf: score a call set against a truth set -- TP, FP, FN and genotype mismatches per variant type, precision, recall and F1,
the same at every integer QUAL cut-off 0 .. 1023, and the cut-off with the best F1.

    python -m clair_amd.compare_vcf --vcf_fn calls.vcf.gz --truth_vcf_fn truth.vcf.gz [--bed_fn confident.bed] [--ref_fn ref.fa [--left_align]]
                                    [--ctgName chr20] [--backend auto|device|host] [--json_fn out.json] [--detail_fn out.tsv] [--min_qual Q]

The reference has no such tool: what its README says about accuracy comes from an external comparison.  docs/compare_vcf.md states the rule
this one follows.  Parsing, allele normalisation, the join and the counting are native: `device` runs them on the GPU (csrc/compare.hip),
`host` in the sequential twin (hostsrc/host_compare.cpp), both over csrc/compare_core.h, and both give the same integers.  This module
reads the files, builds the contig table and the merged regions, sorts the 8-byte keys when a side is out of order, and turns the integers
into the report.  With --left_align it also reads the sequences of the contigs in use from --ref_fn, and both sides' indels are moved to
their leftmost position before the join (docs/compare_vcf.md, "Left alignment"), natively again.
"""
import ctypes
import gzip
import json
import os
import re
import sys
from argparse import ArgumentParser

import numpy as np

BACKENDS = ("auto", "device", "host")
SIDES = ("calls", "truth")
TYPES = ("SNP", "INS", "DEL", "MNP")
OUTCOMES = ("TP", "GT", "FP", "FN", "DUP", "OUTSIDE")
KINDS = ("tp", "gt", "fp")
ROWS = (("SNP", ("SNP",)), ("INS", ("INS",)), ("DEL", ("DEL",)), ("INDEL", ("INS", "DEL")), ("MNP", ("MNP",)), ("ALL", TYPES))
QUAL_BINS = 1024
STATS = ("lines", "rows", "records", "symbolic", "unknown_contig", "too_long", "sorted")
LEFT_ALIGN_STATS = ("examined", "shifted", "ref_mismatch", "at_contig_start", "no_sequence", "sorted", "arena_bytes")       # _left_align's stats[8]
# the counter block (CLAIR_COMPARE_COUNTS, csrc/compare_core.h; the table in docs/compare_vcf.md)
AT_COUNTS = 0
AT_HIST = 2 * len(TYPES) * len(OUTCOMES)
AT_AT_LEAST = AT_HIST + len(TYPES) * len(KINDS) * QUAL_BINS
AT_DROPS = AT_AT_LEAST + len(TYPES) * len(KINDS) * QUAL_BINS
N_COUNTS = AT_DROPS + 2 * 3
# struct clair_compare_record
RECORD_DTYPE = np.dtype([("ctg", "<i4"), ("pos", "<i4"), ("ref_off", "<u4"), ("alt_off", "<u4"), ("ref_len", "<u2"), ("alt_len", "<u2"),
                         ("qual_bin", "<u2"), ("copies", "u1"), ("type", "u1"), ("line", "<u4"), ("pad", "<u4")])
assert RECORD_DTYPE.itemsize == 32 and N_COUNTS == 24630
HEADER = "type\ttruth\tcalls\tTP\tFP\tFN\tGT\tprecision\trecall\tF1\tbest_qual\tbest_F1"


# -- inputs --------------------------------------------------------------------------------------------------------------------------------
def read_bytes(path):
    """A plain, gzip or BGZF file as bytes (gzip reads the last two alike)."""
    with open(path, "rb") as f:
        magic = f.read(2)
    with (gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")) as f:
        return f.read()


def concatenate(texts):
    """Files one after the other; a file whose last line has no line feed gets one, so that the next file's first line stays a line."""
    return b"".join(t if not t or t.endswith(b"\n") else t + b"\n" for t in texts)


def var_to_vcf(text):
    """GetTruth rows `ctg pos ref alt g1 g2` -> the minimal VCF line of each, which then goes through the same parser."""
    out = []
    for n, row in enumerate(text.split(b"\n")):
        row = row.rstrip(b"\r")
        if not row:
            continue
        f = row.split()
        if len(f) != 6:
            raise ValueError("truth line %d: a .var row has 6 columns, this one has %d" % (n + 1, len(f)))
        out.append(b"\t".join([f[0], f[1], b".", f[2], f[3], b".", b".", b".", b"GT", f[4] + b"/" + f[5]]))
    return b"".join(r + b"\n" for r in out)


def contigs_of(texts):
    """The contigs of data rows in order of first appearance."""
    seen = {}
    for t in texts:
        for m in re.finditer(rb"^([^#\t\r\n][^\t\r\n]*)\t", t, flags=re.M):
            seen.setdefault(m.group(1), None)
    return [c.decode("latin-1") for c in seen]


def contigs_from_fai(ref_fn):
    fai = ref_fn + ".fai"
    if not os.path.isfile(fai):
        raise ValueError("%s not found: --ref_fn is read through its .fai only" % fai)
    with open(fai) as f:
        return [row.split("\t")[0] for row in f if row.strip()]


def load_reference(ref_fn, contigs):
    """The sequences of `contigs` from a FASTA, read through its .fai -> {contig: bytes}: line ends removed, case kept.  A contig the .fai does
    not have is left out (the native side then counts its indels as no_sequence)."""
    fai = ref_fn + ".fai"
    if not os.path.isfile(fai):
        raise ValueError("%s not found: --ref_fn is read through its .fai only" % fai)
    index = {}
    with open(fai) as f:
        for n, row in enumerate(f):
            cols = row.rstrip("\n").split("\t")
            if not row.strip():
                continue
            if len(cols) < 5 or not all(c.isdigit() for c in cols[1:5]) or int(cols[3]) < 1 or int(cols[4]) < int(cols[3]):
                raise ValueError("%s line %d: not `name length offset linebases linewidth`" % (fai, n + 1))
            index.setdefault(cols[0], tuple(int(c) for c in cols[1:5]))
    out = {}
    with open(ref_fn, "rb") as f:
        for c in contigs:
            if c not in index:
                continue
            length, offset, bases, width = index[c]
            f.seek(offset)
            raw = f.read(length // bases * width + length % bases)
            seq = raw.replace(b"\n", b"").replace(b"\r", b"")
            if len(seq) != length:
                raise ValueError("%s: contig %s has %d bases where its .fai says %d" % (ref_fn, c, len(seq), length))
            out[c] = seq
    return out


def merged_regions(bed_fn, contigs):
    """A BED file -> {contig: [(start, end), ...]} sorted and merged (touching intervals too), for the contigs of the table."""
    raw = {}
    with (gzip.open(bed_fn, "rt") if bed_fn.endswith(".gz") else open(bed_fn)) as f:
        for n, row in enumerate(f):
            cols = row.split()
            if not cols or cols[0] in ("track", "browser") or cols[0].startswith("#"):
                continue
            if len(cols) < 3 or not cols[1].isdigit() or not cols[2].isdigit():
                raise ValueError("%s line %d: not `contig start end`" % (bed_fn, n + 1))
            if int(cols[2]) > int(cols[1]):
                raw.setdefault(cols[0], []).append((int(cols[1]), int(cols[2])))
    return dict((c, merge_intervals(raw[c])) for c in contigs if c in raw)


def merge_intervals(intervals):
    out = []
    for s, e in sorted(intervals):
        if out and s <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


# -- the native comparison -----------------------------------------------------------------------------------------------------------------
class _Native(object):
    """One comparison handle of either library: `prefix` is clair_compare_ (device) or clair_host_compare_ (host).  The host twin borrows the
    texts it parses: the caller keeps them alive until close()."""

    def __init__(self, backend, device=0):
        self._h = ctypes.c_void_p()
        if backend == "device":
            from clair_amd import _capi
            self._lib, self._prefix, self._error = _capi.load(), "clair_compare_", _capi.EngineError
            self._message = lambda: self._lib.clair_compare_last_error(self._h).decode()
            rc = self._lib.clair_compare_create(int(device), ctypes.byref(self._h))
        else:
            from clair_amd import _hostapi
            self._lib, self._prefix, self._error = _hostapi.load(), "clair_host_compare_", ValueError
            self._message = lambda: self._lib.clair_host_last_error().decode()
            rc = self._lib.clair_host_compare_create(ctypes.byref(self._h))
        if rc != 0:
            raise self._error("compare_vcf: " + self._message())

    def call(self, name, *args):
        """Non-zero: a malformed row (ValueError, the message names side and line) or anything else (the library's own exception)."""
        if getattr(self._lib, self._prefix + name)(self._h, *args) != 0:
            message = self._message()
            raise (ValueError if re.match(r"(calls|truth) line \d+: ", message) else self._error)(message)

    def close(self):
        if self._h:
            getattr(self._lib, self._prefix + "destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _address(a):
    return ctypes.c_void_p(a.ctypes.data)


def pick_backend(backend):
    if backend not in BACKENDS:
        raise ValueError("backend %r: one of %s" % (backend, ", ".join(BACKENDS)))
    if backend != "auto":
        return backend
    from clair_amd import _capi
    return "device" if _capi.load().clair_device_count() > 0 else "host"


def compare(calls_text, truth_text, contigs, regions=None, backend="auto", device=0, reference=None):
    """calls_text, truth_text: VCF as bytes; contigs: the names, whose order is the order of the records; regions: {contig: [(start, end)]}
    sorted and merged (merged_regions), or None for no bed file.  -> dict: backend; stats[side] (STATS, plus `permuted`); counts (int64
    [N_COUNTS], the counter block); records[side] (RECORD_DTYPE, in (contig, pos, file) order) and outcomes[side] (uint8, OUTCOMES).
    reference: None, or {contig: sequence as bytes} (load_reference) to left-align the indels of both sides first; then also
    left_align[side] (LEFT_ALIGN_STATS) and alleles[side], the bytes the records' ref_off / alt_off index in place of the text."""
    backend = pick_backend(backend)
    texts = [np.frombuffer(t, dtype=np.uint8) for t in (calls_text, truth_text)]
    names = [c.encode("latin-1") for c in contigs]
    if len(set(names)) != len(names):
        raise ValueError("a contig is named twice in the contig table")
    blob = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)
    offsets = np.zeros(len(names) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(n) for n in names])
    native = _Native(backend, device)
    try:
        native.call("set_contigs", _address(blob), _address(offsets), len(names))
        if regions is None:
            native.call("set_regions", None, None, None, -1)
        else:
            per = [regions.get(c, []) for c in contigs]
            first = np.zeros(len(names) + 1, dtype=np.int64)
            first[1:] = np.cumsum([len(p) for p in per])
            flat = np.array([iv for p in per for iv in p], dtype=np.int64).reshape(-1, 2)
            starts, ends = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
            native.call("set_regions", _address(first), _address(starts), _address(ends), len(starts))
        result = {"backend": backend, "stats": {}, "records": {}, "outcomes": {}}
        if reference is not None:
            sequences = [reference.get(c, b"") for c in contigs]
            ref_offsets = np.zeros(len(names) + 1, dtype=np.int64)
            ref_offsets[1:] = np.cumsum([len(q) for q in sequences])
            ref_blob = np.frombuffer(b"".join(sequences) or b"\0", dtype=np.uint8)      # borrowed by the host twin until close()
            native.call("set_reference", _address(ref_blob), _address(ref_offsets), len(names))
            result["left_align"], result["alleles"] = {}, {}
        for side, text in enumerate(texts):
            stats = np.zeros(8, dtype=np.int64)
            native.call("parse", side, _address(text) if len(text) else None, len(text), _address(stats))
            st = dict(zip(STATS, (int(v) for v in stats)))
            st["permuted"] = 0
            in_order = st["sorted"]
            if reference is not None:
                native.call("left_align", side, _address(stats))
                la = dict(zip(LEFT_ALIGN_STATS, (int(v) for v in stats)))
                in_order = la["sorted"]                  # on the new positions: it supersedes the parse pass's
                alleles = np.zeros(max(la["arena_bytes"], 1), dtype=np.uint8)
                native.call("allele_text", side, _address(alleles))
                result["left_align"][SIDES[side]], result["alleles"][SIDES[side]] = la, alleles[:la["arena_bytes"]].tobytes()
            if not in_order:
                keys = np.zeros(st["records"], dtype=np.int64)
                native.call("keys", side, _address(keys))
                perm = np.ascontiguousarray(np.argsort(keys, kind="stable"), dtype=np.int64)
                native.call("permute", side, _address(perm))
                st["permuted"] = 1
            result["stats"][SIDES[side]] = st
        native.call("run")
        counts = np.zeros(N_COUNTS, dtype=np.int64)
        native.call("counts", _address(counts))
        result["counts"] = counts
        for side, name in enumerate(SIDES):
            n = result["stats"][name]["records"]
            records, outcomes = np.zeros(n, dtype=RECORD_DTYPE), np.zeros(n, dtype=np.uint8)
            native.call("records", side, _address(records) if n else None, _address(outcomes) if n else None)
            result["records"][name], result["outcomes"][name] = records, outcomes
        return result
    finally:
        native.close()


# -- the report ----------------------------------------------------------------------------------------------------------------------------
def ratio(a, b):
    return float(a) / float(b) if b else 0.0


def summary(counts, min_qual=0):
    """The counter block -> one dict per row of the report (ROWS): the integers at min_qual, the three cumulative arrays, the best cut-off."""
    if not 0 <= min_qual < QUAL_BINS:
        raise ValueError("--min_qual %d: 0 .. %d" % (min_qual, QUAL_BINS - 1))
    by = np.asarray(counts[AT_COUNTS:AT_HIST]).reshape(2, len(TYPES), len(OUTCOMES))
    hist = np.asarray(counts[AT_HIST:AT_AT_LEAST]).reshape(len(TYPES), len(KINDS), QUAL_BINS)
    at_least = np.asarray(counts[AT_AT_LEAST:AT_DROPS]).reshape(len(TYPES), len(KINDS), QUAL_BINS)
    rows = []
    for name, members in ROWS:
        ids = [TYPES.index(m) for m in members]
        truth = int(sum(by[1, t, 0] + by[1, t, 1] + by[1, t, 3] for t in ids))      # truth records inside, duplicates out: TP + GT + FN
        al = dict((k, [int(v) for v in at_least[ids, KINDS.index(k)].sum(axis=0)]) for k in KINDS)
        hs = dict((k, [int(v) for v in hist[ids, KINDS.index(k)].sum(axis=0)]) for k in KINDS)

        def at(q):
            tp, gt = al["tp"][q], al["gt"][q]
            fp = al["fp"][q] + gt
            return tp, fp, truth - tp, gt

        best = 0
        for q in range(1, QUAL_BINS):        # F1 = 2 TP / (TP + FP + truth), compared as fractions of integers; the smallest q wins a tie
            tp, fp, _, _ = at(q)
            btp, bfp, _, _ = at(best)
            if tp * (btp + bfp + truth) > btp * (tp + fp + truth):
                best = q
        tp, fp, fn, gt = at(min_qual)
        btp, bfp, bfn, _ = at(best)
        rows.append({"type": name, "truth": truth, "calls": tp + fp, "TP": tp, "FP": fp, "FN": fn, "GT": gt,
                     "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn), "F1": ratio(2 * tp, 2 * tp + fp + fn),
                     "best_qual": best, "best_F1": ratio(2 * btp, 2 * btp + bfp + bfn), "at_least": al, "hist": hs})
    return rows


def report_text(rows):
    lines = [HEADER]
    for r in rows:
        lines.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%d\t%.6f" % (r["type"], r["truth"], r["calls"], r["TP"], r["FP"], r["FN"], r["GT"],
                                                                              r["precision"], r["recall"], r["F1"], r["best_qual"], r["best_F1"]))
    return "".join(line + "\n" for line in lines)


def report_json(result, rows, contigs, min_qual):
    counts = result["counts"]
    by = counts[AT_COUNTS:AT_HIST].reshape(2, len(TYPES), len(OUTCOMES))
    out = {
        "min_qual": min_qual,
        "contigs": list(contigs),
        "stats": dict((s, dict((k, v) for k, v in result["stats"][s].items())) for s in SIDES),
        "counts": dict((s, dict((t, dict((o, int(by[i, j, k])) for k, o in enumerate(OUTCOMES))) for j, t in enumerate(TYPES))) for i, s in enumerate(SIDES)),
        "rows": rows,
    }
    if "left_align" in result:
        out["left_align"] = dict((s, dict(result["left_align"][s])) for s in SIDES)
    return out


def detail_lines(result, texts, contigs):
    """One line per FP, FN or GT record: side ctg pos ref alt copies qual outcome, the alleles and the position the normalised ones.
    texts: what the records' offsets index, per side: the parsed texts, or result["alleles"] after left alignment (upper-cased then)."""
    for side, text in zip(SIDES, texts):
        records, outcomes = result["records"][side], result["outcomes"][side]
        for i in np.flatnonzero((outcomes >= 1) & (outcomes <= 3)):
            r = records[i]
            ref = text[int(r["ref_off"]):int(r["ref_off"]) + int(r["ref_len"])].decode("latin-1")
            alt = text[int(r["alt_off"]):int(r["alt_off"]) + int(r["alt_len"])].decode("latin-1")
            yield "%s\t%s\t%d\t%s\t%s\t%d\t%d\t%s\n" % (side, contigs[int(r["ctg"])], int(r["pos"]), ref, alt, int(r["copies"]), int(r["qual_bin"]),
                                                       OUTCOMES[int(outcomes[i])])


# -- command line --------------------------------------------------------------------------------------------------------------------------
def build_parser():
    parser = ArgumentParser(description="Score a call set against a truth set: TP, FP, FN, genotype mismatches, precision, recall and F1 per variant type, "
                                        "at every QUAL cut-off 0 .. 1023")
    parser.add_argument('--vcf_fn', type=str, action="append", default=None, help="The calls: VCF, plain, gzip or BGZF; repeatable, files are concatenated in the order given")
    parser.add_argument('--truth_vcf_fn', type=str, default=None, help="The truth as a VCF (this or --var_fn)")
    parser.add_argument('--var_fn', type=str, default=None, help="The truth as GetTruth rows `ctg pos ref alt g1 g2` (this or --truth_vcf_fn)")
    parser.add_argument('--bed_fn', type=str, default=None, help="Confident regions; records outside are ignored, optional")
    parser.add_argument('--ref_fn', type=str, default=None, help="Reference fasta; its .fai gives the contig order, and with --left_align the sequences "
                        "of the contigs in use are read through it, optional")
    parser.add_argument('--left_align', action="store_true", help="Move the indels of both sides to their leftmost position in the reference before the join "
                        "(needs --ref_fn), so that one event written at two positions of a repeat matches, default: off")
    parser.add_argument('--ctgName', type=str, default=None, help="Restrict both sides to this contig, optional")
    parser.add_argument('--backend', type=str, default="auto", choices=BACKENDS, help="Where parsing, join and counting run: the GPU, the host twin, or the "
                        "GPU when one is visible; the report is the same, default: %(default)s")
    parser.add_argument('--device', type=int, default=0, help="HIP device ordinal of --backend device, default: %(default)s")
    parser.add_argument('--json_fn', type=str, default=None, help="Write the counts, the cumulative arrays per type and the best cut-offs here, optional")
    parser.add_argument('--detail_fn', type=str, default=None, help="Write one line per FP, FN or genotype-mismatch record here, optional")
    parser.add_argument('--min_qual', type=int, default=0, help="The QUAL cut-off of the printed counts, 0 .. 1023, default: %(default)s")
    return parser


def run(args, stdout=None):
    if not args.vcf_fn:
        raise ValueError("--vcf_fn is required")
    if (args.truth_vcf_fn is None) == (args.var_fn is None):
        raise ValueError("exactly one of --truth_vcf_fn and --var_fn is required")
    if not 0 <= args.min_qual < QUAL_BINS:
        raise ValueError("--min_qual %d: 0 .. %d" % (args.min_qual, QUAL_BINS - 1))
    calls = concatenate([read_bytes(fn) for fn in args.vcf_fn])
    truth = read_bytes(args.truth_vcf_fn) if args.truth_vcf_fn else var_to_vcf(read_bytes(args.var_fn))
    contigs = contigs_from_fai(args.ref_fn) if args.ref_fn else contigs_of([calls, truth])
    if args.ctgName is not None:
        contigs = [args.ctgName]
    regions = merged_regions(args.bed_fn, contigs) if args.bed_fn else None
    reference = None
    if args.left_align:
        if not args.ref_fn:
            raise ValueError("--left_align needs --ref_fn")
        named = set(contigs_of([calls, truth]))
        reference = load_reference(args.ref_fn, [c for c in contigs if c in named])
    result = compare(calls, truth, contigs, regions, backend=args.backend, device=args.device, reference=reference)
    for side in SIDES if reference is not None else ():
        la = result["left_align"][side]
        if la["ref_mismatch"] or la["at_contig_start"] or la["no_sequence"]:
            sys.stderr.write("[WARNING] %s: %d indel records not left-aligned: %d whose REF differs from the reference, %d at a contig start, %d on contigs "
                             "without sequence\n" % (side, la["ref_mismatch"] + la["at_contig_start"] + la["no_sequence"], la["ref_mismatch"],
                                                     la["at_contig_start"], la["no_sequence"]))
    rows = summary(result["counts"], args.min_qual)
    (stdout if stdout is not None else sys.stdout).write(report_text(rows))
    if args.json_fn:
        with open(args.json_fn, "w") as f:
            json.dump(report_json(result, rows, contigs, args.min_qual), f, sort_keys=True)
            f.write("\n")
    if args.detail_fn:
        with open(args.detail_fn, "w") as f:
            f.writelines(detail_lines(result, [result["alleles"][s] for s in SIDES] if reference is not None else (calls, truth), contigs))
    return result


def main(argv=None, stdout=None):
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if argv is None and len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    try:
        run(args, stdout)
    except (ValueError, RuntimeError, OSError) as exc:      # a malformed row, a flag error, no GPU for --backend device, a missing file
        sys.exit("[ERROR] %s" % exc)


if __name__ == "__main__":
    main()
