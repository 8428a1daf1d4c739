"""overlap_variant: drop the lower-QUAL one of two calls when a deletion covers the other.  stdin -> stdout.

Counterpart of the reference's clair/post_processing/overlap_variant.py (:1-285), the last stage of docs/POST_PROCESSING.md: every position
is classified on its own, so a deletion call can cover a following SNP or deletion call; of such a pair the call with the higher QUAL stays.

    python -m clair_amd.overlap_variant [--backend python|host|device] [--device N] < calls.vcf > filtered.vcf

Same output, byte for byte (tests/golden/overlap_small.json.gz, minted from the reference's script; docs/overlap_variant.md has the rule):
  * header rows come out first, unchanged; every kept data row is re-rendered from its parsed fields (:189-213): ID, FILTER and INFO
    become ".", FORMAT "GT:GQ:DP:AF", GQ the integer QUAL; a third ALT is lost, as in the reference;
  * the walk (:237-267) compares each row with the last row kept, in input order, sorted or not.

Parsing and rendering are Python in every backend.  What the backends differ in is who does the walk: `python` the loop below, `host`
clair_host_overlap_keep, `device` clair_overlap_keep on the GPU (csrc/overlap_core.h is the rule both native ones run); they receive the rows
reduced to spans and return one byte per row.  call_var / callVarBam --overlap_filter run the same function over the VCF they wrote.
"""
import sys
from argparse import ArgumentParser
from collections import namedtuple

BACKENDS = ("python", "host", "device")
NO_SECOND_ALT = 1024            # the length a missing second ALT counts with in the longest deletion (:32)

Variant = namedtuple("Variant", ["ctg", "pos", "ref", "alt", "alt2", "qual", "gt", "dp", "af"])


def variant_from(row):
    """:155-186"""
    columns = row.split("\t")
    alternates = columns[4].split(",")
    last = columns[-1].split(":")
    return Variant(ctg=columns[0], pos=int(columns[1]), ref=columns[3], alt=alternates[0], alt2=None if len(alternates) == 1 else alternates[1],
                   qual=int(float(columns[5])), gt=last[0], dp=last[2], af=last[3])


def row_from(v):
    """:189-213"""
    q = str(v.qual)
    return "\t".join([v.ctg, str(v.pos), ".", v.ref, v.alt if v.alt2 is None else v.alt + "," + v.alt2, q, ".", ".", "GT:GQ:DP:AF",
                      ":".join([v.gt, q, v.dp, v.af])])


def longest_deletion(v):
    return len(v.ref) - min(len(v.alt), NO_SECOND_ALT if v.alt2 is None else len(v.alt2))


def is_snp(v):
    return len(v.ref) == len(v.alt) or (v.alt2 is not None and len(v.ref) == len(v.alt2))


def overlaps(last, v):
    """:122-152: the deletion of the row at the lower position (of `last` at equal positions) reaches the other row's SNP or deletion."""
    if last.ctg != v.ctg:
        return False
    a, b = (last, v) if last.pos <= v.pos else (v, last)
    d = longest_deletion(a)
    return d > 0 and (is_snp(b) or longest_deletion(b) > 0) and b.pos <= a.pos + d


def keep_mask(variants):
    """:237-267 as one flag per row: True for the rows that stay."""
    keep = [False] * len(variants)
    last = None
    for i, v in enumerate(variants):
        if last is not None and overlaps(variants[last], v):
            if variants[last].qual > v.qual:
                continue
            keep[last] = False          # equal QUAL: the later row wins (:234)
        keep[i] = True
        last = i
    return keep


def spans_from(variants):
    """The rows as clair_amd._hostapi.SPAN_DTYPE records (csrc/overlap_core.h): what the native walks take."""
    import numpy as np
    from clair_amd._hostapi import OVERLAP_SNP, SPAN_DTYPE
    spans = np.zeros(len(variants), dtype=SPAN_DTYPE)
    ids = {}
    for i, v in enumerate(variants):
        if not -2 ** 31 <= v.qual < 2 ** 31 or not -2 ** 62 <= v.pos < 2 ** 62:
            raise ValueError("row %d (%s:%d, QUAL %d): outside what the native backends hold; --backend python takes it" % (i + 1, v.ctg, v.pos, v.qual))
        spans[i] = (v.pos, ids.setdefault(v.ctg, len(ids)), v.qual, longest_deletion(v), OVERLAP_SNP if is_snp(v) else 0)
    return spans


def native_mask(variants, backend, device=0):
    if backend == "host":
        from clair_amd import _hostapi
        return _hostapi.overlap_keep(spans_from(variants)).astype(bool).tolist()
    from clair_amd import _capi
    return _capi.overlap_keep(spans_from(variants), device=device).astype(bool).tolist()


def split_rows(text):
    """header_and_variant_rows_from_stdin (:216-225): rows are cut at '\\n' and lose their LAST CHARACTER, which for a last row without a line
    end is not a line end -- as in the reference."""
    rows = text.split("\n")
    if rows[-1] == "":
        rows.pop()
    else:
        rows[-1] = rows[-1][:-1]
    header, body = [], []
    for n, row in enumerate(rows):
        if row == "":
            raise ValueError("line %d is empty (the reference fails on it too)" % (n + 1))
        (header if row[0] == "#" else body).append(row)
    return header, body


def filter_vcf_text(text, backend="python", device=0):
    """The filter over a whole VCF as one string -> the filtered VCF as one string."""
    if backend not in BACKENDS:
        raise ValueError("backend %r: one of %s" % (backend, ", ".join(BACKENDS)))
    header, body = split_rows(text) if text else ([], [])
    variants = [variant_from(row) for row in body]
    keep = keep_mask(variants) if backend == "python" else native_mask(variants, backend, device)
    out = header + [row_from(v) for v, k in zip(variants, keep) if k]
    return "".join(row + "\n" for row in out)


def build_parser():
    parser = ArgumentParser(description="Of two calls one of whose deletion covers the other, keep the one with the higher QUAL (VCF, stdin to stdout)")
    parser.add_argument('--backend', type=str, default="python", choices=BACKENDS,
                        help="who walks the rows: this module, the host library, or the GPU; the output is the same, default: %(default)s")
    parser.add_argument('--device', type=int, default=0, help="HIP device ordinal of --backend device, default: %(default)s")
    return parser


def main(argv=None, stdin=None, stdout=None):
    """No help on an empty command line: the reference takes no arguments and reads stdin unconditionally (:277-281)."""
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    text = (stdin if stdin is not None else sys.stdin).read()
    try:
        filtered = filter_vcf_text(text, args.backend, args.device)
    except RuntimeError as exc:          # the device library's errors (no GPU, no library): a message and a non-zero exit
        sys.exit("[ERROR] %s" % exc)
    (stdout if stdout is not None else sys.stdout).write(filtered)


if __name__ == "__main__":
    main()
