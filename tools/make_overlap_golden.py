#!/usr/bin/env python3
"""Mint tests/golden/overlap_small.json.gz from the REAL reference filter (runs only where a reference checkout exists, like the other
tools/make_*_golden.py): clair/post_processing/overlap_variant.py is RUN, as a process, on inputs built here; nothing of it is copied.

    python tools/make_overlap_golden.py --reference DIR        (or $CLAIR_REFERENCE: a checkout of the reference project)

The fixture (data only): {"inputs": [...], "outputs": [...]}, outputs[k] = stdout of the reference's filter given inputs[k] on stdin.
  inputs[0]   tests/golden/e2e_230_default.vcf as it is (a VCF this build writes: header, 230 rows, FILTER '.'; 14 of them go).
  the others  crafted streams, one case each (CASES below).  Every stream with a crafted overlap must lose at least one row and keep at
              least one; the streams without one must come out with every row.
"""
import argparse
import gzip
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "overlap_small.json.gz")
E2E = os.path.join(ROOT, "tests", "golden", "e2e_230_default.vcf")

HEADER = ('##fileformat=VCFv4.1\n'
          '##FILTER=<ID=PASS,Description="All filters passed">\n'
          '##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">\n'
          '##contig=<ID=chr1,length=1000000>\n'
          '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n')


def row(ctg, pos, ref, alt, qual, gt="0/1", dp="30", af="0.5000", flt="."):
    return "\t".join([ctg, str(pos), ".", ref, alt, str(qual), flt, ".", "GT:GQ:DP:AF", ":".join([gt, str(qual), dp, af])]) + "\n"


# (name, has a crafted overlap, with header, rows)
CASES = [
    ("a deletion over a SNP: the SNP inside goes, the one past its reach stays; then a SNP that outscores its deletion", True, True, [
        row("chr1", 100, "ACGT", "A", 50), row("chr1", 102, "G", "T", 20), row("chr1", 103, "T", "C", 49), row("chr1", 104, "A", "G", 10),
        row("chr1", 200, "AC", "A", 10), row("chr1", 201, "C", "G", 30, gt="1/1")]),
    ("a deletion over a deletion", True, True, [
        row("chr1", 100, "ACGTA", "A", 40), row("chr1", 103, "TAG", "T", 60), row("chr1", 110, "TAG", "T", 60), row("chr1", 112, "GCC", "G", 7)]),
    ("a deletion next to a pure insertion: nothing is dropped (no header either)", False, False, [
        row("chr1", 100, "ACG", "A", 50), row("chr1", 101, "C", "CTT", 10), row("chr1", 102, "G", "GA", 90)]),
    ("a 1/2 row whose second ALT decides the longest deletion", True, True, [
        row("chr1", 100, "ACGT", "ACG,A", 50, gt="1/2"), row("chr1", 103, "T", "C", 10), row("chr1", 104, "A", "C", 10),
        row("chr1", 200, "ACGT", "ACG", 50), row("chr1", 203, "T", "C", 10)]),
    ("a 1/2 row whose second ALT makes it a SNP", True, True, [
        row("chr1", 100, "ACGT", "A", 50), row("chr1", 102, "GT", "GTAA,CC", 10, gt="1/2"),
        row("chr1", 300, "ACGT", "A", 50), row("chr1", 302, "GT", "GTAA", 10)]),
    ("a chain of three: the middle row replaces the first and is then replaced", True, True, [
        row("chr1", 100, "ACGTACGT", "A", 10), row("chr1", 103, "TACGT", "T", 20), row("chr1", 106, "G", "T", 30), row("chr1", 107, "T", "A", 1)]),
    ("equal QUAL: the later row wins", True, True, [
        row("chr1", 100, "ACG", "A", 30), row("chr1", 101, "C", "T", 30)]),
    ("QUAL 12.9 is read as 12: a tie with 12, and below 12.99's 12 no more than equal", True, True, [
        row("chr1", 100, "ACG", "A", "12.9"), row("chr1", 101, "C", "T", 12),
        row("chr1", 200, "ACG", "A", 13), row("chr1", 201, "C", "T", "12.99")]),
    ("two contigs with the same positions", True, True, [
        row("chr1", 100, "ACGT", "A", 50), row("chr1", 102, "G", "A", 10),
        row("chr2", 100, "ACGT", "A", 10), row("chr2", 102, "G", "A", 50)]),
    ("a contig that reappears after another one: the row in between shields what follows", True, True, [
        row("chr1", 100, "ACGTACGT", "A", 50), row("chr2", 50, "A", "C", 5), row("chr1", 103, "T", "C", 10),
        row("chr1", 500, "ACG", "A", 50), row("chr1", 501, "C", "T", 10)]),
    ("rows out of position order: the pair is swapped before the intervals are compared", True, True, [
        row("chr1", 105, "G", "T", 10), row("chr1", 100, "ACGTACGT", "A", 50), row("chr1", 102, "G", "T", 70),
        row("chr1", 305, "G", "T", 90), row("chr1", 300, "ACGTACGT", "A", 50), row("chr1", 290, "ACG", "A", 50)]),
    ("a LowQual FILTER (and a PASS) do not survive the rendering", True, True, [
        row("chr1", 100, "ACG", "A", 3, flt="LowQual"), row("chr1", 101, "C", "T", 2, flt="LowQual"), row("chr1", 150, "C", "T", 200, flt="PASS")]),
    ("an exact duplicate row: of an overlapping pair one stays, of a pair of SNPs both", True, True, [
        row("chr1", 100, "ACG", "A", 30), row("chr1", 100, "ACG", "A", 30), row("chr1", 200, "C", "T", 5), row("chr1", 200, "C", "T", 5)]),
    ("header lines alone", False, True, []),
]


def build_inputs():
    """-> [(name, has a crafted overlap, text)]"""
    streams = [("this build's own VCF (nothing crafted, nothing asserted: it happens to hold overlaps)", None, open(E2E).read())]
    for name, crafted, with_header, rows in CASES:
        streams.append((name, crafted, (HEADER if with_header else "") + "".join(rows)))
    return streams


def data_rows(text):
    return [r for r in text.splitlines() if not r.startswith("#")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("CLAIR_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=OUT, help="where the fixture is written, default: %(default)s")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or CLAIR_REFERENCE) is needed: this tool runs the reference's own filter")
    script = os.path.join(args.reference, "clair", "post_processing", "overlap_variant.py")
    if not os.path.isfile(script):
        sys.exit("%s not found: this tool runs the reference's own filter" % script)
    inputs, outputs = [], []
    for name, crafted, text in build_inputs():
        r = subprocess.run([sys.executable, script], input=text, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the reference's filter failed on '%s': %s" % (name, r.stderr))
        n_in, n_out = len(data_rows(text)), len(data_rows(r.stdout))
        if crafted:
            assert 0 < n_out < n_in, "'%s': %d rows in, %d out -- the crafted overlap did not bite" % (name, n_in, n_out)
        elif crafted is not None:
            assert n_out == n_in, "'%s': %d rows in, %d out" % (name, n_in, n_out)
        print("%3d -> %3d rows  %s" % (n_in, n_out, name))
        inputs.append(text)
        outputs.append(r.stdout)
    with open(args.out, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as f:      # no name, no time: the same bytes wherever it is written
        f.write(json.dumps({"inputs": inputs, "outputs": outputs}).encode())
    print("%s: %d bytes, %d streams" % (args.out, os.path.getsize(args.out), len(inputs)))


if __name__ == "__main__":
    main()
