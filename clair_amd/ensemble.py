"""ensemble: average the probabilities several models (or several BAMs) gave the same sites.  stdin -> stdout.

Counterpart of the reference's clair/post_processing/ensemble.py (:10-105), the middle of the chain docs/POST_PROCESSING.md describes:

    call_var --output_for_ensemble   (once per model / BAM)    rows `ctg pos seq 1056 ints 90 x %.6f`
    cat those | ensemble [--minimum_count_to_output N]          one row per site, probabilities averaged
    call_var --input_probabilities                              VCF

Same rows, byte for byte (tests/golden/ensemble_small.json.gz, minted from the reference's script):
  * a site is (ctg, pos) as text; sites come out in the order they were first seen;
  * seq and the 1056 counts are those of the site's FIRST row (a later row with another tensor does not change them);
  * probabilities are read with float(), added in input order in double, divided by the number of rows of the site and printed
    with '{:.6f}' (:33-43, :67);
  * sites with fewer than --minimum_count_to_output rows are left out (:58-59); no arguments at all prints the help, exit 1 (:98-100).

K models over ONE set of candidates need none of this text: call_var / callVarBam --ensemble_chkpnt_fn run the K forward passes and the
same arithmetic on the GPU, and callVarBam --ensemble_bam_fn merges runs whose sites differ (model x BAM) in a site table there
(docs/ensemble.md).  This filter stays for rows that were written elsewhere, and as the yardstick of both.
"""
import sys
from argparse import ArgumentParser

N_COUNTS = 33 * 8 * 4


class Site(object):
    __slots__ = ("seq", "counts", "sums", "rows")

    def __init__(self, seq, counts, probabilities):
        self.seq, self.counts, self.sums, self.rows = seq, counts, probabilities, 1

    def add(self, probabilities):
        self.sums = [s + p for s, p in zip(self.sums, probabilities)]       # input order, double: ensemble.py:39-43
        self.rows += 1


def sites_from(stream):
    """{(ctg, pos): Site} in first-seen order."""
    sites = {}
    for row in stream:
        cols = row.split("\t")
        key = (cols[0], cols[1])
        probabilities = [float(v) for v in cols[3 + N_COUNTS:]]
        site = sites.get(key)
        if site is None:
            sites[key] = Site(cols[2], [int(v) for v in cols[3:3 + N_COUNTS]], probabilities)
        else:
            if len(probabilities) < len(site.sums):
                raise IndexError("site %s:%s: a row with %d probabilities after one with %d" % (key[0], key[1], len(probabilities), len(site.sums)))
            site.add(probabilities)
    return sites


def rows_from(sites, minimum_count_to_output=0):
    for (ctg, pos), site in sites.items():
        if site.rows < minimum_count_to_output:
            continue
        yield "\t".join([ctg, pos, site.seq, "\t".join(str(c) for c in site.counts),
                         "\t".join("{:.6f}".format(s / site.rows) for s in site.sums)])


def build_parser():
    parser = ArgumentParser(description="Average the probabilities of call_var --output_for_ensemble rows per site (stdin to stdout)")
    parser.add_argument('--minimum_count_to_output', type=int, default=0, help="minimum # of calls to output the probabilities")
    return parser


def main(argv=None, stdin=None, stdout=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    if len(argv) == 0:
        parser.print_help()
        sys.exit(1)
    out = stdout if stdout is not None else sys.stdout
    for row in rows_from(sites_from(stdin if stdin is not None else sys.stdin), args.minimum_count_to_output):
        out.write(row + "\n")


if __name__ == "__main__":
    main()
