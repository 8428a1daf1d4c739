"""Seeded inputs for the overlap filter's walks (tests/test_overlap.py, tests/test_overlap_gpu.py): rows as clair_amd.overlap_variant
Variant tuples -- what its Python walk takes -- and, through its spans_from, as the span arrays the native walks take.

The rows are built to make the walk work: dense positions (gaps of 0 .. 3, so equal positions occur), deletions of a few bases on a
quarter of the rows and of up to 400 on a few (long chains of overlapping rows), 1/2 rows whose second ALT decides the deletion or makes
the row a "SNP", pure insertions, QUAL from a handful of values (ties), copies of the row before, one to four contigs in runs (a contig
may come back), and stretches shuffled out of position order between sorted ones."""
import numpy as np

from clair_amd import overlap_variant as ov


def variants(seed, n, contigs=1, shuffled=True, long_deletions=True):
    rng = np.random.default_rng(seed)
    out = []
    runs = max(1, min(n, contigs + int(rng.integers(0, 2)) if contigs > 1 else 1))       # one run more than contigs: a contig reappears
    cuts = sorted(rng.choice(np.arange(1, n), size=runs - 1, replace=False).tolist()) if runs > 1 else []
    run_of = np.searchsorted(np.asarray(cuts, dtype=np.int64), np.arange(n), side="right") if n else []
    pos = 1000
    for i in range(n):
        if i in cuts:
            pos = 1000 + int(rng.integers(0, 50))          # the next run starts over: the same positions on another contig
        pos += int(rng.integers(0, 4))
        ctg = "ctg%d" % (int(run_of[i]) % contigs)
        kind = rng.random()
        if kind < 0.45:                                     # SNP
            ref, alt, alt2 = "A", "C", None
        elif kind < 0.55:                                   # pure insertion: nothing a deletion can cover
            ref, alt, alt2 = "A", "A" + "T" * int(rng.integers(1, 9)), None
        elif kind < 0.80:                                   # short deletion
            ref, alt, alt2 = "A" * int(rng.integers(2, 7)), "A", None
        elif kind < 0.86:                                   # 1/2: the second ALT is the longer deletion
            ref, alt, alt2 = "A" * int(rng.integers(3, 9)), "AA", "A"
        elif kind < 0.92:                                   # 1/2: an insertion whose second ALT has REF's length
            ref, alt, alt2 = "AC", "ACTT", "GG"
        elif kind < 0.96 or not long_deletions:             # 1/2: a deletion that is a "SNP" as well
            ref, alt, alt2 = "ACG", "A", "TTT"
        else:                                               # a deletion over hundreds of bases
            ref, alt, alt2 = "A" * int(rng.integers(100, 401)), "A", None
        v = ov.Variant(ctg, pos, ref, alt, alt2, int(rng.choice([0, 5, 5, 12, 12, 12, 30, 77, 500])), "0/1", "30", "0.5000")
        if out and rng.random() < 0.05:
            v = out[-1]                                     # an exact duplicate
        out.append(v)
    if shuffled and n > 3:
        for _ in range(max(1, n // 100)):                   # stretches out of position order, inside what else stays sorted
            a = int(rng.integers(0, n - 2))
            b = min(n, a + int(rng.integers(2, 40)))
            out[a:b] = [out[a + int(k)] for k in rng.permutation(b - a)]
    return out


def generated(sizes=(0, 1, 2, 3, 1000)):
    """[(name, rows)]: every size, sorted and shuffled, one to four contigs."""
    cases = []
    for n in sizes:
        for contigs in (1, 2, 3, 4):
            for shuffled in (False, True):
                if (n < 4 and shuffled) or (n < 2 and contigs > 1):
                    continue
                seed = 7919 * n + 31 * contigs + int(shuffled)
                cases.append(("n%d_c%d_%s" % (n, contigs, "shuffled" if shuffled else "sorted"), variants(seed, n, contigs, shuffled)))
    return cases


def spans(rows):
    return ov.spans_from(rows)


def python_mask(rows):
    return np.asarray(ov.keep_mask(rows), dtype=np.uint8)


# -- crafted span arrays for the device path's block scan (B = rows per workgroup of the scan) ------------------------------------------------
def _snps(n, step=10):
    from clair_amd._hostapi import OVERLAP_SNP, SPAN_DTYPE
    s = np.zeros(n, dtype=SPAN_DTYPE)
    s["pos"] = 1000 + step * np.arange(n, dtype=np.int64)
    s["flags"] = OVERLAP_SNP
    s["qual"] = 10 + (np.arange(n) * 7919) % 13
    return s


def reach_crosses_a_block(B):
    """The last row of block 0 is a deletion over the first two rows of block 1: whether row B is a head is decided by block 0's maximum."""
    s = _snps(B + 10)
    s["del"][B - 1], s["qual"][B - 1] = 25, 400
    return s


def reach_carried_over_a_whole_block(B):
    """A deletion in block 0 that outscores every row up to its end inside block 2: block 1 only passes the maximum on."""
    s = _snps(2 * B + 50)
    s["del"][5], s["qual"][5] = 10 * (2 * B + 20 - 5), 400
    return s


def segment_spans_three_blocks(B):
    """Row 0 is a deletion over rows 1 .. 2B + 100, sorted positions: one segment from row 0 into the third block, a chain of replacements."""
    s = _snps(3 * B + 5)
    s["del"][0] = 10 * (2 * B + 100)
    s["del"][1:2 * B + 100:3] = 15          # short deletions on the way keep the chain going by themselves, too
    return s


def contig_changes_at_a_block(B):
    """Block 0's last row is a deletion that would cover block 1's first rows, but block 1 starts another contig at the same positions."""
    s = _snps(B + 40)
    s["ctg"][B:] = 1
    s["del"][B - 1], s["qual"][B - 1] = 200, 400
    s["del"][B + 3], s["qual"][B + 3] = 35, 400
    return s


def every_row_a_head(B):
    return _snps(B + 7)


def only_the_first_row_a_head(B):
    """One deletion over everything, and every row a deletion over the next one: row 0 is the only head, the walk one chain of B + 7 rows."""
    s = _snps(B + 7)
    s["del"] = 15
    s["del"][0] = 10 * (B + 7)
    return s


CRAFTED = (reach_crosses_a_block, reach_carried_over_a_whole_block, segment_spans_three_blocks, contig_changes_at_a_block, every_row_a_head,
           only_the_first_row_a_head)
