"""compare_vcf's yardstick: the rule of docs/compare_vcf.md restated in plain Python -- strings, dicts and `sorted`, nothing of the package --
a seeded generator of call / truth pairs that exercises every clause of it, and crafted cases, some with their expected counts as literals
worked out by hand.  tests/test_compare_vcf.py holds the host twin against this, tests/test_compare_vcf_gpu.py the device against the twin.
"""
import random
import re

TYPES = ("SNP", "INS", "DEL", "MNP")
OUTCOMES = ("TP", "GT", "FP", "FN", "DUP", "OUTSIDE")
TP, GT, FP, FN, DUP, OUTSIDE = range(6)
QUAL_BINS = 1024
AT_COUNTS, AT_HIST = 0, 48
AT_AT_LEAST = AT_HIST + 4 * 3 * QUAL_BINS
AT_DROPS = AT_AT_LEAST + 4 * 3 * QUAL_BINS
N_COUNTS = AT_DROPS + 6
SCAN_BLOCK = 2048           # the device scan's items per workgroup (clair_amd._capi.COMPARE_SCAN_BLOCK; the test checks they agree)
JOIN_BLOCK = 256            # records per workgroup of the join
MAX_POS = 2000000000


class RowError(Exception):
    def __init__(self, side, line, what):
        Exception.__init__(self, "%s line %d: %s" % (side, line, what))
        self.side, self.line = side, line


def up(s):
    """Upper-cased as the rule does it: a-z only."""
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in s)


def symbolic(alt):
    return alt in ("*", ".") or any(c in alt for c in "<[]")


def trim(pos, ref, alt):
    """-> pos, how many bases went at the front, how many at the back."""
    back = front = 0
    r, a = up(ref), up(alt)
    while len(r) > 1 and len(a) > 1 and r[-1] == a[-1]:
        r, a, back = r[:-1], a[:-1], back + 1
    while len(r) > 1 and len(a) > 1 and r[0] == a[0]:
        r, a, front = r[1:], a[1:], front + 1
    return pos + front, front, back


def type_of(ref_len, alt_len):
    return 1 if ref_len < alt_len else 2 if ref_len > alt_len else 0 if ref_len == 1 else 3


def parse_side(text, contigs, side):
    """-> records in file order, each a dict (the fields of the 32-byte record, plus REF / ALT upper-cased and `trimmed`), and the statistics."""
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()
    stats = dict(lines=len(lines), rows=0, records=0, symbolic=0, unknown_contig=0, too_long=0)
    records, at = [], 0
    for n, raw in enumerate(lines):
        start, at = at, at + len(raw) + 1
        line = raw[:-1] if raw.endswith("\r") else raw
        if line == "" or line[0] == "#":
            continue
        cols = line.split("\t")
        if len(cols) < 10:
            raise RowError(side, n + 1, "columns")
        if not re.fullmatch("[0-9]+", cols[1]) or int(cols[1]) > MAX_POS:
            raise RowError(side, n + 1, "POS")
        if cols[5] == ".":
            qual = 0
        elif re.fullmatch(r"[0-9]+(\.[0-9]*)?", cols[5]):
            qual = min(int(cols[5].split(".")[0]), QUAL_BINS - 1)
        else:
            raise RowError(side, n + 1, "QUAL")
        fmt = cols[8].split(":")
        if "GT" not in fmt:
            raise RowError(side, n + 1, "FORMAT")
        sample = cols[9].split(":")
        if fmt.index("GT") >= len(sample):
            raise RowError(side, n + 1, "GT")
        m = re.fullmatch(r"(\.|[0-9]+)(?:[/|](\.|[0-9]+))?", sample[fmt.index("GT")])
        if not m:
            raise RowError(side, n + 1, "GT")
        gt = [0 if g == "." else int(g) for g in m.groups() if g is not None]
        alts = cols[4].split(",")
        if any(g > len(alts) for g in gt):
            raise RowError(side, n + 1, "GT")
        if cols[3] == "":
            raise RowError(side, n + 1, "allele")
        stats["rows"] += 1
        wanted = []
        for g in gt:
            if g != 0 and g not in wanted:
                wanted.append(g)
        if any(alts[g - 1] == "" for g in wanted):
            raise RowError(side, n + 1, "allele")
        ref_at = start + sum(len(c) + 1 for c in cols[:3])
        alt_at = ref_at + len(cols[3]) + 1
        for g in wanted:
            ref, alt = cols[3], alts[g - 1]
            if symbolic(alt):
                stats["symbolic"] += 1
            elif cols[0] not in contigs:
                stats["unknown_contig"] += 1
            elif len(ref) > 65535 or len(alt) > 65535:
                stats["too_long"] += 1
            else:
                pos, front, back = trim(int(cols[1]), ref, alt)
                this_alt_at = alt_at + sum(len(a) + 1 for a in alts[:g - 1])
                ref_len, alt_len = len(ref) - front - back, len(alt) - front - back
                records.append(dict(ctg=contigs.index(cols[0]), pos=pos, ref_off=ref_at + front, alt_off=this_alt_at + front, ref_len=ref_len, alt_len=alt_len,
                                    qual_bin=qual, copies=gt.count(g), type=type_of(ref_len, alt_len), line=n + 1,
                                    ref=up(ref)[front:front + ref_len], alt=up(alt)[front:front + alt_len], trimmed=front + back > 0))
    stats["records"] = len(records)
    return records, stats


def inside(regions, contig, pos):
    return regions is None or any(s < pos <= e for s, e in regions.get(contig, ()))


def restate_full(calls_text, truth_text, contigs, regions):
    """regions: {contig: [(start, end), ...]} as the BED file has them, in any order, overlapping or not; None: no BED file.
    -> dict: counts (the counter block as a list of N_COUNTS ints), stats, records and outcomes per side ("calls", "truth") in
    (contig, pos, file) order."""
    sides, stats, outcomes = {}, {}, {}
    for side, text in (("calls", calls_text), ("truth", truth_text)):
        records, st = parse_side(text, contigs, side)
        keys = [(r["ctg"], r["pos"]) for r in records]
        st["sorted"] = int(all(a <= b for a, b in zip(keys, keys[1:])))
        order = sorted(range(len(records)), key=lambda i: (keys[i], i))
        sides[side], stats[side] = [records[i] for i in order], st
        seen, out = set(), []
        for r in sides[side]:
            allele = (r["ctg"], r["pos"], r["ref"], r["alt"])
            out.append(DUP if allele in seen else None if inside(regions, contigs[r["ctg"]], r["pos"]) else OUTSIDE)
            seen.add(allele)
        outcomes[side] = out
    truth_at = {}
    for j, r in enumerate(sides["truth"]):
        if outcomes["truth"][j] != DUP:
            truth_at[(r["ctg"], r["pos"], r["ref"], r["alt"])] = j
    for i, r in enumerate(sides["calls"]):
        if outcomes["calls"][i] is None:
            j = truth_at.get((r["ctg"], r["pos"], r["ref"], r["alt"]))
            if j is None:
                outcomes["calls"][i] = FP
            else:
                outcomes["calls"][i] = outcomes["truth"][j] = TP if sides["truth"][j]["copies"] == r["copies"] else GT
    outcomes["truth"] = [FN if o is None else o for o in outcomes["truth"]]
    counts = [0] * N_COUNTS
    for k, side in enumerate(("calls", "truth")):
        for r, o in zip(sides[side], outcomes[side]):
            counts[AT_COUNTS + (k * 4 + r["type"]) * 6 + o] += 1
            if side == "calls" and o in (TP, GT, FP):
                counts[AT_HIST + (r["type"] * 3 + o) * QUAL_BINS + r["qual_bin"]] += 1
        for d, name in enumerate(("symbolic", "unknown_contig", "too_long")):
            counts[AT_DROPS + k * 3 + d] = stats[side][name]
    for row in range(12):
        at_least = 0
        for q in reversed(range(QUAL_BINS)):             # at_least[q] = the sum of hist[q ..]
            at_least += counts[AT_HIST + row * QUAL_BINS + q]
            counts[AT_AT_LEAST + row * QUAL_BINS + q] = at_least
    return dict(counts=counts, stats=stats, records=sides, outcomes=outcomes)


def restate(calls_text, truth_text, contigs, regions):
    full = restate_full(calls_text, truth_text, contigs, regions)
    return full["counts"], full["outcomes"]


def side_counts(counts, side, type_name):
    """{outcome name: n} of one side and type of a counter block."""
    at = AT_COUNTS + (("calls", "truth").index(side) * 4 + TYPES.index(type_name)) * 6
    return dict(zip(OUTCOMES, counts[at:at + 6]))


def richness(full):
    """What a generated pair must hold so that a comparison on it means something: per variant type present, every outcome on some side and a
    record that trimming changed.  -> the list of what is missing."""
    missing = []
    present = set(r["type"] for side in full["records"].values() for r in side)
    for t in sorted(present):
        have = set(o for side in ("calls", "truth") for r, o in zip(full["records"][side], full["outcomes"][side]) if r["type"] == t)
        missing += ["%s %s" % (TYPES[t], OUTCOMES[o]) for o in range(6) if o not in have]
        if not any(r["trimmed"] for side in full["records"].values() for r in side if r["type"] == t):
            missing.append("%s trimmed" % TYPES[t])
    return missing


# -- the generator ---------------------------------------------------------------------------------------------------------------------------
CONTIGS = ["chr1", "chr2", "chrX"]
QUALS = ["0", "1023", "1024", "5000", "12.75", ".", "33.", "7", "18", "25", "40", "61", "300"]
HEADER_LINES = ["##fileformat=VCFv4.2", "##source=compare_cases", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE"]


def _bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(rng, base):
    return rng.choice([b for b in "ACGT" if b != base])


def _render(rng, ctg, pos, ref, alts, gt, qual, plain=False):
    """One VCF row; unless `plain`, in one of the spellings the rule reads alike."""
    sep = "/" if plain or rng.random() < 0.8 else "|"
    gt_text = sep.join(str(g) for g in gt)           # one index: haploid
    if not plain and rng.random() < 0.1:
        ref, alts = ref.lower(), [x.lower() for x in alts]
    fmt, sample = "GT", gt_text
    if not plain:
        form = rng.random()
        if form < 0.2:
            fmt, sample = "GT:GQ", gt_text + ":9"
        elif form < 0.3:
            fmt, sample = "GQ:DP:GT", "9:30:" + gt_text
    row = "\t".join([ctg, str(pos), ".", ref, ",".join(alts), qual, "PASS" if rng.random() < 0.5 else ".", ".", fmt, sample])
    if not plain and rng.random() < 0.1:
        row += "\t0/0"                   # a second sample: not read
    if not plain and rng.random() < 0.1:
        row += "\r"
    return row


def _pad(rng, pos, ref, alts):
    """The same alleles with a shared prefix or suffix: trimming undoes it."""
    k = rng.randint(1, 4)
    extra = _bases(rng, k)
    if rng.random() < 0.5 and pos > k:
        return pos - k, extra + ref, [extra + a for a in alts]
    return pos, ref + extra, [a + extra for a in alts]


def generate(seed, n_lines, break_order=True):
    """-> calls_text, truth_text, contigs, regions.  The calls have exactly n_lines lines.  break_order: the call rows are ordered by the
    POS they are written with, so a row padded in front can land before rows it follows once trimmed (the permutation path); otherwise by
    the trimmed position, which keeps the records in order."""
    rng = random.Random(seed)
    truth_rows, call_rows, regions = [], [], {}
    n_sites = max(n_lines, 1)
    for c, ctg in enumerate(CONTIGS):
        pos, bed, sites = 50, [], n_sites // 3 + 1
        for _ in range(sites):
            pos += rng.randint(4, 30)
            kind = rng.choice(("SNP", "SNP", "INS", "DEL", "MNP", "MULTI"))
            base = rng.choice("ACGT")
            if kind == "SNP":
                ref, alts = base, [_other(rng, base)]
            elif kind == "INS":
                ref, alts = base, [base + _bases(rng, rng.randint(1, 6))]
            elif kind == "DEL":
                ref, alts = base + _bases(rng, rng.randint(1, 6)), [base]
            elif kind == "MNP":
                ref = _bases(rng, rng.randint(2, 4))
                alts = ["".join(_other(rng, b) for b in ref)]
            else:
                ref, alts = base, [_other(rng, base), base + _bases(rng, rng.randint(1, 3))]
            gt = (1, 2) if kind == "MULTI" else rng.choice(((0, 1), (1, 1)))
            # the truth row, now and then padded or written twice
            t_pos, t_ref, t_alts = _pad(rng, pos, ref, alts) if rng.random() < 0.1 else (pos, ref, alts)
            if not break_order and any(trim(t_pos, t_ref, a)[0] != pos for a in t_alts):
                t_pos, t_ref, t_alts = pos, ref, alts
            truth_rows.append((c, pos, _render(rng, ctg, t_pos, t_ref, t_alts, gt, ".")))
            if rng.random() < 0.05:
                truth_rows.append((c, pos, _render(rng, ctg, pos, ref, alts, gt, ".")))
            if rng.random() < 0.03:
                truth_rows.append((c, pos, _render(rng, ctg, pos, base, [rng.choice(("<DEL>", "*", "."))], (0, 1), ".")))
            # the call derived from it
            op = rng.random()
            c_pos, c_ref, c_alts, c_gt, sort_pos = pos, ref, alts, gt, pos
            dropped = op < 0.08            # no call: the truth row is a FN
            if not dropped:
                if op < 0.18:
                    c_gt = (1, 1) if gt != (1, 1) else (0, 1)
                elif op < 0.24:
                    c_pos = sort_pos = pos + rng.randint(1, 3)
                elif op < 0.40:
                    c_pos, c_ref, c_alts = _pad(rng, pos, ref, alts)
                    if not break_order and any(trim(c_pos, c_ref, a)[0] != pos for a in c_alts):
                        c_pos, c_ref, c_alts = pos, ref, alts    # (an insertion that ends in its own first base comes back one base to the left)
                if rng.random() < 0.04 and c_gt == (1, 1):
                    c_gt = (1,)          # haploid: one copy
                call_rows.append((c, c_pos if break_order else sort_pos, _render(rng, ctg, c_pos, c_ref, c_alts, c_gt, rng.choice(QUALS))))
                if rng.random() < 0.05:              # the row once more, with another QUAL
                    call_rows.append((c, c_pos if break_order else sort_pos, _render(rng, ctg, c_pos, c_ref, c_alts, c_gt, rng.choice(QUALS))))
            if not dropped and rng.random() < 0.08:            # a false call next to it
                f_base = rng.choice("ACGT")
                f_kind = rng.choice(TYPES)
                f_ref, f_alt = {"SNP": (f_base, _other(rng, f_base)), "INS": (f_base, f_base + _bases(rng, 2)), "DEL": (f_base + _bases(rng, 2), f_base),
                                "MNP": ("AC", "GT")}[f_kind]
                call_rows.append((c, pos + 1, _render(rng, ctg, pos + 1, f_ref, [f_alt], (0, 1), rng.choice(QUALS))))
            if rng.random() < 0.02:
                odd = rng.choice(("<INS>", "*", "A,*"))       # the last: two ALTs, one record and one symbolic drop
                call_rows.append((c, pos, _render(rng, ctg, pos, base, odd.split(","), (1, 2) if "," in odd else (0, 1), "20")))
            if rng.random() < 0.02:
                call_rows.append((c, pos, _render(rng, ctg, pos, base, [_other(rng, base)], (0, 0), "3")))
            if rng.random() < 0.02:
                call_rows.append((c, pos, _render(rng, "chrUn_%d" % c, pos, base, [_other(rng, base)], (0, 1), "9")))
            # most sites lie in a confident interval
            if rng.random() < 0.85:
                bed.append((pos - rng.randint(1, 3), pos + rng.randint(0, 8)))
        regions[ctg] = bed
    call_rows.sort(key=lambda r: (r[0], r[1]))           # stable
    calls = [r[2] for r in call_rows]
    if n_lines >= 8:
        calls = HEADER_LINES + calls
        if len(calls) > 40:
            calls.insert(20, "")                         # an empty line is skipped
    calls = calls[:n_lines]
    calls += ["#filler"] * (n_lines - len(calls))
    truth = HEADER_LINES + [r[2] for r in truth_rows]
    return "".join(r + "\n" for r in calls), "".join(r + "\n" for r in truth), list(CONTIGS), regions


# -- crafted cases ---------------------------------------------------------------------------------------------------------------------------
def row(ctg, pos, ref, alt, gt="0/1", qual="."):
    return "\t".join([ctg, str(pos), ".", ref, alt, str(qual), ".", ".", "GT", gt]) + "\n"


def _unique_insert(i):
    """Insertion i of a family of distinct ones at one base: A plus i in base 4, five digits."""
    return "A" + "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(5))


def case(name, calls, truth, contigs=("chr1",), regions=None, expect=None):
    return dict(name=name, calls=calls, truth=truth, contigs=list(contigs), regions=regions, expect=expect)


def crafted():
    """-> the crafted cases.  `expect`, where given: {(side, type): {outcome: n}} for every non-zero cell, worked out by hand."""
    cases = []
    header = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    cases.append(case("empty", "", "", expect={}))
    cases.append(case("header_only", header, header, expect={}))
    cases.append(case("no_trailing_line_feed", header + row("chr1", 5, "A", "C")[:-1], row("chr1", 5, "A", "C", "1/1")[:-1],
                      expect={("calls", "SNP"): {"GT": 1}, ("truth", "SNP"): {"GT": 1}}))
    cases.append(case("calls_empty", "", row("chr1", 5, "A", "C") + row("chr1", 9, "AT", "A"),
                      expect={("truth", "SNP"): {"FN": 1}, ("truth", "DEL"): {"FN": 1}}))
    cases.append(case("truth_empty", row("chr1", 5, "A", "C") + row("chr1", 9, "A", "ATT"), header,
                      expect={("calls", "SNP"): {"FP": 1}, ("calls", "INS"): {"FP": 1}}))
    # a data line that begins before byte SCAN_BLOCK of the text and ends after it
    filler = "##" + "x" * (SCAN_BLOCK - 30) + "\n"
    straddle = filler + row("chr1", 100, "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", "A", "1/1", 50) + row("chr1", 200, "G", "T", "0/1", 60)
    assert len(filler) < SCAN_BLOCK < len(filler) + 60
    cases.append(case("line_straddles_scan_block", straddle, row("chr1", 100, "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", "A", "1/1") + row("chr1", 201, "G", "T"),
                      expect={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}, ("calls", "SNP"): {"FP": 1}, ("truth", "SNP"): {"FN": 1}}))
    # texts that end at, one byte before and one byte after the end of a scan block, the last line with and without its line feed: the entry
    # that closes the last line is then written by the first thread of a workgroup that has no text of its own
    for total, line_feed in ((SCAN_BLOCK, False), (SCAN_BLOCK, True), (SCAN_BLOCK - 1, False), (SCAN_BLOCK + 1, True)):
        data = row("chr1", 5, "A", "C", "0/1", 7)
        data = data if line_feed else data[:-1]
        text = "#" + "x" * (total - len(data) - 2) + "\n" + data
        assert len(text) == total
        cases.append(case("text_of_%d_bytes%s" % (total, "" if line_feed else "_no_line_feed"), text, text,
                          expect={("calls", "SNP"): {"TP": 1}, ("truth", "SNP"): {"TP": 1}}))
    # SCAN_BLOCK record slots exactly (two per line), the last of them kept
    half = SCAN_BLOCK // 2
    slots = "".join(row("chr1", 10 + i, "A", "C") for i in range(half - 1)) + row("chr1", 10 + half, "A", "C,G", "1/2")
    cases.append(case("slots_fill_scan_block", slots, slots, expect={("calls", "SNP"): {"TP": half + 1}, ("truth", "SNP"): {"TP": half + 1}}))
    # 300 distinct insertions at one position: the run of equal keys crosses a workgroup of the join, starts at record 0 and ends at n - 1;
    # the truth has every third of them, in another order
    n_run = JOIN_BLOCK + 44
    run_calls = "".join(row("chr1", 77, "A", _unique_insert(i), "0/1", i % 50) for i in range(n_run))
    run_truth = "".join(row("chr1", 77, "A", _unique_insert(i), "0/1" if i % 2 else "1/1") for i in reversed(range(0, n_run, 3)))
    cases.append(case("long_run", run_calls, run_truth,
                      expect={("calls", "INS"): {"TP": 50, "GT": 50, "FP": 200}, ("truth", "INS"): {"TP": 50, "GT": 50}}))
    # record 256 repeats record 255: its first copy is in the previous workgroup; record 257 repeats record 3
    dup_calls = "".join(row("chr1", 77, "A", _unique_insert(i)) for i in range(JOIN_BLOCK)) + row("chr1", 77, "a", _unique_insert(JOIN_BLOCK - 1).lower(), "1/1") \
        + row("chr1", 77, "A", _unique_insert(3))
    cases.append(case("duplicate_across_workgroups", dup_calls, row("chr1", 77, "A", _unique_insert(JOIN_BLOCK - 1)) + row("chr1", 77, "A", _unique_insert(3), "1/1"),
                      expect={("calls", "INS"): {"TP": 1, "GT": 1, "FP": JOIN_BLOCK - 2, "DUP": 2}, ("truth", "INS"): {"TP": 1, "GT": 1}}))
    # the contig changes between record 255 and record 256
    change = "".join(row("chr1", 10 + i, "A", "C") for i in range(JOIN_BLOCK)) + "".join(row("chr2", 10 + i, "A", "C") for i in range(5))
    cases.append(case("contig_change_at_block_boundary", change, row("chr1", 10 + JOIN_BLOCK - 1, "A", "C") + row("chr2", 10, "A", "C") + row("chr2", 10 + JOIN_BLOCK - 1, "A", "C"),
                      contigs=("chr1", "chr2"),
                      expect={("calls", "SNP"): {"TP": 2, "FP": JOIN_BLOCK + 3}, ("truth", "SNP"): {"TP": 2, "FN": 1}}))
    # touching, nested and separate intervals; positions at start, start + 1, end and end + 1 of their union (10, 30] and of (40, 50]
    bed = {"chr1": [(20, 30), (10, 20), (12, 15), (40, 50)], "chr2": [(0, 5)]}
    bed_calls = "".join(row("chr1", p, "A", "C") for p in (10, 11, 20, 21, 30, 31, 40, 41, 50, 51))
    cases.append(case("bed_edges", bed_calls, bed_calls, regions=bed, contigs=("chr1", "chr2"),
                      expect={("calls", "SNP"): {"TP": 6, "OUTSIDE": 4}, ("truth", "SNP"): {"TP": 6, "OUTSIDE": 4}}))
    # GATA -> GATC at 10 is A -> C at 13, behind the row at 11 that follows it: the records need the permutation
    moved = row("chr1", 10, "GATA", "GATC", "0/1", 30) + row("chr1", 11, "T", "G", "0/1", 20) + row("chr1", 13, "a", "c", "1/1", 10)
    cases.append(case("trimmed_pos_passes_successor", moved, row("chr1", 11, "T", "G") + row("chr1", 13, "A", "C"),
                      expect={("calls", "SNP"): {"TP": 2, "DUP": 1}, ("truth", "SNP"): {"TP": 2}}))
    # one of everything, worked by hand (docs/compare_vcf.md walks through it)
    mixed_calls = (header
                   + row("chr1", 10, "A", "G", "0/1", 30)             # TP
                   + row("chr1", 20, "AT", "A", "1/1", "12.75")       # the truth has one copy: GT
                   + row("chr1", 30, "C", "CGG,CT", "1|2", ".")       # CGG: FP; CT: the truth has two copies: GT
                   + row("chr1", 40, "G", "T", "1", 5000)             # FP, QUAL bin 1023
                   + row("chr1", 45, "G", "<DEL>", "0/1", 9)          # symbolic
                   + row("chr1", 58, "TCA", "TGA", "0/1", 1024)       # C -> G at 59: TP, bin 1023
                   + row("chr1", 70, "ACG", "TCA", "0/1", 8)          # MNP, TP
                   + row("chrUn", 5, "A", "C", "0/1", 8)              # unknown contig
                   + row("chr1", 90, "A", "C", "0/0", 8))             # no record
    mixed_truth = (row("chr1", 10, "A", "G") + row("chr1", 20, "AT", "A") + row("chr1", 30, "C", "CT", "1/1") + row("chr1", 50, "T", "C")
                   + row("chr1", 59, "C", "G") + row("chr1", 70, "ACG", "TCA") + row("chr1", 70, "acg", "tca", "1/1"))
    cases.append(case("mixed", mixed_calls, mixed_truth,
                      expect={("calls", "SNP"): {"TP": 2, "FP": 1}, ("calls", "INS"): {"GT": 1, "FP": 1}, ("calls", "DEL"): {"GT": 1}, ("calls", "MNP"): {"TP": 1},
                              ("truth", "SNP"): {"TP": 2, "FN": 1}, ("truth", "INS"): {"GT": 1}, ("truth", "DEL"): {"GT": 1}, ("truth", "MNP"): {"TP": 1, "DUP": 1}}))
    return cases


# the report of the case "mixed" at --min_qual 0, worked by hand: SNP  TP 2 (QUAL bins 30, 1023), FP 1 (bin 1023), truth 3 -> P 2/3, R 2/3, F1 4/6;
# INS  GT 1 + FP 1 count as two FP, truth 1; DEL  GT 1 counts as FP; MNP TP 1; ALL  TP 3, FP 4, FN 3 (truth 6) -> P 3/7, R 1/2, F1 6/13.
# Best cut-offs: no cut-off drops an SNP FP without a TP (both 1023-bin records stay to the end), so SNP stays at 0; for ALL, the GT and FP
# records below QUAL 8 (INS at "." = 0, both) go first: from q = 1 TP 3, FP 2 -> 6/11; from q = 9 the MNP TP (8) is lost: 4/10; at 13 the DEL GT
# (12) goes: TP 2, FP 1 -> 4/9; so the best is q = 1 with 6/11.
MIXED_REPORT = (
    "type\ttruth\tcalls\tTP\tFP\tFN\tGT\tprecision\trecall\tF1\tbest_qual\tbest_F1\n"
    "SNP\t3\t3\t2\t1\t1\t0\t0.666667\t0.666667\t0.666667\t0\t0.666667\n"
    "INS\t1\t2\t0\t2\t1\t1\t0.000000\t0.000000\t0.000000\t0\t0.000000\n"
    "DEL\t1\t1\t0\t1\t1\t1\t0.000000\t0.000000\t0.000000\t0\t0.000000\n"
    "INDEL\t2\t3\t0\t3\t2\t2\t0.000000\t0.000000\t0.000000\t0\t0.000000\n"
    "MNP\t1\t1\t1\t0\t0\t0\t1.000000\t1.000000\t1.000000\t0\t1.000000\n"
    "ALL\t6\t7\t3\t4\t3\t2\t0.428571\t0.500000\t0.461538\t1\t0.545455\n"
)

MALFORMED = (
    ("nine columns", "chr1\t5\t.\tA\tC\t.\t.\t.\tGT\n"),
    ("non-numeric POS", "chr1\t5x\t.\tA\tC\t.\t.\t.\tGT\t0/1\n"),
    ("1e3 as QUAL", "chr1\t5\t.\tA\tC\t1e3\t.\t.\tGT\t0/1\n"),
    ("FORMAT without GT", "chr1\t5\t.\tA\tC\t.\t.\t.\tGQ:DP\t3:4\n"),
    ("0/x", "chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/x\n"),
)
