"""compare_vcf --left_align's yardstick: the left-alignment loop of docs/compare_vcf.md ("Left alignment") restated literally in plain Python
on strings, applied after the trimming of tests/compare_cases.py and followed by that file's order, duplicate, region and join rules; a
seeded generator of call / truth pairs on genomes with planted tandem repeats, where one event is written at several equivalent positions;
and crafted cases with their expected results as literals worked out by hand.  tests/test_left_align.py holds the host twin against this,
tests/test_left_align_gpu.py the device against the twin.
"""
import random

import compare_cases as cc

LA_STATS = ("examined", "shifted", "ref_mismatch", "at_contig_start", "no_sequence", "sorted", "arena_bytes")


def left_align(G, pos, ref, alt):
    """The rule, literally.  G: the contig's sequence, upper-cased (compare_cases.up), or "" when none is loaded; pos, ref, alt: a trimmed
    record, the alleles upper-cased.  -> (what, pos, ref, alt) with what one of untouched, no_sequence, ref_mismatch, at_contig_start, aligned."""
    if len(ref) == len(alt):
        return "untouched", pos, ref, alt
    if G == "":
        return "no_sequence", pos, ref, alt
    if pos < 1 or pos - 1 + len(ref) > len(G) or G[pos - 1:pos - 1 + len(ref)] != ref:
        return "ref_mismatch", pos, ref, alt
    p, R, A = pos, ref, alt
    while True:
        changed = False
        if R and A and R[-1] == A[-1]:
            R, A, changed = R[:-1], A[:-1], True
        if not R or not A:
            if p == 1:
                return "at_contig_start", pos, ref, alt
            p -= 1
            R, A, changed = G[p - 1] + R, G[p - 1] + A, True
        if not changed:
            break
    while len(R) > 1 and len(A) > 1 and R[0] == A[0]:
        R, A, p = R[1:], A[1:], p + 1
    return "aligned", p, R, A


def haplotype(G, pos, ref, alt):
    """G upper-cased, as left_align takes it."""
    return G[:pos - 1] + alt + G[pos - 1 + len(ref):]


def align_side(text, contigs, reference, side):
    """-> the side's records in file order after the pass (the dicts of compare_cases.parse_side, with pos, ref, alt, ref_off and alt_off those
    after the pass, plus `what`, `pos_before`, `ref_before`, `alt_before`), the parse statistics, the pass's statistics and the arena (str)."""
    records, st = cc.parse_side(text, contigs, side)
    keys = [(r["ctg"], r["pos"]) for r in records]
    st["sorted"] = int(all(a <= b for a, b in zip(keys, keys[1:])))
    la = dict.fromkeys(LA_STATS, 0)
    arena, upper = [], dict((c, cc.up(s)) for c, s in reference.items())
    for r in records:
        what, pos, ref, alt = left_align(upper.get(contigs[r["ctg"]], ""), r["pos"], r["ref"], r["alt"])
        assert (len(ref), len(alt)) == (r["ref_len"], r["alt_len"])         # the slots are laid out on the lengths before the pass
        r.update(what=what, pos_before=r["pos"], ref_before=r["ref"], alt_before=r["alt"])
        la["examined"] += what != "untouched"
        la["shifted"] += pos != r["pos"]
        for k in ("ref_mismatch", "at_contig_start", "no_sequence"):
            la[k] += what == k
        r.update(pos=pos, ref=ref, alt=alt, ref_off=la["arena_bytes"], alt_off=la["arena_bytes"] + len(ref))
        la["arena_bytes"] += len(ref) + len(alt)
        arena.append(ref + alt)
    keys = [(r["ctg"], r["pos"]) for r in records]
    la["sorted"] = int(all(a <= b for a, b in zip(keys, keys[1:])))
    return records, st, la, "".join(arena)


def restate_full(calls_text, truth_text, contigs, regions, reference):
    """compare_cases.restate_full with the pass between trimming and order.  reference: {contig: sequence}.  -> that function's dict, plus
    left_align[side] (LA_STATS) and alleles[side] (the arena as str); `permuted` of a side is 1 - left_align[side]["sorted"]."""
    sides, stats, outcomes, la, alleles = {}, {}, {}, {}, {}
    for side, text in (("calls", calls_text), ("truth", truth_text)):
        records, stats[side], la[side], alleles[side] = align_side(text, contigs, reference, side)
        order = sorted(range(len(records)), key=lambda i: ((records[i]["ctg"], records[i]["pos"]), i))
        sides[side] = [records[i] for i in order]
        seen, out = set(), []
        for r in sides[side]:
            allele = (r["ctg"], r["pos"], r["ref"], r["alt"])
            out.append(cc.DUP if allele in seen else None if cc.inside(regions, contigs[r["ctg"]], r["pos"]) else cc.OUTSIDE)
            seen.add(allele)
        outcomes[side] = out
    truth_at = {}
    for j, r in enumerate(sides["truth"]):
        if outcomes["truth"][j] != cc.DUP:
            truth_at[(r["ctg"], r["pos"], r["ref"], r["alt"])] = j
    for i, r in enumerate(sides["calls"]):
        if outcomes["calls"][i] is None:
            j = truth_at.get((r["ctg"], r["pos"], r["ref"], r["alt"]))
            if j is None:
                outcomes["calls"][i] = cc.FP
            else:
                outcomes["calls"][i] = outcomes["truth"][j] = cc.TP if sides["truth"][j]["copies"] == r["copies"] else cc.GT
    outcomes["truth"] = [cc.FN if o is None else o for o in outcomes["truth"]]
    counts = [0] * cc.N_COUNTS
    for k, side in enumerate(("calls", "truth")):
        for r, o in zip(sides[side], outcomes[side]):
            counts[cc.AT_COUNTS + (k * 4 + r["type"]) * 6 + o] += 1
            if side == "calls" and o in (cc.TP, cc.GT, cc.FP):
                counts[cc.AT_HIST + (r["type"] * 3 + o) * cc.QUAL_BINS + r["qual_bin"]] += 1
        for d, name in enumerate(("symbolic", "unknown_contig", "too_long")):
            counts[cc.AT_DROPS + k * 3 + d] = stats[side][name]
    for row in range(12):
        at_least = 0
        for q in reversed(range(cc.QUAL_BINS)):
            at_least += counts[cc.AT_HIST + row * cc.QUAL_BINS + q]
            counts[cc.AT_AT_LEAST + row * cc.QUAL_BINS + q] = at_least
    return dict(counts=counts, stats=stats, records=sides, outcomes=outcomes, left_align=la, alleles=alleles)


def richness(full):
    """What a generated pair must hold, by the restatement's own count: every class of the pass on some side, and for insertions and for
    deletions every outcome on some side and a record the pass moved.  -> the list of what is missing."""
    missing = [k for k in ("shifted", "ref_mismatch", "at_contig_start", "no_sequence") if not any(full["left_align"][s][k] for s in ("calls", "truth"))]
    everything = [(r, o) for side in ("calls", "truth") for r, o in zip(full["records"][side], full["outcomes"][side])]
    if not any(r["what"] == "aligned" and r["pos"] == r["pos_before"] for r, _ in everything):
        missing.append("unshifted")
    if not any(r["what"] == "untouched" for r, _ in everything):
        missing.append("untouched")
    for t in (1, 2):
        have = set(o for r, o in everything if r["type"] == t)
        missing += ["%s %s" % (cc.TYPES[t], cc.OUTCOMES[o]) for o in range(6) if o not in have]
        if not any(r["type"] == t and r["pos"] != r["pos_before"] for r, _ in everything):
            missing.append("%s shifted" % cc.TYPES[t])
    return missing


# -- the generator ---------------------------------------------------------------------------------------------------------------------------
CONTIGS = ["ctgA", "ctgB", "ctgNoSeq"]             # the last has no sequence in the reference
ALPHABETS = ("AC", "ACG", "ACGT", "AN")


def _seq(rng, alphabet, n):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _write_event(rng, G, s, unit, copies, kind, m, t, behind=None):
    """The event `m` units of the repeat (starting at 1-based s, `copies` of `unit`) inserted or deleted, written at phase t inside the repeat:
    all phases are one haplotype.  -> pos, ref, alt.  behind: the form whose alleles end, not begin, with the shared base; None: now and then."""
    u = len(unit)
    first = s + t                                  # the first base deleted, or the base the insertion goes in front of
    event = "".join(unit[(t + k) % u] for k in range(m * u))
    if (rng.random() < 0.25 if behind is None else behind) and (kind == "INS" or first + m * u <= len(G)) and first <= len(G):
        after = G[first - 1 + (m * u if kind == "DEL" else 0)]           # the base behind the event
        return (first, after, event + after) if kind == "INS" else (first, event + after, after)
    before = G[first - 2]
    return (first - 1, before, before + event) if kind == "INS" else (first - 1, before + event, before)


def generate(seed, n_lines, break_order=True):
    """-> calls_text, truth_text, contigs, regions, reference.  About n_lines lines per side.  break_order False: the rows of a side are in
    the order of their left-aligned positions, so the records are in order after the pass; True: in the order of the positions written."""
    rng = random.Random(seed)
    reference, rows, regions = {}, {"calls": [], "truth": []}, {}
    per_contig = max(n_lines // 3, 1)
    for c, ctg in enumerate(CONTIGS):
        alphabet = ALPHABETS[(seed + c) % len(ALPHABETS)]
        G, sites, bed = "", [], []
        for k in range(per_contig):
            if k > 0 or rng.random() < 0.5:        # half of the contigs begin with a repeat: an event in it meets the contig's start
                G += _seq(rng, alphabet, rng.randint(2, 9))
            big = rng.random() < 0.02
            unit = _seq(rng, alphabet, rng.choice((63, 64, 65))) if big else _seq(rng, alphabet, rng.randint(1, 4))
            copies = rng.randint(2, 4) if big else rng.randint(2, 9)
            sites.append((len(G) + 1, unit, copies))
            G += unit * copies
        G += _seq(rng, alphabet, 6)
        if rng.random() < 0.3:
            G = G.lower() if rng.random() < 0.5 else "".join(b.lower() if rng.random() < 0.3 else b for b in G)
        if ctg != "ctgNoSeq":
            reference[ctg] = G
        U = cc.up(G)
        for s, unit, copies in sites:
            u = len(unit)
            kind = rng.choice(("INS", "DEL", "DEL", "SNP"))
            if kind == "SNP":
                base = U[s - 1]
                written = [(s, base, cc._other(rng, base))] * 2
            else:
                m = rng.randint(1, min(2, copies - 1))
                room = (copies - m) * u if kind == "DEL" else copies * u
                lo = 1 if s == 1 else 0            # nothing is written at position 0
                written = [_write_event(rng, U, s, unit, copies, kind, m, rng.randint(lo, room)) for _ in range(2)]
            gt = rng.choice(((0, 1), (1, 1)))
            damage = rng.random()
            for side, (pos, ref, alt) in zip(("truth", "calls"), written):
                side_gt, qual = gt, "." if side == "truth" else rng.choice(cc.QUALS)
                if (side == "calls" and damage < 0.08) or (side == "truth" and 0.08 <= damage < 0.14):
                    continue                       # no call: FN; no truth: FP
                if side == "calls" and 0.14 <= damage < 0.22:
                    side_gt = (1, 1) if gt != (1, 1) else (0, 1)
                if damage > 0.97 and kind != "SNP" and len(ref) > 1:
                    ref = ref[:-1] + cc._other(rng, ref[-1])                     # REF is not the reference, on both sides
                if rng.random() < 0.1:
                    ref, alt = ref.lower(), alt.lower()
                rows[side].append((c, pos if break_order else _final_pos(U if ctg in reference else "", pos, ref, alt), cc._render(rng, ctg, pos, ref, [alt], side_gt, qual, plain=True)))
                if rng.random() < 0.04 and kind != "SNP":                      # the event once more at another phase: a duplicate after the pass
                    pos2, ref2, alt2 = _write_event(rng, U, s, unit, copies, kind, m, rng.randint(lo, room))
                    rows[side].append((c, pos2 if break_order else _final_pos(U if ctg in reference else "", pos2, ref2, alt2), cc._render(rng, ctg, pos2, ref2, [alt2], side_gt, qual, plain=True)))
            if rng.random() < 0.85:
                bed.append((max(s - 8, 0), s + 1))
        regions[ctg] = bed
    texts = {}
    for side in ("calls", "truth"):
        rows[side].sort(key=lambda r: (r[0], r[1]))          # stable
        texts[side] = "".join(line + "\n" for line in cc.HEADER_LINES + [r[2] for r in rows[side]])
    return texts["calls"], texts["truth"], list(CONTIGS), regions, reference


def _final_pos(G, pos, ref, alt):
    """Where the row's record stands after trimming and the pass."""
    r, a = cc.up(ref), cc.up(alt)
    pos, front, back = cc.trim(pos, ref, alt)
    return left_align(G, pos, r[front:len(r) - back], a[front:len(a) - back])[1]


# -- crafted cases ---------------------------------------------------------------------------------------------------------------------------
def case(name, calls, truth, reference, contigs=("chr1",), regions=None, **expect):
    return dict(name=name, calls=calls, truth=truth, contigs=list(contigs), regions=regions, reference=reference, expect=expect)


def crafted():
    """-> the crafted cases.  expect, all worked by hand: `cells` {(side, type): {outcome: n}} for every non-zero cell, as compare_cases has it;
    `calls_records` / `truth_records` the (pos, REF, ALT) of the side's records in their final order; `la` {side: {stat: n}} for the stats named;
    `without` the cells without the pass; `permuted` {side: 0 / 1}."""
    row, cases = cc.row, []
    #            1234567890123
    homo = {"chr1": "GCAAAAATCGGTA"}                 # A at 3 .. 7
    # the deletion of one A: the call deletes the last (anchor A6, REF AA at 6), the truth the first (anchor C2, REF CA at 2)
    cases.append(case("homopolymer_deletion_right_against_left", row("chr1", 6, "AA", "A", "0/1", 30), row("chr1", 2, "CA", "C"), homo,
                      cells={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}}, calls_records=[(2, "CA", "C")], truth_records=[(2, "CA", "C")],
                      la={"calls": dict(examined=1, shifted=1, sorted=1, arena_bytes=3), "truth": dict(examined=1, shifted=0)},
                      without={("calls", "DEL"): {"FP": 1}, ("truth", "DEL"): {"FN": 1}}))
    #           123456789012
    di = {"chr1": "TTGACACACGTT"}                    # AC at 4 .. 9, G3 before it
    # the insertion of one AC unit: the truth behind G3, the call one unit to the right (behind C5); and written out of phase, CA behind A6
    cases.append(case("dinucleotide_insertion_one_unit_right", row("chr1", 5, "C", "CAC", "1/1", 9) + row("chr1", 6, "A", "ACA", "1/1", 8), row("chr1", 3, "G", "GAC", "1/1"), di,
                      cells={("calls", "INS"): {"TP": 1, "DUP": 1}, ("truth", "INS"): {"TP": 1}}, calls_records=[(3, "G", "GAC"), (3, "G", "GAC")], truth_records=[(3, "G", "GAC")],
                      la={"calls": dict(examined=2, shifted=2), "truth": dict(examined=1, shifted=0)},
                      without={("calls", "INS"): {"FP": 2}, ("truth", "INS"): {"FN": 1}}))
    #            12345678
    last = {"chr1": "TTCGATTT"}
    # REF=A ALT=GCA at 5: GC goes in before A5; the last bytes agree, so the loop drops them, takes G4 in front: G -> GGC at 4; G4 == C? no: it
    # stops there: (4, G, GGC).  The truth writes that.
    cases.append(case("last_bytes_agree", row("chr1", 5, "A", "GCA"), row("chr1", 4, "G", "GGC"), last,
                      cells={("calls", "INS"): {"TP": 1}, ("truth", "INS"): {"TP": 1}}, calls_records=[(4, "G", "GGC")], truth_records=[(4, "G", "GGC")],
                      la={"calls": dict(examined=1, shifted=1), "truth": dict(examined=1, shifted=0)}))
    # a complex record: neither first nor last bytes agree and both alleles keep more than the event: it must not move, though it lies in a run
    cases.append(case("complex_stays", row("chr1", 4, "AAA", "CT"), row("chr1", 4, "AAA", "CT"), homo,
                      cells={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}}, calls_records=[(4, "AAA", "CT")], truth_records=[(4, "AAA", "CT")],
                      la={"calls": dict(examined=1, shifted=0, ref_mismatch=0), "truth": dict(examined=1, shifted=0)}))
    #             1234567
    start = {"chr1": "GAAAACT"}                      # A at 2 .. 5, G1 before it
    # the deletion of the last A (anchor A4) moves to the anchor G1: it ends exactly at position 1
    cases.append(case("shift_ends_at_position_1", row("chr1", 4, "AA", "A"), row("chr1", 1, "GA", "G"), start,
                      cells={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}}, calls_records=[(1, "GA", "G")], truth_records=[(1, "GA", "G")],
                      la={"calls": dict(examined=1, shifted=1, at_contig_start=0), "truth": dict(examined=1, shifted=0, at_contig_start=0)}))
    #             123456
    edge = {"chr1": "AAAACT"}                        # the run begins the contig: no base is left of it
    # the deletion of one A (anchor A3): the run goes on to position 1 and past it; the record stays exactly as written, upper-cased
    cases.append(case("would_pass_position_1", row("chr1", 3, "aa", "a") + row("chr1", 5, "C", "CC"), row("chr1", 2, "AA", "A"), edge,
                      cells={("calls", "DEL"): {"FP": 1}, ("truth", "DEL"): {"FN": 1}, ("calls", "INS"): {"FP": 1}}, calls_records=[(3, "AA", "A"), (4, "A", "AC")], truth_records=[(2, "AA", "A")],
                      la={"calls": dict(examined=2, shifted=1, at_contig_start=1), "truth": dict(examined=1, shifted=0, at_contig_start=1)}))
    # 1/2: two records that share the row's REF text; AAA -> AA is A -> (nothing) at the run's left end, AAA -> A two of them
    cases.append(case("two_alts_share_ref", row("chr1", 5, "AAA", "AA,A", "1/2", 20), row("chr1", 2, "CA", "C") + row("chr1", 2, "CAA", "C"), homo,
                      cells={("calls", "DEL"): {"TP": 2}, ("truth", "DEL"): {"TP": 2}}, calls_records=[(2, "CA", "C"), (2, "CAA", "C")], truth_records=[(2, "CA", "C"), (2, "CAA", "C")],
                      la={"calls": dict(examined=2, shifted=2, arena_bytes=7), "truth": dict(examined=2, shifted=0)}))
    # two placements of one event on one side: a duplicate once aligned
    cases.append(case("shift_creates_duplicate", row("chr1", 2, "CA", "C", "0/1", 5) + row("chr1", 5, "AA", "A", "0/1", 50), row("chr1", 4, "AA", "A"), homo,
                      cells={("calls", "DEL"): {"TP": 1, "DUP": 1}, ("truth", "DEL"): {"TP": 1}}, calls_records=[(2, "CA", "C"), (2, "CA", "C")], truth_records=[(2, "CA", "C")],
                      la={"calls": dict(examined=2, shifted=1), "truth": dict(examined=1, shifted=1)}))
    # C2 -> T at 2 ... wait: an SNP at 4 stands before the deletion at 6, which moves to 2: the order breaks
    cases.append(case("shift_breaks_order", row("chr1", 4, "A", "T") + row("chr1", 6, "AA", "A"), row("chr1", 2, "CA", "C") + row("chr1", 4, "A", "T"), homo,
                      cells={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}, ("calls", "SNP"): {"TP": 1}, ("truth", "SNP"): {"TP": 1}},
                      calls_records=[(2, "CA", "C"), (4, "A", "T")], truth_records=[(2, "CA", "C"), (4, "A", "T")], permuted={"calls": 1, "truth": 0},
                      la={"calls": dict(examined=1, shifted=1, sorted=0), "truth": dict(examined=1, shifted=0, sorted=1)}))
    # the interval (1, 2] holds position 2 alone.  The deletion at 6 moves into it; on a second contig with the same bases and the interval (5, 6]
    # it moves out of it
    both = {"chr1": homo["chr1"], "chr2": homo["chr1"]}
    cases.append(case("shift_crosses_bed", row("chr1", 6, "AA", "A") + row("chr2", 6, "AA", "A"), row("chr1", 2, "CA", "C") + row("chr2", 2, "CA", "C"), both,
                      contigs=("chr1", "chr2"), regions={"chr1": [(1, 2)], "chr2": [(5, 6)]},
                      cells={("calls", "DEL"): {"TP": 1, "OUTSIDE": 1}, ("truth", "DEL"): {"TP": 1, "OUTSIDE": 1}},
                      calls_records=[(2, "CA", "C"), (2, "CA", "C")], truth_records=[(2, "CA", "C"), (2, "CA", "C")],
                      la={"calls": dict(examined=2, shifted=2), "truth": dict(examined=2, shifted=0)},
                      without={("calls", "DEL"): {"FP": 1, "OUTSIDE": 1}, ("truth", "DEL"): {"TP": 0, "FN": 1, "OUTSIDE": 1}}))
    # lower case in the reference and in the alleles
    cases.append(case("lower_case", row("chr1", 6, "aa", "a"), row("chr1", 3, "Aa", "a"), {"chr1": "gcAaaAatcggta"},
                      cells={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}}, calls_records=[(2, "CA", "C")], truth_records=[(2, "CA", "C")],
                      la={"calls": dict(examined=1, shifted=1), "truth": dict(examined=1, shifted=1)}))
    # REF is not what the reference has at 6 (AA): the record stays, is counted, and still takes part in the join
    cases.append(case("ref_mismatch", row("chr1", 6, "AT", "A"), row("chr1", 6, "AT", "A") + row("chr1", 2, "CA", "C"), homo,
                      cells={("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1, "FN": 1}}, calls_records=[(6, "AT", "A")], truth_records=[(2, "CA", "C"), (6, "AT", "A")],
                      la={"calls": dict(examined=1, shifted=0, ref_mismatch=1), "truth": dict(examined=2, shifted=0, ref_mismatch=1, sorted=0)}, permuted={"calls": 0, "truth": 1}))
    # a deletion that runs past the contig's end (13 bases): TAC at 12 needs a base 14
    cases.append(case("deletion_past_contig_end", row("chr1", 12, "TAC", "T"), row("chr1", 12, "TA", "T"), homo,
                      cells={("calls", "DEL"): {"FP": 1}, ("truth", "DEL"): {"FN": 1}}, calls_records=[(12, "TAC", "T")], truth_records=[(12, "TA", "T")],
                      la={"calls": dict(examined=1, shifted=0, ref_mismatch=1), "truth": dict(examined=1, shifted=0, ref_mismatch=0)}))
    # chr2 has no sequence: its indels stay and are counted, its SNP is not examined
    cases.append(case("contig_without_sequence", row("chr1", 6, "AA", "A") + row("chr2", 6, "AA", "A") + row("chr2", 9, "C", "T"), row("chr1", 2, "CA", "C") + row("chr2", 2, "CA", "C"), homo,
                      contigs=("chr1", "chr2"),
                      cells={("calls", "DEL"): {"TP": 1, "FP": 1}, ("truth", "DEL"): {"TP": 1, "FN": 1}, ("calls", "SNP"): {"FP": 1}},
                      calls_records=[(2, "CA", "C"), (6, "AA", "A"), (9, "C", "T")], truth_records=[(2, "CA", "C"), (2, "CA", "C")],
                      la={"calls": dict(examined=2, shifted=1, no_sequence=1), "truth": dict(examined=2, shifted=0, no_sequence=1)}))
    return cases


# -- the shapes at which the wave-parallel search can go wrong (tests/test_left_align_gpu.py; the host twin takes them on the CPU too) -------------
SHIFTS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 200)
LENGTHS = (1, 2, 3, 63, 64, 65, 130)


def _unit(L, salt):
    """L bases without a T: one G, then A / C by the bits of salt."""
    return "G" + "".join("AC"[(salt >> (k % 7)) & 1] for k in range(L - 1))


def shift_grid(lengths=LENGTHS, shifts=SHIFTS):
    """Per (L, k), four blocks of one contig, each a run of period L behind a T (no unit holds a T, so every search stops at that T):
    a deletion of the run's last L bases, where the run has k + L bases, and an insertion of the period's next L bases behind a run of k
    bases -- either moves exactly k to the left -- each written once with the shared base in front (where the base before the event equals
    the event's last one, for k > 0, that is the form that ends with the shared base one position to the left: k - 1 steps) and once with
    the shared base behind.  The truth holds every event left-aligned, worked out here from the block's layout: anchor = the T.
    -> calls, truth, contigs, reference, how many call records move."""
    G, calls, truth, n_moved = "T", [], [], 0
    for L in lengths:
        for k in shifts:
            period = _unit(L, 5 * L + k) * (k // L + 3)
            for kind in ("INS", "DEL"):
                for form in ("front", "behind"):
                    n_run = k + L if kind == "DEL" else k
                    start = len(G) + 1                     # the run's first base; G[start - 1] is the T
                    G += period[:n_run] + "T"
                    end = start + n_run - 1
                    if kind == "DEL":
                        event = period[k:k + L]            # = G[end - L + 1 .. end]
                        written = (end - L, G[end - L - 1] + event, G[end - L - 1]) if form == "front" else (end - L + 1, event + "T", "T")
                        want = (start - 1, "T" + period[:L], "T")
                    else:
                        event = period[k:k + L]            # what the period goes on with
                        written = (end, G[end - 1], G[end - 1] + event) if form == "front" else (end + 1, "T", event + "T")
                        want = (start - 1, "T", "T" + period[:L])
                    calls.append(cc.row("chr1", written[0], written[1], written[2], "0/1", 10))
                    truth.append(cc.row("chr1", want[0], want[1], want[2]))
                    n_moved += want[0] != written[0]
    return "".join(calls), "".join(truth), ["chr1"], {"chr1": G}, n_moved


def big_event(L=5000):
    """An event of L bases in a run of two copies of its unit, deleted at the right and inserted behind the run: both move L to the left."""
    unit = _unit(L, 11)
    G = "CT" + unit * 2 + "TG"
    calls = cc.row("chr1", 2 + L, unit[-1] + unit, unit[-1], "1/1", 40) + cc.row("chr1", 2 + 2 * L, unit[-1], unit[-1] + unit, "0/1", 30)
    truth = cc.row("chr1", 2, "T" + unit, "T", "1/1") + cc.row("chr1", 2, "T", "T" + unit)
    return dict(name="big_event_%d" % L, calls=calls, truth=truth, contigs=["chr1"], regions=None, reference={"chr1": G})


def contig_boundaries():
    """Runs that begin exactly at a contig's first base (the event cannot be left-aligned: at_contig_start) and one base behind it (the shift
    ends at position 1), on the first contig and on later ones.  Every contig's tail is the repeat the next one begins with, so a search that
    read across the boundary would go on; the runs are longer than two rounds of 64 steps.  The truth holds what is right, worked by hand."""
    reference = {"c1": "A" * 150, "c2": "A" * 150 + "CG" + "AAAA", "c3": "G" + "A" * 150 + "TTACAC", "c4": "AC" * 80 + "GTAC", "c5": "T" + "AC" * 80}
    calls = (cc.row("c1", 140, "AA", "A") + cc.row("c1", 150, "A", "AAA")                     # both at_contig_start on the first contig
             + cc.row("c2", 149, "AA", "A") + cc.row("c2", 150, "A", "AA")                    # the same where a contig lies in front
             + cc.row("c3", 150, "AA", "A") + cc.row("c3", 151, "A", "AA")                    # one base short of the start: both end at position 1
             + cc.row("c4", 157, "ACA", "A") + cc.row("c4", 160, "C", "CAC")                  # a two-base unit, at_contig_start
             + cc.row("c5", 159, "CAC", "C") + cc.row("c5", 161, "C", "CAC"))                 # and one base short of it
    truth = (cc.row("c1", 140, "AA", "A") + cc.row("c1", 150, "A", "AAA") + cc.row("c2", 149, "AA", "A") + cc.row("c2", 150, "A", "AA")
             + cc.row("c3", 1, "GA", "G") + cc.row("c3", 1, "G", "GA") + cc.row("c4", 157, "ACA", "A") + cc.row("c4", 160, "C", "CAC")
             + cc.row("c5", 1, "TAC", "T") + cc.row("c5", 1, "T", "TAC"))
    return dict(name="contig_boundaries", calls=calls, truth=truth, contigs=["c1", "c2", "c3", "c4", "c5"], regions=None, reference=reference)


def record_count(n, indels="some"):
    """Exactly n records per side, one per row, on a contig of n blocks `T AAAAA CG`: the calls delete an A at the right end of the run or
    change the C, the truth has the deletion at the left end.  indels: "some" (two rows in three), "none" or "all" of the calls."""
    G = "TAAAAACG" * n
    calls, truth = [], []
    for i in range(n):
        at = 8 * i                                 # the block's T is at at + 1, its A at at + 2 .. at + 6, its C at at + 7
        if indels == "all" or (indels == "some" and i % 3 != 0):
            calls.append(cc.row("chr1", at + 5, "AA", "A", "0/1", i % 60))
            truth.append(cc.row("chr1", at + 1, "TA", "T", "0/1" if i % 5 else "1/1"))
        else:
            calls.append(cc.row("chr1", at + 7, "C", "G", "0/1", i % 60))
            truth.append(cc.row("chr1", at + 7, "C", "G" if i % 7 else "T"))
    return dict(name="records_%d_%s" % (n, indels), calls="".join(calls), truth="".join(truth), contigs=["chr1"], regions=None, reference={"chr1": G})
