"""What tests/test_markdup_bam.py and tests/test_markdup_bam_gpu.py share (test support, not a test): the shuffled fixture with every clause
of docs/markdup_bam.md in it, the yardstick -- the rule restated in plain Python over bam_fixture.Record objects, with dictionaries keyed by
the real read names and by tuples, no hashes and no sorts of keys, sharing no code with the twin or the device --, the summaries and the
file the rule implies, and the synthetic summaries of the resolution tests."""
import random
import re

import numpy as np

from bam_fixture import Bam, ref_span
from sort_bam_cases import inflated, read_bgzf  # noqa: F401  (the tests read files through them)

REFS = [("chr1", 5000000), ("chr2", 300000)]
WAYS = {"straddle": dict(block=300), "whole": dict(block=65280), "per_record": dict(per_record=True)}
PAYLOAD = 65280
MIN_QUALITY = 15
SCORE_MAX = 0xffffffff
TINY = 2100                                       # fragments on one end: more than a radix tile of 2048


def row(name, flag, ref, pos1, cigar, quals, rnext="*", pnext=0):
    """One SAM line; quals: one quality for every base, a list of them, or None (absent)."""
    n = sum(int(a) for a, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X") if cigar != "*" else 30
    if isinstance(quals, int):
        quals = [quals] * n
    qual = "*" if quals is None else "".join(chr(q + 33) for q in quals)
    assert quals is None or len(quals) == n
    return "\t".join([name, str(flag), ref, str(pos1), "60", cigar, rnext, str(pnext), "0", "A" * n, qual])


def pair(name, ref1, pos1, cigar1, q1, rev1, ref2, pos2, cigar2, q2, rev2, swap=False):
    """Two lines: read 1 and read 2 of one name (swap: the first of them is read 2)"""
    n1, n2 = (0x80, 0x40) if swap else (0x40, 0x80)
    return [row(name, 1 | n1 | (16 if rev1 else 0) | (32 if rev2 else 0), ref1, pos1, cigar1, q1, "=" if ref1 == ref2 else ref2, pos2),
            row(name, 1 | n2 | (16 if rev2 else 0) | (32 if rev1 else 0), ref2, pos2, cigar2, q2, "=" if ref1 == ref2 else ref1, pos1)]


def sam_text(seed=7):
    rng = random.Random(seed)
    rows = []
    # forward fragments on one unclipped end through S and H clips, and two clipped to a negative position
    rows += [row("fwd_plain", 0, "chr1", 1000, "50M", 30), row("fwd_soft", 0, "chr1", 1005, "5S45M", 20), row("fwd_hard_soft", 0, "chr1", 1010, "3H7S40M", 40)]
    rows += [row("negative_a", 0, "chr1", 3, "10S40M", 25), row("negative_b", 0, "chr1", 1, "8S42M", 35)]
    # reverse fragments on one unclipped end with different positions (and one four bases further)
    rows += [row("rev_plain", 16, "chr1", 2000, "50M", 30), row("rev_short", 16, "chr1", 2010, "40M", 33), row("rev_soft", 16, "chr1", 2005, "40M5S", 31),
             row("rev_other_end", 16, "chr1", 2000, "30M10D10M4H", 39)]
    # pairs of one signature in every orientation, three each; FR once more with the read numbers the other way round
    for k, (tag, rev1, rev2) in enumerate([("FR", False, True), ("RF", True, False), ("FF", False, False), ("RR", True, True)]):
        at = 10000 * (k + 1)
        for j, (q1, q2) in enumerate([(20, 25), (30, 35), (22, 22)]):
            c1, p1 = ("50M", at) if j != 1 or rev1 else ("4S46M", at + 4)
            rows += pair("pair%s_%d" % (tag, j), "chr1", p1, c1, q1, rev1, "chr1", at + 200, "50M", q2, rev2)
    rows += pair("pairFR_swapped", "chr1", 10000, "50M", 38, False, "chr1", 10200, "50M", 38, True, swap=True)
    # mates on two references
    rows += pair("two_refs_a", "chr1", 50000, "50M", 20, False, "chr2", 1000, "50M", 20, True)
    rows += pair("two_refs_b", "chr1", 50000, "50M", 21, False, "chr2", 1000, "50M", 21, True)
    # ties the input index breaks: two fragments, and two pairs of one signature whose scores add up to the same
    rows += [row("tie_frag_a", 0, "chr1", 60000, "50M", 30), row("tie_frag_b", 0, "chr1", 60000, "50M", 30)]
    rows += pair("tie_pair_a", "chr1", 61000, "50M", 30, False, "chr1", 61300, "50M", 20, True)
    rows += pair("tie_pair_b", "chr1", 61000, "50M", 20, False, "chr1", 61300, "50M", 30, True)
    # a fragment at the end of paired records, however good
    rows.append(row("frag_at_pair_end", 0, "chr1", 10000, "50M", 60))
    # flag 8: the mate is unmapped, so these are fragments; their mates are placed and not examined
    for k, q in enumerate((30, 31)):
        rows.append(row("mate_unmapped_%d" % k, 1 | 8 | 0x40, "chr1", 70000, "50M", q, "=", 70000))
        rows.append(row("mate_unmapped_%d" % k, 1 | 4 | 0x80 | 0x400, "chr1", 70000, "*", 10, "=", 70000))
    # a paired record whose mate is not in the file; several records of one name and read number
    rows.append(row("mate_missing", 1 | 0x40, "chr1", 71000, "50M", 30, "=", 71300))
    for k in range(3):
        rows.append(row("multi", 1 | 0x40, "chr1", 72000 + 10 * k, "50M", 30, "=", 72300))
    for k in range(2):
        rows.append(row("multi", 1 | 0x80 | 16, "chr1", 72300 + 10 * k, "50M", 30, "=", 72000))
    rows.append(row("both_numbers", 1 | 0xc0, "chr1", 73000, "50M", 30, "=", 73300))       # neither read 1 nor read 2: a fragment
    # secondary and supplementary copies with a stale 0x400; examined records with a stale 0x400, one to clear and one to keep
    rows += [row("fwd_plain", 0x100 | 0x400, "chr1", 1000, "50M", 30), row("fwd_plain", 0x800 | 0x400, "chr1", 1000, "20M30H", 30), row("fwd_soft", 0x800, "chr1", 1005, "45M", 9)]
    rows += [row("stale_cleared", 0x400, "chr1", 80000, "50M", 30), row("stale_kept_a", 0x400, "chr1", 81000, "50M", 10), row("stale_kept_b", 0, "chr1", 81000, "50M", 40)]
    # unplaced reads
    rows += [row("nowhere%02d" % k, rng.choice([4, 4 | 0x400, 77, 141]), "*", 0, "*", 12) for k in range(15)]
    # absent qualities, and qualities around 15
    rows += [row("absent_a", 0, "chr1", 82000, "50M", None), row("absent_b", 0, "chr1", 82000, "50M", None), row("absent_vs", 0, "chr1", 82500, "50M", None),
             row("present_vs", 0, "chr1", 82500, "50M", 16)]
    rows += [row("many_14", 0, "chr1", 83000, "50M", 14), row("few_15", 0, "chr1", 83000, "10M", 15), row("mixed", 0, "chr1", 83000, "8M", [14, 15, 14, 16, 2, 15, 14, 14])]
    # more than 70 000 bases with real qualities, against a short read on its end
    rows += [row("long", 0, "chr2", 1000, "70001M", [k % 41 for k in range(70001)]), row("long_rival", 0, "chr2", 1000, "50M", 40)]
    # more than 65 535 CIGAR operations, soft clips at both ends, on both strands, each against a rival on its unclipped end
    many = "7S" + "1M1I" * 33000 + "1M" + "9S"                                               # 66 003 operations, 66 017 bases, span 33 001
    rows += [row("cg_forward", 0, "chr2", 100000, many, 20), row("cg_forward_rival", 0, "chr2", 99993, "50M", 41)]
    rows += [row("cg_reverse", 16, "chr2", 150000, many, 20), row("cg_reverse_rival", 16, "chr2", 150000 + 33001 + 9 - 50, "50M", 41)]
    # more fragments on one end than a radix tile holds
    rows += [row("tiny%04d" % k, 0, "chr2", 5000, "4M", [rng.randrange(10, 40) for _ in range(4)]) for k in range(TINY)]
    # a background of fragments and pairs
    for k in range(80):
        n = rng.randrange(30, 120)
        rows.append(row("bg%03d" % k, rng.choice([0, 16]), "chr1", rng.randrange(100000, 100400), "%dM" % n, [rng.randrange(2, 41) for _ in range(n)]))
    for k in range(40):
        a = rng.randrange(200000, 200040)
        rows += pair("bgp%03d" % k, "chr1", a, "50M", rng.randrange(10, 40), False, "chr1", a + rng.randrange(300, 304), "50M", rng.randrange(10, 40), True, swap=k % 2 == 1)
    rng.shuffle(rows)
    return "\n".join(rows) + "\n"


def bam(seed=7):
    return Bam(sam_text(seed), REFS, sort=False)


# ---- the yardstick
def examined(r):
    return not r.flag & 4 and r.tid >= 0 and not r.flag & 0x900


def end_of(r):
    """(tid, unclipped 5' position, reverse) from the real CIGAR"""
    lead = trail = 0
    for n, op in r.cigar:
        if op not in (4, 5):
            break
        lead += n
    for n, op in reversed(r.cigar):
        if op not in (4, 5):
            break
        trail += n
    reverse = bool(r.flag & 16)
    return (r.tid, r.pos + ref_span(r.cigar) - 1 + trail if reverse else r.pos - lead, reverse)


def score_of(r):
    if r.qual is None or not r.qual:
        return 0
    return min(sum(q for q in r.qual if q >= MIN_QUALITY), SCORE_MAX)


def read_number(r):
    return {0x40: 1, 0x80: 2}.get(r.flag & 0xc0)


def resolve(records):
    """-> (duplicate: list of bool, one per record; counts: dict)"""
    n = len(records)
    by_name = {}
    for i, r in enumerate(records):
        if examined(r) and r.flag & 1 and not r.flag & 8 and read_number(r):
            by_name.setdefault(r.qname, {1: [], 2: []})[read_number(r)].append(i)
    mate = {}
    for reads in by_name.values():
        for a, b in zip(reads[1], reads[2]):             # the lowest indices pair up in order
            mate[a], mate[b] = b, a
    duplicate = [False] * n
    by_signature = {}
    for a, b in mate.items():
        if a < b:
            ends = tuple(sorted([end_of(records[a]), end_of(records[b])]))
            by_signature.setdefault(ends, []).append((min(score_of(records[a]) + score_of(records[b]), SCORE_MAX), a, b))
    duplicate_pairs = 0
    for pairs in by_signature.values():
        best = max(pairs, key=lambda p: (p[0], -p[1]))
        for p in pairs:
            if p is not best:
                duplicate[p[1]] = duplicate[p[2]] = True
                duplicate_pairs += 1
    paired_ends = {end_of(records[i]) for i in mate}
    by_end = {}
    fragments = [i for i, r in enumerate(records) if examined(r) and i not in mate]
    for i in fragments:
        by_end.setdefault(end_of(records[i]), []).append(i)
    duplicate_fragments = 0
    for end, members in by_end.items():
        best = None if end in paired_ends else max(members, key=lambda i: (score_of(records[i]), -i))
        for i in members:
            if i != best:
                duplicate[i] = True
                duplicate_fragments += 1
    counts = dict(records=n, examined=sum(examined(r) for r in records), pairs=len(mate) // 2, fragments=len(fragments), duplicate_pairs=duplicate_pairs,
                  duplicate_fragments=duplicate_fragments, duplicates=2 * duplicate_pairs + duplicate_fragments)
    return duplicate, counts


def pair_ties(records):
    """signatures on which two pairs share the best score (the index decides there)"""
    duplicate, _ = resolve(records)
    by_name = {}
    for i, r in enumerate(records):
        by_name.setdefault(r.qname, []).append(i)
    out = []
    for name in ("tie_pair_a", "tie_pair_b"):
        members = [i for i in by_name[name] if examined(records[i])]
        out.append((name, sum(score_of(records[i]) for i in members), tuple(sorted(end_of(records[i]) for i in members)), min(members), duplicate[members[0]]))
    return out


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def end_key(end):
    tid, pos, reverse = end
    return tid << 33 | (max(-(1 << 31), min(pos, (1 << 31) - 1)) + (1 << 31)) << 1 | int(reverse)


def summaries(records, dtype):
    """the summary of every record as docs/markdup_bam.md states it"""
    out = np.zeros(len(records), dtype=dtype)
    for i, r in enumerate(records):
        out[i]["index"] = i
        out[i]["end"] = 0xffffffffffffffff
        if not examined(r):
            continue
        number = read_number(r)
        pairable = bool(r.flag & 1 and not r.flag & 8 and number)
        out[i]["end"], out[i]["hash"], out[i]["score"] = end_key(end_of(r)), fnv1a(r.qname.encode()), score_of(r)
        out[i]["bits"] = 1 | (2 if pairable else 0) | (4 if pairable and number == 2 else 0) | (8 if r.flag & 16 else 0)
    return out


def stream_of(b):
    """-> (the records back to back, their starts)"""
    pieces = [r.encode() for r in b.records]
    starts = np.cumsum([0] + [len(p) for p in pieces[:-1]]).astype(np.int64)
    return b"".join(pieces), starts


def patched(record, is_examined, is_duplicate):
    """the record's bytes with bit 0x400 as the rule decides it (an examined record) or as they are"""
    if not is_examined:
        return record
    high = (record[19] & ~0x04) | (0x04 if is_duplicate else 0)
    return record[:19] + bytes([high]) + record[20:]


def expected_stream(b, remove=False):
    """what the output inflates to"""
    duplicate, _ = resolve(b.records)
    out = [b.header()]
    for r, d in zip(b.records, duplicate):
        if not (remove and d):
            out.append(patched(r.encode(), examined(r), d))
    return b"".join(out)


# ---- the resolution alone: summaries that cross a radix tile (2048) and a digit boundary
def synthetic(n, kind, dtype, seed=0):
    """n summaries: 70 % of them in pairs (read 1 and read 2 of one hash at random places), the rest fragments.  kind: "mixed" few ends and
    scores, "all_equal" one end for everything, "all_distinct" every end its own, "equal_scores" few ends and one score."""
    rng = np.random.default_rng(100 + seed + n)
    out = np.zeros(n, dtype=dtype)
    out["index"] = np.arange(n)
    out["bits"] = 1 | (rng.integers(0, 2, n) << 3)
    if kind == "all_equal":
        ends = np.full(n, 5 << 33 | 77 << 1, dtype=np.uint64)
    elif kind == "all_distinct":
        ends = (rng.permutation(n).astype(np.uint64) * np.uint64(0x10001) + np.uint64(3 << 33)) << np.uint64(1)          # low digits and digits above them differ
    else:
        ends = (rng.integers(0, 3, n).astype(np.uint64) << np.uint64(33)) | (rng.integers(250, 262, n).astype(np.uint64) << np.uint64(1))
    out["end"] = ends | ((out["bits"] >> 3) & 1).astype(np.uint64) if kind != "all_equal" else ends
    out["score"] = 1000 if kind == "equal_scores" else rng.integers(0, 6, n) * 100 if kind == "mixed" else rng.integers(0, 1 << 32, n, dtype=np.uint64)
    out["hash"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    places = rng.permutation(n)[:int(0.7 * n) // 2 * 2]
    for a, b in zip(places[0::2], places[1::2]):
        out[b]["hash"] = out[a]["hash"]
        out[a]["bits"] |= 2
        out[b]["bits"] |= 2 | 4
    if n > 8:                                             # one hash with three read 1s and two read 2s, and a record that is not examined
        group = rng.permutation(n)[:6]
        out["hash"][group[:5]] = 0x1234
        out["bits"][group[:3]] = (out["bits"][group[:3]] & 8) | 1 | 2
        out["bits"][group[3:5]] = (out["bits"][group[3:5]] & 8) | 1 | 2 | 4
        out[group[5]] = (0xffffffffffffffff, 0, 0, group[5], 0, 0)
    return out


def resolve_summaries(s):
    """the rule over summaries, with dictionaries: the yardstick of the resolution tests"""
    n = len(s)
    end, hashes, score, bits = s["end"].tolist(), s["hash"].tolist(), s["score"].tolist(), s["bits"].tolist()
    groups = {}
    for i in range(n):
        if bits[i] & 2:
            groups.setdefault(hashes[i], {0: [], 4: []})[bits[i] & 4].append(i)
    mate = {}
    for reads in groups.values():
        for a, b in zip(reads[0], reads[4]):
            mate[a], mate[b] = b, a
    duplicate = np.zeros(n, dtype=np.uint8)
    by_signature = {}
    for a, b in mate.items():
        if a < b:
            by_signature.setdefault((min(end[a], end[b]), max(end[a], end[b])), []).append((min(score[a] + score[b], SCORE_MAX), a, b))
    for pairs in by_signature.values():
        best = max(pairs, key=lambda p: (p[0], -p[1]))
        for p in pairs:
            if p is not best:
                duplicate[p[1]] = duplicate[p[2]] = 1
    paired_ends = {end[i] for i in mate}
    by_end = {}
    for i in range(n):
        if bits[i] & 1 and i not in mate:
            by_end.setdefault(end[i], []).append(i)
    for e, members in by_end.items():
        best = None if e in paired_ends else max(members, key=lambda i: (score[i], -i))
        for i in members:
            if i != best:
                duplicate[i] = 1
    return duplicate
