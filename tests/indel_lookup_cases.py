"""Cases for the indel look-up (test support, not a test): BAMs synthesised with tests/bam_fixture.py next to the pileup columns pysam
would show for them, written in Python from the CIGAR strings alone -- independently of clair_amd/csrc/indel_lookup_core.h -- in the JSON
shape tests/fake_pysam.py reads, so that clair_amd.call_var.AlignmentLookup over the fake pysam is the yardstick of the table look-up."""
import gzip
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import fake_pysam  # noqa: E402

from clair_amd import _hostapi  # noqa: E402

GOLD = os.path.join(HERE, "golden")
FILTER = 2316


def columns_of(sam_text, ctg):
    """{0-based column: [tokens]} as pysam's get_query_sequences(add_indels=True) spells them, reads in file order (the text must be
    sorted by position already): every read of `ctg` with a CIGAR that passes -F 2316, whatever its MAPQ.  An indel is appended to the
    token of the last base of an M / = / X operation when it is the very next operation."""
    cols = {}
    for line in sam_text.splitlines():
        if not line or line.startswith("@"):
            continue
        c = line.split("\t")
        flag, pos, cigar, seq = int(c[1]), int(c[3]) - 1, c[5], c[9]
        if flag & FILTER or c[2] != ctg or cigar == "*":
            continue
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=XB])", cigar)]
        case = (lambda s: s.lower()) if flag & 16 else (lambda s: s.upper())
        rp, qp = pos, 0
        for k, (n, op) in enumerate(ops):
            if op in "M=X":
                for i in range(n):
                    tok = case(seq[qp + i])
                    if i == n - 1 and k + 1 < len(ops) and ops[k + 1][0] > 0:
                        n2, op2 = ops[k + 1]
                        if op2 == "I":
                            tok += "+%d%s" % (n2, case(seq[qp + n:qp + n + n2]))
                        elif op2 == "D":
                            tok += "-%d%s" % (n2, case("N" * n2))
                    cols.setdefault(rp + i, []).append(tok)
                rp += n
                qp += n
            elif op == "I" or op == "S":
                qp += n
            elif op == "D":
                for i in range(n):
                    cols.setdefault(rp + i, []).append("*")
                rp += n
            elif op == "N":
                for i in range(n):
                    cols.setdefault(rp + i, []).append("<" if flag & 16 else ">")
                rp += n
    return cols


class FakePysam(object):
    """sys.modules["pysam"] for a run whose --bam_fn / --ref_fn are a real BAM and FASTA: the columns come from <bam>.columns.json, the
    sequences from <fasta>.json (tests/fake_pysam.py's formats)."""

    class AlignmentFile(fake_pysam.AlignmentFile):
        def __init__(self, path, mode="rb"):
            fake_pysam.AlignmentFile.__init__(self, path + ".columns.json", mode)

    class FastaFile(fake_pysam.FastaFile):
        def __init__(self, filename=None):
            fake_pysam.FastaFile.__init__(self, filename + ".json")


def write_case(tmp, sam_text, ctg, ref_seq, others=(), block=4000):
    """BAM + .bai, FASTA + .fai and the two JSON files of FakePysam -> (bam_fn, fasta_fn)"""
    refs = [(ctg, len(ref_seq))] + [(n, len(s)) for n, s in others]
    bam = bf.Bam(sam_text, refs)
    bam_fn, fa = os.path.join(tmp, "reads.bam"), os.path.join(tmp, "ref.fa")
    bam.write(bam_fn, block=block)
    seqs = dict([(ctg, ref_seq)] + list(others))
    text, fai = bf.fasta_of(seqs)
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    json.dump({ctg: {str(p): t for p, t in columns_of(bam.canonical(), ctg).items()}}, open(bam_fn + ".columns.json", "w"))
    json.dump(seqs, open(fa + ".json", "w"))
    return bam_fn, fa


def host_slabs(bam_fn, ctg, region=(None, None), lookup=True, **kw):
    """the BAM through the native reader, its renderer and the host packer -> [(reads, ops, op_elem, seq)], the packer's stats"""
    r = _hostapi.BamReader(bam_fn, threads=2)
    r.query(ctg, *region)
    buf, off = np.empty(1 << 22, np.uint8), _hostapi.bam_offsets_for(1 << 22)
    p = _hostapi.SamPacker(ctg, lookup=lookup, **kw)
    while True:
        n, k = r.readinto(buf, off)
        if not k:
            break
        p.feed(r.render(buf, off, k), final=True)
    r.close()
    return [p.slab_arrays()], p.stats()


def host_tables(slabs):
    return lambda positions, capacity: _hostapi.indel_table(slabs, positions, capacity)


# ---- the fixture the real reference wrote rows for (tests/golden/pysam_*) as a BAM ------------------------------------------------------
def golden_case():
    z = np.load(os.path.join(GOLD, "pysam_cases.npz"))
    P = z["probs"]
    with gzip.open(os.path.join(GOLD, "pysam_rows.json.gz"), "rt") as f:
        rows = json.load(f)
    return z["x"].astype(np.float32), json.loads(str(z["infos"])), [P[:, 0:21], P[:, 21:24], P[:, 24:57], P[:, 57:90]], rows


def golden_sam():
    """One read per token of tests/golden/pysam_bam.json, in token order: B+nSEQ -> 1M nI 1M and B-n.. -> 1M nD 1M at the column, a bare
    base -> 1M, '*' -> 1M 1D 1M two columns to the left; a lower-case token is a reverse-strand read."""
    cols = json.load(open(os.path.join(GOLD, "pysam_bam.json")))
    ref = json.load(open(os.path.join(GOLD, "pysam_ref.json")))
    (ctg, by_pos), = cols.items()
    lines, k = [], 0
    for p0 in sorted(int(p) for p in by_pos):
        for tok in by_pos[str(p0)]:
            flag = 16 if tok[0].islower() or (tok[0] == "*" and k % 2) else 0
            start = p0
            m = re.match(r"(.)([+-])(\d+)(.*)$", tok)
            if tok == "*":
                start, cigar, seq = p0 - 2, "1M1D1M", "AC"
            elif m is None:
                cigar, seq = "1M", tok
            elif m.group(2) == "+":
                assert len(m.group(4)) == int(m.group(3))
                cigar, seq = "1M%dI1M" % int(m.group(3)), m.group(1) + m.group(4) + "A"
            else:
                cigar, seq = "1M%dD1M" % int(m.group(3)), m.group(1) + "A"
            lines.append("t%d\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*" % (k, flag, ctg, start + 1, cigar, seq.upper()))
            k += 1
    return "\n".join(lines) + "\n", ctg, ref[ctg]


# ---- randomised read sets ---------------------------------------------------------------------------------------------------------
def random_case(seed, ref_len=1400, n_sites=24, dcov=6, leading=True):
    """-> (sam text, ctg, reference, queried 1-based positions): reads of both strands over a few indel sites each, with a small alphabet of
    inserted sequences per site (ties, repeats, lengths up to 60), soft clips, N operations, leading indels, I directly after D (and D
    after I), P before an I, low MAPQ, filtered flags, another contig, a `*` CIGAR, and bursts of more than `dcov` reads at one start.
    leading=False leaves the leading indels out: two of them at one start take a run out of the device front end's regime (CLAIR_FE_LEAD_INDEL)."""
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), ref_len))
    sites = sorted(int(s) for s in rng.choice(np.arange(60, ref_len - 120), n_sites, replace=False))       # 0-based anchor columns
    alphabet = {}
    for s in sites:
        lens = [int(x) for x in rng.choice([1, 2, 3, 5, 16, 17, 18, 30, 49, 50, 51, 60], 4)]
        alphabet[s] = [("I", "".join(rng.choice(list("ACGTacgt"), n))) for n in lens] + [("D", int(n)) for n in rng.choice([1, 2, 16, 17, 20, 50, 55], 3)]
        alphabet[s].append(("I", alphabet[s][0][1].upper()))                                             # the same key in another case
    lines = []

    def add(start, cigar, seq, flag=None, mq=None, ctg="chrL"):
        flag = int(rng.choice([0, 16])) if flag is None else flag
        mq = int(rng.choice([0, 3, 20, 60, 60, 60])) if mq is None else mq
        lines.append((start, "r%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*" % (len(lines), flag, ctg, start + 1, mq, cigar, seq or "*")))

    def bases(n):
        return "".join(rng.choice(list("ACGT"), n))

    for _ in range(int(rng.integers(150, 260))):
        at = int(rng.integers(0, len(sites) - 2))
        start = sites[at] - int(rng.integers(3, 40))
        cigar, seq, rp = "", "", start
        if rng.random() < 0.2:
            n = int(rng.integers(1, 6)); cigar += "%dS" % n; seq += bases(n)
        if rng.random() < 0.1 and leading:                                                               # a leading indel
            if rng.random() < 0.5:
                n = int(rng.integers(1, 4)); cigar += "%dI" % n; seq += bases(n)
            else:
                n = int(rng.integers(1, 4)); cigar += "%dD" % n; rp += n
        after_n = False
        for s in sites[at:at + int(rng.integers(1, 4))]:
            if s < rp or after_n:           # (nothing is asked about the part of a spliced alignment behind its N: docs/indel_lookup.md, third unpinned point)
                continue
            n = s - rp + 1
            cigar += "%d%s" % (n, rng.choice(list("M=X"))); seq += bases(n); rp += n
            kind, what = alphabet[s][int(rng.integers(0, len(alphabet[s])))]
            u = rng.random()
            if u < 0.08:
                n = int(rng.integers(2, 9)); cigar += "%dN" % n; rp += n                                   # the indel follows an N
                after_n = True
            elif u < 0.12:
                cigar += "2P"                                                                            # ... or a pad
            elif u < 0.2:
                if rng.random() < 0.5:
                    cigar += "2D"; rp += 2                                                               # I (or D) directly after a D
                else:
                    cigar += "2I"; seq += bases(2)
            if u >= 0.9:
                continue                                                                                 # no indel here
            if kind == "I":
                cigar += "%dI" % len(what); seq += what
            else:
                cigar += "%dD" % what; rp += what
        n = int(rng.integers(1, 30))
        if rp + n >= ref_len:
            continue
        cigar += "%dM" % n; seq += bases(n)
        if rng.random() < 0.2:
            n = int(rng.integers(1, 6)); cigar += "%dS" % n; seq += bases(n)
        add(start, cigar, seq)
        if rng.random() < 0.04:                                                                          # more than dcov reads at one start
            for _ in range(dcov + 3):
                add(start, cigar, seq)
    for s in sites[:6]:                                                                                  # records the view drops, another contig, no CIGAR
        add(s - 2, "3M2I3M", "ACGTTACG", flag=int(rng.choice([4, 256, 2048, 8])))
        add(s - 2, "3M2I3M", "ACGTTACG", ctg="chrOther")
        add(s - 2, "*", "ACGT", flag=0)
    lines.sort(key=lambda t: t[0])
    return "\n".join(l for _, l in lines) + "\n", "chrL", ref, [s + 1 for s in sites] + [sites[0] + 2, sites[-1] + 200]


def table_bytes(tables, positions, capacity=32):
    e, n, d, s = tables(np.asarray(sorted(set(positions)), dtype=np.int64), capacity)
    return e.tobytes(), n.tolist(), d.tolist(), s.tolist()
