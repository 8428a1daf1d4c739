"""Read subsampling (docs/subsample.md): the rule restated in Python integers and the fixtures of tests/test_subsample.py and
tests/test_subsample_gpu.py (test support, not a test).

One builder (tests/bam_fixture.py) writes a BAM A with all records and a BAM B with exactly the records the restatement below keeps: A read
with the rule must be B read without it.  The restatement is written from the formula of the document and imports nothing of the package.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import pileup_synth  # noqa: E402

M32 = 0xffffffff
# QNAME, S, h, k, (k & 0xffffff) / 2^24: worked out from the formula by a stand-alone restatement
ANCHORS = [(b"a", 0, 0x00000061, 0xad8b4236, 0.5439790487289429),
           (b"read0", 0, 0x0675d95a, 0xc32df5d6, 0.17953240871429443),
           (b"read0", 11, 0x0675d95a, 0xc4253ff8, 0.1455073356628418),
           (b"r1", 0, 0x00000dff, 0xf0f8c8cd, 0.971813976764679),
           (b"m64011_190830_220126/1/ccs", 0, 0xc9ce52a3, 0x19bb4715, 0.7315533757209778),
           (b"x" * 254, 7, 0xeb1fb100, 0xa426bf64, 0.15135788917541504)]
# F, S, names kept of read0 .. read299
KEPT_OF_300 = [(0.5, 0, 150), (0.5, 11, 140), (0.1, 0, 33), (0.8, 0, 232), (0.8, 11, 232)]
NAME_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 253, 254)


def name_hash(name):
    h = 0
    for c in bytes(name).split(b"\0", 1)[0]:
        h = ((h << 5) - h + (c - 256 if c >= 128 else c)) & M32
    return h


def mixed(k):
    k = (k + (~(k << 15) & M32)) & M32
    k ^= k >> 10
    k = (k + (k << 3)) & M32
    k ^= k >> 6
    k = (k + (~(k << 11) & M32)) & M32
    k ^= k >> 16
    return k


def quotient(name, seed):
    return (mixed(name_hash(name) ^ seed) & 0xffffff) / 16777216.0


def keeps(name, seed, frac):
    return frac <= 0 or not quotient(name, seed) >= frac


def viewable(line, ctg, region=None):
    """`samtools view -F 2316 <bam> ctg[:lo-hi]` prints this SAM line"""
    col = line.split("\t")
    if int(col[1]) & 2316 or col[2] != ctg:
        return False
    if region is None:
        return True
    pos = int(col[3])
    end = pos + max(bf.ref_span(bf.parse_cigar(col[5])), 1) - 1
    return pos <= region[1] and end >= region[0]


def with_mates(lines):
    """every fourth name gets a second record: the two carry paired flags and share their fate"""
    out = []
    for k, line in enumerate(lines):
        col = line.split("\t")
        if k % 4 == 1:
            out.append("\t".join(col[:1] + [str(int(col[1]) | 1 | 64)] + col[2:]))
            out.append("\t".join(col[:1] + [str(int(col[1]) | 1 | 128)] + col[2:]))
        else:
            out.append(line)
    return out


def write_pair(tmp, lines, refs, seed, frac, stem, block=5000):
    """BAM A of all `lines` and BAM B of those whose name the restatement keeps -> (path A, path B, lines of A, lines of B), in file order"""
    paths, kept = [], []
    for tag, some in (("a", lines), ("b", [l for l in lines if keeps(l.split("\t")[0].encode("latin-1"), seed, frac)])):
        bam = bf.Bam("\n".join(some) + "\n", refs)
        paths.append(os.path.join(str(tmp), "%s_%s.bam" % (stem, tag)))
        bam.write(paths[-1], block=block)
        kept.append(bam.canonical().splitlines())
    return paths[0], paths[1], kept[0], kept[1]


def assert_a_real_subset(lines_a, lines_b, ctg, region=None):
    """B holds at least 10 % and at most 90 % of A's viewable records: an all-or-nothing rule does not pass"""
    a = sum(viewable(l, ctg, region) for l in lines_a)
    b = sum(viewable(l, ctg, region) for l in lines_b)
    assert a > 0 and 0.1 * a <= b <= 0.9 * a, (a, b)
    return a, b


def world(tmp, seed=0, frac=0.5, synth_seed=91, n_reads=300, ref_len=3000):
    """read0 .. read299 with mates, records the view drops anyway (flags, another contig) sprinkled in by the generator -> dict"""
    tmp = str(tmp)
    case = pileup_synth.synth_case(seed=synth_seed, n_reads=n_reads, ref_len=ref_len, read_len=(150, 400))
    ctg = case["ctg"]
    seq = "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:])
    fa = os.path.join(tmp, "ref.fa")
    if not os.path.isfile(fa):
        text, fai = bf.fasta_of({ctg: seq, "chrOther": "ACGT" * 30})
        open(fa, "w").write(text)
        open(fa + ".fai", "w").write(fai)
    lines = with_mates([l for l in case["sam"].splitlines() if l and not l.startswith("@")])
    refs = [(ctg, case["ref_len"]), ("chrOther", 120)]
    a, b, lines_a, lines_b = write_pair(tmp, lines, refs, seed, frac, "s%d_%s" % (seed, str(frac).replace(".", "")))
    return dict(ctg=ctg, ref=seq.upper(), ref_len=case["ref_len"], fa=fa, a=a, b=b, lines_a=lines_a, lines_b=lines_b, seed=seed, frac=frac)


def name_family(tmp, seed=0, frac=0.5, ref_len=1500):
    """Names of NAME_LENGTHS bytes, eight of each, between records of every size mod 4: the shapes at which the dword reads of a name can go
    wrong -> dict like world()'s.  (The name of a record starts 36 bytes into it: where it lands mod 4 is the sum of the sizes before it.)"""
    case = pileup_synth.synth_case(seed=17, n_reads=1, ref_len=ref_len, iupac=False, second_ctg=False)
    ctg = case["ctg"]
    seq = "".join(case["fasta"].splitlines()[1:]).upper()
    lines, k = [], 0
    for n in NAME_LENGTHS:
        # a record is 4 + 32 + (n + 1) + 4 (one CIGAR operation) + ceil(span / 2) + span bytes: with a size of 1 mod 4 the eight names of a
        # length, consecutive in the file (the positions ascend), land on every alignment twice
        spans = [s for s in range(20, 28) if (41 + n + (s + 1) // 2 + s) % 4 == 1]
        for j in range(8):
            pos, span = 1 + 7 * k, spans[j % 2]
            bases = seq[pos - 1:pos - 1 + span]
            if j % 3 == 0:                                   # a mismatch column: something for the candidate search
                bases = bases[:9] + "ACGT"[("ACGT".index(bases[9]) + 1) % 4] + bases[10:]
            lines.append("%s\t%d\t%s\t%d\t60\t%dM\t*\t0\t0\t%s\t%s" % (chr(ord("a") + j) * n, 16 * (k & 1), ctg, pos, span, bases, "I" * span))
            k += 1
    a, b, lines_a, lines_b = write_pair(tmp, lines, [(ctg, ref_len)], seed, frac, "names", block=3001)
    return dict(ctg=ctg, ref=seq, ref_len=ref_len, a=a, b=b, lines_a=lines_a, lines_b=lines_b, seed=seed, frac=frac)
