"""Inputs and expected values for the training-set builder's tests (test support): the rules restated in plain Python, independent of
csrc/train_set_core.h -- the class of a position by the DICT CONSTRUCTION the reference runs (ExtractVariantCandidates.py:59-101), the draw
in Python integers, the pairing loop of PairWithNonVariants.py:17-90 -- the labels through evaluate.labelled_batches, the golden records
minted from the reference's scripts (tests/golden/train_set_*.json.gz, tools/make_train_set_goldens.py) and small synthetic worlds on disk."""
import glob
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frontend_cases as fc  # noqa: E402
import pileup_synth  # noqa: E402

from clair_amd.extract_variant_candidates import BedRegions  # noqa: E402

EVC_GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "train_set_evc_*.json.gz")))
PAIR_GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "train_set_pair_*.json.gz")))
FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))
MASK = (1 << 64) - 1
OUTSIDE, NEAR, TRUTH = 0, 1, 2
NEAR_PROB, OUTSIDE_PROB, PLAIN_PROB = 3500000.0 * 1.0 * 2.0 / 14000000, 3500000.0 * 2.0 / (3000000000 - 14000000), 7000000.0 * 2.0 / 3000000000


# ---- the draw in Python integers ------------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def fnv1a64(name):
    h = 0xCBF29CE484222325
    for b in name.encode():
        h = ((h ^ b) * 0x100000001B3) & MASK
    return h


def key_of(seed, ctg, stage):
    return mix64(mix64(seed & MASK) ^ mix64(fnv1a64(ctg) ^ stage))


def draw_of(key, pos):
    return mix64((key + pos) & MASK) >> 11


def u_of(key, pos):
    return draw_of(key, pos) * 2.0 ** -53


def signed(key):
    return key - (1 << 64) if key >> 63 else key


# ---- the class of a position: the reference's two dicts -------------------------------------------------------------------------------
def near_map(truth, lower=15, upper=16):
    """non_variants_map_near_variants_from (ExtractVariantCandidates.py:59-101) over positions of one contig -> the set of its keys"""
    variants = dict((int(p), True) for p in truth)
    non_variants, to_exclude = {}, {}
    for position in variants:
        for i in range(upper * 2 + 1):
            offset = -upper + i
            temp = position + offset
            if temp <= 0:
                continue
            if temp not in variants and temp not in non_variants and (-upper <= offset <= -lower or lower <= offset <= upper):
                non_variants[temp] = True
            if lower > offset > -lower:
                to_exclude[temp] = True
    for k in to_exclude:
        if k in non_variants:
            del non_variants[k]
    return set(non_variants)


def classes_of(truth, positions):
    near, variants = near_map(truth), set(int(p) for p in truth)
    return np.array([TRUTH if int(p) in variants else NEAR if int(p) in near else OUTSIDE for p in positions], dtype=np.uint8)


def sampled_of(eligible, truth, p_near, p_outside, seed, ctg):
    """-> (sampled positions, n_near, n_outside): :330-343 with the counter-based draw in place of random.uniform(0, 1)"""
    key = key_of(seed, ctg, 1)
    cls = classes_of(truth, eligible)
    keep = [c != TRUTH and u_of(key, int(p)) <= (p_near if c == NEAR else p_outside) for p, c in zip(eligible, cls)]
    keep = np.array(keep, dtype=bool).reshape(len(eligible))
    return np.asarray(eligible, dtype=np.int64)[keep], int((cls[keep] == NEAR).sum()), int((cls[keep] != NEAR).sum())


# ---- the pairing ----------------------------------------------------------------------------------------------------------------------
def pair_of(centres, truth, bed, amp, seed, ctg):
    """PairWithNonVariants.py:17-90 over window centres -> (kept indices: variant windows, then non-variant ones; dict v, c, r, kept_var, kept_non)"""
    variants, regions = set(int(p) for p in truth), None if bed is None else BedRegions(bed)
    var = [i for i, p in enumerate(centres) if int(p) in variants]
    usable = [i for i, p in enumerate(centres) if int(p) not in variants and (regions is None or int(p) in regions)]
    v, c = len(var), len(usable)
    r = 1.0 if c == 0 else min(1.0, float(v * amp) / c)
    key = key_of(seed, ctg, 2)
    non = [i for i in usable if u_of(key, int(centres[i])) < r]
    return np.array(var + non, dtype=np.int64), dict(v=v, c=c, r=r, kept_var=v, kept_non=len(non))


def expected_set(tmp, tensor_text, truth_rows_text, bed_text):
    """The data set get_training_array makes of the paired rows, through evaluate.labelled_batches -> (X float32, keys, labels uint8)"""
    from clair_amd.evaluate import labelled_batches
    t, v, b = (os.path.join(str(tmp), n) for n in ("expected_tensors.gz", "expected_truth.var", "expected.bed"))
    with gzip.open(t, "wt") as f:
        f.write(tensor_text)
    open(v, "w").write(truth_rows_text)
    if bed_text is not None:
        open(b, "w").write(bed_text)
    xs, keys, ys = [], [], []
    for X, k, y in labelled_batches(t, v, b if bed_text is not None else None, 512):
        xs.append(np.array(X, dtype=np.float32))
        keys += list(k)
        ys.append(y)
    if not xs:
        return np.zeros((0, 33, 8, 4), np.float32), [], np.zeros((0, 4), np.uint8)
    return np.concatenate(xs), keys, np.concatenate(ys)


# ---- golden records and synthetic worlds ----------------------------------------------------------------------------------------------
def evc_golden(path):
    """-> the case of frontend_cases.evc_golden_case plus truth (int64 positions in file order, or None), counters, uniform"""
    case, doc = fc.evc_golden_case(path), fc.load(path)
    case["truth"] = None if doc["truth"] is None else np.array([int(r.split()[1]) for r in doc["truth"].splitlines()], dtype=np.int64)
    case["counters"], case["uniform"] = doc["counters"], doc["uniform"]
    return case


def eligible_of(case):
    rng = case.get("ctg_range") or (None, None)
    return fc.host_candidates(case, threshold=0.0, min_coverage=case["min_coverage"], min_mq=0, ctg_start=rng[0], ctg_end=rng[1], bed=case["bed"])


TRUTH_ALLELES = (("A", "C", 0, 1), ("AT", "A", 1, 1), ("G", "GTT", 0, 1), ("C", "A,T", 1, 2), ("T", "TAA,TA", 1, 2), ("G", "C", 1, 1))


def truth_rows(ctg, positions, rng):
    """rows `ctg pos ref alt g1 g2` with SNPs, indels and multi-allelic calls (positions may repeat: the last row of one wins)"""
    rows = []
    for p in positions:
        ref, alt, g1, g2 = TRUTH_ALLELES[int(rng.integers(0, len(TRUTH_ALLELES)))]
        rows.append("%s %d %s %s %d %d" % (ctg, int(p), ref, alt, g1, g2))
    return rows


def truth_table(rows):
    """-> (positions ascending, labels [n,4]) as make_train_set hands them to the front end"""
    from clair_amd.make_train_set import truth_table as table
    return table([r.split() for r in rows])


def world(tmp, seed, truth_positions, bed=None, **synth_kw):
    """A synthetic contig on disk: ref.fa(.fai), reads.sam (the `BAM` of tests/fake_samtools.py), truth.var, regions.bed -> dict of paths and the case"""
    tmp = str(tmp)
    raw = pileup_synth.synth_case(seed=seed, **synth_kw)
    ref, ref0 = fc.reference_of(raw["fasta"], raw["ctg"])
    case = dict(ctg=raw["ctg"], ref=ref, ref0=ref0, sam=fc.viewed(raw["sam"], raw["ctg"]), candidates=np.zeros(0, np.int64))
    paths = dict((n, os.path.join(tmp, n)) for n in ("ref.fa", "reads.sam", "truth.var", "regions.bed"))
    open(paths["ref.fa"], "w").write(raw["fasta"])
    open(paths["ref.fa"] + ".fai", "w").write("%s\t%d\t6\t60\t61\n" % (raw["ctg"], raw["ref_len"]))
    open(paths["reads.sam"], "w").write(raw["sam"])
    rows = truth_rows(raw["ctg"], truth_positions, np.random.default_rng(seed))
    open(paths["truth.var"], "w").write("".join(r + "\n" for r in rows))
    bed_text = None
    if bed is not None:
        bed_text = "".join("%s\t%d\t%d\n" % (raw["ctg"], s, e) for s, e in bed)
        open(paths["regions.bed"], "w").write(bed_text)
    return dict(case=case, paths=paths, rows=rows, bed=bed, bed_text=bed_text, ref_len=raw["ref_len"])


def cli_args(w, *more):
    p = w["paths"]
    args = ["--bam_fn", p["reads.sam"], "--ref_fn", p["ref.fa"], "--ctgName", w["case"]["ctg"], "--var_fn", p["truth.var"], "--samtools", FAKE_SAMTOOLS]
    if w["bed"] is not None:
        args += ["--bed_fn", p["regions.bed"]]
    return args + list(more)
