#!/usr/bin/env python3
"""Mint golden vectors for the training-set builder from the REAL reference scripts (build container only).

Runs /root/reference/dataPrepScripts/{ExtractVariantCandidates,CreateTensor,PairWithNonVariants}.py as sub-processes, unmodified, on the
synthetic inputs of tests/pileup_synth.py, as tools/make_pileup_goldens.py does (fake samtools, the intervaltree stand-in).  The two
scripts that thin their output with Python's random module run under tools/run_with_fixed_random.py, which presets every draw to one
value: what is minted is their RULE -- which sites are eligible, which class they have, which rows are usable -- not their stream.
Committed output: data only,

    tests/golden/train_set_evc_<case>.json.gz  = {"args", "uniform", "fasta", "sam", "bed", "truth", "expected", "counters"}
    tests/golden/train_set_pair_<case>.json.gz = {"amp", "uniform", "bed", "var_tensors", "can_tensors", "expected", "log"}

`expected`: the candidate rows / the paired tensor rows; `counters`: the reference's "# of candidates near / outside variant";
`log`: PairWithNonVariants' log lines.
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pileup_synth  # noqa: E402
from make_pileup_goldens import FAKE, GOLD, INTERVALTREE_STUB  # noqa: E402

RUNNER = os.path.join(ROOT, "tools", "run_with_fixed_random.py")
BED = "chrS\t100\t600\nchrS\t550\t900\nchrS\t1500\t1500\nchrS\t2000\t2900\nchrOther\t0\t50\n"


def run_reference(module, args, uniform, cwd, stub_path, stdin_text=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(["/root/reference", stub_path])
    r = subprocess.run([sys.executable, RUNNER, repr(uniform), module] + args, input=stdin_text, capture_output=True, text=True, cwd=cwd, env=env)
    if r.returncode != 0:
        raise RuntimeError("%s failed: %s" % (module, r.stderr[-2000:]))
    return r.stdout, r.stderr


def last_covered(sam):
    """the last 1-based position an alignment of the first contig covers"""
    end = 0
    for line in sam.splitlines():
        col = line.split("\t")
        if line.startswith("@") or col[2] != "chrS":
            continue
        span = sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", col[5]) if op in "MD=X")
        end = max(end, int(col[3]) + span - 1)
    return end


def truth_positions(case):
    """Clusters whose neighbours are 14, 15, 16 and 17 apart, a pair with the sites 15 and 16 from BOTH between them, a site within 16 of the
    contig's start, one beside the last covered position; a repeated row."""
    end = last_covered(case["sam"])
    return [5, 200, 214, 400, 415, 650, 666, 800, 817, 1000, 1031, 1300, 1330, 1700, 1700, 2100, 2400, end - 1]


def write_inputs(tmp, case):
    fa, sam = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.sam")
    open(fa, "w").write(case["fasta"])
    open(fa + ".fai", "w").write("%s\t%d\t6\t60\t61\n" % (case["ctg"], case["ref_len"]))
    open(sam, "w").write(case["sam"])
    stub = os.path.join(tmp, "stub", "intervaltree")
    os.makedirs(stub)
    open(os.path.join(stub, "__init__.py"), "w").write(INTERVALTREE_STUB)
    return fa, sam, os.path.dirname(stub)


EVC_CASES = {
    # name: (synth kwargs, extra CLI args, bed?, truth rows?, the value of every draw)
    "all_bed": (dict(seed=41, n_reads=400), ["--outputProb", "1.0"], True, False, 0.5),
    "all_region_cov": (dict(seed=42, n_reads=400), ["--outputProb", "1.0", "--ctgStart", "400", "--ctgEnd", "2400", "--minCoverage", "6"], False, False, 0.5),
    # 0.4: above the probability of a site outside (0.0023), below that of a site near a variant (0.5): exactly the eligible near sites
    "var_near": (dict(seed=43, n_reads=400), [], False, True, 0.4),
    # 0.0: every eligible site that is no truth site
    "var_all": (dict(seed=43, n_reads=400), [], False, True, 0.0),
}


def mint_candidates():
    for name, (kw, extra, with_bed, with_truth, uniform) in EVC_CASES.items():
        case = pileup_synth.synth_case(**kw)
        truth = None
        with tempfile.TemporaryDirectory() as tmp:
            fa, sam, stub = write_inputs(tmp, case)
            args = ["--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"], "--samtools", FAKE, "--gen4Training"] + extra
            if with_bed:
                open(os.path.join(tmp, "regions.bed"), "w").write(BED)
                args += ["--bed_fn", os.path.join(tmp, "regions.bed")]
            if with_truth:
                truth = "".join("%s %d A C 0 1\n" % (case["ctg"], p) for p in truth_positions(case))
                open(os.path.join(tmp, "truth.var"), "w").write(truth)
                args += ["--var_fn", os.path.join(tmp, "truth.var")]
            out, _ = run_reference("dataPrepScripts.ExtractVariantCandidates", args, uniform, tmp, stub)
        rows = [r for r in out.splitlines() if not r.startswith("#")]
        counters = [int(r.split(":")[1]) for r in out.splitlines() if r.startswith("#")]
        doc = {"tool": "ExtractVariantCandidates --gen4Training", "args": extra, "uniform": uniform, "ctg": case["ctg"], "ref_len": case["ref_len"],
               "fasta": case["fasta"], "sam": case["sam"], "bed": BED if with_bed else None, "truth": truth,
               "expected": "".join(r + "\n" for r in rows), "counters": counters or None}
        with gzip.open(os.path.join(GOLD, "train_set_evc_%s.json.gz" % name), "wt", compresslevel=9) as f:
            json.dump(doc, f)
        print(name, "rows:", len(rows), "counters:", counters)


PAIR_CASES = {
    # name: (synth kwargs, bed?, amp: large enough for r = 1)
    "bed": (dict(seed=44, n_reads=300), True, 100.0),
    "nobed": (dict(seed=45, n_reads=300), False, 50.0),
}


def mint_pairs():
    for name, (kw, with_bed, amp) in PAIR_CASES.items():
        case = pileup_synth.synth_case(**kw)
        truth = sorted(set(truth_positions(case)))
        sampled = [p for p in range(90, case["ref_len"], 47)] + truth[2:5]     # a few sampled sites ARE truth sites: PairWithNonVariants drops them
        with tempfile.TemporaryDirectory() as tmp:
            fa, sam, stub = write_inputs(tmp, case)
            texts = []
            for sites in (truth, sorted(sampled)):
                cands = "".join("%s\t%d\tA\t10\n" % (case["ctg"], p) for p in sites)
                out, _ = run_reference("dataPrepScripts.CreateTensor", ["--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"], "--samtools", FAKE], 0.5, tmp, stub, cands)
                texts.append(out)
            var_fn, can_fn, out_fn = (os.path.join(tmp, n) for n in ("var.gz", "can.gz", "paired.gz"))
            for fn, text in zip((var_fn, can_fn), texts):
                with gzip.open(fn, "wt") as f:
                    f.write(text)
            args = ["--tensor_var_fn", var_fn, "--tensor_can_fn", can_fn, "--output_fn", out_fn, "--amp", repr(amp)]
            if with_bed:
                open(os.path.join(tmp, "regions.bed"), "w").write(BED)
                args += ["--bed_fn", os.path.join(tmp, "regions.bed")]
            _, log = run_reference("dataPrepScripts.PairWithNonVariants", args, 0.5, tmp, stub)
            expected = gzip.open(out_fn, "rt").read()
        doc = {"tool": "PairWithNonVariants", "amp": amp, "uniform": 0.5, "ctg": case["ctg"], "bed": BED if with_bed else None,
               "var_tensors": texts[0], "can_tensors": texts[1], "expected": expected, "log": log.replace(tmp, "@TMP@")}
        with gzip.open(os.path.join(GOLD, "train_set_pair_%s.json.gz" % name), "wt", compresslevel=9) as f:
            json.dump(doc, f)
        print(name, "var rows:", texts[0].count("\n"), "can rows:", texts[1].count("\n"), "paired:", expected.count("\n"), [l for l in log.splitlines() if l[0].isdigit()])


if __name__ == "__main__":
    mint_candidates()
    mint_pairs()
