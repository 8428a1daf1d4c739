#!/usr/bin/env python3
"""make_train_set on one GPU, once per front end, then one epoch of train on the set it wrote (docs/train_set.md, "Baseline").

    python tools/train_set_bench.py [ref_len] [depth] [out_dir]

The synthetic contig of tools/e2e_bam_bench.py (tools/fast_reads.py: 50x of 2-9 kb reads over 2 Mb by default) with a truth row every
~1 000 bases; `samtools` is the same shell stand-in.  Prints the wall time of each run with the front end's own stage split, checks
that the two sets are the same file, and trains one epoch from it (out_dir/model-000001).
"""
import os
import stat
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fast_reads  # noqa: E402


def main():
    ref_len = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    with tempfile.TemporaryDirectory() as tmp:         # (200 MB of SAM text: gone when the run is)
        return run(tmp, ref_len, depth, sys.argv[3] if len(sys.argv) > 3 else os.path.join(tmp, "out"))


def run(tmp, ref_len, depth, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    case = fast_reads.make(ref_len=ref_len, depth=depth, noisy_every=25, seed=5)
    fa, sam, var = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.sam"), os.path.join(tmp, "truth.var")
    open(fa, "w").write(case["fasta"])
    open(fa + ".fai", "w").write("%s\t%d\t6\t60\t61\n" % (case["ctg"], case["ref_len"]))
    open(sam, "wb").write(case["sam"])
    rng = np.random.default_rng(8)
    alleles = (("A", "C", 0, 1), ("AT", "A", 1, 1), ("G", "GTT", 0, 1), ("C", "A,T", 1, 2))
    sites = np.unique(rng.integers(100, ref_len - 100, ref_len // 1000))
    with open(var, "w") as f:
        for p in sites.tolist():
            f.write("%s %d %s %s %d %d\n" % ((case["ctg"], p) + alleles[int(rng.integers(0, len(alleles)))]))
    fake = os.path.join(tmp, "samtools")
    open(fake, "w").write("#!/bin/sh\nif [ \"$1\" = view ]; then exec cat %s; fi\nexec %s %s \"$@\"\n" % (sam, sys.executable, os.path.join(ROOT, "tests", "fake_samtools.py")))
    os.chmod(fake, os.stat(fake).st_mode | stat.S_IEXEC)
    print("inputs: %.1f MB SAM, %d reads over %d bases at %dx, %d truth rows (%.0f s to generate)"
          % (len(case["sam"]) / 1e6, case["n_reads"], ref_len, depth, len(sites), time.time() - t0), flush=True)
    sets = {}
    for front_end in ("device", "host"):
        sets[front_end] = os.path.join(out_dir, "set_%s.npz" % front_end)
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set", "--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"], "--var_fn", var,
                            "--samtools", fake, "--front_end", front_end, "--outputProb", "0.01", "--seed", "1", "--set_fn", sets[front_end]],
                           cwd=ROOT, capture_output=True, text=True)
        dt = time.time() - t0
        if r.returncode != 0:
            print(r.stderr[-2000:])
            return 1
        print("make_train_set --front_end %s: %.2f s wall, %d rows in the set" % (front_end, dt, len(np.load(sets[front_end])["positions"])), flush=True)
        for line in r.stderr.splitlines():
            print("   ", line)
    same = open(sets["device"], "rb").read() == open(sets["host"], "rb").read()
    print("the two sets are the same file: %s" % same)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "clair_amd.train", "--set_fn", sets["device"], "--ochk_prefix", os.path.join(out_dir, "model"), "--max_epochs", "1",
                        "--seed", "1"], cwd=ROOT, capture_output=True, text=True)
    print("train --set_fn, one epoch: %.2f s wall, exit %d, checkpoint written: %s"
          % (time.time() - t0, r.returncode, sorted(n for n in os.listdir(out_dir) if n.startswith("model-"))))
    for line in r.stderr.splitlines()[:12]:
        print("   ", line)
    return 0 if same and r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
