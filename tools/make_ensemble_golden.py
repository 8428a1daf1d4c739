#!/usr/bin/env python3
"""Mint tests/golden/ensemble_small.json.gz from the REAL reference filter (runs only where a reference checkout exists, like the other
tools/make_*_goldens.py): clair/post_processing/ensemble.py is RUN, as a process, on inputs built here; nothing of it is copied.

    python tools/make_ensemble_golden.py --reference DIR        (or $CLAIR_REFERENCE: a checkout of the reference project)

The fixture (data only):
  inputs    three streams in call_var --output_for_ensemble format (clair/call_var.py:950-1000), one per "model": the probabilities of
            this project's float32 oracle (oracle/c_oracle.py) under weights.synthetic_weights(seed, head_gain=4) for three seeds, over
            40 synthetic ONT sites, written by this build's own writer.  Arranged so that
              - the sites of a stream are NOT in position order, and each stream has its own order;
              - seven sites are missing from the second stream, six from the third, three of those from both (count 1, 2 and 3 all occur);
              - one site carries a different tensor and sequence in the second stream (the first row of a site wins);
              - one site appears twice in the first stream (count 4 with three inputs: the divisor is the row count, not the stream count).
  outputs   stdout of the reference's filter over the concatenation first + second + third for --minimum_count_to_output 0, 2 and 3.
"""
import argparse
import gzip
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "ensemble_small.json.gz")
SEEDS = (101, 202, 303)
N_SITES = 40


def build_inputs():
    from clair_amd import call_var, synth, weights
    from oracle import c_oracle
    raw, infos = synth.synthetic_candidates(N_SITES, "ont", seed=77)
    x = synth.to_model_input(raw)
    rng = np.random.default_rng(5)
    streams = []
    for k, seed in enumerate(SEEDS):
        Y = c_oracle.forward(weights.synthetic_weights(seed=seed, head_gain=4.0), x)
        xs, inf = x, [list(i) for i in infos]
        if k == 1:                      # another tensor and another sequence at one site: neither may reach the output
            xs = x.copy()
            xs[11] = x[12]
            inf[11][2] = infos[12][2]
        rows = call_var.VariantDecoder._ensemble_rows(xs, inf, *Y)
        assert len(rows) == N_SITES
        order = rng.permutation(N_SITES).tolist()
        drop = {0: set(), 1: {3, 8, 13, 21, 30, 34, 39}, 2: {3, 8, 13, 5, 17, 26}}[k]
        rows = [rows[i] for i in order if i not in drop]
        if k == 0:
            rows.append(rows[4])
        streams.append("".join(r + "\n" for r in rows))
    return streams


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("CLAIR_REFERENCE"), help="checkout of the reference project")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or CLAIR_REFERENCE) is needed: this tool runs the reference's own filter")
    script = os.path.join(args.reference, "clair", "post_processing", "ensemble.py")
    if not os.path.isfile(script):
        sys.exit("%s not found: this tool runs the reference's own filter" % script)
    streams = build_inputs()
    outputs = {}
    for threshold in (0, 2, 3):
        r = subprocess.run([sys.executable, script, "--minimum_count_to_output", str(threshold)], input="".join(streams), capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the reference's filter failed: %s" % r.stderr)
        outputs[str(threshold)] = r.stdout
    n = [len(outputs[t].splitlines()) for t in ("0", "2", "3")]
    assert n[0] == N_SITES and n[0] > n[1] > n[2] > 0, n
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"inputs": streams, "outputs": outputs}).encode())
    print("%s: %d bytes, rows per threshold %r" % (OUT, os.path.getsize(OUT), n))


if __name__ == "__main__":
    main()
