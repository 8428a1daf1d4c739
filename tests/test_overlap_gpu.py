"""The overlap filter's walk on the MI355X (clair_overlap_keep, csrc/overlap.hip) against its host twin (clair_host_overlap_keep), which
tests/test_overlap.py pins to the Python walk and, through the text, to the reference's script."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import overlap_cases  # noqa: E402
from clair_amd import _capi, _hostapi, overlap_variant as ov  # noqa: E402

B = _capi.OVERLAP_SCAN_BLOCK
FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))


def _same(spans, name):
    want = _hostapi.overlap_keep(spans)
    got = _capi.overlap_keep(spans)
    assert got.dtype == np.uint8 and got.shape == want.shape, name
    assert np.array_equal(got, want), "%s: first difference at row %d of %d" % (name, int(np.flatnonzero(got != want)[0]), len(want))
    return want


def test_device_walk_equals_the_host_walk_on_generated_rows():
    """Bit for bit on the generator of tests/test_overlap.py, at the sizes that cross the two-level scan: n in {0, 1, 2, B - 1, B, B + 1, 3 B + 5}."""
    assert B == 2048
    dropped = 0
    for name, rows in overlap_cases.generated(sizes=(0, 1, 2, B - 1, B, B + 1, 3 * B + 5)):
        dropped += int((_same(overlap_cases.spans(rows), name) == 0).sum())
    assert dropped > 5000


def test_device_walk_on_crafted_block_boundaries():
    """A deletion's reach carried into the next block and across a whole block, a segment over three blocks, a contig change exactly at a block
    boundary, every row a head, only the first row a head -- each with what makes it the case checked on the host twin's answer."""
    keep = {f.__name__: _same(f(B), f.__name__) for f in overlap_cases.CRAFTED}
    k = keep["reach_crosses_a_block"]
    assert k[B - 1] == 1 and k[B] == 0 and k[B + 1] == 0 and k[B + 2] == 1
    k = keep["reach_carried_over_a_whole_block"]
    assert k[:6].all() and not k[6:2 * B + 21].any() and k[2 * B + 21:].all()
    k = keep["segment_spans_three_blocks"]
    assert 0 < k[:2 * B + 101].sum() < 2 * B and k[2 * B + 102:].all()
    k = keep["contig_changes_at_a_block"]
    assert k[B - 1] == 1 and k[B] == 1 and k[B + 1] == 1 and k[B + 3] == 1 and k[B + 4] == 0
    assert keep["every_row_a_head"].all()
    k = keep["only_the_first_row_a_head"]
    assert 0 < k.sum() < (B + 7) // 2           # a chain: of two neighbours at most one stays


def test_filter_on_the_device_reproduces_the_reference():
    with gzip.open(os.path.join(HERE, "golden", "overlap_small.json.gz")) as f:
        g = json.load(f)
    for k, (text, want) in enumerate(zip(g["inputs"], g["outputs"])):
        assert ov.filter_vcf_text(text, "device") == want, "stream %d" % k


def test_callVarBam_overlap_filter_device_writes_the_filtered_vcf(tmp_path):
    """callVarBam --overlap_filter device on the alignments of tests/test_e2e_gpu.py == the filter over its plain output."""
    import pileup_synth
    from clair_amd import callVarBam, weights
    tmp = str(tmp_path)
    case = pileup_synth.synth_case(seed=91)
    fa, sam = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.sam")
    open(fa, "w").write(case["fasta"])
    open(fa + ".fai", "w").write("%s\t%d\t6\t60\t61\nchrOther\t120\t3100\t120\t121\n" % (case["ctg"], case["ref_len"]))
    open(sam, "w").write(case["sam"])
    ck = weights.save_weights(os.path.join(tmp, "model"), weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1))[:-4]
    base = ["--chkpnt_fn", ck, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"],
            "--samtools", FAKE_SAMTOOLS]
    plain, filtered = os.path.join(tmp, "plain.vcf"), os.path.join(tmp, "filtered.vcf")
    callVarBam.main(base + ["--call_fn", plain])
    callVarBam.main(base + ["--call_fn", filtered, "--overlap_filter", "device"])
    text = open(plain).read()
    assert len(text.splitlines()) > 30
    assert open(filtered).read() == ov.filter_vcf_text(text, "python")
