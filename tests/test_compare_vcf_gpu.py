"""compare_vcf on the device (csrc/compare.hip) against its host twin, bit for bit: counts, outcomes, records and the sortedness flag, on the
crafted cases and generated pairs of tests/compare_cases.py; through the command line; and end to end on a VCF callVarBam wrote."""
import io
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compare_cases as cc  # noqa: E402
from clair_amd import compare_vcf as cv  # noqa: E402
from test_compare_vcf import GENERATED, assert_same, generated, plain, run_case  # noqa: E402

FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))


@pytest.mark.parametrize("case", cc.crafted(), ids=lambda c: c["name"])
def test_device_equals_the_host_twin_on_crafted_cases(case):
    assert_same(plain(run_case(case, "device")), plain(run_case(case, "host")), case["name"])


@pytest.mark.parametrize("seed,n,break_order", GENERATED)
def test_device_equals_the_host_twin_on_generated_pairs(seed, n, break_order):
    case, _ = generated(seed, n, break_order)
    assert_same(plain(run_case(case, "device")), plain(run_case(case, "host")), case["name"])


def test_device_equals_the_host_twin_when_many_workgroups_flush():
    """About 20 000 lines: the counting pass has some ten workgroups per side, each adding its histogram to the same block."""
    calls, truth, contigs, regions = cc.generate(108, 20000, True)
    case = dict(name="generated_20000", calls=calls, truth=truth, contigs=contigs, regions=regions)
    device, host = run_case(case, "device"), run_case(case, "host")
    assert host["stats"]["calls"]["records"] > 8 * 2048 and host["stats"]["calls"]["permuted"] == 1
    assert int(host["counts"][cv.AT_AT_LEAST:cv.AT_DROPS].max()) > 1000
    assert_same(plain(device), plain(host), case["name"])


def _cli(argv):
    out = io.StringIO()
    cv.main(argv, stdout=out)
    return out.getvalue()


def test_command_line_prints_the_same_on_both_backends(tmp_path):
    case, _ = generated(105, cc.SCAN_BLOCK + 1, True)
    paths = {}
    for name, text in (("calls.vcf", case["calls"]), ("truth.vcf", case["truth"]),
                       ("conf.bed", "".join("%s\t%d\t%d\n" % (c, s, e) for c, v in case["regions"].items() for s, e in v))):
        paths[name] = str(tmp_path / name)
        with open(paths[name], "w") as f:
            f.write(text)
    outputs = {}
    for backend in ("device", "host", "auto"):
        argv = ["--vcf_fn", paths["calls.vcf"], "--truth_vcf_fn", paths["truth.vcf"], "--bed_fn", paths["conf.bed"], "--backend", backend, "--min_qual", "10",
                "--json_fn", str(tmp_path / (backend + ".json")), "--detail_fn", str(tmp_path / (backend + ".tsv"))]
        outputs[backend] = (_cli(argv), open(str(tmp_path / (backend + ".json"))).read(), open(str(tmp_path / (backend + ".tsv"))).read())
    assert outputs["device"] == outputs["host"] == outputs["auto"]
    assert outputs["device"][0].count("\n") == 7 and len(outputs["device"][2]) > 1000


def test_end_to_end_on_a_vcf_callVarBam_wrote(tmp_path):
    """callVarBam on the alignments of tests/test_overlap_gpu.py; its VCF against itself, then against a copy with known damage."""
    import pileup_synth
    from clair_amd import callVarBam, weights
    tmp = str(tmp_path)
    case = pileup_synth.synth_case(seed=91)
    fa, sam, vcf = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.sam"), os.path.join(tmp, "calls.vcf")
    open(fa, "w").write(case["fasta"])
    open(fa + ".fai", "w").write("%s\t%d\t6\t60\t61\nchrOther\t120\t3100\t120\t121\n" % (case["ctg"], case["ref_len"]))
    open(sam, "w").write(case["sam"])
    ck = weights.save_weights(os.path.join(tmp, "model"), weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1))[:-4]
    callVarBam.main(["--chkpnt_fn", ck, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"],
                     "--samtools", FAKE_SAMTOOLS, "--call_fn", vcf])
    text = open(vcf).read()
    contigs = [case["ctg"], "chrOther"]
    # against itself: every record is a TP (or the repeat of one), F1 = 1 at cut-off 0
    own = cv.compare(text.encode(), text.encode(), contigs, None, backend="device")
    rows = dict((r["type"], r) for r in cv.summary(own["counts"]))
    n = rows["ALL"]["truth"]
    assert n > 20 and set(int(o) for o in own["outcomes"]["calls"]) <= {cc.TP, cc.DUP}
    assert (rows["ALL"]["TP"], rows["ALL"]["FP"], rows["ALL"]["FN"], rows["ALL"]["GT"]) == (n, 0, 0, 0)
    assert (rows["ALL"]["F1"], rows["ALL"]["best_qual"], rows["ALL"]["best_F1"]) == (1.0, 0, 1.0)
    # the damage: rows with one record of their own, a plain diploid genotype and no repeat
    full = cc.restate_full(text, text, contigs, None)
    per_line = {}
    for r, o in zip(full["records"]["calls"], full["outcomes"]["calls"]):
        per_line.setdefault(r["line"], []).append(o)
    lines = text.split("\n")
    simple = [k for k, outcomes in sorted(per_line.items()) if outcomes == [cc.TP] and lines[k - 1].split("\t")[9].split(":")[0] in ("0/1", "1/1")]
    assert len(simple) >= 7
    deleted, regenotyped, shifted = simple[0:3], simple[3:5], simple[5:7]
    damaged = []
    for k, line in enumerate(lines, 1):
        cols = line.split("\t")
        if k in deleted:
            continue
        if k in regenotyped:
            sample = cols[9].split(":")
            sample[0] = "1/1" if sample[0] == "0/1" else "0/1"
            cols[9] = ":".join(sample)
        if k in shifted:
            cols[1] = str(int(cols[1]) + 1000000)
        damaged.append("\t".join(cols))
    got = cv.compare("\n".join(damaged).encode(), text.encode(), contigs, None, backend="device")
    assert got["stats"]["calls"]["permuted"] == 1          # the shifted rows are out of order now
    by = [int(v) for v in got["counts"]]
    calls = dict((o, sum(cc.side_counts(by, "calls", t)[o] for t in cc.TYPES)) for o in cc.OUTCOMES)
    truth = dict((o, sum(cc.side_counts(by, "truth", t)[o] for t in cc.TYPES)) for o in cc.OUTCOMES)
    assert (calls["FP"], calls["GT"], calls["TP"]) == (2, 2, n - 7) and (truth["FN"], truth["GT"], truth["TP"]) == (3 + 2, 2, n - 7)
    all_row = dict((r["type"], r) for r in cv.summary(got["counts"]))["ALL"]
    assert (all_row["truth"], all_row["TP"], all_row["FP"], all_row["FN"], all_row["GT"]) == (n, n - 7, 4, 7, 2)
