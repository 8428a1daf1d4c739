"""compare_vcf on the CPU: the host twin (hostsrc/host_compare.cpp over csrc/compare_core.h) against the plain-Python restatement of
docs/compare_vcf.md (tests/compare_cases.py), the hand-worked cases against their literals, the malformed rows, the report and the flags."""
import functools
import io
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import compare_cases as cc  # noqa: E402
from clair_amd import _capi, _hostapi, bgzf, compare_vcf as cv  # noqa: E402

B = _capi.COMPARE_SCAN_BLOCK
# (seed, lines of the calls, break_order): every size around the scan's workgroup, and both orders at the largest
GENERATED = [(100, 0, True), (101, 1, True), (102, 2, True), (103, B - 1, True), (104, B, False), (105, B + 1, True), (106, 3 * B + 5, False), (107, 3 * B + 5, True)]
RICH_FROM = 1000        # lines from which a generated pair must hold every outcome per type: a pair of 0, 1 or 2 lines cannot
FIELDS = ("ctg", "pos", "ref_off", "alt_off", "ref_len", "alt_len", "qual_bin", "copies", "type", "line")


@functools.lru_cache(maxsize=None)
def generated(seed, n, break_order):
    """-> the pair and its restatement, computed once and shared (nothing changes them)."""
    calls, truth, contigs, regions = cc.generate(seed, n, break_order)
    return dict(name="generated_%d_%d" % (seed, n), calls=calls, truth=truth, contigs=contigs, regions=regions), cc.restate_full(calls, truth, contigs, regions)


def run_case(case, backend, device=0):
    regions = None if case["regions"] is None else dict((c, cv.merge_intervals(v)) for c, v in case["regions"].items())
    return cv.compare(case["calls"].encode("latin-1"), case["truth"].encode("latin-1"), case["contigs"], regions, backend=backend, device=device)


def plain(result):
    """A result of compare_vcf.compare as plain Python: what two backends, or a backend and the restatement, must agree on."""
    out = {"counts": [int(v) for v in result["counts"]]}
    for side in cv.SIDES:
        out[side] = dict(stats=dict((k, result["stats"][side][k]) for k in cv.STATS), outcomes=[int(o) for o in result["outcomes"][side]],
                         records=[tuple(int(r[f]) for f in FIELDS) for r in result["records"][side]], permuted=result["stats"][side]["permuted"])
    return out


def plain_restated(full):
    out = {"counts": list(full["counts"])}
    for side in cv.SIDES:
        out[side] = dict(stats=dict((k, full["stats"][side][k]) for k in cv.STATS), outcomes=list(full["outcomes"][side]),
                         records=[tuple(r[f] for f in FIELDS) for r in full["records"][side]], permuted=1 - full["stats"][side]["sorted"])
    return out


def assert_same(got, want, name):
    assert got["counts"][:cc.AT_HIST] == want["counts"][:cc.AT_HIST], name
    for side in cv.SIDES:
        for key in ("stats", "permuted", "outcomes", "records"):
            assert got[side][key] == want[side][key], "%s: %s %s" % (name, side, key)
    assert got["counts"] == want["counts"], name


def test_layout_constants_agree():
    assert B == cc.SCAN_BLOCK and cv.N_COUNTS == cc.N_COUNTS and cv.TYPES == cc.TYPES and cv.OUTCOMES == cc.OUTCOMES
    assert (cv.AT_COUNTS, cv.AT_HIST, cv.AT_AT_LEAST, cv.AT_DROPS) == (cc.AT_COUNTS, cc.AT_HIST, cc.AT_AT_LEAST, cc.AT_DROPS)
    header = open(os.path.join(ROOT, "include", "clair_amd.h")).read()
    assert "#define CLAIR_COMPARE_COUNTS %d\n" % cv.N_COUNTS in header
    core = open(os.path.join(ROOT, "clair_amd", "csrc", "compare_core.h")).read()
    assert "sizeof(clair_compare_record) == 32" in core and cv.RECORD_DTYPE.itemsize == 32
    assert "BLOCK = 256 * ITEMS" in open(os.path.join(ROOT, "clair_amd", "csrc", "compare.hip")).read() and B == 256 * 8


@pytest.mark.parametrize("case", cc.crafted(), ids=lambda c: c["name"])
def test_host_twin_equals_the_restatement_on_crafted_cases(case):
    full = cc.restate_full(case["calls"], case["truth"], case["contigs"], case["regions"])
    assert_same(plain(run_case(case, "host")), plain_restated(full), case["name"])


@pytest.mark.parametrize("case", [c for c in cc.crafted() if c["expect"] is not None], ids=lambda c: c["name"])
def test_hand_worked_counts(case):
    counts = [int(v) for v in run_case(case, "host")["counts"]]
    got = {}
    for side in cv.SIDES:
        for t in cv.TYPES:
            cell = dict((k, v) for k, v in cc.side_counts(counts, side, t).items() if v)
            if cell:
                got[(side, t)] = cell
    assert got == case["expect"]


def test_crafted_cases_take_the_paths_they_are_named_for():
    by_name = dict((c["name"], c) for c in cc.crafted())
    moved = run_case(by_name["trimmed_pos_passes_successor"], "host")
    assert moved["stats"]["calls"]["sorted"] == 0 and moved["stats"]["calls"]["permuted"] == 1 and moved["stats"]["truth"]["permuted"] == 0
    assert [int(p) for p in moved["records"]["calls"]["pos"]] == [11, 13, 13] and [int(n) for n in moved["records"]["calls"]["line"]] == [2, 1, 3]
    run = run_case(by_name["long_run"], "host")
    assert len(set(run["records"]["calls"]["pos"])) == 1 and len(run["records"]["calls"]) > cc.JOIN_BLOCK
    assert run["stats"]["truth"]["sorted"] == 1        # equal keys in any allele order are in order


@pytest.mark.parametrize("seed,n,break_order", GENERATED)
def test_host_twin_equals_the_restatement_on_generated_pairs(seed, n, break_order):
    case, full = generated(seed, n, break_order)
    assert case["calls"].count("\n") == n
    if n >= RICH_FROM:
        assert cc.richness(full) == [], "seed %d is too thin" % seed
    assert_same(plain(run_case(case, "host")), plain_restated(full), case["name"])


def test_generated_sweep_takes_both_orders():
    permuted = [1 - generated(*g)[1]["stats"][side]["sorted"] for g in GENERATED if g[1] >= RICH_FROM for side in cv.SIDES]
    pairs = [max(permuted[i:i + 2]) for i in range(0, len(permuted), 2)]
    assert 1 in pairs and 0 in pairs
    drops = [sum(generated(*g)[1]["stats"]["calls"][k] for g in GENERATED) for k in ("symbolic", "unknown_contig")]
    assert min(drops) > 0


@pytest.mark.parametrize("what,bad", cc.MALFORMED, ids=[m[0] for m in cc.MALFORMED])
@pytest.mark.parametrize("side", cv.SIDES)
def test_malformed_row_names_side_and_line(what, bad, side):
    good = "##header\n" + cc.row("chr1", 4, "A", "C")
    texts = {"calls": good, "truth": good}
    texts[side] = good + bad + cc.row("chr1", 9, "A", "C")
    with pytest.raises(cc.RowError) as restated:
        cc.restate_full(texts["calls"], texts["truth"], ["chr1"], None)
    assert (restated.value.side, restated.value.line) == (side, 3)
    with pytest.raises(ValueError) as ei:
        cv.compare(texts["calls"].encode(), texts["truth"].encode(), ["chr1"], None, backend="host")
    assert str(ei.value).startswith("%s line 3: " % side)


def test_first_malformed_line_is_reported():
    text = cc.row("chr1", 4, "A", "C") + cc.MALFORMED[2][1] + cc.MALFORMED[0][1]
    with pytest.raises(ValueError) as ei:
        cv.compare(text.encode(), b"", ["chr1"], None, backend="host")
    assert str(ei.value).startswith("calls line 2: QUAL")


def test_other_row_errors_and_limits():
    for bad, what in ((cc.row("chr1", 5, "A", "C", "0/2"), "GT"), (cc.row("chr1", 5, "", "C"), "empty REF"), (cc.row("chr1", 5, "A", "C,", "1/2"), "empty REF or ALT"),
                      (cc.row("chr1", 2000000001, "A", "C"), "POS"), (cc.row("chr1", 5, "A", "C", "0/1/1"), "GT"), (cc.row("chr1", 5, "A", "C", "", 3), "GT"),
                      (cc.row("chr1", 5, "A", "C", "0/1", ".5"), "QUAL")):
        with pytest.raises(ValueError) as ei:
            cv.compare(bad.encode(), b"", ["chr1"], None, backend="host")
        assert str(ei.value).startswith("calls line 1: ") and what in str(ei.value), bad
    long_allele = "A" * 65536
    result = cv.compare((cc.row("chr1", 5, long_allele, "A") + cc.row("chr1", 9, long_allele[:-1], "A")).encode(), b"", ["chr1"], None, backend="host")
    assert result["stats"]["calls"]["too_long"] == 1 and [int(n) for n in result["records"]["calls"]["ref_len"]] == [65535]
    assert int(result["counts"][cv.AT_DROPS + 2]) == 1


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


def _cli(argv):
    out = io.StringIO()
    cv.main(argv, stdout=out)
    return out.getvalue()


def _mixed():
    return dict((c["name"], c) for c in cc.crafted())["mixed"]


def test_report_text_and_json_of_the_hand_worked_case(tmp_path):
    case = _mixed()
    calls, truth = _write(str(tmp_path / "calls.vcf"), case["calls"]), _write(str(tmp_path / "truth.vcf"), case["truth"])
    js, detail = str(tmp_path / "out.json"), str(tmp_path / "detail.tsv")
    text = _cli(["--vcf_fn", calls, "--truth_vcf_fn", truth, "--ctgName", "chr1", "--backend", "host", "--json_fn", js, "--detail_fn", detail])
    assert text == cc.MIXED_REPORT
    got = json.load(open(js))
    assert got["min_qual"] == 0 and got["contigs"] == ["chr1"]
    assert got["stats"]["calls"] == dict(lines=11, rows=9, records=7, symbolic=1, unknown_contig=1, too_long=0, sorted=1, permuted=0)
    assert got["counts"]["calls"]["SNP"] == dict(TP=2, GT=0, FP=1, FN=0, DUP=0, OUTSIDE=0) and got["counts"]["truth"]["MNP"]["DUP"] == 1
    rows = dict((r["type"], r) for r in got["rows"])
    assert [rows["ALL"][k] for k in ("truth", "calls", "TP", "FP", "FN", "GT", "best_qual")] == [6, 7, 3, 4, 3, 2, 1]
    assert rows["ALL"]["at_least"]["tp"][:10] == [3] * 9 + [2] and rows["ALL"]["at_least"]["tp"][1023] == 1 and len(rows["ALL"]["at_least"]["fp"]) == 1024
    assert rows["SNP"]["hist"]["fp"][1023] == 1 and rows["INS"]["at_least"]["gt"][:2] == [1, 0]
    assert open(detail).read() == ("calls\tchr1\t20\tAT\tA\t2\t12\tGT\ncalls\tchr1\t30\tC\tCGG\t1\t0\tFP\ncalls\tchr1\t30\tC\tCT\t1\t0\tGT\ncalls\tchr1\t40\tG\tT\t1\t1023\tFP\n"
                                   "truth\tchr1\t20\tAT\tA\t1\t0\tGT\ntruth\tchr1\t30\tC\tCT\t2\t0\tGT\ntruth\tchr1\t50\tT\tC\t1\t0\tFN\n")
    # the headline row at a cut-off: from QUAL 13 the DEL genotype mismatch is gone, from 31 the first SNP
    at_13 = _cli(["--vcf_fn", calls, "--truth_vcf_fn", truth, "--ctgName", "chr1", "--backend", "host", "--min_qual", "13"]).splitlines()
    assert at_13[1] == "SNP\t3\t3\t2\t1\t1\t0\t0.666667\t0.666667\t0.666667\t0\t0.666667" and at_13[3] == "DEL\t1\t0\t0\t0\t1\t0\t0.000000\t0.000000\t0.000000\t0\t0.000000"
    assert at_13[6] == "ALL\t6\t3\t2\t1\t4\t0\t0.666667\t0.333333\t0.444444\t1\t0.545455"


def test_var_fn_equals_truth_vcf_fn(tmp_path):
    case, full = generated(103, B - 1, True)
    calls, truth = _write(str(tmp_path / "calls.vcf"), case["calls"]), _write(str(tmp_path / "truth.vcf"), case["truth"])
    rows = []
    for r in full["records"]["truth"]:       # the truth's records, each as a GetTruth row of its own
        line = case["truth"].split("\n")[r["line"] - 1].rstrip("\r").split("\t")
        alt = case["truth"][r["alt_off"]:r["alt_off"] + r["alt_len"]]
        rows.append("%s %d %s %s %s\n" % (line[0], r["pos"], case["truth"][r["ref_off"]:r["ref_off"] + r["ref_len"]], alt, "1 1" if r["copies"] == 2 else "0 1"))
    var = _write(str(tmp_path / "truth.var"), "".join(rows))
    bed = _write(str(tmp_path / "conf.bed"), "".join("%s\t%d\t%d\n" % (c, s, e) for c, v in case["regions"].items() for s, e in v))
    common = ["--vcf_fn", calls, "--bed_fn", bed, "--backend", "host"]
    from_vcf, from_var = _cli(common + ["--truth_vcf_fn", truth]), _cli(common + ["--var_fn", var])
    assert from_vcf == from_var and from_vcf.count("\n") == 7
    assert cv.var_to_vcf(b"chr1 5 A C 0 1\n") == b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/1\n"
    # and the report is the restatement's: the ALL row from its counts
    by = full["counts"]
    tp = sum(cc.side_counts(by, "calls", t)["TP"] for t in cc.TYPES)
    assert int(from_vcf.splitlines()[6].split("\t")[3]) == tp > 100


def test_gzip_bgzf_and_several_call_files(tmp_path):
    case, _ = generated(103, B - 1, True)
    lines = case["calls"].splitlines(True)
    first, second = "".join(lines[:900]), "".join(lines[900:])
    truth = _write(str(tmp_path / "truth.vcf"), case["truth"])
    whole = _write(str(tmp_path / "calls.vcf"), case["calls"])
    a_gz, b_plain = str(tmp_path / "a.vcf.gz"), _write(str(tmp_path / "b.vcf"), second[:-1])      # the second file without its last line feed
    with bgzf.BgzfWriter(a_gz) as w:
        w.write(first.encode("latin-1"))
    assert open(a_gz, "rb").read(4) == b"\x1f\x8b\x08\x04" and cv.read_bytes(a_gz) == first.encode("latin-1")
    want = _cli(["--vcf_fn", whole, "--truth_vcf_fn", truth, "--backend", "host"])
    assert _cli(["--vcf_fn", a_gz, "--vcf_fn", b_plain, "--truth_vcf_fn", truth, "--backend", "host"]) == want
    truth_gz = str(tmp_path / "truth.vcf.gz")
    with bgzf.BgzfWriter(truth_gz) as w:
        w.write(case["truth"].encode("latin-1"))
    assert _cli(["--vcf_fn", whole, "--truth_vcf_fn", truth_gz, "--backend", "host"]) == want


def test_contig_order_from_fai_and_first_appearance(tmp_path):
    calls = cc.row("chr2", 5, "A", "C") + cc.row("chr1", 5, "A", "C")
    truth = cc.row("chr3", 5, "A", "C") + cc.row("chr1", 5, "A", "C")
    assert cv.contigs_of([calls.encode(), truth.encode()]) == ["chr2", "chr1", "chr3"]
    ref = str(tmp_path / "ref.fa")
    _write(ref + ".fai", "chr1\t100\t6\t60\t61\nchr2\t100\t120\t60\t61\n")
    assert cv.contigs_from_fai(ref) == ["chr1", "chr2"]
    c, t = _write(str(tmp_path / "c.vcf"), calls), _write(str(tmp_path / "t.vcf"), truth)
    js = str(tmp_path / "o.json")
    _cli(["--vcf_fn", c, "--truth_vcf_fn", t, "--ref_fn", ref, "--backend", "host", "--json_fn", js])
    got = json.load(open(js))
    assert got["contigs"] == ["chr1", "chr2"] and got["stats"]["calls"]["sorted"] == 0 and got["stats"]["calls"]["permuted"] == 1
    assert got["stats"]["truth"]["unknown_contig"] == 1 and got["counts"]["calls"]["SNP"]["TP"] == 1 and got["counts"]["calls"]["SNP"]["FP"] == 1
    _cli(["--vcf_fn", c, "--truth_vcf_fn", t, "--backend", "host", "--json_fn", js])
    assert json.load(open(js))["stats"]["calls"]["sorted"] == 1


def test_merge_intervals():
    assert cv.merge_intervals([(20, 30), (10, 20), (12, 15), (40, 50), (45, 60), (61, 70)]) == [(10, 30), (40, 60), (61, 70)]


def test_flag_errors(tmp_path, capsys):
    f = _write(str(tmp_path / "x.vcf"), cc.row("chr1", 5, "A", "C"))
    for argv, what in ((["--truth_vcf_fn", f], "--vcf_fn is required"), (["--vcf_fn", f], "exactly one of"),
                       (["--vcf_fn", f, "--truth_vcf_fn", f, "--var_fn", f], "exactly one of"),
                       (["--vcf_fn", f, "--truth_vcf_fn", f, "--min_qual", "1024"], "--min_qual"),
                       (["--vcf_fn", f, "--truth_vcf_fn", f, "--ref_fn", str(tmp_path / "none.fa")], ".fai not found"),
                       (["--vcf_fn", str(tmp_path / "none.vcf"), "--truth_vcf_fn", f], "none.vcf")):
        with pytest.raises(SystemExit) as ei:
            cv.main(argv + ["--backend", "host"], stdout=io.StringIO())
        assert str(ei.value.code).startswith("[ERROR] ") and what in str(ei.value.code), argv
    with pytest.raises(SystemExit):
        cv.main(["--vcf_fn", f, "--truth_vcf_fn", f, "--backend", "gpu"])
    assert "invalid choice" in capsys.readouterr().err


def test_submodule_is_dispatched():
    from clair_amd import __main__ as dispatcher
    assert dispatcher.SUBMODULES["compare_vcf"] == "clair_amd.compare_vcf"


def test_symbols_are_declared_and_exported():
    lib, host = _capi.load(), _hostapi.load()
    amd_h, host_h = open(os.path.join(ROOT, "include", "clair_amd.h")).read(), open(os.path.join(ROOT, "include", "clair_host.h")).read()
    names = ("create", "destroy", "set_contigs", "set_regions", "parse", "keys", "permute", "run", "counts", "records")
    for name in names + ("last_error",):
        assert "clair_compare_" + name in _capi.SYMBOLS and hasattr(lib, "clair_compare_" + name) and re.search(r"\bclair_compare_%s\(" % name, amd_h)
    for name in names:
        assert "clair_host_compare_" + name in _hostapi.SYMBOLS and hasattr(host, "clair_host_compare_" + name) and re.search(r"\bclair_host_compare_%s\(" % name, host_h)


def test_device_backend_without_a_device_names_the_host_twin():
    if _capi.load().clair_device_count() > 0:
        assert cv.pick_backend("auto") == "device"
        return
    assert cv.pick_backend("auto") == "host"
    with pytest.raises(RuntimeError) as ei:
        cv.compare(b"", b"", ["chr1"], None, backend="device")
    assert "no HIP device" in str(ei.value) and "--backend host" in str(ei.value)
