"""compare_vcf --left_align on the CPU: the host twin (hostsrc/host_compare.cpp over csrc/compare_core.h) against the literal restatement of
the left-alignment loop (tests/leftalign_cases.py), the hand-worked cases against their literals, the properties that hold by construction,
the command line, the ABI, and the twin once more as a stand-alone program under the address and undefined-behaviour sanitizers."""
import functools
import io
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import compare_cases as cc  # noqa: E402
import leftalign_cases as lc  # noqa: E402
from clair_amd import _capi, _hostapi, compare_vcf as cv  # noqa: E402

FIELDS = ("ctg", "pos", "ref_off", "alt_off", "ref_len", "alt_len", "qual_bin", "copies", "type", "line")
# (seed, lines asked for, break_order): seeds whose pairs are rich (test below); the first leaves a side out of order after the pass, the
# second has every side in order after it though not before; a small pair; an empty one
GENERATED = [(300, 1200, True), (300, 1200, False), (302, 1200, True), (310, 40, True), (311, 0, True)]
RICH_FROM = 1000


@functools.lru_cache(maxsize=None)
def generated(seed, n, break_order):
    """-> the pair as a case and its restatement, computed once and shared (nothing changes them)."""
    if n == 0:
        calls, truth, contigs, regions, reference = "", "", list(lc.CONTIGS), None, {"ctgA": "ACGT"}
    else:
        calls, truth, contigs, regions, reference = lc.generate(seed, n, break_order)
    case = dict(name="generated_%d_%d_%d" % (seed, n, break_order), calls=calls, truth=truth, contigs=contigs, regions=regions, reference=reference)
    return case, lc.restate_full(calls, truth, contigs, regions, reference)


@functools.lru_cache(maxsize=None)
def grid():
    calls, truth, contigs, reference, n_moved = lc.shift_grid()
    case = dict(name="shift_grid", calls=calls, truth=truth, contigs=contigs, regions=None, reference=reference)
    return case, lc.restate_full(calls, truth, contigs, None, reference), n_moved


def run_case(case, backend, device=0, left_align=True):
    regions = None if case["regions"] is None else dict((c, cv.merge_intervals(v)) for c, v in case["regions"].items())
    reference = dict((c, s.encode("latin-1")) for c, s in case["reference"].items()) if left_align else None
    return cv.compare(case["calls"].encode("latin-1"), case["truth"].encode("latin-1"), case["contigs"], regions, backend=backend, device=device, reference=reference)


def plain(result):
    """A left-aligned result of compare_vcf.compare as plain Python: what two backends, or a backend and the restatement, must agree on."""
    out = {"counts": [int(v) for v in result["counts"]]}
    for side in cv.SIDES:
        out[side] = dict(stats=dict((k, result["stats"][side][k]) for k in cv.STATS), outcomes=[int(o) for o in result["outcomes"][side]],
                         records=[tuple(int(r[f]) for f in FIELDS) for r in result["records"][side]], permuted=result["stats"][side]["permuted"],
                         left_align=dict(result["left_align"][side]), alleles=result["alleles"][side].decode("latin-1"))
    return out


def plain_restated(full):
    out = {"counts": list(full["counts"])}
    for side in cv.SIDES:
        out[side] = dict(stats=dict((k, full["stats"][side][k]) for k in cv.STATS), outcomes=list(full["outcomes"][side]),
                         records=[tuple(r[f] for f in FIELDS) for r in full["records"][side]], permuted=1 - full["left_align"][side]["sorted"],
                         left_align=dict(full["left_align"][side]), alleles=full["alleles"][side])
    return out


def assert_same(got, want, name):
    for side in cv.SIDES:
        for key in ("stats", "left_align", "permuted", "alleles", "records", "outcomes"):
            assert got[side][key] == want[side][key], "%s: %s %s" % (name, side, key)
    assert got["counts"] == want["counts"], name


def alleles_of(result, side):
    """[(pos, REF, ALT)] of a side's records after the pass, read where the records point: the arena."""
    text = result["alleles"][side]
    return [(int(r["pos"]), text[int(r["ref_off"]):int(r["ref_off"]) + int(r["ref_len"])].decode(), text[int(r["alt_off"]):int(r["alt_off"]) + int(r["alt_len"])].decode())
            for r in result["records"][side]]


def cells(counts):
    got = {}
    for side in cv.SIDES:
        for t in cv.TYPES:
            cell = dict((k, v) for k, v in cc.side_counts([int(v) for v in counts], side, t).items() if v)
            if cell:
                got[(side, t)] = cell
    return got


def nonzero(expect):
    return dict((k, dict((o, n) for o, n in v.items() if n)) for k, v in expect.items())


# -- the case the feature is for: it fails on a tree without the pass --------------------------------------------------------------------------
def test_homopolymer_deletion_written_at_the_right_end_matches_the_truth_at_the_left_end():
    case = dict((c["name"], c) for c in lc.crafted())["homopolymer_deletion_right_against_left"]
    without = run_case(case, "host", left_align=False)
    assert cells(without["counts"]) == {("calls", "DEL"): {"FP": 1}, ("truth", "DEL"): {"FN": 1}}
    aligned = run_case(case, "host")
    assert cells(aligned["counts"]) == {("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}}
    assert alleles_of(aligned, "calls") == alleles_of(aligned, "truth") == [(2, "CA", "C")]
    assert aligned["left_align"]["calls"] == dict(examined=1, shifted=1, ref_mismatch=0, at_contig_start=0, no_sequence=0, sorted=1, arena_bytes=3)


@pytest.mark.parametrize("case", lc.crafted(), ids=lambda c: c["name"])
def test_host_twin_equals_the_restatement_on_crafted_cases(case):
    full = lc.restate_full(case["calls"], case["truth"], case["contigs"], case["regions"], case["reference"])
    assert_same(plain(run_case(case, "host")), plain_restated(full), case["name"])


@pytest.mark.parametrize("case", lc.crafted(), ids=lambda c: c["name"])
def test_hand_worked_literals(case):
    expect, got = case["expect"], run_case(case, "host")
    assert cells(got["counts"]) == nonzero(expect["cells"])
    for side in cv.SIDES:
        assert alleles_of(got, side) == expect[side + "_records"], side
        for k, v in expect.get("la", {}).get(side, {}).items():
            assert got["left_align"][side][k] == v, (side, k)
        if "permuted" in expect:
            assert got["stats"][side]["permuted"] == expect["permuted"][side]
    if "without" in expect:
        assert cells(run_case(case, "host", left_align=False)["counts"]) == nonzero(expect["without"])


@pytest.mark.parametrize("seed,n,break_order", GENERATED)
def test_host_twin_equals_the_restatement_on_generated_pairs(seed, n, break_order):
    case, full = generated(seed, n, break_order)
    if n >= RICH_FROM:
        assert min(case["calls"].count("\n"), case["truth"].count("\n")) >= RICH_FROM
        assert lc.richness(full) == [], "seed %d is too thin" % seed
    assert_same(plain(run_case(case, "host")), plain_restated(full), case["name"])


def test_generated_sweep_takes_both_orders():
    broken, full = generated(300, 1200, True)[1], generated(300, 1200, False)[1]
    assert [broken["left_align"][s]["sorted"] for s in cv.SIDES] == [0, 0]
    # in order after the pass though not before it: the pass's flag supersedes the parse pass's, and nothing is permuted
    assert [full["left_align"][s]["sorted"] for s in cv.SIDES] == [1, 1] and [full["stats"][s]["sorted"] for s in cv.SIDES] == [0, 0]
    assert [run_case(generated(300, 1200, False)[0], "host")["stats"][s]["permuted"] for s in cv.SIDES] == [0, 0]


def test_shift_grid_on_the_host_twin():
    case, full, n_moved = grid()
    got = run_case(case, "host")
    assert_same(plain(got), plain_restated(full), "shift_grid")
    n = len(lc.LENGTHS) * len(lc.SHIFTS) * 2
    assert cells(got["counts"]) == {("calls", "INS"): {"TP": n}, ("calls", "DEL"): {"TP": n}, ("truth", "INS"): {"TP": n}, ("truth", "DEL"): {"TP": n}}
    assert got["left_align"]["calls"]["shifted"] == n_moved == 2 * n - 2 * len(lc.LENGTHS) and got["left_align"]["truth"]["shifted"] == 0
    # every distance of the grid is taken by some record
    moved = set(int(b) - int(a) for a, b in zip(got["records"]["calls"]["pos"], run_case(case, "host", left_align=False)["records"]["calls"]["pos"]))
    assert set(lc.SHIFTS) <= moved


def shaped_cases():
    """The shapes the device test takes, by name: here the twin takes them against the restatement."""
    B = _capi.COMPARE_SCAN_BLOCK
    cases = [lc.big_event(5000), lc.contig_boundaries()] + [lc.record_count(n) for n in (0, 1, B - 1, B, B + 1, 3 * B + 5)]
    return cases + [lc.record_count(B + 1, "none"), lc.record_count(B + 1, "all")]


@pytest.mark.parametrize("case", shaped_cases(), ids=lambda c: c["name"])
def test_host_twin_equals_the_restatement_on_the_shapes_of_the_device_test(case):
    full = lc.restate_full(case["calls"], case["truth"], case["contigs"], case["regions"], case["reference"])
    got = run_case(case, "host")
    assert_same(plain(got), plain_restated(full), case["name"])
    if case["name"] == "contig_boundaries":          # worked by hand: six cannot move, four end at position 1, and every call is the truth's
        assert (got["left_align"]["calls"]["at_contig_start"], got["left_align"]["calls"]["shifted"]) == (6, 4)
        assert cells(got["counts"]) == {("calls", "INS"): {"TP": 5}, ("calls", "DEL"): {"TP": 5}, ("truth", "INS"): {"TP": 5}, ("truth", "DEL"): {"TP": 5}}
    if case["name"] == "big_event_5000":
        assert [p for p, _, _ in alleles_of(got, "calls")] == [2, 2] and cells(got["counts"])[("calls", "DEL")] == {"TP": 1} and cells(got["counts"])[("calls", "INS")] == {"TP": 1}


# -- properties that hold by construction -------------------------------------------------------------------------------------------------------
def _as_vcf(result, side, contigs):
    return "".join(cc.row(contigs[int(r["ctg"])], pos, ref, alt, "1/1" if int(r["copies"]) == 2 else "0/1", int(r["qual_bin"])) for r, (pos, ref, alt) in zip(result["records"][side], alleles_of(result, side)))


def test_properties_on_generated_records():
    case, full = generated(302, 1200, True)
    got, trimmed = run_case(case, "host"), run_case(case, "host", left_align=False)
    n_aligned, upper = 0, dict((c, cc.up(s)) for c, s in case["reference"].items())
    for side in cv.SIDES:
        # the lengths never exceed the trimmed ones: per line of the text they are the trimmed ones
        per_line = [sorted((int(r["line"]), int(r["ref_len"]), int(r["alt_len"]), int(r["copies"])) for r in result["records"][side]) for result in (got, trimmed)]
        assert per_line[0] == per_line[1]
        for r, (pos, ref, alt), restated in zip(got["records"][side], alleles_of(got, side), full["records"][side]):
            G = upper.get(case["contigs"][int(r["ctg"])], "")
            if restated["what"] == "aligned":
                n_aligned += 1
                assert lc.haplotype(G, pos, ref, alt) == lc.haplotype(G, restated["pos_before"], restated["ref_before"], restated["alt_before"])
                assert lc.left_align(G, pos, ref, alt) == ("aligned", pos, ref, alt)
            else:
                assert (pos, ref, alt) == (restated["pos_before"], restated["ref_before"], restated["alt_before"])
    assert n_aligned > 500
    # a second pass, through the twin itself: the aligned records written out as a VCF and aligned again
    again = dict(case, calls=_as_vcf(got, "calls", case["contigs"]), truth=_as_vcf(got, "truth", case["contigs"]))
    second = run_case(again, "host")
    for side in cv.SIDES:
        assert second["left_align"][side]["shifted"] == 0 and second["stats"][side]["permuted"] == 0
        assert alleles_of(second, side) == alleles_of(got, side)
        assert [int(o) for o in second["outcomes"][side]] == [int(o) for o in got["outcomes"][side]]


@pytest.mark.parametrize("unit,copies", [("A", 9), ("AC", 5), ("ACG", 4), ("AACG", 3), (lc._unit(63, 1), 3), (lc._unit(64, 2), 3), (lc._unit(65, 3), 3)], ids=lambda v: str(v)[:8])
def test_all_placements_of_one_event_normalise_to_one(unit, copies):
    G = "TTGCT" + unit * copies + "TGCTT"
    s, u = 6, len(unit)
    for kind in ("INS", "DEL"):
        room = (copies - 1) * u if kind == "DEL" else copies * u
        rows = [lc._write_event(None, G, s, unit, copies, kind, 1, t, behind) for t in range(room + 1) for behind in (False, True)]
        text = "".join(cc.row("chr1", pos, ref, alt) for pos, ref, alt in rows)
        got = cv.compare(text.encode(), b"", ["chr1"], None, backend="host", reference={"chr1": G.encode()})
        assert len(set((pos, ref, alt) for pos, ref, alt in rows)) > room          # every phase was written, in both forms
        assert len(set(alleles_of(got, "calls"))) == 1, kind
        want = (s - 1, "T", "T" + unit) if kind == "INS" else (s - 1, "T" + unit, "T")
        assert alleles_of(got, "calls")[0] == want
        assert sorted(int(o) for o in got["outcomes"]["calls"]) == [cc.FP] + [cc.DUP] * (len(rows) - 1)


def test_the_search_reads_its_own_contig_only():
    """chr1 ends with the repeat chr2 begins with: a deletion in chr2's head stops at chr2's first base (at_contig_start, or one base short of
    it a shift that ends at position 1) whatever chr1's tail holds."""
    reference = {"chr1": "GGT" + "A" * 70, "chr2": "A" * 70 + "CG", "chr3": "C" + "A" * 70 + "CG"}
    calls = cc.row("chr1", 60, "AA", "A") + cc.row("chr2", 60, "AA", "A") + cc.row("chr3", 60, "AA", "A")
    got = cv.compare(calls.encode(), b"", ["chr1", "chr2", "chr3"], None, backend="host", reference=dict((c, s.encode()) for c, s in reference.items()))
    assert alleles_of(got, "calls") == [(3, "TA", "T"), (60, "AA", "A"), (1, "CA", "C")]
    assert got["left_align"]["calls"] == dict(examined=3, shifted=2, ref_mismatch=0, at_contig_start=1, no_sequence=0, sorted=1, arena_bytes=9)


def test_position_zero_and_long_alleles():
    # POS 0 is a valid POS for the parser: no reference base is there, so it is a ref_mismatch, not a read before the contig
    got = cv.compare(cc.row("chr1", 0, "AA", "A").encode(), b"", ["chr1"], None, backend="host", reference={"chr1": b"AAAA"})
    assert got["left_align"]["calls"]["ref_mismatch"] == 1 and alleles_of(got, "calls") == [(0, "AA", "A")]
    # the longest allele a record can have, in a run of its own period
    unit = lc._unit(65534, 9)
    G = "T" + unit * 2 + "T"
    got = cv.compare(cc.row("chr1", 1 + 65534, unit[-1] + unit, unit[-1]).encode(), cc.row("chr1", 1, "T" + unit, "T").encode(), ["chr1"], None, backend="host",
                     reference={"chr1": G.encode()})
    assert cells(got["counts"]) == {("calls", "DEL"): {"TP": 1}, ("truth", "DEL"): {"TP": 1}}
    assert int(got["records"]["calls"]["pos"][0]) == 1 and got["left_align"]["calls"]["arena_bytes"] == 65536


# -- the native interface ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_in_the_tables():
    lib, host = _capi.load(), _hostapi.load()
    amd_h, host_h = open(os.path.join(ROOT, "include", "clair_amd.h")).read(), open(os.path.join(ROOT, "include", "clair_host.h")).read()
    for name in ("set_reference", "left_align", "allele_text"):
        assert "clair_compare_" + name in _capi.SYMBOLS and hasattr(lib, "clair_compare_" + name) and re.search(r"^int clair_compare_%s\(" % name, amd_h, flags=re.M)
        assert "clair_host_compare_" + name in _hostapi.SYMBOLS and hasattr(host, "clair_host_compare_" + name)
        assert re.search(r"^int clair_host_compare_%s\(" % name, host_h, flags=re.M)
    assert lib.clair_abi_version() == 6 and host.clair_host_abi_version() == 6
    assert _capi.SIGNATURES["clair_compare_set_reference"] == _capi.SIGNATURES["clair_compare_set_contigs"]
    core = open(os.path.join(ROOT, "clair_amd", "csrc", "compare_core.h")).read()
    for k, name in enumerate(cv.LEFT_ALIGN_STATS):
        assert re.search(r"CLAIR_CMP_LA_%s = %d\b" % ({"arena_bytes": "ARENA"}.get(name, name.upper()), k), core), name


def test_calls_out_of_order_are_refused():
    native = cv._Native("host")
    names, offsets, stats = np.frombuffer(b"chr1", dtype=np.uint8), np.array([0, 4], dtype=np.int64), np.zeros(8, dtype=np.int64)
    text = np.frombuffer(cc.row("chr1", 3, "AA", "A").encode(), dtype=np.uint8)
    seq = np.frombuffer(b"GCAAAT", dtype=np.uint8)
    try:
        native.call("set_contigs", cv._address(names), cv._address(offsets), 1)
        native.call("parse", 0, cv._address(text), len(text), cv._address(stats))
        with pytest.raises(ValueError, match="set the reference first"):
            native.call("left_align", 0, cv._address(stats))
        with pytest.raises(ValueError, match="2 contigs, the contig table has 1"):
            native.call("set_reference", cv._address(seq), cv._address(np.array([0, 3, 6], dtype=np.int64)), 2)
        with pytest.raises(ValueError, match="was not left-aligned"):
            native.call("allele_text", 0, cv._address(np.zeros(8, dtype=np.uint8)))
        with pytest.raises(ValueError, match="no parsed text"):
            native.call("left_align", 1, cv._address(stats))
        native.call("set_reference", cv._address(seq), cv._address(np.array([0, 6], dtype=np.int64)), 1)
        native.call("left_align", 0, cv._address(stats))
        assert [int(v) for v in stats] == [1, 1, 0, 0, 0, 1, 3, 0]
        with pytest.raises(ValueError, match="left-aligned already"):
            native.call("left_align", 0, cv._address(stats))
        native.call("parse", 0, cv._address(text), len(text), cv._address(stats))       # a new parse starts over
        native.call("left_align", 0, cv._address(stats))
    finally:
        native.close()


# -- the command line ---------------------------------------------------------------------------------------------------------------------------
def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


def _cli(argv):
    out = io.StringIO()
    cv.main(argv, stdout=out)
    return out.getvalue()


def write_fasta(path, reference, width=7, names=None):
    """A FASTA of `width` bases per line and its .fai; names: the order, and more contigs than the reference has are left out of both."""
    at, fai = 0, []
    with open(path, "w") as f:
        for name in names or list(reference):
            seq = reference[name]
            head = ">%s some description\n" % name
            f.write(head)
            at += len(head)
            fai.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), at, width, width + 1))
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")
                at += len(seq[i:i + width]) + 1
    _write(path + ".fai", "".join(fai))
    return path


def case_files(tmp_path, case, width=7):
    paths = dict(calls=_write(str(tmp_path / "calls.vcf"), case["calls"]), truth=_write(str(tmp_path / "truth.vcf"), case["truth"]),
                 ref=write_fasta(str(tmp_path / "ref.fa"), case["reference"], width, [c for c in case["contigs"] if c in case["reference"]]))
    if case["regions"] is not None:
        paths["bed"] = _write(str(tmp_path / "conf.bed"), "".join("%s\t%d\t%d\n" % (c, s, e) for c, v in case["regions"].items() for s, e in v))
    return paths


def cli_outputs(tmp_path, paths, backend, tag, extra=("--left_align",)):
    argv = ["--vcf_fn", paths["calls"], "--truth_vcf_fn", paths["truth"], "--ref_fn", paths["ref"], "--backend", backend, "--min_qual", "10",
            "--json_fn", str(tmp_path / (tag + ".json")), "--detail_fn", str(tmp_path / (tag + ".tsv"))] + list(extra)
    if "bed" in paths:
        argv += ["--bed_fn", paths["bed"]]
    return _cli(argv), open(str(tmp_path / (tag + ".json"))).read(), open(str(tmp_path / (tag + ".tsv"))).read()


def test_load_reference(tmp_path):
    reference = {"chr1": "GCAAAAATCGGTA", "chr2": "acgtNNacg", "chr3": "A" * 7, "chr4": "C" * 15}
    fa = write_fasta(str(tmp_path / "ref.fa"), reference, 7)
    assert cv.load_reference(fa, ["chr2", "chr4", "chrNone", "chr1", "chr3"]) == dict((c, s.encode()) for c, s in reference.items())     # the case is kept
    assert cv.load_reference(fa, ["chr2"]) == {"chr2": b"acgtNNacg"}
    _write(fa + ".fai", "chr1\t500\t24\t7\t8\n")             # more than the file holds
    with pytest.raises(ValueError, match="bases where its .fai says 500"):
        cv.load_reference(fa, ["chr1"])


def test_flag_errors(tmp_path):
    f = _write(str(tmp_path / "x.vcf"), cc.row("chr1", 5, "A", "C"))
    fa = _write(str(tmp_path / "nofai.fa"), ">chr1\nACGT\n")
    for argv, what in ((["--vcf_fn", f, "--truth_vcf_fn", f, "--left_align"], "--left_align needs --ref_fn"),
                       (["--vcf_fn", f, "--truth_vcf_fn", f, "--left_align", "--ref_fn", fa], ".fai not found")):
        with pytest.raises(SystemExit) as ei:
            cv.main(argv + ["--backend", "host"], stdout=io.StringIO())
        assert str(ei.value.code).startswith("[ERROR] ") and what in str(ei.value.code), argv


def test_command_line_on_a_generated_pair(tmp_path, capsys):
    case, full = generated(300, 1200, True)
    paths = case_files(tmp_path, case)
    first, second = cli_outputs(tmp_path, paths, "host", "a"), cli_outputs(tmp_path, paths, "host", "b")
    assert first == second
    # the fai names the contigs that have a sequence: the third is an unknown contig here, on the command line
    table = [c for c in case["contigs"] if c in case["reference"]]
    want = lc.restate_full(case["calls"], case["truth"], table, case["regions"], case["reference"])
    err = capsys.readouterr().err
    for side in cv.SIDES:
        la = want["left_align"][side]
        assert la["ref_mismatch"] + la["at_contig_start"] > 0
        assert ("[WARNING] %s: %d indel records not left-aligned: %d whose REF differs from the reference, %d at a contig start, %d on contigs without sequence\n"
                % (side, la["ref_mismatch"] + la["at_contig_start"] + la["no_sequence"], la["ref_mismatch"], la["at_contig_start"], la["no_sequence"])) in err
    got = json.loads(first[1])
    assert got["left_align"] == want["left_align"] and got["contigs"] == table
    assert got["stats"]["calls"]["permuted"] == 1 - want["left_align"]["calls"]["sorted"] and got["stats"]["calls"]["unknown_contig"] > 100
    assert first[0] == cv.report_text(cv.summary(np.array(want["counts"], dtype=np.int64), 10))
    # the detail file: the aligned alleles, upper-cased, of every FP, FN and GT record
    lines = ["%s\t%s\t%d\t%s\t%s\t%d\t%d\t%s\n" % (side, table[r["ctg"]], r["pos"], r["ref"], r["alt"], r["copies"], r["qual_bin"], cc.OUTCOMES[o])
             for side in cv.SIDES for r, o in zip(want["records"][side], want["outcomes"][side]) if o in (cc.GT, cc.FP, cc.FN)]
    assert first[2] == "".join(lines) and len(lines) > 100
    # without the flag: today's report, and no trace of the pass
    plain_run = cli_outputs(tmp_path, paths, "host", "c", extra=())
    assert "left_align" not in json.loads(plain_run[1]) and plain_run[0] != first[0]
    assert plain_run[0] == cv.report_text(cv.summary(np.array(cc.restate_full(case["calls"], case["truth"], table, case["regions"])["counts"], dtype=np.int64), 10))
    rows = dict((r["type"], r) for r in got["rows"])
    plain_rows = dict((r["type"], r) for r in json.loads(plain_run[1])["rows"])
    assert rows["INDEL"]["TP"] > plain_rows["INDEL"]["TP"] + 100 and rows["SNP"] == plain_rows["SNP"]


def test_left_align_on_a_pair_without_indels_prints_the_same_report(tmp_path, capsys):
    reference = {"chr1": "GCAAAAATCGGTA"}
    calls = cc.row("chr1", 4, "a", "T", "0/1", 20) + cc.row("chr1", 9, "cg", "ta", "1/1", 30) + cc.row("chr1", 12, "T", "G", "0/1", 5)
    truth = cc.row("chr1", 4, "A", "T") + cc.row("chr1", 9, "CG", "TA") + cc.row("chr1", 13, "A", "G")
    paths = case_files(tmp_path, dict(calls=calls, truth=truth, reference=reference, contigs=["chr1"], regions=None))
    with_flag, without = cli_outputs(tmp_path, paths, "host", "a"), cli_outputs(tmp_path, paths, "host", "b", extra=())
    assert with_flag[0] == without[0] and with_flag[0].splitlines()[1].startswith("SNP\t2\t1\t1\t0\t1\t0\t")
    assert json.loads(with_flag[1])["left_align"]["calls"] == dict(examined=0, shifted=0, ref_mismatch=0, at_contig_start=0, no_sequence=0, sorted=1, arena_bytes=8)
    assert with_flag[2] == without[2].replace("\tcg\tta\t", "\tCG\tTA\t") != without[2]          # the arena is upper-cased, the text is as written
    assert capsys.readouterr().err == ""


# -- the twin under the sanitizers, as a program of its own ----------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17"]


def test_host_twin_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    probe = _write(str(tmp_path / "probe.cpp"), "int main() { return 0; }\n")
    if subprocess.run([cxx] + SANITIZE + [probe, "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    program = str(tmp_path / "left_align_sanitize")
    subprocess.check_call([cxx] + SANITIZE + ["-Wall", os.path.join(HERE, "left_align_sanitize.cpp"), os.path.join(ROOT, "clair_amd", "hostsrc", "host_compare.cpp"),
                                               "-o", program])
    crafted = dict((c["name"], c) for c in lc.crafted())
    for n, case in enumerate((crafted["would_pass_position_1"], crafted["contig_without_sequence"], crafted["deletion_past_contig_end"], generated(310, 40, True)[0],
                              generated(302, 1200, True)[0])):
        if case["regions"] is not None:
            case = dict(case, regions=None)              # the program sets no regions
        calls, truth = _write(str(tmp_path / ("calls%d.vcf" % n)), case["calls"]), _write(str(tmp_path / ("truth%d.vcf" % n)), case["truth"])
        ref = _write(str(tmp_path / ("ref%d.tsv" % n)), "".join("%s\t%s\n" % (c, case["reference"].get(c, "")) for c in case["contigs"]))
        done = subprocess.run([program, calls, truth, ref], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                              env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        want = run_case(case, "host")
        lines = done.stdout.splitlines()
        for side, name in enumerate(cv.SIDES):
            la = want["left_align"][name]
            assert lines[side] == "left_align %d: %s 0 %s" % (side, " ".join(str(la[k]) for k in cv.LEFT_ALIGN_STATS), want["alleles"][name].decode())
        assert lines[2] == "counts: " + " ".join(str(int(v)) for v in want["counts"][:cv.AT_HIST])
