"""markdup_bam on the CPU (docs/markdup_bam.md): the host backend (hostsrc/host_markdup.cpp over csrc/markdup_core.h) against the rule
restated in plain Python (tests/markdup_cases.py), the file's bytes under every batch size, segment and block layout, removal, idempotence,
--index, the error verdicts, the command line, the symbol tables, and the host side once more as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import index_bam_cases as ic  # noqa: E402
import markdup_cases as mc  # noqa: E402

from clair_amd import _capi, _hostapi, index_bam, sort_bam  # noqa: E402
from clair_amd import markdup_bam as mb  # noqa: E402
from clair_amd._hostapi import BamError  # noqa: E402

ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the shuffled BAM written three ways, the yardstick's verdicts (computed once), and the marked file of the plain call"""
    tmp = tmp_path_factory.mktemp("markdup")
    b = mc.bam()
    paths = {}
    for way, kw in mc.WAYS.items():
        paths[way] = str(tmp / (way + ".bam"))
        b.write(paths[way], index=False, **kw)
    duplicate, counts = mc.resolve(b.records)
    out = str(tmp / "marked.bam")
    result = mb.markdup_bam(paths["straddle"], out, backend="host")
    return dict(bam=b, paths=paths, marked=out, result=result, duplicate=duplicate, counts=counts, tmp=tmp)


def _records(stream, header_len):
    out, at = [], header_len
    while at < len(stream):
        size = 4 + struct.unpack_from("<I", stream, at)[0]
        out.append(stream[at:at + size])
        at += size
    assert at == len(stream)
    return out


# -- the fixture and the rule -----------------------------------------------------------------------------------------------------------------
def test_the_fixture_has_what_the_issue_lists(case):
    records, duplicate = case["bam"].records, case["duplicate"]
    by_name = {}
    for i, r in enumerate(records):
        by_name.setdefault(r.qname, []).append(i)
    one = lambda name: [i for i in by_name[name] if mc.examined(records[i])]     # noqa: E731
    end = lambda name: mc.end_of(records[one(name)[0]])                           # noqa: E731
    assert 2300 <= len(records) <= 2500 and len(records) - mc.TINY < 400
    # equal unclipped ends through clips, different positions; a negative one
    assert end("fwd_plain") == end("fwd_soft") == end("fwd_hard_soft") == (0, 999, False)
    assert len({records[one(n)[0]].pos for n in ("fwd_plain", "fwd_soft", "fwd_hard_soft")}) == 3
    assert [duplicate[one(n)[0]] for n in ("fwd_plain", "fwd_soft", "fwd_hard_soft")] == [True, True, False]
    assert end("negative_a") == end("negative_b") == (0, -8, False) and duplicate[one("negative_a")[0]] and not duplicate[one("negative_b")[0]]
    assert end("rev_plain") == end("rev_short") == end("rev_soft") == (0, 2048, True) != end("rev_other_end")
    assert [duplicate[one(n)[0]] for n in ("rev_plain", "rev_short", "rev_soft", "rev_other_end")] == [False, True, True, False]      # 1500, 1320, 1395 on one end
    # pairs in four orientations; the swapped FR pair has the FR pairs' signature and the best score
    for tag, strands in (("FR", [False, True]), ("RF", [True, False]), ("FF", [False, False]), ("RR", [True, True])):
        members = [one("pair%s_%d" % (tag, j)) for j in range(3)]
        assert all(len(m) == 2 for m in members)
        assert sorted(mc.end_of(records[i])[2] for i in members[0]) == sorted(strands)
        assert len({tuple(sorted(mc.end_of(records[i]) for i in m)) for m in members}) == 1
        best = "pairFR_swapped" if tag == "FR" else "pair%s_1" % tag
        assert [all(duplicate[i] for i in m) for m in members] == [True, best != "pair%s_1" % tag, True] and not any(duplicate[i] for i in one(best))
    assert {records[i].tid for i in one("two_refs_a")} == {0, 1} and all(duplicate[i] for i in one("two_refs_a")) and not any(duplicate[i] for i in one("two_refs_b"))
    # ties: the lower index wins
    a, b = one("tie_frag_a")[0], one("tie_frag_b")[0]
    assert mc.score_of(records[a]) == mc.score_of(records[b]) and duplicate[max(a, b)] and not duplicate[min(a, b)]
    ties = mc.pair_ties(records)
    assert ties[0][1] == ties[1][1] and ties[0][2] == ties[1][2] and ties[0][3] != ties[1][3]
    assert [t[4] for t in ties] == [t[3] != min(x[3] for x in ties) for t in ties]
    assert duplicate[one("frag_at_pair_end")[0]] and mc.score_of(records[one("frag_at_pair_end")[0]]) > 38 * 50      # better than any one record of the pairs there
    assert sum(duplicate[i] for n in ("mate_unmapped_0", "mate_unmapped_1") for i in one(n)) == 1 and not duplicate[one("mate_missing")[0]]
    assert sorted(duplicate[i] for i in one("multi")) == [False] * 5 and not duplicate[one("both_numbers")[0]]
    # records that are not examined carry what they carried
    stale = [r for r in records if not mc.examined(r) and r.flag & 0x400]
    assert {bool(r.flag & 0x100) for r in stale} == {True, False} and any(r.flag & 0x800 for r in stale) and any(r.tid < 0 for r in stale)
    assert records[one("stale_cleared")[0]].flag & 0x400 and not duplicate[one("stale_cleared")[0]]
    assert records[one("stale_kept_a")[0]].flag & 0x400 and duplicate[one("stale_kept_a")[0]]
    assert sum(r.tid < 0 for r in records) >= 10
    # qualities
    assert records[one("absent_a")[0]].qual is None and sum(duplicate[i] for n in ("absent_a", "absent_b") for i in one(n)) == 1
    assert duplicate[one("absent_vs")[0]] and not duplicate[one("present_vs")[0]]
    assert [mc.score_of(records[one(n)[0]]) for n in ("many_14", "few_15", "mixed")] == [0, 150, 46]
    assert [duplicate[one(n)[0]] for n in ("many_14", "few_15", "mixed")] == [True, False, True]
    assert len(records[one("long")[0]].seq) > 70000 and not duplicate[one("long")[0]] and duplicate[one("long_rival")[0]]
    for name, rival in (("cg_forward", "cg_forward_rival"), ("cg_reverse", "cg_reverse_rival")):
        r = records[one(name)[0]]
        assert len(r.cigar) > 65535 and r.cigar[0][1] == r.cigar[-1][1] == 4 and end(name) == end(rival) and end(name)[1] not in (r.pos, r.end() - 1)
        assert not duplicate[one(name)[0]] and duplicate[one(rival)[0]]               # flagged only because the long read's end is the rival's
        assert struct.unpack_from("<H", r.encode(), 16)[0] == 2                        # stored as the placeholder
    tiny = [i for i, r in enumerate(records) if r.qname.startswith("tiny")]
    assert len(tiny) > 2048 and sum(not duplicate[i] for i in tiny) == 1
    assert any(b < a for a, b in zip([r.pos for r in records], [r.pos for r in records][1:]))      # and the input is in no order


def test_the_twins_bits_and_counts_are_the_yardsticks(case):
    b = case["bam"]
    stream, starts = mc.stream_of(b)
    got = mb.host_debug_summary(stream, starts, len(mc.REFS))
    want = mc.summaries(b.records, mb.SUMMARY)
    for field in mb.SUMMARY.names:
        assert np.array_equal(got[field], want[field]), field
    assert np.array_equal(mb.host_debug_resolve(got), np.array(case["duplicate"], dtype=np.uint8))
    r = case["result"]
    assert {k: r[k] for k in case["counts"]} == case["counts"]
    assert (r["written"], r["backend"], r["path"]) == (len(b.records), "host", case["marked"])
    assert r["bytes_in"] == os.path.getsize(case["paths"]["straddle"]) and r["bytes_out"] == os.path.getsize(case["marked"])
    assert 0 < r["duplicate_pairs"] < r["pairs"] and 0 < r["duplicate_fragments"] < r["fragments"] and r["examined"] < r["records"]


@pytest.mark.parametrize("kind", ["mixed", "all_equal", "all_distinct", "equal_scores"])
def test_the_twins_resolution_of_synthetic_summaries(kind):
    for n in (0, 1, 2, 2047, 2048, 2049, 5000):
        s = mc.synthetic(n, kind, mb.SUMMARY)
        assert np.array_equal(mb.host_debug_resolve(s), mc.resolve_summaries(s)), (kind, n)


def test_the_output_is_the_input_with_only_the_flag_bytes_changed(case):
    b = case["bam"]
    got, eof = mc.read_bgzf(case["marked"])
    stream = b"".join(got)
    assert eof and stream == mc.expected_stream(b)
    header = len(b.header())
    sizes = [len(p) for p in got]
    assert sizes[0] == header and all(s == mc.PAYLOAD for s in sizes[1:-2]) and 0 < sizes[-2] <= mc.PAYLOAD and sizes[-1] == 0 and len(sizes) > 4
    assert stream[:header] == b.header()                                               # no @PG line, SO as it was
    changed = 0
    for r, d, after in zip(b.records, case["duplicate"], _records(stream, header)):
        before = r.encode()
        assert before[:19] == after[:19] and before[20:] == after[20:]
        assert after[19] ^ before[19] in (0, 4) and bool(after[19] & 4) == (d if mc.examined(r) else bool(r.flag & 0x400))
        changed += before != after
    assert changed == sum(mc.examined(r) and bool(r.flag & 0x400) != d for r, d in zip(b.records, case["duplicate"])) > 2000
    assert not [f for f in os.listdir(str(case["tmp"])) if ".tmp." in f]


def test_remove_duplicates_writes_exactly_the_survivors(case, tmp_path):
    b = case["bam"]
    out = str(tmp_path / "removed.bam")
    r = mb.markdup_bam(case["paths"]["whole"], out, remove=True, backend="host")
    assert mc.inflated(out) == mc.expected_stream(b, remove=True)
    assert r["written"] == len(b.records) - case["counts"]["duplicates"] and {k: r[k] for k in case["counts"]} == case["counts"]
    kept = _records(mc.inflated(out), len(b.header()))
    assert len(kept) == r["written"] and not [k for k, rec in zip(kept, [x for x, d in zip(b.records, case["duplicate"]) if not d]) if k[19] & 4 and mc.examined(rec)]
    again = str(tmp_path / "again.bam")                                                # nothing is left to flag
    r2 = mb.markdup_bam(out, again, remove=True, backend="host")
    assert r2["duplicates"] == 0 and open(again, "rb").read() == open(out, "rb").read()


def test_the_tool_is_idempotent(case, tmp_path):
    again = str(tmp_path / "again.bam")
    r = mb.markdup_bam(case["marked"], again, backend="host")
    assert open(again, "rb").read() == open(case["marked"], "rb").read()
    assert {k: r[k] for k in case["counts"]} == case["counts"]


# -- invariance -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_blocks", [1, 2, 64])
@pytest.mark.parametrize("segment", [64, 4096, 8192])
def test_batches_and_segments_do_not_change_the_file(case, max_blocks, segment, tmp_path):
    out = str(tmp_path / "out.bam")
    mb.markdup_bam(case["paths"]["straddle" if max_blocks == 64 else "whole"], out, backend="host", max_blocks=max_blocks, segment_bytes=segment, threads=1 + max_blocks % 3)
    assert open(out, "rb").read() == open(case["marked"], "rb").read()


@pytest.mark.parametrize("way", list(mc.WAYS))
@pytest.mark.parametrize("remove", [False, True])
def test_the_inputs_blocks_do_not_change_the_file(case, way, remove, tmp_path):
    out, ref = str(tmp_path / "out.bam"), str(tmp_path / "ref.bam")
    mb.markdup_bam(case["paths"][way], out, remove=remove, backend="host", max_blocks=3)
    mb.markdup_bam(case["paths"]["whole"], ref, remove=remove, backend="host")
    assert open(out, "rb").read() == open(ref, "rb").read()
    assert remove or open(out, "rb").read() == open(case["marked"], "rb").read()


def test_zlib_writes_other_bytes_with_the_same_content(case, tmp_path):
    out = str(tmp_path / "zlib.bam")
    mb.markdup_bam(case["paths"]["whole"], out, backend="host", deflate="zlib")
    assert open(out, "rb").read() != open(case["marked"], "rb").read()
    assert mc.read_bgzf(out) == mc.read_bgzf(case["marked"])


# -- with sort_bam and index_bam ------------------------------------------------------------------------------------------------------------
def test_index_after_a_sort_and_the_rule_does_not_depend_on_the_order(case, tmp_path):
    sorted_fn, out = str(tmp_path / "sorted.bam"), str(tmp_path / "marked.bam")
    sort_bam.sort_bam(case["paths"]["whole"], sorted_fn, backend="host")
    r = mb.markdup_bam(sorted_fn, out, backend="host", index=True)
    index_bam.build_index(out, str(tmp_path / "separate.bai"), backend="host")
    assert open(out + ".bai", "rb").read() == open(str(tmp_path / "separate.bai"), "rb").read()
    assert {k: r[k] for k in ("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments")} == {k: case["counts"][k] for k in ("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments")}
    os.remove(out)
    with pytest.raises(BamError, match=r"marked\.bam\.bai exists: --force"):               # the index alone is in the way
        mb.markdup_bam(sorted_fn, out, backend="host", index=True)
    assert not os.path.exists(out)


def test_an_empty_file(tmp_path):
    from bam_fixture import Bam
    empty = Bam("", mc.REFS)
    empty.write(str(tmp_path / "empty.bam"), index=False)
    r = mb.markdup_bam(str(tmp_path / "empty.bam"), str(tmp_path / "out.bam"), backend="host")
    got, eof = mc.read_bgzf(str(tmp_path / "out.bam"))
    assert eof and got == [empty.header(), b""] and r["records"] == r["written"] == r["duplicates"] == 0


# -- errors -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bad_files(tmp_path_factory):
    return ic.malformed(tmp_path_factory.mktemp("markdup_bad"))


NOT_THIS_TOOLS = ("swapped_records", "swapped_contigs", "mapped_after_unplaced", "beyond_2_29")     # the order and the .bai's extent: index_bam's


@pytest.mark.parametrize("segment", [None, 64])
def test_error_verdicts(bad_files, segment, tmp_path):
    for name, (path, pattern) in bad_files.items():
        out = str(tmp_path / "out.bam")
        if name in NOT_THIS_TOOLS:
            r = mb.markdup_bam(path, out, backend="host", segment_bytes=segment, max_blocks=2)
            assert r["written"] == r["records"] > 0, name
            os.remove(out)
            continue
        with pytest.raises(BamError) as e:
            mb.markdup_bam(path, out, backend="host", segment_bytes=segment, max_blocks=2)
            pytest.fail("%s went through" % name)
        assert re.search(pattern, str(e.value)), (name, str(e.value))
        assert os.path.basename(path) in str(e.value), name
        assert not os.listdir(str(tmp_path)), name            # no partial output, no temporary file


def test_memory_below_the_summaries(case, tmp_path):
    n = len(case["bam"].records)
    out = str(tmp_path / "out.bam")
    mb.markdup_bam(case["paths"]["whole"], out, backend="host", memory=32 * n)
    assert open(out, "rb").read() == open(case["marked"], "rb").read()
    os.remove(out)
    for memory, blocks in ((32 * n - 1, 64), ("1K", 2)):
        with pytest.raises(BamError) as e:
            mb.markdup_bam(case["paths"]["whole"], out, backend="host", memory=memory, max_blocks=blocks)
        assert re.search(r"the summaries of \d+ records need \d+ bytes, more than --memory %d" % sort_bam.parse_memory(memory), str(e.value)), str(e.value)
    assert not os.listdir(str(tmp_path))


def test_existing_output_and_output_equal_to_input(case, tmp_path):
    src = str(tmp_path / "reads.bam")
    shutil.copy(case["paths"]["whole"], src)
    out = str(tmp_path / "out.bam")
    with open(out, "wb") as f:
        f.write(b"old")
    with pytest.raises(BamError, match="exists: --force"):
        mb.markdup_bam(src, out, backend="host")
    assert open(out, "rb").read() == b"old"
    mb.markdup_bam(src, out, backend="host", force=True)
    assert open(out, "rb").read() == open(case["marked"], "rb").read()
    for same in (src, str(tmp_path / "." / "reads.bam")):
        with pytest.raises(BamError, match="the output is the input"):
            mb.markdup_bam(src, same, backend="host", force=True)
    os.symlink(src, str(tmp_path / "link.bam"))
    with pytest.raises(BamError, match="the output is the input"):
        mb.markdup_bam(src, str(tmp_path / "link.bam"), backend="host", force=True)
    assert open(src, "rb").read() == open(case["paths"]["whole"], "rb").read()
    with pytest.raises(BamError, match="auto, device or host"):
        mb.markdup_bam(src, out, backend="gpu", force=True)
    with pytest.raises(BamError, match="needs --backend device"):
        mb.markdup_bam(src, out, backend="host", deflate="device", force=True)
    with pytest.raises(BamError, match="cannot open"):
        mb.markdup_bam(str(tmp_path / "nowhere.bam"), out, force=True)
    assert sorted(os.listdir(str(tmp_path))) == ["link.bam", "out.bam", "reads.bam"]


# -- the command line -----------------------------------------------------------------------------------------------------------------------------
def test_command_line_and_dispatcher(case, bad_files, tmp_path):
    n = len(case["bam"].records)
    for k, module in enumerate((["clair_amd", "markdup_bam"], ["clair_amd.markdup_bam"])):
        out = str(tmp_path / ("out%d.bam" % k))
        cmd = [sys.executable, "-m"] + module + ["--bam_fn", case["paths"]["straddle"], "--marked_fn", out, "--backend", "host", "--bam_threads", "2",
                                                "--memory", "100K", "--json_fn", str(tmp_path / "stats.json")]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
        assert done.returncode == 0 and "%d records" % n in done.stderr and "Traceback" not in done.stderr, done.stderr
        assert open(out, "rb").read() == open(case["marked"], "rb").read()
        stats = json.load(open(str(tmp_path / "stats.json")))
        assert {key: stats[key] for key in case["counts"]} == case["counts"] and stats["written"] == n and stats["backend"] == "host"
        again = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
        assert again.returncode == 1 and "exists: --force" in again.stderr and "Traceback" not in again.stderr
        removed = subprocess.run(cmd + ["--force", "--remove_duplicates"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
        assert removed.returncode == 0 and "%d written" % (n - case["counts"]["duplicates"]) in removed.stderr
        assert mc.inflated(out) == mc.expected_stream(case["bam"], remove=True)
    bad = subprocess.run([sys.executable, "-m", "clair_amd.markdup_bam", "--bam_fn", bad_files["negative_l_seq"][0], "--marked_fn", str(tmp_path / "bad.bam"),
                          "--backend", "host"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
    assert bad.returncode == 1 and "negative l_seq" in bad.stderr and "Traceback" not in bad.stderr and not os.path.exists(str(tmp_path / "bad.bam"))
    from clair_amd.__main__ import SUBMODULES
    assert SUBMODULES["markdup_bam"] == "clair_amd.markdup_bam"


def test_symbols_are_declared_and_in_the_tables():
    amd_h, host_h = open(os.path.join(ROOT, "include", "clair_amd.h")).read(), open(os.path.join(ROOT, "include", "clair_host.h")).read()
    host = _hostapi.load()
    for name in ("create", "destroy", "begin", "batch", "resolve", "mark", "emit", "stats", "backend", "debug_summary", "debug_resolve"):
        assert "clair_markdup_" + name + "(" in amd_h and "clair_markdup_" + name in _capi.SIGNATURES
        assert "clair_host_markdup_" + name + "(" in host_h and "clair_host_markdup_" + name in _hostapi.SIGNATURES and hasattr(host, "clair_host_markdup_" + name)
    assert "clair_markdup_last_error" in _capi.SIGNATURES and "clair_markdup_debug_mark" in _capi.SIGNATURES
    for name in ("clair_host_bam_job_open", "clair_host_bam_job_close", "clair_host_bam_job_header", "clair_host_markdup_run"):
        assert name + "(" in host_h and name in _hostapi.SIGNATURES and hasattr(host, name)
    assert hasattr(_capi.load(), "clair_markdup_debug_resolve")
    core = open(os.path.join(ROOT, "clair_amd", "csrc", "markdup_core.h")).read()
    assert mb.SUMMARY.itemsize == 32 and "MIN_QUALITY = %d;" % mc.MIN_QUALITY in core
    assert (mb.EXAMINED, mb.PAIRABLE, mb.READ2, mb.REVERSE) == (1, 2, 4, 8) and "S_EXAMINED = 1, S_PAIRABLE = 2, S_READ2 = 4, S_REVERSE = 8" in core


# -- the host side under the sanitizers, as a program of its own -------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17"]


def _checksum(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_host_side_under_address_and_undefined_sanitizers(case, bad_files, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([cxx] + SANITIZE + [probe, "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    program = str(tmp_path / "markdup_sanitize")
    hostsrc = os.path.join(ROOT, "clair_amd", "hostsrc")
    subprocess.check_call([cxx] + SANITIZE + ["-Wall", "-pthread", os.path.join(HERE, "markdup_sanitize.cpp"), os.path.join(hostsrc, "host_markdup.cpp"),
                                               os.path.join(hostsrc, "host_bam_job.cpp"), os.path.join(hostsrc, "host_deflate.cpp"), "-o", program, "-lz"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    b, c = case["bam"], case["counts"]
    n = len(b.records)
    head = len(sort_bam.header_blocks(b.header(), "host"))
    removed = str(tmp_path / "removed.bam")
    mb.markdup_bam(case["paths"]["whole"], removed, remove=True, backend="host")
    want = {0: "%016x" % _checksum(open(case["marked"], "rb").read()[head:]), 1: "%016x" % _checksum(open(removed, "rb").read()[head:])}      # what the driver appended
    for way, segment, max_blocks, remove in (("straddle", 0, 64, 0), ("whole", 64, 1, 1), ("whole", 4096, 2, 0), ("per_record", 0, 3, 1), ("straddle", 8192, 64, 1)):
        out = str(tmp_path / "out.part")
        done = subprocess.run([program, case["paths"][way], out, str(segment), str(max_blocks), str(1 << 20), str(remove)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              universal_newlines=True, env=env)
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        counts = [n, c["examined"], c["pairs"], c["fragments"], c["duplicate_pairs"], c["duplicate_fragments"], n - (c["duplicates"] if remove else 0)]
        assert done.stdout.split() == [str(v) for v in counts] + [want[remove]], (way, segment, remove, done.stdout)
        os.remove(out)
    bad = dict(bad_files, over_memory=(case["paths"]["whole"], r"more than --memory"))
    for name, (path, pattern) in bad.items():
        if name in NOT_THIS_TOOLS:
            continue
        for segment in (0, 64):
            done = subprocess.run([program, path, str(tmp_path / "bad.part"), str(segment), "2", str(1000 if name == "over_memory" else 1 << 20), "0"],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
            assert done.returncode == 2 and done.stderr == "" and re.search(pattern, done.stdout), (name, done.stdout, done.stderr[-2000:])
