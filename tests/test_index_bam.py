"""index_bam on the CPU (docs/index_bam.md): the host backend (hostsrc/host_bam_index.cpp over csrc/bam_index_core.h) against the independent
.bai writer of tests/bam_fixture.py, the native reader over the built index, the segmented framing rule against the sequential walk, the
error verdicts, the command line, callVarBamParallel --build_bam_index, and the host side once more as a stand-alone program under the
address and undefined-behaviour sanitizers."""
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

from clair_amd import _capi, _hostapi, index_bam  # noqa: E402
from clair_amd._hostapi import BamError, BamReader  # noqa: E402

ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


@pytest.fixture(scope="module")
def ways(tmp_path_factory):
    return ic.write_ways(tmp_path_factory.mktemp("index_bam"))


def built(bam_fn, out_fn, **kw):
    index_bam.build_index(bam_fn, out_fn, backend="host", force=True, **kw)
    return open(out_fn, "rb").read()


# -- the file ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", list(ic.WAYS))
def test_the_file_equals_the_fixtures(ways, way, tmp_path):
    want = open(ways[way] + ".bai", "rb").read()
    r = index_bam.build_index(ways[way], str(tmp_path / "out.bai"), backend="host")
    assert open(r["path"], "rb").read() == want
    assert (r["references"], r["records"], r["mapped"], r["unplaced"], r["bytes"], r["backend"]) == (3, 17, 14, 2, len(want), "host")
    assert not [f for f in os.listdir(str(tmp_path)) if f != "out.bai"]              # the temporary name is gone


@pytest.mark.parametrize("way", list(ic.WAYS))
@pytest.mark.parametrize("segment,max_blocks", [(index_bam.SEGMENT_MIN, 64), (4096, 3), (None, 2), (index_bam.SEGMENT_DEFAULT, 1)])
def test_segments_and_batch_sizes_do_not_change_the_file(ways, way, segment, max_blocks, tmp_path):
    """the segmented framing, and batches that end inside a record and inside a size word (2 blocks of 211 bytes), give the same bytes"""
    assert built(ways[way], str(tmp_path / "out.bai"), segment_bytes=segment, max_blocks=max_blocks) == open(ways[way] + ".bai", "rb").read()


def test_the_fixture_file_has_what_the_issue_lists(ways):
    """the SAM is what it is meant to be: read back from the fixture's own index"""
    data = open(ways["whole"] + ".bai", "rb").read()
    assert data[:4] == b"BAI\1" and struct.unpack_from("<i", data, 4)[0] == 3
    at, per_ref = 8, []
    for _ in range(3):
        n_bin, = struct.unpack_from("<i", data, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            bins[b] = n_chunk
            at += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", data, at)
        at += 4 + 8 * n_intv
        per_ref.append((bins, n_intv))
    assert at == len(data)                                   # no pseudo-bin's extras, no n_no_coor
    chr1, empty, chr2 = per_ref
    assert empty == ({}, 0)
    assert {0, 1, 9, 73, 585, 4681} <= set(chr1[0]) and 37450 not in chr1[0]
    assert chr1[0][4681] == 2 and chr1[0][585] == 2          # x1 | y | x2: the chunk of bin 4681 is cut in two; y and `windows` are apart
    assert chr1[1] == ((67108860 + 10 - 1) >> 14) + 1
    assert any(len(r.cigar) == 65536 for r in ic.bam().records)


# -- the reader over the built index ---------------------------------------------------------------------------------------------------------
REGIONS = [("chr1", None, None), ("chr1", 1, 10), ("chr1", 1, 1), ("chr1", 11, 99), ("chr1", 16380, 16384), ("chr1", 16385, 16390), ("chr1", 16384, 16384),
           ("chr1", 30000, 30001), ("chr1", 50000, 50010), ("chr1", 70001, 131000), ("chr1", 131100, 131102), ("chr1", 1048576, 1048577),
           ("chr1", 2000001, 2000030), ("chr1", 8388608, 8388608), ("chr1", 67108864, 67108870), ("chr1", 67108871, 69999999), ("chr1", 100, 67108864),
           ("chrEmpty", None, None), ("chrEmpty", 1, 100), ("chr2", None, None), ("chr2", 1, 20), ("chr2", 30000, 40000), ("chr2", 150051, 150051),
           ("chr2", 150052, 160000)]


def _records(path, ctg, beg1, end1, use_index):
    """the records the reader hands out that overlap the region (the brute-force filter: bam_endpos over the real CIGAR is not needed here,
    the placeholder has the right span)"""
    r = BamReader(path, threads=2)
    tid = [n for n, _ in r.references()].index(ctg)
    used = r.query(ctg, beg1, end1, use_index=use_index)
    buf, offsets, out = np.empty(1 << 20, dtype=np.uint8), np.empty(64, dtype=np.int64), []
    while True:
        n_bytes, n_rec = r.readinto(buf, offsets)
        if n_rec == 0:
            break
        for k in range(n_rec):
            rec = bytes(buf[offsets[k]:offsets[k + 1] if k + 1 < n_rec else n_bytes])
            rtid, pos, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", rec, 4)
            ops = struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name)
            span = 0 if flag & 4 else sum(c >> 4 for c in ops if c & 15 in (0, 2, 3, 7, 8))
            end = pos + max(span, 1)
            if rtid == tid and (beg1 is None or (pos + 1 <= end1 and end >= beg1)):
                out.append(rec)
    r.close()
    return used, out


@pytest.mark.parametrize("way", ["whole", "straddle"])
def test_the_reader_gives_the_same_records_over_the_built_index(ways, way, tmp_path):
    fixture_dir, built_dir = tmp_path / "fixture", tmp_path / "built"
    for d in (fixture_dir, built_dir):
        d.mkdir()
        shutil.copy(ways[way], str(d / "reads.bam"))
    shutil.copy(ways[way] + ".bai", str(fixture_dir / "reads.bam.bai"))
    assert not os.path.exists(str(built_dir / "reads.bam.bai"))                      # the fixture's index is not there
    index_bam.build_index(str(built_dir / "reads.bam"), backend="host")
    seen = 0
    for ctg, beg1, end1 in REGIONS:
        with_fixture = _records(str(fixture_dir / "reads.bam"), ctg, beg1, end1, True)
        scanned = _records(str(fixture_dir / "reads.bam"), ctg, beg1, end1, False)
        with_built = _records(str(built_dir / "reads.bam"), ctg, beg1, end1, True)
        assert with_fixture[0] and with_built[0] and not scanned[0]
        assert with_built[1] == with_fixture[1] == scanned[1], (ctg, beg1, end1)
        seen += len(scanned[1])
    assert seen > 30


# -- framing: the segmented rule against the walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segment", [index_bam.SEGMENT_MIN, 4096])
def test_segmented_framing_equals_the_walk(segment):
    n = 0
    for name, (stream, starts), entry in ic.frame_cases(segment):
        walk = index_bam.host_frame(stream, entry, 0)
        seg = index_bam.host_frame(stream, entry, segment)
        assert seg == walk, name
        assert walk[0] == starts, name                       # and both are right
        n += len(starts)
        if name == "block_size_31" or name == "huge_block_size":
            assert walk[2] and walk[1] == len(stream) - 44, name
        elif name == "one_byte_short":
            assert not walk[2] and starts[-1] < walk[1] < len(stream), name     # the tail is the record that runs one byte past the end
        elif name == "size_word_cut":
            assert not walk[2] and walk[1] == len(stream) - 3, name
        else:
            assert not walk[2] and walk[1] == len(stream), name
    assert n > 1500


def test_a_wrong_entry_is_a_verdict_not_a_fault():
    """framing from an offset that is no record start: garbage size words, bounded; both rules agree whatever comes out"""
    stream, _ = ic.record_stream(7, ic.lengths_for(64), 60)
    for entry in range(5, 400, 7):
        assert index_bam.host_frame(stream, entry, 64) == index_bam.host_frame(stream, entry, 0)
    with pytest.raises(BamError):
        index_bam.host_frame(stream, len(stream) + 1, 64)
    with pytest.raises(BamError, match="power of two"):
        index_bam.host_frame(stream, 0, 48)


# -- errors --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bad_files(tmp_path_factory):
    return ic.malformed(tmp_path_factory.mktemp("index_bam_bad"))


@pytest.mark.parametrize("segment", [None, 64])
def test_error_verdicts(bad_files, segment, tmp_path):
    for name, (path, pattern) in bad_files.items():
        with pytest.raises(BamError) as e:
            index_bam.build_index(path, str(tmp_path / "out.bai"), backend="host", segment_bytes=segment, max_blocks=2)
            pytest.fail("%s was indexed" % name)
        assert re.search(pattern, str(e.value)), (name, str(e.value))
        assert os.path.basename(path) in str(e.value), name
        assert not os.listdir(str(tmp_path)), name            # nothing is left behind


def test_an_existing_index_needs_force(ways, tmp_path):
    bam = str(tmp_path / "reads.bam")
    shutil.copy(ways["whole"], bam)
    with open(bam + ".bai", "wb") as f:
        f.write(b"old")
    with pytest.raises(BamError, match="exists: --force"):
        index_bam.build_index(bam, backend="host")
    assert open(bam + ".bai", "rb").read() == b"old"
    index_bam.build_index(bam, backend="host", force=True)
    assert open(bam + ".bai", "rb").read() == open(ways["whole"] + ".bai", "rb").read()
    with pytest.raises(BamError, match="auto, device or host"):
        index_bam.build_index(bam, backend="gpu", force=True)
    with pytest.raises(BamError, match="cannot open"):
        index_bam.build_index(str(tmp_path / "nowhere.bam"))


def test_a_csi_alone_is_still_refused_by_the_reader(ways, tmp_path):
    bam = str(tmp_path / "reads.bam")
    shutil.copy(ways["whole"], bam)
    with open(bam + ".csi", "wb") as f:
        f.write(b"CSI\1")
    r = BamReader(bam)
    with pytest.raises(BamError, match="only a .csi index"):
        r.query("chr1", 1, 100)
    r.close()
    from clair_amd import callVarBamParallel as par
    assert par.build_bam_index(bam, 2) is None and not os.path.exists(bam + ".bai")  # an index of either kind is left alone


# -- the command line -----------------------------------------------------------------------------------------------------------------------------
def test_command_line_and_dispatcher(ways, bad_files, tmp_path):
    want = open(ways["straddle"] + ".bai", "rb").read()
    for k, module in enumerate((["clair_amd", "index_bam"], ["clair_amd.index_bam"])):
        out = str(tmp_path / ("out%d.bai" % k))
        cmd = [sys.executable, "-m"] + module + ["--bam_fn", ways["straddle"], "--bai_fn", out, "--backend", "host", "--bam_threads", "2"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
        assert done.returncode == 0 and "17 records (14 mapped, 2 unplaced)" in done.stderr, done.stderr
        assert open(out, "rb").read() == want
        again = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
        assert again.returncode == 1 and "exists: --force" in again.stderr and "Traceback" not in again.stderr
        assert subprocess.run(cmd + ["--force"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, cwd=str(tmp_path)).returncode == 0
    bad = subprocess.run([sys.executable, "-m", "clair_amd.index_bam", "--bam_fn", bad_files["swapped_records"][0], "--backend", "host", "--force"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=ENV, cwd=str(tmp_path))
    assert bad.returncode == 1 and "not sorted" in bad.stderr and "Traceback" not in bad.stderr
    from clair_amd.__main__ import SUBMODULES
    assert SUBMODULES["index_bam"] == "clair_amd.index_bam"


def test_symbols_are_declared_and_in_the_tables():
    amd_h, host_h = open(os.path.join(ROOT, "include", "clair_amd.h")).read(), open(os.path.join(ROOT, "include", "clair_host.h")).read()
    host = _hostapi.load()
    for name in ("create", "destroy", "begin", "batch", "finish", "backend", "debug_frame"):
        assert "clair_bamidx_" + name + "(" in amd_h and "clair_bamidx_" + name in _capi.SIGNATURES
        assert "clair_host_bamidx_" + name + "(" in host_h and "clair_host_bamidx_" + name in _hostapi.SIGNATURES and hasattr(host, "clair_host_bamidx_" + name)
    assert "clair_bamidx_last_error" in _capi.SIGNATURES
    for name in ("build", "result_info", "result_copy", "result_free"):
        assert "clair_host_bamidx_" + name in _hostapi.SIGNATURES and hasattr(host, "clair_host_bamidx_" + name)
    assert host.clair_host_abi_version() == 6
    assert index_bam.RUN_DTYPE.itemsize == 24


# -- callVarBamParallel --build_bam_index ---------------------------------------------------------------------------------------------------------
def _parallel_args(tmp_path, bam):
    for fn, text in (("ref.fa", ">chr1\n"), ("ref.fa.fai", "chr1\t70000000\t6\t60\t61\nchr2\t200000\t9\t60\t61\n"), ("model.meta", "")):
        (tmp_path / fn).write_text(text)
    return ["--chkpnt_fn", str(tmp_path / "model"), "--ref_fn", str(tmp_path / "ref.fa"), "--bam_fn", bam, "--output_prefix", str(tmp_path / "out" / "var"),
            "--python", "PY", "--includingAllContigs", "--refChunkSize", "40000000", "--bam_reader", "native"]


def test_callVarBamParallel_builds_the_index_before_the_first_worker(ways, tmp_path, monkeypatch):
    import subprocess as sp
    from clair_amd import callVarBamParallel as par
    bam = str(tmp_path / "reads.bam")
    shutil.copy(ways["per_record"], bam)
    argv = _parallel_args(tmp_path, bam)
    seen = []

    class FakeWorker(object):                    # the runner: records what is there when a worker would start
        def __init__(self, cmd, *a, **kw):
            seen.append((list(cmd), os.path.isfile(bam + ".bai")))

        def wait(self):
            return 0
    monkeypatch.setattr(sp, "Popen", FakeWorker)
    without = par.build_parser().parse_args(argv + ["--run"])
    assert par.run(without, par.commands(without)) == 0
    assert seen and not seen[0][1] and not os.path.exists(bam + ".bai")              # without the flag nothing is built
    del seen[:]
    with_flag = par.build_parser().parse_args(argv + ["--run", "--build_bam_index"])
    assert par.run(with_flag, par.commands(with_flag)) == 0
    assert seen and all(there for _, there in seen)
    assert open(bam + ".bai", "rb").read() == open(ways["per_record"] + ".bai", "rb").read()
    # the printed commands do not know the flag: byte for byte those of a run without it
    plain = par.commands(par.build_parser().parse_args(argv))
    assert par.commands(par.build_parser().parse_args(argv + ["--build_bam_index"])) == plain
    assert len(plain) == 3 and all("build_bam_index" not in line for line in plain)
    # with the samtools reader the flag builds nothing
    os.remove(bam + ".bai")
    other = par.build_parser().parse_args([a if a != "native" else "samtools" for a in argv] + ["--run", "--build_bam_index"])
    assert par.run(other, par.commands(other)) == 0 and not os.path.exists(bam + ".bai")


# -- the host side under the sanitizers, as a program of its own -------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17"]


def _checksum(runs, linear):
    h = 0xcbf29ce484222325
    data = b"".join(struct.pack("<iIQQ", int(r["tid"]), int(r["bin"]), int(r["beg"]), int(r["end"])) for r in runs) + linear.astype("<u8").tobytes()
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_host_side_under_address_and_undefined_sanitizers(ways, bad_files, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([cxx] + SANITIZE + [probe, "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    program = str(tmp_path / "index_bam_sanitize")
    subprocess.check_call([cxx] + SANITIZE + ["-Wall", "-pthread", os.path.join(HERE, "index_bam_sanitize.cpp"),
                                               os.path.join(ROOT, "clair_amd", "hostsrc", "host_bam_index.cpp"), "-o", program, "-lz"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    for way, segment, max_blocks in (("whole", 0, 64), ("whole", 64, 64), ("straddle", 0, 2), ("straddle", 4096, 3), ("per_record", 64, 1), ("no_eof", 8192, 64)):
        counts, runs, linear, first_window = index_bam.scan(ways[way], index_bam.HostIndexer(threads=2, max_blocks=max_blocks, segment_bytes=segment))
        done = subprocess.run([program, ways[way], str(segment), str(max_blocks)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
        assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
        assert done.stdout.split() == [str(v) for v in (3, 17, 14, 2, len(runs), len(linear))] + ["%016x" % _checksum(runs, linear)], (way, segment)
    for name, (path, pattern) in bad_files.items():
        for segment in (0, 64):
            done = subprocess.run([program, path, str(segment), "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
            assert done.returncode == 2 and done.stderr == "" and re.search(pattern, done.stdout), (name, done.stdout, done.stderr[-2000:])
