"""sort_bam on the device (csrc/bam_sort.hip): the radix sort alone against np.argsort(kind="stable"), the gather alone against NumPy with
guard regions around its output, the files against the host twin's (hostsrc/host_bam_sort.cpp) byte for byte under batch sizes, segments,
block layouts, --memory and the three compressors, the error verdicts, and the output fed to index_bam and the native reader."""
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import index_bam_cases as ic  # noqa: E402
import sort_bam_cases as sc  # noqa: E402

from clair_amd import index_bam, sort_bam  # noqa: E402
from clair_amd._hostapi import BamError, BamReader  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sorter():
    s = sort_bam.DeviceSorter()
    yield s
    s.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sort_bam_gpu")
    b = sc.bam()
    paths = {}
    for way, kw in sc.WAYS.items():
        paths[way] = str(tmp / (way + ".bam"))
        b.write(paths[way], index=False, **kw)
    host = str(tmp / "host.bam")
    sort_bam.sort_bam(paths["straddle"], host, backend="host")
    assert sc.inflated(host) == sc.expected_stream(b)
    return dict(bam=b, paths=paths, host=open(host, "rb").read(), host_fn=host, tmp=tmp)


# -- the radix sort alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.key_sets(0)))
def test_debug_sort_is_the_stable_order(sorter, name):
    for n in sc.sizes_for(sort_bam.RADIX_TILE):
        keys = sc.key_sets(n)[name]
        got = sorter.sort(keys)
        assert got.dtype == np.uint32 and np.array_equal(got, np.argsort(keys, kind="stable")), (name, n)


def test_debug_sort_of_many_tiles(sorter):
    """more tiles than one workgroup of the scan over the digit table takes (1024 entries: four tiles), few distinct keys in each"""
    rng = np.random.default_rng(5)
    n = 37 * sort_bam.RADIX_TILE + 5
    keys = rng.integers(0, 1 << 11, n, dtype=np.uint64) | (rng.integers(0, 3, n, dtype=np.uint64) << np.uint64(40))
    assert np.array_equal(sorter.sort(keys), np.argsort(keys, kind="stable"))


# -- the gather alone ---------------------------------------------------------------------------------------------------------------------------
def test_debug_gather_writes_the_records_and_nothing_else(sorter):
    stream, starts, perm = sc.gather_case()
    lengths = [4 + struct.unpack_from("<I", stream, s)[0] for s in starts]
    assert {36, 37, 38, 39} <= set(lengths) and max(lengths) > 70000
    want = b"".join(stream[starts[p]:starts[p] + lengths[p]] for p in perm)
    assert sorter.gather(stream, starts, perm) == want                                 # (the guard regions are checked behind the kernel)
    assert sorter.gather(stream, starts, list(range(len(starts)))) == stream[3:-5]
    assert sorter.gather(stream, starts, perm) == sort_bam.host_debug_gather(stream, starts, perm)
    with pytest.raises(BamError, match="no record at"):
        sorter.gather(stream, [starts[0] + 1] + starts[1:], perm)


# -- the device against the host twin ---------------------------------------------------------------------------------------------------------
def _device(case, way="straddle", **kw):
    out = str(case["tmp"] / "device.bam")
    r = sort_bam.sort_bam(case["paths"][way], out, backend="device", force=True, **kw)
    assert r["backend"] == "device"
    return open(out, "rb").read(), r


def test_the_file_equals_the_twins(case):
    got, r = _device(case)
    assert got == case["host"]
    records = case["bam"].records
    assert (r["records"], r["unplaced"], r["groups"], r["input_reads"], r["already_sorted"]) == (len(records), sum(x.tid < 0 for x in records), 1, 1, False)
    assert r["mapped"] == sum(x.tid >= 0 and not x.flag & 4 for x in records)


@pytest.mark.parametrize("way,max_blocks,segment", [("straddle", 1, 64), ("straddle", 2, 4096), ("whole", 64, 8192), ("per_record", 3, None)])
def test_batches_segments_and_blocks_do_not_change_the_file(case, way, max_blocks, segment):
    assert _device(case, way, max_blocks=max_blocks, segment_bytes=segment)[0] == case["host"]


def test_memory_does_not_change_the_file(case):
    hist = sc.bucket_bytes(case["bam"])
    for memory in (sum(hist) - 1, max(hist) + 20000, max(hist)):
        got, r = _device(case, memory=memory, max_blocks=2)
        assert (r["groups"], r["input_reads"]) == sc.expected_groups(case["bam"], memory), memory
        assert got == case["host"], memory
    with pytest.raises(BamError) as e:
        _device(case, memory=max(hist) - 1)
    host = pytest.raises(BamError, sort_bam.sort_bam, case["paths"]["straddle"], str(case["tmp"] / "never.bam"), backend="host", memory=max(hist) - 1)
    assert str(e.value) == str(host.value) and "chr3:1048577-2097152" in str(e.value)


def test_one_group_per_bucket(tmp_path):
    b = sc.bucket_bam()
    hist = sc.bucket_bytes(b)
    b.write(str(tmp_path / "in.bam"), index=False, block=700)
    sort_bam.sort_bam(str(tmp_path / "in.bam"), str(tmp_path / "host.bam"), backend="host")
    r = sort_bam.sort_bam(str(tmp_path / "in.bam"), str(tmp_path / "device.bam"), backend="device", memory=max(hist))
    assert (r["groups"], r["input_reads"]) == (10, 11)
    assert open(str(tmp_path / "device.bam"), "rb").read() == open(str(tmp_path / "host.bam"), "rb").read()
    assert sc.inflated(str(tmp_path / "device.bam")) == sc.expected_stream(b)


def test_the_three_compressors(case):
    assert _device(case, deflate="device")[0] == case["host"]
    assert _device(case, deflate="host")[0] == case["host"]
    out = str(case["tmp"] / "device.bam")
    got = _device(case, deflate="zlib")[0]
    assert got != case["host"] and sc.read_bgzf(out)[0] == sc.read_bgzf(case["host_fn"])[0]


def test_sorted_and_empty_input(case, tmp_path):
    out = str(tmp_path / "again.bam")
    r = sort_bam.sort_bam(case["host_fn"], out, backend="device")
    assert r["already_sorted"] and open(out, "rb").read() == case["host"]
    from bam_fixture import Bam
    Bam("", sc.REFS).write(str(tmp_path / "empty.bam"), index=False)
    for backend in ("device", "host"):
        r = sort_bam.sort_bam(str(tmp_path / "empty.bam"), str(tmp_path / (backend + ".bam")), backend=backend)
        assert r["records"] == 0 and r["already_sorted"]
    assert open(str(tmp_path / "device.bam"), "rb").read() == open(str(tmp_path / "host.bam"), "rb").read()


def test_error_verdicts_are_the_twins(tmp_path):
    bad = ic.malformed(tmp_path)
    for name, (path, pattern) in bad.items():
        messages = {}
        for backend in ("device", "host"):
            out = str(tmp_path / ("%s.%s.sorted" % (name, backend)))
            try:
                sort_bam.sort_bam(path, out, backend=backend, max_blocks=2)
                messages[backend] = None
            except BamError as e:
                messages[backend] = str(e)
                assert not os.path.exists(out) and not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f], name
        assert messages["device"] == messages["host"], name
        if name in ("swapped_records", "swapped_contigs", "mapped_after_unplaced", "beyond_2_29"):
            assert messages["device"] is None, name                                    # the order and the .bai's extent do not stop a sort
            assert open(str(tmp_path / (name + ".device.sorted")), "rb").read() == open(str(tmp_path / (name + ".host.sorted")), "rb").read()
        else:
            assert messages["device"] and re.search(pattern, messages["device"]), (name, messages["device"])


# -- the output feeds the pipeline ----------------------------------------------------------------------------------------------------------------
def test_the_output_feeds_index_bam_and_the_reader(case, tmp_path):
    out = str(tmp_path / "sorted.bam")
    sort_bam.sort_bam(case["paths"]["whole"], out, backend="device", index=True)
    bai = open(out + ".bai", "rb").read()
    index_bam.build_index(out, str(tmp_path / "separate.bai"), backend="device")
    assert bai == open(str(tmp_path / "separate.bai"), "rb").read()
    expected = sc.sorted_records(case["bam"])
    seen = 0
    for ctg, beg1, end1 in [("chr1", None, None), ("chr1", 1, 1), ("chr1", 1048577, 1048600), ("chr1", 3000001, 3000080), ("chr2", 1, 300000),
                            ("chr2", 299999, 300000), ("chr3", 1200000, 1250000), ("chr3", 2097000, 2097010), ("chr3", 2400000, 2500000)]:
        tid = [n for n, _ in sc.REFS].index(ctg)
        r = BamReader(out, threads=2)
        assert r.query(ctg, beg1, end1, use_index=True)
        buf, offsets, got = np.empty(1 << 20, dtype=np.uint8), np.empty(64, dtype=np.int64), []
        while True:
            n_bytes, n_rec = r.readinto(buf, offsets)
            if n_rec == 0:
                break
            got += [bytes(buf[offsets[k]:offsets[k + 1] if k + 1 < n_rec else n_bytes]) for k in range(n_rec)]
        r.close()
        inside = lambda rec: rec.tid == tid and (beg1 is None or (rec.pos + 1 <= end1 and rec.end() >= beg1))     # noqa: E731
        want = [rec.encode() for rec in expected if inside(rec)]
        by_bytes = {rec.encode(): rec for rec in expected}
        assert [g for g in got if inside(by_bytes[g])] == want, (ctg, beg1, end1)
        seen += len(want)
    assert seen > 150
