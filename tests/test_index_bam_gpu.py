"""index_bam on the device (csrc/bam_index.hip) against its host twin (hostsrc/host_bam_index.cpp), bit for bit: the files, the framing alone
on generated streams, batches that end inside a record and inside a size word, a 4 MB synthetic BAM, and the error verdicts."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import index_bam_cases as ic  # noqa: E402

from clair_amd import index_bam  # noqa: E402
from clair_amd._hostapi import BamError  # noqa: E402

pytestmark = pytest.mark.gpu
SCAN_ITEMS = 256 * 4                             # segments per workgroup of the scan over the segments' record counts (clair_bix::ITEMS)


@pytest.fixture(scope="module")
def ways(tmp_path_factory):
    return ic.write_ways(tmp_path_factory.mktemp("index_bam_gpu"))


def both(bam_fn, tmp_path, **kw):
    out = {}
    for backend in ("device", "host"):
        r = index_bam.build_index(bam_fn, str(tmp_path / (backend + ".bai")), backend=backend, force=True, **kw)
        assert r["backend"] == backend
        out[backend] = (open(r["path"], "rb").read(), dict(r, path=None, backend=None))
    return out


@pytest.mark.parametrize("way", list(ic.WAYS))
def test_the_file_equals_the_twins_and_the_fixtures(ways, way, tmp_path):
    got = both(ways[way], tmp_path)
    assert got["device"] == got["host"]
    assert got["device"][0] == open(ways[way] + ".bai", "rb").read()


@pytest.mark.parametrize("segment,max_blocks", [(index_bam.SEGMENT_MIN, 64), (4096, 3), (None, 2)])
def test_batches_that_end_inside_a_record_and_inside_a_size_word(ways, segment, max_blocks, tmp_path):
    """blocks of 211 bytes, two to a batch: the 262 KB record is carried over more than a thousand batches, size words are cut"""
    got = both(ways["straddle"], tmp_path, segment_bytes=segment, max_blocks=max_blocks)
    assert got["device"] == got["host"] and got["device"][0] == open(ways["straddle"] + ".bai", "rb").read()


def _framing_streams(segment):
    for case in ic.frame_cases(segment):
        yield case
    short = [36, 37, 40, 63]
    for n in (64, 65):                           # 64 and 65 records in one segment (when it has room for them)
        yield "%d_in_a_segment" % n, ic.record_stream(20 + n, short, n, tail=bytes(3)), 0
    yield "skips_segments", ic.record_stream(30, [36, 3 * segment + 40, 7 * segment + 1, 64], 12, entry=segment - 2), segment - 2
    if segment == index_bam.SEGMENT_MIN:         # a segment count just below, at and above what one workgroup of the scan takes
        for n_seg in (SCAN_ITEMS - 1, SCAN_ITEMS, SCAN_ITEMS + 1, 2 * SCAN_ITEMS + 3):
            yield "%d_segments" % n_seg, ic.record_stream(40, [64], n_seg), 0
            yield "%d_segments_mixed" % n_seg, ic.record_stream(41, ic.lengths_for(segment)[:7], n_seg * 64 // 60), 0


@pytest.mark.parametrize("segment", [index_bam.SEGMENT_MIN, 4096, index_bam.SEGMENT_DEFAULT])
def test_framing_alone_equals_the_walk(segment):
    dev = index_bam.DeviceIndexer(segment_bytes=segment)
    try:
        for name, (stream, starts), entry in _framing_streams(segment):
            got = dev.frame(stream, entry)
            assert got[3], "%s: the bytes behind the stream or behind the offsets were written" % name
            assert got[:3] == index_bam.host_frame(stream, entry, 0), name
            assert got[0] == starts, name
        stream, _ = ic.record_stream(7, ic.lengths_for(64), 60)
        for entry in range(5, 400, 37):          # from offsets that are no record starts: a verdict, the same one, and no fault
            got = dev.frame(stream, entry)
            assert got[3] and got[:3] == index_bam.host_frame(stream, entry, segment), entry
    finally:
        dev.close()


def test_a_4_mb_synthetic_bam(tmp_path):
    path, n_reads = ic.synthetic_bam(str(tmp_path / "synthetic.bam"))
    assert os.path.getsize(path) > 2 << 20
    got = both(path, tmp_path)                   # the default segment, 64 blocks to a batch
    assert got["device"] == got["host"]
    assert got["device"][1]["records"] == n_reads and got["device"][1]["unplaced"] == 40 and got["device"][1]["chunks"] > 100


def test_error_verdicts_equal_the_twins_and_the_handle_goes_on(ways, tmp_path):
    bad = ic.malformed(tmp_path)
    dev, host = index_bam.DeviceIndexer(max_blocks=2), index_bam.HostIndexer(max_blocks=2)
    try:
        for name, (path, _) in bad.items():
            said = {}
            for backend, indexer in (("device", dev), ("host", host)):
                with pytest.raises(BamError) as e:
                    index_bam.scan(path, indexer)
                said[backend] = str(e.value)
            assert said["device"] == said["host"], name
            counts, runs, linear, first_window = index_bam.scan(ways["whole"], dev)          # the same handle, a good file
            assert index_bam.bai_bytes(3, runs, linear, first_window) == open(ways["whole"] + ".bai", "rb").read(), name
    finally:
        dev.close()
        host.close()
