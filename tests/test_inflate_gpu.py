"""BGZF inflate on the device (clair_inflate_*, csrc/inflate.hip) against zlib and against its host twin, the reader with
inflate="device" against inflate="host", and callVarBam --bam_inflate device end to end.

The corrupt vectors are the ones tests/test_inflate.py has put through the same decoder on the CPU (csrc/inflate_core.h): error paths that
passed there first, not attempts to fault the device."""
import logging
import os
import random
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import frontend_cases as fc  # noqa: E402
import inflate_cases as ic  # noqa: E402
import pileup_synth  # noqa: E402

from clair_amd import _capi, _hostapi  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 48


@pytest.fixture(scope="module")
def inflater():
    inf = _capi.Inflater(device=0, max_blocks=1024)
    yield inf
    inf.close()


def run_batch(inf, blocks, out_lens, order=None):
    """blocks laid out back to back (in `order`), output ranges with GUARD bytes of 0xA5 between them -> (per-block bytes, status), in the
    blocks' own order"""
    order = list(range(len(blocks))) if order is None else order
    in_at, out_at = np.zeros(len(blocks), np.int64), np.zeros(len(blocks), np.int64)
    cat, a, o = [], 0, GUARD + 1                                 # an odd start: unaligned destinations
    for k in order:
        in_at[k], out_at[k] = a, o
        cat.append(blocks[k])
        a += len(blocks[k])
        o += out_lens[k] + GUARD + (k % 3)
    cdata = np.frombuffer(b"".join(cat), dtype=np.uint8)
    out = np.full(o, 0xA5, dtype=np.uint8)
    _, status = inf.blocks(cdata, in_at, [len(b) for b in blocks], out_at, out_lens, out=out)
    covered = np.zeros(o, dtype=bool)
    got = []
    for k in range(len(blocks)):
        got.append(out[out_at[k]:out_at[k] + out_lens[k]].tobytes())
        covered[out_at[k]:out_at[k] + out_lens[k]] = True
    assert (out[~covered] == 0xA5).all(), "bytes outside the output ranges were written"
    return got, status


def test_valid_matrix_in_one_batch(inflater):
    matrix = ic.valid_matrix()
    blocks = [ic.bgzf_block(z, zlib.crc32(data), len(data)) for _, z, data in matrix]
    lens = [len(data) for _, _, data in matrix]
    assert 150 < len(blocks) <= inflater.max_blocks
    got, status = run_batch(inflater, blocks, lens)
    assert not status.any(), [matrix[k][0] for k in np.nonzero(status)[0]]
    for (name, _, data), g in zip(matrix, got):
        assert g == data, name
    order = list(range(len(blocks)))
    random.Random(5).shuffle(order)
    shuffled, status2 = run_batch(inflater, blocks, lens, order)
    again, status3 = run_batch(inflater, blocks, lens, order)
    assert shuffled == got and again == got and not status2.any() and not status3.any()


def test_mixed_batches_give_the_twins_statuses(inflater):
    valid = ic.valid_matrix()[::9]
    bad = [(name, ic.bgzf_block(z, 0x12345678, cap - 1), cap - 1) for name, z, cap in ic.corrupt_cases()] + \
          [(name, block, struct.unpack("<I", block[-4:])[0]) for name, block, _ in ic.status_cases()]
    want = [_hostapi.inflate_bgzf(block) for _, block, _ in bad]
    assert {s for s, _ in want} == {0, 1, 2, 3}
    per = 600
    n_bad = 0
    for lo in range(0, len(bad), per):
        part = bad[lo:lo + per]
        blocks = [ic.bgzf_block(z, zlib.crc32(d), len(d)) for _, z, d in valid] + [b for _, b, _ in part]
        lens = [len(d) for _, _, d in valid] + [n for _, _, n in part]
        order = list(range(len(blocks)))
        random.Random(lo).shuffle(order)
        got, status = run_batch(inflater, blocks, lens, order)
        for k, (name, _, data) in enumerate(valid):
            assert status[k] == 0 and got[k] == data, name
        for j, (name, _, n) in enumerate(part):
            st, data = want[lo + j]
            assert status[len(valid) + j] == st, name
            if st == 0:
                assert got[len(valid) + j] == data, name
            else:
                n_bad += 1
                assert got[len(valid) + j] == b"\xa5" * n, name   # a failed block's range is left alone
    assert n_bad > 3000


def test_bad_arguments_launch_nothing(inflater):
    data = b"hello, world" * 10
    block = ic.bgzf_block(ic.deflate(data), zlib.crc32(data), len(data))
    lib = inflater._lib
    cdata = np.frombuffer(block, np.uint8)
    out = np.full(4096, 0xA5, np.uint8)
    st = np.full(1, -7, np.int32)

    def call(n=1, cbytes=len(block), in_at=0, csize=len(block), out_at=0, out_len=len(data), h=inflater.handle):
        a, c, o, l = np.array([in_at] * max(n, 1), np.int64), np.array([csize] * max(n, 1), np.int32), np.array([out_at] * max(n, 1), np.int64), np.array([out_len] * max(n, 1), np.int32)
        return lib.clair_inflate_blocks(h, cdata.ctypes.data, cbytes, n, a.ctypes.data, c.ctypes.data, o.ctypes.data, l.ctypes.data, out.ctypes.data, st.ctypes.data)
    small = _capi.Inflater(device=0, max_blocks=2)
    try:
        for kw, what in ((dict(n=3, h=small.handle), b"max_blocks"), (dict(in_at=1), b"compressed bytes"), (dict(in_at=-1), b"compressed bytes"),
                         (dict(csize=25), b"csize"), (dict(cbytes=len(block) - 1), b"compressed bytes"), (dict(out_len=65537), b"out_len"),
                         (dict(out_at=-1), b"output"), (dict(out_at=2 * 65536 - 5, h=small.handle), b"output"), (dict(cbytes=3 * 65536, h=small.handle), b"compressed bytes")):
            assert call(**kw) != 0, kw
            assert what in lib.clair_inflate_last_error(kw.get("h", inflater.handle)), (kw, lib.clair_inflate_last_error(kw.get("h", inflater.handle)))
            assert st[0] == -7 and (out == 0xA5).all()
        assert call(h=small.handle) == 0 and st[0] == 0 and out[:len(data)].tobytes() == data and (out[len(data):] == 0xA5).all()
    finally:
        small.close()
    h = _capi.ctypes.c_void_p()
    assert lib.clair_inflate_create(0, 0, _capi.ctypes.byref(h)) != 0 and b"max_blocks" in lib.clair_inflate_last_error(None)


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------
def read_records(path, ctg, lo=None, hi=None, use_index=True, chunk=1 << 16, **kw):
    r = _hostapi.BamReader(path, **kw)
    r.query(ctg, lo, hi, use_index=use_index)
    buf, off, out = np.empty(chunk, np.uint8), _hostapi.bam_offsets_for(chunk), []
    while True:
        n, k = r.readinto(buf, off)
        if not k:
            break
        out.append((buf[:n].tobytes(), off[:k].tolist(), [r.voffset(j) for j in range(k)], r.render(buf, off, k)))
    info = r.info()
    r.close()
    return out, info


@pytest.mark.parametrize("layout", [dict(block=977), dict(per_record=True), dict(block=977, index=False), dict(block=65280)],
                         ids=["straddling", "record_per_block", "scan", "full_blocks"])
def test_reader_with_device_inflate_equals_host_inflate(tmp_path, layout):
    case = fc.synth(3, n_reads=600, ref_len=3000)
    bam = bf.Bam(case["sam"].decode(), [(case["ctg"], 3000)])
    path = str(tmp_path / "x.bam")
    bam.write(path, **layout)
    for region in ((None, None), (500, 1500)):
        host, info_h = read_records(path, case["ctg"], *region, threads=4, inflate="host")
        dev, info_d = read_records(path, case["ctg"], *region, threads=4, inflate="device", device=0)
        assert sum(len(c[1]) for c in host) > 50
        assert dev == host and info_d == info_h


def test_reader_reports_a_corrupt_block_alike(tmp_path):
    case = fc.synth(3, n_reads=200, ref_len=3000)
    bam = bf.Bam(case["sam"].decode(), [(case["ctg"], 3000)])
    path = str(tmp_path / "x.bam")
    bam.write(path, block=977)
    raw = open(path, "rb").read()
    at = 0
    for _ in range(4):
        at += struct.unpack("<H", raw[at + 16:at + 18])[0] + 1
    size = struct.unpack("<H", raw[at + 16:at + 18])[0] + 1
    for what, where, flip, force in (("corrupt deflate data", at + 18, 0, 0x06), ("CRC32 mismatch", at + size - 8, 0x01, 0), ("", at + 18 + (size - 26) // 2, 0x55, 0)):
        bad = bytearray(raw)
        bad[where] = (bad[where] ^ flip) | force                 # block type 3; a CRC32 bit; a byte in the middle of the stream
        p = str(tmp_path / "bad.bam")
        open(p, "wb").write(bytes(bad))
        with pytest.raises(_hostapi.BamError) as by_host:
            read_records(p, case["ctg"], use_index=False, inflate="host")
        with pytest.raises(_hostapi.BamError) as by_device:
            read_records(p, case["ctg"], use_index=False, inflate="device")
        assert str(by_device.value) == str(by_host.value) and "offset %d: %s" % (at, what) in str(by_host.value)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_callVarBam_device_inflate_writes_the_host_inflate_vcf(tmp_path, caplog):
    from clair_amd import callVarBam, weights
    tmp = str(tmp_path)
    case = pileup_synth.synth_case(seed=91, dup_burst=4)
    fa = os.path.join(tmp, "ref.fa")
    text, fai = bf.fasta_of({case["ctg"]: "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:]), "chrOther": "ACGT" * 30})
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    bam_fn = os.path.join(tmp, "reads.bam")
    bf.Bam(case["sam"], [(case["ctg"], case["ref_len"]), ("chrOther", 120)]).write(bam_fn, block=5000)
    w = weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1)
    ck = weights.save_weights(os.path.join(tmp, "model"), w)[:-4]
    base = ["--chkpnt_fn", ck, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--ref_fn", fa, "--ctgName", case["ctg"], "--bam_fn", bam_fn,
            "--samtools", "/nonexistent/samtools", "--bam_reader", "native"]
    rows = 0
    for region in ([], ["--ctgStart", "300", "--ctgEnd", "2500"]):
        for fe in ("device", "host"):
            want, got = os.path.join(tmp, "want.vcf"), os.path.join(tmp, "got.vcf")
            callVarBam.main(base + region + ["--call_fn", want, "--front_end", fe, "--bam_inflate", "host"])
            with caplog.at_level(logging.INFO):
                callVarBam.main(base + region + ["--call_fn", got, "--front_end", fe, "--bam_inflate", "device", "--bam_threads", "1"])
            assert open(got).read() == open(want).read(), (region, fe)
            rows += len([l for l in open(want).read().splitlines() if not l.startswith("#")])
    assert rows > 60
