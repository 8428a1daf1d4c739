"""The device inflate's host twin (clair_host_inflate_block / _bgzf: csrc/inflate_core.h compiled for the host) against zlib, the reader's
inflater hook, and the --bam_inflate flag.  No GPU."""
import ctypes
import os
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

from clair_amd import _hostapi  # noqa: E402

GUARD = 64


def twin(stream, cap):
    """the twin on a buffer with guard bytes on both sides -> (status, bytes, crc32)"""
    lib = _hostapi.load()
    src = np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8)
    buf = np.full(GUARD + cap + GUARD, 0xA5, dtype=np.uint8)
    n, crc, status = ctypes.c_int64(-1), ctypes.c_uint32(0), ctypes.c_int(-1)
    assert lib.clair_host_inflate_block(src.ctypes.data, len(stream), buf.ctypes.data + GUARD, cap, ctypes.byref(n), ctypes.byref(crc), ctypes.byref(status)) == 0
    assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + cap:] == 0xA5).all(), "guard bytes overwritten"
    return status.value, buf[GUARD:GUARD + n.value].tobytes(), crc.value


def test_valid_matrix_equals_zlib():
    matrix = ic.valid_matrix()
    assert len(matrix) > 150
    seen = set()
    for name, stream, data in matrix:
        assert ic.zlib_inflate(stream, len(data) + 1) == data, name
        status, out, crc = twin(stream, len(data) + 1)
        assert status == 0 and out == data and crc == (zlib.crc32(data) & 0xffffffff), name
        status, out, _ = twin(stream, len(data))                # room for exactly the bytes is enough
        assert status == 0 and out == data, name
        if data:
            assert twin(stream, len(data) - 1)[0] == 1, name    # one byte short is not
        seen.add(stream[0] >> 1 & 3)
    assert seen == {0, 1, 2}                                    # stored, fixed and dynamic first blocks all occur


def test_corruption_fuzz_gives_zlibs_verdict():
    cases = ic.corrupt_cases()
    assert len(cases) > 5000
    ok = bad = 0
    for name, stream, cap in cases:
        want = ic.zlib_inflate(stream, cap)
        assert ic.zlib_inflate(stream, cap) == want, name       # zlib itself is deterministic on the vector
        status, out, crc = twin(stream, cap)
        if want is None:
            assert status == 1, name
            bad += 1
        else:
            assert status == 0 and out == want and crc == (zlib.crc32(want) & 0xffffffff), name
            ok += 1
    assert ok > 300 and bad > 3000                              # both verdicts are well covered; none is excluded


def test_status_mapping():
    for name, block, want in ic.status_cases():
        status, out = _hostapi.inflate_bgzf(block)
        assert status == want, name
        # what the reader's zlib path says about the same block
        isize = struct.unpack("<I", block[-4:])[0]
        ref = ic.zlib_inflate(block[18:-8], isize + 1)
        zstatus = 1 if ref is None else 2 if len(ref) != isize else 0 if zlib.crc32(ref) == struct.unpack("<I", block[-8:-4])[0] else 3
        assert zstatus == want, name
    lib = _hostapi.load()
    n, st = ctypes.c_int64(0), ctypes.c_int(0)
    out = np.zeros(65537, np.uint8)
    short = np.zeros(25, np.uint8)
    assert lib.clair_host_inflate_bgzf(short.ctypes.data, 25, out.ctypes.data, ctypes.byref(n), ctypes.byref(st)) != 0


def test_host_symbols_are_exported_and_listed():
    lib = _hostapi.load()
    header = open(os.path.join(os.path.dirname(HERE), "include", "clair_host.h")).read()
    for name in ("clair_host_bam_set_inflater", "clair_host_inflate_block", "clair_host_inflate_bgzf"):
        assert name in _hostapi.SYMBOLS and hasattr(lib, name) and name + "(" in header
    from clair_amd import _capi
    amd = open(os.path.join(os.path.dirname(HERE), "include", "clair_amd.h")).read()
    for name in ("clair_inflate_create", "clair_inflate_destroy", "clair_inflate_last_error", "clair_inflate_blocks", "clair_inflate_blocks_cb"):
        assert name in _capi.SYMBOLS and name + "(" in amd
    assert _capi.load().clair_abi_version() == 6


# ---- the reader and its hook --------------------------------------------------------------------------------------------------------------
def read_records(path, ctg, lo=None, hi=None, use_index=True, chunk=1 << 16, **kw):
    hook = kw.pop("hook", None)
    r = _hostapi.BamReader(path, **kw)
    if hook is not None:
        r.set_inflater(hook, None, 3)
    r.query(ctg, lo, hi, use_index=use_index)
    buf, off, out = np.empty(chunk, np.uint8), _hostapi.bam_offsets_for(chunk), []
    while True:
        n, k = r.readinto(buf, off)
        if not k:
            break
        out.append((buf[:n].tobytes(), off[:k].tolist(), [r.voffset(j) for j in range(k)]))
    info = r.info()
    r.close()
    return out, info


def zlib_hook(force=None, calls=None):
    """an inflater in Python: zlib on every block; force = (compressed size of the block to fail, status)"""
    def fn(ctx, cdata, cbytes, n, in_at, csize, out_at, out_len, out, status):
        in_at, out_at = np.ctypeslib.as_array(ctypes.cast(in_at, ctypes.POINTER(ctypes.c_int64)), (n,)), np.ctypeslib.as_array(ctypes.cast(out_at, ctypes.POINTER(ctypes.c_int64)), (n,))
        csize, out_len = np.ctypeslib.as_array(ctypes.cast(csize, ctypes.POINTER(ctypes.c_int32)), (n,)), np.ctypeslib.as_array(ctypes.cast(out_len, ctypes.POINTER(ctypes.c_int32)), (n,))
        st = np.ctypeslib.as_array(ctypes.cast(status, ctypes.POINTER(ctypes.c_int32)), (n,))
        data = ctypes.string_at(cdata, cbytes)
        if calls is not None:
            calls.append(n)
        for i in range(n):
            block = data[in_at[i]:in_at[i] + csize[i]]
            got = ic.zlib_inflate(block[18:-8], int(out_len[i]) + 1) or b""
            got = got[:out_len[i]]
            ctypes.memmove(out + int(out_at[i]), got, len(got))
            st[i] = 0
            if force is not None and block == force[0]:
                st[i] = force[1]
        return 0
    return _hostapi.INFLATE_FN(fn)


def _bam(tmp_path, **write):
    case = fc.synth(3, n_reads=200, ref_len=3000)
    bam = bf.Bam(case["sam"].decode(), [(case["ctg"], 3000)])
    path = str(tmp_path / "x.bam")
    bam.write(path, **write)
    return path, case


@pytest.mark.parametrize("layout", [dict(block=977), dict(per_record=True), dict(block=977, index=False)], ids=["straddling", "record_per_block", "scan"])
def test_host_inflate_and_the_hook_equal_the_plain_reader(tmp_path, layout):
    path, case = _bam(tmp_path, **layout)
    for region in ((None, None), (500, 1500)):
        plain, info = read_records(path, case["ctg"], *region, threads=3)
        assert sum(len(c[1]) for c in plain) > 20
        named, info_named = read_records(path, case["ctg"], *region, threads=3, inflate="host")
        assert named == plain and info_named == info
        calls = []
        hooked, info_hooked = read_records(path, case["ctg"], *region, threads=3, hook=zlib_hook(calls=calls))
        assert hooked == plain and info_hooked == info and calls and max(calls) <= 3
    with pytest.raises(_hostapi.BamError, match="bam_inflate"):
        _hostapi.BamReader(path, inflate="gpu")


@pytest.mark.parametrize("status", [1, 2, 3])
def test_a_forced_status_gives_the_zlib_paths_message(tmp_path, status):
    path, case = _bam(tmp_path, block=977)
    raw = bytearray(open(path, "rb").read())
    at = 0
    for _ in range(4):                                          # the fifth block: records, not the header
        at += struct.unpack("<H", raw[at + 16:at + 18])[0] + 1
    size = struct.unpack("<H", raw[at + 16:at + 18])[0] + 1
    good = bytes(raw[at:at + size])
    if status == 1:
        raw[at + 18] |= 0x06                                    # block type 3
    elif status == 2:
        raw[at + size - 4:at + size] = struct.pack("<I", struct.unpack("<I", raw[at + size - 4:at + size])[0] - 1)
    else:
        raw[at + size - 8] ^= 1
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(_hostapi.BamError) as by_zlib:
        read_records(bad, case["ctg"], use_index=False, threads=2)
    assert "offset %d: %s" % (at, _hostapi.INFLATE_STATUS[status]) in str(by_zlib.value)
    with pytest.raises(_hostapi.BamError) as by_hook:            # the intact file, the hook reporting that status for that block
        read_records(path, case["ctg"], use_index=False, threads=2, hook=zlib_hook(force=(good, status)))
    assert str(by_hook.value).replace(path, "F") == str(by_zlib.value).replace(bad, "F")


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_bam_inflate_device_needs_the_native_reader(tmp_path):
    from clair_amd import callVarBam
    for fn in ("a.bam", "ref.fa"):
        open(str(tmp_path / fn), "w").write("")
    base = ["--chkpnt_fn", "x", "--bam_fn", str(tmp_path / "a.bam"), "--ref_fn", str(tmp_path / "ref.fa"), "--ctgName", "c", "--call_fn", str(tmp_path / "o.vcf")]
    with pytest.raises(SystemExit, match=r"^\[ERROR\] --bam_inflate device .*--bam_reader native$"):
        callVarBam.main(base + ["--bam_inflate", "device"])
    args = callVarBam.build_parser().parse_args(base)
    assert args.bam_inflate == "host"
    args = callVarBam.normalise(callVarBam.build_parser().parse_args(base + ["--bam_reader", "native", "--bam_inflate", "device", "--bam_threads", "2"]))
    assert args.bam_inflate == "device" and args.bam_threads == 2


def test_parallel_commands_pass_bam_inflate_on_only_when_given(tmp_path):
    import shlex
    from clair_amd import callVarBam, callVarBamParallel as par
    for fn, text in (("ref.fa", ">x\n"), ("ref.fa.fai", "chr1\t25000000\t6\t60\t61\n"), ("a.bam", ""), ("model.meta", "")):
        open(str(tmp_path / fn), "w").write(text)
    argv = ["--chkpnt_fn", str(tmp_path / "model"), "--ref_fn", str(tmp_path / "ref.fa"), "--bam_fn", str(tmp_path / "a.bam"),
            "--output_prefix", str(tmp_path / "var"), "--python", "PY"]
    plain = par.commands(par.build_parser().parse_args(argv + ["--bam_reader", "native"]))
    given = par.commands(par.build_parser().parse_args(argv + ["--bam_reader", "native", "--bam_inflate", "device"]))
    assert len(plain) == len(given) == 3 and all("--bam_inflate" not in l for l in plain)
    assert all(l.endswith(' --bam_reader "native" --bam_inflate "device"') or ' --bam_reader "native" --bam_inflate "device" ' in l for l in given)
    words = shlex.split(given[0])
    args = callVarBam.build_parser().parse_args(words[words.index("clair_amd.callVarBam") + 1:])
    assert args.bam_inflate == "device" and args.bam_reader == "native"
