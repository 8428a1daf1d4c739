"""clair_amd.tabix: the .tbi it writes, read back by a small reader written here from the tabix specification -- header fields, bins, chunks and
the linear index -- and used to fetch regions from the BGZF file by virtual offset; what it fetches equals a brute-force filter of the text."""
import gzip
import io
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clair_amd import _hostapi, tabix  # noqa: E402
from clair_amd.bgzf import BgzfWriter  # noqa: E402


def reg2bins(beg, end):
    """The specification's reg2bins: every bin that can hold a record overlapping [beg, end)."""
    bins, end = [0], end - 1
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += list(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def parse_tbi(raw):
    data = gzip.decompress(raw)
    assert data[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack("<8i", data[4:36])
    names = data[36:36 + l_nm].split(b"\0")
    assert names.pop() == b"" and len(names) == n_ref
    at, refs = 36 + l_nm, []
    for _ in range(n_ref):
        n_bin, = struct.unpack("<i", data[at:at + 4])
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack("<Ii", data[at:at + 8])
            at += 8
            bins[b] = [struct.unpack("<QQ", data[at + 16 * k:at + 16 * k + 16]) for k in range(n_chunk)]
            at += 16 * n_chunk
        n_intv, = struct.unpack("<i", data[at:at + 4])
        at += 4
        linear = list(struct.unpack("<%dQ" % n_intv, data[at:at + 8 * n_intv]))
        at += 8 * n_intv
        refs.append((bins, linear))
    n_no_coor, = struct.unpack("<Q", data[at:at + 8])
    assert at + 8 == len(data)
    return dict(header=(fmt, col_seq, col_beg, col_end, meta, skip), names=[n.decode() for n in names], refs=refs, n_no_coor=n_no_coor)


class BgzfFile(object):
    """Seek by virtual offset, read lines: blocks inflated by the project's own decoder."""

    def __init__(self, data):
        self.data = data

    def block(self, coffset):
        size = struct.unpack("<H", self.data[coffset + 16:coffset + 18])[0] + 1
        status, payload = _hostapi.inflate_bgzf(self.data[coffset:coffset + size])
        assert status == 0
        return payload, coffset + size

    def lines_between(self, v_beg, v_end):
        """The bytes from one virtual offset to another, as lines."""
        coffset, uoffset, out = v_beg >> 16, v_beg & 0xffff, b""
        while coffset < v_end >> 16:
            payload, after = self.block(coffset)
            out += payload[uoffset:]
            coffset, uoffset = after, 0
        if v_end & 0xffff:
            payload, _ = self.block(coffset)
            out += payload[uoffset:v_end & 0xffff]
        assert out == b"" or out.endswith(b"\n")
        return out.decode().splitlines()


def fetch(index, bgzf_file, ctg, beg, end):
    """Rows overlapping the 0-based half-open [beg, end) of ctg, through bins, linear index and chunks."""
    if ctg not in index["names"]:
        return []
    bins, linear = index["refs"][index["names"].index(ctg)]
    if not linear:
        return []
    window = beg >> 14
    min_offset = linear[window] if window < len(linear) else linear[-1]
    rows = []
    chunks = sorted(c for b in reg2bins(beg, end) if b in bins for c in bins[b] if c[1] > min_offset)
    for v_beg, v_end in chunks:
        for row in bgzf_file.lines_between(v_beg, v_end):
            col = row.split("\t")
            b0 = int(col[1]) - 1
            if col[0] == ctg and b0 < end and b0 + len(col[3]) > beg:
                rows.append(row)
    return rows


def make_rows():
    rows = []
    for pos in (1, 16384, 16385, 131072, 131073):                           # linear-window and bin-level borders
        rows.append(("ctgA", pos, "A", "G"))
    rows.append(("ctgA", 32760, "A" * 20, "A"))                              # a deletion across the 16 KiB border at 32768: parent bin
    pos = 140000
    for k in range(800):                                                     # more than one BGZF block
        pos += 37 + (k * 7919) % 400
        rows.append(("ctgA", pos, "ACGT"[k % 4], "TGCA"[k % 4]))
    rows.sort(key=lambda r: r[1])
    for k in range(30):
        rows.append(("ctgC", 5 + 1000 * k, "C", "T"))
    return ["%s\t%d\t.\t%s\t%s\t%d\t.\t.\tGT:GQ:DP:AF\t0/1:%d:30:0.5000%s" % (c, p, r, a, p % 997, p % 997, "x" * 150) for c, p, r, a in rows]


@pytest.fixture(scope="module")
def indexed():
    header = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    rows = make_rows()
    names = ["ctgA", "ctgB", "ctgC"]                                         # ctgB has no records
    f = io.BytesIO()
    w = BgzfWriter(f, deflate="host", threads=2)
    w.write(header.encode())
    records, at = [], len(header)
    for row in rows:
        col = row.split("\t")
        records.append((names.index(col[0]), int(col[1]), len(col[3]), at, at + len(row) + 1))
        w.write((row + "\n").encode())
        at += len(row) + 1
    w.close()
    t = io.BytesIO()
    with BgzfWriter(t, deflate="host") as tw:
        tw.write(tabix.tbi_bytes(names, records, w.virtual_offset))
    return rows, f.getvalue(), parse_tbi(t.getvalue())


def test_header_fields_and_empty_reference(indexed):
    rows, data, index = indexed
    assert index["header"] == (2, 1, 2, 0, ord("#"), 0)
    assert index["names"] == ["ctgA", "ctgB", "ctgC"] and index["n_no_coor"] == 0
    assert index["refs"][1] == ({}, [])                                      # n_bin = 0, n_intv = 0
    assert max(c[0] >> 16 for c in sum(index["refs"][0][0].values(), [])) > 0      # chunks beyond the first BGZF block


def test_bins_and_linear_index(indexed):
    rows, data, index = indexed
    bins, linear = index["refs"][0]
    assert 4681 in bins and 4681 + 1 in bins                                 # POS 1 .. 16384 | 16385 ..: two leaf bins
    assert 585 in bins                                                       # the deletion across 32768 lies in the 128 KiB bin 585 + 0
    assert tabix.reg2bin(32759, 32779) == 585 and tabix.reg2bin(0, 1) == 4681 and tabix.reg2bin(16383, 16384) == 4681
    assert tabix.reg2bin(16384, 16385) == 4682 and tabix.reg2bin(131071, 131072) == 4681 + 7 and tabix.reg2bin(131072, 131073) == 4681 + 8
    assert all(a <= b for a, b in zip(linear, linear[1:]))
    assert linear[3] == linear[2]                                            # window 3 (49152 ..) is empty: it carries window 2's value
    for chunks in bins.values():
        assert all(beg < end for beg, end in chunks)


QUERIES = [("ctgA", 0, 1), ("ctgA", 0, 16384), ("ctgA", 16383, 16385), ("ctgA", 16384, 16385), ("ctgA", 32767, 32769), ("ctgA", 32770, 32771),
           ("ctgA", 131071, 131073), ("ctgA", 131072, 140000), ("ctgA", 150000, 200000), ("ctgA", 0, 1 << 29), ("ctgA", 250000, 250001),
           ("ctgB", 0, 100000), ("ctgC", 0, 3000), ("ctgC", 28000, 40000), ("ctgA", 400000000, 400000001)]


@pytest.mark.parametrize("ctg,beg,end", QUERIES)
def test_fetch_equals_brute_force(indexed, ctg, beg, end):
    rows, data, index = indexed
    want = [r for r in rows if r.split("\t")[0] == ctg and int(r.split("\t")[1]) - 1 < end and int(r.split("\t")[1]) - 1 + len(r.split("\t")[3]) > beg]
    assert fetch(index, BgzfFile(data), ctg, beg, end) == want


def test_position_beyond_tbi_is_an_error():
    with pytest.raises(ValueError) as ei:
        tabix.tbi_bytes(["c"], [(0, (1 << 29) + 1, 1, 0, 10)], lambda u: u)
    assert ".csi" in str(ei.value)
    tabix.tbi_bytes(["c"], [(0, 1 << 29, 1, 0, 10)], lambda u: u)            # the last position a .tbi holds
