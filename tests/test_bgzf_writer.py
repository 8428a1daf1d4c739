"""clair_amd.bgzf.BgzfWriter: block cuts, the EOF marker, virtual offsets, and files every BGZF reader at hand accepts."""
import gzip
import io
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflate_cases import vcf_text  # noqa: E402

from clair_amd import _hostapi  # noqa: E402
from clair_amd.bgzf import BLOCK_INPUT, EOF_MARKER, BgzfWriter  # noqa: E402

TEXT = vcf_text(3 * BLOCK_INPUT, seed=11)
SIZES = (0, 1, BLOCK_INPUT, BLOCK_INPUT + 1, 3 * BLOCK_INPUT)


def blocks_of(data):
    """[(compressed offset, block bytes)] of a BGZF file, read from the BSIZE fields."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        size = struct.unpack("<H", data[at + 16:at + 18])[0] + 1
        out.append((at, data[at:at + size]))
        at += size
    assert at == len(data)
    return out


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("size", SIZES)
def test_file_is_gzip_of_the_input_and_ends_with_the_eof_marker(tmp_path, deflate, size):
    path = str(tmp_path / "x.gz")
    w = BgzfWriter(path, deflate=deflate, threads=2, batch_blocks=2)
    for k in range(0, size, 50000):                     # pieces that do not line up with the blocks
        w.write(TEXT[k:min(size, k + 50000)])
    assert w.tell() == size
    w.close()
    data = open(path, "rb").read()
    assert len(EOF_MARKER) == 28 and data.endswith(EOF_MARKER) and w.compressed_bytes == len(data)
    assert gzip.decompress(data) == TEXT[:size]
    blocks = blocks_of(data)
    assert len(blocks) == (size + BLOCK_INPUT - 1) // BLOCK_INPUT + 1
    payload = b""
    for _, block in blocks:                             # the project's own decoder takes every block
        status, piece = _hostapi.inflate_bgzf(block)
        assert status == 0
        payload += piece
    assert payload == TEXT[:size]
    assert [struct.unpack("<I", b[-4:])[0] for _, b in blocks[:-1]] == [min(BLOCK_INPUT, size - k) for k in range(0, size, BLOCK_INPUT)]


def test_virtual_offsets():
    f = io.BytesIO()
    w = BgzfWriter(f, deflate="host", threads=1)
    w.write(TEXT[:2 * BLOCK_INPUT + 100])
    with pytest.raises(ValueError):
        w.virtual_offset(0)
    w.close()
    starts = [at for at, _ in blocks_of(f.getvalue())]
    assert len(starts) == 4 and starts[0] == 0
    assert w.virtual_offset(0) == 0
    assert w.virtual_offset(5) == 5
    assert w.virtual_offset(BLOCK_INPUT - 1) == BLOCK_INPUT - 1
    assert w.virtual_offset(BLOCK_INPUT) == starts[1] << 16                  # a block's end is the next block's start
    assert w.virtual_offset(BLOCK_INPUT + 7) == starts[1] << 16 | 7
    assert w.virtual_offset(2 * BLOCK_INPUT) == starts[2] << 16
    assert w.virtual_offset(2 * BLOCK_INPUT + 99) == starts[2] << 16 | 99
    assert w.virtual_offset(2 * BLOCK_INPUT + 100) == starts[3] << 16       # the end of the data: the EOF block
    with pytest.raises(ValueError):
        w.virtual_offset(2 * BLOCK_INPUT + 101)


def test_host_and_zlib_files_hold_the_same_text_and_host_is_deterministic():
    files = []
    for deflate, threads in (("host", 1), ("host", 4), ("zlib", 1)):
        f = io.BytesIO()
        with BgzfWriter(f, deflate=deflate, threads=threads) as w:
            w.write(TEXT)
        files.append(f.getvalue())
    assert files[0] == files[1] and files[0] != files[2]
    assert gzip.decompress(files[0]) == gzip.decompress(files[2]) == TEXT


def test_arguments():
    with pytest.raises(ValueError):
        BgzfWriter(io.BytesIO(), deflate="gzip")
    w = BgzfWriter(io.BytesIO())
    w.close()
    w.close()
    with pytest.raises(ValueError):
        w.write(b"x")
