"""The host twin of the device BGZF compressor (clair_host_deflate_bgzf; csrc/deflate_core.h): what it writes is legal, exact and deterministic
for every payload of deflate_cases.py, and on real text it is an LZ coder, not a literal coder."""
import gzip
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflate_cases import MAX_IN, PAYLOADS, REAL_TEXT, batch, vcf_text  # noqa: E402

from clair_amd import _hostapi  # noqa: E402
from clair_amd.bgzf import EOF_MARKER  # noqa: E402

BLOCKS = {}


def block_of(name):
    if name not in BLOCKS:
        BLOCKS[name] = _hostapi.deflate_bgzf(PAYLOADS[name])
    return BLOCKS[name]


@pytest.mark.parametrize("name", list(PAYLOADS))
def test_block_is_a_legal_bgzf_block_of_the_payload(name):
    payload, block = PAYLOADS[name], block_of(name)
    assert 26 <= len(block) <= 65536
    assert block[:4] == b"\x1f\x8b\x08\x04" and block[10:16] == b"\x06\x00BC\x02\x00"
    assert struct.unpack("<H", block[16:18])[0] == len(block) - 1                     # BSIZE
    d = zlib.decompressobj(-15)
    assert d.decompress(block[18:-8]) == payload
    assert d.eof and d.unused_data == b""                                             # the stream ends exactly where the footer begins
    crc, isize = struct.unpack("<II", block[-8:])
    assert crc == zlib.crc32(payload) & 0xffffffff and isize == len(payload)
    status, back = _hostapi.inflate_bgzf(block)                                       # the project's own decoder
    assert status == 0 and back == payload


@pytest.mark.parametrize("name", list(PAYLOADS))
def test_two_runs_give_the_same_bytes(name):
    assert _hostapi.deflate_bgzf(PAYLOADS[name]) == block_of(name)


def test_blocks_concatenated_are_a_gzip_file():
    names = list(PAYLOADS)
    assert gzip.decompress(b"".join(block_of(n) for n in names) + EOF_MARKER) == b"".join(PAYLOADS[n] for n in names)


def test_stored_fallback_and_window_limit():
    assert (block_of("incompressible")[18] >> 1) & 3 == 0 and len(block_of("incompressible")) == 18 + 5 + MAX_IN + 8
    assert len(block_of("window_32768")) < 40000          # the second copy is found at distance 32768 ...
    assert len(block_of("window_32769")) > 62000          # ... and not used at 32769
    assert len(block_of("run_%d" % MAX_IN)) < 400


def test_bad_arguments():
    with pytest.raises(ValueError) as ei:
        _hostapi.deflate_bgzf(b"x" * (MAX_IN + 1))
    assert "65280" in str(ei.value)


def _entropy_bytes(payload):
    counts = np.bincount(np.frombuffer(payload, dtype=np.uint8), minlength=256).astype(np.float64)
    counts = counts[counts > 0]
    return float(-(counts * np.log2(counts / len(payload))).sum() / 8)


@pytest.mark.parametrize("name", REAL_TEXT)
def test_real_text_beats_its_order_0_entropy(name):
    """No literal-only coder gets below the order-0 entropy of the bytes: the matches work."""
    assert len(block_of(name)) < _entropy_bytes(PAYLOADS[name])


# Measured (docs/merge_vcf.md): the twin's excess over zlib level 1 is negative on all three texts (vcf_text -4.1 %, tensor_text -12.9 %, the
# 16 MB VCF -4.2 %), so m, "the measured excess rounded up to the next 0.05", is 0.0 for VCF text and tensor text alike.
MARGIN = 0.0


def _zlib_bgzf_size(payload, level):
    total = 0
    for k in range(0, len(payload), MAX_IN):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(payload[k:k + MAX_IN]) + c.flush()) + 26
    return total


@pytest.mark.parametrize("name", REAL_TEXT)
def test_twin_is_within_the_margin_of_zlib_level_1(name):
    """The yardstick is zlib: a later regression to a much weaker matcher fails here."""
    assert len(block_of(name)) <= (1 + MARGIN) * _zlib_bgzf_size(PAYLOADS[name], 1)


def test_twin_is_within_the_margin_of_zlib_level_1_on_a_long_vcf():
    text = vcf_text(8 * MAX_IN, seed=9)
    mine = sum(len(_hostapi.deflate_bgzf(text[k:k + MAX_IN])) for k in range(0, len(text), MAX_IN))
    assert mine <= (1 + MARGIN) * _zlib_bgzf_size(text, 1)


def test_batch_shapes_are_what_they_claim():
    for n in (1, 2, 65):
        data, at, lens, picked = batch(n)
        assert len(at) == len(lens) == n and lens[-1] == 3
        assert all(data[a:a + m] == p for a, m, p in zip(at, lens, picked))
