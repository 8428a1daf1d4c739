"""BGZF deflate on the device (clair_deflate_*, csrc/deflate.hip) against its host twin, byte for byte, and back through the device inflate.

Every payload has passed through the same compressor on the CPU first (tests/test_deflate.py, csrc/deflate_core.h)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from deflate_cases import PAYLOADS, batch  # noqa: E402

from clair_amd import _capi, _hostapi  # noqa: E402

pytestmark = pytest.mark.gpu
TWIN = {}


def twin(payload):
    if payload not in TWIN:
        TWIN[payload] = _hostapi.deflate_bgzf(payload)
    return TWIN[payload]


@pytest.fixture(scope="module")
def deflater():
    d = _capi.Deflater(device=0, max_blocks=65)
    yield d
    d.close()


def check_against_twin(out, csize, payloads):
    assert out.shape == (len(payloads), 65536) and len(csize) == len(payloads)
    for k, payload in enumerate(payloads):
        want = twin(payload)
        assert csize[k] == len(want), (k, len(payload))
        assert out[k, :csize[k]].tobytes() == want, (k, len(payload))
        assert not out[k, csize[k]:].any()


def test_every_payload_equals_the_twin(deflater):
    names = list(PAYLOADS)
    data = b"".join(PAYLOADS[n] for n in names)
    lens = [len(PAYLOADS[n]) for n in names]
    at = np.cumsum([0] + lens[:-1])
    out, csize = deflater.blocks(data, at, lens)
    check_against_twin(out, csize, [PAYLOADS[n] for n in names])


@pytest.mark.parametrize("n", [1, 2, 65])
def test_batch_shapes_equal_the_twin_and_inflate_on_the_device(deflater, n):
    data, at, lens, picked = batch(n)
    out, csize = deflater.blocks(data, at, lens)
    check_against_twin(out, csize, picked)
    again, csize2 = deflater.blocks(data, at, lens)                          # two calls, the same bytes
    assert np.array_equal(csize, csize2) and np.array_equal(out, again)
    inf = _capi.Inflater(device=0, max_blocks=65)
    try:
        out_at = np.cumsum([0] + lens[:-1])
        back, status = inf.blocks(out.reshape(-1), np.arange(n, dtype=np.int64) * 65536, csize, out_at, lens)
    finally:
        inf.close()
    assert not status.any()
    assert back.tobytes() == b"".join(picked)


def test_bad_arguments_launch_nothing(deflater):
    ok = np.frombuffer(b"abcdefgh", dtype=np.uint8)
    for at, lens, what in (([0] * 66, [1] * 66, "max_blocks"), ([0], [65281], "65280"), ([0], [-1], "65280"), ([4], [5], "outside"), ([-1], [2], "outside")):
        with pytest.raises(_capi.EngineError) as ei:
            deflater.blocks(ok, at, lens)
        assert what in str(ei.value)
    out, csize = deflater.blocks(ok, [], [])                                 # no block: nothing to do
    assert out.shape == (0, 65536) and len(csize) == 0
    out, csize = deflater.blocks(ok, [0], [8])                               # the handle still works
    check_against_twin(out, csize, [b"abcdefgh"])
