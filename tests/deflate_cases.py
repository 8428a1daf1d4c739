"""Payloads for the BGZF compressor's tests (test_deflate.py: the host twin; test_deflate_gpu.py: the device), from fixed seeds: the smallest
shapes at which a deflate coder can go wrong.  PAYLOADS is built once and never changed."""
import inspect
import random
from collections import OrderedDict

import numpy as np

from clair_amd import call_var, create_tensor

MAX_IN = 65280
# call_var's own row format (clair_amd/call_var.py, the last statement of the row maker): asserted below to be what that module still uses
VCF_ROW = "%s\\t%d\\t.\\t%s\\t%s\\t%d\\t%s\\t%s\\tGT:GQ:DP:AF\\t%s:%d:%d:%.4f"
assert VCF_ROW in inspect.getsource(call_var)
VCF_ROW = VCF_ROW.replace("\\t", "\t")


def _random_bytes(seed, n, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, n).astype(np.uint8).tobytes()


def vcf_text(n_bytes, seed=5):
    """VCF rows as call_var prints them (SNPs, insertions, deletions; QUAL, depth and allele frequency vary), n_bytes of them."""
    rr = random.Random(seed)
    rows, size, pos = [], 0, 10000
    while size < n_bytes:
        pos += rr.randint(1, 3000)
        ref = rr.choice("ACGT")
        kind = rr.random()
        if kind < 0.8:
            alt = rr.choice("ACGT".replace(ref, ""))
        elif kind < 0.9:
            alt = ref + "".join(rr.choice("ACGT") for _ in range(rr.randint(1, 6)))
        else:
            ref, alt = ref + "".join(rr.choice("ACGT") for _ in range(rr.randint(1, 6))), ref
        qual, depth = rr.randint(0, 999), rr.randint(8, 90)
        row = VCF_ROW % ("chr20", pos, ref, alt, qual, ".", ".", rr.choice(["0/1", "1/1"]), qual, depth, rr.randint(1, depth) / float(depth)) + "\n"
        rows.append(row)
        size += len(row)
    return "".join(rows).encode()[:n_bytes]


def tensor_text(n_bytes, seed=6):
    """CreateTensor text rows (create_tensor.format_record): sparse small counts, as pileups are."""
    rng = np.random.RandomState(seed)
    rows, size, pos = [], 0, 500000
    while size < n_bytes:
        pos += int(rng.randint(1, 400))
        counts = (rng.randint(0, 40, (33, 8, 4)) * (rng.random_sample((33, 8, 4)) < 0.15)).astype(np.int32)
        refseq = "".join("ACGT"[b] for b in rng.randint(0, 4, 33))
        row = create_tensor.format_record("chr20", pos, refseq, counts) + "\n"
        rows.append(row)
        size += len(row)
    return "".join(rows).encode()[:n_bytes]


def _fibonacci_payload():
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = []
    for i, f in enumerate(fib):
        data += [65 + i] * f
    random.Random(3).shuffle(data)
    return bytes(data)


def _build():
    p = OrderedDict()
    for n in (0, 1, 2, 3, 4):
        p["tiny_%d" % n] = _random_bytes(10 + n, n, 65, 70)
    for n in (63, 64, 65):
        p["step_%d" % n] = _random_bytes(20 + n, n, 65, 69)
    for n in (258, 259, 260, MAX_IN):
        p["run_%d" % n] = b"a" * n
    p["two_bytes"] = _random_bytes(30, 5000, 0, 2)
    p["every_byte"] = bytes(range(256))
    p["incompressible"] = _random_bytes(31, MAX_IN)
    window = _random_bytes(32, 32768)
    p["window_32768"] = window + window[:30000]               # distance exactly 32768: legal
    p["window_32769"] = window + b"\x00" + window[:30000]     # distance 32769: must not be used
    p["fibonacci"] = _fibonacci_payload()
    assert len(p["fibonacci"]) == 46367
    p["vcf_text"] = vcf_text(MAX_IN)
    p["tensor_text"] = tensor_text(MAX_IN)
    return p


PAYLOADS = _build()
REAL_TEXT = ("vcf_text", "tensor_text")


def batch(n):
    """n payloads of unequal lengths, the last one short -> (data bytes, in_at, in_len): the ranges lie back to back with a gap of one byte."""
    names = list(PAYLOADS)
    picked = [PAYLOADS[names[(3 * k + 5) % len(names)]] for k in range(n - 1)] + [PAYLOADS["tiny_3"]]
    data, at, lens = bytearray(), [], []
    for piece in picked:
        data += b"\xff"
        at.append(len(data))
        lens.append(len(piece))
        data += piece
    return bytes(data), at, lens, picked
