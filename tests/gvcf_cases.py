"""Inputs and the yardstick for the gVCF tests (test support; docs/gvcf.md).

The yardstick is a restatement of the stage that shares no code with the product: a plain Python walk over the CIGAR operations of the
alignments the candidate search is given, the rule and the segmentation in Python integers.  The filtered alignment list comes from
oracle/frontend_np.pack_sam (read-only), so that the flag filters are not restated; nothing here includes csrc/gvcf_core.h or calls
the host twin.

Two kinds of input: depth-d stacks of all-M reads over a made-up contig, which set the counts of every position exactly, and the SAM
and FASTA inside the committed tests/golden/pileup_evc_*.json.gz fixtures (plus a few tests/pileup_synth.py seeds)."""
import bisect
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from oracle import frontend_np as fe  # noqa: E402

KEYS, ACGT = "ACGTURYSWKMBDHVN", "ACGTTACCAGACAAAN"      # IUPAC_base_to_ACGT_base_dict, N stays N (shared/utils.py:19-28)
GATK_BANDS = list(range(1, 61)) + [70, 80, 90, 99]


def restate_costs(e):
    return (int(round(-10 * math.log10(1 - e) * 1024)), int(round(-10 * math.log10(e) * 1024)), int(round(-10 * math.log10(0.5) * 1024)))


def restate_tallies(sam, ctg, lo, hi, pile_region=None, dcov=250):
    """[hi - lo][7] Python ints: A C G T I D N per 0-based position, from the alignments flagged for the search."""
    s = fe.pack_sam(sam, ctg, dcov=dcov, pile_region=pile_region)
    t = [[0] * 7 for _ in range(hi - lo)]
    seq = bytes(s["seq"]).decode("latin-1")
    for r in range(len(s["pos0"])):
        if not int(s["flags"][r]) & fe.F_EVC:
            continue
        pos0, seq0 = int(s["pos0"][r]), int(s["seq0"][r])
        for j in range(int(s["op0"][r]), int(s["op0"][r]) + int(s["n_ops"][r])):
            code, n, rp, qp = int(s["op_code"][j]), int(s["op_len"][j]), pos0 + int(s["op_ref"][j]), int(s["op_q"][j])
            if code == fe.OP_M:
                for k in range(n):
                    base = seq[seq0 + qp + k].upper()
                    col = "ACGTN".index(ACGT[KEYS.index(base)])
                    if lo <= rp + k < hi:
                        t[rp + k - lo][6 if col == 4 else col] += 1
            elif lo <= rp - 1 < hi:                      # once per operation, at the base before it
                t[rp - 1 - lo][4 if code == fe.OP_I else 5] += 1
    return t


def restate_site(t, ref_base, costs):
    """one position -> (DP, GQ, PL00, PL01, PL11)"""
    c_match, c_err, c_half = costs
    dp = t[0] + t[1] + t[2] + t[3] + t[6]
    r = 0
    if ref_base is not None and ref_base.upper() in KEYS and ref_base.upper() != "N":
        r = max(0, t["ACGT".index(ACGT[KEYS.index(ref_base.upper())])] - t[4] - t[5])
    a = dp - r
    s = (r * c_match + a * c_err, dp * c_half, r * c_err + a * c_match)
    m = min(s)
    pl = [(x - m + 512) >> 10 for x in s]
    return dp, (min(99, pl[1], pl[2]) if s[0] == m else 0), pl[0], pl[1], pl[2]


def restate_allowed(span, table, bed, rows):
    """span, table: (lo, hi); bed: [(start, end), ...] or None (an empty interval counts as one position, as the candidate search reads a bed
    file); rows: [(0-based POS, len(REF)), ...] -> maximal runs [(start, end), ...]"""
    ok = set(range(max(span[0], table[0]), min(span[1], table[1])))
    if bed is not None:
        inside = set()
        for a, b in bed:
            inside.update(range(a, b if b > a else a + 1))
        ok &= inside
    for p, n in rows:
        ok.difference_update(range(p, p + n))
    runs = []
    for p in sorted(ok):
        if runs and runs[-1][1] == p:
            runs[-1][1] = p + 1
        else:
            runs.append([p, p + 1])
    return [tuple(r) for r in runs]


def restate_blocks(tallies, lo, ref, ref0, costs, bounds, allowed):
    """-> [(start, end, MIN_DP, DP, GQ, PL00, PL01, PL11), ...]; bounds: the bands' lower bounds (0 is implied)"""
    bounds = sorted(set([0] + list(bounds)))
    out = []
    for a, b in allowed:
        cur, band = None, None
        for p in range(a, b):
            i = p - ref0
            site = restate_site(tallies[p - lo], ref[i] if 0 <= i < len(ref) else None, costs)
            bd = bisect.bisect_right(bounds, site[1]) - 1
            if cur is None or bd != band:
                if cur is not None:
                    out.append(cur)
                cur = [p, p + 1, site[0], site[0], site[1], site[2], site[3], site[4]]
            else:
                cur = [cur[0], p + 1, min(cur[2], site[0]), cur[3] + site[0], min(cur[4], site[1]), min(cur[5], site[2]), min(cur[6], site[3]),
                       min(cur[7], site[4])]
            band = bd
        if cur is not None:
            out.append(cur)
    return [(c[0], c[1], c[2], c[3] // (c[1] - c[0]), c[4], c[5], c[6], c[7]) for c in out]


def records_as_tuples(rec):
    return [(int(r["start"]), int(r["end"]), int(r["min_dp"]), int(r["dp"]), int(r["gq"]), int(r["pl"][0]), int(r["pl"][1]), int(r["pl"][2])) for r in rec]


def restate_row(ctg, ref, ref0, b):
    i = b[0] - ref0
    return "%s\t%d\t.\t%s\t<NON_REF>\t.\t.\tEND=%d\tGT:GQ:DP:MIN_DP:PL\t0/0:%d:%d:%d:%d,%d,%d\n" % (
        ctg, b[0] + 1, ref[i] if 0 <= i < len(ref) else "N", b[1], b[4], b[3], b[2], b[5], b[6], b[7])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def stack_case(length, segments, seed=5, ctg="chrG", alt=None, ref_edit=None):
    """A made-up contig of `length` bases and, per (start, end, depth) of `segments`, depth all-M reads over [start, end) that repeat the
    reference -- except at the 0-based positions of `alt` ({position: base, or None for the next base in ACGT}), where every read carries
    another base.  ref_edit: {position: base} written into the reference after the reads were made (N, IUPAC codes).
    -> dict(ctg, ref, ref0, sam bytes, lo, hi)"""
    alt = alt or {}
    rng = np.random.default_rng(seed)
    ref = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
    lines, k = [], 0
    for start, end, depth in sorted(segments):
        seq = "".join((alt[p] or "ACGT"[("ACGT".index(ref[p]) + 1) % 4]) if p in alt else ref[p] for p in range(start, end))
        for _ in range(depth):
            lines.append("s%d\t%d\t%s\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\n" % (k, 16 * (k & 1), ctg, start + 1, end - start, seq, "I" * len(seq)))
            k += 1
    for p, base in (ref_edit or {}).items():
        ref = ref[:p] + base + ref[p + 1:]
    return dict(ctg=ctg, ref=ref, ref0=0, sam="".join(lines).encode(), lo=0, hi=length)


def golden_case(path):
    import frontend_cases as fc
    c = fc.evc_golden_case(path)
    return dict(ctg=c["ctg"], ref=c["ref"], ref0=c["ref0"], sam=c["sam"], lo=c["ref0"] - 64, hi=c["ref0"] + len(c["ref"]) + 64, bed=c["bed"],
                ctg_range=c["ctg_range"])


def synth_case(seed, **kw):
    import frontend_cases as fc
    c = fc.synth(seed, **kw)
    return dict(ctg=c["ctg"], ref=c["ref"], ref0=c["ref0"], sam=c["sam"], lo=c["ref0"] - 64, hi=c["ref0"] + len(c["ref"]) + 64)


def perf_case(length=4 << 20, depth=30, read_len=8192, seed=11):
    """The region the numbers in docs/gvcf.md were taken on: `length` positions at about `depth`x, as packed arrays for Frontend.add_arrays /
    HostTallies.add_arrays (no SAM text: 100 M bases of it would only be parsed away).  Reads repeat the reference but for one base in 50,
    and every 97th read carries a 2-base deletion, so that bands and blocks vary."""
    from clair_amd import _hostapi
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, length).astype(np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    n_reads = length * depth // read_len
    starts = np.sort(rng.integers(0, length - read_len, n_reads)).astype(np.int64)
    reads = np.zeros(n_reads, dtype=_hostapi.READ_DTYPE)
    with_del = (np.arange(n_reads) % 97) == 0
    n_ops = np.where(with_del, 3, 1)
    reads["pos0"], reads["seq_len"], reads["n_ops"], reads["flags"] = starts, read_len, n_ops, 2 | 4
    reads["seq0"] = np.arange(n_reads, dtype=np.int64) * read_len
    reads["op0"] = np.concatenate([[0], np.cumsum(n_ops)[:-1]])
    ops = np.zeros(int(n_ops.sum()), dtype=_hostapi.OP_DTYPE)
    half = read_len // 2
    k = 0
    for r in range(n_reads):
        if with_del[r]:      # half M, 2 D, the rest M
            ops[k] = (r, half << 2 | 0, 0, 0)
            ops[k + 1] = (r, 2 << 2 | 2, half, half)
            ops[k + 2] = (r, (read_len - half) << 2 | 0, half + 2, half)
            k += 3
        else:
            ops[k] = (r, read_len << 2 | 0, 0, 0)
            k += 1
    op_elem = np.concatenate([[0], np.cumsum(ops["code_len"] >> 2)]).astype(np.uint32)
    seq = np.empty(n_reads * read_len, dtype=np.uint8)
    for a in range(0, n_reads, 512):                 # 512 reads at a time: the index arrays stay small
        b = min(a + 512, n_reads)
        idx = starts[a:b, None] + np.arange(read_len)[None, :]
        idx[with_del[a:b], half:] += 2
        bases = ref[np.minimum(idx, length - 1)]
        flip = rng.random(bases.shape, dtype=np.float32) < 0.02
        seq[a * read_len:b * read_len] = letters[np.where(flip, (bases + 1) & 3, bases)].reshape(-1)
    return dict(ctg="chrP", ref=letters[ref].tobytes().decode(), ref0=0, lo=0, hi=length, arrays=(reads, ops, op_elem, seq))


# ---- the product's two backends over a case ------------------------------------------------------------------------------------------------
def packed(case, **kw):
    from clair_amd import _hostapi
    p = _hostapi.SamPacker(case["ctg"], **kw)
    p.feed(case["sam"], final=True)
    return p


def host_tallies(case, **kw):
    from clair_amd import gvcf
    t = gvcf.HostTallies(case["lo"], case["hi"])
    t.add_slab(packed(case, **kw))
    return t


def device_front_end(case, **kw):
    from clair_amd import _capi
    f = _capi.Frontend(0, case["ref"], case["ref0"], case["lo"], case["hi"])
    f.add_slab(packed(case, **kw))
    return f


def check_tiling(blocks, allowed):
    """every allowed position in exactly one block, no block position outside the allowed set"""
    covered = []
    for b in blocks:
        assert b[1] > b[0]
        covered.extend(range(b[0], b[1]))
    want = [p for a, b in allowed for p in range(a, b)]
    assert covered == want
