"""gVCF on the MI355X (docs/gvcf.md): tallies, block records and file bytes of the device path against the host twin and the restatement of
tests/gvcf_cases.py, at the smallest shapes at which the kernels can still go wrong (T = positions per workgroup of the block scan)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gvcf_cases as gc  # noqa: E402

from clair_amd import _capi, gvcf  # noqa: E402

T = gvcf.SCAN_TILE
FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))
COSTS = (469, 10240, 3083)          # e = 0.1
HEADER = ["##fileformat=VCFv4.1\n", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"]
GUARD = 4


def _file(case, records, bounds):
    return b"".join(bytes(p) for p in gvcf.gvcf_text_parts(HEADER, [], np.zeros(0, np.int64), records, case["ctg"], case["ref"], case["ref0"], bounds))


def _compare(case, allowed, band_lists=(gc.GATK_BANDS, list(range(1, 100)))):
    """device == twin == restatement: tallies, records (with a guard tail behind them), file bytes.  -> the restated blocks of the first band list"""
    lo, n = case["lo"], case["hi"] - case["lo"]
    st = np.array([a for a, _ in allowed], dtype=np.int64)
    en = np.array([b for _, b in allowed], dtype=np.int64)
    want_t = gc.restate_tallies(case["sam"], case["ctg"], case["lo"], case["hi"])
    host_t = gc.host_tallies(case)
    f = gc.device_front_end(case)
    try:
        assert f.stats()["anomalies"] == 0
        dev_t = f.position_tallies(lo, n)
        assert dev_t.shape == (n, 7) and dev_t.tolist() == want_t and host_t.tallies.tolist() == want_t
        first = None
        for band_list in band_lists:
            bounds = gvcf.parse_bands(band_list)
            table = gvcf.band_table(bounds)
            want = gc.restate_blocks(want_t, lo, case["ref"], case["ref0"], COSTS, band_list, allowed)
            gc.check_tiling(want, allowed)
            dev = f.gvcf_blocks(COSTS, table, st, en, guard=GUARD)
            host = gvcf.host_blocks(host_t.tallies, lo, case["ref"], case["ref0"], COSTS, table, st, en, guard=GUARD)
            assert (dev[-GUARD:].view(np.uint8) == 0xA5).all() and (host[-GUARD:].view(np.uint8) == 0xA5).all()      # the bytes behind the records
            assert gc.records_as_tuples(dev[:-GUARD]) == want and gc.records_as_tuples(host[:-GUARD]) == want
            assert dev[:-GUARD].tobytes() == host[:-GUARD].tobytes()
            text = _file(case, dev[:-GUARD], bounds)
            assert text == _file(case, host[:-GUARD], bounds)
            assert text.decode().splitlines(True)[-len(want):] == [gc.restate_row(case["ctg"], case["ref"], case["ref0"], b) for b in want] or not want
            first = want if first is None else first
        return first
    finally:
        f.close()


@pytest.mark.parametrize("length", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_region_lengths(length):
    case = gc.stack_case(length, [(0, length, 3), (length // 3, 2 * length // 3 + 1, 6), (length // 2, length // 2 + 1, 30)], alt={length // 2: None})
    blocks = _compare(case, [(0, length)])
    assert blocks[0][0] == 0 and blocks[-1][1] == length and (len(blocks) >= 3 or length < 3)


def test_one_block_across_three_workgroups():
    n = 2 * T + 100
    case = gc.stack_case(n + 200, [(0, 100, 4), (n + 100, n + 200, 4)])
    blocks = _compare(case, [(0, n + 200)])
    assert (100, 100 + n, 0, 0, 0, 0, 0, 0) in blocks and len(blocks) == 3


def test_every_position_its_own_block():
    case = gc.stack_case(T + 1, [(p, p + 1, 2 if p & 1 else 6) for p in range(T + 1)])
    blocks = _compare(case, [(0, T + 1)], band_lists=(gc.GATK_BANDS,))
    assert len(blocks) == T + 1 and all(b[1] == b[0] + 1 for b in blocks)


@pytest.mark.parametrize("edge", [T - 1, T, T + 1])
def test_block_boundary_on_a_workgroup_edge(edge):
    case = gc.stack_case(T + 500, [(0, edge, 2), (edge, T + 500, 6)])
    blocks = _compare(case, [(0, T + 500)], band_lists=(gc.GATK_BANDS,))
    assert [(b[0], b[1]) for b in blocks] == [(0, edge), (edge, T + 500)]


def test_allowed_intervals_on_workgroup_edges_and_of_length_one():
    n = 2 * T + 50
    case = gc.stack_case(n, [(0, n, 5), (T - 3, T + 3, 9)])
    allowed = [(0, 1), (5, 6), (7, 8), (T - 1, T), (T, T + 1), (T + 10, 2 * T), (2 * T, 2 * T + 1), (2 * T + 3, n)]
    blocks = _compare(case, allowed)
    assert len(blocks) == len(allowed)          # adjacent intervals stay apart: an interval's first position is a block head
    blocks = _compare(case, [(0, T), (T, 2 * T), (2 * T, n)], band_lists=(gc.GATK_BANDS,))
    assert [(b[0], b[1]) for b in blocks] == [(0, T - 3), (T - 3, T), (T, T + 3), (T + 3, 2 * T), (2 * T, n)]
    assert _compare(case, [], band_lists=([],)) == []


def test_verdicts_are_the_twins_and_leave_the_handle_usable():
    case = gc.stack_case(300, [(20, 280, 5)])
    host_t = gc.host_tallies(case)
    table = gvcf.band_table(gvcf.parse_bands(None))
    f = gc.device_front_end(case)
    try:
        for st, en in (([50, 10], [60, 20]), ([10, 15], [20, 30]), ([10], [10]), ([-5], [10]), ([10], [301])):
            with pytest.raises(_capi.BadArgument) as dev:
                f.gvcf_blocks(COSTS, table, st, en)
            with pytest.raises(gvcf.GvcfArgumentError) as host:
                gvcf.host_blocks(host_t.tallies, 0, case["ref"], 0, COSTS, table, st, en)
            assert str(dev.value) == str(host.value) and "allowed interval" in str(dev.value)
        with pytest.raises(_capi.BadArgument, match="cost c_match"):
            f.gvcf_blocks((0, 10240, 3083), table, [0], [10])
        with pytest.raises(_capi.BadArgument, match="outside the tables"):
            f.position_tallies(290, 20)
        good = f.gvcf_blocks(COSTS, table, [0], [300])
        assert good.tobytes() == gvcf.host_blocks(host_t.tallies, 0, case["ref"], 0, COSTS, table, [0], [300]).tobytes() and len(good) == 3
        assert f.gvcf_device_ms() >= 0.0
    finally:
        f.close()


def test_a_handle_with_an_anomaly_bit_refuses_and_the_twin_answers():
    """Alignments whose starts decrease: CLAIR_FE_UNSORTED.  The device refuses to band tallies that may be incomplete; the Python layer
    lands on the twin, with the bytes the twin gives for the same alignments."""
    case = gc.stack_case(500, [(300, 450, 4), (10, 200, 3)])
    p = gc.packed(case)
    reads, ops, op_elem, seq = p.slab_arrays()
    order = np.argsort(-reads["pos0"], kind="stable")
    inverse = np.empty(len(order), dtype=np.int64)
    inverse[order] = np.arange(len(order))
    ops["read"] = inverse[ops["read"]]                  # an operation names its alignment by index
    table = gvcf.band_table(gvcf.parse_bands(None))
    twin = gvcf.HostTallies(0, 500)
    twin.add_arrays(reads[order], ops, op_elem, seq)
    f = _capi.Frontend(0, case["ref"], 0, 0, 500)
    try:
        f.add_arrays(reads[order], ops, op_elem, seq)
        assert f.stats()["anomalies"] & 1
        assert f.position_tallies(0, 500).tolist() == twin.tallies.tolist()       # (this handle's counts happen to be whole; the rule is the bit)
        with pytest.raises(_capi.TalliesIncomplete, match="anomaly bits 0x1"):
            f.gvcf_blocks(COSTS, table, [0], [500])
        calls = []

        def answer():
            calls.append(1)
            return gvcf.host_blocks(twin.tallies, 0, case["ref"], 0, COSTS, table, [0], [500])
        records, backend = gvcf.device_or_host_blocks(f, answer, COSTS, table, [0], [500])
        assert backend == "host" and calls == [1]
        want = gc.restate_blocks(gc.restate_tallies(case["sam"], case["ctg"], 0, 500), 0, case["ref"], 0, COSTS, gc.GATK_BANDS, [(0, 500)])
        assert gc.records_as_tuples(records) == want and len(want) == 5
    finally:
        f.close()


def test_callVarBam_gvcf_equals_both_stand_alone_backends(tmp_path):
    """callVarBam --gvcf_fn on the device front end (the live handle, no second read of the BAM), python -m clair_amd.gvcf --backend host on the
    VCF that run wrote, and --backend device: byte-identical, and the file the restatement gives."""
    import pileup_synth
    from clair_amd import weights
    from test_gvcf import _expected_file
    tmp = str(tmp_path)
    case = pileup_synth.synth_case(seed=91)
    fa, sam = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.sam")
    open(fa, "w").write(case["fasta"])
    open(fa + ".fai", "w").write("%s\t%d\t6\t60\t61\nchrOther\t120\t3100\t120\t121\n" % (case["ctg"], case["ref_len"]))
    open(sam, "w").write(case["sam"])
    ck = weights.save_weights(os.path.join(tmp, "model"), weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1))[:-4]
    common = ["--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"], "--samtools", FAKE_SAMTOOLS, "--ctgStart", "300", "--ctgEnd", "2500"]
    vcf, live = os.path.join(tmp, "calls.vcf"), os.path.join(tmp, "live.g.vcf")

    def run(argv):
        r = subprocess.run([sys.executable, "-m"] + argv, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return r
    r = run(["clair_amd.callVarBam", "--chkpnt_fn", ck, "--call_fn", vcf, "--gvcf_fn", live, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64",
             "--front_end", "device", "--overlap_filter", "host"] + common)
    assert "device front end not used" not in r.stderr and "(device backend" in r.stderr
    outs = {}
    for backend in ("host", "device"):
        outs[backend] = os.path.join(tmp, backend + ".g.vcf")
        r = run(["clair_amd.gvcf", "--vcf_fn", vcf, "--gvcf_fn", outs[backend], "--backend", backend] + common)
        assert "(%s backend" % backend in r.stderr
    text = open(live).read()
    assert open(outs["host"]).read() == text and open(outs["device"]).read() == text
    # a run on the host front end has no tallies on the GPU: the stand-alone path with the host backend reads the region once more
    vcf2, fallen = os.path.join(tmp, "calls2.vcf"), os.path.join(tmp, "host_fe.g.vcf")
    r = run(["clair_amd.callVarBam", "--chkpnt_fn", ck, "--call_fn", vcf2, "--gvcf_fn", fallen, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64",
             "--front_end", "host", "--overlap_filter", "host"] + common)
    assert "(host backend" in r.stderr and open(vcf2).read() == open(vcf).read() and open(fallen).read() == text
    lines = open(vcf).read().splitlines(True)
    header, rows = [l for l in lines if l.startswith("#")], [l for l in lines if not l.startswith("#")]
    assert len(rows) > 20
    import frontend_cases as fc
    ref, ref0 = fc.reference_of(case["fasta"], case["ctg"], 300, 2500)
    c = dict(ctg=case["ctg"], ref=ref, ref0=ref0, lo=0, hi=case["ref_len"])
    tallies = gc.restate_tallies(fc.viewed(case["sam"], case["ctg"]), case["ctg"], 0, case["ref_len"], pile_region=(300, 2500))
    want, blocks, _ = _expected_file(c, header, rows, (299, 2500), None, COSTS, gc.GATK_BANDS, tallies=tallies)
    assert text == want and len(blocks) > 100
