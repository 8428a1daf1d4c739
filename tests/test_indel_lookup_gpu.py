"""The indel look-up on the MI355X: clair_frontend_indel_table (csrc/indel_lookup.hip) over BAM records decoded on the device with the
look-up option against the host twin (clair_host_indel_table) over the host packer's slab of the same BAM, byte for byte; callVarBam
--indel_lookup native against the same run with pysam stood in for by tests/fake_pysam.py."""
import logging
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import indel_lookup_cases as lc  # noqa: E402
import pileup_synth  # noqa: E402

from clair_amd import _capi, _hostapi  # noqa: E402


def device_frontend(bam_fn, ctg, ref, per_chunk, lookup=True, **kw):
    r = _hostapi.BamReader(bam_fn, threads=2)
    r.query(ctg, None, None)
    f = _capi.Frontend(0, ref, 0, -64, len(ref) + 64)
    f.bam_options(r.tid, **kw)
    if lookup:
        f.bam_lookup(True)
    buf, off = np.empty(1 << 22, np.uint8), np.empty(per_chunk, np.int64)
    while True:
        n, k = r.readinto(buf, off)
        if not k:
            break
        f.add_bam(buf, n, off, k)
    r.close()
    return f


@pytest.mark.parametrize("seed", range(4))
def test_device_tables_equal_the_host_twins_bytes(tmp_path, seed):
    sam, ctg, ref, positions = lc.random_case(seed)
    bam_fn, fa = lc.write_case(str(tmp_path), sam, ctg, ref, others=[("chrOther", "ACGT" * 500)])
    kw = dict(dcov=6, evc_min_mq=10, pile_min_mq=10)
    slabs, _ = lc.host_slabs(bam_fn, ctg, **kw)
    every = list(range(1, len(ref), 3))
    for per_chunk in ([100000, 37] if seed % 2 == 0 else [53]):                         # one slab, or several (ranks run on across slabs)
        f = device_frontend(bam_fn, ctg, ref, per_chunk, **kw)
        assert (f.stats()["slabs"] > 1) == (per_chunk < 1000)
        for pos, cap in ((positions, 32), (every, 8), (positions[:1], 1)):
            want, got = lc.table_bytes(lc.host_tables(slabs), pos, cap), lc.table_bytes(f.indel_table, pos, cap)
            assert got == want, (per_chunk, cap)
        assert sum(lc.table_bytes(f.indel_table, positions)[1]) > 40
        # the look-up leaves the stages alone: the same candidates and windows as a front end fed without the option
        g = device_frontend(bam_fn, ctg, ref, per_chunk, lookup=False, **kw)
        assert f.find_candidates(min_coverage=3, threshold=0.1) == g.find_candidates(min_coverage=3, threshold=0.1) > 0
        assert np.array_equal(f.candidates(), g.candidates())
        wf, wg = f.build_windows(min_coverage=0), g.build_windows(min_coverage=0)
        assert wf == wg > 0 and np.array_equal(f.window_counts(0, wf), g.window_counts(0, wg)) and f.stats()["anomalies"] == g.stats()["anomalies"]
        assert lc.table_bytes(f.indel_table, positions) == lc.table_bytes(lc.host_tables(slabs), positions)      # also once the candidates are fixed
        f.close()
        g.close()


def test_golden_fixture_tables_and_rows_on_the_device(tmp_path):
    from clair_amd import call_var as cvar
    sam, ctg, ref = lc.golden_sam()
    bam_fn, fa = lc.write_case(str(tmp_path), sam, ctg, ref, block=60000)
    slabs, _ = lc.host_slabs(bam_fn, ctg)
    f = device_frontend(bam_fn, ctg, ref, 1500)
    x, infos, Y, rows = lc.golden_case()
    positions = [int(i[1]) for i in infos]
    assert lc.table_bytes(f.indel_table, positions, 16) == lc.table_bytes(lc.host_tables(slabs), positions, 16)
    for mode in ("default", "pysam_all"):
        lookup = cvar.IndelTableLookup(f.indel_table, fa)
        dec = cvar.VariantDecoder(cvar.OutputConfig(False, False, False, False, False, None), lookup, always_use_bam=(mode == "pysam_all"), arith="numpy2")
        assert dec.decode_batch(x, infos, Y) == [ln for r in rows[mode] for ln in r]
        assert lookup.calls == 1
    f.close()


def test_overflows_are_reported_and_answered_by_the_twin(tmp_path):
    ref = "ACGT" * 200
    lines = ["k%d\t0\tchrL\t50\t60\t5M%dI5M\t*\t0\t0\t%s\t*" % (k, 1 + k % 7, "A" * (11 + k % 7)) for k in range(40)]
    lines += ["h%d\t%d\tchrL\t300\t60\t5M%dI5M\t*\t0\t0\t%s\t*" % (k, 16 * (k % 2), 2 + k % 3, "ACGTA" + "CG"[k % 2] * (2 + k % 3) + "ACGTA") for k in range(700)]
    bam_fn, fa = lc.write_case(str(tmp_path), "\n".join(lines) + "\n", "chrL", ref)
    slabs, _ = lc.host_slabs(bam_fn, "chrL", dcov=1000)
    f = device_frontend(bam_fn, "chrL", ref, 100000, dcov=1000)
    pos = [54, 55, 304]
    he, hn, hd, hs = _hostapi.indel_table(slabs, pos, 4)
    de, dn, dd, ds = f.indel_table(pos, 4)
    # more distinct keys than the table holds: both say so, with the same first four entries and the number there are
    assert hs.tolist() == [_hostapi.LOOKUP_ENTRIES, 0, _hostapi.LOOKUP_ENTRIES] and hn.tolist() == [7, 0, 6]
    # more than 512 hits at one position: the device hands the query to the twin and says so; the bytes are the twin's
    assert ds.tolist() == [_hostapi.LOOKUP_ENTRIES, 0, _hostapi.LOOKUP_ENTRIES | _hostapi.LOOKUP_HITS]
    assert de.tobytes() == he.tobytes() and dn.tolist() == hn.tolist() and dd.tolist() == hd.tolist() == [40, 40, 700]
    he, hn, hd, hs = _hostapi.indel_table(slabs, pos, 8)
    de, dn, dd, ds = f.indel_table(pos, 8)
    assert de.tobytes() == he.tobytes() and dn.tolist() == hn.tolist() and ds.tolist() == [0, 0, _hostapi.LOOKUP_HITS] and hs.tolist() == [0, 0, 0]
    assert sorted(int(c) for c in de[2]["count"][:6]) == sorted([117, 117, 117, 117, 116, 116])
    f.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _model(tmp):
    from clair_amd import weights
    w = weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1)
    return weights.save_weights(os.path.join(tmp, "model"), w)[:-4]


def _rows(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


@pytest.mark.parametrize("all_indels", [False, True], ids=["long_indels", "all_indels"])
def test_callVarBam_native_lookup_writes_the_fake_pysam_vcf(tmp_path, monkeypatch, caplog, all_indels):
    """on a BAM of the randomised read sets (tests/indel_lookup_cases.py), whose pysam columns the helper writes next to it"""
    from clair_amd import callVarBam
    tmp = str(tmp_path)
    sam, ctg, ref, _ = lc.random_case(3 if all_indels else 5, ref_len=3000, n_sites=60, leading=False)
    bam_fn, fa = lc.write_case(tmp, sam, ctg, ref, others=[("chrOther", "ACGT" * 30)], block=5000)
    ck = _model(tmp)
    base = ["--chkpnt_fn", ck, "--threshold", "0.15", "--minCoverage", "3", "--batch_size", "64", "--ref_fn", fa, "--ctgName", ctg, "--bam_fn", bam_fn,
            "--samtools", "/nonexistent/samtools", "--bam_reader", "native"] + (["--pysam_for_all_indel_bases"] if all_indels else [])
    plain, want, got = [os.path.join(tmp, n) for n in ("plain.vcf", "want.vcf", "got.vcf")]
    monkeypatch.setitem(sys.modules, "pysam", None)                     # no pysam: every look-up answers ""
    callVarBam.main(base + ["--call_fn", plain])
    monkeypatch.setitem(sys.modules, "pysam", lc.FakePysam)
    callVarBam.main(base + ["--call_fn", want])
    monkeypatch.setitem(sys.modules, "pysam", None)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        callVarBam.main(base + ["--call_fn", got, "--indel_lookup", "native"])
    m = re.search(r"indel look-up: (\d+) positions in (\d+) device calls", caplog.text)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0 and "lookup_over_depth 0" in caplog.text
    assert open(got).read() == open(want).read()
    assert len(_rows(got)) > 10
    if all_indels:
        assert open(plain).read() != open(want).read()                 # the look-up changes rows here: the comparison above is not vacuous


def test_callVarBam_without_the_flag_is_unchanged(tmp_path):
    """--indel_lookup absent = --indel_lookup pysam = the run before the flag existed: the slabs are fed without the option (their bytes are
    pinned in tests/test_indel_lookup.py) and the VCF equals the samtools run's, as tests/test_bam_gpu.py pins it"""
    from clair_amd import callVarBam
    tmp = str(tmp_path)
    case = pileup_synth.synth_case(seed=91, dup_burst=4)
    seq = "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:])
    bam_fn, fa = lc.write_case(tmp, case["sam"].decode() if isinstance(case["sam"], bytes) else case["sam"], case["ctg"], seq, others=[("chrOther", "ACGT" * 30)], block=5000)
    sam = os.path.join(tmp, "canon.sam")
    open(sam, "w").write(bf.Bam(case["sam"].decode() if isinstance(case["sam"], bytes) else case["sam"], [(case["ctg"], len(seq))]).canonical())
    ck = _model(tmp)
    base = ["--chkpnt_fn", ck, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--ref_fn", fa, "--ctgName", case["ctg"]]
    a, b, c = [os.path.join(tmp, n) for n in ("a.vcf", "b.vcf", "c.vcf")]
    fake = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))
    callVarBam.main(base + ["--bam_fn", sam, "--samtools", fake, "--call_fn", a])
    callVarBam.main(base + ["--bam_fn", bam_fn, "--samtools", "/nonexistent/samtools", "--bam_reader", "native", "--call_fn", b])
    callVarBam.main(base + ["--bam_fn", bam_fn, "--samtools", "/nonexistent/samtools", "--bam_reader", "native", "--indel_lookup", "pysam", "--call_fn", c])
    assert open(a).read() == open(b).read() == open(c).read() and len(_rows(a)) > 30
