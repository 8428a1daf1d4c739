"""--bam_reader native on the MI355X: BAM records decoded on the device (clair_frontend_bam_options / _add_bam, fe_bam_* in
csrc/frontend.hip) against the text path (clair_frontend_add_text) on the canonical text `samtools view` prints for the same BAM, and
callVarBam / callVarBamParallel on the BAM against the same runs with samtools on that text."""
import logging
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import frontend_cases as fc  # noqa: E402
import pileup_synth  # noqa: E402

from clair_amd import _capi, _hostapi  # noqa: E402

FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))


def with_filtered_records(sam, ctg):
    """the case's lines plus records `samtools view -F 2316 <bam> ctg` drops: secondary / supplementary / unmapped copies, another contig"""
    out = []
    for k, line in enumerate(sam.decode().splitlines()):
        out.append(line)
        col = line.split("\t")
        if k % 7 == 3:
            out.append("\t".join(col[:1] + [str(int(col[1]) | (256, 2048, 4, 8)[k % 4])] + col[2:]))
        if k % 11 == 5:
            out.append("\t".join(col[:2] + ["chrOther"] + col[3:]))
    return "\n".join(out) + "\n"


def bam_of(tmp, case, sort=True, extra_filtered=True):
    sam = with_filtered_records(case["sam"], case["ctg"]) if extra_filtered else case["sam"].decode()
    bam = bf.Bam(sam, [(case["ctg"], case["ref0"] + len(case["ref"]) + 100000), ("chrOther", 1 << 20)], sort=sort)
    path = os.path.join(tmp, "c.bam")
    bam.write(path, block=3001)
    canon = "".join(l + "\n" for l in bam.canonical().splitlines() if not int(l.split("\t")[1]) & 2316 and l.split("\t")[2] == case["ctg"])
    return path, canon.encode()


def frontend_of(case, margin=64):
    return _capi.Frontend(0, case["ref"], case["ref0"], case["ref0"] - margin, case["ref0"] + len(case["ref"]) + margin)


def feed_bam(path, case, records_per_chunk, region=None, **kw):
    r = _hostapi.BamReader(path, threads=2)
    r.query(case["ctg"], *(region or (None, None)))
    f = frontend_of(case)
    f.bam_options(r.tid, region=region, **kw)
    buf = np.empty(1 << 22, np.uint8)
    off = np.empty(records_per_chunk, np.int64)
    while True:
        n, k = r.readinto(buf, off)
        if not k:
            break
        f.add_bam(buf, n, off, k)
    r.close()
    return f


def feed_text(case, text, **kw):
    f = frontend_of(case)
    f.text_options(case["ctg"], **kw)
    if text:
        f.add_text(text)
    return f


def same_results(f, g, evc=None, min_coverage=0):
    a, b = [np.concatenate(x.slab_reads) if x.slab_reads else np.zeros(0, _hostapi.READ_DTYPE) for x in (f, g)]
    assert f.text_stats() == g.text_stats()
    for name in ("pos0", "seq_len", "n_ops", "flags"):
        assert np.array_equal(a[name], b[name]), name
    evc = evc or dict(min_coverage=3, threshold=0.1)
    nf, ng = f.find_candidates(**evc), g.find_candidates(**evc)
    assert nf == ng and np.array_equal(f.candidates(), g.candidates())
    wf = f.build_windows(min_coverage=min_coverage, drop_non_iupac_centre=False)
    wg = g.build_windows(min_coverage=min_coverage, drop_non_iupac_centre=False)
    assert wf == wg
    if wf:
        for x, y in zip(f.window_info(0, wf), g.window_info(0, wg)):
            assert np.array_equal(x, y)
        assert np.array_equal(f.window_counts(0, wf), g.window_counts(0, wg))
    assert f.stats()["anomalies"] == g.stats()["anomalies"]
    return len(a), wf


@pytest.mark.parametrize("per_chunk", [1, 37, 100000])
@pytest.mark.parametrize("path", fc.CT_GOLDEN + fc.EVC_GOLDEN, ids=lambda p: os.path.basename(p).split(".")[0])
def test_records_on_the_device_equal_the_text_on_the_device(tmp_path, path, per_chunk):
    case = fc.ct_golden_case(path) if "pileup_ct_" in path else fc.evc_golden_case(path)
    bam_fn, canon = bam_of(str(tmp_path), case)
    kw = dict(pile_region=case.get("pile_region"), dcov=case.get("dcov", 250))
    f = feed_bam(bam_fn, case, per_chunk, **kw)
    g = feed_text(case, canon, **kw)
    n, _ = same_results(f, g)
    assert n > 0 and f.text_stats()["lines"] == len(canon.splitlines())


@pytest.mark.parametrize("block", range(2))
def test_differential_fuzz_records_against_text(tmp_path, block):
    done = 0
    for seed in range(100 + block * 10, 110 + block * 10):
        case, pile_kw, evc_kw, region = fc.fuzz_case(seed)
        bam_fn, canon = bam_of(str(tmp_path), case)
        kw = dict(dcov=pile_kw["dcov"], pile_min_mq=pile_kw["min_mq"], evc_min_mq=evc_kw["min_mq"], pile_region=region)
        f = feed_bam(bam_fn, case, [1, 5, 64, 100000][seed % 4], **kw)
        g = feed_text(case, canon, **kw)
        rng = dict(ctg_start=region[0], ctg_end=region[1]) if region else {}
        n, w = same_results(f, g, evc=dict(min_coverage=evc_kw["min_coverage"], threshold=evc_kw["threshold"], bed=evc_kw["bed"], **rng),
                            min_coverage=pile_kw["min_coverage"])
        done += w
        f.close()
        g.close()
    assert done > 200


@pytest.mark.parametrize("region", [(1, 1), (300, 900), (1500, 5000)])
def test_the_view_region_is_applied_on_the_device(tmp_path, region):
    case = fc.synth(61, n_reads=300, ref_len=3000)
    bam_fn, canon = bam_of(str(tmp_path), case)
    sam = str(tmp_path / "canon.sam")
    open(sam, "wb").write(canon)
    text = subprocess.run([sys.executable, os.path.join(HERE, "fake_samtools.py"), "view", "-F", "2316", sam, "%s:%d-%d" % ((case["ctg"],) + region)],
                          capture_output=True).stdout
    f = feed_bam(bam_fn, case, 50, region=region)
    g = feed_text(case, text)
    same_results(f, g)


def test_anomalies_raise_the_same_bits(tmp_path):
    ok = "r%d\t0\tchrS\t%d\t60\t5M\t*\t0\t0\tACGTA\tIIIII"
    cases = {"unsorted": [ok % (1, 50), ok % (2, 40), ok % (3, 60)],
             "zero_indel": [ok % (1, 10), "z\t0\tchrS\t12\t60\t3M0I2M\t*\t0\t0\tACGTA\tIIIII"],
             "bad_base": [ok % (1, 10), "b\t0\tchrS\t12\t60\t5M\t*\t0\t0\tAC=TA\tIIIII"],
             "long_span": [ok % (1, 10), "l\t0\tchrS\t20\t60\t2M300000D3M\t*\t0\t0\tACGTA\tIIIII"],
             "star_seq": [ok % (1, 10), "s\t0\tchrS\t12\t60\t5M\t*\t0\t0\t*\t*", "t\t0\tchrS\t14\t60\t*\t*\t0\t0\tACG\tIII"],
             "lead_indel": [ok % (1, 10), "d\t0\tchrS\t10\t60\t2D5M\t*\t0\t0\tACGTA\tIIIII"]}
    ref = "".join("ACGT"[(i * 7) % 4] for i in range(400000))
    case = dict(ctg="chrS", ref=ref, ref0=0)
    seen = 0
    for name, lines in cases.items():
        case["sam"] = ("\n".join(lines) + "\n").encode()
        bam_fn, canon = bam_of(str(tmp_path), case, sort=False, extra_filtered=False)
        for per_chunk in (1, 100):
            f = feed_bam(bam_fn, case, per_chunk)
            g = feed_text(case, canon)
            f.find_candidates(min_coverage=1, threshold=0.1)
            g.find_candidates(min_coverage=1, threshold=0.1)
            assert f.text_stats() == g.text_stats(), name
            assert f.stats()["anomalies"] == g.stats()["anomalies"], name
            seen |= f.stats()["anomalies"]
    assert seen & 1 and seen & 2 and seen & 4


def test_the_aux_walk_on_the_device_equals_the_host_renderer(tmp_path):
    """the ten placeholder-CIGAR records of tests/aux_walk_cases.py in one chunk, starting at every offset modulo 4, the last one ending at
    the chunk's last byte: the records on the device against the text path on the lines the host renderer prints for them"""
    import aux_walk_cases as aw
    bam, want = aw.bam()
    path = str(tmp_path / "aux.bam")
    bam.write(path)
    r = _hostapi.BamReader(path, threads=1)
    r.query(aw.CTG)
    big, off = np.empty(1 << 16, np.uint8), np.empty(16, np.int64)
    n, k = r.readinto(big, off)
    assert k == 10 and {int(o) % 4 for o in off[:k]} == {0, 1, 2, 3}
    chunk = big[:n].copy()                                                      # the last record ends with the buffer
    assert off[k - 1] + 4 + int.from_bytes(chunk[off[k - 1]:off[k - 1] + 4].tobytes(), "little") == len(chunk) == n
    text = r.render(chunk, off, k)
    assert [l.split(b"\t")[5].decode() for l in text.splitlines()] == want
    case = dict(ctg=aw.CTG, ref="".join("ACGT"[(i * 7) % 4] for i in range(aw.REF_LEN)), ref0=0)
    f = frontend_of(case)
    f.bam_options(r.tid)
    f.add_bam(chunk, n, off, k)
    g = feed_text(case, text)
    r.close()
    reads, _ = same_results(f, g, evc=dict(min_coverage=1, threshold=0.1))
    assert reads > 0 and f.text_stats()["lines"] == 10
    f.close()
    g.close()


def test_a_malformed_record_is_named(tmp_path):
    case = fc.synth(5, n_reads=40, ref_len=2000)
    bam_fn, _ = bam_of(str(tmp_path), case, extra_filtered=False)
    r = _hostapi.BamReader(bam_fn, threads=1)
    r.query(case["ctg"])
    buf, off = np.empty(1 << 20, np.uint8), np.empty(1000, np.int64)
    n, k = r.readinto(buf, off)
    buf[off[3] + 20:off[3] + 24] = np.frombuffer(np.int32(100000).tobytes(), np.uint8)     # l_seq beyond block_size
    f = frontend_of(case)
    f.bam_options(r.tid)
    with pytest.raises(_capi.MalformedRecord) as ei:
        f.add_bam(buf, n, off, k)
    assert ei.value.index == 3


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _files(tmp, seed=91, index=True, **kw):
    case = pileup_synth.synth_case(seed=seed, **kw)
    fa = os.path.join(tmp, "ref.fa")
    seq = "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:])
    text, fai = bf.fasta_of({case["ctg"]: seq, "chrOther": "ACGT" * 30})
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    bam = bf.Bam(case["sam"], [(case["ctg"], case["ref_len"]), ("chrOther", 120)])
    bam_fn = os.path.join(tmp, "reads.bam")
    bam.write(bam_fn, block=5000, index=index)
    sam = os.path.join(tmp, "canon.sam")
    open(sam, "w").write(bam.canonical())
    return case, fa, bam_fn, sam


def _model(tmp):
    from clair_amd import weights
    w = weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1)
    return weights.save_weights(os.path.join(tmp, "model"), w)[:-4]


@pytest.mark.parametrize("index", [True, False], ids=["bai", "scan"])
def test_callVarBam_native_writes_the_samtools_vcf(tmp_path, monkeypatch, caplog, index):
    from clair_amd import callVarBam
    tmp = str(tmp_path)
    case, fa, bam_fn, sam = _files(tmp, index=index, dup_burst=4)
    ck = _model(tmp)
    base = ["--chkpnt_fn", ck, "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--ref_fn", fa, "--ctgName", case["ctg"]]
    n_rows = 0
    for region in ([], ["--ctgStart", "300", "--ctgEnd", "2500"]):
        for fe in ("device", "host"):
            want, got = os.path.join(tmp, "want.vcf"), os.path.join(tmp, "got.vcf")
            callVarBam.main(base + region + ["--bam_fn", sam, "--samtools", FAKE_SAMTOOLS, "--call_fn", want, "--front_end", fe])
            with caplog.at_level(logging.INFO):
                caplog.clear()
                callVarBam.main(base + region + ["--bam_fn", bam_fn, "--samtools", "/nonexistent/samtools", "--bam_reader", "native", "--call_fn", got,
                                                 "--front_end", fe])
            assert open(got).read() == open(want).read(), (region, fe)
            if fe == "device":
                assert "BAM records decoded on the device" in caplog.text
            n_rows += len([l for l in open(want).read().splitlines() if not l.startswith("#")])
    assert n_rows > 60
    # the device front end's fall-back to the host stages reads the rendered text
    monkeypatch.setattr(_capi.Frontend, "budget_binds", lambda self, available_slots=5000000: True)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        callVarBam.main(base + ["--bam_fn", bam_fn, "--samtools", "/nonexistent/samtools", "--bam_reader", "native", "--call_fn", got, "--front_end", "auto"])
    assert "device front end not used" in caplog.text
    callVarBam.main(base + ["--bam_fn", sam, "--samtools", FAKE_SAMTOOLS, "--call_fn", want, "--front_end", "host"])
    assert open(got).read() == open(want).read()


def test_callVarBamParallel_run_native(tmp_path):
    from clair_amd import callVarBamParallel as par
    tmp = str(tmp_path)
    case, fa, bam_fn, sam = _files(tmp, seed=55)
    ck = _model(tmp)
    common = ["--chkpnt_fn", ck, "--bam_fn", bam_fn, "--ref_fn", fa, "--samtools", "/nonexistent/samtools", "--includingAllContigs", "--refChunkSize", "700",
              "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--python", sys.executable, "--bam_reader", "native"]
    lines = par.commands(par.build_parser().parse_args(common + ["--output_prefix", os.path.join(tmp, "one", "var")]))
    lines = [l for l in lines if '--ctgName "%s"' % case["ctg"] in l]
    assert len(lines) == 5 and all('--bam_reader "native"' in l for l in lines)
    os.makedirs(os.path.join(tmp, "one"))
    for line in lines:
        argv = shlex.split(line)
        r = subprocess.run([sys.executable, "-m"] + argv[argv.index("-m") + 1:], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, "-m", "clair_amd.callVarBamParallel", "--run", "--readers", "2", "--output_prefix", os.path.join(tmp, "all", "var")] + common,
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = sorted(n for n in os.listdir(os.path.join(tmp, "one")) if case["ctg"] in n)
    assert len(names) == 5
    rows = 0
    for n in names:
        a, b = open(os.path.join(tmp, "one", n)).read(), open(os.path.join(tmp, "all", n)).read()
        assert a == b, n
        rows += len([x for x in a.splitlines() if not x.startswith("#")])
    assert rows > 30
