"""Read subsampling on the MI355X (docs/subsample.md): clair_frontend_bam_subsample, the clause fe_bam_records_kernel adds to the view.
A BAM A read with the rule against a BAM B that holds exactly the records a Python restatement keeps (tests/subsample_cases.py): the same
line counters, slabs, candidates, windows and indel tables, and the same files out of callVarBam and make_train_set."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import subsample_cases as sc  # noqa: E402

from clair_amd import _capi, _hostapi  # noqa: E402


def records_of(path, ctg, region=None):
    """every record the reader yields, as one chunk -> (buffer, bytes, offsets, records)"""
    r = _hostapi.BamReader(path, threads=2)
    r.query(ctg, *(region or (None, None)))
    buf, off = np.empty(1 << 22, np.uint8), np.empty(4096, np.int64)
    n, k = r.readinto(buf, off)
    assert 0 < k < len(off) and r.readinto(np.empty(1 << 16, np.uint8), np.empty(8, np.int64)) == (0, 0)
    tid = r.tid
    r.close()
    return buf, n, off[:k].copy(), k, tid


def name_of(buf, at):
    return buf[at + 36:at + 36 + int(buf[at + 12]) - 1].tobytes()


def fed(w, path, subsample=None, split=None, lookup=False, region=None):
    """a front end fed the records of `path`: in one add_bam call, or in two that meet at record `split` -> (front end, chunk)"""
    buf, n, off, k, tid = records_of(path, w["ctg"], region)
    f = _capi.Frontend(0, w["ref"], 0, -64, len(w["ref"]) + 64)
    f.bam_options(tid, region=region)
    if lookup:
        f.bam_lookup(True)
    if subsample is not None:
        f.bam_subsample(*subsample)
    if split is None:
        f.add_bam(buf[:n], n, off, k)              # the chunk ends with its last record: the last name is read near the end of the buffer
    else:
        cut = int(off[split])
        f.add_bam(buf[:cut], cut, off[:split], split)
        f.add_bam(buf[cut:n], n - cut, off[split:] - cut, k - split)
    return f, (buf, n, off, k)


def same_front_ends(f, g, evc):
    assert f.text_stats() == g.text_stats() and f.text_stats()["lines"] > 0
    assert f.stats()["slabs"] == g.stats()["slabs"] == len(f.slab_reads) == len(g.slab_reads)
    for s, (a, b) in enumerate(zip(f.slab_reads, g.slab_reads)):                  # the alignments of every slab, every field of them
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), s
    assert f.find_candidates(**evc) == g.find_candidates(**evc) and np.array_equal(f.candidates(), g.candidates())
    n = f.build_windows(min_coverage=0, drop_non_iupac_centre=False)
    assert n == g.build_windows(min_coverage=0, drop_non_iupac_centre=False)
    for x, y in zip(f.window_info(0, n), g.window_info(0, n)):
        assert np.array_equal(x, y)
    assert np.array_equal(f.window_counts(0, n), g.window_counts(0, n))
    for s in range(len(f.slab_reads)):                                            # what every alignment's operations and bases offer the windows
        assert np.array_equal(f.read_tuples(s), g.read_tuples(s)), s
    assert f.stats()["anomalies"] == g.stats()["anomalies"]
    return n


def compare(w, evc, region=None):
    n_a, n_b = sc.assert_a_real_subset(w["lines_a"], w["lines_b"], w["ctg"], region)
    rule = (w["seed"], w["frac"])
    f, (buf, _, off, k) = fed(w, w["a"], subsample=rule, region=region)
    g, (_, _, _, k_b) = fed(w, w["b"], region=region)
    assert f.text_stats()["lines"] == n_b
    n = same_front_ends(f, g, evc)
    f.close()
    g.close()
    # again in two calls that meet at a record boundary in the middle: B is cut where A's cut falls among its records
    half = k // 2
    half_b = sum(sc.keeps(name_of(buf, int(off[i])), *rule) for i in range(half))
    assert 0 < half_b < k_b
    f, _ = fed(w, w["a"], subsample=rule, split=half, region=region)
    g, _ = fed(w, w["b"], split=half_b, region=region)
    assert f.stats()["slabs"] == 2 and same_front_ends(f, g, evc) == n
    # and the rule off (F <= 0) or at F = 1 is A as it stands
    for frac in (0.0, 1.0):
        h, _ = fed(w, w["a"], subsample=(w["seed"], frac), region=region)
        assert h.text_stats()["lines"] == n_a
        h.close()
    f.close()
    g.close()
    return n


@pytest.mark.parametrize("frac,seed", [(0.5, 0), (0.5, 11), (0.1, 0)])
def test_a_with_the_rule_is_b(tmp_path, frac, seed):
    w = sc.world(tmp_path, seed=seed, frac=frac)
    assert compare(w, dict(min_coverage=3, threshold=0.1)) > 20


def test_a_with_the_rule_is_b_inside_a_region(tmp_path):
    w = sc.world(tmp_path, seed=0, frac=0.5)
    assert compare(w, dict(min_coverage=3, threshold=0.1), region=(700, 1900)) > 10


def test_names_of_every_length_at_every_alignment(tmp_path):
    w = sc.name_family(tmp_path)
    buf, n, off, k, _ = records_of(w["a"], w["ctg"])
    seen = {}
    for at in off.tolist():
        seen.setdefault(int(buf[at + 12]) - 1, set()).add((at + 36) % 4)
    assert seen == {length: {0, 1, 2, 3} for length in sc.NAME_LENGTHS}
    assert int(buf[off[-1] + 12]) - 1 == 254 and n - (int(off[-1]) + 36 + 254) < 64      # the longest name sits in the last record of the chunk
    assert compare(w, dict(min_coverage=1, threshold=0.1)) > 0


def test_the_rule_is_refused_after_the_first_record(tmp_path):
    w = sc.name_family(tmp_path)
    f, _ = fed(w, w["a"], subsample=(0, 0.5))
    lines = f.text_stats()["lines"]
    with pytest.raises(_capi.EngineError) as ei:
        f.bam_subsample(0, 0.8)
    assert "cannot change once records were added" in str(ei.value)
    with pytest.raises(_capi.EngineError) as lookup:                              # the error bam_lookup gives in the same situation
        f.bam_lookup(True)
    assert str(lookup.value).replace("look-up", "subsample").replace("bam_lookup", "bam_subsample") == str(ei.value)
    assert f.text_stats()["lines"] == lines
    f.close()
    g = _capi.Frontend(0, w["ref"], 0, -64, len(w["ref"]) + 64)
    with pytest.raises(_capi.EngineError) as ei:                                  # ... and before bam_options
        g.bam_subsample(0, 0.5)
    assert "clair_frontend_bam_options first" in str(ei.value)
    g.bam_options(0)
    for seed in (-1, 1 << 32):
        with pytest.raises(_capi.EngineError) as ei:
            g.bam_subsample(seed, 0.5)
        assert "4294967295" in str(ei.value)
    g.close()


def test_a_malformed_record_the_rule_would_drop_is_still_reported(tmp_path):
    w = sc.world(tmp_path, seed=0, frac=0.5)
    buf, n, off, k, tid = records_of(w["a"], w["ctg"])
    dropped = [i for i in range(k) if not sc.keeps(name_of(buf, int(off[i])), 0, 0.5) and not int.from_bytes(buf[off[i] + 18:off[i] + 20].tobytes(), "little") & 2316]
    victim = dropped[len(dropped) // 2]
    assert victim > 0
    buf[off[victim] + 20:off[victim] + 24] = np.frombuffer(np.int32(100000).tobytes(), np.uint8)     # l_seq beyond block_size
    f = _capi.Frontend(0, w["ref"], 0, -64, len(w["ref"]) + 64)
    f.bam_options(tid)
    f.bam_subsample(0, 0.5)
    with pytest.raises(_capi.MalformedRecord) as ei:
        f.add_bam(buf[:n], n, off, k)
    assert ei.value.index == victim
    f.close()


def indel_positions(lines, ctg):
    """1-based positions around the insertions and deletions of the viewable lines, ascending"""
    out = set()
    for line in lines:
        if not sc.viewable(line, ctg):
            continue
        col = line.split("\t")
        rp = int(col[3])
        for n, op in bf.parse_cigar(col[5]):
            if op in (1, 2):
                out.update((rp - 1, rp))
            if op in (0, 2, 3, 7, 8):
                rp += n
    return np.array(sorted(p for p in out if p > 0), dtype=np.int64)


def test_indel_tables_of_a_with_the_rule_are_those_of_b(tmp_path):
    w = sc.world(tmp_path, seed=0, frac=0.5)
    positions = indel_positions(w["lines_b"], w["ctg"])[::7][:24]
    f, _ = fed(w, w["a"], subsample=(0, 0.5), lookup=True)
    g, _ = fed(w, w["b"], lookup=True)
    whole, _ = fed(w, w["a"], lookup=True)
    got, want, more = f.indel_table(positions), g.indel_table(positions), whole.indel_table(positions)
    assert len(positions) >= 12 and int((want[1] > 0).sum()) >= 6
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert not np.array_equal(more[2], want[2])                                   # the depth of the whole file is another
    for x in (f, g, whole):
        x.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _model(tmp):
    from clair_amd import weights
    w = weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1)
    return weights.save_weights(os.path.join(tmp, "model"), w)[:-4]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("subsample_e2e"))
    w = sc.world(tmp, seed=0, frac=0.5)
    sc.assert_a_real_subset(w["lines_a"], w["lines_b"], w["ctg"])
    w["tmp"] = tmp
    w["base"] = ["--chkpnt_fn", _model(tmp), "--threshold", "0.15", "--minCoverage", "4", "--batch_size", "64", "--ref_fn", w["fa"], "--ctgName", w["ctg"],
                 "--samtools", "/nonexistent/samtools", "--bam_reader", "native"]
    return w


def vcf_of(w, name, *flags):
    from clair_amd import callVarBam
    path = os.path.join(w["tmp"], name + ".vcf")
    callVarBam.main(w["base"] + ["--call_fn", path] + list(flags))
    return open(path, "rb").read()


def rows_of(vcf):
    return [l for l in vcf.decode().splitlines() if not l.startswith("#")]


def test_callVarBam_ensemble_subsample_is_the_ensemble_with_b(e2e):
    w = e2e
    want = vcf_of(w, "files", "--bam_fn", w["a"], "--ensemble_bam_fn", w["b"])
    got = vcf_of(w, "virtual", "--bam_fn", w["a"], "--ensemble_subsample", "0.5")
    assert got == want and len(rows_of(want)) > 30
    assert want != vcf_of(w, "alone", "--bam_fn", w["a"])
    # the order of the sources: --bam_fn, the files whole, the virtual BAMs
    want = vcf_of(w, "files3", "--bam_fn", w["a"], "--ensemble_bam_fn", w["a"], "--ensemble_bam_fn", w["b"])
    assert vcf_of(w, "mixed3", "--bam_fn", w["a"], "--ensemble_bam_fn", w["a"], "--ensemble_subsample", "0.5:0") == want


def test_callVarBam_subsample_with_the_native_look_up_is_the_plain_run_on_b(e2e):
    w = e2e
    for more in ([], ["--pysam_for_all_indel_bases"]):
        want = vcf_of(w, "plain_b", "--bam_fn", w["b"], "--indel_lookup", "native", *more)
        got = vcf_of(w, "half_a", "--bam_fn", w["a"], "--subsample", "0.5", "--indel_lookup", "native", *more)
        assert got == want and len(rows_of(want)) > 20
        assert got != vcf_of(w, "whole_a", "--bam_fn", w["a"], "--indel_lookup", "native", *more)


def test_make_train_set_device_equals_host_with_the_flag(e2e):
    from clair_amd import make_train_set as mts
    w = e2e
    var = os.path.join(w["tmp"], "truth.var")
    open(var, "w").write("".join("%s %d A C 0 1\n" % (w["ctg"], p) for p in (100, 420, 435, 900, 1500, 2380, 2600)))
    out = {}
    for name, bam, more in (("device", w["a"], ["--front_end", "device", "--subsample", "0.5"]), ("host", w["a"], ["--front_end", "host", "--subsample", "0.5"]),
                            ("physical", w["b"], ["--front_end", "device"])):
        out[name] = [os.path.join(w["tmp"], name + ".gz"), os.path.join(w["tmp"], name + ".npz")]
        mts.main(["--ref_fn", w["fa"], "--ctgName", w["ctg"], "--var_fn", var, "--samtools", "/nonexistent/samtools", "--bam_reader", "native", "--bam_fn", bam,
                  "--outputProb", "0.05", "--amp", "6", "--minCoverage", "3", "--tensor_fn", out[name][0], "--set_fn", out[name][1]] + more)
    for a, b in zip(out["device"], out["host"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    assert open(out["device"][0], "rb").read() == open(out["physical"][0], "rb").read()
    assert len(np.load(out["device"][1])["positions"]) > 10
