"""The training-set builder on the GPU (clair_amd/csrc/train_set.hip through the C ABI): sampled sites, pairing, labels and gathered windows
against the sequential host stages, the host twin (clair_host_train_set_*) and the plain-Python rules of tests/train_set_cases.py -- every
compared quantity an integer or a byte string -- and make_train_set --front_end device against --front_end host."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import frontend_cases as fc  # noqa: E402
import train_set_cases as tc  # noqa: E402
from test_frontend_gpu import device_frontend  # noqa: E402

from clair_amd import _hostapi  # noqa: E402

pytestmark = pytest.mark.gpu


def check(case, rows, seed, p_near, p_outside, amp, bed=None, region=None, evc_min_coverage=4.0, evc_min_mq=0, dcov=250, pile_min_mq=0, min_coverage=0,
          left_edge=True, slabs=1):
    """One case through the device path and through the host path -> (sampled sites, stats of the pairing); asserts that they agree."""
    ctg = case["ctg"]
    truth, truth_labels = tc.truth_table(rows)
    rng = region or (None, None)
    keys = (_hostapi.train_set_key(ctg, seed, 1), _hostapi.train_set_key(ctg, seed, 2))
    # expected: the sequential candidate search with threshold 0, filtered by the dict-construction restatement and the draw in Python integers
    eligible = fc.host_candidates(case, threshold=0.0, min_coverage=evc_min_coverage, min_mq=evc_min_mq, ctg_start=rng[0], ctg_end=rng[1], bed=bed)
    sampled, n_near, n_outside = tc.sampled_of(eligible, truth, p_near, p_outside, seed, ctg)
    lo, hi = case["ref0"] - 64, case["ref0"] + len(case["ref"]) + 64
    inside = truth[(truth >= rng[0]) & (truth <= rng[1])] if region else truth
    sites = np.union1d(inside[(inside - 1 >= lo) & (inside - 1 < hi)], sampled).astype(np.int64)

    f = device_frontend(case, slabs=slabs, dcov=dcov, pile_min_mq=pile_min_mq, evc_min_mq=evc_min_mq, pile_region=region)
    try:
        got = f.sample_candidates(truth, p_near, p_outside, keys[0], min_coverage=evc_min_coverage, ctg_start=rng[0], ctg_end=rng[1], bed=bed)
        assert got == (len(sites), n_near, n_outside)
        assert np.array_equal(f.candidates(), sites)
        n = f.build_windows(min_coverage=min_coverage, drop_non_iupac_centre=False, consider_left_edge=left_edge)
        assert f.stats()["anomalies"] == 0 and f.host_anomalies == 0 and not f.budget_binds()
        hc, hs, hcounts = fc.host_windows(case, candidates=sites, pile_region=region, dcov=dcov, min_mq=pile_min_mq, min_coverage=min_coverage,
                                          consider_left_edge=left_edge)
        assert n == len(hc)
        # pairing and labels: the twin over the host's windows, and the plain-Python loop
        kept, want = _hostapi.train_set_pair(hc, truth, bed, amp, keys[1])
        py_kept, py_want = tc.pair_of(hc, truth, bed, amp, seed, ctg)
        assert np.array_equal(kept, py_kept) and want == py_want
        labels, in_set = _hostapi.train_set_labels(hc[kept], hs[kept][:, 16] if len(kept) else np.zeros(0, np.uint8), truth, truth_labels, bed)
        stats = f.pair(truth, truth_labels, amp, keys[1], bed=bed)
        assert stats == dict(v=want["v"], c=want["c"], kept_var=want["kept_var"], kept_non=want["kept_non"], in_set=int(in_set.sum()))
        k = len(kept)
        centres, seqs, dl, ds = f.train_set_info(0, k)
        assert np.array_equal(centres, hc[kept]) and np.array_equal(seqs, hs[kept].reshape(k, 34))         # order: variant windows, then the kept non-variant ones
        assert np.array_equal(dl, labels) and np.array_equal(ds, in_set)
        counts = f.train_set_counts(0, k)
        assert counts.dtype == np.int16 and counts.tobytes() == hcounts[kept].astype(np.int16).tobytes()
        if k > 3:       # a range inside the list
            assert f.train_set_counts(2, k - 3).tobytes() == counts[2:k - 1].tobytes()
            assert np.array_equal(f.train_set_info(2, k - 3)[0], centres[2:k - 1])
        with pytest.raises(Exception):
            f.train_set_counts(0, k + 1)
    finally:
        f.close()
    want.update(n_near=n_near, n_outside=n_outside, windows=len(hc), kept=k, in_set=int(in_set.sum()))
    return sampled, want


@pytest.mark.parametrize("path", tc.EVC_GOLDEN, ids=lambda p: os.path.basename(p)[len("train_set_evc_"):-len(".json.gz")])
def test_golden_cases(path):
    """The inputs of the records minted from ExtractVariantCandidates --gen4Training: with the probabilities on either side of the record's
    draw the sampled sites are the reference's rows; with both modes' probabilities they are the restatement's."""
    case = tc.evc_golden(path)
    rng = np.random.default_rng(1)
    positions = case["truth"] if case["truth"] is not None else np.sort(rng.integers(1, len(case["ref"]), 25))
    rows = tc.truth_rows(case["ctg"], positions, rng)
    u = case["uniform"]
    exact = (1.0, 1.0) if case["truth"] is None else (1.0 if u <= tc.NEAR_PROB else 0.0, 1.0 if u <= tc.OUTSIDE_PROB else 0.0)
    kw = dict(bed=case["bed"], region=case["ctg_range"], evc_min_coverage=case["min_coverage"], slabs=2)
    if "var_near" in path:
        sampled, st = check(case, rows, 5, exact[0], exact[1], 2.0, **kw)
        assert np.array_equal(sampled, case["expected_positions"]) and [st["n_near"], st["n_outside"]] == case["counters"]
    elif "var_all" in path:
        # (every eligible site: 2 965 windows; the record's own probabilities, and a thinner draw of both classes)
        sampled, st = check(case, rows, 5, exact[0], exact[1], 0.5, **kw)
        assert np.array_equal(sampled, case["expected_positions"]) and [st["n_near"], st["n_outside"]] == case["counters"]
        sampled, st = check(case, rows, 6, 0.6, 0.05, 2.0, min_coverage=4, **kw)
        assert st["n_near"] > 5 and st["n_outside"] > 50 and 0 < st["kept_non"] < st["c"]
    else:
        # the record's own rows: --outputProb 1.0 without truth rows pins the device's eligibility rule (bed, ctg range, --minCoverage) to the reference's
        sampled, st = check(case, [], 7, exact[0], exact[1], 2.0, **kw)
        assert np.array_equal(sampled, case["expected_positions"]) and st["n_near"] == 0 and st["n_outside"] == len(sampled) > 1000
        sampled, st = check(case, rows, 7, 0.3, 0.3, 1.0, min_coverage=2, left_edge="bed" in path, **kw)
        assert len(sampled) > 200 and st["v"] > 10 and 0 < st["kept_non"] < st["c"] and st["in_set"] > 10


@pytest.mark.parametrize("block", range(4))
def test_fuzz_against_the_host_path(block):
    """Random alignments x random truth lists x the options of both stages (regions, bed intervals, depth floors, dcov, slab cuts) x both
    modes with probabilities 0.05 - 1.0."""
    done = kept = 0
    for seed in range(block * 12, block * 12 + 6):
        case, pile_kw, evc_kw, region = fc.fuzz_case(seed)
        rng = np.random.default_rng(500 + seed)
        positions = np.sort(rng.integers(1, len(case["ref"]) + 1, int(rng.integers(0, 40))))      # repeats and clusters included
        rows = tc.truth_rows(case["ctg"], positions, rng)
        p_near = float(rng.choice([0.05, 0.3, 1.0]))
        p_outside = p_near if seed % 2 else float(rng.choice([0.05, 0.2, 1.0]))      # odd seeds: plain mode
        _sampled, st = check(case, rows, seed, p_near, p_outside, float(rng.choice([0.5, 2, 2, 50])), bed=evc_kw["bed"], region=region,
                             evc_min_coverage=evc_kw["min_coverage"], evc_min_mq=evc_kw["min_mq"], dcov=pile_kw["dcov"], pile_min_mq=pile_kw["min_mq"],
                             min_coverage=pile_kw["min_coverage"], left_edge=seed % 3 != 0, slabs=1 + seed % 3)
        done += st["windows"]
        kept += st["kept"]
    assert done > 200 and kept > 60


def test_more_windows_than_a_scan_block():
    """ref_len 5 200 with probability 1: more than 4 096 windows are compacted (two scan blocks) and gathered in one call (11 MB: two rounds
    through the staging buffer of 4 096 rows)."""
    case = fc.synth(61, n_reads=700, ref_len=5200, read_len=(100, 400), iupac=False)
    rng = np.random.default_rng(2)
    rows = tc.truth_rows(case["ctg"], np.sort(rng.integers(1, 5200, 60)), rng)
    _sampled, st = check(case, rows, 1, 1.0, 1.0, 1000.0, evc_min_coverage=1.0, slabs=2)
    assert st["windows"] > 4096 and st["kept"] > 4096 and st["r"] == 1.0


EDGES = {
    "no_truth_rows": dict(truth=[], p=0.2),
    "no_sampled_site": dict(truth=[300, 900, 1500], p=0.0),                          # c == 0 as well: r = 1, only the truth windows
    "nothing_at_all": dict(truth=[], p=0.0),
    "every_non_variant_outside_the_bed": dict(truth=[300, 900, 1500], p=0.3, bed=[(100, 1600)], pair_bed=[(299, 300), (899, 900), (4000, 5000)]),
    "duplicate_truth_keys": dict(truth=[300, 300, 900, 900, 900, 1500], p=0.2),
    "bed_ends_at_a_site": dict(truth=[300, 800, 801, 1500], p=0.5, bed=[(100, 800), (1000, 1800)]),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_cases(name):
    e = EDGES[name]
    case = fc.synth(62, n_reads=260, ref_len=1900, iupac=False)
    rng = np.random.default_rng(3)
    rows = tc.truth_rows(case["ctg"], e["truth"], rng)
    if name == "duplicate_truth_keys":         # the last row of a key wins: make the rows of one position differ, a multi-allelic one among them
        rows = ["chrS 300 A C 0 1", "chrS 300 C A,T 1 2", "chrS 900 G GTT 0 1", "chrS 900 AT A 1 1", "chrS 900 T TAA,TA 1 2", "chrS 1500 G C 1 1"]
    bed = e.get("bed")
    if "pair_bed" in e:
        # sampled inside one bed, paired against another that holds the truth sites only (looked up as they stand): c == 0 with windows present
        sampled, st = check_two_beds(case, rows, e["p"], bed, e["pair_bed"])
        assert st["c"] == 0 and st["kept_non"] == 0 and st["v"] == 3 and st["windows"] > 20
        return
    _sampled, st = check(case, rows, 4, e["p"], e["p"], 2.0, bed=bed)
    if name == "no_truth_rows":
        assert st["v"] == 0 and st["c"] > 20 and st["r"] == 0.0 and st["kept"] == 0
    elif name == "no_sampled_site":
        assert st["v"] == 3 and st["c"] == 0 and st["r"] == 1.0 and st["kept"] == 3
    elif name == "nothing_at_all":
        assert st["windows"] == 0 and st["kept"] == 0
    elif name == "duplicate_truth_keys":
        assert st["v"] == 3 and st["kept_var"] == 3
    else:
        assert st["v"] == 4 and st["in_set"] < st["kept"]        # 800: the interval's end, outside as it stands; 801 too; 300 and 1500 inside


def check_two_beds(case, rows, p, sample_bed, pair_bed):
    """check() with the pairing's bed different from the sampling's"""
    ctg = case["ctg"]
    truth, truth_labels = tc.truth_table(rows)
    keys = (_hostapi.train_set_key(ctg, 4, 1), _hostapi.train_set_key(ctg, 4, 2))
    eligible = fc.host_candidates(case, threshold=0.0, min_coverage=4.0, min_mq=0, bed=sample_bed)
    sampled, n_near, n_outside = tc.sampled_of(eligible, truth, p, p, 4, ctg)
    sites = np.union1d(truth, sampled).astype(np.int64)
    f = device_frontend(case)
    try:
        assert f.sample_candidates(truth, p, p, keys[0], bed=sample_bed) == (len(sites), n_near, n_outside)
        f.build_windows(min_coverage=0, drop_non_iupac_centre=False)
        assert f.stats()["anomalies"] == 0 and f.host_anomalies == 0 and not f.budget_binds()
        hc, hs, hcounts = fc.host_windows(case, candidates=sites)
        kept, want = tc.pair_of(hc, truth, pair_bed, 2.0, 4, ctg)
        labels, in_set = _hostapi.train_set_labels(hc[kept], hs[kept][:, 16], truth, truth_labels, pair_bed)
        stats = f.pair(truth, truth_labels, 2.0, keys[1], bed=pair_bed)
        assert stats == dict(v=want["v"], c=want["c"], kept_var=want["kept_var"], kept_non=want["kept_non"], in_set=int(in_set.sum()))
        centres, seqs, dl, ds = f.train_set_info(0, len(kept))
        assert np.array_equal(centres, hc[kept]) and np.array_equal(dl, labels) and np.array_equal(ds, in_set)
        assert f.train_set_counts(0, len(kept)).tobytes() == hcounts[kept].astype(np.int16).tobytes()
    finally:
        f.close()
    want["windows"] = len(hc)
    return sampled, want


def test_pair_needs_windows_and_a_new_build_forgets_the_set():
    case = fc.synth(62, n_reads=260, ref_len=1900, iupac=False)
    truth, labels = tc.truth_table(["chrS 300 A C 0 1"])
    f = device_frontend(case)
    try:
        with pytest.raises(Exception, match="no windows yet"):
            f.pair(truth, labels, 2.0, 0)
        f.sample_candidates(truth, 0.1, 0.1, 0)
        f.build_windows(min_coverage=0, drop_non_iupac_centre=False)
        with pytest.raises(Exception, match="no paired set yet"):
            f.train_set_counts(0, 1)
        st = f.pair(truth, labels, 2.0, 0)
        assert st["v"] == 1 and len(f.train_set_counts(0, 1)) == 1
        f.build_windows(min_coverage=0, drop_non_iupac_centre=False)
        with pytest.raises(Exception, match="no paired set yet"):
            f.train_set_info(0, 1)
        with pytest.raises(Exception, match="not ascending"):
            f.pair(np.array([5, 3]), np.zeros((2, 4), np.uint8), 2.0, 0)
    finally:
        f.close()


@pytest.mark.parametrize("region", [[], ["--ctgStart", "400", "--ctgEnd", "2400"]], ids=["contig", "region"])
def test_cli_device_equals_cli_host(tmp_path, region):
    """make_train_set --front_end device and --front_end host on one synthetic BAM, whole contig and a ctg range: both output files, byte for byte."""
    truth = [5, 200, 214, 400, 415, 650, 666, 800, 817, 1000, 1031, 1700, 1700, 2100, 2400, 2950]
    w = tc.world(tmp_path, 51, truth, bed=[(100, 800), (900, 1300), (1500, 1500), (1600, 2960)], n_reads=400)
    out = {}
    for where in ("device", "host"):
        out[where] = [str(tmp_path / (where + ".gz")), str(tmp_path / (where + ".npz"))]
        r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set"] + tc.cli_args(w, "--front_end", where, "--tensor_fn", out[where][0], "--set_fn", out[where][1],
                                                                                           "--sampling", "near_variant", "--near_prob", "0.7", "--outside_prob", "0.06",
                                                                                           "--seed", "12", "--minCoverage", "3", *region),
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        assert ("device front end:" in r.stderr) == (where == "device") and "device front end not used" not in r.stderr
    for a, b in zip(out["device"], out["host"]):
        assert os.path.getsize(a) > 2000 and open(a, "rb").read() == open(b, "rb").read()
    positions = np.load(out["device"][1])["positions"]
    # (a set of some size: 9 of the truth sites lie in the range and in the bed, and amp 2 pairs non-variant windows with them)
    assert len(positions) > (15 if region else 25) and (not region or (positions.min() >= 400 and positions.max() <= 2400 and 415 in positions.tolist()))
