"""The training-set builder without a GPU: the rules of csrc/train_set_core.h through the host twin (clair_host_train_set_*) against their
plain-Python restatement (tests/train_set_cases.py) and against golden records minted from the reference's scripts, make_train_set's
host path end to end, the PairWithNonVariants filter, and --set_fn of train."""
import gzip
import json
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

from clair_amd import _hostapi, make_train_set as mts  # noqa: E402


def golden_id(path):
    return os.path.basename(path)[len("train_set_"):-len(".json.gz")]


# -- 1. the draws ---------------------------------------------------------------------------------------------------------------------
def test_known_answer_draw():
    key = _hostapi.train_set_key("chrS", 7, _hostapi.TS_STAGE_SAMPLE)
    assert key & tc.MASK == 0x3dbe70b4759934f6 == tc.key_of(7, "chrS", 1)
    _cls, draws, _s, _n, _o = _hostapi.train_set_sample([1000], [], 1.0, 1.0, key)
    assert int(draws[0]) == 0x7cd44b49ac63 == tc.draw_of(tc.key_of(7, "chrS", 1), 1000)


def test_draws_equal_the_python_integers():
    rng = np.random.default_rng(5)
    for ctg, seed, stage in (("chr20", 0, 1), ("chrS", 2 ** 40 + 3, 2), ("1", -5, 1)):
        key = _hostapi.train_set_key(ctg, seed, stage)
        assert key == tc.signed(tc.key_of(seed, ctg, stage))
        pos = rng.integers(1, 2 ** 31, 500)
        draws = _hostapi.train_set_sample(pos, [], 0.5, 0.5, key)[1]
        assert draws.tolist() == [tc.draw_of(key & tc.MASK, int(p)) for p in pos]


@pytest.mark.parametrize("ctg", ["chr20", "chrS"])
@pytest.mark.parametrize("seed", range(4))
def test_sampling_rate_is_binomial(seed, ctg):
    """The kept share of positions 1 .. 200 000 lies within 4 sigma of n p for the three default probabilities."""
    pos = np.arange(1, 200001)
    key = _hostapi.train_set_key(ctg, seed, 1)
    for p in (tc.PLAIN_PROB, tc.NEAR_PROB, tc.OUTSIDE_PROB):
        kept = int(_hostapi.train_set_sample(pos, [], p, p, key)[2].sum())
        sigma = (len(pos) * p * (1 - p)) ** 0.5
        print("seed %d %s p %.5f: kept %d, expected %.1f, %.2f sigma" % (seed, ctg, p, kept, len(pos) * p, (kept - len(pos) * p) / sigma))
        assert abs(kept - len(pos) * p) <= 4 * sigma


def test_two_seeds_differ_and_one_seed_repeats():
    pos = np.arange(1, 50001)
    a = _hostapi.train_set_sample(pos, [], 0.01, 0.01, _hostapi.train_set_key("chr20", 1, 1))[2]
    b = _hostapi.train_set_sample(pos, [], 0.01, 0.01, _hostapi.train_set_key("chr20", 2, 1))[2]
    again = _hostapi.train_set_sample(pos, [], 0.01, 0.01, _hostapi.train_set_key("chr20", 1, 1))[2]
    assert a.sum() > 300 and b.sum() > 300 and not np.array_equal(a, b) and np.array_equal(a, again)
    # the two stages and two contigs draw independently as well
    assert not np.array_equal(a, _hostapi.train_set_sample(pos, [], 0.01, 0.01, _hostapi.train_set_key("chr20", 1, 2))[2])
    assert not np.array_equal(a, _hostapi.train_set_sample(pos, [], 0.01, 0.01, _hostapi.train_set_key("chr21", 1, 1))[2])


# -- 2. the class rule: closed form against the reference's dict construction ----------------------------------------------------------
def test_classes_equal_the_dict_construction():
    rng = np.random.default_rng(11)
    seen = set()
    for k in range(200):
        top = int(rng.choice([60, 300, 3000]))
        truth = np.sort(rng.integers(1, top + 1, int(rng.integers(0, 41))))
        pos = np.arange(1, top + 40)
        got = _hostapi.train_set_sample(pos, truth, 1.0, 1.0, 0)[0]
        want = tc.classes_of(truth, pos)
        assert np.array_equal(got, want), "case %d: %r" % (k, truth.tolist())
        seen.update(np.diff(np.unique(truth)).tolist())
    assert {14, 15, 16, 17, 30, 31, 32, 33} <= seen        # the gaps at which two truth sites' maps touch


def test_sample_counters_and_modes():
    truth = np.array([100, 115, 400], dtype=np.int64)
    pos = np.arange(1, 600)
    cls, _d, sampled, near, outside = _hostapi.train_set_sample(pos, truth, 1.0, 0.0, 0)
    assert near == sampled.sum() == (cls == tc.NEAR).sum() and outside == 0
    assert pos[cls == tc.NEAR].tolist() == [84, 85, 130, 131, 384, 385, 415, 416]      # 100 and 115 are 15 apart: nothing between them is near
    cls, _d, sampled, near, outside = _hostapi.train_set_sample(pos, truth, 0.0, 1.0, 0)
    assert near == 0 and outside == sampled.sum() == (cls == tc.OUTSIDE).sum() and not sampled[cls == tc.TRUTH].any()
    with pytest.raises(ValueError):
        _hostapi.train_set_sample(pos, truth[::-1], 1.0, 1.0, 0)


# -- 3. golden records from the reference's scripts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", tc.EVC_GOLDEN, ids=golden_id)
def test_sampled_sites_reproduce_the_reference_rows(path):
    """ExtractVariantCandidates --gen4Training with every draw preset to one value u: the rows are the eligible sites whose probability
    admits u.  The twin with probabilities 1 / 0 on either side of u keeps the same positions and counts them alike."""
    case = tc.evc_golden(path)
    eligible = tc.eligible_of(case)
    u = case["uniform"]
    if case["truth"] is None:
        truth, p_near, p_outside = np.zeros(0, np.int64), 1.0, 1.0
    else:
        truth = np.sort(case["truth"])
        p_near, p_outside = (1.0 if u <= tc.NEAR_PROB else 0.0), (1.0 if u <= tc.OUTSIDE_PROB else 0.0)
    cls, _d, sampled, near, outside = _hostapi.train_set_sample(eligible, truth, p_near, p_outside, _hostapi.train_set_key(case["ctg"], 0, 1))
    assert len(case["expected_positions"]) > 40
    assert np.array_equal(eligible[sampled != 0], case["expected_positions"])
    assert np.array_equal(cls, tc.classes_of(truth, eligible))
    if case["counters"]:
        assert [near, outside] == case["counters"]


@pytest.mark.parametrize("path", tc.EVC_GOLDEN, ids=golden_id)
def test_cli_samples_the_reference_rows(path, tmp_path):
    """make_train_set --front_end host on every record's inputs with the record's own options (bed, ctg range, --minCoverage), probabilities on
    either side of the record's draw and an --amp that makes r = 1: the counters are the reference's, and the non-truth rows of --tensor_fn
    are the record's rows -- those whose window the pileup writes and whose position, as it stands, the pairing finds inside the bed."""
    case, doc = tc.evc_golden(path), fc.load(path)
    files = dict((n, str(tmp_path / n)) for n in ("ref.fa", "reads.sam", "truth.var", "regions.bed", "o.gz", "o.npz"))
    open(files["ref.fa"], "w").write(doc["fasta"])
    open(files["ref.fa"] + ".fai", "w").write("%s\t%d\t6\t60\t61\n" % (doc["ctg"], doc["ref_len"]))
    open(files["reads.sam"], "w").write(doc["sam"])
    u, rng = case["uniform"], case["ctg_range"]
    if doc["truth"] is None:        # a record without --var_fn: the CLI needs truth rows (v > 0 for r = 1), some of them outside the record's range
        truth_text = "".join("%s %d A C 0 1\n" % (doc["ctg"], p) for p in (150, 390, 410, 1000, 1015, 2390, 2410, 2800))
        mode = ["--sampling", "plain"]
    else:
        truth_text = doc["truth"]
        mode = ["--sampling", "near_variant", "--near_prob", "1.0" if u <= tc.NEAR_PROB else "0.0", "--outside_prob", "1.0" if u <= tc.OUTSIDE_PROB else "0.0"]
    open(files["truth.var"], "w").write(truth_text)
    truth = np.array(sorted(int(r.split()[1]) for r in truth_text.splitlines()), dtype=np.int64)
    argv = [sys.executable, "-m", "clair_amd.make_train_set", "--bam_fn", files["reads.sam"], "--ref_fn", files["ref.fa"], "--ctgName", doc["ctg"], "--var_fn",
            files["truth.var"], "--samtools", tc.FAKE_SAMTOOLS, "--front_end", "host", "--amp", "1000000", "--tensor_fn", files["o.gz"], "--set_fn", files["o.npz"]]
    if doc["bed"] is not None:
        open(files["regions.bed"], "w").write(doc["bed"])
        argv += ["--bed_fn", files["regions.bed"]]
    r = subprocess.run(argv + mode + doc["args"], capture_output=True, text=True, cwd=ROOT)       # doc["args"]: --outputProb 1.0 [--ctgStart --ctgEnd --minCoverage]
    assert r.returncode == 0, r.stderr
    # the sampled sites: the record's rows, less the truth sites (never sampled: they come in through the truth list)
    rows = case["expected_positions"][~np.isin(case["expected_positions"], truth)]
    cls = tc.classes_of(truth, rows)
    counters = case["counters"] or [int((cls == tc.NEAR).sum()), int((cls != tc.NEAR).sum())]
    meta = json.loads(str(np.load(files["o.npz"])["meta"]))
    assert [meta["n_near"], meta["n_outside"]] == counters and sum(counters) == len(rows) > 30 and meta["r"] == 1.0
    if doc["truth"] is not None:
        assert "# of candidates near variant: %d\n" % counters[0] in r.stderr and "# of candidates outside variant: %d\n" % counters[1] in r.stderr
    inside = truth if rng is None else truth[(truth >= rng[0]) & (truth <= rng[1])]
    assert rng is None or 0 < len(inside) < len(truth)
    min_coverage = int(case["min_coverage"])
    centres, seqs, counts = fc.host_windows(case, candidates=np.union1d(inside, rows), pile_region=rng, min_coverage=min_coverage)
    regions = None if case["bed"] is None else tc.BedRegions(case["bed"])
    is_truth = np.isin(centres, truth)
    keep = np.array([regions is None or int(c) in regions for c in centres], dtype=bool).reshape(len(centres)) & ~is_truth
    order = np.concatenate([np.flatnonzero(is_truth), np.flatnonzero(keep)])
    assert is_truth.sum() > 0 and 30 < keep.sum() <= len(rows) and set(centres[keep].tolist()) <= set(rows.tolist())
    assert gzip.open(files["o.gz"], "rt").read() == fc.text_of(doc["ctg"], centres[order], seqs[order], counts[order])
    assert "%d usable non-variant\n" % keep.sum() in r.stderr and "%d Truth Variants\n" % is_truth.sum() in r.stderr


def _pair_files(doc, tmp_path):
    files = dict((n, str(tmp_path / n)) for n in ("var.gz", "can.gz", "regions.bed", "paired.gz"))
    for name, key in (("var.gz", "var_tensors"), ("can.gz", "can_tensors")):
        with gzip.open(files[name], "wt") as f:
            f.write(doc[key])
    if doc["bed"] is not None:
        open(files["regions.bed"], "w").write(doc["bed"])
    return files


@pytest.mark.parametrize("path", tc.PAIR_GOLDEN, ids=golden_id)
def test_pair_filter_reproduces_the_reference_file(path, tmp_path):
    """PairWithNonVariants with an --amp that makes r = 1: the output and the logged counts of the reference's script, byte for byte; the
    twin over the two files' positions keeps the same rows."""
    doc = fc.load(path)
    files = _pair_files(doc, tmp_path)
    argv = [sys.executable, "-m", "clair_amd", "PairWithNonVariants", "--tensor_var_fn", files["var.gz"], "--tensor_can_fn", files["can.gz"], "--output_fn", files["paired.gz"],
            "--amp", repr(doc["amp"])] + (["--bed_fn", files["regions.bed"]] if doc["bed"] is not None else [])
    r = subprocess.run(argv, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert gzip.open(files["paired.gz"], "rt").read() == doc["expected"] and doc["expected"].count("\n") > 40
    wanted = [line for line in doc["log"].splitlines() if line[:1].isdigit()]
    assert len(wanted) == 5 and [line for line in r.stderr.splitlines() if line[:1].isdigit()] == wanted
    # the twin: windows = the rows of both files, truth = the variant file's positions
    var = np.array([int(x.split()[1]) for x in doc["var_tensors"].splitlines()], dtype=np.int64)
    can = np.array([int(x.split()[1]) for x in doc["can_tensors"].splitlines()], dtype=np.int64)
    bed = None if doc["bed"] is None else [(int(x.split()[1]), int(x.split()[2])) for x in doc["bed"].splitlines() if x.split()[0] == doc["ctg"]]
    v, c = _hostapi.train_set_pair_count(can, np.unique(var), bed)
    assert "%d usable non-variant" % c in wanted and _hostapi.train_set_ratio(len(var), doc["amp"], c) == 1.0
    kept, n_var = _hostapi.train_set_pair_keep(can, np.unique(var), bed, 1.0, 0)
    assert v == n_var == len(set(var.tolist()) & set(can.tolist())) > 0
    rows = doc["can_tensors"].splitlines()
    assert "".join(x.strip() + "\n" for x in doc["var_tensors"].splitlines()) + "".join(rows[i].strip() + "\n" for i in kept[n_var:]) == doc["expected"]


def test_pair_filter_thins_by_the_draws(tmp_path):
    """--amp 1: r < 1, the kept rows are those whose stage-2 draw is below r; another seed keeps another set."""
    doc = fc.load(tc.PAIR_GOLDEN[0])
    files = _pair_files(doc, tmp_path)
    outs = []
    for seed in (1, 1, 2):
        argv = [sys.executable, "-m", "clair_amd.pair_with_non_variants", "--tensor_var_fn", files["var.gz"], "--tensor_can_fn", files["can.gz"], "--output_fn",
                files["paired.gz"], "--amp", "1", "--seed", str(seed), "--bed_fn", files["regions.bed"]]
        r = subprocess.run(argv, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append(gzip.open(files["paired.gz"], "rt").read())
    var = [int(x.split()[1]) for x in doc["var_tensors"].splitlines()]
    can = [int(x.split()[1]) for x in doc["can_tensors"].splitlines()]
    bed = [(int(x.split()[1]), int(x.split()[2])) for x in doc["bed"].splitlines() if x.split()[0] == doc["ctg"]]
    kept, stats = tc.pair_of(can, var, bed, 1.0, 1, doc["ctg"])
    stats["v"] = len(var)
    r = min(1.0, float(len(var)) / stats["c"])
    key = tc.key_of(1, doc["ctg"], 2)
    regions = tc.BedRegions(bed)
    want = [p for p in can if p not in set(var) and p in regions and tc.u_of(key, p) < r]
    assert 0 < len(want) < stats["c"]
    assert [int(x.split()[1]) for x in outs[0].splitlines()] == var + want
    assert outs[0] == outs[1] != outs[2]


# -- 4. pairing and labels: the twin against the restatement --------------------------------------------------------------------------------
def test_pair_and_labels_equal_the_restatement(tmp_path):
    rng = np.random.default_rng(3)
    for k in range(40):
        centres = np.unique(rng.integers(1, 3000, int(rng.integers(0, 200))))
        truth_pos = np.sort(rng.choice(centres, int(rng.integers(0, min(len(centres), 20) + 1)))) if len(centres) else np.zeros(0, np.int64)   # repeats included
        bed = None if k % 3 == 0 else sorted((int(x), int(x + rng.integers(0, 600))) for x in rng.integers(0, 3000, int(rng.integers(1, 5))))
        amp = float(rng.choice([0.5, 1, 2, 100]))
        kept, stats = _hostapi.train_set_pair(centres, truth_pos, bed, amp, _hostapi.train_set_key("chrS", k, 2))
        want_kept, want = tc.pair_of(centres, truth_pos, bed, amp, k, "chrS")
        assert np.array_equal(kept, want_kept) and stats == want, "case %d" % k
        # labels: rows with SNPs, indels, multi-allelic calls; the last row of a repeated position wins; the set is labelled_batches'
        rows = tc.truth_rows("chrS", truth_pos, rng)
        tp, tl = tc.truth_table(rows)
        bases = rng.choice(list(b"ACGTUNRacgtn"), len(centres)).astype(np.uint8)
        labels, in_set = _hostapi.train_set_labels(centres, bases, tp, tl, bed)
        seqs = np.full((len(centres), 33), ord("A"), dtype=np.uint8)
        seqs[:, 16] = bases
        if k % 4 == 0:
            text = "".join("chrS %d %s %s\n" % (c, seqs[i].tobytes().decode().upper(), " ".join(["0"] * 1056)) for i, c in enumerate(centres.tolist()))
            bed_text = None if bed is None else "".join("chrS\t%d\t%d\n" % iv for iv in bed)
            _x, keys, want_labels = tc.expected_set(tmp_path, text, "".join(r + "\n" for r in rows), bed_text)
            rows_in = in_set != 0       # (the text holds the upper-cased sequence, as CreateTensor writes it; the rule upper-cases for itself)
            assert keys == ["chrS:%d" % c for c in centres[rows_in]] and np.array_equal(labels[rows_in], want_labels)
        assert np.array_equal(in_set != 0, np.array([chr(b).upper() in "ACGTU" and (bed is None or int(c) in tc.BedRegions(bed)) for b, c in zip(bases, centres)], dtype=bool).reshape(len(centres)))


# -- 5. make_train_set --front_end host, end to end -----------------------------------------------------------------------------------------
def _run_cli(w, *more):
    r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set"] + tc.cli_args(w, *more), capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def host_world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("train_set_host")
    truth = [5, 200, 214, 400, 415, 650, 666, 800, 817, 1000, 1031, 1700, 1700, 2100, 2400, 2950]
    # the interval [100, 800) ends exactly at the site 800: position 800, looked up as it stands, is outside; 799, the base before 800 counts as inside
    w = tc.world(tmp, 51, truth, bed=[(100, 800), (900, 1300), (1500, 1500), (1600, 2960)], n_reads=400)
    w["out"] = dict(tensor=str(tmp / "paired.gz"), set=str(tmp / "set.npz"))
    w["flags"] = ["--outputProb", "0.08", "--seed", "9", "--minCoverage", "3", "--amp", "1.5"]
    w["run"] = _run_cli(w, "--front_end", "host", "--tensor_fn", w["out"]["tensor"], "--set_fn", w["out"]["set"], *w["flags"])
    return w


def expected_rows(w, p, seed, min_coverage, amp, left_edge=True):
    """Positions, windows and pairing worked out from the sequential host stages and the plain-Python rules"""
    case, ctg = w["case"], w["case"]["ctg"]
    truth = np.array(sorted(int(r.split()[1]) for r in w["rows"]), dtype=np.int64)
    eligible = fc.host_candidates(case, threshold=0.0, min_coverage=min_coverage, min_mq=0, bed=w["bed"])
    sampled, n_near, n_outside = tc.sampled_of(eligible, truth, p, p, seed, ctg)
    sites = np.union1d(truth, sampled)
    centres, seqs, counts = fc.host_windows(case, candidates=sites, min_coverage=int(min_coverage), consider_left_edge=left_edge)
    kept, stats = tc.pair_of(centres, truth, w["bed"], amp, seed, ctg)
    stats.update(n_near=n_near, n_outside=n_outside)
    return centres[kept], seqs[kept], counts[kept], stats


def test_cli_host_path_writes_the_expected_rows(host_world, tmp_path):
    w = host_world
    centres, seqs, counts, stats = expected_rows(w, 0.08, 9, 3.0, 1.5)
    assert stats["kept_var"] >= 12 and stats["kept_non"] >= 15 and stats["c"] > stats["kept_non"]        # r < 1: the pairing thins
    text = fc.text_of(w["case"]["ctg"], centres, seqs, counts)
    assert gzip.open(w["out"]["tensor"], "rt").read() == text
    for line in ("%d Truth Variants" % stats["v"], "%d usable non-variant" % stats["c"], "%.2f of all non-variants are selected" % stats["r"]):
        assert line + "\n" in w["run"].stderr
    X, keys, labels = tc.expected_set(tmp_path, text, "".join(r + "\n" for r in w["rows"]), w["bed_text"])
    z = np.load(w["out"]["set"])
    assert len(keys) > 20 and ["%s:%d" % (str(z["ctg"]), p) for p in z["positions"]] == keys
    assert z["counts"].dtype == np.int16 and z["counts"].shape == (len(keys), 33, 8, 4) and z["labels"].dtype == np.uint8
    assert np.array_equal(_hostapi.counts_to_input(z["counts"]), X) and np.array_equal(z["labels"], labels)
    assert [s.decode() for s in z["refseq"]] == [seqs[i].tobytes().split(b"\0")[0].decode() for i, c in enumerate(centres) if "%s:%d" % (w["case"]["ctg"], c) in set(keys)]
    meta = json.loads(str(z["meta"]))
    assert meta == dict(seed=9, sampling="plain", p_near=0.08, p_outside=0.08, amp=1.5, v=stats["v"], c=stats["c"], r=stats["r"], n_near=stats["n_near"],
                        n_outside=stats["n_outside"])
    # the off-by-one of the bed look-up: a window at 799 (if any) is in the set, one at 800 -- a truth site, the interval's end -- is not
    assert "chrS:800" not in keys and 800 in centres.tolist()


def test_cli_is_reproducible_and_seeded(host_world, tmp_path):
    w = host_world
    again, other = str(tmp_path / "again.npz"), str(tmp_path / "other.npz")
    _run_cli(w, "--front_end", "host", "--set_fn", again, *w["flags"])
    assert open(again, "rb").read() == open(w["out"]["set"], "rb").read()
    _run_cli(w, "--front_end", "host", "--set_fn", other, *(w["flags"][:3] + ["10"] + w["flags"][4:]))
    assert not np.array_equal(np.load(other)["positions"], np.load(again)["positions"])


def test_train_loads_the_set_as_it_loads_the_text(host_world):
    from clair_amd import train
    w = host_world
    np.random.seed(4)
    Xs, Ys = train.load_dataset(None, None, None, [w["out"]["set"]])
    np.random.seed(4)
    Xt, Yt = train.load_dataset(w["out"]["tensor"], w["paths"]["truth.var"], w["paths"]["regions.bed"])
    assert len(Xs) > 20 and Xs.dtype == Xt.dtype == np.float32 and Xs.tobytes() == Xt.tobytes() and np.array_equal(Ys, Yt)
    np.random.seed(4)
    order = np.random.permutation(len(Xs))                      # undo the shuffle: the rows are the file's, in its order
    X, _keys, Y = mts.load_sets([w["out"]["set"]])
    assert np.array_equal(Xs, X[order]) and np.array_equal(Ys, Y[order])
    # two files: concatenated, the first row of a site wins
    X2, keys2, _ = mts.load_sets([w["out"]["set"], w["out"]["set"]])
    assert len(X2) == len(X) and len(set(keys2)) == len(keys2)
    assert train.build_parser().parse_args([]).set_fn is None
    assert train.build_parser().parse_args(["--set_fn", "a", "--set_fn", "b"]).set_fn == ["a", "b"]


def test_evaluate_reads_the_set_as_it_reads_the_text(host_world):
    from clair_amd import evaluate
    w = host_world
    from_set = list(mts.set_batches([w["out"]["set"]], 16))
    from_text = list(evaluate.labelled_batches(w["out"]["tensor"], w["paths"]["truth.var"], w["paths"]["regions.bed"], 16))
    assert len(from_set) > 1 and len(from_text) > 1 and max(len(b[0]) for b in from_set) == 16
    # (the text reader filters after it has cut a batch, so its batches are the shorter ones: the rows and their order are what is compared)
    joined = [(np.concatenate([np.asarray(b[0], dtype=np.float32) for b in part]), sum((list(b[1]) for b in part), []), np.concatenate([b[2] for b in part]))
              for part in (from_set, from_text)]
    assert joined[0][0].tobytes() == joined[1][0].tobytes() and joined[0][1] == joined[1][1] and np.array_equal(joined[0][2], joined[1][2])
    assert evaluate.build_parser().parse_args([]).set_fn is None
    assert evaluate.build_parser().parse_args(["--set_fn", "a", "--set_fn", "b"]).set_fn == ["a", "b"]


def test_cli_vcf_input_and_left_edge_flag(host_world, tmp_path):
    """--vcf_fn runs GetTruth's code: the same files as --var_fn with the rows GetTruth writes for that VCF; --stop_consider_left_edge reaches the pileup."""
    w = host_world
    vcf, var = str(tmp_path / "truth.vcf"), str(tmp_path / "from_vcf.var")
    seen, lines = set(), ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for row in w["rows"]:
        ctg, pos, ref, alt, g1, g2 = row.split()
        if pos not in seen:
            seen.add(pos)
            lines.append("%s\t%s\t.\t%s\t%s\t50\tPASS\t.\tGT\t%s/%s" % (ctg, pos, ref, alt, g1, g2))
    open(vcf, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([sys.executable, "-m", "clair_amd", "GetTruth", "--vcf_fn", vcf, "--ctgName", "chrS", "--var_fn", var], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    out = {}
    for name, truth_flags in (("vcf", ["--vcf_fn", vcf]), ("var", ["--var_fn", var])):
        out[name] = [str(tmp_path / (name + ".gz")), str(tmp_path / (name + ".npz"))]
        args = [a for a in tc.cli_args(w, "--front_end", "host", "--stop_consider_left_edge", "--tensor_fn", out[name][0], "--set_fn", out[name][1], *w["flags"])]
        k = args.index("--var_fn")
        args[k:k + 2] = truth_flags
        r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set"] + args, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
    for a, b in zip(out["vcf"], out["var"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    # the rows: the expected ones with the pileup's left-edge rule off; they differ from the default's
    w2 = dict(w, rows=[line for line in gzip.open(var, "rt").read().splitlines()])
    centres, seqs, counts, stats = expected_rows(w2, 0.08, 9, 3.0, 1.5, left_edge=False)
    text = fc.text_of("chrS", centres, seqs, counts)
    assert gzip.open(out["vcf"][0], "rt").read() == text and text != gzip.open(w["out"]["tensor"], "rt").read() and stats["kept_non"] > 10


def test_cli_native_bam_reader_equals_samtools_on_the_text(tmp_path):
    """--bam_reader native on a BAM (tests/bam_fixture.py) = the default reader on the text samtools prints for it, with a ctg range: both files"""
    import bam_fixture as bf
    import pileup_synth
    case = pileup_synth.synth_case(seed=301, n_reads=500, ref_len=3000)
    fa = str(tmp_path / "ref.fa")
    text, fai = bf.fasta_of({case["ctg"]: "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:]), "chrOther": "ACGT" * 30})
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    bam = bf.Bam(case["sam"], [(case["ctg"], 3000), ("chrOther", 120)])
    bam_fn, canon, var = str(tmp_path / "reads.bam"), str(tmp_path / "canon.sam"), str(tmp_path / "truth.var")
    bam.write(bam_fn, block=3000, index=True)
    open(canon, "w").write(bam.canonical())
    open(var, "w").write("".join("chrS %d A C 0 1\n" % p for p in (100, 420, 435, 900, 1500, 2380, 2600)))
    out = {}
    for name, reader in (("native", ["--bam_fn", bam_fn, "--bam_reader", "native"]), ("text", ["--bam_fn", canon])):
        out[name] = [str(tmp_path / (name + ".gz")), str(tmp_path / (name + ".npz"))]
        r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set", "--ref_fn", fa, "--ctgName", "chrS", "--var_fn", var, "--samtools", tc.FAKE_SAMTOOLS,
                            "--front_end", "host", "--ctgStart", "400", "--ctgEnd", "2400", "--outputProb", "0.05", "--amp", "6", "--tensor_fn", out[name][0], "--set_fn",
                            out[name][1]] + reader, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
    for a, b in zip(out["native"], out["text"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    positions = np.load(out["native"][1])["positions"]
    assert len(positions) > 20 and positions.min() >= 400 and positions.max() <= 2400 and {420, 435, 900, 1500, 2380} <= set(positions.tolist())


def test_cli_argument_checks(host_world):
    w = host_world
    for more, word in (([], "nothing to write"), (["--set_fn", "x.npz", "--vcf_fn", "t.vcf"], "one of the two")):
        r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set"] + tc.cli_args(w, *more), capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and word in r.stderr


# -- 6. the dispatcher --------------------------------------------------------------------------------------------------------------------
def test_dispatcher_lists_the_new_submodules():
    r = subprocess.run([sys.executable, "-m", "clair_amd"], capture_output=True, text=True, cwd=ROOT)
    assert "PairWithNonVariants" in r.stdout and "make_train_set" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "make_train_set"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--set_fn" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "PairWithNonVariants"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--tensor_can_fn" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "train"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "outside this build" in r.stderr
    r = subprocess.run([sys.executable, "-m", "clair_amd.extract_variant_candidates", "--gen4Training"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "training" in r.stderr and "make_train_set" in r.stderr
