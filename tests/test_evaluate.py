"""evaluate / GetTruth without a GPU: label encoders, truth rows, the NumPy twin of the scoring kernel, the data-set builder and the
report, against goldens minted from the reference (tools/make_evaluate_goldens.py, tools/make_get_truth_golden.py)."""
import json
import os
import re
import stat
import subprocess
import sys

import numpy as np
import pytest

from clair_amd import _capi, evaluate, get_truth, task

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SMALL = os.path.join(GOLD, "evaluate_small")


@pytest.fixture(scope="module")
def small():
    z = np.load(SMALL + ".npz")
    out = {k: z[k] for k in ("keys", "labels", "probs", "counts")}
    out.update(json.load(open(SMALL + ".json")))
    return out


def crafted_rows():
    """Probabilities with exact ties where the rules differ, and every class as true label.  -> (P float32 [n,90], labels uint8 [n,4])"""
    rows, labels = [], []

    def add(gt21, genotype, len1, len2, lab):
        rows.append(np.concatenate([np.asarray(v, dtype=np.float32) for v in (gt21, genotype, len1, len2)]))
        labels.append(lab)

    flat21, flat3, flat33 = np.full(21, 1 / 21.0), np.full(3, 1 / 3.0), np.full(33, 1 / 33.0)
    for t in range(21):                       # all equal: arg-max 0; order = descending index, so 20 is first and 19 second
        add(flat21, flat3, flat33, flat33, (t, t % 3, t, 32 - t))
    for t in range(33):                       # every length class as true label, both orders of the pair
        add(flat21, flat3, flat33, flat33, (t % 21, 0, t, (t * 7) % 33))
    g = np.full(21, 0.01)
    g[[4, 9]] = 0.4                           # tie in first place between 4 and 9: 9 is first, 4 second, arg-max 4
    for t in (4, 9, 0):
        add(g, [0.5, 0.5, 0.0], flat33, flat33, (t, 1, 16, 16))
    g = np.full(21, 0.005)
    g[2] = 0.5
    g[[7, 12]] = 0.2                          # tie in second place: 12 is second, 7 third
    for t in (2, 7, 12):
        add(g, [0.2, 0.4, 0.4], flat33, flat33, (t, 2, 16, 16))
    g = np.full(21, 0.001)
    g[1], g[3] = 0.5, 0.3
    g[[5, 6]] = 0.05                          # tie in third place: neither is in the top two
    for t in (5, 6, 3):
        add(g, [0.1, 0.2, 0.7], flat33, flat33, (t, 0, 16, 16))
    a, b = np.full(33, 0.001), np.full(33, 0.001)
    a[20], b[20] = 0.9, 0.9                   # equal arg-maxes in the two length heads
    add(flat21, flat3, a, b, (0, 0, 20, 20))
    a, b = np.full(33, 0.001), np.full(33, 0.001)
    a[25], b[3] = 0.9, 0.9                    # predicted pair out of order, true pair out of order
    add(flat21, flat3, a, b, (0, 0, 30, 2))
    a = np.full(33, 0.001)
    a[[8, 30]] = 0.4                          # tie inside a length head: the lowest index
    add(flat21, flat3, a, b, (0, 0, 8, 3))
    return np.stack(rows).astype(np.float32), np.array(labels, dtype=np.uint8)


def test_label_encoders_match_the_reference():
    g = json.load(open(os.path.join(GOLD, "evaluate_labels.json")))
    assert len(g["rows"]) >= 30
    seen = set()
    for row, vec in g["rows"]:
        idx = task.labels_from_vcf_columns(row.split())
        assert task.one_hot_labels(idx) == vec, row
        seen.add(idx[0])
    assert len(seen) >= 12                                     # SNP hom/het, base+Ins, base+Del, InsIns, DelDel, InsDel ...
    for base, vec in g["reference"]:
        assert task.one_hot_labels(task.labels_from_reference(base)) == vec
    assert task.labels_from_vcf_columns(["c", "1", "A", "A" + "C" * 40, "1", "1"])[2:] == (32, 32)       # clamp at +16
    assert task.labels_from_vcf_columns(["c", "1", "A" + "C" * 40, "A", "0", "1"])[2:] == (0, 16)        # clamp at -16, reference allele 0


def _fake_samtools(tmp_path):
    sam = tmp_path / "samtools"
    sam.write_text("#!/bin/sh\nexec %s %s/tests/fake_samtools.py \"$@\"\n" % (sys.executable, ROOT))
    sam.chmod(sam.stat().st_mode | stat.S_IEXEC)
    env = dict(os.environ)
    env["PATH"] = str(tmp_path) + os.pathsep + env["PATH"]
    return env


def test_get_truth_stdout_byte_for_byte(tmp_path):
    g = json.load(open(os.path.join(GOLD, "get_truth.json")))
    (tmp_path / "t.vcf").write_text(g["vcf"])
    (tmp_path / "ref.fa").write_text(g["fasta"])
    env = _fake_samtools(tmp_path)
    assert len(g["cases"]) == 2
    for name, case in g["cases"].items():
        r = subprocess.run([sys.executable, "-m", "clair_amd", "GetTruth", "--vcf_fn", str(tmp_path / "t.vcf"), "--ref_fn", str(tmp_path / "ref.fa"),
                            "--ctgName", "chrS"] + case["extra"], capture_output=True, text=True, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout == case["stdout"], name
    # to a file: gzip of the same rows
    out = tmp_path / "truth.var"
    r = subprocess.run([sys.executable, "-m", "clair_amd", "GetTruth", "--vcf_fn", str(tmp_path / "t.vcf"), "--ref_fn", str(tmp_path / "ref.fa"),
                        "--ctgName", "chrS", "--var_fn", str(out)], capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 0 and r.stdout == ""
    import gzip
    assert gzip.open(str(out), "rt").read() == g["cases"]["all"]["stdout"]


def test_vcf_positions_of_callVarBam_are_the_truth_rows_positions(tmp_path, monkeypatch):
    """callVarBam --vcf_fn walks the same records: its positions are column 2 of GetTruth's rows."""
    from clair_amd import callVarBam
    g = json.load(open(os.path.join(GOLD, "get_truth.json")))
    (tmp_path / "t.vcf").write_text(g["vcf"])
    for case in g["cases"].values():
        extra = dict(zip(case["extra"][0::2], case["extra"][1::2]))
        lo, hi = (int(extra["--ctgStart"]), int(extra["--ctgEnd"])) if extra else (None, None)
        got = callVarBam.positions_from_vcf(str(tmp_path / "t.vcf"), "chrS", lo, hi)
        assert got.tolist() == [int(r.split()[1]) for r in case["stdout"].split("\n") if r]


def test_get_truth_parser_flags_and_defaults():
    a = get_truth.build_parser().parse_args([])
    assert (a.vcf_fn, a.var_fn, a.ref_fn, a.ctgName, a.ctgStart, a.ctgEnd) == ("input.vcf", "PIPE", None, "chr17", None, None)


def test_evaluate_parser_flags_and_defaults():
    a = evaluate.build_parser().parse_args([])
    assert (a.bin_fn, a.train_bin_fn, a.validation_bin_fn, a.tensor_fn, a.var_fn, a.bed_fn, a.chkpnt_fn) == (None, None, None, "vartensors", "truthvars", None, None)
    assert (a.batch_size, a.device, a.score_on) == (None, 0, "device")
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(["--score_on", "nowhere"])


def test_fixture_gaps_hold_on_the_oracle(small):
    """What makes the GPU report comparable exactly: first-second and second-third gaps >= 1e-4 in every head (five times what two
    probabilities within the 1e-5 contract can move a gap by)."""
    P = small["probs"]
    assert P.dtype == np.float32 and P.shape == (small["candidates"], 90) and small["candidates"] >= 200
    for a, b in ((0, 21), (21, 24), (24, 57), (57, 90)):
        s = -np.sort(-P[:, a:b], axis=1)
        assert (s[:, 0] - s[:, 1]).min() >= 1e-4 and (s[:, 1] - s[:, 2]).min() >= 1e-4
    assert small["dropped_for_gap"] <= 0.10 * (small["dropped_for_gap"] + small["candidates"])


def test_host_counts_equal_the_reference_loop(small):
    counts = evaluate.evaluate_counts_host(small["probs"], small["labels"])
    assert counts.dtype == np.int64 and counts.shape == (2631,) == (_capi.EVAL_COUNTS,)
    assert np.array_equal(counts, small["counts"])
    c = evaluate.split_counts(counts)
    assert c["all"] == small["candidates"] == c["gt21"].sum() == c["genotype"].sum() == c["len1"].sum() == c["len2"].sum()
    assert (c["gt21"] > 0).sum() - (np.diag(c["gt21"]) > 0).sum() >= 10          # not one diagonal cell
    # in pieces, in any order: counts add up
    order = np.random.default_rng(1).permutation(len(small["labels"]))
    parts = sum(evaluate.evaluate_counts_host(small["probs"][i], small["labels"][i]) for i in np.array_split(order, 7))
    assert np.array_equal(parts, counts)
    # the list form call_var's predictions come in
    P = small["probs"]
    assert np.array_equal(evaluate.evaluate_counts_host([P[:, :21], P[:, 21:24], P[:, 24:57], P[:, 57:]], small["labels"]), counts)


def test_tie_rule_on_crafted_rows():
    """arg-max: lowest index among equals.  top-1 / top-2: descending probability, then descending index."""
    P, lab = crafted_rows()
    flat = np.full((1, 90), 0.25, dtype=np.float32)
    for t, top1, top2 in ((20, 1, 1), (19, 0, 1), (18, 0, 0), (0, 0, 0)):
        c = evaluate.split_counts(evaluate.evaluate_counts_host(flat, np.array([[t, 0, 5, 9]], dtype=np.uint8)))
        assert (c["all"], c["top1"], c["top2"]) == (1, top1, top2)
        assert c["gt21"][t, 0] == 1 and c["genotype"][0, 0] == 1 and c["len1"][5, 0] == 1 and c["len2"][9, 0] == 1
    g = np.full(21, 0.01, dtype=np.float32)
    g[[4, 9]] = 0.4
    row = np.concatenate([g, [0.5, 0.5, 0.0], np.full(66, 0.1)]).astype(np.float32)[None, :]
    for t, top1, top2 in ((9, 1, 1), (4, 0, 1), (0, 0, 0)):
        c = evaluate.split_counts(evaluate.evaluate_counts_host(row, np.array([[t, 1, 16, 16]], dtype=np.uint8)))
        assert (c["top1"], c["top2"]) == (top1, top2) and c["gt21"][t, 4] == 1 and c["genotype"][1, 0] == 1
    # the pairs of the two length heads are sorted: true (30, 2) -> (2, 30), predicted (25, 3) -> (3, 25)
    a, b = np.full(33, 0.001), np.full(33, 0.001)
    a[25], b[3] = 0.9, 0.9
    row = np.concatenate([np.full(24, 0.1), a, b]).astype(np.float32)[None, :]
    c = evaluate.split_counts(evaluate.evaluate_counts_host(row, np.array([[0, 0, 30, 2]], dtype=np.uint8)))
    assert c["len1"][2, 3] == 1 and c["len2"][30, 25] == 1 and c["len1"].sum() == c["len2"].sum() == 1
    # where nothing ties the rule is the reference's argsort()[::-1]
    rng = np.random.default_rng(3)
    R = rng.random((500, 90)).astype(np.float32)
    L = np.stack([rng.integers(0, k, 500) for k in (21, 3, 33, 33)], axis=1).astype(np.uint8)
    order = np.argsort(R[:, :21], axis=1)[:, ::-1]
    c = evaluate.split_counts(evaluate.evaluate_counts_host(R, L))
    assert c["top1"] == (order[:, 0] == L[:, 0]).sum() and c["top2"] == ((order[:, 0] == L[:, 0]) | (order[:, 1] == L[:, 0])).sum()
    # the crafted set as a whole: every class is a true label somewhere
    c = evaluate.split_counts(evaluate.evaluate_counts_host(P, lab))
    assert (c["gt21"].sum(axis=1) > 0).all() and (c["genotype"].sum(axis=1) > 0).all() and c["all"] == len(P)
    with pytest.raises(ValueError):
        evaluate.evaluate_counts_host(P[:1], np.array([[21, 0, 0, 0]], dtype=np.uint8))


def test_data_set_builder_matches_the_reference(small):
    """Bed filter with the reference's off-by-one, first tensor of a position wins, non-ACGTU centres dropped, sites without a truth
    row get the reference label: keys and labels are get_training_array's (sorted as it sorts them)."""
    keys, labels, X = [], [], []
    for x, k, lab in evaluate.labelled_batches(SMALL + ".txt.gz", SMALL + ".var", SMALL + ".bed", 64):
        assert x.dtype == np.float32 and x.shape[1:] == (33, 8, 4) and len(x) == len(k) == len(lab) <= 64 and lab.dtype == np.uint8
        keys += k
        labels.append(lab)
        X.append(x)
    labels = np.concatenate(labels)
    assert len(keys) == len(set(keys)) == small["candidates"] < small["tensor_lines"] - 6
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    assert [keys[i] for i in order] == small["keys"].tolist()
    assert np.array_equal(labels[order], small["labels"])
    assert (labels[:, 1] == 0).sum() > 50 and (labels[:, 1] != 0).sum() > 50
    # without a bed nothing is filtered; without truth rows every label is the reference label
    n_all = sum(len(k) for _, k, _ in evaluate.labelled_batches(SMALL + ".txt.gz", SMALL + ".var", None, 1000))
    assert n_all > small["candidates"]
    for _, _, lab in evaluate.labelled_batches(SMALL + ".txt.gz", None, None, 1000):
        assert (lab[:, 1:] == (0, 16, 16)).all() and set(lab[:, 0].tolist()) <= {0, 4, 7, 9}


def _numbers(text):
    return [float(v) for v in re.findall(r"[-+]?\d*\.?\d+(?:[eE][-+]?\d+)?", text)]


def assert_same_report(got, want):
    """Matrix and count lines byte for byte; the values of the f-measure arrays to 1e-8 (their layout is NumPy's print options)."""
    def split(text):
        plain, arrays = [], []
        for chunk in re.split(r"(\[INFO\] f-measure:  \[[^\]]*\])", text):
            (arrays if chunk.startswith("[INFO] f-measure:") else plain).append(chunk)
        return plain, arrays
    gp, ga = split(got)
    wp, wa = split(want)
    assert gp == wp
    assert len(ga) == len(wa) == 4
    for a, b in zip(ga, wa):
        x, y = _numbers(a.split(":", 1)[1]), _numbers(b.split(":", 1)[1])
        assert len(x) == len(y) and np.allclose(x, y, rtol=0, atol=1e-8)


def test_report_is_the_reference_stdout(small):
    text = "\n".join(evaluate.report_lines(small["counts"])) + "\n"
    assert_same_report(text, small["stdout"])
    assert text == small["stdout"]            # under the NumPy that minted it even the array layout agrees
    f = evaluate.f1_score(np.array([[2, 1], [0, 0]]))
    assert f.dtype == np.float64 and abs(f[0] - 0.8) < 1e-12 and f[1] == 0.0


def test_dispatcher_runs_the_new_submodules():
    for name, flag in (("evaluate", "--chkpnt_fn"), ("GetTruth", "--vcf_fn")):
        r = subprocess.run([sys.executable, "-m", "clair_amd", name], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 1 and flag in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd"], capture_output=True, text=True, cwd=ROOT)
    assert "evaluate" in r.stdout and "GetTruth" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "train"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "outside this build" in r.stderr


@pytest.mark.parametrize("flag", ["--bin_fn", "--train_bin_fn", "--validation_bin_fn"])
def test_blosc_binaries_exit_with_the_message(flag):
    r = subprocess.run([sys.executable, "-m", "clair_amd", "evaluate", flag, "some.bin", "--chkpnt_fn", "model"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "blosc" in r.stderr and len(r.stderr.strip().split("\n")) == 1


def test_symbols_load_on_a_gpu_less_host():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "clair_amd.h")).read()
    for name in ("clair_eval_reset", "clair_submit_eval", "clair_eval", "clair_eval_read"):
        assert hasattr(lib, name) and name in _capi.SYMBOLS and re.search(r"\bint %s\(" % name, header)
    assert re.search(r"#define CLAIR_EVAL_COUNTS \(3 \+ 21 \* 21 \+ 3 \* 3 \+ 33 \* 33 \+ 33 \* 33\)", header)
    assert "#define CLAIR_ABI_VERSION 6" in header and lib.clair_abi_version() == 6
    assert lib.clair_eval_reset(None) != 0 and b"NULL" in lib.clair_last_error(None)
