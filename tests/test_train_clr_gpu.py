"""train_clr and learning_rate_finder on the MI355X: the accuracy counts of clair_train_accuracy against the NumPy twin
(clair_amd.model.accuracy_counts) on the probabilities the same accumulate left, Clair.lr_train against Clair.train, and both commands
end to end.  Counts are integers: every comparison is for equality."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from clair_amd import _capi, param, synth, weights
from clair_amd.model import Clair, accuracy_counts, accuracy_from_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
HEADS = ((0, 21), (21, 24), (24, 57), (57, 90))
DROPOUT = (0.5, 0.5, 0.2, 0.2, 0.2, 0.2)
NO_DROPOUT = (0.0,) * 6
MICRO = 320


def _batch(n, seed=7):
    x, _ = synth.synthetic_input(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return x, np.stack([rng.integers(0, s, n) for s in (21, 3, 33, 33)], axis=1).astype(np.uint8)


def _crafted_labels(p):
    """Labels made from the probabilities themselves, four kinds of row in turn: everything right; everything right through a swapped indel
    pair; everything wrong; gt21 and the smaller indel right, genotype and the larger wrong.  So each head is hit on at least n // 4 rows
    and missed on at least n // 4."""
    top = np.stack([np.argmax(p[:, a:b], axis=1) for a, b in HEADS], axis=1)
    lab = top.copy()
    for i in range(len(p)):
        small, large = sorted(top[i, 2:])
        kind = i % 4
        if kind == 1:
            lab[i, 2], lab[i, 3] = top[i, 3], top[i, 2]
        elif kind == 2:
            other = next(v for v in range(3) if v != small and v != large)
            lab[i] = ((top[i, 0] + 1) % 21, (top[i, 1] + 1) % 3, other, other)
        elif kind == 3:
            lab[i, 1] = (top[i, 1] + 1) % 3
            lab[i, 2:] = (large + 1, small) if large < 32 else (small, small) if small < large else (31, 32)      # given swapped where it can be
    return lab.astype(np.uint8)


@pytest.fixture(scope="module")
def trainer():
    t = _capi.Trainer(0, MICRO)
    t.set_tensors(weights.synthetic_weights(lstm_gain=2, forget_bias=1, input_gain=0.05, head_gain=3))
    yield t
    t.close()


def _counts_after_crafting(t, n, training):
    x, lab = _batch(n, seed=7 + n)
    t.accumulate(x, lab, training=training)
    p = t.probabilities()
    random_tp = t.accuracy()
    assert np.array_equal(random_tp, accuracy_counts(p, lab))
    crafted = _crafted_labels(p)
    if training:
        t.zero_grad()
    t.accumulate(x, crafted, training=training)
    again = t.probabilities()
    assert np.array_equal(again.view(np.uint32), p.view(np.uint32))              # the forward pass does not depend on the labels
    tp, want = t.accuracy(), accuracy_counts(again, crafted)
    print("n=%d training=%d: tp %s (random labels: %s)" % (n, training, tp, random_tp))
    assert tp.dtype == np.int64 and np.array_equal(tp, want)
    assert (want >= n // 4).all() and (want <= n - n // 4).all()
    assert np.array_equal(t.accuracy(), want)                                    # asking again changes nothing
    return tp


@pytest.mark.parametrize("n", [1, 5, 64, 65, 257, 300])
def test_counts_equal_the_twin_validation_mode(trainer, n):
    """one wavefront and one row past it, one workgroup of 256 and one row past it, a partial last workgroup"""
    trainer.config(dropout_rates=NO_DROPOUT, seed=3)
    _counts_after_crafting(trainer, n, False)


def test_counts_equal_the_twin_training_mode_dropout_on(trainer):
    """the masks are a hash of (seed, optimizer step, row): the same accumulate twice draws the same ones"""
    trainer.config(dropout_rates=DROPOUT, seed=5)
    trainer.zero_grad()
    _counts_after_crafting(trainer, 11, True)
    trainer.config(dropout_rates=NO_DROPOUT, seed=3)


def test_ties_on_the_device_take_the_lowest_index():
    n = 70
    x, _ = _batch(n)
    zeros = {k: np.zeros(shape, dtype=np.float32) for k, shape in weights.TENSOR_TABLE.items()}
    t = _capi.Trainer(0, 128)
    try:
        t.set_tensors(zeros)
        t.config(dropout_rates=NO_DROPOUT)
        for value, want in ((0, [n] * 4), (1, [0] * 4)):
            t.accumulate(x, np.full((n, 4), value, dtype=np.uint8), training=False)
            p = t.probabilities()
            assert all((p[:, a:b] == p[:, a:a + 1]).all() for a, b in HEADS)         # uniform heads, bit-equal values
            assert list(t.accuracy()) == want
    finally:
        t.close()


def test_accuracy_before_any_accumulate_fails_with_a_message():
    t = _capi.Trainer(0, 8)
    try:
        with pytest.raises(_capi.EngineError) as ei:
            t.accuracy()
        assert "no accumulate" in str(ei.value)
    finally:
        t.close()


def test_lr_train_is_train_plus_prediction_and_accuracy():
    x, _ = _batch(11)
    models = [Clair(max_batch=16, n_slots=1, micro_batch=8, seed=1) for _ in range(3)]
    try:
        probe, m, twin = models
        for model in models:
            model.init()
        lab = _crafted_labels(np.concatenate(probe.lr_train(x, _batch(11)[1])[0], axis=1))      # the same seed and step: the same masks
        got = m.lr_train(x, lab)
        twin.train(x, lab)
        assert got[0] is m.prediction and got[1] == m.training_loss_on_one_batch == twin.training_loss_on_one_batch and got[2] is None
        assert [p.shape for p in m.prediction] == [(11, 21), (11, 3), (11, 33), (11, 33)] and all(p.dtype == np.float32 for p in m.prediction)
        w, w2 = m.get_parameters(), twin.get_parameters()
        assert all(np.array_equal(w[k].view(np.uint32), w2[k].view(np.uint32)) for k in w)
        want = accuracy_counts(np.concatenate(m.prediction, axis=1), lab)
        print("lr_train: tp %s of 11" % m.training_tp)
        assert m.training_tp.dtype == np.int64 and np.array_equal(m.training_tp, want) and (want >= 2).all() and (want <= 9).all()
        assert m.training_accuracy == accuracy_from_counts(want, 11)
    finally:
        for model in models:
            model.close()


# ---- the two commands end to end -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_clr")
    raw, infos = synth.synthetic_candidates(60, "ont", seed=11)
    tensors, var_fn = str(d / "tensors.txt"), str(d / "truth.var")
    open(tensors, "w").write("\n".join(synth.tensor_records(raw, infos)) + "\n")
    with open(var_fn, "w") as f:
        for i, (ctg, pos, seq) in enumerate(infos[:10]):
            ref = seq[16]
            alt = "ACGT"[("ACGT".index(ref) + 1 + i % 3) % 4]
            f.write("%s %s %s %s %d %d\n" % (ctg, pos, ref, alt, i % 2, 1))
    return d, ["--tensor_fn", tensors, "--var_fn", var_fn, "--batch_size", "8", "--micro_batch", "8", "--seed", "1"]


NUMBER = r"-?\d+\.\d+(e-?\d+)?"
REPORT = "[INFO] Evaluation on gt21:\n[INFO] all/top1/top2/top1p/top2p: 60/"


def _run(module, arguments):
    return subprocess.run([sys.executable, "-m", module] + arguments, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_train_clr_command_end_to_end(data_set):
    d, common = data_set
    prefix = str(d / "clr")
    r = _run("clair_amd.train_clr", common + ["--max_epochs", "2", "--clr_mode", "tri2", "--ochk_prefix", prefix])
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.isfile(prefix + "-000001.index") and os.path.isfile(prefix + "-000002.index") and not os.path.exists(prefix + "-000003.index")
    for epoch in (1, 2):
        assert re.search(r"^%d Training loss: %s$" % (epoch, NUMBER), r.stderr, flags=re.M), r.stderr
        assert re.search(r"^%d Validation loss \(Total/Base/Genotype/Indel_1_2\):(\t%s){5}$" % (epoch, NUMBER), r.stderr, flags=re.M), r.stderr
    assert "[INFO] Learning rate: 1.00e-04" in r.stderr and "[INFO] The size of dataset: 60" in r.stderr and "[INFO] Best validation loss at epoch:" in r.stderr
    assert r.stdout.startswith(REPORT) and "[INFO] evaluation on indel length 2:" in r.stdout


def test_learning_rate_finder_command_end_to_end(data_set):
    d, common = data_set
    texts = []
    for k in range(2):
        olr_fn = str(d / ("rates%d.txt" % k))
        r = _run("clair_amd.learning_rate_finder", common + ["--ochk_prefix", str(d / ("finder%d" % k)), "--olr_fn", olr_fn])
        assert r.returncode == 0, r.stderr[-3000:]
        texts.append(open(olr_fn).read())
    assert texts[0] == texts[1]                                                  # the same seed: the same bytes
    lines = texts[0].splitlines()
    assert lines[0] == "lr,accuracy,loss,diff" and len(lines) == 1 + 6           # 54 training rows: seven batches, the first row dropped
    rows = [[float(v) for v in line.split(",")] for line in lines[1:]]

    class Bare(object):
        clr = Clair.clr
    bare, global_step, max_lr, rates = Bare(), 0, param.max_lr, []
    for _ in range(7):
        rate, global_step, max_lr = bare.clr(global_step, np.ceil(54 / 8 + 1), max_lr, "tri")
        rates.append(float(rate))
    assert [row[0] for row in rows] == rates[1:]
    for row, n_batch in zip(rows, [8] * 5 + [6]):                                # counts over 4 heads and n_batch rows
        assert 0.0 <= row[1] <= 1.0 and abs(row[1] * 4 * n_batch - round(row[1] * 4 * n_batch)) <= 1e-12, row    # a few float64 roundings of k / 6
        assert row[2] > 0
    found = re.search(r"^\[INFO\] min_lr: (\S+), max_lr: (\S+)$", r.stderr, flags=re.M)
    assert found and float(found.group(1)) <= float(found.group(2)) and "[INFO] Learning rate: 1.00e-06" in r.stderr
    assert os.path.isfile(str(d / "finder1") + "-000001.index") and r.stdout.startswith(REPORT)
