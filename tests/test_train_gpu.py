"""train on the MI355X: the device gradients, losses, masks, optimizer steps and trajectories against the autograd oracle
(tools/torch_train_ref.py), Clair's training members, and `python -m clair_amd.train` end to end.

The yardstick of every comparison with the float64 oracle is the float32 oracle's own error against it, measured in the same test on
the same inputs (docs/train.md records the worst ratios seen):
    gradients / weights   || dev - f64 || <= 8 * max(max_k || f32_k - f64_k || / || f64_k ||, eps32) * || f64 ||     per tensor
    losses, stats         |  dev - f64 |  <= 16 * max(| f32 - f64 |, eps32 * | f64 |)
    probabilities         max | dev - f64 | <= 16 * max(max | f32 - f64 |, eps32)                                 per micro-batch

That yardstick means something only while no SELU input of the batch lies so close to zero that the two oracles (or the device) put it
on different sides: the derivative jumps there.  Every gradient case therefore runs on weights prepared for its batch and masks by
R.clear_of_the_selu_kink and asserts that they are clear of the kink before it compares anything (docs/train.md).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from clair_amd import _capi, synth, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_num_threads(4)
EPS32 = float(np.finfo(np.float32).eps)
TRAINED_LIKE = dict(lstm_gain=2, forget_bias=1, input_gain=0.05, head_gain=3)
NO_DROPOUT = (0.0,) * 6
_WEIGHTS = {}
_PREPARED = {}


def _weights(recipe):
    if recipe not in _WEIGHTS:
        _WEIGHTS[recipe] = weights.synthetic_weights(**(TRAINED_LIKE if recipe == "trained" else {}))
    return _WEIGHTS[recipe]


def _batch(n, seed=7):
    x, _ = synth.synthetic_input(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return x, np.stack([rng.integers(0, s, n) for s in (21, 3, 33, 33)], axis=1).astype(np.uint8)


def _accumulate(t, x, lab, micro, training=True, masks=False):
    """the batch through the trainer in micro-batches -> (losses [4], masks of the whole batch or None)"""
    losses, got = np.zeros(4), {k: [] for k in range(6)}
    for first in range(0, len(x), micro):
        losses += t.accumulate(x[first:first + micro], lab[first:first + micro], first_row=first, training=training)
        if masks:
            for k in range(6):
                got[k].append(t.read_mask(k))
    return losses, ({k: np.concatenate(v, axis=1 if k == 0 else 0) for k, v in got.items()} if masks else None)


def _yardstick(f32, f64):
    return max(max(np.linalg.norm(f32[k].astype(np.float64) - f64[k]) / np.linalg.norm(f64[k]) for k in f64), EPS32)


def _assert_tensors(dev, f32, f64, what):
    yard = _yardstick(f32, f64)
    worst = 0.0
    for k in f64:
        err = np.linalg.norm(dev[k].astype(np.float64) - f64[k]) / np.linalg.norm(f64[k])
        worst = max(worst, err / yard)
    print("%s: float32-oracle yardstick %.3g, worst device error / yardstick %.3g" % (what, yard, worst))
    for k in f64:
        assert np.linalg.norm(dev[k].astype(np.float64) - f64[k]) <= 8 * yard * np.linalg.norm(f64[k]), (what, k)


def _assert_scalars(dev, f32, f64, what):
    dev, f32, f64 = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (dev, f32, f64))
    bound = 16 * np.maximum(np.abs(f32 - f64), EPS32 * np.abs(f64))
    print("%s: device %s float64 %s, worst error / bound %.3g" % (what, dev, f64, float(np.max(np.abs(dev - f64) / bound))))
    assert (np.abs(dev - f64) <= bound).all(), (what, dev, f32, f64)


def _assert_probabilities(dev, p32, p64, what):
    """dev: the rows of the last micro-batch"""
    p32, p64 = p32[-len(dev):].astype(np.float64), p64[-len(dev):]
    bound = 16 * max(float(np.abs(p32 - p64).max()), EPS32)
    worst = float(np.abs(dev.astype(np.float64) - p64).max())
    print("%s: %d rows, worst error / bound %.3g" % (what, len(dev), worst / bound))
    assert dev.shape == p64.shape and worst <= bound, (what, worst, bound)


def _assert_clear_of_the_kink(w, x, masks, rates, report, r32, r64, what):
    """the three conditions under which the float32 oracle is a yardstick at all (docs/train.md): conditions, not measurements"""
    z64, z32 = (R.pre_activations(w, x, masks, rates, dtype=d) for d in (torch.float64, torch.float32))
    print("%s: margin %.3g, %d rounds, %d biases moved, smallest |z| %.3g" % (what, report["margin"], report["rounds"], report["moved"], report["smallest"]))
    assert R.sign_disagreements(z32, z64) == 0, what
    assert R.smallest_pre_activation(z64) >= report["margin"], what
    assert _yardstick(r32["gradients"], r64["gradients"]) <= 1e-5, what


def _check_gradients(n, loss, recipe, rates, micro=8):
    """The weights are first moved clear of the SELU kink for this batch and these masks (R.clear_of_the_selu_kink).  The masks depend on
    (seed, step, row) and not on the weights, so with dropout on one accumulate reads them back before the weights are prepared."""
    w = _weights(recipe)
    x, lab = _batch(n)
    dropout = any(rates)
    t = _capi.Trainer(0, micro, "Adam", loss)
    try:
        t.config(dropout_rates=rates, seed=5)
        masks = None
        if dropout:
            t.set_tensors(w)
            t.zero_grad()
            _, masks = _accumulate(t, x, lab, micro, masks=True)
        key = (recipe, n) if not dropout else None                     # without masks the preparation is the same for both losses
        if key not in _PREPARED:
            _PREPARED[key] = R.clear_of_the_selu_kink(w, x, masks, rates)
        prepared, report = _PREPARED[key] if key else _PREPARED.pop(key)
        t.set_tensors(prepared)
        t.zero_grad()
        losses, again = _accumulate(t, x, lab, micro, masks=dropout)
        assert not dropout or all(np.array_equal(again[k], masks[k]) for k in range(6))
        grads = t.get_tensors("gradients")
        probs = t.probabilities()
    finally:
        t.close()
    r64, r32 = (R.loss_and_gradients(prepared, x, lab, loss, masks=masks, rates=rates, dtype=d) for d in (torch.float64, torch.float32))
    what = "%s %s n=%d/%d dropout %s" % (recipe, loss, n, micro, "on" if dropout else "off")
    _assert_clear_of_the_kink(prepared, x, masks, rates, report, r32, r64, what)
    _assert_scalars(losses, r32["parts"], r64["parts"], what + " losses")
    _assert_probabilities(probs, r32["probabilities"], r64["probabilities"], what + " probabilities")
    _assert_tensors(grads, r32["gradients"], r64["gradients"], what + " gradients")


@pytest.mark.parametrize("recipe", ["fresh", "trained"])
@pytest.mark.parametrize("loss", ["FocalLoss", "CrossEntropy"])
@pytest.mark.parametrize("n", [1, 5, 11])
def test_gradients_dropout_off(n, loss, recipe):
    """n = 11 spans two micro-batches of 8, the second ragged"""
    _check_gradients(n, loss, recipe, NO_DROPOUT)


@pytest.mark.parametrize("recipe", ["fresh", "trained"])
@pytest.mark.parametrize("loss", ["FocalLoss", "CrossEntropy"])
def test_gradients_dropout_on(loss, recipe):
    """the masks the device drew are read back and handed to the oracle"""
    _check_gradients(11, loss, recipe, R.DEFAULT_RATES)


@pytest.mark.parametrize("recipe", ["fresh", "trained"])
@pytest.mark.parametrize("loss", ["FocalLoss", "CrossEntropy"])
@pytest.mark.parametrize("n", [65, 130])
def test_gradients_past_one_row_block(n, loss, recipe):
    """one micro-batch of more than 64 rows: the recurrent products (M = n) take a second and third 64-row block of C with accumulate set,
    n = 65 leaves a last block of one row and K = 4 * 16 + 1 in the tail's weight gradients, n = 130 is a third lap of the loss reduction"""
    _check_gradients(n, loss, recipe, NO_DROPOUT, micro=130)


@pytest.mark.parametrize("recipe,loss,rates", [("fresh", "FocalLoss", R.DEFAULT_RATES), ("trained", "CrossEntropy", NO_DROPOUT)], ids=["fresh_focal_dropout", "trained_ce"])
def test_gradients_cut_at_a_full_row_block(recipe, loss, rates):
    """150 rows as 64 + 64 + 22 with first_row 0, 64, 128: exactly one full tile per piece, weight gradients added up over three pieces"""
    _check_gradients(150, loss, recipe, rates, micro=64)


def test_validation_forward_of_300_rows():
    """validation mode on 300 rows in one piece: the four loss sums (five laps of loss_reduce_kernel, the last ragged) and the probabilities
    against the oracle.  No preparation: the forward pass is continuous at the kink."""
    w = _weights("trained")
    x, lab = _batch(300)
    t = _capi.Trainer(0, 320, "Adam", "FocalLoss")
    try:
        t.set_tensors(w)
        losses = t.accumulate(x, lab, training=False)
        probs = t.probabilities()
    finally:
        t.close()
    with torch.no_grad():
        got = {}
        for d in (torch.float64, torch.float32):
            logits = R.network({k: torch.tensor(v, dtype=d) for k, v in w.items()}, torch.tensor(x, dtype=d))
            parts, p = R.head_losses(logits, lab)
            got[d] = np.array([v.item() for v in parts]), p.numpy()
    _assert_scalars(losses, got[torch.float32][0], got[torch.float64][0], "validation n=300 losses")
    _assert_probabilities(probs, got[torch.float32][1], got[torch.float64][1], "validation n=300 probabilities")


def test_masks_of_130_rows_whole_and_in_three_pieces():
    w = _weights("fresh")
    x, lab = _batch(130)
    got = []
    for micro in (130, 64):
        t = _capi.Trainer(0, micro)
        try:
            t.set_tensors(w)
            t.config(dropout_rates=R.DEFAULT_RATES, seed=9)
            t.zero_grad()
            got.append(_accumulate(t, x, lab, micro, masks=True)[1])
        finally:
            t.close()
    whole, pieces = got
    assert whole[0].shape == (33, 130, 256) and whole[1].shape == (130, 192) and whole[5].shape == (130, 96)
    for k, rate in enumerate(R.DEFAULT_RATES):
        assert whole[k].dtype == np.uint8 and np.array_equal(whole[k], pieces[k]), k
        count, keep = whole[k].size, 1.0 - rate
        assert set(np.unique(whole[k])) <= {0, 1}
        assert abs(whole[k].mean() - keep) <= 6 * np.sqrt(keep * (1 - keep) / count), (k, whole[k].mean(), count)


def test_masks():
    w = _weights("fresh")
    x, lab = _batch(16)
    t = _capi.Trainer(0, 16)
    try:
        t.set_tensors(w)
        t.config(dropout_rates=R.DEFAULT_RATES, seed=9)
        t.zero_grad()
        _, m16 = _accumulate(t, x, lab, 16, masks=True)
        for k, rate in enumerate(R.DEFAULT_RATES):                      # keep fraction within 6 sigma of the binomial
            count, keep = m16[k].size, 1.0 - rate
            assert set(np.unique(m16[k])) <= {0, 1}
            assert abs(m16[k].mean() - keep) <= 6 * np.sqrt(keep * (1 - keep) / count), (k, m16[k].mean(), count)
        assert m16[0].shape == (33, 16, 256) and m16[1].shape == (16, 192) and m16[5].shape == (16, 96)
        assert not np.array_equal(m16[2], m16[3])                      # the layers draw their own masks
        _, again = _accumulate(t, x, lab, 16, masks=True)             # same seed and step: the same masks
        assert all(np.array_equal(again[k], m16[k]) for k in range(6))
        # validation mode: no dropout, equal to the dropout-off forward pass
        valid = t.accumulate(x, lab, training=False)
        p_valid = t.probabilities()
        t.step(1e-3, 0.0)                                               # the next optimizer step draws other masks
        t.set_tensors(w)
        _, later = _accumulate(t, x, lab, 16, masks=True)
        assert all(not np.array_equal(later[k], m16[k]) for k in range(6))
        t.config(dropout_rates=NO_DROPOUT, seed=9)
        off = t.accumulate(x, lab, training=True)
        assert np.array_equal(off, valid) and np.array_equal(t.probabilities().view(np.uint32), p_valid.view(np.uint32))
        with pytest.raises(_capi.EngineError):
            t.accumulate(np.concatenate([x, x]), np.concatenate([lab, lab]))       # more rows than the micro-batch
        bad = lab.copy()
        bad[3, 1] = 3
        with pytest.raises(_capi.EngineError):
            t.accumulate(x, bad)
    finally:
        t.close()
    t8 = _capi.Trainer(0, 8)                                            # micro-batch 8: the same masks for the same rows of the whole batch
    try:
        t8.set_tensors(w)
        t8.config(dropout_rates=R.DEFAULT_RATES, seed=9)
        t8.zero_grad()
        _, m8 = _accumulate(t8, x, lab, 8, masks=True)
        assert all(np.array_equal(m8[k], m16[k]) for k in range(6))
    finally:
        t8.close()


def test_same_accumulate_twice_gives_identical_bits():
    _check_identical_bits(11, 8)


def test_same_accumulate_twice_gives_identical_bits_in_pieces_of_64():
    """130 rows as 64 + 64 + 2"""
    _check_identical_bits(130, 64)


def _check_identical_bits(n, micro):
    w = _weights("trained")
    x, lab = _batch(n)
    t = _capi.Trainer(0, micro)
    try:
        t.set_tensors(w)
        t.config(dropout_rates=R.DEFAULT_RATES, seed=2)
        runs = []
        for _ in range(2):
            t.zero_grad()
            losses, _ = _accumulate(t, x, lab, micro)
            runs.append((losses, t.get_tensors("gradients")))
    finally:
        t.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k].view(np.uint32), runs[1][1][k].view(np.uint32)), k
        assert np.abs(runs[0][1][k]).max() > 0, k


@pytest.mark.parametrize("task_weights,clipped", [((0.01, 0.01, 0.01, 0.01, 1), False), ((1, 1, 1, 1, 1), True)], ids=["clip_inactive", "clip_active"])
@pytest.mark.parametrize("optimizer,step", [("Adam", 1), ("Adam", 3), ("SGDM", 1)])
def test_optimizer_step_alone(optimizer, step, task_weights, clipped):
    """weights, gradients, m and v go in through clair_train_set_tensor; one step against the NumPy twin of TensorFlow's update"""
    w = _weights("fresh")
    x, lab = _batch(5)
    lr, lambd = 1e-3, 0.005
    r64, r32 = (R.loss_and_gradients(w, x, lab, task_loss_weights=task_weights, l2_lambda=0.0, dtype=d) for d in (torch.float64, torch.float32))
    g = r32["gradients"]
    m = {k: (0.3 * v).astype(np.float32) for k, v in g.items()}
    v = {k: (0.5 * v * v + 1e-12).astype(np.float32) for k, v in g.items()}
    t = _capi.Trainer(0, 8, optimizer)
    try:
        t.config(task_loss_weights=task_weights, dropout_rates=NO_DROPOUT)
        for _ in range(step - 1):                                       # the steps before: only the step count matters, everything is set anew
            t.step(lr, lambd)
        t.set_tensors(w)
        t.set_tensors(g, "gradients")
        t.set_tensors(m, "m")
        t.set_tensors(v, "v")
        l2, norm = t.step(lr, lambd)
        got = {which: t.get_tensors(which) for which in ("weights", "m", "v")}
    finally:
        t.close()
    coefficient = task_weights[4] * lambd
    reg32 = R.regularized(g, w, coefficient)
    clipped32, norm32 = R.clip_by_global_norm(reg32)
    norm64 = R.global_norm(R.regularized(r64["gradients"], w, coefficient, dtype=np.float64))
    print("%s step %d: global norm %.4g (clip %s)" % (optimizer, step, norm, "active" if norm > 5 else "inactive"))
    assert (norm > 5.0) == clipped
    _assert_scalars([l2, norm], [r32["l2"], norm32], [r64["l2"], norm64], "stats")
    for k in w:
        # the moments are sums of a moment and a gradient term: their rounding errors scale with the larger of the two
        gk = np.abs(clipped32[k])
        if optimizer == "Adam":
            want, m_want, v_want = R.adam_step(w[k], clipped32[k], m[k], v[k], step, lr)
            assert (np.abs(got["m"][k] - m_want) <= 4 * EPS32 * np.maximum(np.abs(m[k]), gk)).all(), k
            assert (np.abs(got["v"][k] - v_want) <= 4 * EPS32 * np.maximum(v[k], gk * gk)).all(), k
        else:
            want, m_want = R.momentum_step(w[k], clipped32[k], m[k], lr)
            assert (np.abs(got["m"][k] - m_want) <= 4 * EPS32 * np.maximum(np.abs(m[k]), gk)).all(), k
        bound = 4 * EPS32 * np.maximum(np.abs(w[k]), lr)
        worst = float(np.max(np.abs(got["weights"][k].astype(np.float64) - want) / bound))
        assert worst <= 1.0, (k, worst)
        assert not np.array_equal(got["weights"][k], w[k]), k


def _oracle_trajectory(w, x, lab, steps, lr, lambd, dtype, np_dtype):
    w = {k: np.asarray(v, dtype=np_dtype) for k, v in w.items()}
    acc = {k: np.zeros_like(v) for k, v in w.items()}
    for _ in range(steps):
        r = R.loss_and_gradients(w, x, lab, rates=NO_DROPOUT, l2_lambda=lambd, dtype=dtype)
        clipped, _ = R.clip_by_global_norm(r["gradients"], dtype=np_dtype)
        for k in w:
            w[k], acc[k] = R.momentum_step(w[k], clipped[k], acc[k], lr, dtype=np_dtype)
    return w


def test_trajectory():
    w = _weights("fresh")
    x, lab = _batch(6)
    lr, lambd = 0.01, 0.005
    t = _capi.Trainer(0, 8, "SGDM")
    try:
        t.set_tensors(w)
        t.config(dropout_rates=NO_DROPOUT)
        for _ in range(3):
            t.zero_grad()
            _accumulate(t, x, lab, 8)
            t.step(lr, lambd)
        dev = t.get_tensors()
    finally:
        t.close()
    w64 = _oracle_trajectory(w, x, lab, 3, lr, lambd, torch.float64, np.float64)
    w32 = _oracle_trajectory(w, x, lab, 3, lr, lambd, torch.float32, np.float32)
    _assert_tensors(dev, w32, w64, "three momentum steps, weights")
    moved = {k: dev[k].astype(np.float64) - w[k] for k in w}           # the same bound on what the three steps changed
    _assert_tensors(moved, {k: w32[k].astype(np.float64) - w[k] for k in w}, {k: w64[k] - w[k] for k in w}, "three momentum steps, change of the weights")
    a = _capi.Trainer(0, 8, "Adam")
    try:
        a.set_tensors(w)
        a.config(dropout_rates=NO_DROPOUT)
        totals = []
        for _ in range(20):
            a.zero_grad()
            losses, _ = _accumulate(a, x, lab, 8)
            totals.append(float(losses.sum()))
            a.step(1e-3, lambd)
    finally:
        a.close()
    print("20 Adam steps: loss %.4f -> %.4f" % (totals[0], totals[-1]))
    assert totals[-1] < totals[0]


def test_clair_members(tmp_path):
    from clair_amd.model import Clair
    x, lab = _batch(11)
    one_hot = np.zeros((11, 90), dtype=np.float32)
    for k, a in enumerate((0, 21, 24, 57)):
        one_hot[np.arange(11), a + lab[:, k]] = 1.0
    models = [Clair(max_batch=16, n_slots=1, micro_batch=8, seed=1) for _ in range(2)]
    try:
        m, m2 = models
        m.init()
        m2.init()
        before = m.predict(x)
        m.train(x, one_hot)
        m2.train(x, lab)
        assert m.training_loss_on_one_batch == m2.training_loss_on_one_batch and m.training_loss_on_one_batch > 0
        w, w2 = m.get_parameters(), m2.get_parameters()
        assert all(np.array_equal(w[k].view(np.uint32), w2[k].view(np.uint32)) for k in w)
        after = m.predict(x)
        assert all(np.abs(a - b).max() > 0 for a, b in zip(after, before))
        total = m.validate(x, one_hot)
        parts = (m.gt21_loss, m.genotype_loss, m.indel_length_loss_1, m.indel_length_loss_2)
        assert total == m.validation_loss_on_one_batch == pytest.approx(sum(parts)) and all(p > 0 for p in parts)
        assert m.indel_length_loss == pytest.approx(m.indel_length_loss_1 + m.indel_length_loss_2)
        l2 = sum(float(np.sum(v.astype(np.float64) ** 2)) / 2 for k, v in w.items() if not k.endswith("_bias"))
        assert m.l2_loss == pytest.approx(l2 * 0.005)
        for a, b in zip(m.validation_prediction, after):               # the trainer's forward pass and the engine's agree
            assert np.abs(a - b).max() <= 3e-6
        prefix = str(tmp_path / "saved")
        m.save_parameters(prefix)
        assert os.path.isfile(prefix + ".index")
        back = weights.load_weights(prefix)
        assert all(np.array_equal(back[k].view(np.uint32), w[k].view(np.uint32)) for k in w)
        assert m.set_learning_rate(0.01) == 0.01 and m.decay_learning_rate() == pytest.approx(0.001)
    finally:
        for model in models:
            model.close()


def test_train_command_end_to_end(tmp_path):
    raw, infos = synth.synthetic_candidates(60, "ont", seed=11)
    tensors, var_fn, prefix = str(tmp_path / "tensors.txt"), str(tmp_path / "truth.var"), str(tmp_path / "model")
    open(tensors, "w").write("\n".join(synth.tensor_records(raw, infos)) + "\n")
    with open(var_fn, "w") as f:
        for i, (ctg, pos, seq) in enumerate(infos[:10]):
            ref = seq[16]
            alt = "ACGT"[("ACGT".index(ref) + 1 + i % 3) % 4]
            f.write("%s %s %s %s %d %d\n" % (ctg, pos, ref, alt, i % 2, 1))
    r = subprocess.run([sys.executable, "-m", "clair_amd.train", "--tensor_fn", tensors, "--var_fn", var_fn, "--batch_size", "16", "--micro_batch", "8",
                        "--max_epochs", "2", "--seed", "1", "--ochk_prefix", prefix], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.isfile(prefix + "-000001.index") and os.path.isfile(prefix + "-000002.index")
    number = r"-?\d+\.\d+(e-?\d+)?"
    for epoch in (1, 2):
        assert re.search(r"^%d Training loss: %s$" % (epoch, number), r.stderr, flags=re.M), r.stderr
        assert re.search(r"^%d Validation loss \(Total/Base/Genotype/Indel_1_2\):(\t%s){5}$" % (epoch, number), r.stderr, flags=re.M), r.stderr
    assert "[INFO] The size of dataset: 60" in r.stderr and "[INFO] Best validation loss at epoch:" in r.stderr
    assert r.stdout.startswith("[INFO] Evaluation on gt21:\n[INFO] all/top1/top2/top1p/top2p: 60/") and "[INFO] evaluation on indel length 2:" in r.stdout
    vcf = str(tmp_path / "calls.vcf")
    c = subprocess.run([sys.executable, "-m", "clair_amd.call_var", "--chkpnt_fn", prefix + "-000002", "--tensor_fn", tensors, "--call_fn", vcf, "--batch_size", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    assert open(vcf).read().startswith("##fileformat=VCF")
