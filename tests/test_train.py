"""train without a GPU: the autograd oracle (tools/torch_train_ref.py) against the forward oracle and a NumPy restatement of the losses, the
dropout_selu constants, the NumPy optimizer twin on hand-worked values, the learning-rate predicates, the block shuffle and the split,
the parser, and Clair's training keywords."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from clair_amd import _capi, param, synth, weights       # noqa: E402
from clair_amd import train as T                          # noqa: E402

import torch                                              # noqa: E402
import torch_ref                                          # noqa: E402
import torch_train_ref as R                               # noqa: E402

HEADS = ((0, 21), (21, 24), (24, 57), (57, 90))


def _labels(n, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, s, n) for s in (21, 3, 33, 33)], axis=1).astype(np.uint8)


@pytest.fixture(scope="module")
def case():
    torch.set_num_threads(4)
    w = weights.synthetic_weights(head_gain=3.0)
    x, _ = synth.synthetic_input(5, seed=7)
    lab = _labels(5)
    return w, x, lab


def test_oracle_forward_equals_torch_ref(case):
    w, x, lab = case
    want, _ = torch_ref.forward(w, x, dtype=torch.float64)
    got = R.loss_and_gradients(w, x, lab, dtype=torch.float64)["probabilities"]
    assert np.abs(got - np.concatenate(want, axis=1)).max() < 1e-12


def _numpy_losses(P, lab, loss, class_weights):
    """clair/model.py:247-263 and 784-805 from probabilities, float64"""
    parts = []
    for k, (a, b) in enumerate(HEADS):
        p = P[:, a:b].astype(np.float64)
        y = np.zeros_like(p)
        y[np.arange(len(p)), lab[:, k]] = 1.0
        if loss == "CrossEntropy":
            parts.append(float(-np.sum(y * np.log(p + 1e-10) * class_weights[a:b])))
        else:
            pos = np.where(y > 0, y - p, 0.0)
            neg = np.where(y > 0, 0.0, p)
            parts.append(float(-np.sum(pos ** 2 * np.log(np.clip(p, 1e-8, 1.0)) + neg ** 2 * np.log(np.clip(1.0 - p, 1e-8, 1.0)))))
    return np.array(parts)


@pytest.mark.parametrize("loss", ["FocalLoss", "CrossEntropy"])
def test_oracle_losses_equal_numpy_restatement(case, loss):
    w, x, lab = case
    cw = np.linspace(0.5, 2.0, 90)
    r = R.loss_and_gradients(w, x, lab, loss, class_weights=cw, task_loss_weights=(1, 2, 3, 4, 0.5), l2_lambda=0.005, dtype=torch.float64)
    want = _numpy_losses(r["probabilities"], lab, loss, cw)
    assert np.allclose(r["parts"], want, rtol=1e-12, atol=0)
    l2 = sum(float(np.sum(v.astype(np.float64) ** 2)) / 2 for k, v in w.items() if not k.endswith("_bias"))
    assert abs(r["l2"] - l2) <= 1e-12 * l2
    assert abs(r["total"] - (np.dot([1, 2, 3, 4], want) + 0.5 * 0.005 * l2)) <= 1e-12 * r["total"]
    assert set(r["gradients"]) == set(weights.TENSOR_TABLE) and all(r["gradients"][k].shape == tuple(s) for k, s in weights.TENSOR_TABLE.items())


def test_oracle_float32_is_close_to_float64(case):
    w, x, lab = case
    r64, r32 = (R.loss_and_gradients(w, x, lab, dtype=d) for d in (torch.float64, torch.float32))
    for k in r64["gradients"]:
        assert np.linalg.norm(r32["gradients"][k] - r64["gradients"][k]) <= 1e-5 * np.linalg.norm(r64["gradients"][k]), k


def test_pre_activations_are_the_networks_own(case):
    """selu of the heads' pre-activations is network()'s output, and the shapes are the documented ones"""
    w, x, lab = case
    z = R.pre_activations(w, x)
    assert [(k, v.shape) for k, v in z.items()] == [("l3", (5, 30, 256)), ("l4", (5, 192)), ("l5_0", (5, 96)), ("head_gt21", (5, 21)), ("l5_1", (5, 96)),
                                                    ("head_genotype", (5, 3)), ("l5_2", (5, 96)), ("head_len1", (5, 33)), ("l5_3", (5, 96)), ("head_len2", (5, 33))]
    logits = torch.cat([R.selu(torch.tensor(z["head_%s" % name])) for name, _, _ in R.HEADS], dim=1)
    _, probs = R.head_losses(logits, lab)
    assert np.array_equal(probs.numpy(), R.loss_and_gradients(w, x, lab, dtype=torch.float64)["probabilities"])
    assert all(v.dtype == np.float32 for v in R.pre_activations(w, x, dtype=torch.float32).values())


@pytest.mark.parametrize("n,seed", [(130, 7), (70, 9)])
def test_clear_of_the_selu_kink(n, seed):
    """Fresh weights on these two batches (built as tests/test_train_gpu.py builds them) put one L3 unit so close to zero that the float32
    and the float64 oracle disagree on its sign; SELU's derivative jumps there, and the float32 oracle's distance from float64 -- the yardstick
    of the device tests -- grows from 1e-6 to 3e-4 and more.  After the preparation no unit is within the margin and the yardstick is back."""
    torch.set_num_threads(4)
    w = weights.synthetic_weights()
    x, _ = synth.synthetic_input(n, seed=seed)
    lab = _labels(n, seed + 1)

    def yardsticks(w):
        r64, r32 = (R.loss_and_gradients(w, x, lab, dtype=d)["gradients"] for d in (torch.float64, torch.float32))
        return {k: np.linalg.norm(r32[k] - r64[k]) / np.linalg.norm(r64[k]) for k in r64}

    z64, z32 = (R.pre_activations(w, x, dtype=d) for d in (torch.float64, torch.float32))
    assert R.sign_disagreements(z32, z64) >= 1
    before = max(yardsticks(w).values())
    assert before > 1e-4
    prepared, report = R.clear_of_the_selu_kink(w, x)
    print("n=%d seed %d: yardstick %.3g before; margin %.3g, %d rounds, %d biases moved, smallest |z| %.3g" %
          (n, seed, before, report["margin"], report["rounds"], report["moved"], report["smallest"]))
    z64, z32 = (R.pre_activations(prepared, x, dtype=d) for d in (torch.float64, torch.float32))
    assert R.sign_disagreements(z32, z64) == 0
    assert all(np.abs(v).min() >= report["margin"] for v in z64.values()) and report["smallest"] >= report["margin"]
    assert 1e-8 < report["margin"] < 1e-4 and 1 <= report["rounds"] <= 40 and report["moved"] >= 1
    for k, err in yardsticks(prepared).items():
        assert err <= 1e-5, (k, err)
    for k in w:
        assert prepared[k].dtype == np.float32 and prepared[k].shape == w[k].shape
        assert k.endswith("_bias") or np.array_equal(prepared[k], w[k]), k
    assert any(not np.array_equal(prepared[k], w[k]) for k in w)
    again = weights.synthetic_weights()
    assert all(np.array_equal(w[k], again[k]) for k in w)      # the argument is left as it was


@pytest.mark.parametrize("rate", [0.5, 0.2])
def test_dropout_selu_constants(rate):
    """clair/selu.py:64-66: a and b keep mean 0 and variance 1 of a unit-variance input"""
    alpha, a, b = R.dropout_selu_constants(rate)
    keep = 1.0 - rate
    assert alpha == -1.7580993408473766
    assert a == pytest.approx((keep * ((1 - keep) * alpha ** 2 + 1)) ** -0.5, rel=1e-15)
    assert b == pytest.approx(-a * (1 - keep) * alpha, rel=1e-15)
    # mean of a * (x * m + alpha (1 - m)) + b over x ~ (0, 1), m ~ Bernoulli(keep) is 0 and its variance 1
    assert a * (1 - keep) * alpha + b == pytest.approx(0.0, abs=1e-15)
    assert a * a * (keep * 1.0 + (1 - keep) * alpha ** 2 - ((1 - keep) * alpha) ** 2) == pytest.approx(1.0, rel=1e-12)
    x = torch.tensor([[1.0, -2.0]], dtype=torch.float64)
    out = R.dropout_selu(x, torch.tensor([[1.0, 0.0]], dtype=torch.float64), rate).numpy()
    assert out[0, 0] == pytest.approx(a * 1.0 + b) and out[0, 1] == pytest.approx(a * alpha + b)
    assert R.dropout_selu_constants(0.0)[1:] == (1.0, 0.0)


def test_adam_twin_two_steps_by_hand():
    """w = 1, g = 0.5 then 0.25, lr = 0.1: m1 = 0.05, v1 = 0.00025, lr_1 = 0.1 sqrt(0.001) / 0.1 -> w1 = 1 - 0.1 (the sign step);
    m2 = 0.07, v2 = 0.00031225, lr_2 = 0.1 sqrt(0.001999) / 0.19"""
    w, m, v = R.adam_step([1.0], [0.5], [0.0], [0.0], 1, 0.1)
    assert m[0] == pytest.approx(0.05, rel=1e-6) and v[0] == pytest.approx(0.00025, rel=1e-4)
    assert w[0] == pytest.approx(1.0 - 0.1 * 0.05 / (np.sqrt(0.00025) + 1e-8) * np.sqrt(0.001) / 0.1, rel=1e-6)
    assert w[0] == pytest.approx(0.9, abs=1e-6)
    w2, m2, v2 = R.adam_step(w, [0.25], m, v, 2, 0.1)
    assert m2[0] == pytest.approx(0.07, rel=1e-6) and v2[0] == pytest.approx(0.00031225, rel=1e-4)
    lr_2 = 0.1 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    assert w2[0] == pytest.approx(0.9 - lr_2 * 0.07 / (np.sqrt(0.00031225) + 1e-8), rel=1e-6)
    assert all(a.dtype == np.float32 for a in (w2, m2, v2))


def test_momentum_twin_two_steps_by_hand():
    w, acc = R.momentum_step([1.0], [0.5], [0.0], 0.1)
    assert acc[0] == pytest.approx(0.5) and w[0] == pytest.approx(0.95, rel=1e-6)
    w, acc = R.momentum_step(w, [0.25], acc, 0.1)
    assert acc[0] == pytest.approx(0.7, rel=1e-6) and w[0] == pytest.approx(0.88, rel=1e-6)


def test_clip_by_global_norm_below_and_above_5():
    g = {"a_kernel": np.array([3.0, 0.0], dtype=np.float32), "a_bias": np.array([0.0, 4.0], dtype=np.float32)}     # norm 5: untouched at the edge
    clipped, norm = R.clip_by_global_norm(g)
    assert norm == pytest.approx(5.0) and all(np.array_equal(clipped[k], g[k]) for k in g)
    small = {k: v * np.float32(0.5) for k, v in g.items()}
    clipped, norm = R.clip_by_global_norm(small)
    assert norm == pytest.approx(2.5) and all(np.array_equal(clipped[k], small[k]) for k in g)
    big = {k: v * np.float32(4) for k, v in g.items()}
    clipped, norm = R.clip_by_global_norm(big)
    assert norm == pytest.approx(20.0)
    assert np.allclose(clipped["a_kernel"], [3.0, 0.0], rtol=1e-6) and np.allclose(clipped["a_bias"], [0.0, 4.0], rtol=1e-6)
    assert R.global_norm(clipped) == pytest.approx(5.0, rel=1e-6)
    reg = R.regularized(g, {"a_kernel": np.array([10.0, 10.0]), "a_bias": np.array([10.0, 10.0])}, 0.5)
    assert np.array_equal(reg["a_kernel"], [8.0, 5.0]) and np.array_equal(reg["a_bias"], [0.0, 4.0])           # biases are not regularised


def _schedule(totals):
    return T.minimum_is_recent(totals), T.zigzags(totals), T.stays_above_minimum(totals)


def test_learning_rate_predicates_on_written_out_histories():
    """(minimum among the last five, last six alternate, last five all above the minimum) -- the truth tables of clair/train.py:18-62"""
    assert _schedule([5, 4, 3, 2, 1]) == (True, False, False)
    assert _schedule([1, 2, 1, 2, 1, 2]) == (True, False, False)              # six epochs or fewer: the two later questions are never yes
    assert _schedule([0.5, 3, 2, 3, 2, 3, 2]) == (False, True, True)          # minimum at the start, the last six go down-up-down-up-down
    assert _schedule([0.5, 2, 3, 2, 3, 2, 3]) == (False, True, True)          # ... or up-down-up-down-up
    assert _schedule([0.5, 3, 2, 3, 2, 2, 3]) == (False, False, True)         # a flat step breaks the alternation
    assert _schedule([7, 6, 5, 4, 3, 2, 1]) == (True, False, False)
    assert _schedule([1, 2, 1.5, 4, 5, 6, 7]) == (False, False, True)
    assert _schedule([5, 4, 3, 1, 2, 3, 4]) == (True, False, False)           # the minimum is among the last five
    assert _schedule([1, 9, 9, 9, 9, 9, 1]) == (True, False, False)           # a tie with the minimum counts as reaching it
    # the switch rule: six epochs at a rate for the zigzag, eight for the steady rise
    zigzag, rising = [0.5, 3, 2, 3, 2, 3, 2], [1, 2, 1.5, 4, 5, 6, 7, 8]
    assert not T.learning_rate_is_due(5, zigzag) and T.learning_rate_is_due(6, zigzag)
    assert not T.learning_rate_is_due(7, rising) and T.learning_rate_is_due(8, rising)
    assert not T.learning_rate_is_due(30, [7, 6, 5, 4, 3, 2, 1])


def test_block_shuffle_and_split_on_1203_rows():
    n_train, n_validation, n_blocks = T.split_sizes(1203)
    assert (n_train, n_validation, n_blocks) == (1082, 121, 2)
    blocks = np.arange(3)                                 # 1203 rows: blocks of 500, 500 and 203 rows
    np.random.seed(4)
    seen = set()
    for _ in range(20):
        out = T.permute_leading_blocks(blocks, n_blocks)
        assert sorted(out[:2]) == [0, 1] and out[2] == 2      # only the first two blocks are permuted
        seen.add(tuple(int(b) for b in out))
        rows = T.row_order(out, 1203)
        assert len(rows) == 1203 and sorted(rows) == list(range(1203)) and list(rows[1000:]) == list(range(1000, 1203))
        assert list(rows[:3]) == [out[0] * 500 + k for k in range(3)]
    assert seen == {(0, 1, 2), (1, 0, 2)}
    assert list(blocks) == [0, 1, 2]                      # the argument is left as it was
    whole = T.permute_leading_blocks(np.arange(3), 5)    # n past the end: everything is shuffled
    assert sorted(whole) == [0, 1, 2]
    assert list(T.permute_leading_blocks(np.arange(1), 0)) == [0]
    assert T.checkpoint_name("out/model", 7) == "out/model-000007"


def test_parser_defaults_are_the_references():
    a = T.build_parser().parse_args([])
    assert (a.SGDM, a.Adam, a.cross_entropy, a.focal_loss) == (False, False, False, False)
    assert (a.bin_fn, a.train_bin_fn, a.validation_bin_fn, a.tensor_fn, a.var_fn, a.bed_fn, a.chkpnt_fn) == (None, None, None, "vartensors", "truthvars", None, None)
    assert (a.learning_rate, a.lambd, a.ochk_prefix, a.olog_dir) == (1e-3, 0.005, None, None)
    assert (a.batch_size, a.micro_batch, a.device, a.seed, a.max_epochs) == (10000, 1024, 0, None, 30)
    assert (param.default_optimizer, param.default_loss_function, param.momentum, param.maxEpoch) == ("Adam", "FocalLoss", 0.9, 30)
    assert (param.learningRateDecay, param.maxLearningRateSwitch, param.trainingDatasetPercentage, param.bloscBlockSize) == (0.1, 3, 0.9, 500)
    assert (param.l2RegularizationLambdaDecay, param.parameterOutputPlaceHolder, param.trainBatchSize) == (1, 6, 10000)


@pytest.mark.parametrize("flag", ["--bin_fn", "--train_bin_fn", "--validation_bin_fn"])
def test_binary_flags_exit_with_the_message(flag):
    from clair_amd.evaluate import BINARY_MESSAGE
    with pytest.raises(SystemExit) as ei:
        T.check_arguments(T.build_parser().parse_args([flag, "x.bin", "--ochk_prefix", "out"]))
    assert ei.value.code == BINARY_MESSAGE


def test_ochk_prefix_is_required():
    with pytest.raises(SystemExit) as ei:
        T.check_arguments(T.build_parser().parse_args(["--tensor_fn", "t"]))
    assert ei.value.code == "[ERROR] --ochk_prefix is required"
    T.check_arguments(T.build_parser().parse_args(["--ochk_prefix", "out"]))


def test_clair_accepts_the_training_keywords():
    from clair_amd.model import Clair, training_defaults
    d = training_defaults()
    assert (d["optimizer_name"], d["loss_function"], d["LSTM2_dropout_rate"], d["L4_dropout_rate"], d["L5_3_dropout_rate"]) == ("Adam", "FocalLoss", 0.5, 0.5, 0.2)
    assert (d["initial_learning_rate"], d["learning_rate_decay"], d["l2_regularization_lambda"], d["l2_regularization_lambda_decay_rate"]) == (1e-3, 0.1, 0.005, 1)
    kwargs = dict(d, optimizer_name="SGDM", loss_function="CrossEntropy", task_loss_weights=[1, 2, 3, 4, 5], initial_learning_rate=0.01, max_batch=16, n_slots=1)
    printed = io.StringIO()
    m = None
    with contextlib.redirect_stdout(printed):
        try:
            m = Clair(no_such_parameter=3, **kwargs)
        except _capi.EngineError as exc:                  # no HIP device here: the keywords were read before the engine was asked for
            assert "no HIP device" in str(exc)
    assert printed.getvalue() == "Info: the parameter no_such_parameter, with value 3 is not supported\n"
    if m is not None:
        assert (m.optimizer_name, m.loss_function, m.learning_rate_value) == ("SGDM", "CrossEntropy", 0.01) and list(m.task_loss_weights) == [1, 2, 3, 4, 5]
        assert m.decay_learning_rate() == pytest.approx(0.001) and m.set_l2_regularization_lambda(0.1) == 0.1 and m.decay_l2_regularization_lambda() == 0.1
        m.close()
    with pytest.raises(ValueError):
        Clair(optimizer_name="RMSProp", max_batch=16, n_slots=1)


def test_label_indices_from_one_hot_rows():
    from clair_amd.model import Clair
    lab = _labels(7)
    one_hot = np.zeros((7, 90), dtype=np.float32)
    for k, (a, _) in enumerate(HEADS):
        one_hot[np.arange(7), a + lab[:, k]] = 1.0
    assert np.array_equal(Clair.label_indices(one_hot), lab) and np.array_equal(Clair.label_indices(lab), lab)
    with pytest.raises(ValueError):
        Clair.label_indices(np.zeros((7, 3)))


def test_trainer_create_argument_validation_and_missing_device():
    import ctypes
    lib = _capi.load()
    h = ctypes.c_void_p()
    for args, word in (((0, 0, 0, 0), b"micro_batch"), ((0, 8, 2, 0), b"optimizer"), ((0, 8, 0, 2), b"loss")):
        assert lib.clair_train_create(*args, ctypes.byref(h)) != 0 and not h.value
        assert word in lib.clair_train_last_error(None)
    if lib.clair_device_count() <= 0:
        with pytest.raises(_capi.EngineError) as ei:
            _capi.Trainer(0, 8)
        assert "no HIP device" in str(ei.value)
