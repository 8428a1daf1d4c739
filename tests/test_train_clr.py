"""train_clr and learning_rate_finder without a device: Clair.clr, the accuracy rule and lr_finder against what the reference's own functions
gave (tests/golden/train_clr_cases.json, minted by tools/mint_train_clr_golden.py), the two loops over a stand-in for Clair, the parsers and
the dispatcher."""
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from clair_amd import learning_rate_finder as F
from clair_amd import param, train, train_clr
from clair_amd.model import Clair, accuracy_counts, accuracy_from_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "train_clr_cases.json")))


def _clr_case(mode, step_size):
    return next(c for c in GOLDEN["clr"] if c["mode"] == mode and c["step_size"] == step_size)


class Bare(object):
    clr = Clair.clr


# ---- Clair.clr ----------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_references():
    assert {k: getattr(param, k) for k in GOLDEN["param"]} == GOLDEN["param"]
    assert sorted(GOLDEN["param"]) == sorted(["clr_max_lr", "clr_min_lr", "stepsizeConstant", "clrGamma", "min_lr", "max_lr", "lr_finder_max_epoch"])


@pytest.mark.parametrize("case", GOLDEN["clr"], ids=lambda c: "%s-%s" % (c["mode"], c["step_size"]))
def test_clr_equals_the_reference_call_by_call(case):
    m, global_step, max_lr = Bare(), 0, case["max_lr"]
    step_size = case["step_size"] if isinstance(case["step_size"], int) else np.float64(case["step_size"])      # np.ceil's type in the loops
    for k, (want_rate, want_step, want_max) in enumerate(case["calls"]):
        rate, global_step, max_lr = m.clr(global_step, step_size, max_lr, case["mode"])
        assert float(rate) == want_rate and float(m.learning_rate_value) == want_rate, (k, rate, want_rate)     # equal, not close
        assert global_step == want_step and float(max_lr) == want_max, (k, global_step, max_lr)


def test_clr_cases_cover_three_cycles_of_every_mode_at_two_step_sizes():
    for mode in ("tri", "tri2", "exp"):
        for step_size in (4, 7.0):
            steps = [c[1] for c in _clr_case(mode, step_size)["calls"]]
            assert steps.count(0) >= 3 and len(steps) >= 3 * (2 * step_size + 1)


@pytest.mark.parametrize("mode,after_one_cycle", [("tri", 3e-2), ("tri2", 0.015), ("exp", 3e-2 * 0.95)])
def test_clr_by_hand_at_step_size_4(mode, after_one_cycle):
    """up over calls 1..4, down over 5..8, call 9 starts the next cycle at the floor: a period of 2 * step_size + 1 calls"""
    m, global_step, max_lr, rates = Bare(), 0, 3e-2, []
    for _ in range(18):
        rate, global_step, max_lr = m.clr(global_step, 4, max_lr, mode)
        rates.append(rate)
        if len(rates) == 9:
            assert max_lr == after_one_cycle and global_step == 0
    assert rates[7] == 1e-4 and rates[8] == 1e-4 and rates[3] == 1e-4 + (3e-2 - 1e-4) and abs(rates[3] - 3e-2) < 1e-17
    assert rates[0] == 1e-4 + (3e-2 - 1e-4) * 0.25
    assert [r > 1e-4 for r in rates[:9]] == [True] * 7 + [False] * 2
    if mode == "tri":
        assert rates[9:] == rates[:9]
    else:
        assert rates[12] == 1e-4 + (after_one_cycle - 1e-4) and after_one_cycle == pytest.approx({"tri2": 0.015, "exp": 0.0285}[mode], rel=1e-15)
        assert rates[17] == 1e-4


def test_clr_default_mode_is_tri():
    a, b = Bare(), Bare()
    assert a.clr(8, 4, 3e-2) == b.clr(8, 4, 3e-2, "tri") == (1e-4, 0, 3e-2)


# ---- the accuracy rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN["accuracy"], ids=lambda c: c["name"])
def test_accuracy_counts_and_accuracy(case):
    p, lab = np.array(case["probabilities"], dtype=np.float32), np.array(case["labels"], dtype=np.uint8)
    tp = accuracy_counts(p, lab)
    assert tp.dtype == np.int64 and tp.shape == (4,)
    if case["counts"] is not None:
        assert list(tp) == case["counts"]
    assert accuracy_from_counts(tp, len(p)) == case["accuracy"]             # the reference's float, not a close one


def test_accuracy_cases_cover_what_they_are_for():
    names = [c["name"] for c in GOLDEN["accuracy"]]
    assert any("swapped on either side, equal elements" in n for n in names) and any("ties" in n for n in names)
    assert sum(len(c["labels"]) == 1 for c in GOLDEN["accuracy"]) >= 2
    four = GOLDEN["accuracy"][0]
    assert four["accuracy"] == 0.875 and four["counts"] == [3, 4, 4, 3]
    tie = next(c for c in GOLDEN["accuracy"] if "ties" in c["name"])
    p = np.array(tie["probabilities"], dtype=np.float32)
    assert (p[0, :21] == p[0, :21].max()).sum() == 2 and (p[0, 57:] == p[0, 57:].max()).sum() == 2      # real ties, bit-equal values


def test_accuracy_counts_takes_one_hot_free_inputs_and_refuses_other_shapes():
    assert list(accuracy_counts(np.zeros((0, 90), dtype=np.float32), np.zeros((0, 4), dtype=np.uint8))) == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        accuracy_counts(np.zeros((2, 90)), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        accuracy_counts(np.zeros((2, 89)), np.zeros((2, 4)))
    assert accuracy_from_counts(np.array([1, 2, 3, 4]), 4) == (0.25 + 0.5 + 0.75 + 1.0) / 4


# ---- lr_finder -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in GOLDEN["lr_finder"] if "raises" not in c], ids=lambda c: c["name"])
def test_lr_finder_rates_table_and_csv_bytes(case):
    minimum_lr, maximum_lr, table = F.lr_finder(case["rows"])
    assert (minimum_lr, maximum_lr) == (case["min_lr"], case["max_lr"]) and minimum_lr <= maximum_lr
    assert [list(r) for r in table] == case["table"] and len(table) == len(case["rows"]) - 1
    assert F.table_text(table) == case["csv"] and case["csv"].startswith("lr,accuracy,loss,diff\n")


def test_lr_finder_ties_take_the_first_row_of_the_references_sort():
    """the reference raises on both (recorded); here the largest rate among the rows tied for min_lr, the smallest among those tied for max_lr"""
    tied = {c["name"]: c for c in GOLDEN["lr_finder"] if "raises" in c}
    assert len(tied) == 2 and all(c["raises"] == "ValueError" for c in tied.values())
    rows = tied["tied for the largest diff"]["rows"]            # diffs .25 -.125 .25 -.625: 0.02 and 0.04 tie for the largest
    assert F.lr_finder(rows)[:2] == (0.04, 0.05)
    rows = tied["tied for the smallest diff"]["rows"]           # diffs -.25 .5 -.25: 0.02 and 0.04 tie for the smallest; 0.03 rises most -> swapped
    assert F.lr_finder(rows)[:2] == (0.02, 0.03)
    with pytest.raises(ValueError):
        F.lr_finder([(0.1, 0.5, 1.0)])


# ---- the loops over a stand-in for Clair ---------------------------------------------------------------------------------------------------
class StandIn(object):
    """Records (what, learning_rate_value, rows) per train / lr_train / validate call; clr is Clair's own."""
    clr = Clair.clr

    def __init__(self):
        self.learning_rate_value, self.calls, self.saved, self.restored = None, [], [], []

    def set_learning_rate(self, v):
        self.learning_rate_value = v
        return v

    def set_l2_regularization_lambda(self, v):
        self.lambd = v
        return v

    def restore_parameters(self, path):
        self.restored.append(path)

    def save_parameters(self, path):
        self.saved.append(path)

    def train(self, x, y):
        self.calls.append(("train", self.learning_rate_value, len(x)))
        self.training_loss_on_one_batch = 2.0 * len(x)

    def lr_train(self, x, y):
        self.calls.append(("lr_train", self.learning_rate_value, len(x)))
        self.training_loss_on_one_batch = 2.0 * len(x)
        self.training_accuracy = (len(self.calls) * 7 % 16) / 16.0

    def validate(self, x, y):
        self.calls.append(("validate", self.learning_rate_value, len(x)))
        self.validation_loss_on_one_batch = float(len(self.calls))
        self.gt21_loss = self.genotype_loss = self.indel_length_loss_1 = self.indel_length_loss_2 = 0.25


N_ROWS, BATCH = 2345, 300         # 2110 training rows: seven batches of 300 and one of 10; 235 validation rows: one batch


def _data():
    return np.zeros((N_ROWS, 1), dtype=np.float32), np.zeros((N_ROWS, 4), dtype=np.uint8)


def test_step_size_for_sizes_that_do_not_divide():
    n_train, n_validation, _ = train.split_sizes(N_ROWS)
    assert (n_train, n_validation) == (2110, 235)
    assert train_clr.step_size_of(n_train, n_validation, BATCH) == 9 + 2 == param.stepsizeConstant * (np.ceil(2110 / 300 + 1) + np.ceil(235 / 1000 + 1))
    assert train_clr.step_size_of(n_train, n_validation, BATCH, with_validation=False) == 9
    assert train_clr.step_size_of(9000, 1000, 1000) == 10 + 2                     # sizes that divide: n / b + 1 is whole already
    assert train_clr.step_size_of(9001, 1001, 1000) == 11 + 3
    assert train_clr.step_size_of(7, 3, 2) == 5 + 2                               # true division: 7 / 2 + 1 = 4.5


@pytest.mark.parametrize("mode", ["tri", "tri2", "exp"])
def test_train_clr_loop_advances_clr_once_before_every_batch(mode, tmp_path):
    """three epochs of nine batches at step_size 11: the cycle wraps in the third epoch, so global_step and the decayed max_lr are carried"""
    m, (X, Y) = StandIn(), _data()
    np.random.seed(3)
    cycle = train_clr.Cycle(m, train_clr.step_size_of(2110, 235, BATCH), param.clr_max_lr, mode)
    prefix = str(tmp_path / "model")
    history = train_clr.train_model(m, X, Y, 5e-3, 0.005, prefix, None, BATCH, 3, cycle)
    want = [c[0] for c in _clr_case(mode, 11.0)["calls"]]
    epoch = [("train", 300)] * 7 + [("train", 10), ("validate", 235)]
    assert [(what, n) for what, _, n in m.calls] == epoch * 3
    assert [float(rate) for _, rate, _ in m.calls] == want[:27]                   # two epochs are the first 18; the third crosses the wrap at call 23
    assert want[:18] == sorted(want[:11]) + sorted(want[11:18], reverse=True) and want[21] == want[22] == 1e-4
    assert (cycle.global_step, float(cycle.max_lr)) == tuple(_clr_case(mode, 11.0)["calls"][26][1:])
    assert m.saved == [os.path.abspath("%s-%06d" % (prefix, e)) for e in (1, 2, 3)] and m.restored == []
    assert [e for _, e in history] == [1, 2, 3] and [v for v, _ in history] == [9.0, 18.0, 27.0]
    assert m.lambd == 0.005


def test_train_clr_loop_numbers_epochs_from_the_checkpoint_and_max_epochs_is_absolute(tmp_path, caplog):
    m, (X, Y) = StandIn(), _data()
    start, prefix = str(tmp_path / "old-000004"), str(tmp_path / "new")
    cycle = train_clr.Cycle(m, 11.0, param.clr_max_lr, "exp")
    with caplog.at_level(logging.INFO):
        history = train_clr.train_model(m, X, Y, 7e-3, 0.005, prefix, start, BATCH, 6, cycle)
    assert [e for _, e in history] == [5, 6] and m.restored == [os.path.abspath(start)]
    assert m.saved == [os.path.abspath(prefix + "-000005"), os.path.abspath(prefix + "-000006")]
    lines = caplog.text
    assert "[INFO] Learning rate: 7.00e-03" in lines                             # --learning_rate shows here and nowhere else
    assert all(rate != 7e-3 for _, rate, _ in m.calls) and float(m.calls[0][1]) == _clr_case("exp", 11.0)["calls"][0][0]
    assert "5 Training loss: 2.0" in lines and "6 Validation loss (Total/Base/Genotype/Indel_1_2):\t" in lines and "[INFO] Shuffled:" in lines
    assert "New learning rate" not in lines
    with pytest.raises(SystemExit) as ei:
        train_clr.train_model(StandIn(), X, Y, 7e-3, 0.005, prefix, start, BATCH, 4, cycle)
    assert str(ei.value.code).startswith("[ERROR]") and "absolute" in ei.value.code


def test_train_clr_has_no_learning_rate_switch_and_no_early_stop(tmp_path):
    """validation totals that rise for nine epochs make train switch its rate; here nothing but clr touches it and every epoch runs"""
    m, (X, Y) = StandIn(), _data()
    cycle = train_clr.Cycle(m, 11.0, param.clr_max_lr, "tri")
    history = train_clr.train_model(m, X, Y, 1e-4, 0.005, str(tmp_path / "m"), None, 2110, 12, cycle)
    assert len(history) == 12 and [v for v, _ in history] == sorted(v for v, _ in history)
    assert train.learning_rate_is_due(9, [v for v, _ in history][:9])
    want = [c[0] for c in _clr_case("tri", 11.0)["calls"]]
    assert [float(rate) for _, rate, _ in m.calls] == want[:24]


def test_finder_loop_rows_table_and_log(tmp_path, caplog):
    m, (X, Y) = StandIn(), _data()
    olr_fn = str(tmp_path / "rates.txt")
    with caplog.at_level(logging.INFO):
        history = F.find_rates(m, X, Y, 0.005, str(tmp_path / "f"), None, BATCH, olr_fn)
    want = [c[0] for c in _clr_case("tri", 9.0)["calls"]]                        # step_size 9: the training batches alone
    assert [what for what, _, _ in m.calls] == ["lr_train"] * 8 + ["validate"]
    assert [float(rate) for _, rate, _ in m.calls] == want[:9]                   # clr advanced before the validation batch too
    assert [e for _, e in history] == [1] and m.saved == [os.path.abspath(str(tmp_path / "f") + "-000001")]
    text = open(olr_fn).read().splitlines()
    assert text[0] == "lr,accuracy,loss,diff" and len(text) == 8
    rows = [[float(v) for v in line.split(",")] for line in text[1:]]
    assert [r[0] for r in rows] == want[1:8]                                     # the first row is dropped
    accuracies = [((k + 1) * 7 % 16) / 16.0 for k in range(8)]
    assert [r[1] for r in rows] == accuracies[1:] and [r[3] for r in rows] == [b - a for a, b in zip(accuracies, accuracies[1:])]
    assert [r[2] for r in rows] == [600.0] * 6 + [20.0]
    minimum_lr, maximum_lr, _ = F.lr_finder(list(zip(want[:8], accuracies, [0.0] * 8)))
    assert "[INFO] min_lr: %g, max_lr: %g" % (minimum_lr, maximum_lr) in caplog.text
    assert "[INFO] Learning rate: %.2e" % param.min_lr in caplog.text and all(rate >= param.clr_min_lr for _, rate, _ in m.calls)


def test_finder_needs_two_training_batches(tmp_path):
    m, (X, Y) = StandIn(), _data()
    with pytest.raises(SystemExit) as ei:
        F.find_rates(m, X, Y, 0.005, str(tmp_path / "f"), None, 2110, str(tmp_path / "rates.txt"))
    assert str(ei.value.code).startswith("[ERROR]") and m.calls == [] and not os.path.exists(str(tmp_path / "rates.txt"))


def test_run_epoch_without_hooks_is_trains(tmp_path):
    m, (X, Y) = StandIn(), _data()
    trained, validated = train.run_epoch(m, X, Y, np.arange(N_ROWS), 2110, BATCH)
    assert [what for what, _, _ in m.calls] == ["train"] * 8 + ["validate"] and trained == 2.0 * 2110 and validated[0] == 9.0


# ---- parsers, exits, dispatcher --------------------------------------------------------------------------------------------------------------
def test_train_clr_parser_defaults_are_the_references():
    a = train_clr.build_parser().parse_args([])
    assert a.clr_mode == "exp" and a.learning_rate == param.clr_min_lr == 1e-4
    assert (a.SGDM, a.Adam, a.cross_entropy, a.focal_loss) == (False, False, False, False)
    assert (a.bin_fn, a.train_bin_fn, a.validation_bin_fn, a.tensor_fn, a.var_fn, a.bed_fn, a.chkpnt_fn) == (None, None, None, "vartensors", "truthvars", None, None)
    assert (a.lambd, a.ochk_prefix, a.olog_dir) == (0.005, None, None)
    assert (a.batch_size, a.micro_batch, a.device, a.seed, a.max_epochs, a.set_fn) == (10000, 1024, 0, None, param.maxEpoch, None)
    assert train.build_parser().parse_args([]).learning_rate == 1e-3              # train's own default is untouched
    for mode in ("tri", "tri2", "exp"):
        assert train_clr.build_parser().parse_args(["--clr_mode", mode]).clr_mode == mode
    with pytest.raises(SystemExit):
        train_clr.build_parser().parse_args(["--clr_mode", "cosine"])


def test_finder_parser_defaults_are_the_references():
    a = F.build_parser().parse_args([])
    assert (a.bin_fn, a.tensor_fn, a.var_fn, a.bed_fn, a.chkpnt_fn) == (None, "vartensors", "truthvars", None, None)
    assert (a.learning_rate, a.lambd, a.ochk_prefix, a.olog_dir, a.olr_fn) == (param.initialLearningRate, 0.005, None, None, "lr_finder.txt")
    assert (a.batch_size, a.micro_batch, a.device, a.seed, a.set_fn) == (10000, 1024, 0, None, None)
    assert (a.SGDM, a.Adam, a.cross_entropy, a.focal_loss) == (False, False, False, False)
    for flag in ("--train_bin_fn", "--validation_bin_fn", "--max_epochs"):       # not flags of the reference's finder
        with pytest.raises(SystemExit):
            F.build_parser().parse_args([flag, "1"])


@pytest.mark.parametrize("module,flag", [(train_clr, "--bin_fn"), (train_clr, "--train_bin_fn"), (train_clr, "--validation_bin_fn"), (F, "--bin_fn")])
def test_binary_flags_exit_with_the_message(module, flag):
    from clair_amd.evaluate import BINARY_MESSAGE
    with pytest.raises(SystemExit) as ei:
        train.check_arguments(module.build_parser().parse_args([flag, "x.bin", "--ochk_prefix", "out"]))
    assert ei.value.code == BINARY_MESSAGE


@pytest.mark.parametrize("module", [train_clr, F])
def test_ochk_prefix_is_required(module):
    with pytest.raises(SystemExit) as ei:
        train.check_arguments(module.build_parser().parse_args(["--tensor_fn", "t"]))
    assert ei.value.code == "[ERROR] --ochk_prefix is required"
    train.check_arguments(module.build_parser().parse_args(["--ochk_prefix", "out"]))


def test_commands_exit_before_anything_is_loaded():
    from clair_amd.evaluate import BINARY_MESSAGE
    for module in ("clair_amd.train_clr", "clair_amd.learning_rate_finder"):
        r = subprocess.run([sys.executable, "-m", module, "--bin_fn", "x.bin", "--ochk_prefix", "out"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and BINARY_MESSAGE in r.stderr
        r = subprocess.run([sys.executable, "-m", module, "--tensor_fn", "t"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and "[ERROR] --ochk_prefix is required" in r.stderr
        r = subprocess.run([sys.executable, "-m", module], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 1 and "--ochk_prefix" in r.stdout


def test_dispatcher_lists_train_clr_and_prints_its_help():
    r = subprocess.run([sys.executable, "-m", "clair_amd"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "      - train_clr" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "train_clr"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--clr_mode {tri,tri2,exp}" in r.stdout and "usage: train_clr" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "learning_rate_finder"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "not found" in r.stderr                         # started as a module, as in the reference
