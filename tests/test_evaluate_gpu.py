"""evaluate on the device: eval_kernel (clair_amd/csrc/evaluate.hip.h) against its NumPy twin, and the command end to end against the
report the reference's own loop printed for the oracle's probabilities (tests/golden/evaluate_small.*)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clair_amd import _capi, evaluate, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_evaluate import SMALL, assert_same_report, crafted_rows  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = ((0, 21), (21, 24), (24, 57), (57, 90))


def _labels(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, k, n) for k in (21, 3, 33, 33)], axis=1).astype(np.uint8)


def test_clair_eval_on_crafted_ties(engine):
    P, lab = crafted_rows()
    engine.eval_reset()
    assert not engine.eval_read().any()
    engine.eval_probabilities([P[:, a:b] for a, b in SPLITS], lab)
    got = engine.eval_read()
    assert np.array_equal(got, evaluate.evaluate_counts_host(P, lab))
    # one row at a time, on both slots: the same block
    engine.eval_reset()
    for i in range(len(P)):
        engine.eval_probabilities([P[i:i + 1, a:b] for a, b in SPLITS], lab[i:i + 1], slot=i % 2)
    assert np.array_equal(engine.eval_read(), got)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 1024])
@pytest.mark.parametrize("counts", [False, True])
def test_submit_eval_scores_the_pass_it_ran(engine, n, counts):
    raw, _ = synth.synthetic_candidates(n, "ont", seed=100 + n)
    batch = raw.astype(np.int16) if counts else synth.to_model_input(raw)
    lab = _labels(n, n)
    engine.eval_reset()
    engine.submit_eval(0, batch, lab, counts=counts, with_probabilities=True)
    Y = engine.wait(0)
    got = engine.eval_read()
    assert np.array_equal(got, evaluate.evaluate_counts_host(Y, lab))          # the probabilities that same pass returned
    assert got[0] == n
    # the scoring does not disturb the pass: bit-identical to clair_submit_ex on the same input
    engine.submit_calls(1, batch, np.tile(np.array([[65, 33]], dtype=np.uint8), (n, 1)), counts=counts, with_probabilities=True)
    _, Y_ex = engine.wait(1)
    for a, b in zip(Y, Y_ex):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # evaluation mode proper: nothing but the counters comes back
    engine.eval_reset()
    engine.submit_eval(1, batch, lab, counts=counts)
    assert engine.wait(1) is None
    assert np.array_equal(engine.eval_read(), got)


def test_accumulation_over_slots_in_flight_reset_and_repeat(synth_weights):
    e = _capi.Engine(device=0, max_batch=512, n_slots=4)
    try:
        e.load_weights(synth_weights)
        sizes = (512, 100, 257, 64, 333, 512, 1, 480)
        X = [synth.synthetic_input(n, "ont", seed=900 + k)[0] for k, n in enumerate(sizes)]
        L = [_labels(n, 50 + k) for k, n in enumerate(sizes)]
        singles = []
        for x, lab in zip(X, L):
            e.eval_reset()
            e.submit_eval(0, x, lab)
            e.wait(0)
            singles.append(e.eval_read())
        assert [int(s[0]) for s in singles] == list(sizes)

        def run():
            e.eval_reset()
            inflight = []
            for k, (x, lab) in enumerate(zip(X, L)):
                if len(inflight) == 4:
                    e.wait(inflight.pop(0))
                e.submit_eval(k % 4, x, lab)
                inflight.append(k % 4)
            block = e.eval_read()                                  # waits for the slots' device work itself
            for s in inflight:
                e.wait(s)
            return block
        first = run()
        assert np.array_equal(first, sum(singles))
        assert np.array_equal(run(), first)                        # the same run twice: the same block
        e.eval_reset()
        assert not e.eval_read().any()
    finally:
        e.close()


def test_label_out_of_range_is_an_error_and_counts_nothing(engine):
    x, _ = synth.synthetic_input(8, "ont", seed=5)
    lab = _labels(8, 5)
    engine.eval_reset()
    engine.submit_eval(0, x, lab)
    engine.wait(0)
    before = engine.eval_read()
    for column, value in ((0, 21), (1, 3), (2, 33), (3, 255)):
        bad = lab.copy()
        bad[5, column] = value
        with pytest.raises(_capi.EngineError, match="out of range"):
            engine.submit_eval(0, x, bad)
        P = np.full((8, 90), 0.1, dtype=np.float32)
        with pytest.raises(_capi.EngineError, match="out of range"):
            engine.eval_probabilities([P[:, a:b] for a, b in SPLITS], bad)
    assert np.array_equal(engine.eval_read(), before)
    engine.submit_eval(0, x, lab)                                  # the slot is free and the engine still scores
    engine.wait(0)
    assert np.array_equal(engine.eval_read(), 2 * before)


@pytest.mark.parametrize("score_on", ["device", "host"])
def test_evaluate_command_prints_the_reference_report(tmp_path, synth_weights, score_on):
    chk = str(tmp_path / "model.npz")
    weights.save_weights(chk, synth_weights)
    r = subprocess.run([sys.executable, "-m", "clair_amd", "evaluate", "--chkpnt_fn", chk, "--tensor_fn", SMALL + ".txt.gz", "--var_fn", SMALL + ".var",
                        "--bed_fn", SMALL + ".bed", "--batch_size", "128", "--score_on", score_on], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr
    assert_same_report(r.stdout, json.load(open(SMALL + ".json"))["stdout"])
