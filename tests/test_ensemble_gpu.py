"""Ensemble calling on the MI355X: the averaging kernel against its host twin on crafted rows, clair_submit_ensemble against three
single-model engines averaged by that twin, and the two command lines against the text chain they replace (docs/ensemble.md)."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))
SEEDS = (20250928, 515, 9001)
SIZES = (1, 33, 64, 65, 1024)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def packed(Y):
    return np.concatenate([np.asarray(a, dtype=np.float32) for a in Y], axis=1)


@pytest.fixture(scope="module")
def model_weights():
    from clair_amd import weights
    return [weights.synthetic_weights(seed=s, head_gain=4.0) for s in SEEDS]


@pytest.fixture(scope="module")
def ens_engine(model_weights):
    """One handle with the three checkpoints (the session's `engine` fixture has one)."""
    from clair_amd import _capi
    e = _capi.Engine(device=0, max_batch=1024, n_slots=2)
    e.load_ensemble(model_weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    from clair_amd import _hostapi, synth
    raw, infos = synth.synthetic_candidates(1024, "ont", seed=31)
    return {"x": synth.to_model_input(raw), "counts": raw.astype(np.int16), "centre": _hostapi.centre_bytes(infos)}


@pytest.fixture(scope="module")
def single_model_results(model_weights, batch):
    """{n: [Y of model 0, Y of model 1, Y of model 2]}: plain submit_calls(..., with_probabilities=True), one single-model engine per
    checkpoint, computed once."""
    from clair_amd import _capi
    out = {n: [] for n in SIZES}
    for w in model_weights:
        e = _capi.Engine(device=0, max_batch=1024, n_slots=1)
        try:
            e.load_weights(w)
            for n in SIZES:
                e.submit_calls(0, batch["x"][:n], batch["centre"][:n], with_probabilities=True)
                out[n].append(e.wait(0)[1])
        finally:
            e.close()
    return out


# -- 1. the kernel alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("models", [1, 2, 3, 8])
def test_device_average_equals_the_host_twin_on_crafted_rows(ens_engine, models):
    import ensemble_cases as cases
    from clair_amd import _hostapi
    rows = cases.crafted_rows(models, 1000 * 90).reshape(models, 1000, 90)       # the rows of tests/test_ensemble.py, half of them exact half-way means
    for n in (1, 63, 64, 65, 1000):
        P = np.ascontiguousarray(rows[:, 1000 - n:])
        want = _hostapi.ensemble_average(P)
        for slot in (0, 1):
            got = ens_engine.ensemble_average(P, slot=slot)
            assert got.shape == (n, 90) and np.array_equal(bits(got), bits(want)), (models, n, slot)
    assert np.array_equal(bits(want[:50]), bits(cases.text_average(P[:, :50].reshape(models, -1)).reshape(50, 90)))       # and the twin is the text path's


# -- 2. K forward passes and the average behind one submit ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float32", "counts"])
@pytest.mark.parametrize("n", SIZES)
def test_submit_ensemble_equals_three_engines_averaged_by_the_twin(ens_engine, batch, single_model_results, n, kind):
    from clair_amd import _capi, _hostapi
    e = ens_engine
    singles = single_model_results[n]
    want = _hostapi.ensemble_average(np.stack([packed(Y) for Y in singles]))
    want_Y = _capi.split_outputs(want)
    want_calls = _hostapi.resolve_calls(batch["x"][:n], want_Y, batch["centre"][:n])
    source = batch["counts"][:n] if kind == "counts" else batch["x"][:n]
    runs = []
    for slot in (0, 1):                                                           # twice, once per slot: the same bits
        e.submit_ensemble(slot, source, batch["centre"][:n], counts=kind == "counts", with_probabilities=True)
        runs.append(e.wait(slot))
    for calls, Y in runs:
        assert np.array_equal(bits(packed(Y)), bits(want))
        assert calls.tobytes() == want_calls.tobytes()
    assert (bits(want) != bits(packed(singles[0]))).any()                         # an average, not model 0
    # without call records: the averaged probabilities alone
    e.submit_ensemble(0, source, None, counts=kind == "counts")
    assert np.array_equal(bits(packed(e.wait(0))), bits(want))
    # call records alone
    e.submit_ensemble(1, source, batch["centre"][:n], counts=kind == "counts")
    assert e.wait(1).tobytes() == want_calls.tobytes()
    # a handle that loaded an ensemble still gives today's bits through the plain submit
    e.submit_calls(0, source, batch["centre"][:n], counts=kind == "counts", with_probabilities=True)
    calls0, Y0 = e.wait(0)
    assert np.array_equal(bits(packed(Y0)), bits(packed(singles[0])))
    assert calls0.tobytes() == _hostapi.resolve_calls(batch["x"][:n], singles[0], batch["centre"][:n]).tobytes()


def test_errors(ens_engine, batch, model_weights, monkeypatch):
    from clair_amd import _capi
    with pytest.raises(_capi.EngineError):
        ens_engine.ensemble_average(np.zeros((9, 4, 90), np.float32))             # at most 8 models
    with pytest.raises(ValueError):
        ens_engine.load_ensemble([model_weights[0]] * 9)
    plain = _capi.Engine(device=0, max_batch=64, n_slots=1)
    try:
        plain.load_weights(model_weights[0])
        plain._check(plain._lib.clair_ensemble_models(plain._h, 2), "clair_ensemble_models")
        with pytest.raises(_capi.EngineError) as ei:                              # image 1 was never loaded
            plain.submit_ensemble(0, batch["x"][:8], batch["centre"][:8])
        assert "model 1" in str(ei.value)
    finally:
        plain.close()
    monkeypatch.setenv("CLAIR_AMD_LSTM2_FUSED", "1")                              # not on a handle that opted into the fused layer-2 launch
    fused = _capi.Engine(device=0, max_batch=64, n_slots=1)
    try:
        with pytest.raises(_capi.EngineError) as ei:
            fused.load_ensemble(model_weights[:2])
        assert "CLAIR_AMD_LSTM2_FUSED" in str(ei.value)
        with pytest.raises(_capi.EngineError):
            fused.ensemble_average(np.zeros((2, 4, 90), np.float32))
    finally:
        fused.close()


# -- 3. call_var: the flag against the chain it replaces -------------------------------------------------------------------------------
def _checkpoints(tmp):
    from clair_amd import weights
    return [weights.save_weights(os.path.join(tmp, "model%d" % k), weights.synthetic_weights(seed=s, head_gain=6.0, lstm_bias_scale=0.1))[:-4]
            for k, s in enumerate((4242, 4343, 4444))]


def test_call_var_flag_writes_the_vcf_of_the_text_chain(tmp_path, monkeypatch):
    from clair_amd import call_var, ensemble
    tmp = str(tmp_path)
    cks = _checkpoints(tmp)
    tensors = os.path.join(HERE, "golden", "e2e_230.txt.gz")
    common = ["--tensor_fn", tensors, "--batch_size", "128", "--sampleName", "S"]

    def run(argv):
        call_var.Run(call_var.build_parser().parse_args(argv))

    one = os.path.join(tmp, "one.vcf")
    run(["--chkpnt_fn", cks[0], "--ensemble_chkpnt_fn", cks[1], "--ensemble_chkpnt_fn", cks[2], "--call_fn", one, "--showRef"] + common)
    rows = []
    for k, ck in enumerate(cks):                                                  # the chain, with this build's own commands
        out = os.path.join(tmp, "probs%d.txt" % k)
        run(["--chkpnt_fn", ck, "--call_fn", out, "--output_for_ensemble"] + common)
        rows.append(open(out).read())
    averaged = io.StringIO()
    ensemble.main(["--minimum_count_to_output", "3"], stdin=io.StringIO("".join(rows)), stdout=averaged)
    chain = os.path.join(tmp, "chain.vcf")
    monkeypatch.setattr(sys, "stdin", io.StringIO(averaged.getvalue()))
    run(["--input_probabilities", "--call_fn", chain, "--showRef", "--sampleName", "S"])
    got, want = open(one).read(), open(chain).read()
    assert got == want
    assert len([ln for ln in want.splitlines() if not ln.startswith("#")]) > 200
    single = os.path.join(tmp, "single.vcf")
    run(["--chkpnt_fn", cks[0], "--call_fn", single, "--showRef"] + common)
    assert open(single).read() != want                                            # the other two checkpoints had their say
    # a host decode (a float --qual is outside the native decoders) goes on from the averaged probabilities
    args = call_var.build_parser().parse_args(["--chkpnt_fn", cks[0], "--ensemble_chkpnt_fn", cks[1], "--ensemble_chkpnt_fn", cks[2],
                                               "--call_fn", os.path.join(tmp, "host.vcf"), "--showRef"] + common)
    args.qual = 0.0
    call_var.Run(args)
    strip = lambda text: [ln.split("\t")[:6] + ln.split("\t")[7:] for ln in text.splitlines() if not ln.startswith("#")]     # noqa: E731  (FILTER differs: "." vs PASS)
    assert strip(open(os.path.join(tmp, "host.vcf")).read()) == strip(want)


# -- 4. callVarBam: the lean device path (windows never leave HBM) against the host front end ------------------------------------------------
def test_callVarBam_native_with_the_flag_lean_equals_host_front_end(tmp_path):
    import bam_fixture as bf
    import pileup_synth
    from clair_amd import callVarBam
    tmp = str(tmp_path)
    case = pileup_synth.synth_case(seed=91, dup_burst=4)
    fa = os.path.join(tmp, "ref.fa")
    seq = "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:])
    text, fai = bf.fasta_of({case["ctg"]: seq, "chrOther": "ACGT" * 30})
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    bam_fn = os.path.join(tmp, "reads.bam")
    bf.Bam(case["sam"], [(case["ctg"], case["ref_len"]), ("chrOther", 120)]).write(bam_fn, block=5000, index=True)
    cks = _checkpoints(tmp)
    base = ["--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--ref_fn", fa, "--ctgName", case["ctg"], "--bam_fn", bam_fn,
            "--samtools", "/nonexistent/samtools", "--bam_reader", "native", "--chkpnt_fn", cks[0]]
    flag = ["--ensemble_chkpnt_fn", cks[1], "--ensemble_chkpnt_fn", cks[2]]
    out = {}
    for name, extra in (("lean", flag + ["--front_end", "device"]), ("host", flag + ["--front_end", "host"]), ("single", ["--front_end", "device"])):
        out[name] = os.path.join(tmp, name + ".vcf")
        callVarBam.main(base + extra + ["--call_fn", out[name]])
    lean = open(out["lean"]).read()
    assert lean == open(out["host"]).read()
    assert len([ln for ln in lean.splitlines() if not ln.startswith("#")]) > 15
    assert lean != open(out["single"]).read()
