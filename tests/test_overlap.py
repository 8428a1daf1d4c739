"""The overlap filter (clair_amd/overlap_variant.py) against a fixture minted from the reference's own script
(tests/golden/overlap_small.json.gz, tools/make_overlap_golden.py), its host walk (clair_host_overlap_keep, csrc/overlap_core.h) against the
Python walk, and --overlap_filter on the callers.  The device walk is tests/test_overlap_gpu.py."""
import gzip
import io
import json
import os
import subprocess
import sys
from contextlib import redirect_stderr

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import overlap_cases  # noqa: E402
from clair_amd import _hostapi, overlap_variant as ov  # noqa: E402

GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(GOLD, "overlap_small.json.gz")) as f:
        g = json.load(f)
    assert len(g["inputs"]) == len(g["outputs"]) == 15
    return g


def _rows(text):
    return [r for r in text.splitlines() if not r.startswith("#")]


def test_the_fixture_holds_what_it_is_for(golden):
    """The first stream is this build's own VCF as committed; every other stream but two loses rows and keeps rows."""
    assert golden["inputs"][0] == open(os.path.join(GOLD, "e2e_230_default.vcf")).read()
    losing = [k for k, (i, o) in enumerate(zip(golden["inputs"], golden["outputs"])) if 0 < len(_rows(o)) < len(_rows(i))]
    assert len(losing) == 13
    assert any("\tLowQual\t" in i and "\tLowQual\t" not in o for i, o in zip(golden["inputs"], golden["outputs"]))
    assert any("\t12.9\t" in i and "\t12.9\t" not in o for i, o in zip(golden["inputs"], golden["outputs"]))


@pytest.mark.parametrize("backend", ["python", "host"])
def test_filter_reproduces_the_reference_byte_for_byte(golden, backend):
    for k, (text, want) in enumerate(zip(golden["inputs"], golden["outputs"])):
        assert ov.filter_vcf_text(text, backend) == want, "stream %d" % k


def test_the_module_as_a_process_reproduces_the_reference(golden):
    """python -m clair_amd.overlap_variant: stdin to stdout, no arguments needed (and no help printed for none)."""
    for k in (0, 6, 11):
        r = subprocess.run([sys.executable, "-m", "clair_amd.overlap_variant"], input=golden["inputs"][k], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == golden["outputs"][k], "stream %d" % k
    r = subprocess.run([sys.executable, "-m", "clair_amd.overlap_variant", "--backend", "host"], input=golden["inputs"][11], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout == golden["outputs"][11]


def test_main_takes_streams(golden):
    out = io.StringIO()
    ov.main([], stdin=io.StringIO(golden["inputs"][1]), stdout=out)
    assert out.getvalue() == golden["outputs"][1]
    with pytest.raises(ValueError):
        ov.filter_vcf_text(golden["inputs"][1], "cuda")


def test_host_walk_equals_the_python_walk():
    """clair_host_overlap_keep == overlap_variant.keep_mask on generated rows: sorted and shuffled runs, long deletions over dense rows, ties,
    duplicates, one to four contigs, n in {0, 1, 2, 3, 1000}."""
    dropped = chains = 0
    for name, rows in overlap_cases.generated():
        want = overlap_cases.python_mask(rows)
        got = _hostapi.overlap_keep(overlap_cases.spans(rows))
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        assert np.array_equal(got, want), "%s: first difference at row %d" % (name, int(np.flatnonzero(got != want)[0]))
        dropped += int((want == 0).sum())
        if len(rows) == 1000:
            zeros = np.flatnonzero(want == 0)
            chains += int((np.diff(zeros) == 1).sum())          # neighbours dropped together: more than an isolated pair
    assert dropped > 1000 and chains > 200                      # the generator bites


def test_span_record_layout():
    """The record the native walks read (csrc/overlap_core.h): 24 bytes, pos first."""
    assert _hostapi.SPAN_DTYPE.itemsize == 24
    assert [(_hostapi.SPAN_DTYPE.fields[k][1]) for k in ("pos", "ctg", "qual", "del", "flags")] == [0, 8, 12, 16, 20]
    s = ov.spans_from([ov.Variant("a", 7, "ACGT", "ACG", "A", 3, "1/2", "1", "0.1"), ov.Variant("b", 9, "AC", "ACTT", "GG", 4, "1/2", "1", "0.1"),
                       ov.Variant("a", 9, "A", "ATT", None, 5, "0/1", "1", "0.1")])
    assert s["ctg"].tolist() == [0, 1, 0] and s["del"].tolist() == [3, 0, -2] and s["flags"].tolist() == [0, 1, 0] and s["qual"].tolist() == [3, 4, 5]


def test_the_reach_of_a_deletion_does_not_wrap_near_2_to_31():
    """POS + the deletion's length is formed in 64 bits: a deletion that starts below 2^31 and ends above it covers the SNP there."""
    top = 2 ** 31
    rows = [ov.Variant("c", top - 2, "ACGTAC", "A", None, 50, "0/1", "30", "0.5"), ov.Variant("c", top + 1, "G", "T", None, 10, "0/1", "30", "0.5"),
            ov.Variant("c", top + 4, "G", "T", None, 10, "0/1", "30", "0.5"),
            ov.Variant("c", 2 * top - 3, "ACGTAC", "A", None, 50, "0/1", "30", "0.5"), ov.Variant("c", 2 * top + 2, "G", "T", None, 90, "0/1", "30", "0.5")]
    want = [1, 0, 1, 0, 1]
    assert overlap_cases.python_mask(rows).tolist() == want
    assert _hostapi.overlap_keep(ov.spans_from(rows)).tolist() == want
    text = "".join(ov.row_from(v) + "\n" for v in rows)
    assert ov.filter_vcf_text(text, "host") == ov.filter_vcf_text(text, "python") == "".join(ov.row_from(v) + "\n" for v, k in zip(rows, want) if k)


class _OracleClair(object):
    """What call_var.Run asks of clair_amd.model.Clair, answered by the float32 oracle on the CPU."""

    def __init__(self, device=0, max_batch=None, n_slots=None):
        from clair_amd import weights
        self.w = weights.synthetic_weights(seed=4242, head_gain=6.0, lstm_bias_scale=0.1)
        self.prediction = None

    def init(self):
        pass

    def restore_parameters(self, path):
        pass

    def close(self):
        pass

    def predict(self, batchX):
        from oracle import model_np
        self.prediction = model_np.forward(self.w, batchX)
        return self.prediction


def _call_var(tmp_path, monkeypatch, name, extra):
    from clair_amd import call_var, model
    monkeypatch.setattr(model, "Clair", _OracleClair)
    out = str(tmp_path / name)
    args = call_var.build_parser().parse_args(["--tensor_fn", os.path.join(GOLD, "e2e_230.txt.gz"), "--call_fn", out, "--chkpnt_fn", str(tmp_path / "none"),
                                               "--batch_size", "100", "--arith", "numpy2"] + extra)
    with redirect_stderr(io.StringIO()):
        call_var.Run(args)
    return open(out).read()


def test_call_var_overlap_filter_writes_the_filtered_file(tmp_path, monkeypatch, golden):
    """call_var --overlap_filter host writes exactly what the filter prints for the file written without the flag."""
    plain = _call_var(tmp_path, monkeypatch, "plain.vcf", [])
    assert plain == golden["inputs"][0]                         # the run is the one the fixture's first stream came from
    filtered = _call_var(tmp_path, monkeypatch, "filtered.vcf", ["--overlap_filter", "host"])
    assert filtered == ov.filter_vcf_text(plain, "python") == golden["outputs"][0]
    assert len(_rows(filtered)) < len(_rows(plain))
    assert _call_var(tmp_path, monkeypatch, "off.vcf", ["--overlap_filter", "off"]) == plain


def test_overlap_filter_with_output_for_ensemble_is_refused(tmp_path):
    from clair_amd import callVarBam, callVarBamParallel, call_var
    out = str(tmp_path / "o.txt")
    args = call_var.build_parser().parse_args(["--tensor_fn", os.path.join(GOLD, "e2e_230.txt.gz"), "--call_fn", out, "--overlap_filter", "host",
                                               "--output_for_ensemble"])
    with pytest.raises(SystemExit, match="--overlap_filter"):
        call_var.Run(args)
    assert not os.path.exists(out)
    fa = str(tmp_path / "r.fa")
    open(fa, "w").write(">c\nACGT\n")
    with pytest.raises(SystemExit, match="--overlap_filter"):
        callVarBam.normalise(callVarBam.build_parser().parse_args(["--bam_fn", fa, "--ref_fn", fa, "--ctgName", "c", "--call_fn", out,
                                                                    "--overlap_filter", "device", "--output_for_ensemble"]))
    with pytest.raises(SystemExit):
        call_var.build_parser().parse_args(["--overlap_filter", "python"])       # the callers offer the native walks only
    assert callVarBam.build_parser().parse_args([]).overlap_filter == "off"
    assert callVarBamParallel.build_parser().parse_args([]).overlap_filter is None


def test_callVarBamParallel_passes_the_flag_on(tmp_path):
    from clair_amd import callVarBamParallel as par
    tmp = str(tmp_path)
    for name, text in (("m.npz", ""), ("r.fa", ">c\nACGT\n"), ("r.fa.fai", "c\t4\t3\t4\t5\n"), ("a.bam", "")):
        open(os.path.join(tmp, name), "w").write(text)
    base = ["--chkpnt_fn", os.path.join(tmp, "m"), "--bam_fn", os.path.join(tmp, "a.bam"), "--ref_fn", os.path.join(tmp, "r.fa"), "--includingAllContigs",
            "--output_prefix", os.path.join(tmp, "var")]
    with_flag = par.commands(par.build_parser().parse_args(base + ["--overlap_filter", "device"]))
    without = par.commands(par.build_parser().parse_args(base))
    assert with_flag and all('--overlap_filter "device"' in c for c in with_flag)
    assert without and not any("overlap_filter" in c for c in without)
