"""Ensemble calling without a GPU: the `ensemble` submodule against the reference's own output (tests/golden/ensemble_small.json.gz,
tools/make_ensemble_golden.py), and the host twin of the device averaging (clair_host_ensemble_*, csrc/ensemble_core.h) against the
text path it restates -- printf and strtod, never the rule itself (tests/ensemble_cases.py)."""
import ctypes
import gzip
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ensemble_cases as cases
from clair_amd import _capi, _hostapi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("clair_ensemble_models", "clair_ensemble_set_tensor", "clair_ensemble_finalize_weights", "clair_submit_ensemble", "clair_ensemble_average")


@pytest.fixture(scope="module")
def golden():
    return json.loads(gzip.open(os.path.join(HERE, "golden", "ensemble_small.json.gz")).read().decode())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# -- 1. the submodule ----------------------------------------------------------------------------------------------------------------
def test_the_fixture_has_the_cases_it_is_there_for(golden):
    streams = [[r.split("\t") for r in s.splitlines()] for s in golden["inputs"]]
    keys = [[(c[0], c[1]) for c in rows] for rows in streams]
    assert len(streams) == 3 and len(set(keys[0])) == 40
    assert all([int(k[1]) for k in ks] != sorted(int(k[1]) for k in ks) for ks in keys)              # no stream is in position order
    count = {}
    for ks in keys:
        for k in ks:
            count[k] = count.get(k, 0) + 1
    assert {1, 2, 3, 4} <= set(count.values())                                                         # missing from two, from one, from none; one site twice
    first = {k: c for c in streams[0] for k in [(c[0], c[1])]}
    differs = [k for c in streams[1] for k in [(c[0], c[1])] if c[2:3 + 1056] != first[k][2:3 + 1056]]
    assert len(differs) == 1                                                                           # another tensor in the second input
    assert [len(golden["outputs"][t].splitlines()) for t in ("0", "2", "3")] == [40, 37, 30]


@pytest.mark.parametrize("threshold", [0, 2, 3])
def test_submodule_equals_the_reference_filter_byte_for_byte(golden, threshold):
    from clair_amd import ensemble
    out = io.StringIO()
    ensemble.main(["--minimum_count_to_output", str(threshold)], stdin=io.StringIO("".join(golden["inputs"])), stdout=out)
    assert out.getvalue() == golden["outputs"][str(threshold)]


# -- 3. the dispatcher ---------------------------------------------------------------------------------------------------------------
def test_dispatcher_runs_ensemble(golden):
    text = "".join(golden["inputs"])
    r = subprocess.run([sys.executable, "-m", "clair_amd", "ensemble", "--minimum_count_to_output", "2"], input=text, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden["outputs"]["2"]
    r = subprocess.run([sys.executable, "-m", "clair_amd", "ensemble"], input="", capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--minimum_count_to_output" in r.stdout           # the reference's no-argument help, status 1
    r = subprocess.run([sys.executable, "-m", "clair_amd"], capture_output=True, text=True, cwd=ROOT)
    assert "ensemble" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd", "overlap_variant"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "outside this build" in r.stderr


# -- 2. the host twin against the text path -----------------------------------------------------------------------------------------
def test_quantise_is_what_six_decimals_print():
    v = cases.float_values()
    assert len(v) >= 100000
    text = cases.text_of(v)
    sample = v[:: len(v) // 2000]
    assert ["{:0.6f}".format(s) for s in sample] == cases.text_of(sample)          # the writer's spelling, on float32 scalars
    want = np.array([int(t.replace(".", "")) for t in text], dtype=np.int64)
    got = _hostapi.ensemble_quantise(v)
    assert np.array_equal(got, want)
    ties = v[-72:-8]                                                               # the 64 exact half-way values: ties went to even
    assert np.array_equal(ties.astype(np.float64) * 1e6 % 1.0, np.full(64, 0.5)) and (_hostapi.ensemble_quantise(ties) % 2 == 0).all()


def test_value_is_the_float32_the_reader_holds():
    m = np.arange(cases.MILLION + 1, dtype=np.int32)
    want = np.array(["%d.%06d" % divmod(i, cases.MILLION) for i in m.tolist()], dtype=np.float32)      # clair/call_var.py:1291
    assert np.array_equal(bits(_hostapi.ensemble_value(m)), bits(want))


@pytest.mark.parametrize("models", [1, 2, 3, 4, 8])
def test_average_equals_the_text_round_trip(models):
    P = cases.crafted_rows(models, 50000)
    want = cases.text_average(P)
    got = _hostapi.ensemble_average(P)
    wrong = np.flatnonzero(bits(got) != bits(want))
    assert wrong.size == 0, "K=%d: %d of %d differ, first %r" % (models, wrong.size, P.shape[1], (P[:, wrong[0]].tolist(), float(got[wrong[0]]), float(want[wrong[0]])))
    if models % 2 == 0:
        k = np.rint(P.astype(np.float64) * 1e6).astype(np.int64).sum(axis=0)
        halfway = (k % models) == models // 2
        assert halfway.sum() >= P.shape[1] // 2
        # the set has teeth: the rounded product of the mean with 1e6 lands on the wrong side of many of these
        assert (cases.naive_average(P)[halfway] != want[halfway]).sum() > 1000
    if models == 1:
        assert not np.array_equal(_hostapi.ensemble_average(cases.float_values()[None]), cases.float_values())      # not the identity: six decimals


def test_average_shapes_and_arguments():
    P = cases.crafted_rows(3, 90 * 7).reshape(3, 7, 90)
    out = _hostapi.ensemble_average(P)
    assert out.shape == (7, 90) and np.array_equal(bits(out).ravel(), bits(cases.text_average(P.reshape(3, -1))))
    with pytest.raises(ValueError):
        _hostapi.ensemble_average(np.zeros((9, 4), np.float32))                    # at most 8 models


# -- 4. the surface ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_and_the_abi_stays():
    lib = _capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
    assert lib.clair_abi_version() == 6 and "#define CLAIR_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "clair_amd.h")).read()
    assert "CLAIR_K_COUNT = 8" in header                                           # no new kernel id
    host = _hostapi.load()
    host_header = open(os.path.join(ROOT, "include", "clair_host.h")).read()
    for name in ("clair_host_ensemble_average", "clair_host_ensemble_quantise", "clair_host_ensemble_value"):
        assert name in host_header and hasattr(host, name)
    assert host.clair_host_abi_version() == 6
    # without a device the new entry points fail like every other: loudly, on a NULL handle
    assert lib.clair_ensemble_models(None, 3) != 0 and b"NULL" in lib.clair_last_error(None)
    from clair_amd.build import csrc_digest
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:                                     # the averaging sources are part of what a build is stamped with
        for f in ("ensemble.hip.h", "ensemble_core.h"):
            open(os.path.join(tmp, f), "w").write("a")
        a = csrc_digest(tmp)
        open(os.path.join(tmp, "ensemble_core.h"), "w").write("b")
        assert csrc_digest(tmp) != a


def test_flags():
    from clair_amd import call_var, callVarBam, callVarBamParallel
    for mod in (call_var, callVarBam, callVarBamParallel):
        a = mod.build_parser().parse_args(["--chkpnt_fn", "A", "--ensemble_chkpnt_fn", "B", "--ensemble_chkpnt_fn", "C"])
        assert a.ensemble_chkpnt_fn == ["B", "C"]
        assert mod.build_parser().parse_args([]).ensemble_chkpnt_fn is None
    a = call_var.build_parser().parse_args(["--chkpnt_fn", "A", "--ensemble_chkpnt_fn", "B", "--output_for_ensemble"])
    with pytest.raises(SystemExit) as ei:
        call_var.check_ensemble_flags(a)
    assert "--output_for_ensemble" in str(ei.value)
    a = call_var.build_parser().parse_args(["--chkpnt_fn", "A", "--ensemble_chkpnt_fn", "B", "--input_probabilities"])
    with pytest.raises(SystemExit) as ei:
        call_var.check_ensemble_flags(a)
    assert "--input_probabilities" in str(ei.value)
    call_var.check_ensemble_flags(call_var.build_parser().parse_args(["--chkpnt_fn", "A", "--output_for_ensemble"]))       # without the flag: as ever


def test_callVarBamParallel_passes_the_flag_on_only_when_given(tmp_path):
    from clair_amd import callVarBamParallel as par
    for fn, text in (("ref.fa", ">x\n"), ("ref.fa.fai", "chr1\t1000\t3\t60\t61\n"), ("a.bam", ""), ("model.meta", "")):
        (tmp_path / fn).write_text(text)
    argv = ["--chkpnt_fn", str(tmp_path / "model"), "--ref_fn", str(tmp_path / "ref.fa"), "--bam_fn", str(tmp_path / "a.bam"),
            "--output_prefix", str(tmp_path / "out" / "var"), "--python", "PY"]
    plain = par.commands(par.build_parser().parse_args(argv))
    assert len(plain) == 1 and "ensemble_chkpnt_fn" not in plain[0]
    both = par.commands(par.build_parser().parse_args(argv + ["--ensemble_chkpnt_fn", str(tmp_path / "m2"), "--ensemble_chkpnt_fn", str(tmp_path / "m3")]))
    want = ' --ensemble_chkpnt_fn "%s" --ensemble_chkpnt_fn "%s" ' % (tmp_path / "m2", tmp_path / "m3")
    assert len(both) == 1 and want in both[0] and both[0].replace(want, " ") == plain[0]
    import shlex
    from clair_amd import callVarBam
    words = shlex.split(both[0])
    a = callVarBam.build_parser().parse_args(words[words.index("clair_amd.callVarBam") + 1:])
    assert a.ensemble_chkpnt_fn == [str(tmp_path / "m2"), str(tmp_path / "m3")]
