"""Read subsampling on the host (docs/subsample.md): the rule of csrc/subsample_core.h through clair_host_subsample_keeps against the
anchor values and a restatement in Python integers (tests/subsample_cases.py), clair_host_bam_render with the rule on a BAM A against a BAM
B that holds exactly the records the restatement keeps, make_train_set --subsample on A against the plain run on B, load_sets over sets of
several depths, and the flag checks of callVarBam and make_train_set."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import subsample_cases as sc  # noqa: E402

from clair_amd import _hostapi  # noqa: E402
from clair_amd import make_train_set as mts  # noqa: E402

ULP = 2.0 ** -24           # the quotients are multiples of it


# -- 1. the rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,h,k,q", sc.ANCHORS, ids=lambda v: None)
def test_anchor_values(name, seed, h, k, q):
    assert (sc.name_hash(name), sc.mixed(h ^ seed), sc.quotient(name, seed)) == (h, k, q)      # the restatement the other tests lean on
    assert (k & 0xffffff) / 16777216.0 == q
    # dropped <=> q >= F: at F = q the record goes, one step above it stays
    assert not _hostapi.subsample_keeps(name, seed, q)
    assert _hostapi.subsample_keeps(name, seed, q + ULP)
    if q > 0:
        assert not _hostapi.subsample_keeps(name, seed, q - ULP)


def all_names():
    names = [b"read%d" % i for i in range(300)]
    names += [bytes([ord("a") + j]) * n for n in sc.NAME_LENGTHS for j in range(8)]
    return names + [a[0] for a in sc.ANCHORS] + [b"", b"caf\xc3\xa9", b"\xff\x80\x7f", b"q\xe9" * 40]


@pytest.mark.parametrize("frac,seed,kept", sc.KEPT_OF_300)
def test_host_rule_equals_the_restatement(frac, seed, kept):
    names = all_names()
    got = [_hostapi.subsample_keeps(n, seed, frac) for n in names]
    assert got == [sc.keeps(n, seed, frac) for n in names]
    assert sum(got[:300]) == kept


def test_a_byte_from_0x80_on_is_signed():
    assert sc.name_hash(b"\xff") == 0xffffffff and sc.name_hash(b"\x80a") == (-128 * 31 + 97) & sc.M32
    for name in (b"\xff", b"\x80a", b"ab\xfe"):
        unsigned = 0
        for c in name:
            unsigned = (unsigned * 31 + c) & sc.M32
        q_signed, q_unsigned = sc.quotient(name, 0), (sc.mixed(unsigned) & 0xffffff) / 16777216.0
        assert q_signed != q_unsigned
        lo, hi = sorted((q_signed, q_unsigned))
        assert _hostapi.subsample_keeps(name, 0, hi) == (q_signed == lo)      # a fraction between the two tells them apart


def test_the_name_ends_at_a_nul():
    for frac, seed, _ in sc.KEPT_OF_300:
        for i in range(40):
            assert _hostapi.subsample_keeps(b"read%d\0tail%d" % (i, i), seed, frac) == sc.keeps(b"read%d" % i, seed, frac)


def test_off_and_all():
    for name in all_names():
        for seed in (0, 11, 0xffffffff):
            assert _hostapi.subsample_keeps(name, seed, 0.0) and _hostapi.subsample_keeps(name, seed, -1.0)      # F <= 0: off
            assert _hostapi.subsample_keeps(name, seed, 1.0) and _hostapi.subsample_keeps(name, seed, 2.0)       # F >= 1: all
    with pytest.raises(ValueError):
        _hostapi.subsample_keeps(b"a", -1, 0.5)
    with pytest.raises(ValueError):
        _hostapi.subsample_keeps(b"a", 1 << 32, 0.5)


# -- 2. clair_host_bam_render ---------------------------------------------------------------------------------------------------------------
def rendered(path, ctg, region=None, subsample=None):
    r = _hostapi.BamReader(path, threads=2)
    if subsample is not None:
        r.set_subsample(*subsample)
    r.query(ctg, *(region or (None, None)))
    buf, off, out, n_rec = np.empty(1 << 22, np.uint8), np.empty(97, np.int64), b"", 0
    while True:
        _, k = r.readinto(buf, off)
        if not k:
            break
        out += r.render(buf, off, k)
        n_rec += k
    r.close()
    return out, n_rec


@pytest.mark.parametrize("frac,seed", [(0.5, 0), (0.5, 11), (0.1, 0), (0.8, 11)])
@pytest.mark.parametrize("region", [None, (700, 1900)], ids=["contig", "region"])
def test_render_of_a_with_the_rule_is_the_render_of_b(tmp_path, frac, seed, region):
    w = sc.world(tmp_path, seed=seed, frac=frac)
    n_a, n_b = sc.assert_a_real_subset(w["lines_a"], w["lines_b"], w["ctg"], region)
    plain, records_a = rendered(w["a"], w["ctg"], region)
    want, _ = rendered(w["b"], w["ctg"], region)
    got, records_with_rule = rendered(w["a"], w["ctg"], region, subsample=(seed, frac))
    assert got == want and len(want.splitlines()) == n_b and len(plain.splitlines()) == n_a
    assert records_with_rule == records_a                            # clair_host_bam_next frames records and does not filter
    # without set_subsample, and with the rule off again, the render is what it was
    assert plain == "".join(l + "\n" for l in w["lines_a"] if sc.viewable(l, w["ctg"], region)).encode()
    assert rendered(w["a"], w["ctg"], region, subsample=(seed, 0.0))[0] == plain
    assert rendered(w["a"], w["ctg"], region, subsample=(seed, 1.0))[0] == plain
    mates = [l.split("\t")[0] for l in want.decode().splitlines() if int(l.split("\t")[1]) & 1]
    assert mates and all(mates.count(m) == 2 for m in mates)         # mates share a name, so they share their fate


def test_render_over_the_name_lengths(tmp_path):
    w = sc.name_family(tmp_path)
    sc.assert_a_real_subset(w["lines_a"], w["lines_b"], w["ctg"])
    assert rendered(w["a"], w["ctg"], subsample=(0, 0.5))[0] == rendered(w["b"], w["ctg"])[0]


def test_set_subsample_checks_the_seed(tmp_path):
    w = sc.name_family(tmp_path)
    r = _hostapi.BamReader(w["a"], threads=1)
    for seed in (-1, 1 << 32):
        with pytest.raises(_hostapi.BamError) as ei:
            r.set_subsample(seed, 0.5)
        assert "4294967295" in str(ei.value)
    r.close()


# -- 3. make_train_set --front_end host -----------------------------------------------------------------------------------------------------
TRUTH = (100, 420, 435, 900, 1500, 2380, 2600)


def make_set(w, tmp, name, bam, *more):
    var = os.path.join(str(tmp), "truth.var")
    open(var, "w").write("".join("%s %d A C 0 1\n" % (w["ctg"], p) for p in TRUTH))
    out = [os.path.join(str(tmp), name + ".gz"), os.path.join(str(tmp), name + ".npz")]
    r = subprocess.run([sys.executable, "-m", "clair_amd.make_train_set", "--ref_fn", w["fa"], "--ctgName", w["ctg"], "--var_fn", var, "--samtools", "/nonexistent/samtools",
                        "--front_end", "host", "--bam_reader", "native", "--bam_fn", bam, "--outputProb", "0.05", "--amp", "6", "--minCoverage", "3",
                        "--tensor_fn", out[0], "--set_fn", out[1]] + list(more), capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return out


def members(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("subsample_sets")
    w = sc.world(tmp, seed=0, frac=0.5)
    sc.assert_a_real_subset(w["lines_a"], w["lines_b"], w["ctg"])
    return dict(w=w, tmp=tmp, virtual=make_set(w, tmp, "virtual", w["a"], "--subsample", "0.5"), physical=make_set(w, tmp, "physical", w["b"]),
                whole=make_set(w, tmp, "whole", w["a"]))


def test_make_train_set_on_a_with_the_flag_is_the_plain_run_on_b(sets):
    assert open(sets["virtual"][0], "rb").read() == open(sets["physical"][0], "rb").read()
    assert open(sets["virtual"][0], "rb").read() != open(sets["whole"][0], "rb").read()
    got, want = members(sets["virtual"][1]), members(sets["physical"][1])
    assert sorted(got) == sorted(want) and len(got["positions"]) > 10
    for name in want:
        if name != "meta":
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    meta, plain = json.loads(str(got["meta"])), json.loads(str(want["meta"]))
    assert meta.pop("subsample") == 0.5 and meta.pop("subsample_seed") == 0 and meta == plain      # the two new keys are the only difference


def test_without_the_flag_the_meta_has_no_new_key(sets):
    for path in (sets["physical"][1], sets["whole"][1]):
        meta = json.loads(str(members(path)["meta"]))
        assert sorted(meta) == sorted(("seed", "sampling", "p_near", "p_outside", "amp", "v", "c", "r", "n_near", "n_outside"))


def test_the_seed_reaches_the_reader_and_the_meta(sets):
    w, tmp = sets["w"], sets["tmp"]
    other = make_set(w, tmp, "seed11", w["a"], "--subsample", "0.5", "--subsample_seed", "11")
    meta = json.loads(str(members(other[1])["meta"]))
    assert (meta["subsample"], meta["subsample_seed"]) == (0.5, 11)
    assert open(other[0], "rb").read() != open(sets["virtual"][0], "rb").read()


def test_load_sets_keeps_a_site_once_per_depth(sets):
    whole, half = sets["whole"][1], sets["virtual"][1]
    xw, kw, yw = mts.load_sets([whole])
    xh, kh, yh = mts.load_sets([half])
    assert len(kw) > 10 and len(kh) > 10 and set(kw) & set(kh)                 # one seed samples the same sites where the depth allows
    x, keys, y = mts.load_sets([whole, half])
    assert keys == kw + kh and np.array_equal(x, np.concatenate([xw, xh])) and np.array_equal(y, np.concatenate([yw, yh]))
    assert all(":" in k and k.count(":") == 1 for k in keys)                   # the key strings stay ctg:pos
    # two copies of one set, of either kind, are one; the physical copy carries no tag, so it is another depth than the virtual one
    for path, n in ((whole, len(kw)), (half, len(kh))):
        assert len(mts.load_sets([path, path])[1]) == n
    assert len(mts.load_sets([whole, half, whole, half])[1]) == len(kw) + len(kh)


# -- 4. the flags ---------------------------------------------------------------------------------------------------------------------------
def bam_args(tmp_path, *more):
    from clair_amd import callVarBam
    for fn in ("a.bam", "b.bam", "ref.fa"):
        (tmp_path / fn).write_text("")
    argv = ["--chkpnt_fn", "M", "--bam_fn", str(tmp_path / "a.bam"), "--ref_fn", str(tmp_path / "ref.fa"), "--ctgName", "chr1", "--call_fn", str(tmp_path / "o.vcf")]
    return callVarBam.build_parser().parse_args(argv + list(more))


def exit_message(args):
    from clair_amd import callVarBam
    with pytest.raises(SystemExit) as ei:
        callVarBam.normalise(args)
    return str(ei.value)


NATIVE = ("--bam_reader", "native")


def test_flag_defaults_and_what_normalise_makes_of_them(tmp_path):
    from clair_amd import callVarBam
    a = callVarBam.normalise(bam_args(tmp_path))
    assert (a.subsample, a.subsample_seed, a.ensemble_subsample) == (None, 0, None) and callVarBam.site_sources(a) == []
    b = callVarBam.normalise(bam_args(tmp_path, "--subsample", "0.8", "--subsample_seed", "3", "--indel_lookup", "native", "--ensemble_bam_fn", str(tmp_path / "b.bam"),
                                      "--ensemble_subsample", "0.4", "--ensemble_subsample", "0.2:9", *NATIVE))
    assert callVarBam.subsample_of(b) == (0.8, 3)
    # --bam_fn first (call_sites puts it there), then the files whole, then the virtual BAMs; SEED defaults to --subsample_seed
    assert callVarBam.site_sources(b) == [(str(tmp_path / "b.bam"), None), (str(tmp_path / "a.bam"), (0.4, 3)), (str(tmp_path / "a.bam"), (0.2, 9))]
    # --ensemble_subsample alone makes an ensemble run and does not need --indel_lookup native: only BAM 0, read whole, is ever asked
    c = callVarBam.normalise(bam_args(tmp_path, "--ensemble_subsample", "0.5", "--minimum_count_to_output", "2", *NATIVE))
    assert callVarBam.site_sources(c) == [(str(tmp_path / "a.bam"), (0.5, 0))]


def test_the_flags_need_the_native_reader(tmp_path):
    for flags in (["--subsample", "0.5", "--indel_lookup", "native"], ["--subsample_seed", "4"], ["--ensemble_subsample", "0.5"]):
        msg = exit_message(bam_args(tmp_path, *flags))
        assert "--bam_reader native" in msg and "--samtools_view_args" in msg and "-s " in msg, flags


def test_subsample_does_not_go_with_the_pysam_look_up(tmp_path):
    msg = exit_message(bam_args(tmp_path, "--subsample", "0.5", *NATIVE))
    assert "--subsample" in msg and "--indel_lookup pysam" in msg and "--indel_lookup native" in msg and "whole file" in msg


def test_too_many_sources(tmp_path):
    from clair_amd import callVarBam
    files = [w for _ in range(4) for w in ("--ensemble_bam_fn", str(tmp_path / "b.bam"))]
    virtual = [w for k in range(1, 5) for w in ("--ensemble_subsample", "0.%d" % k)]
    callVarBam.normalise(bam_args(tmp_path, *(files + virtual[:6] + list(NATIVE))))                  # --bam_fn + 4 + 3 = 8
    msg = exit_message(bam_args(tmp_path, *(files + virtual + list(NATIVE))))
    assert "--ensemble_bam_fn" in msg and "--ensemble_subsample" in msg and "8 BAMs, at most 7" in msg


@pytest.mark.parametrize("flags,word", [
    (["--subsample", "0"], "0 < FRAC <= 1"), (["--subsample", "1.5"], "0 < FRAC <= 1"), (["--subsample", "-0.5"], "0 < FRAC <= 1"),
    (["--subsample", "nan"], "0 < FRAC <= 1"), (["--ensemble_subsample", "1.01"], "0 < FRAC <= 1"), (["--ensemble_subsample", "0:3"], "0 < FRAC <= 1"),
    (["--ensemble_subsample", "half"], "FRAC:SEED"), (["--ensemble_subsample", "0.5:x"], "FRAC:SEED"), (["--ensemble_subsample", "0.5:"], "FRAC:SEED"),
    (["--ensemble_subsample", "0.5:1:2"], "FRAC:SEED"), (["--ensemble_subsample", "0.5:-1"], "4294967295"), (["--subsample", "0.5", "--subsample_seed", "4294967296"], "4294967295")])
def test_fractions_and_seeds_out_of_range(tmp_path, flags, word):
    msg = exit_message(bam_args(tmp_path, "--indel_lookup", "native", *(flags + list(NATIVE))))
    assert word in msg and flags[0] in msg


def test_callVarBamParallel_passes_the_flags_on_only_when_given(tmp_path):
    import shlex
    from clair_amd import callVarBam
    from clair_amd import callVarBamParallel as par
    for fn, text in (("ref.fa", ">x\n"), ("ref.fa.fai", "chr1\t1000\t3\t60\t61\n"), ("a.bam", ""), ("model.meta", "")):
        (tmp_path / fn).write_text(text)
    argv = ["--chkpnt_fn", str(tmp_path / "model"), "--ref_fn", str(tmp_path / "ref.fa"), "--bam_fn", str(tmp_path / "a.bam"),
            "--output_prefix", str(tmp_path / "out" / "var"), "--python", "PY"]
    plain = par.commands(par.build_parser().parse_args(argv))
    assert len(plain) == 1 and "subsample" not in plain[0]
    given = par.commands(par.build_parser().parse_args(argv + ["--subsample", "0.8", "--subsample_seed", "5", "--ensemble_subsample", "0.4", "--ensemble_subsample", "0.2:7"]))
    want = ' --subsample "0.8" --subsample_seed "5" --ensemble_subsample "0.4" --ensemble_subsample "0.2:7" '
    assert len(given) == 1 and want in given[0] and given[0].replace(want, " ") == plain[0]
    words = shlex.split(given[0])
    a = callVarBam.build_parser().parse_args(words[words.index("clair_amd.callVarBam") + 1:])
    assert (a.subsample, a.subsample_seed, a.ensemble_subsample) == (0.8, 5, ["0.4", "0.2:7"])


def test_make_train_set_flag_checks(sets):
    w, tmp = sets["w"], sets["tmp"]
    base = [sys.executable, "-m", "clair_amd.make_train_set", "--ref_fn", w["fa"], "--ctgName", w["ctg"], "--var_fn", os.path.join(str(tmp), "truth.var"),
            "--bam_fn", w["a"], "--front_end", "host", "--set_fn", os.path.join(str(tmp), "never.npz")]
    for more, word in ((["--subsample", "0.5"], "--bam_reader native"), (["--subsample", "1.5", "--bam_reader", "native"], "0 < FRAC <= 1"),
                       (["--subsample", "0", "--bam_reader", "native"], "0 < FRAC <= 1")):
        r = subprocess.run(base + more, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and word in r.stderr, more
    assert not os.path.exists(os.path.join(str(tmp), "never.npz"))
