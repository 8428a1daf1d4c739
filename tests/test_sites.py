"""Ensemble across BAMs, CPU side: the host twin of the site table (clair_host_sites_*) against the text filter, the edge shapes of its merge, its
errors, and the command-line rules of callVarBam --ensemble_bam_fn.  tests/test_sites_gpu.py holds the device table to this twin."""
import math

import numpy as np
import pytest

import sites_cases as cases
from clair_amd import _hostapi


def filled(sources, **kw):
    t = _hostapi.HostSiteTable()
    cases.fill(t, sources, **kw)
    return t


# -- 1. the twin against the text path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("models", [1, 2, 3, 8])
@pytest.mark.parametrize("n_sources", [1, 2, 3, 8])
def test_twin_equals_the_text_filter(n_sources, models):
    sources, expected = cases.crafted_sources(n_sources, models)
    text = cases.ensemble_rows_text(sources)
    t = filled(sources)
    runs = n_sources * models
    for minimum in (0, 1, math.ceil(runs / 2), runs, runs + 1):
        positions, seq, x, rows = cases.text_filter(text, minimum)
        got = cases.snapshot(t, minimum, "chain")
        assert np.array_equal(got[0], positions), "sites or their order differ at N=%d" % minimum
        assert got[1].tolist() == [expected[p] for p in positions.tolist()]
        assert np.array_equal(got[2], seq)
        assert np.array_equal(cases.bits(got[3]), cases.bits(x))
        assert np.array_equal(cases.bits(got[4]), cases.bits(rows)), "averaged rows differ at N=%d" % minimum
        if minimum == runs + 1:
            assert len(positions) == 0


def test_the_cases_cover_the_counts_they_are_there_for():
    seen = set()
    for n_sources in (1, 2, 3, 8):
        for models in (1, 2, 3, 8):
            seen.update(cases.crafted_sources(n_sources, models)[1].values())
    assert {1, 2, 3, 4, 6, 8, 9, 16, 24, 64} <= seen


def test_half_of_the_crafted_means_are_exact_half_way_points():
    sources, expected = cases.crafted_sources(2, 2)
    both = sorted(set(sources[0].positions.tolist()) & set(sources[1].positions.tolist()))
    assert both
    p = both[0]
    rows = [s.probs[:, s.positions.tolist().index(p), :] for s in sources]
    k = np.rint(np.concatenate(rows).astype(np.float64) * 1e6).astype(np.int64).sum(axis=0)
    assert expected[p] == 4 and (k[:45] % 4 == 2).all()


# -- 2. edge shapes of the merge -----------------------------------------------------------------------------------------------------------
def chain_order(sources):
    seen = []
    for s in sources:
        seen.extend(p for p in s.positions.tolist() if p not in seen)
    return seen


@pytest.mark.parametrize("name,lists", cases.MERGE_SHAPES)
def test_merge_shapes(name, lists):
    sources = [cases.one_source(p, value=0.125 * (b + 1)) for b, p in enumerate(lists)]
    t = filled(sources)
    want = chain_order(sources)
    positions, counts, seq, x, rows = cases.snapshot(t, 0, "chain")
    assert positions.tolist() == want
    assert counts.tolist() == [sum(p in s.positions.tolist() for s in sources) for p in want]
    first = {p: next(b for b, s in enumerate(sources) if p in s.positions.tolist()) for p in want}
    for i, p in enumerate(want):        # window and seq of the first source that has the site
        s = sources[first[p]]
        at = s.positions.tolist().index(p)
        assert np.array_equal(seq[i], s.seq[at]) and np.array_equal(x[i], s.x[at])
    by_position = cases.snapshot(t, 0, "position")
    order = np.argsort(positions, kind="stable")
    for a, b in zip(by_position, (positions, counts, seq, x, rows)):
        assert np.array_equal(cases.bits(a), cases.bits(b[order]))
    assert cases.snapshot(t, len(sources) + 1, "chain")[0].tolist() == []      # N that drops everything
    assert t.rows(0, 0).shape == (0, 90)


def test_position_order_is_a_stable_sort_of_chain_order():
    sources, _ = cases.crafted_sources(3, 2)
    t = filled(sources)
    for minimum in (0, 4):
        chain = cases.snapshot(t, minimum, "chain")
        order = np.argsort(chain[0], kind="stable")
        assert not np.array_equal(order, np.arange(len(order)))
        for a, b in zip(cases.snapshot(t, minimum, "position"), chain):
            assert np.array_equal(cases.bits(a), cases.bits(b[order]))


def test_a_row_begun_but_never_fed_is_no_site():
    t = _hostapi.HostSiteTable()
    t.begin_source(np.array([3, 4], dtype=np.int64))
    t.add_rows(1, np.full((1, 90), 0.5, dtype=np.float32))
    assert cases.snapshot(t, 0)[0].tolist() == [4]


def test_rows_in_pieces_give_the_same_table():
    sources, _ = cases.crafted_sources(3, 3)
    whole, pieces = cases.snapshot(filled(sources), 0), cases.snapshot(filled(sources, piece=2), 0)
    for a, b in zip(whole, pieces):
        assert np.array_equal(cases.bits(a), cases.bits(b))


def test_errors():
    cases.check_errors(_hostapi.HostSiteTable)


def test_sixty_four_rows_are_fine():
    t = _hostapi.HostSiteTable()
    t.begin_source(np.array([5], dtype=np.int64))
    for _ in range(64):
        t.add_rows(0, np.full((1, 90), 0.5, dtype=np.float32))
    positions, counts, _, _, rows = cases.snapshot(t, 64)
    assert counts.tolist() == [64] and (rows == np.float32(0.5)).all()


# -- 3. the command line -------------------------------------------------------------------------------------------------------------------
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


def test_flag_defaults_and_a_plain_run_is_untouched(tmp_path):
    from clair_amd import callVarBam
    a = bam_args(tmp_path)
    assert (a.ensemble_bam_fn, a.minimum_count_to_output, a.ensemble_order) == (None, 0, "chain")
    callVarBam.normalise(a)
    b = bam_args(tmp_path, "--ensemble_bam_fn", str(tmp_path / "b.bam"), "--ensemble_bam_fn", str(tmp_path / "a.bam"), "--minimum_count_to_output", "3",
                 "--ensemble_order", "position", "--overlap_filter", "device")
    callVarBam.normalise(b)
    assert b.ensemble_bam_fn == [str(tmp_path / "b.bam"), str(tmp_path / "a.bam")] and b.minimum_count_to_output == 3


def test_minimum_count_needs_ensemble_bams(tmp_path):
    msg = exit_message(bam_args(tmp_path, "--minimum_count_to_output", "2"))
    assert "--minimum_count_to_output" in msg and "--ensemble_bam_fn" in msg


def test_ensemble_bams_do_not_go_with_output_for_ensemble(tmp_path):
    msg = exit_message(bam_args(tmp_path, "--ensemble_bam_fn", str(tmp_path / "b.bam"), "--output_for_ensemble"))
    assert "--ensemble_bam_fn" in msg and "--output_for_ensemble" in msg and "use one of the two" in msg


def test_overlap_filter_needs_position_order(tmp_path):
    msg = exit_message(bam_args(tmp_path, "--ensemble_bam_fn", str(tmp_path / "b.bam"), "--overlap_filter", "host"))
    assert "--overlap_filter" in msg and "--ensemble_order position" in msg


def test_at_most_seven_ensemble_bams(tmp_path):
    seven = [w for _ in range(7) for w in ("--ensemble_bam_fn", str(tmp_path / "b.bam"))]
    from clair_amd import callVarBam
    callVarBam.normalise(bam_args(tmp_path, *seven))
    msg = exit_message(bam_args(tmp_path, *(seven + ["--ensemble_bam_fn", str(tmp_path / "b.bam")])))
    assert "8 BAMs, at most 7" in msg


def test_ensemble_bams_do_not_go_with_front_end_workers(tmp_path):
    msg = exit_message(bam_args(tmp_path, "--ensemble_bam_fn", str(tmp_path / "b.bam"), "--front_end_workers", "2"))
    assert "--ensemble_bam_fn" in msg and "--front_end_workers" in msg


def test_a_missing_ensemble_bam_is_reported(tmp_path):
    assert "nowhere.bam not found" in exit_message(bam_args(tmp_path, "--ensemble_bam_fn", str(tmp_path / "nowhere.bam")))


def test_callVarBamParallel_passes_the_flags_on_only_when_given(tmp_path):
    import shlex
    from clair_amd import callVarBam
    from clair_amd import callVarBamParallel as par
    for fn, text in (("ref.fa", ">x\n"), ("ref.fa.fai", "chr1\t1000\t3\t60\t61\n"), ("a.bam", ""), ("b.bam", ""), ("c.bam", ""), ("model.meta", "")):
        (tmp_path / fn).write_text(text)
    argv = ["--chkpnt_fn", str(tmp_path / "model"), "--ref_fn", str(tmp_path / "ref.fa"), "--bam_fn", str(tmp_path / "a.bam"),
            "--output_prefix", str(tmp_path / "out" / "var"), "--python", "PY"]
    plain = par.commands(par.build_parser().parse_args(argv))
    assert len(plain) == 1
    for word in ("ensemble_bam_fn", "minimum_count_to_output", "ensemble_order"):
        assert word not in plain[0]
    given = par.commands(par.build_parser().parse_args(argv + ["--ensemble_bam_fn", str(tmp_path / "b.bam"), "--ensemble_bam_fn", str(tmp_path / "c.bam"),
                                                               "--minimum_count_to_output", "2", "--ensemble_order", "position"]))
    want = ' --ensemble_bam_fn "%s" --ensemble_bam_fn "%s" --minimum_count_to_output "2" --ensemble_order "position" ' % (tmp_path / "b.bam", tmp_path / "c.bam")
    assert len(given) == 1 and want in given[0] and given[0].replace(want, " ") == plain[0]
    words = shlex.split(given[0])
    a = callVarBam.build_parser().parse_args(words[words.index("clair_amd.callVarBam") + 1:])
    assert a.ensemble_bam_fn == [str(tmp_path / "b.bam"), str(tmp_path / "c.bam")] and a.minimum_count_to_output == 2 and a.ensemble_order == "position"


def test_new_symbols_are_declared_and_the_abi_stays():
    from clair_amd import _capi
    for name in ("clair_sites_create", "clair_sites_begin_source", "clair_submit_sites", "clair_sites_add_rows", "clair_sites_finish", "clair_sites_info",
                 "clair_sites_rows", "clair_submit_site_calls"):
        assert name in _capi.SIGNATURES and hasattr(_capi.load(), name)
        assert name.replace("clair_", "clair_host_") in _hostapi.SIGNATURES or name.startswith("clair_submit")
    assert _capi.load().clair_abi_version() == 6 and _hostapi.load().clair_host_abi_version() == 6
