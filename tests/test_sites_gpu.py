"""Ensemble across BAMs on the MI355X: the device site table against its host twin on crafted rows and at the scan's size boundaries,
clair_submit_sites + clair_sites_finish + clair_submit_site_calls against single-model engines accumulated by that twin and decoded by the
existing decode, and callVarBam --ensemble_bam_fn against the text chain it replaces (docs/ensemble.md)."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sites_cases as cases  # noqa: E402

SEEDS = (20250928, 515, 9001)
BATCH = 64
SCAN_BLOCK = 256           # items the table's scan takes per step (csrc/sites.hip.h: one workgroup, 256 at a time -- not hierarchical)


def same(a, b):
    return all(np.array_equal(cases.bits(x), cases.bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def model_weights():
    from clair_amd import weights
    return [weights.synthetic_weights(seed=s, head_gain=4.0) for s in SEEDS]


@pytest.fixture(scope="module")
def table_engine():
    """A handle without weights: the table's own entry points need none."""
    from clair_amd import _capi
    e = _capi.Engine(device=0, max_batch=512, n_slots=2)
    yield e
    e.close()


# -- 4. the device table equals the twin ----------------------------------------------------------------------------------------------------
def both_tables(engine, sources, **kw):
    from clair_amd import _hostapi
    host, dev = _hostapi.HostSiteTable(), engine.site_table()
    cases.fill(host, sources, **kw)
    cases.fill(dev, sources, **kw)
    return host, dev


@pytest.mark.parametrize("n_sources,models", [(1, 1), (2, 2), (3, 3), (3, 8), (8, 2), (8, 8)])
def test_device_table_equals_the_twin_on_crafted_sources(table_engine, n_sources, models):
    sources, expected = cases.crafted_sources(n_sources, models)
    host, dev = both_tables(table_engine, sources)
    runs = n_sources * models
    for order in ("chain", "position"):
        for minimum in (0, (runs + 1) // 2, runs, runs + 1):
            want, got = cases.snapshot(host, minimum, order), cases.snapshot(dev, minimum, order)
            assert same(got, want), (order, minimum)
    positions, counts, seq, x, rows = cases.snapshot(dev, 0)
    assert counts.tolist() == [expected[p] for p in cases.snapshot(host, 0)[0].tolist()]
    # the decode of the output list on this handle, which has no weights: the existing decode on the same rows and windows
    from clair_amd import _capi
    n = min(len(positions), 64)
    centre = np.stack([seq[:n, 16], np.full(n, 33, np.uint8)], axis=1)
    want_calls = table_engine.decode(x[:n], _capi.split_outputs(rows[:n]), centre, slot=1)
    table_engine.submit_site_calls(0, dev, 0, n)
    assert table_engine.wait(0).tobytes() == want_calls.tobytes()
    dev.close()


@pytest.mark.parametrize("first_size", [0, 1, 64, 65])
def test_device_table_at_the_scan_boundaries(table_engine, first_size):
    """later sources one below, on and above the scan's step (the smallest multi-step size: the scan is one workgroup walking 256 at a time)"""
    sources = cases.sized_sources([first_size, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 3], seed=9 + first_size)
    host, dev = both_tables(table_engine, sources, piece=200)
    for order in ("chain", "position"):
        for minimum in (0, 2, 5):
            assert same(cases.snapshot(dev, minimum, order), cases.snapshot(host, minimum, order)), (order, minimum)
    n = dev.finish(0, "position")
    assert host.finish(0, "position") == n > 2 * SCAN_BLOCK and (np.diff(dev.info(0, n)[0]) > 0).all()
    assert same([dev.rows(n - 5, 5), dev.windows(n - 5, 5)], [host.rows(n - 5, 5), host.windows(n - 5, 5)])       # a range that is not the whole list
    dev.close()


def test_device_table_without_windows_and_merge_edges(table_engine):
    for name, lists in cases.MERGE_SHAPES:
        sources = [cases.one_source(p, value=0.125 * (b + 1)) for b, p in enumerate(lists)]
        host, dev = both_tables(table_engine, sources, with_windows=False)
        for order in ("chain", "position"):
            want, got = cases.snapshot(host, 0, order), cases.snapshot(dev, 0, order)
            assert same(got, want), (name, order)                  # windows and seqs nobody brought are zeros on both sides
        assert dev.finish(len(lists) + 1, "chain") == 0 and dev.rows(0, 0).shape == (0, 90)
        dev.close()


def test_device_table_errors(table_engine, monkeypatch):
    from clair_amd import _capi
    cases.check_errors(table_engine.site_table)
    t = table_engine.site_table()                                      # 64 rows are fine, and finish reports the 65th too
    t.begin_source(np.array([5], dtype=np.int64))
    for _ in range(64):
        t.add_rows(0, np.full((1, 90), 0.5, dtype=np.float32))
    assert t.finish(64, "chain") == 1 and t.info(0, 1)[1].tolist() == [64] and (t.rows(0, 1) == np.float32(0.5)).all()
    t.close()
    other = _capi.Engine(device=0, max_batch=16, n_slots=1)
    try:
        t = other.site_table()
        t.begin_source(np.array([5], dtype=np.int64))
        with pytest.raises(_capi.EngineError) as ei:                   # a table of another engine
            table_engine.submit_site_calls(0, t, 0, 1)
        assert "another engine" in str(ei.value)
    finally:
        other.close()
    monkeypatch.setenv("CLAIR_AMD_LSTM2_FUSED", "1")                   # not on a handle that opted into the fused layer-2 launch
    fused = _capi.Engine(device=0, max_batch=64, n_slots=1)
    try:
        with pytest.raises(_capi.EngineError) as ei:
            fused.site_table()
        assert "CLAIR_AMD_LSTM2_FUSED" in str(ei.value)
    finally:
        fused.close()


# -- 5. forward passes into the table, finish, decode ---------------------------------------------------------------------------------------
SIZE_CASES = [(1, 64, 130), (63, 65, 64), (130, 1, 63), (65, 130, 65)]          # every size of {1, 63, 64, 65, 130} as a first and as a later source


@pytest.fixture(scope="module")
def windows():
    """Windows in device memory (a Frontend) and their host copies: what the three input forms are cut from."""
    import frontend_cases as fc
    from clair_amd import _capi, _hostapi
    case = fc.synth(55, n_reads=1200, ref_len=9000, read_len=(100, 1200))
    f = _capi.Frontend(0, case["ref"], case["ref0"], case["ref0"] - 64, case["ref0"] + len(case["ref"]) + 64)
    p = _hostapi.SamPacker(case["ctg"])
    assert p.feed(case["sam"], final=True) == b""
    f.add_slab(p)
    f.find_candidates(min_coverage=4, threshold=0.125)
    n = f.build_windows(drop_non_iupac_centre=True)
    assert n > 330
    _, seqs = f.window_info(0, n)
    counts = f.window_counts(0, n)
    yield {"frontend": f, "n": n, "seq": seqs, "counts": counts, "x": _hostapi.counts_to_input(counts.astype(np.int32)),
           "centre": np.stack([seqs[:, 16], (seqs[:, :33] != 0).sum(axis=1).astype(np.uint8)], axis=1)}
    f.close()


def sources_of(sizes):
    """[(first window, site labels)] per source: source b is windows [w, w + n) of the pool, labelled with sites that overlap the other
    sources' -- so the same site comes with ANOTHER window from each source, and the first one has to win."""
    labels = 5000 + 7 * np.arange(400, dtype=np.int64)
    starts = (0, 40, 100)          # first label of each source: overlapping ranges
    firsts = (0, 150, 60)          # first window of each source
    return [(firsts[b], labels[starts[b]:starts[b] + n]) for b, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def reference(model_weights, windows):
    """{sizes: twin table} -- every model's probabilities of every source from plain submit on a single-model engine, in batches of 64 as the
    feature cuts them, accumulated by the host twin in (source, model) order.  Computed once."""
    from clair_amd import _capi, _hostapi
    probs = {}                      # (sizes, source, model) -> [n, 90]
    for model, w in enumerate(model_weights):
        e = _capi.Engine(device=0, max_batch=BATCH, n_slots=1)
        try:
            e.load_weights(w)
            for sizes in SIZE_CASES:
                for b, (w0, labels) in enumerate(sources_of(sizes)):
                    rows = []
                    for first in range(0, len(labels), BATCH):
                        n = min(BATCH, len(labels) - first)
                        e.submit(0, windows["x"][w0 + first:w0 + first + n])
                        rows.append(np.concatenate(e.wait(0), axis=1))
                    probs[sizes, b, model] = np.concatenate(rows)
        finally:
            e.close()
    out = {}
    for sizes in SIZE_CASES:
        t = _hostapi.HostSiteTable()
        for b, (w0, labels) in enumerate(sources_of(sizes)):
            n = len(labels)
            t.begin_source(labels)
            for model in range(len(model_weights)):
                t.add_rows(0, probs[sizes, b, model], windows["x"][w0:w0 + n], windows["centre"][w0:w0 + n], windows["seq"][w0:w0 + n])
        out[sizes] = t
    return out


@pytest.fixture(scope="module")
def sites_engine(model_weights):
    from clair_amd import _capi
    e = _capi.Engine(device=0, max_batch=BATCH, n_slots=2)
    e.load_ensemble(model_weights)
    yield e
    e.close()


@pytest.mark.parametrize("kind", ["float32", "counts", "device"])
@pytest.mark.parametrize("sizes", SIZE_CASES, ids=lambda s: "-".join(map(str, s)))
def test_submit_sites_finish_and_site_calls_equal_the_reference(sites_engine, windows, reference, sizes, kind):
    from clair_amd import _capi
    e, twin = sites_engine, reference[sizes]
    t = e.site_table()
    for w0, labels in sources_of(sizes):
        t.begin_source(labels)
        inflight = []
        for k, first in enumerate(range(0, len(labels), BATCH)):
            n = min(BATCH, len(labels) - first)
            a = w0 + first
            batch = _capi.DeviceWindows(windows["frontend"], a, n) if kind == "device" else windows["x" if kind == "float32" else "counts"][a:a + n]
            if len(inflight) == 2:
                assert e.wait(inflight.pop(0)) is None
            e.submit_sites(k % 2, t, first, batch, windows["centre"][a:a + n], windows["seq"][a:a + n], counts=kind != "float32")
            inflight.append(k % 2)
        for slot in inflight:
            e.wait(slot)
    for order in ("chain", "position"):
        for minimum in (0, 4):
            want, got = cases.snapshot(twin, minimum, order), cases.snapshot(t, minimum, order)
            assert same(got, want), (order, minimum)                   # sites, counts, seqs, windows and averaged rows, bit for bit
            n_out = len(want[0])
            centre = np.stack([want[2][:, 16], (want[2] != 0).sum(axis=1).astype(np.uint8)], axis=1)
            for k, first in enumerate(range(0, n_out, BATCH)):
                n = min(BATCH, n_out - first)
                sl = slice(first, first + n)
                want_calls = e.decode(want[3][sl], _capi.split_outputs(want[4][sl]), centre[sl], slot=(k + 1) % 2)      # the existing decode on the twin's rows and windows
                e.submit_site_calls(k % 2, t, first, n, with_probabilities=True)
                calls, Y = e.wait(k % 2)
                assert calls.tobytes() == want_calls.tobytes()
                assert np.array_equal(cases.bits(np.concatenate(Y, axis=1)), cases.bits(want[4][sl]))
                e.submit_site_calls(k % 2, t, first, n)                # call records alone
                assert e.wait(k % 2).tobytes() == want_calls.tobytes()
                e.submit_site_calls(k % 2, t, first, n, with_calls=False)      # probabilities alone
                assert np.array_equal(cases.bits(np.concatenate(e.wait(k % 2), axis=1)), cases.bits(want[4][sl]))
    counts = cases.snapshot(twin, 0)[1]
    assert set(counts.tolist()) >= {3, 6} and (cases.snapshot(twin, 4)[1] >= 4).all()
    t.close()


# -- 6. callVarBam --ensemble_bam_fn against the chain ----------------------------------------------------------------------------------------
def body(text):
    return [ln for ln in text.splitlines() if not ln.startswith("#")]


def sorted_by_position(text):
    lines = text.splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    return "".join(ln + "\n" for ln in head + sorted(body(text), key=lambda ln: int(ln.split("\t")[1])))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Three BAMs of one read set (all reads; those with i % 3 != 0; those with i % 2 != 1), two checkpoints, and the six
    --output_for_ensemble runs of the chain, concatenated BAM-major."""
    import bam_fixture as bf
    import pileup_synth
    from clair_amd import callVarBam, weights
    tmp = str(tmp_path_factory.mktemp("sites"))
    case = pileup_synth.synth_case(seed=91, dup_burst=4)
    fa = os.path.join(tmp, "ref.fa")
    seq = "".join(case["fasta"].split(">chrOther")[0].splitlines()[1:])
    text, fai = bf.fasta_of({case["ctg"]: seq, "chrOther": "ACGT" * 30})
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    sam = case["sam"]
    sep = b"\n" if isinstance(sam, bytes) else "\n"
    at = b"@" if isinstance(sam, bytes) else "@"
    lines = sam.split(sep)
    if lines and not lines[-1]:
        lines.pop()
    head, reads = [ln for ln in lines if ln.startswith(at)], [ln for ln in lines if not ln.startswith(at)]
    picks = (lambda i: True, lambda i: i % 3 != 0, lambda i: i % 2 != 1)
    bams = []
    for b, keep in enumerate(picks):
        bam_fn = os.path.join(tmp, "reads%d.bam" % b)
        part = sep.join(head + [ln for i, ln in enumerate(reads) if keep(i)]) + sep
        bf.Bam(part, [(case["ctg"], case["ref_len"]), ("chrOther", 120)]).write(bam_fn, block=5000, index=True)
        bams.append(bam_fn)
    cks = [weights.save_weights(os.path.join(tmp, "model%d" % k), weights.synthetic_weights(seed=s, head_gain=6.0, lstm_bias_scale=0.1))[:-4]
           for k, s in enumerate((4242, 4343))]
    base = ["--threshold", "0.15", "--minCoverage", "5", "--batch_size", str(BATCH), "--ref_fn", fa, "--ctgName", case["ctg"],
            "--samtools", "/nonexistent/samtools", "--bam_reader", "native"]
    rows, sites = [], []
    for bam_fn in bams:
        for k, ck in enumerate(cks):
            out = os.path.join(tmp, "probs.txt")
            callVarBam.main(base + ["--bam_fn", bam_fn, "--chkpnt_fn", ck, "--call_fn", out, "--output_for_ensemble"])
            rows.append(open(out).read())
            if k == 0:
                sites.append(set(ln.split("\t", 2)[1] for ln in rows[-1].splitlines()))
    return {"tmp": tmp, "fa": fa, "bams": bams, "cks": cks, "base": base, "rows": "".join(rows), "sites": sites, "chain": {}, "ctg": case["ctg"]}


def chain_vcf(world, minimum):
    """ensemble --minimum_count_to_output N | call_var --input_probabilities --bam_fn <BAM 0>, once per N"""
    from clair_amd import call_var, ensemble
    if minimum not in world["chain"]:
        averaged = io.StringIO()
        ensemble.main(["--minimum_count_to_output", str(minimum)], stdin=io.StringIO(world["rows"]), stdout=averaged)
        out = os.path.join(world["tmp"], "chain%d.vcf" % minimum)
        stdin, sys.stdin = sys.stdin, io.StringIO(averaged.getvalue())
        try:
            call_var.Run(call_var.build_parser().parse_args(["--input_probabilities", "--call_fn", out, "--bam_fn", world["bams"][0], "--ref_fn", world["fa"]]))
        finally:
            sys.stdin = stdin
        world["chain"][minimum] = open(out).read()
    return world["chain"][minimum]


def feature(world, name, *extra, bams=None, cks=None):
    from clair_amd import callVarBam
    bams = world["bams"] if bams is None else bams
    cks = world["cks"] if cks is None else cks
    out = os.path.join(world["tmp"], name + ".vcf")
    more = [w for b in bams[1:] for w in ("--ensemble_bam_fn", b)]
    callVarBam.main(world["base"] + ["--bam_fn", bams[0], "--chkpnt_fn", cks[0], "--ensemble_chkpnt_fn", cks[1], "--call_fn", out] + more + list(extra))
    return open(out).read()


def test_the_three_bams_overlap_in_every_way(world):
    a, b, c = world["sites"]
    per_site = [sum(p in s for s in (a, b, c)) for p in a | b | c]
    assert per_site.count(3) > 0 and per_site.count(2) > 0 and per_site.count(1) > 0


@pytest.mark.parametrize("minimum", [0, 4])
def test_feature_writes_the_vcf_of_the_chain(world, minimum):
    want = chain_vcf(world, minimum)
    got = feature(world, "chain_order%d" % minimum, "--minimum_count_to_output", str(minimum))
    assert got == want
    assert len(body(want)) > 15
    positions = [int(ln.split("\t")[1]) for ln in body(want)]
    assert positions != sorted(positions)                                        # the chain's order is not position order
    single = feature(world, "single%d" % minimum, bams=world["bams"][:1])         # the ensemble over checkpoints alone, BAM 0
    assert single != want


@pytest.mark.parametrize("minimum", [0, 4])
def test_position_order_is_the_chain_sorted(world, minimum):
    got = feature(world, "position%d" % minimum, "--minimum_count_to_output", str(minimum), "--ensemble_order", "position")
    assert got == sorted_by_position(chain_vcf(world, minimum))


def test_position_order_through_the_overlap_filter(world):
    from clair_amd import overlap_variant
    got = feature(world, "overlap", "--minimum_count_to_output", "4", "--ensemble_order", "position", "--overlap_filter", "device")
    assert got == overlap_variant.filter_vcf_text(sorted_by_position(chain_vcf(world, 4)), "host", 0)


def test_host_front_end_writes_the_same_vcf(world):
    assert feature(world, "host_fe", "--minimum_count_to_output", "4", "--front_end", "host") == chain_vcf(world, 4)


def chain_with_native_lookup(world, minimum, bam_fn):
    """The chain's last two steps with --pysam_for_all_indel_bases and the look-up answered from the alignments of `bam_fn` by the native
    look-up's HOST twin (clair_host_indel_table over the host packer's slab; tests/test_indel_lookup_gpu.py holds the device tables to it
    byte for byte): ensemble --minimum_count_to_output N, then call_var's --input_probabilities loop."""
    import indel_lookup_cases as lc
    from clair_amd import call_var as cv
    from clair_amd import ensemble
    averaged = io.StringIO()
    ensemble.main(["--minimum_count_to_output", str(minimum)], stdin=io.StringIO(world["rows"]), stdout=averaged)
    slabs, _ = lc.host_slabs(bam_fn, world["ctg"])
    lookup = cv.IndelTableLookup(lc.host_tables(slabs), world["fa"])
    config = cv.OutputConfig(is_show_reference=False, is_debug=False, is_haploid_precision_mode_enabled=False, is_haploid_sensitive_mode_enabled=False,
                             is_output_for_ensemble=False, quality_score_for_pass=None)
    decoder = cv.VariantDecoder(config, lookup, always_use_bam=True)
    out = os.path.join(world["tmp"], "chain_native.vcf")
    writer = cv.VcfWriter(out, "SAMPLE", world["fa"])
    try:
        cv.call_variants_with_probabilities_input(None, decoder, writer, stream=io.StringIO(averaged.getvalue()))
    finally:
        writer.close()
        lookup.close()
    return open(out).read()


def test_native_lookup_writes_the_chain_vcf_with_bam_zero_answering(world, caplog):
    """--indel_lookup native --pysam_for_all_indel_bases, the whole file: against the chain whose look-up is answered from BAM 0's alignments
    by the native look-up's host twin.  (tests/fake_pysam.py does not serve as that look-up on this read set: it and the native look-up
    disagree at some positions, docs/ensemble.md; the host twin is what the device look-up is pinned to.)  Every indel row consults the
    look-up, sites that only BAM 1 or BAM 2 produced included, so a question sent to another BAM's front end, or a wrong window or
    probability row out of the table, changes the file -- as asking BAM 2 instead does."""
    import logging
    import re
    with caplog.at_level(logging.INFO):
        caplog.clear()
        got = feature(world, "native", "--minimum_count_to_output", "4", "--front_end", "device", "--indel_lookup", "native", "--pysam_for_all_indel_bases")
    m = re.search(r"indel look-up: (\d+) positions in (\d+) device calls", caplog.text)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0
    want = chain_with_native_lookup(world, 4, world["bams"][0])
    assert got == want
    asked = set(ln.split("\t")[1] for ln in body(want))
    assert asked - world["sites"][0]                                             # rows at sites BAM 0 itself did not produce
    assert len(body(want)) > 15 and chain_with_native_lookup(world, 4, world["bams"][2]) != want      # the file does depend on which BAM answers
    in_position_order = feature(world, "native_pos", "--minimum_count_to_output", "4", "--ensemble_order", "position", "--indel_lookup", "native",
                                "--pysam_for_all_indel_bases")
    assert in_position_order == sorted_by_position(want)
