"""Crafted sources for the site table of ensemble calling across BAMs (tests/test_sites.py on the host twin, tests/test_sites_gpu.py on the
device table) and the yardstick both are measured against: the text filter `python -m clair_amd ensemble` over the runs' --output_for_ensemble
rows (itself pinned to the reference's script by tests/golden/ensemble_small.json.gz).  Never the rule under test."""
import io

import numpy as np
import pytest

MILLION = 1000000
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


class Source(object):
    """One BAM's runs: positions int64 [n] ascending, seq uint8 [n,33], x float32 [n,33,8,4] (whole numbers, as pileup counts are),
    probs float32 [K,n,90] -- one packed row per model and site."""

    def __init__(self, positions, seq, x, probs):
        self.positions, self.seq, self.x, self.probs = positions, seq, x, probs

    def __len__(self):
        return len(self.positions)

    @property
    def centre(self):
        return np.stack([self.seq[:, 16], np.full(len(self), 33, np.uint8)], axis=1)


def membership(n_sources, universe, rng):
    """bool [n_sources, universe]: which source has which site.  Site 0 is in every source, 1 in the first only, 2 in the last only, 3 in the
    first two, 4 in the first three, the rest in a random non-empty subset -- so that every number of sources up to 3 (and all of them) occurs."""
    has = rng.random((n_sources, universe)) < 0.5
    for u in range(universe):
        if not has[:, u].any():
            has[rng.integers(n_sources), u] = True
    fixed = {0: range(n_sources), 1: [0], 2: [n_sources - 1], 3: range(min(2, n_sources)), 4: range(min(3, n_sources))}
    for u, members in fixed.items():
        has[:, u] = False
        has[list(members), u] = True
    return has


def crafted_sources(n_sources, models, universe=12, seed=5):
    """-> (sources, expected counts {position: rows}).  Positions are drawn without order between site number and position, so later sources
    bring keys below, between and above the known ones.  For every site whose row count c is even, the first 45 of its 90 values are built
    so that the six-decimal values of its c rows sum to c/2 modulo c: the true mean lies EXACTLY half-way between two six-decimal numbers."""
    rng = np.random.default_rng(seed + 100 * n_sources + models)
    pos_of = rng.choice(np.arange(1000, 1000 + 40 * universe), universe, replace=False).astype(np.int64)
    has = membership(n_sources, universe, rng)
    k = rng.integers(0, MILLION - 64, (n_sources, models, universe, 90))
    small = rng.random((universe, 90)) < 1.0 / 3.0
    k[:, :, small] = rng.integers(0, 60, (n_sources, models, int(small.sum())))
    counts = {}
    for u in range(universe):
        members = np.flatnonzero(has[:, u])
        c = len(members) * models
        counts[int(pos_of[u])] = c
        if c % 2 == 0:
            total = k[members, :, u, :45].sum(axis=(0, 1))
            k[members[-1], models - 1, u, :45] += (c // 2 - total) % c
            assert ((k[members, :, u, :45].sum(axis=(0, 1)) % c) == c // 2).all()
    sources = []
    for b in range(n_sources):
        sites = np.flatnonzero(has[b])
        sites = sites[np.argsort(pos_of[sites])]
        n = len(sites)
        p = (k[b][:, sites, :] / 1e6).astype(np.float32)
        assert np.array_equal(np.rint(p.astype(np.float64) * 1e6).astype(np.int64), k[b][:, sites, :])
        seq = BASES[rng.integers(0, 4, (n, 33))]
        x = rng.integers(-40, 60, (n, 33, 8, 4)).astype(np.float32)
        sources.append(Source(pos_of[sites], seq, x, p))
    return sources, counts


def sized_sources(sizes, models=1, seed=9):
    """Sources of given sizes over one pool of positions (overlapping at random): for the merge's and the scan's size boundaries."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(np.arange(1, 4 * max(max(sizes), 1) + 8), 2 * max(max(sizes), 1) + 4, replace=False)).astype(np.int64)
    sources = []
    for n in sizes:
        positions = np.sort(rng.choice(pool, n, replace=False))
        p = (rng.integers(0, MILLION, (models, n, 90)) / 1e6).astype(np.float32)
        sources.append(Source(positions, BASES[rng.integers(0, 4, (n, 33))], rng.integers(-9, 9, (n, 33, 8, 4)).astype(np.float32), p))
    return sources


MERGE_SHAPES = [
    ("empty first source", [[], [5, 9]]),
    ("empty later source", [[5, 9], [], [9, 11]]),
    ("all sites known", [[5, 9, 11], [5, 11]]),
    ("all sites new", [[5, 9], [6, 10]]),
    ("new keys below and above", [[50, 60], [10, 20, 70, 80]]),
    ("interleaved", [[10, 30, 50], [5, 20, 30, 40, 60], [1, 10, 35, 60, 99]]),
    ("one site only", [[7]]),
    ("one site, twice", [[7], [7]]),
]


def one_source(positions, value=0.25, models=1):
    """A source of given positions whose windows say which position they belong to and whose probabilities are all `value`."""
    positions = np.asarray(positions, dtype=np.int64)
    n = len(positions)
    return Source(positions, BASES[np.arange(n * 33).reshape(n, 33) % 4], np.tile(positions.astype(np.float32)[:, None, None, None], (1, 33, 8, 4)),
                  np.full((models, n, 90), value, dtype=np.float32))


def ensemble_rows_text(sources, ctg="chr1"):
    """What `cat` of the runs' files holds: for each BAM, for each model, its --output_for_ensemble rows (call_var's own writer)."""
    from clair_amd.call_var import VariantDecoder
    from clair_amd._capi import split_outputs
    out = []
    for s in sources:
        infos = [[ctg, str(p), q.tobytes().decode()] for p, q in zip(s.positions.tolist(), s.seq)]
        for model in range(s.probs.shape[0]):
            out.extend(VariantDecoder._ensemble_rows(s.x, infos, *split_outputs(s.probs[model])))
    return "".join(row + "\n" for row in out)


def text_filter(text, minimum_count):
    """The yardstick: the rows through clair_amd.ensemble.main -> (positions int64, seq uint8 [n,33], x float32 [n,33,8,4], rows float32 [n,90])
    in the filter's order, every number read as call_var --input_probabilities reads it."""
    from clair_amd import ensemble
    buf = io.StringIO()
    ensemble.main(["--minimum_count_to_output", str(minimum_count)], stdin=io.StringIO(text), stdout=buf)
    positions, seqs, xs, rows = [], [], [], []
    for row in buf.getvalue().splitlines():
        cols = row.split("\t")
        positions.append(int(cols[1]))
        seqs.append(np.frombuffer(cols[2].encode(), dtype=np.uint8))
        xs.append(np.array(cols[3:3 + 1056], dtype=np.float32).reshape(33, 8, 4))
        rows.append(np.array(cols[3 + 1056:], dtype=np.float32))
    n = len(positions)
    return (np.array(positions, dtype=np.int64), np.array(seqs, dtype=np.uint8).reshape(n, 33), np.array(xs, dtype=np.float32).reshape(n, 33, 8, 4),
            np.array(rows, dtype=np.float32).reshape(n, 90))


def fill(table, sources, with_windows=True, piece=None):
    """The sources into a table (host twin or device): per source begin_source, then one add_rows per model (in pieces of `piece` rows)."""
    for s in sources:
        table.begin_source(s.positions)
        n = len(s)
        step = piece or max(n, 1)
        for model in range(s.probs.shape[0]):
            for first in range(0, n, step):
                sl = slice(first, min(n, first + step))
                if with_windows:
                    table.add_rows(first, s.probs[model][sl], s.x[sl], s.centre[sl], s.seq[sl])
                else:
                    table.add_rows(first, s.probs[model][sl])


def snapshot(table, min_count, order="chain"):
    """Everything a finished table says: (positions, counts, seq [n,33], windows, rows)."""
    n = table.finish(min_count, order)
    positions, counts, seq = table.info(0, n)
    return positions, counts, seq[:, :33], table.windows(0, n), table.rows(0, n)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_errors(make):
    """Every error of the table, on whichever implementation `make` gives (the device test runs this too)."""
    row = np.full((1, 90), 0.5, dtype=np.float32)
    t = make()
    for bad in ([5, 5], [9, 5]):                                   # not strictly ascending
        with pytest.raises(Exception) as ei:
            t.begin_source(np.array(bad, dtype=np.int64))
        assert "strictly ascending" in str(ei.value)
    with pytest.raises(Exception) as ei:                           # rows before any source
        t.add_rows(0, row)
    assert "no source begun" in str(ei.value)
    t.begin_source(np.array([5, 9], dtype=np.int64))
    for first, n in ((2, 1), (1, 2), (-1, 1)):                      # a row range outside the current source
        with pytest.raises(Exception) as ei:
            t.add_rows(first, np.repeat(row, n, axis=0))
        assert "outside the current source" in str(ei.value)
    with pytest.raises(Exception) as ei:                           # the output list before finish
        t.rows(0, 1)
    assert "finish" in str(ei.value)
    t.add_rows(0, np.repeat(row, 2, axis=0))
    assert t.finish(0, "chain") == 2
    with pytest.raises(Exception) as ei:                           # a range outside the output list
        t.info(1, 2)
    assert "outside the output list" in str(ei.value)
    for call in (lambda: t.begin_source(np.array([1], dtype=np.int64)), lambda: t.add_rows(0, row)):      # use after finish
        with pytest.raises(Exception) as ei:
            call()
        assert "finished" in str(ei.value)
    t = make()                                                     # a 65th row of a site
    t.begin_source(np.array([5], dtype=np.int64))
    for _ in range(64):
        t.add_rows(0, row)
    with pytest.raises(Exception) as ei:
        t.add_rows(0, row)
    assert "more than 64 rows" in str(ei.value)
