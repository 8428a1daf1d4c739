// Host-side helpers of the Clair hot path (include/clair_host.h): compare_vcf's parse, join and counting, the twin of the device's
// (clair_amd/csrc/compare.hip).  Plain C++17, no HIP.  The rule itself is csrc/compare_core.h, the code the kernels run; this is the same
// passes as sequential loops, entry point for entry point.  The texts and the reference are borrowed: they stay the caller's until the handle
// is destroyed.
#include "../../include/clair_host.h"
#include "../csrc/compare_core.h"

#include <string.h>

#include <vector>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

struct clair_host_compare {
    std::vector<uint8_t> names;
    std::vector<int64_t> name_off, first, starts, ends;
    bool have_regions = false;
    const uint8_t *ref_seq = nullptr;
    std::vector<int64_t> ref_off;             // empty: no reference set
    struct Side {
        const uint8_t *text = nullptr;        // what the records point into: the parsed text, or the arena once the side is left-aligned
        std::vector<uint8_t> arena;
        bool aligned = false;
        std::vector<clair_compare_record> rec;
        std::vector<uint8_t> outcome;
        int64_t drops[3] = {0, 0, 0};
        bool parsed = false, sorted = false;
    } side[2];
    std::vector<int64_t> counts;
    bool ran = false;
};

namespace {

const char *const SIDE_NAME[2] = {"calls", "truth"};

bool keys_ascend(const std::vector<clair_compare_record> &r) {
    for (size_t i = 1; i < r.size(); ++i) if (clair_compare_key(r[i - 1]) > clair_compare_key(r[i])) return false;
    return true;
}

}  // namespace

extern "C" {

int clair_host_compare_create(clair_host_compare_t **out) {
    if (!out) return clair_host_fail("compare create: NULL argument");
    *out = new clair_host_compare();
    return 0;
}

void clair_host_compare_destroy(clair_host_compare_t *h) { delete h; }

int clair_host_compare_set_contigs(clair_host_compare_t *h, const uint8_t *names, const int64_t *offsets, int n_contigs) {
    if (!h || n_contigs < 0 || !offsets || (n_contigs > 0 && !names)) return clair_host_fail("compare set_contigs: bad arguments");
    for (int k = 0; k < n_contigs; ++k) if (offsets[k] > offsets[k + 1] || offsets[0] != 0) return clair_host_fail("compare set_contigs: offsets must ascend from 0");
    h->name_off.assign(offsets, offsets + n_contigs + 1);
    h->names.assign(names, names + offsets[n_contigs]);
    h->side[0].parsed = h->side[1].parsed = h->have_regions = h->ran = false;      // ids mean something else now
    h->ref_off.clear();
    return 0;
}

int clair_host_compare_set_reference(clair_host_compare_t *h, const uint8_t *seq, const int64_t *offsets, int n_contigs) {
    if (!h || !offsets) return clair_host_fail("compare set_reference: bad arguments");
    if (h->name_off.empty()) return clair_host_fail("compare set_reference: set the contigs first");
    if (n_contigs != (int)h->name_off.size() - 1) return clair_host_fail("compare set_reference: %d contigs, the contig table has %d", n_contigs, (int)h->name_off.size() - 1);
    for (int k = 0; k < n_contigs; ++k) if (offsets[0] != 0 || offsets[k] > offsets[k + 1]) return clair_host_fail("compare set_reference: offsets must ascend from 0");
    if (offsets[n_contigs] > 0 && !seq) return clair_host_fail("compare set_reference: NULL sequence");
    h->ref_seq = seq;
    h->ref_off.assign(offsets, offsets + n_contigs + 1);
    return 0;
}

int clair_host_compare_set_regions(clair_host_compare_t *h, const int64_t *first, const int64_t *starts, const int64_t *ends, int64_t n_intervals) {
    if (!h) return clair_host_fail("compare set_regions: NULL handle");
    h->ran = false;
    if (n_intervals < 0) { h->have_regions = false; return 0; }
    const int64_t n_ctg = (int64_t)h->name_off.size() - 1;
    if (n_ctg < 0) return clair_host_fail("compare set_regions: set the contigs first");
    if (!first || (n_intervals > 0 && (!starts || !ends))) return clair_host_fail("compare set_regions: NULL argument");
    if (first[0] != 0 || first[n_ctg] != n_intervals) return clair_host_fail("compare set_regions: first[] must run from 0 to n_intervals");
    for (int64_t k = 0; k < n_ctg; ++k) {
        if (first[k] > first[k + 1]) return clair_host_fail("compare set_regions: first[] must ascend");
        for (int64_t i = first[k]; i < first[k + 1]; ++i)
            if (starts[i] >= ends[i] || (i > first[k] && starts[i] <= ends[i - 1])) return clair_host_fail("compare set_regions: interval %lld is empty or not sorted and merged", (long long)i);
    }
    h->first.assign(first, first + n_ctg + 1);
    h->starts.assign(starts, starts + n_intervals);
    h->ends.assign(ends, ends + n_intervals);
    h->have_regions = true;
    return 0;
}

int clair_host_compare_parse(clair_host_compare_t *h, int side, const uint8_t *text, int64_t len, int64_t *stats) {
    if (!h || side < 0 || side > 1 || len < 0 || (len > 0 && !text) || !stats) return clair_host_fail("compare parse: bad arguments");
    if (h->name_off.empty()) return clair_host_fail("compare parse: set the contigs first");
    if (len > (int64_t)UINT32_MAX) return clair_host_fail("compare parse: the %s text has %lld bytes, the limit is 2^32 - 1", SIDE_NAME[side], (long long)len);
    clair_host_compare::Side &s = h->side[side];
    s.parsed = false;
    h->ran = false;
    s.text = text;
    s.aligned = false;
    s.arena.clear();
    s.rec.clear();
    s.drops[0] = s.drops[1] = s.drops[2] = 0;
    const clair_compare_contigs contigs{h->names.data(), h->name_off.data(), (int32_t)h->name_off.size() - 1};
    int64_t lines = 0, rows = 0;
    for (int64_t b = 0; b < len;) {
        const void *nl = memchr(text + b, '\n', (size_t)(len - b));
        const int64_t e = nl ? (const uint8_t *)nl - text : len;
        ++lines;
        clair_compare_row row;
        const int code = clair_compare_parse_line(text, b, e, (uint32_t)lines, contigs, &row);
        if (code > CLAIR_CMP_ROW_DATA) return clair_host_fail("%s line %lld: %s", SIDE_NAME[side], (long long)lines, clair_compare_row_error(code));
        rows += code == CLAIR_CMP_ROW_DATA;
        for (int w = 0; w < 2; ++w) {
            if (row.slot[w] == CLAIR_CMP_SLOT_KEPT) s.rec.push_back(row.rec[w]);
            else if (row.slot[w] != CLAIR_CMP_SLOT_NONE) ++s.drops[row.slot[w] - CLAIR_CMP_SLOT_SYMBOLIC];
        }
        b = e + 1;
    }
    s.sorted = keys_ascend(s.rec);
    s.parsed = true;
    const int64_t out[CLAIR_CMP_STATS] = {lines, rows, (int64_t)s.rec.size(), s.drops[0], s.drops[1], s.drops[2], s.sorted ? 1 : 0, 0};
    memcpy(stats, out, sizeof out);
    return 0;
}

int clair_host_compare_left_align(clair_host_compare_t *h, int side, int64_t *stats) {
    if (!h || side < 0 || side > 1 || !stats || !h->side[side].parsed) return clair_host_fail("compare left_align: no parsed text on that side");
    if (h->ref_off.empty()) return clair_host_fail("compare left_align: set the reference first");
    clair_host_compare::Side &s = h->side[side];
    if (s.aligned) return clair_host_fail("compare left_align: the %s are left-aligned already", SIDE_NAME[side]);
    h->ran = false;
    const clair_compare_reference g{h->ref_seq, h->ref_off.data()};
    int64_t out[CLAIR_CMP_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t bytes = 0;
    for (const clair_compare_record &r : s.rec) bytes += (uint64_t)r.ref_len + r.alt_len;
    s.arena.assign((size_t)bytes, 0);
    uint32_t slot = 0;
    for (clair_compare_record &r : s.rec) {
        const uint32_t mine = slot;
        slot += (uint32_t)r.ref_len + r.alt_len;
        clair_compare_event ev;
        const int what = clair_compare_la_case(g, s.text, r, &ev);
        out[CLAIR_CMP_LA_EXAMINED] += what != CLAIR_CMP_LA_UNTOUCHED;
        out[CLAIR_CMP_LA_NO_SEQUENCE] += what == CLAIR_CMP_LA_IS_NO_SEQUENCE;
        out[CLAIR_CMP_LA_REF_MISMATCH] += what == CLAIR_CMP_LA_IS_REF_MISMATCH;
        const bool ins = r.ref_len < r.alt_len;
        if (what != CLAIR_CMP_LA_CANDIDATE) clair_compare_la_copy(s.text, r, mine, s.arena.data());
        else {
            const uint8_t *contig = g.seq + g.off[r.ctg];
            int64_t steps = 0;
            while (!clair_compare_la_stops(contig, s.text, ev, steps)) ++steps;
            const uint32_t at_short = ins ? mine : mine + r.ref_len, at_long = ins ? mine + r.ref_len : mine;
            for (uint32_t k = 0; k <= ev.len; ++k) s.arena[at_long + k] = clair_compare_la_long_byte(contig, s.text, ev, steps, k);
            s.arena[at_short] = clair_compare_la_short_byte(contig, s.text, ev, steps);
            if (ev.a - steps < 1) ++out[CLAIR_CMP_LA_AT_CONTIG_START];
            else {
                out[CLAIR_CMP_LA_SHIFTED] += ev.a - steps != r.pos;
                r.pos = (int32_t)(ev.a - steps);
            }
        }
        r.ref_off = mine;
        r.alt_off = mine + r.ref_len;
    }
    s.text = s.arena.data();
    s.aligned = true;
    s.sorted = keys_ascend(s.rec);
    out[CLAIR_CMP_LA_SORTED] = s.sorted ? 1 : 0;
    out[CLAIR_CMP_LA_ARENA] = (int64_t)bytes;
    memcpy(stats, out, sizeof out);
    return 0;
}

int clair_host_compare_allele_text(clair_host_compare_t *h, int side, uint8_t *out) {
    if (!h || side < 0 || side > 1 || !h->side[side].parsed || !h->side[side].aligned) return clair_host_fail("compare allele_text: that side was not left-aligned");
    const clair_host_compare::Side &s = h->side[side];
    if (!s.arena.empty()) {
        if (!out) return clair_host_fail("compare allele_text: NULL argument");
        memcpy(out, s.arena.data(), s.arena.size());
    }
    return 0;
}

int clair_host_compare_keys(clair_host_compare_t *h, int side, int64_t *keys) {
    if (!h || side < 0 || side > 1 || !h->side[side].parsed) return clair_host_fail("compare keys: no parsed text on that side");
    const auto &r = h->side[side].rec;
    if (!r.empty() && !keys) return clair_host_fail("compare keys: NULL argument");
    for (size_t i = 0; i < r.size(); ++i) keys[i] = clair_compare_key(r[i]);
    return 0;
}

int clair_host_compare_permute(clair_host_compare_t *h, int side, const int64_t *perm) {
    if (!h || side < 0 || side > 1 || !h->side[side].parsed) return clair_host_fail("compare permute: no parsed text on that side");
    clair_host_compare::Side &s = h->side[side];
    const int64_t n = (int64_t)s.rec.size();
    if (n > 0 && !perm) return clair_host_fail("compare permute: NULL argument");
    std::vector<clair_compare_record> to((size_t)n);
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (perm[i] < 0 || perm[i] >= n || seen[(size_t)perm[i]]) return clair_host_fail("compare permute: entry %lld is no permutation of 0 .. %lld", (long long)i, (long long)n - 1);
        seen[(size_t)perm[i]] = 1;
        to[(size_t)i] = s.rec[(size_t)perm[i]];
    }
    s.rec.swap(to);
    s.sorted = keys_ascend(s.rec);
    h->ran = false;
    return 0;
}

int clair_host_compare_run(clair_host_compare_t *h) {
    if (!h) return clair_host_fail("compare run: NULL handle");
    for (int k = 0; k < 2; ++k) {
        if (!h->side[k].parsed) return clair_host_fail("compare run: the %s were not parsed", SIDE_NAME[k]);
        if (!h->side[k].sorted) return clair_host_fail("compare run: the %s records are not in (contig, pos) order: permute them first", SIDE_NAME[k]);
    }
    const clair_compare_regions g{h->have_regions ? h->first.data() : nullptr, h->starts.data(), h->ends.data()};
    clair_host_compare::Side &c = h->side[CLAIR_CMP_CALLS], &t = h->side[CLAIR_CMP_TRUTH];
    const int64_t n_c = (int64_t)c.rec.size(), n_t = (int64_t)t.rec.size();
    c.outcome.assign((size_t)n_c, 0);
    t.outcome.assign((size_t)n_t, 0);
    for (int64_t i = 0; i < n_t; ++i) t.outcome[(size_t)i] = clair_compare_classify(t.rec.data(), t.text, i, g);
    for (int64_t i = 0; i < n_c; ++i) {
        uint8_t o = clair_compare_classify(c.rec.data(), c.text, i, g);
        if (o == CLAIR_CMP_PENDING) {
            const int64_t j = clair_compare_find(t.rec.data(), n_t, t.text, c.rec[(size_t)i], c.text);
            o = j < 0 ? CLAIR_CMP_FP : t.rec[(size_t)j].copies == c.rec[(size_t)i].copies ? CLAIR_CMP_TP : CLAIR_CMP_GT;
            if (j >= 0) t.outcome[(size_t)j] = o;
        }
        c.outcome[(size_t)i] = o;
    }
    for (int64_t i = 0; i < n_t; ++i) if (t.outcome[(size_t)i] == CLAIR_CMP_PENDING) t.outcome[(size_t)i] = CLAIR_CMP_FN;

    h->counts.assign(CLAIR_CMP_COUNTS, 0);
    int64_t *cnt = h->counts.data();
    for (int k = 0; k < 2; ++k) {
        const clair_host_compare::Side &s = h->side[k];
        for (size_t i = 0; i < s.rec.size(); ++i) {
            const int type = s.rec[i].type, o = s.outcome[i];
            ++cnt[CLAIR_CMP_AT_COUNTS + (k * CLAIR_CMP_TYPES + type) * CLAIR_CMP_OUTCOMES + o];
            if (k == CLAIR_CMP_CALLS && o < CLAIR_CMP_KINDS) ++cnt[CLAIR_CMP_AT_HIST + (type * CLAIR_CMP_KINDS + o) * CLAIR_CMP_QUAL_BINS + s.rec[i].qual_bin];
        }
        for (int d = 0; d < 3; ++d) cnt[CLAIR_CMP_AT_DROPS + k * 3 + d] = s.drops[d];
    }
    for (int row = 0; row < CLAIR_CMP_TYPES * CLAIR_CMP_KINDS; ++row) {
        int64_t sum = 0;
        for (int q = CLAIR_CMP_QUAL_BINS - 1; q >= 0; --q) {
            sum += cnt[CLAIR_CMP_AT_HIST + row * CLAIR_CMP_QUAL_BINS + q];
            cnt[CLAIR_CMP_AT_AT_LEAST + row * CLAIR_CMP_QUAL_BINS + q] = sum;
        }
    }
    h->ran = true;
    return 0;
}

int clair_host_compare_counts(clair_host_compare_t *h, int64_t *counts) {
    if (!h || !counts || !h->ran) return clair_host_fail("compare counts: nothing was run");
    memcpy(counts, h->counts.data(), sizeof(int64_t) * CLAIR_CMP_COUNTS);
    return 0;
}

int clair_host_compare_records(clair_host_compare_t *h, int side, clair_compare_record_t *records, uint8_t *outcomes) {
    if (!h || side < 0 || side > 1 || !h->side[side].parsed) return clair_host_fail("compare records: no parsed text on that side");
    const clair_host_compare::Side &s = h->side[side];
    if (records && !s.rec.empty()) memcpy(records, s.rec.data(), s.rec.size() * sizeof(clair_compare_record));
    if (outcomes) {
        if (!h->ran) return clair_host_fail("compare records: nothing was run, so there are no outcomes");
        if (!s.outcome.empty()) memcpy(outcomes, s.outcome.data(), s.outcome.size());
    }
    return 0;
}

}  // extern "C"
