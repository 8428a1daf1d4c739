// The indel look-up over packed alignments (include/clair_reads.h, "the indel look-up"): the rule for one operation, shared by the
// device kernels (csrc/indel_lookup.hip) and the host, and the whole table in plain sequential C++ -- the host twin
// (hostsrc/host_indel.cpp: clair_host_indel_table) and what clair_frontend_indel_table runs for a query the device could not finish.
// Restates what clair/call_var.py:102-170 reads out of pysam's pileup column: a token B+nSEQ / B-nNN.. of a read in column p - 1.
#ifndef CLAIR_INDEL_LOOKUP_CORE_H
#define CLAIR_INDEL_LOOKUP_CORE_H

#include "../../include/clair_reads.h"

#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define CLAIR_LOOKUP_HD __host__ __device__
#else
#define CLAIR_LOOKUP_HD
#endif

// Does operation j of the slab (an operation of alignment r) count as an indel of the look-up?  *p1 = the 1-based position it counts at.
// Every index is checked against the slab's sizes: a slab a caller packed wrongly yields no hit, not a read out of bounds.
CLAIR_LOOKUP_HD inline bool clair_lookup_indel_counts(const clair_read_t &r, const clair_op_t *ops, int64_t n_ops, int64_t seq_bytes, int64_t j, int64_t *p1) {
    if (!(r.flags & CLAIR_READ_LOOKUP)) return false;
    if (j <= (int64_t)r.op0 || j >= (int64_t)r.op0 + (int64_t)r.n_ops || j >= n_ops) return false;      // the first operation has nothing before it
    const clair_op_t op = ops[j], before = ops[j - 1];
    const uint32_t code = op.code_len & 3u, len = op.code_len >> 2;
    if (code != CLAIR_OP_I && code != CLAIR_OP_D) return false;
    if (len < 1 || len > CLAIR_LOOKUP_MAX_LEN) return false;
    if ((before.code_len & 3u) != CLAIR_OP_M || (int64_t)before.ref_off + (int64_t)(before.code_len >> 2) != (int64_t)op.ref_off) return false;
    const int64_t k = j - (int64_t)r.op0;
    if (r.reserved >> (k < 31 ? k : 31) & 1u) return false;                                              // something the slab does not hold lies between
    if (code == CLAIR_OP_I && ((uint64_t)op.q_off + len > r.seq_len || (uint64_t)r.seq0 + op.q_off + len > (uint64_t)seq_bytes)) return false;
    *p1 = r.pos0 + (int64_t)op.ref_off;
    return true;
}

CLAIR_LOOKUP_HD inline uint8_t clair_lookup_upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }

struct ClairLookupSlab {
    const clair_read_t *reads;
    int64_t n_reads;
    const clair_op_t *ops;
    int64_t n_ops;
    const uint8_t *seq;
    int64_t seq_bytes;
};

// positions[n] strictly ascending.  only != NULL: the queries with only[q] == 0 are left as they are.
inline void clair_indel_table_core(const ClairLookupSlab *slabs, int64_t n_slabs, const int64_t *positions, int64_t n, const uint8_t *only,
                                   clair_indel_entry_t *entries, int capacity, int32_t *n_entries, int32_t *depth, uint32_t *status) {
    std::vector<std::vector<clair_indel_entry_t>> table((size_t)n);
    std::vector<int32_t> cover((size_t)n, 0);
    auto lower = [&](int64_t p) { int64_t a = 0, b = n; while (a < b) { const int64_t m = (a + b) >> 1; if (positions[m] < p) a = m + 1; else b = m; } return a; };
    uint32_t rank0 = 0;
    for (int64_t s = 0; s < n_slabs; ++s) {
        const ClairLookupSlab &d = slabs[s];
        for (int64_t i = 0; i < d.n_reads; ++i) {
            const clair_read_t &r = d.reads[i];
            if (!(r.flags & CLAIR_READ_LOOKUP)) continue;
            for (int64_t j = r.op0; j < (int64_t)r.op0 + (int64_t)r.n_ops && j < d.n_ops; ++j) {
                const clair_op_t op = d.ops[j];
                const uint32_t code = op.code_len & 3u, len = op.code_len >> 2;
                if (code != CLAIR_OP_I) {                  // an M or D covers the columns [start, start + len): the queries p with p - 1 among them
                    const int64_t start = r.pos0 + (int64_t)op.ref_off;
                    for (int64_t q = lower(start + 1); q < n && positions[q] <= start + (int64_t)len; ++q) ++cover[(size_t)q];
                }
                int64_t p1 = 0;
                if (!clair_lookup_indel_counts(r, d.ops, d.n_ops, d.seq_bytes, j, &p1)) continue;
                const int64_t q = lower(p1);
                if (q >= n || positions[q] != p1 || (only && !only[q])) continue;
                clair_indel_entry_t e;
                memset(&e, 0, sizeof e);
                e.sign = code == CLAIR_OP_I ? 1 : -1;
                e.length = (uint8_t)len;
                if (code == CLAIR_OP_I)
                    for (uint32_t k = 0; k < len; ++k) e.bases[k] = clair_lookup_upper(d.seq[(size_t)r.seq0 + op.q_off + k]);
                bool seen = false;
                for (clair_indel_entry_t &have : table[(size_t)q])
                    if (have.sign == e.sign && have.length == e.length && memcmp(have.bases, e.bases, sizeof e.bases) == 0) { ++have.count; seen = true; break; }
                if (!seen) {
                    e.count = 1;
                    e.first_rank = rank0 + (uint32_t)i;
                    table[(size_t)q].push_back(e);
                }
            }
        }
        rank0 += (uint32_t)d.n_reads;
    }
    for (int64_t q = 0; q < n; ++q) {
        if (only && !only[q]) continue;
        const std::vector<clair_indel_entry_t> &t = table[(size_t)q];
        clair_indel_entry_t *out = entries + (size_t)q * (size_t)capacity;
        const size_t fit = t.size() < (size_t)capacity ? t.size() : (size_t)capacity;
        memset(out, 0, (size_t)capacity * sizeof *out);
        if (fit) memcpy(out, t.data(), fit * sizeof *out);
        n_entries[q] = (int32_t)t.size();
        depth[q] = cover[(size_t)q];
        status[q] = t.size() > (size_t)capacity ? (uint32_t)CLAIR_LOOKUP_ENTRIES : 0u;
    }
}

#endif
