// The gVCF stage on the CPU (include/clair_host.h: clair_host_gvcf_*; docs/gvcf.md): the host twin of csrc/gvcf.hip.  The rule, the block
// record and the argument checks are csrc/gvcf_core.h's, the same lines the kernels compile; what is restated here is the walk over the
// alignments (fe_tally_kernel's candidate-search half, element by element) and the segmentation (one sequential pass in place of the scan).
// Plain C++17, no HIP.
#include "../../include/clair_host.h"
#include "../../include/clair_reads.h"

#define CLAIR_GVCF_FN static inline
#include "../csrc/gvcf_core.h"

#include <cstring>
#include <string>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

namespace {

// the search's index of a READ base (IUPAC codes through IUPAC_base_to_ACGT_base_dict, N stays N = 6; shared/utils.py:19-28); 255: not a key
inline uint8_t read_base_index(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    if (c == 'N') return 6;
    const int r = clair_gvcf_ref_index(c);
    return r < 0 ? (uint8_t)255 : (uint8_t)r;
}

inline char *put_uint(char *p, uint64_t v) {
    char tmp[24];
    int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) *p++ = tmp[--k];
    return p;
}
inline char *put_int(char *p, int64_t v) {
    if (v < 0) { *p++ = '-'; return put_uint(p, (uint64_t)(-v)); }
    return put_uint(p, (uint64_t)v);
}
inline char *put_str(char *p, const char *s, size_t n) { memcpy(p, s, n); return p + n; }

}  // namespace

extern "C" {

int clair_host_gvcf_tally(const clair_read_t *reads, int64_t n_reads, const clair_op_t *ops, int64_t n_ops, const uint8_t *seq, int64_t seq_bytes, int64_t lo,
                          int64_t n, uint32_t *tallies, uint32_t *anomalies) {
    if (n_reads < 0 || n_ops < 0 || seq_bytes < 0 || n < 0) return clair_host_fail("gvcf: negative size");
    if ((n_reads > 0 && !reads) || (n_ops > 0 && !ops) || (seq_bytes > 0 && !seq) || (n > 0 && !tallies)) return clair_host_fail("gvcf: NULL argument");
    uint32_t bits = 0;
    for (int64_t i = 0; i < n_reads; ++i) {
        const clair_read_t &r = reads[i];
        if (!(r.flags & CLAIR_READ_EVC)) continue;
        if ((int64_t)r.op0 + r.n_ops > n_ops) return clair_host_fail("gvcf: alignment %lld names operations beyond the slab", (long long)i);
        for (uint32_t o = 0; o < r.n_ops; ++o) {
            const clair_op_t &op = ops[r.op0 + o];
            const uint32_t code = op.code_len & 3u;
            const int64_t len = op.code_len >> 2, rp = r.pos0 + op.ref_off;
            if (code == CLAIR_OP_M) {
                for (int64_t k = 0; k < len; ++k) {
                    const uint64_t qp = (uint64_t)op.q_off + (uint64_t)k;
                    if (qp >= r.seq_len || (int64_t)(r.seq0 + qp) >= seq_bytes) { bits |= CLAIR_FE_SEQ_OVERRUN; continue; }
                    const uint8_t ei = read_base_index(seq[r.seq0 + qp]);
                    if (ei == 255) { bits |= CLAIR_FE_BAD_BASE; continue; }
                    const int64_t t = rp + k - lo;
                    if (t >= 0 && t < n) tallies[t * 7 + ei] += 1;
                }
            } else {                                        // once per operation, at the base before it
                const int64_t t = rp - 1 - lo;
                if (t >= 0 && t < n) tallies[t * 7 + (code == CLAIR_OP_I ? 4 : 5)] += 1;
            }
        }
    }
    if (anomalies) *anomalies |= bits;
    return 0;
}

int clair_host_gvcf_blocks(const uint32_t *tallies, int64_t lo, int64_t n, const uint8_t *ref, int64_t ref_len, int64_t ref0, int c_match, int c_err, int c_half,
                           const uint8_t *band_of_gq, const int64_t *iv_start, const int64_t *iv_end, int64_t n_iv, clair_gvcf_block_t *out, int64_t capacity,
                           int64_t *n_blocks) {
    if (!n_blocks) return clair_host_fail("n_blocks is NULL");
    if (n < 0 || (n > 0 && !tallies) || ref_len < 0 || (ref_len > 0 && !ref)) return clair_host_fail("gvcf: tables or reference missing");
    char verdict[320];
    if (clair_gvcf_check_arguments(c_match, c_err, c_half, band_of_gq, iv_start, iv_end, n_iv, lo, n, verdict, sizeof verdict)) {
        clair_host_fail("%s", verdict);
        return 2;
    }
    if (capacity < 0 || (capacity > 0 && !out)) { clair_host_fail("gvcf: room for %lld records at a NULL pointer", (long long)capacity); return 2; }
    const clair_gvcf_costs c{c_match, c_err, c_half};
    int64_t count = 0;
    for (int64_t i = 0; i < n_iv; ++i) {
        clair_gvcf_run run = clair_gvcf_run_identity();
        int band = -1;
        for (int64_t p = iv_start[i]; p < iv_end[i]; ++p) {
            const int64_t t = p - lo, ri = p - ref0;
            const clair_gvcf_site s = clair_gvcf_rule(tallies + t * 7, ri >= 0 && ri < ref_len ? clair_gvcf_ref_index(ref[ri]) : -1, c);
            const int b = band_of_gq[s.gq];
            const bool head = p == iv_start[i] || b != band;
            if (head && p > iv_start[i]) {
                if (count < capacity) out[count] = clair_gvcf_block_of(run, lo, (uint32_t)(t - 1));
                ++count;
            }
            run = clair_gvcf_run_join(run, clair_gvcf_run_of(s, head, (uint32_t)t));
            band = b;
        }
        if (count < capacity) out[count] = clair_gvcf_block_of(run, lo, (uint32_t)(iv_end[i] - 1 - lo));
        ++count;
    }
    *n_blocks = count;
    return 0;
}

int clair_host_gvcf_format(const clair_gvcf_block_t *blocks, int64_t first, int64_t n, const char *ctg_name, const uint8_t *ref, int64_t ref_len, int64_t ref0,
                           char *out, int64_t out_cap, int64_t *out_len, int64_t *row_offsets) {
    if (first < 0 || n < 0 || (n > 0 && !blocks) || !ctg_name || !out_len || !row_offsets || out_cap < 0 || (out_cap > 0 && !out) || ref_len < 0 || (ref_len > 0 && !ref))
        return clair_host_fail("gvcf: bad argument");
    const size_t cl = strlen(ctg_name);
    static const char mid[] = "\t<NON_REF>\t.\t.\tEND=", fmt[] = "\tGT:GQ:DP:MIN_DP:PL\t0/0:";
    const int64_t worst = (int64_t)cl + 200;       // a row: the contig, eleven numbers of at most 20 characters, the fixed text
    int64_t at = 0;
    bool fits = true;
    for (int64_t k = 0; k < n; ++k) {
        const clair_gvcf_block_t &b = blocks[first + k];
        row_offsets[k] = at;
        char row[256], *big = nullptr, *p = row;
        if (worst > (int64_t)sizeof row) p = big = new char[(size_t)worst];
        char *const row0 = p;
        p = put_str(p, ctg_name, cl);
        *p++ = '\t';
        p = put_int(p, b.start + 1);
        p = put_str(p, "\t.\t", 3);
        const int64_t ri = b.start - ref0;
        *p++ = ri >= 0 && ri < ref_len ? (char)ref[ri] : 'N';
        p = put_str(p, mid, sizeof mid - 1);
        p = put_int(p, b.end);
        p = put_str(p, fmt, sizeof fmt - 1);
        p = put_int(p, b.gq); *p++ = ':';
        p = put_uint(p, b.dp); *p++ = ':';
        p = put_uint(p, b.min_dp); *p++ = ':';
        p = put_int(p, b.pl[0]); *p++ = ',';
        p = put_int(p, b.pl[1]); *p++ = ',';
        p = put_int(p, b.pl[2]); *p++ = '\n';
        const int64_t len = p - row0;
        if (fits && at + len <= out_cap) memcpy(out + at, row0, (size_t)len); else fits = false;
        at += len;
        delete[] big;
    }
    row_offsets[n] = at;
    *out_len = at;
    return 0;
}

}  // extern "C"
