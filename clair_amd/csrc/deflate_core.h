// One RFC 1951 (DEFLATE) compressor for one BGZF block, compiled twice: by g++ into libclair_host.so (clair_host_deflate_bgzf, the twin that
// is tested and run under the host sanitizer) and by hipcc into deflate_bgzf_kernel (csrc/deflate.hip), a wave per block.  Plain C++17: no
// HIP type appears here.  The includer may define CLAIR_DEF_FN (`__device__ inline` on the device) and defines CLAIR_DEF_WAVE when the 64
// lanes are a wave's; without it the lanes are a loop from 0 to 63.  docs/merge_vcf.md has the rule in prose.
//
// The rule (device and twin agree by construction: nothing below depends on the order in which lanes run)
//   The code is a sequence of regions.  A LANES region runs its body once per lane; inside one, a lane reads only what earlier regions
//   wrote and writes only its own elements, or combines by OR / add (commutative).  A ONE region runs once (lane 0).  Regions are separated
//   by sync().
//   Matches: steps of 64 positions.  Lane l of the step at `base` looks at p = base + l.  It hashes the 4 bytes at p (14 bits).  Its
//   candidate is the nearest lower position of the step with the same hash, else the position the table held for the hash BEFORE this step.
//   When there is one at a distance of at most 32768 and p is not already covered by a match taken in an earlier step, it counts how many
//   bytes agree (4 .. 258, not beyond the block's end).  Then the step's positions enter the table: where several lanes have one hash the
//   highest position is stored (a lane stores when no higher lane of the step has its hash).  Matches are taken greedily from left to
//   right: p's match is taken iff no match taken before covers p; an uncovered p without a match is a literal.
//   Deflate blocks: tokens are cut, at a step boundary, before they exceed 8192; every cut is one dynamic-Huffman block (BTYPE 2).  The
//   code lengths come from the two-queue Huffman construction over the symbols sorted by (count, symbol), limited to 15 (7 for the
//   code-length code) by moving leaves down as zlib's gen_bitlen does; a set with fewer than two used symbols gets the lowest unused
//   ones added, so every set sent is complete.  The lengths are run-length coded with 16 / 17 / 18, HLIT / HDIST / HCLEN trimmed.
//   Bits: every token's bit string is placed by the prefix sum of the lengths of the tokens before it and ORed into a staging window of
//   words, which is flushed to the output as whole words.
//   Stored: when the stream up to and including the block about to be sent would not be smaller than the stored form (5 + n bytes), the
//   whole BGZF block is rewritten as one stored block (BTYPE 0).  18 + 5 + 65280 + 8 = 65311 <= 65536: it always fits.
// Totality: every loop is bounded by the block length n, the token count (<= 8192), the symbol count (<= 288) or 64; every staging index is
// below STAGE_WORDS + 2 (ensure_room), every output word below 16384 (the stored bound above).
#ifndef CLAIR_DEFLATE_CORE_H
#define CLAIR_DEFLATE_CORE_H

#include <stdint.h>

#ifndef CLAIR_DEF_FN
#define CLAIR_DEF_FN inline
#endif
#ifndef CLAIR_INF_FN
#define CLAIR_INF_FN CLAIR_DEF_FN
#endif
#include "inflate_core.h"                        // the lane-chunked CRC-32, bit_reverse

#ifdef CLAIR_DEF_WAVE
#define CLAIR_DEF_LANES(c, lane) for (uint32_t lane = (c).lane_id(), once_ = 1; once_; once_ = 0)
#define CLAIR_DEF_ONE(c) if ((c).lane_id() == 0)
#else
#define CLAIR_DEF_LANES(c, lane) for (uint32_t lane = 0; lane < clair_def::LANES; ++lane)
#define CLAIR_DEF_ONE(c) if (true)
#endif

namespace clair_def {

constexpr uint32_t LANES = 64;
constexpr uint32_t MAX_IN = 65280;               // bgzip's 0xff00
constexpr uint32_t SLOT = 65536;                 // a BGZF block at most
constexpr uint32_t HASH_BITS = 14;
constexpr uint32_t TOK_MAX = 8192;               // tokens of one deflate block
constexpr uint32_t STAGE_WORDS = 2048;           // the staging window: 8 KiB
constexpr uint32_t MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr uint32_t EMPTY = 0xffff;               // no position (positions are below 65280), no hash (hashes are below 2^14)
constexpr uint32_t TOKEN_BITS = 48;              // 15 + 5 + 15 + 13
constexpr uint32_t HEADER_ROOM = 8192;           // a dynamic header is at most 17 + 57 + 316 * 14 bits

struct Work {                                    // LDS on the device: 144.9 KiB (the budget is in csrc/deflate.hip)
    uint32_t in32[MAX_IN / 4];                   // the block's input
    uint32_t tok[TOK_MAX];                       // literal: the byte; match: 1 << 31 | (length - 3) << 16 | (distance - 1)
    uint32_t stage[STAGE_WORDS + 2];
    uint16_t table[1u << HASH_BITS];             // hash -> the highest position entered with it
    uint32_t crc_table[256];
    uint32_t freq_ll[288], freq_d[32], freq_cl[20];
    uint32_t node_freq[2 * 288];
    uint32_t nb[LANES];                          // bits of the lane's token; the lanes' CRC shares
    uint16_t parent[2 * 288], order[288];
    uint16_t code_ll[288], code_d[32], code_cl[20];
    uint16_t clseq[320];                         // the run-length coded lengths: symbol | extra << 8
    uint16_t m_len[LANES], m_dist[LANES], m_hash[LANES];
    uint8_t depth[2 * 288];
    uint8_t m_top[LANES];                        // the lane is the highest of the step with its hash
    uint8_t len_ll[288], len_d[32], len_cl[20];
    uint32_t bitpos;                             // bits of the BGZF block written so far (from its first header byte)
    uint32_t w0;                                 // the output word stage[0] stands for
    uint32_t ntok, cover, extra_bits, n_clseq, stored, crc;
};

CLAIR_DEF_FN uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }      // v > 0

// length 3 .. 258 -> literal/length symbol, extra bits and their value
CLAIR_DEF_FN void length_symbol(uint32_t length, uint32_t *sym, uint32_t *eb, uint32_t *ev) {
    const uint32_t l = length - 3;
    if (length == 258) { *sym = 285; *eb = 0; *ev = 0; return; }
    if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; return; }
    const uint32_t e = log2_floor(l) - 2;
    *sym = 257 + 4 * (e + 1) + ((l >> e) & 3);
    *eb = e;
    *ev = l & ((1u << e) - 1);
}

// distance 1 .. 32768 -> distance symbol, extra bits and their value
CLAIR_DEF_FN void distance_symbol(uint32_t distance, uint32_t *sym, uint32_t *eb, uint32_t *ev) {
    const uint32_t d = distance - 1;
    if (d < 4) { *sym = d; *eb = 0; *ev = 0; return; }
    const uint32_t hb = log2_floor(d), e = hb - 1;
    *sym = 2 * hb + ((d >> e) & 1);
    *eb = e;
    *ev = d & ((1u << e) - 1);
}

// -- ONE-region helpers (serial) ------------------------------------------------------------------------------------------------------
CLAIR_DEF_FN void put_bits(Work &w, uint32_t v, uint32_t nbits) {        // nbits <= 32, v < 2^nbits; room was ensured
    const uint32_t rel = w.bitpos - w.w0 * 32, i = rel >> 5, sh = rel & 31;
    w.stage[i] |= v << sh;
    if (sh + nbits > 32) w.stage[i + 1] |= v >> (32 - sh);
    w.bitpos += nbits;
}

// freq[0..nsym) -> lens[0..nsym), at most max_len, a complete code over at least two symbols
CLAIR_DEF_FN void build_lengths(Work &w, const uint32_t *freq, uint32_t nsym, uint32_t max_len, uint8_t *lens) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        lens[s] = 0;
        if (freq[s]) w.order[m++] = (uint16_t)s;
    }
    for (uint32_t s = 0; m < 2 && s < nsym; ++s)             // the lowest unused symbols, weight 1
        if (!freq[s]) w.order[m++] = (uint16_t)s;
    // sort by (weight, symbol): insertion sort, the order is unique
    for (uint32_t i = 1; i < m; ++i) {
        const uint32_t s = w.order[i], fs = freq[s] ? freq[s] : 1;
        uint32_t j = i;
        while (j > 0) {
            const uint32_t t = w.order[j - 1], ft = freq[t] ? freq[t] : 1;
            if (ft < fs || (ft == fs && t < s)) break;
            w.order[j] = (uint16_t)t;
            --j;
        }
        w.order[j] = (uint16_t)s;
    }
    for (uint32_t i = 0; i < m; ++i) w.node_freq[i] = freq[w.order[i]] ? freq[w.order[i]] : 1;
    // two queues: the sorted leaves [0, m) and the internal nodes [m, 2m - 1) in the order they are made (their weights never fall)
    uint32_t leaf = 0, inner = m, next = m;
    while (next < 2 * m - 1) {
        uint32_t pick[2];
        for (int k = 0; k < 2; ++k) {
            if (leaf < m && (inner >= next || w.node_freq[leaf] <= w.node_freq[inner])) pick[k] = leaf++;
            else pick[k] = inner++;
        }
        w.node_freq[next] = w.node_freq[pick[0]] + w.node_freq[pick[1]];
        w.parent[pick[0]] = w.parent[pick[1]] = (uint16_t)next;
        ++next;
    }
    // depths from the root down (a parent's index is above its children's), clamped; `overflow` counts every clamped node (zlib, gen_bitlen)
    uint32_t count[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    const uint32_t root = 2 * m - 2;
    int overflow = 0;
    w.depth[root] = 0;
    for (uint32_t i = root; i-- > 0;) {
        uint32_t d = (uint32_t)w.depth[w.parent[i]] + 1;
        if (d > max_len) { d = max_len; ++overflow; }
        w.depth[i] = (uint8_t)d;
        if (i < m) count[d] += 1;
    }
    if (overflow <= 0) {
        for (uint32_t i = 0; i < m; ++i) lens[w.order[i]] = w.depth[i];
        return;
    }
    do {                                         // each turn takes 2^-max_len off the Kraft sum
        uint32_t bits = max_len - 1;
        while (bits > 0 && count[bits] == 0) --bits;
        count[bits] -= 1;
        count[bits + 1] += 2;
        count[max_len] -= 1;
        overflow -= 2;
    } while (overflow > 0);
    uint32_t at = 0;                             // the longest codes to the rarest symbols
    for (uint32_t bits = max_len; bits > 0; --bits)
        for (uint32_t k = 0; k < count[bits] && at < m; ++k) lens[w.order[at++]] = (uint8_t)bits;
}

// canonical codes, bit-reversed (deflate sends a code's most significant bit first)
CLAIR_DEF_FN void make_codes(const uint8_t *lens, uint32_t nsym, uint16_t *codes) {
    uint32_t count[16], next[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < nsym; ++s) count[lens[s] & 15] += 1;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (uint32_t s = 0; s < nsym; ++s) {
        const uint32_t l = lens[s] & 15;
        codes[s] = l ? (uint16_t)clair_inf::bit_reverse(next[l]++, l) : 0;
    }
}

CLAIR_DEF_FN uint32_t cl_extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }

CLAIR_DEF_FN void cl_emit(Work &w, uint32_t sym, uint32_t extra) {
    if (w.n_clseq < 320) w.clseq[w.n_clseq++] = (uint16_t)(sym | extra << 8);
    w.freq_cl[sym] += 1;
}

// The codes of the block whose counts are in freq_ll / freq_d, and its header's parts.  -> the bits of the whole block (header, tokens, end)
CLAIR_DEF_FN uint32_t plan_block(Work &w, uint32_t *hlit_out, uint32_t *hdist_out, uint32_t *hclen_out) {
    build_lengths(w, w.freq_ll, 286, 15, w.len_ll);
    build_lengths(w, w.freq_d, 30, 15, w.len_d);
    make_codes(w.len_ll, 286, w.code_ll);
    make_codes(w.len_d, 30, w.code_d);
    uint32_t hlit = 286, hdist = 30;
    while (hlit > 257 && w.len_ll[hlit - 1] == 0) --hlit;
    while (hdist > 1 && w.len_d[hdist - 1] == 0) --hdist;
    const uint32_t total = hlit + hdist;
    for (int s = 0; s < 20; ++s) w.freq_cl[s] = 0;
    w.n_clseq = 0;
    uint32_t i = 0;
    while (i < total) {                          // every turn takes at least one length
        const uint32_t v = i < hlit ? w.len_ll[i] : w.len_d[i - hlit];
        uint32_t run = 1;
        while (i + run < total && (i + run < hlit ? w.len_ll[i + run] : w.len_d[i + run - hlit]) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const uint32_t r = run < 138 ? run : 138; cl_emit(w, 18, r - 11); run -= r; }
            if (run >= 3) { cl_emit(w, 17, run - 3); run = 0; }
            for (; run > 0; --run) cl_emit(w, 0, 0);
        } else {
            cl_emit(w, v, 0);
            run -= 1;
            while (run >= 3) { const uint32_t r = run < 6 ? run : 6; cl_emit(w, 16, r - 3); run -= r; }
            for (; run > 0; --run) cl_emit(w, v, 0);
        }
    }
    build_lengths(w, w.freq_cl, 19, 7, w.len_cl);
    make_codes(w.len_cl, 19, w.code_cl);
    const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = 19;
    while (hclen > 4 && w.len_cl[cl_order[hclen - 1]] == 0) --hclen;
    uint32_t bits = 3 + 14 + 3 * hclen + w.extra_bits;
    for (uint32_t s = 0; s < 19; ++s) bits += w.freq_cl[s] * (w.len_cl[s] + cl_extra_bits(s));
    for (uint32_t s = 0; s < 286; ++s) bits += w.freq_ll[s] * w.len_ll[s];
    for (uint32_t s = 0; s < 30; ++s) bits += w.freq_d[s] * w.len_d[s];
    *hlit_out = hlit;
    *hdist_out = hdist;
    *hclen_out = hclen;
    return bits;
}

CLAIR_DEF_FN void put_block_header(Work &w, uint32_t final_block, uint32_t hlit, uint32_t hdist, uint32_t hclen) {
    const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    put_bits(w, final_block | 2u << 1, 3);
    put_bits(w, hlit - 257, 5);
    put_bits(w, hdist - 1, 5);
    put_bits(w, hclen - 4, 4);
    for (uint32_t k = 0; k < hclen; ++k) put_bits(w, w.len_cl[cl_order[k]], 3);
    for (uint32_t k = 0; k < w.n_clseq; ++k) {
        const uint32_t sym = w.clseq[k] & 255, extra = w.clseq[k] >> 8;
        put_bits(w, w.code_cl[sym], w.len_cl[sym]);
        if (sym >= 16) put_bits(w, extra, cl_extra_bits(sym));
    }
}

// a token's bit string: -> its length (<= 48), *v = the bits
CLAIR_DEF_FN uint32_t token_bits(const Work &w, uint32_t tok, uint64_t *v) {
    if (!(tok >> 31)) {
        *v = w.code_ll[tok & 255];
        return w.len_ll[tok & 255];
    }
    uint32_t ls, leb, lev, ds, deb, dev;
    length_symbol(((tok >> 16) & 255) + 3, &ls, &leb, &lev);
    distance_symbol((tok & 0x7fff) + 1, &ds, &deb, &dev);
    uint32_t at = 0;
    uint64_t bits = w.code_ll[ls];
    at += w.len_ll[ls];
    bits |= (uint64_t)lev << at;
    at += leb;
    bits |= (uint64_t)w.code_d[ds] << at;
    at += w.len_d[ds];
    bits |= (uint64_t)dev << at;
    at += deb;
    *v = bits;
    return at;
}

// a byte of the block in its stored form (n input bytes): header, 01 LEN NLEN, the input, CRC-32, ISIZE
CLAIR_DEF_FN uint32_t stored_byte(const Work &w, uint32_t n, uint32_t k) {
    const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    const uint8_t *in = (const uint8_t *)w.in32;
    const uint32_t bsize = 18 + 5 + n + 8 - 1;
    if (k < 16) return head[k];
    if (k < 18) return (bsize >> (8 * (k - 16))) & 255;
    if (k == 18) return 1;
    if (k < 21) return (n >> (8 * (k - 19))) & 255;
    if (k < 23) return ((n ^ 0xffff) >> (8 * (k - 21))) & 255;
    if (k < 23 + n) return in[k - 23];
    if (k < 27 + n) return (w.crc >> (8 * (k - 23 - n))) & 255;
    if (k < 31 + n) return (n >> (8 * (k - 27 - n))) & 255;
    return 0;
}

CLAIR_DEF_FN uint32_t load4(const uint8_t *in, uint32_t at) {
    return (uint32_t)in[at] | (uint32_t)in[at + 1] << 8 | (uint32_t)in[at + 2] << 16 | (uint32_t)in[at + 3] << 24;
}

// -- regions --------------------------------------------------------------------------------------------------------------------------
template <class Ctx>
CLAIR_DEF_FN void or_bits32(Ctx &c, Work &w, uint32_t rel, uint32_t x) {
    const uint32_t i = rel >> 5, sh = rel & 31;
    if (x << sh) c.or_word(&w.stage[i], x << sh);
    if (sh && (x >> (32 - sh))) c.or_word(&w.stage[i + 1], x >> (32 - sh));
}

// the complete words of the staging window go out; the word being filled becomes stage[0]
template <class Ctx>
CLAIR_DEF_FN void flush(Ctx &c, Work &w) {
    const uint32_t w0 = c.uniform(w.w0), done = (c.uniform(w.bitpos) >> 5) - w0;       // done <= STAGE_WORDS + 1
    CLAIR_DEF_LANES(c, lane)
        for (uint32_t i = lane; i < done; i += LANES) c.store_word(w0 + i, w.stage[i]);
    c.sync();
    const uint32_t part = c.uniform(w.stage[done]);
    c.sync();
    CLAIR_DEF_LANES(c, lane)
        for (uint32_t i = lane; i < done + 2 && i < STAGE_WORDS + 2; i += LANES) w.stage[i] = 0;
    c.sync();
    CLAIR_DEF_ONE(c) {
        w.stage[0] = part;
        w.w0 = w0 + done;
    }
    c.sync();
}

template <class Ctx>
CLAIR_DEF_FN void ensure_room(Ctx &c, Work &w, uint32_t bits) {          // bits <= HEADER_ROOM
    if (c.uniform(w.bitpos) - c.uniform(w.w0) * 32 + bits > STAGE_WORDS * 32) flush(c, w);
}

// one step of 64 positions from `base` (a multiple of 64 below n): matches measured, table updated, tokens appended
template <class Ctx>
CLAIR_DEF_FN void match_step(Ctx &c, Work &w, uint32_t n, uint32_t base) {
    const uint8_t *in = (const uint8_t *)w.in32;
    CLAIR_DEF_LANES(c, lane) {
        const uint32_t p = base + lane;
        uint32_t h = EMPTY;
        if (p + MIN_MATCH <= n) {
            h = (load4(in, p) * 2654435761u) >> (32 - HASH_BITS);
        }
        w.m_hash[lane] = (uint16_t)h;
    }
    c.sync();
    CLAIR_DEF_LANES(c, lane) {
        const uint32_t p = base + lane, h = w.m_hash[lane];
        uint32_t len = 0, dist = 0, top = 0;
        if (h != EMPTY) {
            uint32_t cand = w.table[h];          // the table as it was before this step ...
            uint16_t nearest = 0, higher = 0;    // a fixed trip count and no branch: the host compiler vectorises it
            for (uint32_t k = 0; k < LANES; ++k) {
                const uint16_t same = w.m_hash[k] == h ? 0xffff : 0, below = k < lane ? 0xffff : 0, above = k > lane ? 1 : 0;
                const uint16_t mine = (uint16_t)(k + 1) & same & below;
                nearest = mine > nearest ? mine : nearest;
                higher |= same & above;
            }
            if (nearest) cand = base + nearest - 1;   // ... unless a lower lane of the step has the hash: the nearest one
            top = higher ^ 1;
            if (cand != EMPTY && cand < p && p - cand <= MAX_DIST && p >= w.cover) {
                const uint32_t most = n - p < MAX_MATCH ? n - p : MAX_MATCH;
                uint32_t l = 0, x = 0;           // four bytes a turn: the loads of a turn do not wait for each other
                while (l + 4 <= most && (x = load4(in, cand + l) ^ load4(in, p + l)) == 0) l += 4;
                if (x) l += (uint32_t)__builtin_ctz(x) >> 3;
                else while (l < most && in[cand + l] == in[p + l]) ++l;
                if (l >= MIN_MATCH) { len = l; dist = p - cand; }
            }
        }
        w.m_len[lane] = (uint16_t)len;
        w.m_dist[lane] = (uint16_t)(dist - (dist ? 1 : 0));
        w.m_top[lane] = (uint8_t)top;
    }
    c.sync();
    CLAIR_DEF_LANES(c, lane)
        if (w.m_top[lane]) w.table[w.m_hash[lane]] = (uint16_t)(base + lane);
    // the greedy walk: which positions of the step start a token.  The same in every lane; one turn per token, at most 64
    const uint32_t cover0 = c.uniform(w.cover), nt0 = c.uniform(w.ntok), limit = n - base < LANES ? n - base : LANES;
    uint64_t taken = 0;
    uint32_t l = cover0 > base ? cover0 - base : 0;
    while (l < limit) {
        taken |= 1ull << l;
        const uint32_t len = c.uniform(w.m_len[l]);
        l += len ? len : 1;
    }
    CLAIR_DEF_LANES(c, lane) {
        if (!((taken >> lane) & 1)) continue;
        const uint32_t at = nt0 + (uint32_t)__builtin_popcountll(taken & ((1ull << lane) - 1)), len = w.m_len[lane];
        if (at < TOK_MAX) w.tok[at] = len ? 1u << 31 | (len - 3) << 16 | w.m_dist[lane] : in[base + lane];
    }
    CLAIR_DEF_ONE(c) {
        w.cover = base + l > cover0 ? base + l : cover0;
        w.ntok = nt0 + (uint32_t)__builtin_popcountll(taken);
    }
    c.sync();
}

// The BGZF block of the n <= 65280 bytes in w.in32, through c.store_word / c.store_bsize.  -> its size in bytes (the same in every lane)
template <class Ctx>
CLAIR_DEF_FN uint32_t deflate_bgzf(Ctx &c, uint32_t n) {
    Work &w = c.work();
    const uint8_t *in = (const uint8_t *)w.in32;
    CLAIR_DEF_LANES(c, lane) {
        for (uint32_t i = lane; i < (1u << HASH_BITS); i += LANES) w.table[i] = (uint16_t)EMPTY;
        for (uint32_t i = lane; i < STAGE_WORDS + 2; i += LANES) w.stage[i] = 0;
        for (uint32_t i = lane; i < 256; i += LANES) w.crc_table[i] = clair_inf::crc_table_entry(i);
    }
    CLAIR_DEF_ONE(c) {
        w.bitpos = 0; w.w0 = 0; w.cover = 0; w.stored = 0; w.ntok = 0; w.extra_bits = 0; w.n_clseq = 0; w.crc = 0;
    }
    c.sync();
    CLAIR_DEF_LANES(c, lane) {
        const auto byte_at = [in](uint32_t i) { return (uint32_t)in[i]; };
        w.nb[lane] = clair_inf::crc_lane_share(byte_at, w.crc_table, n, lane, LANES);
    }
    c.sync();
    CLAIR_DEF_ONE(c) {
        uint32_t acc = clair_inf::crc_init_share(n);
        for (uint32_t l = 0; l < LANES; ++l) acc ^= w.nb[l];
        w.crc = ~acc;
        for (uint32_t k = 0; k < 16; ++k) put_bits(w, stored_byte(w, n, k), 8);       // the 16 constant header bytes
        put_bits(w, 0, 16);                                                           // BSIZE: store_bsize, at the end
    }
    c.sync();

    uint32_t pos = 0;
    for (;;) {                                   // every turn takes at least 64 positions, or is the last
        CLAIR_DEF_LANES(c, lane) {
            for (uint32_t s = lane; s < 288; s += LANES) w.freq_ll[s] = 0;
            if (lane < 32) w.freq_d[lane] = 0;
        }
        CLAIR_DEF_ONE(c) { w.ntok = 0; w.extra_bits = 0; }
        c.sync();
        while (pos < n && c.uniform(w.ntok) + LANES <= TOK_MAX) {
            match_step(c, w, n, pos);
            pos += LANES;
        }
        const uint32_t ntok = c.uniform(w.ntok), final_block = pos >= n ? 1u : 0u;
        CLAIR_DEF_LANES(c, lane) {
            for (uint32_t i = lane; i < ntok; i += LANES) {
                const uint32_t tok = w.tok[i];
                if (!(tok >> 31)) {
                    c.add_word(&w.freq_ll[tok & 255], 1);
                } else {
                    uint32_t ls, leb, lev, ds, deb, dev;
                    length_symbol(((tok >> 16) & 255) + 3, &ls, &leb, &lev);
                    distance_symbol((tok & 0x7fff) + 1, &ds, &deb, &dev);
                    c.add_word(&w.freq_ll[ls], 1);
                    c.add_word(&w.freq_d[ds], 1);
                    if (leb + deb) c.add_word(&w.extra_bits, leb + deb);
                }
            }
            if (lane == 0) c.add_word(&w.freq_ll[256], 1);
        }
        c.sync();
        ensure_room(c, w, HEADER_ROOM);
        CLAIR_DEF_ONE(c) {
            uint32_t hlit, hdist, hclen;
            const uint32_t bits = plan_block(w, &hlit, &hdist, &hclen);
            if ((w.bitpos + bits + 7) / 8 >= 18 + 5 + n) w.stored = 1;      // the stream so far, with this block, is no smaller than stored
            else put_block_header(w, final_block, hlit, hdist, hclen);
        }
        c.sync();
        if (c.uniform(w.stored)) break;
        for (uint32_t g = 0; g < ntok; g += LANES) {
            ensure_room(c, w, LANES * TOKEN_BITS);
            CLAIR_DEF_LANES(c, lane) {
                uint64_t v = 0;
                w.nb[lane] = g + lane < ntok ? token_bits(w, w.tok[g + lane], &v) : 0;
            }
            c.sync();
            CLAIR_DEF_LANES(c, lane) {
                if (g + lane >= ntok) continue;
                uint32_t before = 0;
                for (uint32_t k = 0; k < lane; ++k) before += w.nb[k];
                uint64_t v = 0;
                (void)token_bits(w, w.tok[g + lane], &v);
                const uint32_t rel = w.bitpos - w.w0 * 32 + before;
                or_bits32(c, w, rel, (uint32_t)v);
                if (v >> 32) or_bits32(c, w, rel + 32, (uint32_t)(v >> 32));
            }
            c.sync();
            CLAIR_DEF_ONE(c) {
                uint32_t total = 0;
                for (uint32_t k = 0; k < LANES; ++k) total += w.nb[k];
                w.bitpos += total;
            }
            c.sync();
        }
        ensure_room(c, w, 128);
        CLAIR_DEF_ONE(c) {
            put_bits(w, w.code_ll[256], w.len_ll[256]);
            if (final_block) {
                w.bitpos = (w.bitpos + 7) & ~7u;
                put_bits(w, w.crc, 32);
                put_bits(w, n, 32);
            }
        }
        c.sync();
        if (final_block) break;
    }

    if (c.uniform(w.stored)) {
        const uint32_t csize = 18 + 5 + n + 8;
        c.fence();                               // the words flushed so far are overwritten
        CLAIR_DEF_LANES(c, lane)
            for (uint32_t j = lane; j * 4 < csize; j += LANES)
                c.store_word(j, stored_byte(w, n, 4 * j) | stored_byte(w, n, 4 * j + 1) << 8 | stored_byte(w, n, 4 * j + 2) << 16 | stored_byte(w, n, 4 * j + 3) << 24);
        return csize;
    }
    const uint32_t csize = c.uniform(w.bitpos) >> 3;                     // a whole number of bytes
    CLAIR_DEF_ONE(c) { w.bitpos = (w.bitpos + 31) & ~31u; }              // the last word goes out whole
    c.sync();
    flush(c, w);
    c.fence();
    CLAIR_DEF_ONE(c) { c.store_bsize(csize - 1); }
    return csize;
}

}  // namespace clair_def
#endif
