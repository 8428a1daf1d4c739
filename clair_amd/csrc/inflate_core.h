// One RFC 1951 (DEFLATE) decoder for one raw stream, compiled twice: by g++ into libclair_host.so (clair_host_inflate_block, the twin
// that is tested, fuzzed and run under the host sanitizer) and by hipcc into inflate_bgzf_kernel (csrc/inflate.hip), a wave per stream.
// Plain C++17: no HIP type appears here.  The includer may define CLAIR_INF_FN (`__device__ inline` on the device).
//
// Everything that touches memory goes through a context object, so the device can hand the input staging and the copies to the wave:
//   uint32_t word(uint32_t i)                      input bytes [4i, 4i + 4) little-endian, bytes at or beyond the stream's end read as 0
//   void put(uint32_t pos, uint32_t byte)          one literal
//   void copy(uint32_t pos, uint32_t dist, uint32_t len)     a match: out[pos + k] = out[pos - dist + k % dist], k < len
//   void stored(uint32_t pos, uint32_t at, uint32_t len)     out[pos + k] = input byte at + k
//   uint32_t uniform(uint32_t v)                   v, known to be the same in every lane (the device: readfirstlane)
//   uint32_t lane(), lanes()                       this lane and how many share the work (host: 0 of 1)
//   void sync()                                    the lanes' writes to the tables become visible to each other
//   Tables &tables()
// Control flow is the same in every lane: every lane runs the symbol loop on the same values, lane 0 stores.
//
// Acceptance is zlib's inflate(Z_FINISH) with windowBits = -15 on a fresh stream with the whole output buffer given at once:
//   block type 3, LEN != ~NLEN, HLIT > 286 or HDIST > 30, an over-subscribed code set, an incomplete one unless its longest code is one
//   bit long (no distance code at all is fine until one is used; the code-length code must be complete), a repeat with no previous
//   length or running past HLIT + HDIST, no end-of-block code, the unused code of an incomplete set, literal/length symbols 286 and 287,
//   distance symbols 30 and 31, a distance beyond the bytes produced, input that ends before the final block does, output beyond `cap`:
//   all errors.  Input left over after the final block is not looked at.
// Totality: every bit consumed is counted against the stream's length (Bits::left) and every loop consumes at least one bit per turn or
// is counted; word() is only asked for words that start inside the stream; every table index is masked or compared first; put / copy /
// stored are only called for positions below `cap`.
#ifndef CLAIR_INFLATE_CORE_H
#define CLAIR_INFLATE_CORE_H

#include <stdint.h>

#ifndef CLAIR_INF_FN
#define CLAIR_INF_FN inline
#endif

namespace clair_inf {

constexpr int LIT_ROOT = 10, DIST_ROOT = 8;      // bits the one-probe tables resolve; longer codes take the canonical walk
constexpr uint32_t CRC_POLY = 0xedb88320u;       // CRC-32 (IEEE 802.3), reflected

// per-block status of a BGZF block (the host reader's three messages)
enum { BGZF_OK = 0, BGZF_CORRUPT = 1, BGZF_SIZE = 2, BGZF_CRC = 3 };

struct Code {                                    // a canonical Huffman code: symbols sorted by (length, symbol)
    uint16_t count[16];                          // codes of each length
    uint16_t first[16];                          // the first code of each length
    uint16_t offs[16];                           // where that length's symbols start in sym[]
    uint16_t sym[288];
};

struct Tables {
    uint16_t lit_fast[1 << LIT_ROOT];            // length << 9 | symbol for codes of at most LIT_ROOT bits, indexed by the next bits; 0 = walk
    uint16_t dist_fast[1 << DIST_ROOT];
    Code lit, dist;                              // lit doubles as the code-length code while a dynamic header is read
    uint8_t lens[320];                           // 286 + 30 code lengths; the fixed code uses 288 + 32
};

struct Bits {
    uint64_t buf;
    uint32_t cnt;                                // valid bits in buf
    uint32_t next;                               // next input word
    uint32_t left;                               // bits of the stream not yet consumed
};

template <class Ctx>
CLAIR_INF_FN void need(Ctx &c, Bits &b, uint32_t n_in) {     // at least 32 bits in buf (zeros beyond the stream)
    if (b.cnt < 32) {
        const uint32_t w = (uint64_t)b.next * 4 < n_in ? c.word(b.next) : 0u;
        b.next += 1;
        b.buf |= (uint64_t)w << b.cnt;
        b.cnt += 32;
    }
}

CLAIR_INF_FN bool drop(Bits &b, uint32_t n) {                // n <= 32, after need()
    if (n > b.left) return false;
    b.buf >>= n;
    b.cnt -= n;
    b.left -= n;
    return true;
}

template <class Ctx>
CLAIR_INF_FN void seek(Ctx &c, Bits &b, uint32_t n_in, uint32_t byte_at) {   // byte_at <= n_in
    b.buf = 0;
    b.cnt = 0;
    b.next = byte_at >> 2;
    b.left = (n_in - byte_at) * 8 + (byte_at & 3) * 8;
    need(c, b, n_in);
    (void)drop(b, (byte_at & 3) * 8);
}

// lens[0..n) -> code.  Returns what is left of the code space (0 complete, > 0 incomplete, < 0 over-subscribed); *max_len = longest code.
// Lane 0 sorts, the caller syncs.
template <class Ctx>
CLAIR_INF_FN int build_code(Ctx &c, Code &code, const uint8_t *lens, uint32_t n, uint32_t *max_len) {
    if (c.lane() == 0) {
        for (int l = 0; l < 16; ++l) code.count[l] = 0;
        for (uint32_t s = 0; s < n; ++s) code.count[lens[s] & 15] += 1;
        uint32_t at = 0, first = 0;
        code.offs[0] = 0; code.first[0] = 0;
        for (int l = 1; l < 16; ++l) {
            code.offs[l] = (uint16_t)at;
            code.first[l] = (uint16_t)first;     // of an over-subscribed set this wraps; such a set is never decoded with
            at += code.count[l];
            first = (first + code.count[l]) << 1;
        }
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t l = lens[s] & 15;
            if (l) code.sym[code.offs[l]++] = (uint16_t)s;   // at most n <= 288 entries in all
        }
        for (int l = 1; l < 16; ++l) code.offs[l] -= code.count[l];
    }
    c.sync();
    int left = 1;
    uint32_t mx = 0;
    for (int l = 1; l < 16; ++l) {
        const uint32_t k = c.uniform(code.count[l]);
        left = (left << 1) - (int)k;
        if (left < 0) return left;
        if (k) mx = (uint32_t)l;
    }
    *max_len = mx;
    return left;
}

CLAIR_INF_FN uint32_t bit_reverse(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) { r = r << 1 | (v & 1); v >>= 1; }
    return r;
}

// the one-probe table of a code: the lanes share the symbols
template <class Ctx>
CLAIR_INF_FN void build_fast(Ctx &c, const Code &code, const uint8_t *lens, uint32_t n, uint16_t *fast, uint32_t root) {
    const uint32_t size = 1u << root;
    for (uint32_t i = c.lane(); i < size; i += c.lanes()) fast[i] = 0;
    c.sync();
    uint32_t used = 0;
    for (int l = 1; l < 16; ++l) used += c.uniform(code.count[l]);
    if (used > 288) used = 288;
    for (uint32_t i = c.lane(); i < used; i += c.lanes()) {
        const uint32_t s = code.sym[i] & 511;
        const uint32_t l = s < n ? (lens[s] & 15) : 0;
        if (l == 0 || l > root) continue;
        const uint32_t value = (uint32_t)code.first[l] + (i - code.offs[l]);
        for (uint32_t k = bit_reverse(value, l) & (size - 1); k < size; k += 1u << l) fast[k] = (uint16_t)(l << 9 | s);
    }
    c.sync();
}

// the canonical walk over the next 15 bits: -> symbol, *len = its code's length; -1 when no code matches (incomplete set)
template <class Ctx>
CLAIR_INF_FN int walk(Ctx &c, const Code &code, uint32_t bits15, uint32_t *len) {
    uint32_t value = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        value |= bits15 & 1;
        bits15 >>= 1;
        const uint32_t count = c.uniform(code.count[l]);
        if (value - first < count) {             // unsigned: value >= first always holds here
            *len = l;
            const uint32_t at = index + (value - first);
            return at < 288 ? (int)c.uniform(code.sym[at]) : -1;
        }
        index += count;
        first = (first + count) << 1;
        value <<= 1;
    }
    return -1;
}

template <class Ctx>
CLAIR_INF_FN int decode(Ctx &c, const Code &code, const uint16_t *fast, uint32_t root, Bits &b) {   // after need(); -1 = error
    const uint32_t bits15 = (uint32_t)b.buf & 0x7fff;
    const uint32_t e = c.uniform(fast[bits15 & ((1u << root) - 1)]);
    uint32_t len = e >> 9;
    int sym = (int)(e & 511);
    if (e == 0) sym = walk(c, code, bits15, &len);
    if (sym < 0 || !drop(b, len)) return -1;
    return sym;
}

// the dynamic block's header: code lengths into t.lens, the two codes and their tables built.  false = error
template <class Ctx>
CLAIR_INF_FN bool dynamic_header(Ctx &c, Tables &t, Bits &b, uint32_t n_in, uint32_t *n_lit, uint32_t *n_dist) {
    need(c, b, n_in);
    const uint32_t nlen = ((uint32_t)b.buf & 31) + 257, ndist = ((uint32_t)(b.buf >> 5) & 31) + 1, ncode = ((uint32_t)(b.buf >> 10) & 15) + 4;
    if (!drop(b, 14)) return false;
    if (nlen > 286 || ndist > 30) return false;
    // code-length code lengths, in their permuted order (RFC 1951 3.2.7), 3 bits each
    uint64_t packed = 0;                         // 19 lengths of 3 bits, by symbol
    for (uint32_t i = 0; i < ncode; ++i) {
        need(c, b, n_in);
        const uint32_t v = (uint32_t)b.buf & 7;
        if (!drop(b, 3)) return false;
        // position -> symbol: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const uint32_t s = i < 3 ? 16 + i : (i & 1) ? (i == 3 ? 0 : 8 - ((i - 3) >> 1)) : 7 + ((i - 2) >> 1);
        packed |= (uint64_t)v << (3 * s);
    }
    if (c.lane() == 0)
        for (uint32_t s = 0; s < 19; ++s) t.lens[s] = (uint8_t)(packed >> (3 * s) & 7);
    c.sync();
    uint32_t mx = 0;
    if (build_code(c, t.lit, t.lens, 19, &mx) != 0) return false;      // the code-length code must be complete
    // the literal/length and distance code lengths, run-length coded with it
    uint32_t have = 0, prev = 0;
    const uint32_t total = nlen + ndist;
    // the walk reads only count / sym of the code-length code, so its own lengths in t.lens[0..19) may be overwritten now
    while (have < total) {                       // every turn consumes at least one bit
        need(c, b, n_in);
        uint32_t len = 0;
        const int sym = walk(c, t.lit, (uint32_t)b.buf & 0x7fff, &len);
        if (sym < 0 || !drop(b, len)) return false;
        uint32_t value = 0, repeat = 1;
        if (sym < 16) {
            value = (uint32_t)sym;
        } else {
            uint32_t extra, base;
            if (sym == 16) { if (have == 0) return false; value = prev; extra = 2; base = 3; }
            else if (sym == 17) { extra = 3; base = 3; }
            else { extra = 7; base = 11; }
            need(c, b, n_in);
            repeat = base + ((uint32_t)b.buf & ((1u << extra) - 1));
            if (!drop(b, extra)) return false;
            if (have + repeat > total) return false;
        }
        if (c.lane() == 0)
            for (uint32_t k = 0; k < repeat; ++k) t.lens[have + k] = (uint8_t)value;   // have + repeat <= total <= 316
        have += repeat;
        prev = value;
    }
    c.sync();
    if (c.uniform(t.lens[256]) == 0) return false;           // no end-of-block code
    *n_lit = nlen;
    *n_dist = ndist;
    return true;
}

// the two codes of a block from t.lens[0..n_lit) and t.lens[n_lit..n_lit + n_dist).  false = a set zlib refuses
template <class Ctx>
CLAIR_INF_FN bool build_block_codes(Ctx &c, Tables &t, uint32_t n_lit, uint32_t n_dist) {
    uint32_t mx = 0;
    int left = build_code(c, t.lit, t.lens, n_lit, &mx);
    if (left < 0 || (left > 0 && mx != 1)) return false;
    build_fast(c, t.lit, t.lens, n_lit, t.lit_fast, LIT_ROOT);
    left = build_code(c, t.dist, t.lens + n_lit, n_dist, &mx);
    if (left < 0 || (left > 0 && mx > 1)) return false;      // no distance code at all (mx == 0) is an error only when one is used
    build_fast(c, t.dist, t.lens + n_lit, n_dist, t.dist_fast, DIST_ROOT);
    return true;
}

// the symbols of one compressed block.  false = error
template <class Ctx>
CLAIR_INF_FN bool symbols(Ctx &c, Tables &t, Bits &b, uint32_t n_in, uint32_t cap, uint32_t *produced) {
    uint32_t out = *produced;
    for (;;) {                                   // every turn consumes at least one bit
        need(c, b, n_in);
        const int sym = decode(c, t.lit, t.lit_fast, LIT_ROOT, b);
        if (sym < 0) return false;
        if (sym < 256) {
            if (out >= cap) return false;
            c.put(out, (uint32_t)sym);
            out += 1;
            continue;
        }
        if (sym == 256) break;
        if (sym >= 286) return false;
        uint32_t len, extra;
        if (sym < 265) { len = (uint32_t)sym - 254; extra = 0; }
        else if (sym == 285) { len = 258; extra = 0; }
        else { extra = ((uint32_t)sym - 261) >> 2; len = 3 + ((4 + (((uint32_t)sym - 265) & 3)) << extra); }
        len += (uint32_t)b.buf & ((1u << extra) - 1);
        if (!drop(b, extra)) return false;
        need(c, b, n_in);
        const int dsym = decode(c, t.dist, t.dist_fast, DIST_ROOT, b);
        if (dsym < 0 || dsym >= 30) return false;
        uint32_t dist;
        if (dsym < 4) { dist = (uint32_t)dsym + 1; extra = 0; }
        else { extra = ((uint32_t)dsym >> 1) - 1; dist = 1 + ((2 + ((uint32_t)dsym & 1)) << extra); }
        dist += (uint32_t)b.buf & ((1u << extra) - 1);
        if (!drop(b, extra)) return false;
        if (dist > out) return false;            // beyond the bytes produced so far
        if (len > cap - out) return false;       // out <= cap
        c.copy(out, dist, len);
        out += len;
    }
    *produced = out;
    return true;
}

// One raw deflate stream: input bytes [start, n_in) of what word() serves (the device serves from the 16-byte boundary below the stream).
// -> true when the final block ended with at most `cap` bytes produced; *produced = their count.
template <class Ctx>
CLAIR_INF_FN bool inflate(Ctx &c, uint32_t start, uint32_t n_in, uint32_t cap, uint32_t *produced) {
    Tables &t = c.tables();
    Bits b;
    seek(c, b, n_in, start);
    uint32_t out = 0;
    *produced = 0;
    for (;;) {                                   // every block consumes at least three bits
        need(c, b, n_in);
        const uint32_t final_block = (uint32_t)b.buf & 1, type = (uint32_t)(b.buf >> 1) & 3;
        if (!drop(b, 3)) return false;
        if (type == 0) {
            if (!drop(b, b.left & 7)) return false;          // to the byte boundary: left counts bits up to the stream's end, a whole byte count
            need(c, b, n_in);
            const uint32_t len = (uint32_t)b.buf & 0xffff, nlen = (uint32_t)(b.buf >> 16) & 0xffff;
            if (!drop(b, 32)) return false;
            if (len != (nlen ^ 0xffff)) return false;
            if (len > (b.left >> 3)) return false;
            if (len > cap - out) return false;
            const uint32_t at = n_in - (b.left >> 3);
            if (len) c.stored(out, at, len);
            out += len;
            seek(c, b, n_in, at + len);
        } else if (type == 3) {
            return false;
        } else {
            uint32_t n_lit = 288, n_dist = 32;
            if (type == 1) {
                for (uint32_t s = c.lane(); s < 320; s += c.lanes())
                    t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                c.sync();
            } else if (!dynamic_header(c, t, b, n_in, &n_lit, &n_dist)) {
                return false;
            }
            if (!build_block_codes(c, t, n_lit, n_dist)) return false;
            if (!symbols(c, t, b, n_in, cap, &out)) return false;
        }
        if (final_block) break;
    }
    *produced = out;
    return true;
}

// -- CRC-32 over `n` bytes, split over `lanes` chunks whose raw remainders are combined by multiplication modulo the polynomial.
// In the reflected representation bit 31 is x^0.
CLAIR_INF_FN uint32_t crc_mul(uint32_t a, uint32_t b) {      // a * b mod P
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? CRC_POLY : 0u);
    }
    return p;
}

CLAIR_INF_FN uint32_t crc_xpow8(uint32_t n) {                // x^(8 n) mod P
    uint32_t r = 0x80000000u, base = 0x00800000u;            // 1, x^8
    for (int i = 0; i < 32 && n; ++i, n >>= 1) {
        if (n & 1) r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}

CLAIR_INF_FN uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1) ? CRC_POLY : 0u);
    return i;
}

// bytes per lane: a whole number of dwords, an odd one (the lanes' dword reads then fall on different LDS banks)
CLAIR_INF_FN uint32_t crc_chunk(uint32_t n, uint32_t lanes) {
    uint32_t dwords = ((n + lanes - 1) / lanes + 3) / 4;
    dwords |= 1;
    return dwords * 4;
}

// lane's share of the CRC: the raw remainder of its chunk moved to the chunk's place in the message; the lanes' shares, the share of the
// initial value (crc_init_share) and the final inversion make the CRC:  crc = ~(crc_init_share(n) ^ xor of crc_lane_share)
template <class Byte>
CLAIR_INF_FN uint32_t crc_lane_share(const Byte &byte_at, const uint32_t *table, uint32_t n, uint32_t lane, uint32_t lanes) {
    const uint32_t chunk = crc_chunk(n, lanes);
    const uint32_t beg = lane * chunk < n ? lane * chunk : n, end = beg + chunk < n ? beg + chunk : n;
    uint32_t r = 0;
    for (uint32_t i = beg; i < end; ++i) r = table[(r ^ byte_at(i)) & 255] ^ (r >> 8);
    return end > beg ? crc_mul(crc_xpow8(n - end), r) : 0u;
}

CLAIR_INF_FN uint32_t crc_init_share(uint32_t n) { return crc_mul(crc_xpow8(n), 0xffffffffu); }

CLAIR_INF_FN int bgzf_status(bool ended, uint32_t produced, uint32_t isize, uint32_t crc, uint32_t want) {
    if (!ended) return BGZF_CORRUPT;
    if (produced != isize) return BGZF_SIZE;
    return crc == want ? BGZF_OK : BGZF_CRC;
}

// (host side only, as what follows) the verdicts as words; a status that is none of them reads as the first
inline const char *bgzf_status_text(int status) {
    static const char *const what[] = {"corrupt deflate data", "inflated size differs from ISIZE", "CRC32 mismatch"};
    return what[status >= BGZF_CORRUPT && status <= BGZF_CRC ? status - 1 : 0];
}

// A batch of block descriptors before anything reads through them: n within max_blocks, each block's csize and out_len those of a BGZF block
// and its compressed bytes inside the cbytes given.  -> 0, or what `fail` (printf-style: a HipFail, clair_host_fail) returns for the first breach.
template <class Fail>
inline int check_blocks(const Fail &fail, int n, int max_blocks, int64_t cbytes, const int64_t *in_at, const int32_t *csize, const int32_t *out_len) {
    if (n < 0 || n > max_blocks) return fail("%d blocks in a batch: 0 .. max_blocks = %d", n, max_blocks);
    for (int i = 0; i < n; ++i) {
        if (csize[i] < 26 || csize[i] > 65536) return fail("block %d: csize %d (26 .. 65536)", i, csize[i]);
        if (in_at[i] < 0 || in_at[i] > cbytes - csize[i]) return fail("block %d: compressed bytes [%lld, +%d) outside the %lld given", i, (long long)in_at[i], csize[i], (long long)cbytes);
        if (out_len[i] < 0 || out_len[i] > 65536) return fail("block %d: out_len %d (0 .. 65536)", i, out_len[i]);
    }
    return 0;
}

}  // namespace clair_inf
#endif
