// Device front end of the C ABI (include/clair_amd.h, "front end"): `samtools view` text (or alignments already packed by the host,
// include/clair_reads.h) -> candidate sites -> pileup count windows [n][33][8][4] int16 that stay in HBM for clair_submit_ex.
// SURVEY.md 8(f) N4, the GPU half.
//
// What the reference does per read base in two interpreters (dataPrepScripts/ExtractVariantCandidates.py:296-316: a dict of
// per-position tallies; CreateTensor.py:289-365 + :29-65: a tuple per (read base, open window), summed when the window is written)
// is done here per reference POSITION: one thread per read base adds to per-position tables with atomics (pass 1), the candidate
// filter runs over the tallies, one thread per read base counts the windows it lies in and scatters the inserted bases (pass 2), and
// the windows are assembled from 33 table columns each.  Why that is the same result -- and when it is not (a tuple budget that
// binds, unsorted input, bases outside the IUPAC alphabet: reported as CLAIR_FE_* bits, the caller then runs the sequential host
// code) -- is in oracle/frontend_np.py, the NumPy restatement these kernels are tested against, and in LABNOTES.md part B section 3 / 6b.
//
// All integer work, HBM/atomic bound: nothing here is a matrix product.  Tables are sized for the whole region and the packed reads
// stay resident (a 10 Mb region at 50x: ~0.7 GB of tables, 1.3 - 2.1 GB of reads; a whole chromosome fits the 288 GB many times over), so
// there is no streaming window to manage and pass 2 re-reads the reads from HBM instead of from the host.
#include "../../include/clair_amd.h"
#include "../../include/clair_reads.h"

#include <hip/hip_runtime.h>

#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"
#define CLAIR_REC_FN __device__ inline
#include "bam_record_core.h"
#include "subsample_core.h"
#define CLAIR_GVCF_FN __device__ __host__ inline
#include "gvcf_core.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

namespace {

thread_local std::string g_fe_error;

constexpr int N_POS = 33, N_ROW = 8, N_QUAD = N_POS * N_ROW;   // 264 (position, row) quads of four channels
constexpr int WINDOW_VALUES = N_QUAD * 4;                        // 1056

// IUPAC_base_to_num_dict (shared/utils.py:24-27) and IUPAC_base_to_ACGT_base_dict through evc_base_from (:19-22, 27-28; N stays N = 6);
// 255: not a key
struct BaseTables {
    uint8_t pile[256], evc[256];
    constexpr BaseTables() : pile(), evc() {
        for (int i = 0; i < 256; ++i) { pile[i] = 255; evc[i] = 255; }
        const char keys[17] = "ACGTURYSWKMBDHVN";
        const uint8_t rows[16] = {0, 1, 2, 3, 3, 0, 1, 1, 0, 2, 0, 1, 0, 0, 0, 0};
        const char acgt[17] = "ACGTTACCAGACAAAA";
        for (int i = 0; i < 16; ++i) {
            pile[(unsigned char)keys[i]] = rows[i];
            evc[(unsigned char)keys[i]] = (uint8_t)(acgt[i] == 'A' ? 0 : acgt[i] == 'C' ? 1 : acgt[i] == 'G' ? 2 : 3);
        }
        evc[(unsigned char)'N'] = 6;
        // both scripts upper-case SEQ first (EVC :301, CT :262): a slab parsed on the device keeps the text as samtools printed it
        for (int c = 'a'; c <= 'z'; ++c) { pile[c] = pile[c - 32]; evc[c] = evc[c - 32]; }
    }
};
__constant__ BaseTables BASES = BaseTables();

struct Region {          // what every kernel needs to know about the tables and the reference
    int64_t lo, n;       // tables cover 0-based positions [lo, lo + n)
    const uint8_t *ref;  // upper-cased reference bytes for [ref0, ref0 + ref_len)
    int64_t ref0, ref_len;
    // Per position and base row b (A C G T, IUPAC codes mapped as the scripts map them) ONE 64-bit word of three 21-bit counters, so that
    // a matched base costs one atomic: bits 0-20 pileup reads on the forward strand with read base b, 21-41 the same on the reverse
    // strand, 42-62 the candidate search's tally of b.  (Matched bases per strand = the sum over the four rows.)
    unsigned long long *pq;   // [n][4]
    uint32_t *misc;      // [n][8]  0,1 D per strand (rp > POS) | 2 D at rp == POS | 3 inserted bases (rp > POS) | 4 M at rp == POS | 5,6,7 the search's I, D, N tallies
    uint32_t *anomalies;
};

constexpr int PQ_BITS = 21;
constexpr unsigned long long PQ_MASK = (1ull << PQ_BITS) - 1;
__device__ inline uint32_t pq_field(unsigned long long w, int field) { return (uint32_t)((w >> (field * PQ_BITS)) & PQ_MASK); }

struct Slab {
    DeviceBuffer reads, ops, op_elem, seq;   // clair_read_t, clair_op_t, uint32_t [n_ops + 1], uint8_t
    DeviceBuffer tuples;                     // uint64_t per read, pass 2
    int64_t n_reads = 0, n_ops = 0, n_elem = 0, seq_bytes = 0;
};

struct SlabHostCopy { std::vector<clair_read_t> reads; std::vector<clair_op_t> ops; std::vector<uint8_t> seq; };   // indel look-up, host fallback

struct SlabView {
    const clair_read_t *reads;
    const clair_op_t *ops;
    const uint32_t *op_elem;
    const uint8_t *seq;
    uint64_t *tuples;
    uint32_t n_ops;
    uint32_t n_elem;
};

// the read base / deleted base a thread stands for
struct Element {
    clair_read_t r;
    int64_t rp;
    uint32_t qp, k, code, read;
};

__device__ inline Element element_of(const SlabView &s, uint32_t e) {
    uint32_t a = 0, b = s.n_ops;             // largest j with op_elem[j] <= e
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (s.op_elem[mid] <= e) a = mid; else b = mid;
    }
    const clair_op_t op = s.ops[a];
    Element el;
    el.read = op.read;
    el.r = s.reads[op.read];
    el.k = e - s.op_elem[a];
    el.code = op.code_len & 3u;
    el.rp = el.r.pos0 + op.ref_off + (el.code == CLAIR_OP_I ? 0 : (int64_t)el.k);
    el.qp = op.q_off + (el.code == CLAIR_OP_D ? 0u : el.k);
    return el;
}

__device__ inline uint8_t ref_row(const Region &g, int64_t p) {
    const int64_t i = p - g.ref0;
    return (i >= 0 && i < g.ref_len) ? BASES.pile[g.ref[i]] : (uint8_t)255;
}

__device__ inline void flag(const Region &g, uint32_t bit) { atomicOr(g.anomalies, bit); }

// ---- pass 1: the per-position tables ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fe_tally_kernel(Region g, SlabView s) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= s.n_elem) return;
    const Element el = element_of(s, e);
    const bool evc = el.r.flags & CLAIR_READ_EVC, pile = el.r.flags & CLAIR_READ_PILE;
    if (!evc && !pile) return;               // kept for the indel look-up only (CLAIR_READ_LOOKUP): neither stage walks it
    const int so = (el.r.flags & CLAIR_READ_REVERSE) ? 1 : 0;
    const int64_t t = el.rp - g.lo;
    const bool inside = t >= 0 && t < g.n;
    if (el.code == CLAIR_OP_M) {
        if (el.qp >= el.r.seq_len) { flag(g, CLAIR_FE_SEQ_OVERRUN); return; }
        if (pile && inside && ref_row(g, el.rp) == 255) flag(g, CLAIR_FE_BAD_REF);
        const uint8_t base = s.seq[el.r.seq0 + el.qp];
        const uint8_t ei = BASES.evc[base];
        if (ei == 255) { flag(g, CLAIR_FE_BAD_BASE); return; }
        if (!inside) return;
        // the search's base index and the pileup's row agree for every code but N (tally N, row of A)
        const int row = BASES.pile[base];
        unsigned long long add = pile ? 1ull << (so * PQ_BITS) : 0;
        if (evc && ei < 4) add += 1ull << (2 * PQ_BITS);
        if (add) {      // (the reply costs nothing measurable: the atomic unit at the memory side is the bound either way)
            const unsigned long long before = atomicAdd(&g.pq[t * 4 + row], add);
            if ((pile && pq_field(before, so) == PQ_MASK) || (evc && ei < 4 && pq_field(before, 2) == PQ_MASK))
                flag(g, CLAIR_FE_OVERFLOW);                     // a counter was full: 2 097 151 reads over one position
        }
        if (evc && ei >= 4) atomicAdd(&g.misc[t * 8 + 7], 1u);
        if (pile && el.rp == el.r.pos0) atomicAdd(&g.misc[t * 8 + 4], 1u);
    } else if (el.code == CLAIR_OP_I) {
        if (el.k == 0 && evc && t - 1 >= 0 && t - 1 < g.n) atomicAdd(&g.misc[(t - 1) * 8 + 5], 1u);   // once per operation, at the base before it
        if (!pile) return;
        if (el.qp >= el.r.seq_len) { flag(g, CLAIR_FE_SEQ_OVERRUN); return; }
        if (el.rp <= el.r.pos0) return;                                                              // no window is open yet (CreateTensor.py:326-341)
        if (BASES.pile[s.seq[el.r.seq0 + el.qp]] == 255) flag(g, CLAIR_FE_BAD_BASE);
        if (inside) atomicAdd(&g.misc[t * 8 + 3], 1u);
    } else {
        if (el.k == 0 && evc && t - 1 >= 0 && t - 1 < g.n) atomicAdd(&g.misc[(t - 1) * 8 + 6], 1u);
        if (!pile || !inside) return;
        if (ref_row(g, el.rp) == 255) flag(g, CLAIR_FE_BAD_REF);
        if (el.rp > el.r.pos0) atomicAdd(&g.misc[t * 8 + so], 1u);
        else atomicAdd(&g.misc[t * 8 + 2], 1u);
    }
}

// ---- pass 1 without a device-scope atomic per base (round 4) --------------------------------------------------
// fe_tally_kernel above sends one 32-byte atomic request per aligned base to the memory side of the L2 (3.3 GB per 102 M bases, ten times
// the text in plus tables out: the atomic unit is its bound).  Alignments come sorted by position, so the ~depth bases that land on one
// position are found together if the work is cut by POSITION instead of by base: a workgroup owns a tile of TT_POS table positions,
// keeps the tile's 64 bytes of counters per position in LDS, walks the part of every alignment that crosses the tile -- the alignments
// with POS in (tile start - longest span of the slab, tile end), found by bisection; each one's first operation in the tile by bisection
// in its operation list, all alignments of the tile at once, a thread each -- and adds its tile to the tables once: one atomic per
// non-zero counter word and tile (the neighbour's I / D tally at "the position before" may land in this tile's words at the same time).
// The tile of the first / last position also owns everything left / right of the tables: those bases tally nothing but are still
// examined (sequence overrun, bases outside the alphabet), as the per-base kernel does.
constexpr int TT_POS = 512;              // table positions per tile: 16 KB + 16 KB of counters
constexpr int TT_THREADS = 1024;
constexpr int TT_WAVES = TT_THREADS / 64;
constexpr int TT_LIST = TT_THREADS;      // alignments examined per round, one thread each

__global__ __launch_bounds__(256) void fe_slab_span_kernel(SlabView s, uint32_t n_reads, uint32_t *span) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_reads) return;
    const clair_read_t r = s.reads[i];
    if (!r.n_ops) return;
    const clair_op_t last = s.ops[r.op0 + r.n_ops - 1];
    const uint32_t len = last.code_len >> 2, code = last.code_len & 3u;
    const int64_t reach = (int64_t)last.ref_off + (code == CLAIR_OP_I ? 1 : (int64_t)len);      // positions pos0 .. pos0 + reach - 1 are touched
    atomicMax(span, (uint32_t)std::min<int64_t>(std::max<int64_t>(reach, 0), 0x7fffffff));
}

struct TileOp { int32_t rel; uint32_t code_len, q_off, first, k0; };    // an operation as the tile sees it: start relative to the tile, its first flat element, first k inside

__global__ __launch_bounds__(TT_THREADS) void fe_tally_tile_kernel(Region g, SlabView s, uint32_t n_reads, const uint32_t *slab_span, int64_t tile0) {
    __shared__ unsigned long long pq_l[TT_POS * 4];
    __shared__ uint32_t misc_l[TT_POS * 8];
    __shared__ uint2 list[TT_LIST];             // (alignment, its first operation that reaches into the tile)
    __shared__ uint32_t n_list;
    __shared__ TileOp opbuf[TT_WAVES][64];
    __shared__ uint8_t evc_l[256], pile_l[256];  // the base tables and the tile's reference rows next to the counters: what a base needs besides its own byte
    __shared__ uint8_t ref_l[TT_POS];            // is one LDS read away (from constant / global memory each is a dependent trip of its own)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the launch covers table tiles tile0 .. tile0 + gridDim.x - 1: where this slab's alignments lie (a guess is enough: the first and the last
    // workgroup own everything left / right of their tile, and tally what falls inside the tables but outside their LDS window straight into them)
    const int64_t t_lo = (tile0 + (int64_t)blockIdx.x) * TT_POS;
    const bool first = blockIdx.x == 0, last = blockIdx.x == gridDim.x - 1;
    const int64_t p_lo = first ? INT64_MIN / 4 : g.lo + t_lo, p_hi = last ? INT64_MAX / 4 : g.lo + t_lo + TT_POS;     // positions this tile owns
    const int64_t p_base = g.lo + t_lo;
    for (int i = tid; i < TT_POS * 4; i += TT_THREADS) pq_l[i] = 0ull;
    for (int i = tid; i < TT_POS * 8; i += TT_THREADS) misc_l[i] = 0u;
    if (tid < 256) { evc_l[tid] = BASES.evc[tid]; pile_l[tid] = BASES.pile[tid]; }
    else if (tid < 256 + TT_POS) ref_l[tid - 256] = ref_row(g, p_base + (tid - 256));
    // alignments that may reach into the tile: POS < p_hi, and POS + (longest reach of the slab) > p_lo
    const int64_t span = (int64_t)*slab_span;
    uint32_t ra = 0, rb = n_reads;
    if (!first) { uint32_t a = 0, b = n_reads; while (a < b) { const uint32_t m = (a + b) >> 1; if (s.reads[m].pos0 + span > p_lo) b = m; else a = m + 1; } ra = a; }
    if (!last) { uint32_t a = ra, b = n_reads; while (a < b) { const uint32_t m = (a + b) >> 1; if (s.reads[m].pos0 >= p_hi) b = m; else a = m + 1; } rb = a; }
    for (uint32_t base = ra; base < rb; base += TT_LIST) {
        if (tid == 0) n_list = 0u;
        __syncthreads();
        const uint32_t i = base + (uint32_t)tid;
        if (i < rb) {
            const clair_read_t r = s.reads[i];
            if (r.n_ops && r.pos0 < p_hi && (r.flags & (CLAIR_READ_EVC | CLAIR_READ_PILE))) {     // (not what is kept for the indel look-up only)
                // operations are ordered and their ends (start + length; an insertion counts as one position) never decrease: first one ending beyond p_lo
                uint32_t a = 0, b = r.n_ops;
                while (a < b) {
                    const uint32_t m = (a + b) >> 1;
                    const clair_op_t op = s.ops[r.op0 + m];
                    const int64_t end = r.pos0 + op.ref_off + ((op.code_len & 3u) == CLAIR_OP_I ? 1 : (int64_t)(op.code_len >> 2));
                    if (end > p_lo) b = m; else a = m + 1;
                }
                if (a < r.n_ops) list[atomicAdd(&n_list, 1u)] = make_uint2(i, r.op0 + a);
            }
        }
        __syncthreads();
        const uint32_t n = n_list;
        for (uint32_t li = (uint32_t)wave; li < n; li += TT_WAVES) {      // a wave per alignment
            const uint2 ent = list[li];
            const uint32_t ri = __builtin_amdgcn_readfirstlane(ent.x);
            const clair_read_t r = s.reads[ri];
            const bool evc = r.flags & CLAIR_READ_EVC, pile = r.flags & CLAIR_READ_PILE;
            const int so = (r.flags & CLAIR_READ_REVERSE) ? 1 : 0;
            const uint32_t jend = r.op0 + r.n_ops;
            for (uint32_t j = __builtin_amdgcn_readfirstlane(ent.y); j < jend; j += 64) {          // 64 operations at a time, one per lane
                const uint32_t jj = j + (uint32_t)lane;
                const bool valid = jj < jend;
                clair_op_t op{};
                if (valid) op = s.ops[jj];
                const uint32_t code = op.code_len & 3u, len = op.code_len >> 2;
                const int64_t start = r.pos0 + op.ref_off;
                const bool beyond = valid && start >= p_hi;
                const bool in = valid && !beyond && start + (code == CLAIR_OP_I ? 1 : (int64_t)len) > p_lo;
                uint32_t k0 = 0, k1 = 0;
                if (in) {
                    if (code == CLAIR_OP_I) { k1 = len; }
                    else { k0 = (uint32_t)std::max<int64_t>(0, p_lo - start); k1 = (uint32_t)std::min<int64_t>((int64_t)len, p_hi - start); }
                }
                const uint32_t cnt = k1 - k0;
                uint32_t incl = cnt;                       // inclusive prefix sum over the wave
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
                const uint32_t total = __shfl(incl, 63);
                opbuf[wave][lane] = TileOp{(int32_t)(start - p_base), op.code_len, op.q_off, incl - cnt, k0};
                // an element in two steps, so that two of them are in flight per lane: find its operation (LDS) and fetch its read base; tally
                struct Prep { int64_t lt; uint32_t oc, k, qp; uint8_t bs; };
                auto prep = [&](uint32_t e) {
                    int a = 0, b = 64;                     // last operation whose first flat element is <= e (empty ones share their successor's `first`: take the last)
                    while (b - a > 1) { const int m = (a + b) >> 1; if (opbuf[wave][m].first <= e) a = m; else b = m; }
                    const TileOp o = opbuf[wave][a];
                    Prep q;
                    q.oc = o.code_len & 3u;
                    q.k = o.k0 + (e - o.first);
                    q.lt = (int64_t)o.rel + (q.oc == CLAIR_OP_I ? 0 : (int64_t)q.k);   // position relative to the tile (outside [0, TT_POS) only in the first / last workgroup)
                    q.qp = o.q_off + (q.oc == CLAIR_OP_D ? 0u : q.k);
                    q.bs = (q.oc != CLAIR_OP_D && q.qp < r.seq_len) ? s.seq[r.seq0 + q.qp] : (uint8_t)0;
                    return q;
                };
                auto apply = [&](const Prep &q) {
                    const int64_t lt = q.lt, t = t_lo + lt, rp = p_base + lt;
                    const bool inside = t >= 0 && t < g.n;
                    auto row_of = [&](int64_t at, int64_t pos) -> uint8_t { return at >= 0 && at < TT_POS ? ref_l[at] : ref_row(g, pos); };
                    auto bump = [&](int64_t at, int word) {          // misc counter `word` of tile position `at`: the tile's copy, or the table itself
                        if (at >= 0 && at < TT_POS) atomicAdd(&misc_l[at * 8 + word], 1u); else atomicAdd(&g.misc[(t_lo + at) * 8 + word], 1u);
                    };
                    if (q.oc == CLAIR_OP_M) {
                        if (q.qp >= r.seq_len) { flag(g, CLAIR_FE_SEQ_OVERRUN); return; }
                        if (pile && inside && row_of(lt, rp) == 255) flag(g, CLAIR_FE_BAD_REF);
                        const uint8_t ei = evc_l[q.bs];
                        if (ei == 255) { flag(g, CLAIR_FE_BAD_BASE); return; }
                        if (!inside) return;
                        const int row = pile_l[q.bs];
                        unsigned long long add = pile ? 1ull << (so * PQ_BITS) : 0;
                        if (evc && ei < 4) add += 1ull << (2 * PQ_BITS);
                        if (add) {
                            if (lt >= 0 && lt < TT_POS) atomicAdd(&pq_l[lt * 4 + row], add);
                            else {
                                const unsigned long long before = atomicAdd(&g.pq[t * 4 + row], add);
                                if ((pile && pq_field(before, so) == PQ_MASK) || (evc && ei < 4 && pq_field(before, 2) == PQ_MASK)) flag(g, CLAIR_FE_OVERFLOW);
                            }
                        }
                        if (evc && ei >= 4) bump(lt, 7);
                        if (pile && rp == r.pos0) bump(lt, 4);
                    } else if (q.oc == CLAIR_OP_I) {
                        if (q.k == 0 && evc && t - 1 >= 0 && t - 1 < g.n) bump(lt - 1, 5);   // once per operation, at the base before it
                        if (!pile) return;
                        if (q.qp >= r.seq_len) { flag(g, CLAIR_FE_SEQ_OVERRUN); return; }
                        if (rp <= r.pos0) return;                                   // no window is open yet (CreateTensor.py:326-341)
                        if (pile_l[q.bs] == 255) flag(g, CLAIR_FE_BAD_BASE);
                        if (inside) bump(lt, 3);
                    } else {
                        if (q.k == 0 && evc && t - 1 >= 0 && t - 1 < g.n) bump(lt - 1, 6);
                        if (!pile || !inside) return;
                        if (row_of(lt, rp) == 255) flag(g, CLAIR_FE_BAD_REF);
                        bump(lt, rp > r.pos0 ? so : 2);
                    }
                };
                for (uint32_t e = (uint32_t)lane; e < total; e += 128) {
                    const Prep q0 = prep(e);
                    const bool two = e + 64 < total;
                    Prep q1 = q0;
                    if (two) q1 = prep(e + 64);
                    apply(q0);
                    if (two) apply(q1);
                }
                if (__ballot(beyond || !valid)) break;      // the rest of the alignment lies beyond the tile (or there is no rest)
            }
        }
        __syncthreads();
    }
    __syncthreads();
    // the tile into the tables: one atomic per counter word that moved
    for (int i = tid; i < TT_POS * 4; i += TT_THREADS) {
        const unsigned long long add = pq_l[i];
        const int64_t t = t_lo + (i >> 2);
        if (add && t >= 0 && t < g.n) {
            const unsigned long long before = atomicAdd(&g.pq[t * 4 + (i & 3)], add);
            for (int fld = 0; fld < 3; ++fld)
                if (pq_field(before, fld) + pq_field(add, fld) > PQ_MASK) flag(g, CLAIR_FE_OVERFLOW);       // a 21-bit counter ran over: 2 097 151 reads over one position
        }
    }
    for (int i = tid; i < TT_POS * 8; i += TT_THREADS) {
        const uint32_t add = misc_l[i];
        const int64_t t = t_lo + (i >> 3);
        if (add && t >= 0 && t < g.n) atomicAdd(&g.misc[t * 8 + (i & 7)], add);
    }
}

// ---- the candidate filter (ExtractVariantCandidates.py:347-393) over the tallies: one flag per position -----------------------
struct CandidateRule {
    double min_depth, min_af;
    int64_t ctg_start, ctg_end;      // 1-based inclusive; -1: no range
    const int64_t *bed_start, *bed_end;
    int64_t n_bed;                   // -1: no bed file; intervals sorted, merged, 0-based half-open
};

__global__ __launch_bounds__(256) void fe_candidate_flags_kernel(Region g, CandidateRule rule, uint8_t *flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= g.n) return;
    const ulonglong2 w01 = *(const ulonglong2 *)(g.pq + t * 4), w23 = *(const ulonglong2 *)(g.pq + t * 4 + 2);
    const uint4 hi4 = *(const uint4 *)(g.misc + t * 8 + 4);
    const uint32_t n[7] = {pq_field(w01.x, 2), pq_field(w01.y, 2), pq_field(w23.x, 2), pq_field(w23.y, 2), hi4.y, hi4.z, hi4.w};
    uint8_t keep = 0;
    do {
        if (!(n[0] | n[1] | n[2] | n[3] | n[4] | n[5] | n[6])) break;       // not a key of the reference's dict
        const int64_t p0 = g.lo + t;
        if (rule.ctg_start >= 0 && !(rule.ctg_start <= p0 + 1 && p0 + 1 <= rule.ctg_end)) break;
        if (rule.n_bed >= 0) {
            int64_t a = 0, b = rule.n_bed;                                  // first interval starting after p0
            while (a < b) { const int64_t mid = (a + b) >> 1; if (rule.bed_start[mid] <= p0) a = mid + 1; else b = mid; }
            if (a == 0 || !(p0 < rule.bed_end[a - 1])) break;
        }
        int64_t i = p0 - g.ref0;
        if (i < 0) i += g.ref_len;                                          // Python's negative index
        if (i < 0 || i >= g.ref_len) break;
        const uint8_t rb = BASES.evc[g.ref[i]];
        if (rb == 255) break;
        int64_t depth = 0;
        for (int k = 0; k < 7; ++k) depth += n[k];
        depth -= (int64_t)n[4] + n[5];
        if ((double)depth < rule.min_depth) break;
        int first = 0;                                                      // a stable descending sort keeps dict order among equals
        for (int k = 1; k < 7; ++k) if (n[k] > n[first]) first = k;
        int second = first == 0 ? 1 : 0;
        for (int k = 0; k < 7; ++k) if (k != first && n[k] > n[second]) second = k;
        const int64_t denom = depth > 0 ? depth : 1;
        keep = (first != rb || (double)n[second] / (double)denom >= rule.min_af) ? 1 : 0;
    } while (false);
    flags[t] = keep;
}

__global__ __launch_bounds__(256) void fe_given_flags_kernel(const int64_t *positions, int64_t n_positions, int64_t lo, int64_t n, uint8_t *flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_positions) return;
    const int64_t t = positions[i] - 1 - lo;
    if (t >= 0 && t < n) flags[t] = 1;
}

// ---- the block scan (device_scan.h): sums of 4096 items per workgroup, one workgroup over the block sums, then every workgroup writes ----
// Instantiated for flags -> exclusive prefix (uint32, n + 1 entries) and the list of flagged indices (candidates, kept windows, kept lines;
// line feeds of the text), and for 64-bit inclusive running sums (the candidate prefix; the second differences of pass 2, in place).
constexpr int SCAN_ITEMS = 16, SCAN_BLOCK = 256 * SCAN_ITEMS;

using clair_scan::SumScan;
using ScanU32 = SumScan<uint32_t, unsigned long long>;
using ScanU64 = SumScan<unsigned long long, unsigned long long>;
using ScanInt = SumScan<int, long long>;
using ScanFlags = clair_scan::FlagScan<false>;
using ScanNewlines = clair_scan::FlagScan<true>;

// what is written for item i, `before` the sum of the items before it.  Flags: the exclusive prefix (optional; entry n = the total) and the list of set indices
struct WriteCompact {
    static constexpr int PAST_END = 1;      // the thread that owns index n writes the total
    uint32_t *prefix;
    int64_t *list, list_base;
    __device__ inline uint32_t seed() const { return 0; }
    template <typename P> __device__ inline void write(const P &, int64_t i, int64_t n, uint32_t before, uint32_t item) const {
        if (prefix) prefix[i] = before;
        if (i < n && item) list[before] = list_base + i;
    }
};
// the inclusive running sum, seeded with 0 (fold == NULL), fold[0], or (second) lo fold[0] - fold[1]: see fe_windows_per_op_noleft_kernel
struct WriteRunning {
    static constexpr int PAST_END = 0;
    unsigned long long *out;
    const unsigned long long *fold;
    int second;
    int64_t lo;
    __device__ inline unsigned long long seed() const { return !fold ? 0 : second ? (unsigned long long)lo * fold[0] - fold[1] : fold[0]; }
    template <typename P> __device__ inline void write(const P &, int64_t i, int64_t, unsigned long long before, unsigned long long item) const { out[i] = before + item; }
};

// ---- pass 2: windows per read base (the tuple counts), inserted bases into their windows ---------------------------------------
struct Candidates {
    const int64_t *centre;       // 1-based, ascending
    const uint32_t *before;      // before[t] = candidates with centre - 1 - lo < t; n + 1 entries
    uint32_t *ins;               // [n_candidates][33][8]
    const unsigned long long *before_sum;   // before_sum[t] = before[0] + ... + before[t]: windows over a RUN of positions in four look-ups
    // --stop_consider_left_edge only (NULL otherwise): what reads that START inside a window added to the tables under it -- per
    // window and column 8 read-base rows, M per strand, D per strand -- and the tuples per window as range additions over the index
    uint32_t *late;              // [n_candidates][33][12]
    int *tuple_diff;             // [n_candidates + 1]  (per-base pass 2, CLAIR_AMD_FE_PASS2=base: range additions over the candidate index)
    // per-operation pass 2: the same totals as SECOND differences over the centre value u (index u - lo, n + 2 entries; 64-bit two's complement):
    // tuples(u) = sum over p <= u of (u - p + 1) d2[p]; what falls left of the tables goes into fold[0] = sum v, fold[1] = sum v p
    unsigned long long *d2, *fold;
};
constexpr int LATE_ROW = 12;

__device__ inline uint32_t before_at(const Region &g, const Candidates &c, int64_t t) {
    return c.before[t < 0 ? 0 : (t > g.n ? g.n : t)];
}

// generate_tensor :51-53: the k-th base (row: its base row + 4 on the reverse strand) of an insertion at rp into the windows i0 .. i1 - 1 that
// hold it: column min(idx + k, 32), channel 1
__device__ inline void scatter_inserted_base(const Candidates &c, uint32_t i0, uint32_t i1, int64_t rp, int64_t k, int row) {
    for (uint32_t i = i0; i < i1; ++i) {
        const int64_t col = rp - c.centre[i] + 17 + k;
        atomicAdd(&c.ins[((size_t)i * N_POS + (col < N_POS - 1 ? col : N_POS - 1)) * N_ROW + row], 1u);
    }
}

// nc tuples of `read` from every lane (whole waves only): one atomic per run of equal reads in the wave (64 consecutive bases or operations are
// nearly always one alignment's): 64 lanes adding to one address serialise at the memory side, which made this pass four times the first one
__device__ inline void add_read_tuples(const SlabView &s, uint32_t read, unsigned long long nc) {
    unsigned long long todo = __ballot(nc != 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t r = __shfl(read, leader, 64);
        const bool mine = nc != 0 && read == r;
        unsigned long long v = mine ? nc : 0;
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd((unsigned long long *)&s.tuples[r], v);
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(256) void fe_windows_per_base_kernel(Region g, SlabView s, Candidates c) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    uint32_t read = 0xffffffffu;
    uint64_t nc = 0;
    if (e < s.n_elem) {
        const Element el = element_of(s, e);
        if (el.r.flags & CLAIR_READ_PILE) {
            // centres whose window is open while this base is offered (CreateTensor.py:296-361)
            const bool left_edge = c.late == nullptr;
            const int so = (el.r.flags & CLAIR_READ_REVERSE) ? 4 : 0;
            int64_t a = -1, b = -2;
            if (el.code == CLAIR_OP_M) {
                a = el.rp > el.r.pos0 ? el.rp - 17 : el.r.pos0 - 16;
                b = el.rp + 17;
            } else if (el.rp > el.r.pos0) {
                a = el.rp - 17;
                b = el.rp + 16;
            }
            // without left-edge windows a read opens only the windows whose first column it walks: centres from POS + 17 on
            if (!left_edge && a < el.r.pos0 + 17) a = el.r.pos0 + 17;
            if (b >= a) {
                const uint32_t i0 = before_at(g, c, a - 1 - g.lo), i1 = before_at(g, c, b - g.lo);
                nc = i1 - i0;
                if (!left_edge && nc) { atomicAdd(&c.tuple_diff[i0], 1); atomicSub(&c.tuple_diff[i1], 1); }
            }
            read = el.read;
            if (!left_edge && el.rp - el.r.pos0 <= 31 && (el.code == CLAIR_OP_M || (el.code == CLAIR_OP_D && el.rp > el.r.pos0))) {
                // ... and what this base put into the tables belongs to none of the windows it starts inside: centres rp - 15 .. POS + 16
                const uint8_t row = el.code == CLAIR_OP_M && el.qp < el.r.seq_len ? BASES.pile[s.seq[el.r.seq0 + el.qp]] : (uint8_t)255;
                if (el.code == CLAIR_OP_D || row != 255) {
                    const uint32_t j0 = before_at(g, c, el.rp - 15 - 1 - g.lo), j1 = before_at(g, c, el.r.pos0 + 16 - g.lo);
                    for (uint32_t j = j0; j < j1; ++j) {
                        uint32_t *cell = c.late + ((size_t)j * N_POS + (el.rp - c.centre[j] + 17)) * LATE_ROW;
                        if (el.code == CLAIR_OP_M) { atomicAdd(cell + row + so, 1u); atomicAdd(cell + 8 + (so >> 2), 1u); }
                        else atomicAdd(cell + 10 + (so >> 2), 1u);
                    }
                }
            }
            if (el.code == CLAIR_OP_I && el.rp > el.r.pos0 && el.qp < el.r.seq_len) {
                const uint8_t row = BASES.pile[s.seq[el.r.seq0 + el.qp]];
                if (row != 255) {
                    int64_t first = el.rp - 15;
                    if (!left_edge && first < el.r.pos0 + 17) first = el.r.pos0 + 17;
                    scatter_inserted_base(c, before_at(g, c, first - 1 - g.lo), before_at(g, c, el.rp + 16 - g.lo), el.rp, (int64_t)el.k, row + so);
                }
            }
        }
    }
    add_read_tuples(s, read, nc);
}

// ---- pass 2 with left-edge windows, per OPERATION: the windows open over a run of positions is a difference of sums of the prefix ----
// F(x) = candidates with centre <= x (the prefix, clamped to the span); G(x) = F(lo) + ... + F(x).  A base at rp lies in F(rp + 17) -
// F(rp - 18) open windows (rp + 16 for a deleted or inserted base), so an operation over rp = A..B lies in
// [G(B + 17) - G(A + 16)] - [G(B - 18) - G(A - 19)]: no walk over its bases.  Only a read's very first matched base differs (its
// windows start one centre later, CreateTensor.py:296-305), and the inserted bases still go to their windows one by one.
__device__ inline unsigned long long prefix_sum_at(const Region &g, const Candidates &c, int64_t x) {
    const int64_t i = x - g.lo;
    if (i < 0) return 0;
    if (i <= g.n) return c.before_sum[i];
    return c.before_sum[g.n] + (unsigned long long)(i - g.n) * c.before[g.n];
}

__global__ __launch_bounds__(256) void fe_windows_per_op_kernel(Region g, SlabView s, Candidates c) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    uint32_t read = 0xffffffffu;
    unsigned long long nc = 0;
    if (j < s.n_ops) {
        const clair_op_t op = s.ops[j];
        const clair_read_t r = s.reads[op.read];
        if (r.flags & CLAIR_READ_PILE) {
            read = op.read;
            const uint32_t code = op.code_len & 3u;
            const int64_t len = op.code_len >> 2, pos0 = r.pos0;
            int64_t a = pos0 + op.ref_off, b = a + len - 1;          // first and last reference position of the run (I: both the same)
            if (code == CLAIR_OP_M) {
                if (a == pos0) {                                       // the read's first base: windows of centres POS - 16 .. POS + 17
                    nc += before_at(g, c, pos0 + 17 - g.lo) - before_at(g, c, pos0 - 17 - g.lo);
                    ++a;
                }
                if (b >= a) nc += (prefix_sum_at(g, c, b + 17) - prefix_sum_at(g, c, a + 16)) - (prefix_sum_at(g, c, b - 18) - prefix_sum_at(g, c, a - 19));
            } else if (code == CLAIR_OP_D) {
                if (a == pos0) ++a;                                    // offered before any window is open
                if (b >= a) nc += (prefix_sum_at(g, c, b + 16) - prefix_sum_at(g, c, a + 15)) - (prefix_sum_at(g, c, b - 18) - prefix_sum_at(g, c, a - 19));
            } else if (a > pos0) {
                nc += (unsigned long long)len * (before_at(g, c, a + 16 - g.lo) - before_at(g, c, a - 18 - g.lo));
                const int so = (r.flags & CLAIR_READ_REVERSE) ? 4 : 0;
                const uint32_t i0 = before_at(g, c, a - 15 - 1 - g.lo), i1 = before_at(g, c, a + 16 - g.lo);
                for (int64_t k = 0; k < len && i1 > i0; ++k) {
                    if (op.q_off + k >= r.seq_len) break;
                    const uint8_t row = BASES.pile[s.seq[r.seq0 + op.q_off + k]];
                    if (row != 255) scatter_inserted_base(c, i0, i1, a, k, row + so);
                }
            }
        }
    }
    add_read_tuples(s, read, nc);
}

// ---- pass 2 WITHOUT left-edge windows, per operation (round 4; per base: fe_windows_per_base_kernel above, kept as the checker) ----
// A base at rp of an alignment that starts at POS lies in the windows of centres u in [max(rp - 17, POS + 17), rp + 17] (rp + 16 for a deleted
// or inserted base): the lower clamp is "a read opens only the windows whose first column it walks".  Per operation over rp = A..B:
//   * the alignment's tuple count is again a difference of running sums of the candidate prefix, the clamped part (rp < POS + 34) a
//     multiple of one prefix value;
//   * the tuples PER WINDOW are a trapezoid over u (a ramp of min(length, window width) centres up, a plateau, the same ramp down), cut off
//     below POS + 17: six second-difference entries over the centre VALUE instead of two range additions per base over the candidate index;
//     two running sums over the positions and a gather at the centres give the totals (the block scan with WriteRunning, fe_window_totals_at_kernel).
__device__ inline void d2_add(const Region &g, const Candidates &c, int64_t u, long long v) {
    const int64_t i = u - g.lo;
    if (i < 0) { atomicAdd(&c.fold[0], (unsigned long long)v); atomicAdd(&c.fold[1], (unsigned long long)(v * u)); }
    else if (i <= g.n + 1) atomicAdd(&c.d2[i], (unsigned long long)v);
}
// tuples a run of bases rp = A..B adds to the window of centre u, for u >= c0: #{rp: rp - 17 <= u <= rp + reach}
__device__ inline void d2_add_run(const Region &g, const Candidates &c, int64_t A, int64_t B, int reach, int64_t c0) {
    if (B < A || B + reach < c0) return;
    const int64_t L = B - A + 1, W = 17 + reach + 1, m = L < W ? L : W;
    int64_t from = INT64_MIN / 4;
    if (A - 17 < c0) {            // the window of c0 and its right neighbours only: a step up to T(c0), then the rest of the shape
        const int64_t hi = B < c0 + 17 ? B : c0 + 17, lo = A > c0 - reach ? A : c0 - reach;
        const long long t0 = hi >= lo ? hi - lo + 1 : 0;
        if (t0) { d2_add(g, c, c0, t0); d2_add(g, c, c0 + 1, -t0); }
        from = c0 + 1;
    }
    const int64_t u0 = A - 17 > from ? A - 17 : from, u1 = A - 17 + m - 1;            // first differences +1
    if (u0 <= u1) { d2_add(g, c, u0, 1); d2_add(g, c, u1 + 1, -1); }
    const int64_t w0 = B + reach + 2 - m > from ? B + reach + 2 - m : from, w1 = B + reach + 1;   // first differences -1
    if (w0 <= w1) { d2_add(g, c, w0, -1); d2_add(g, c, w1 + 1, 1); }
}

__global__ __launch_bounds__(256) void fe_windows_per_op_noleft_kernel(Region g, SlabView s, Candidates c) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    uint32_t read = 0xffffffffu;
    unsigned long long nc = 0;
    if (j < s.n_ops) {
        const clair_op_t op = s.ops[j];
        const clair_read_t r = s.reads[op.read];
        if (r.flags & CLAIR_READ_PILE) {
            read = op.read;
            const uint32_t code = op.code_len & 3u;
            const int64_t len = op.code_len >> 2, pos0 = r.pos0, c0 = pos0 + 17;
            int64_t a = pos0 + op.ref_off, b = a + len - 1;          // first and last reference position of the run (I: both the same)
            auto below = [&](int64_t A, int64_t B) -> unsigned long long {      // sum over rp = A..B of the prefix at max(rp - 18, POS + 16)
                unsigned long long v = 0;
                const int64_t r1 = B < pos0 + 33 ? B : pos0 + 33;
                if (r1 >= A) v += (unsigned long long)(r1 - A + 1) * before_at(g, c, pos0 + 16 - g.lo);
                const int64_t a2 = A > pos0 + 34 ? A : pos0 + 34;
                if (B >= a2) v += prefix_sum_at(g, c, B - 18) - prefix_sum_at(g, c, a2 - 19);
                return v;
            };
            if (code == CLAIR_OP_M) {
                nc += (prefix_sum_at(g, c, b + 17) - prefix_sum_at(g, c, a + 16)) - below(a, b);
                d2_add_run(g, c, a, b, 17, c0);
            } else if (code == CLAIR_OP_D) {
                if (a == pos0) ++a;                                    // offered before any window is open
                if (b >= a) {
                    nc += (prefix_sum_at(g, c, b + 16) - prefix_sum_at(g, c, a + 15)) - below(a, b);
                    d2_add_run(g, c, a, b, 16, c0);
                }
            } else if (a > pos0) {
                const int64_t lo_u = a - 17 > c0 ? a - 17 : c0;
                if (lo_u <= a + 16) {
                    nc += (unsigned long long)len * (before_at(g, c, a + 16 - g.lo) - before_at(g, c, lo_u - 1 - g.lo));
                    d2_add(g, c, lo_u, len); d2_add(g, c, lo_u + 1, -len);
                    d2_add(g, c, a + 17, -len); d2_add(g, c, a + 18, len);
                }
                const int so = (r.flags & CLAIR_READ_REVERSE) ? 4 : 0;
                const int64_t first = a - 15 > c0 ? a - 15 : c0;
                const uint32_t i0 = before_at(g, c, first - 1 - g.lo), i1 = before_at(g, c, a + 16 - g.lo);
                for (int64_t k = 0; k < len && i1 > i0; ++k) {
                    if (op.q_off + k >= r.seq_len) break;
                    const uint8_t row = BASES.pile[s.seq[r.seq0 + op.q_off + k]];
                    if (row != 255) scatter_inserted_base(c, i0, i1, a, k, row + so);
                }
            }
        }
    }
    add_read_tuples(s, read, nc);
}

// what the first 32 walked positions of an alignment put into the tables belongs to none of the windows it starts inside (centres rp - 15 ..
// POS + 16): collected per window and column, the assembly takes it out again.  One thread per alignment: at most 32 positions of it.
__global__ __launch_bounds__(256) void fe_late_starters_kernel(Region g, SlabView s, Candidates c, uint32_t n_reads) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_reads) return;
    const clair_read_t r = s.reads[i];
    if (!(r.flags & CLAIR_READ_PILE)) return;
    const int so = (r.flags & CLAIR_READ_REVERSE) ? 4 : 0;
    const uint32_t j1 = before_at(g, c, r.pos0 + 16 - g.lo);
    for (uint32_t o = 0; o < r.n_ops; ++o) {
        const clair_op_t op = s.ops[r.op0 + o];
        if (op.ref_off > 31) break;
        const uint32_t code = op.code_len & 3u;
        if (code == CLAIR_OP_I) continue;
        const int64_t len = op.code_len >> 2;
        for (int64_t k = 0; k < len && op.ref_off + k <= 31; ++k) {
            const int64_t rp = r.pos0 + op.ref_off + k;
            if (code == CLAIR_OP_D && rp <= r.pos0) continue;
            uint8_t row = 255;
            if (code == CLAIR_OP_M) {
                const uint32_t qp = op.q_off + (uint32_t)k;
                if (qp < r.seq_len) row = BASES.pile[s.seq[r.seq0 + qp]];
                if (row == 255) continue;
            }
            for (uint32_t j = before_at(g, c, rp - 15 - 1 - g.lo); j < j1; ++j) {
                uint32_t *cell = c.late + ((size_t)j * N_POS + (rp - c.centre[j] + 17)) * LATE_ROW;
                if (code == CLAIR_OP_M) { atomicAdd(cell + row + so, 1u); atomicAdd(cell + 8 + (so >> 2), 1u); }
                else atomicAdd(cell + 10 + (so >> 2), 1u);
            }
        }
    }
}

// the tuples per window from the second differences: two running sums in place (WriteRunning: d2 -> first differences, seeded with fold[0] ->
// tuples per centre value, seeded with the tuples of u = lo - 1: lo fold[0] - fold[1]; two's complement throughout: signed sums come out
// right modulo 2^64), then a gather at the centres
__global__ __launch_bounds__(256) void fe_window_totals_at_kernel(const unsigned long long *tuples_at, const int64_t *centre, int64_t n_candidates, int64_t lo, int64_t n,
                                                                  uint64_t *window_tuples) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_candidates) return;
    const int64_t at = centre[i] - lo;
    window_tuples[i] = at >= 0 && at <= n + 1 ? tuples_at[at] : 0;
}

// ---- per candidate: was its window ever opened, how many tuples did it hold, does it survive -----------------------------------
struct WindowRule {
    int min_coverage;
    int drop_non_iupac_centre;   // clair/utils.py:90-91
    const uint32_t *late;        // --stop_consider_left_edge: see Candidates; window_tuples then comes in filled (fe_window_totals_at_kernel, or the running sum of tuple_diff)
};

__global__ __launch_bounds__(256) void fe_window_flags_kernel(Region g, const int64_t *centre, int64_t n_candidates, WindowRule rule,
                                                              uint8_t *keep, uint64_t *window_tuples) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_candidates) return;
    const int64_t c = centre[i];
    uint64_t walked = 0, tuples = 0;
    uint32_t depth_centre = 0;
    for (int64_t rp = c - 17; rp <= c + 17; ++rp) {
        const int64_t t = rp - g.lo;
        if (t < 0 || t >= g.n) continue;
        const ulonglong2 w01 = *(const ulonglong2 *)(g.pq + t * 4), w23 = *(const ulonglong2 *)(g.pq + t * 4 + 2);
        const uint4 a = *(const uint4 *)(g.misc + t * 8);
        const uint32_t start_m = g.misc[t * 8 + 4];
        uint64_t m = 0;
        for (int field = 0; field < 2; ++field) m += (uint64_t)pq_field(w01.x, field) + pq_field(w01.y, field) + pq_field(w23.x, field) + pq_field(w23.y, field);
        const uint64_t d = (uint64_t)a.x + a.y;
        if (rule.late ? rp == c - 17 : rp <= c + 16) walked += m + d + a.z;   // M or D (incl. a read's first D) opens the window
        tuples += m;
        if (rp == c + 17) tuples -= start_m;                        // a read that STARTS there never opened this window
        if (rp >= c - 16) tuples += d + a.w;
        if (rp == c - 1) depth_centre = (uint32_t)m;
    }
    const bool opened = walked > 0;
    if (rule.late) {
        const uint32_t *cell = rule.late + ((size_t)i * N_POS + 16) * LATE_ROW;
        depth_centre -= cell[8] + cell[9];
        tuples = window_tuples[i];
    }
    const int64_t nrp = c - g.ref0;
    bool ok = opened && nrp - 17 >= 0 && (int64_t)depth_centre >= (int64_t)rule.min_coverage;
    if (ok && rule.drop_non_iupac_centre) {
        const int64_t at = nrp - 17 + 16;                           // refseq[16] of the slice [nrp-17, nrp+16) clamped to the sequence
        ok = at < g.ref_len && BASES.pile[g.ref[at]] != 255;
    }
    keep[i] = ok ? 1 : 0;
    window_tuples[i] = opened ? tuples : 0;
}

// ---- assembly: 264 (position, row) quads per kept window ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fe_assemble_kernel(Region g, const int64_t *centre, const int64_t *kept, int64_t n_kept, const uint32_t *ins,
                                                          const uint32_t *late, short4 *counts, int64_t *out_centre, uint8_t *out_refseq) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t o = id / N_QUAD;
    if (o >= n_kept) return;
    const int quad = (int)(id - o * N_QUAD), idx = quad >> 3, row = quad & 7, so = row >> 2, b = row & 3;
    const int64_t ci = kept[o], c = centre[ci];
    const int64_t rp = c - 17 + idx, t = rp - g.lo;
    uint32_t qv = 0, mw = 0, dw = 0;
    if (t >= 0 && t < g.n) {
        const ulonglong2 w01 = *(const ulonglong2 *)(g.pq + t * 4), w23 = *(const ulonglong2 *)(g.pq + t * 4 + 2);
        const unsigned long long w[4] = {w01.x, w01.y, w23.x, w23.y};
        qv = pq_field(w[b], so);
        mw = pq_field(w[0], so) + pq_field(w[1], so) + pq_field(w[2], so) + pq_field(w[3], so);
        dw = g.misc[t * 8 + so];
    }
    if (late) {
        const uint32_t *cell = late + ((size_t)ci * N_POS + idx) * LATE_ROW;
        qv -= cell[row];
        mw -= cell[8 + so];
        dw -= cell[10 + so];
    }
    const bool is_ref = ref_row(g, rp) == b;
    const uint32_t ch0 = is_ref ? mw : 0, ch1 = qv + ins[((size_t)ci * N_POS + idx) * N_ROW + row];
    const uint32_t ch2 = is_ref ? mw + (idx >= 1 ? dw : 0) : 0, ch3 = qv;
    if ((ch0 | ch1 | ch2 | ch3) > 32767u) flag(g, CLAIR_FE_OVERFLOW);
    counts[id] = make_short4((short)ch0, (short)ch1, (short)ch2, (short)ch3);
    if (quad == 0) out_centre[o] = c;
    if (quad < 34) {                                                 // reference_sequence[nrp-17 : nrp+16], NUL-padded to 34
        const int64_t nrp = c - g.ref0, at = nrp - 17 + quad;
        out_refseq[o * 34 + quad] = (quad < 33 && at >= 0 && at < g.ref_len) ? g.ref[at] : (uint8_t)0;
    }
}

// ---- `samtools view` text parsed on the device: the line handling of clair_host_sampack_* (hostsrc/host_sampack.cpp), one thread per line ---
// What the host packer does per line -- split on whitespace, FLAG / RNAME / POS / MAPQ / CIGAR / SEQ, the two stages' filters, the CIGAR
// reduced to M / I / D operations -- on the text where the copy from the pipe left it; the host only moves bytes.  Of the text only the
// SEQ columns of the kept alignments stay resident (fe_text_seq_kernel packs them, 4-byte aligned per alignment, into the slab's `seq`):
// QNAME, QUAL and the tags are more than half of a line, and a region's text is what fills the HBM first (64 B per position of tables
// against ~75 B of text per position at 30x).  The per-read state the scripts carry from line
// to line (--dcov, sortedness) is recovered from the sorted start positions (a read's rank among the pileup reads of its start
// position is its index minus the lower bound of that position) and carried from chunk to chunk by the host.
struct TextOptions {
    const uint8_t *ctg;
    int ctg_len;
    int dcov, evc_min_mq, pile_min_mq;
    int64_t pile_start, pile_end;        // 1-based inclusive, -1 -1: none
    int lookup;                          // clair_frontend_bam_lookup: keep and mark what the indel look-up counts (BAM records only)
};

struct TextLine {                        // what pass A learns about a line
    int64_t pos0;
    uint32_t cigar_off, cigar_len, seq_off, seq_len;
    uint32_t n_ops, n_elem;
    uint32_t flags;                      // CLAIR_READ_REVERSE | CLAIR_READ_EVC | TL_CANDIDATE | TL_ZERO_INDEL | TL_LONG_SPAN | TL_LEAD_INDEL
    uint32_t pad_mask;                   // TL_LOOKUP: clair_read_t.reserved (clair_reads.h)
};
// TL_LEAD_INDEL: an I / D while the reference cursor is still at POS.  The last three are set for BAM records only -- TL_BAM_NOSEQ: SEQ '*' (l_seq 0): the
// slab holds the one byte '*' the text path stores; TL_LOOKUP: becomes CLAIR_READ_LOOKUP, counted by the indel look-up and kept whatever the stages think
// of it; TL_OFFSETS: the part of TL_LONG_SPAN that is about 32-bit offsets, an anomaly for every kept alignment (the rest only where a stage walks it)
enum { TL_CANDIDATE = 16, TL_ZERO_INDEL = 32, TL_LONG_SPAN = 64, TL_LEAD_INDEL = 128, TL_BAM_NOSEQ = 256, TL_LOOKUP = 512, TL_OFFSETS = 1024 };

struct TextState {                       // carried from chunk to chunk (host copy in clair_frontend)
    int64_t prev_pos, depth_cap;         // CreateTensor.py:249-250, 277-287
    int64_t last_pos, have_last;         // sortedness of the kept alignments
    int64_t evc_last_pos, have_evc_last; // POS of the last alignment the candidate search accepted (CLAIR_FE_LEAD_INDEL)
    int64_t lines, evc_reads, pile_reads;
    uint32_t anomalies, malformed;       // malformed: 1 + index of the first line the host packer would reject
};

__device__ inline bool text_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }

// end of the token that starts at q: 16 bytes at a time while none of them is below 0x21 (every white-space character is; SEQ and QUAL
// bytes are not), byte by byte from the first word that holds one
__device__ inline int64_t token_end(const uint8_t *t, int64_t q, int64_t end) {
    while (q < end && (q & 15)) { if (text_space(t[q])) return q; ++q; }
    while (q + 16 <= end) {
        const uint4 w = *(const uint4 *)(t + q);
        const uint32_t low = ((w.x - 0x21212121u) & ~w.x) | ((w.y - 0x21212121u) & ~w.y) | ((w.z - 0x21212121u) & ~w.z) | ((w.w - 0x21212121u) & ~w.w);
        if (low & 0x80808080u) break;
        q += 16;
    }
    while (q < end && !text_space(t[q])) ++q;
    return q;
}

// one CIGAR operation of `adv` bases, `ch` its letter: the rules of the walk shared by the text and the binary CIGAR; EMIT writes the kept operations
struct CigarWalk {
    int64_t rp = 0, qp = 0, soft = 0, total = 0, rlen = 0;
    uint32_t n_ops = 0;
    uint64_t elems = 0;
    bool zero = false, lead = false;
    uint32_t pad_mask = 0;               // I / D operations behind something the slab does not hold that is no M (clair_reads.h: CLAIR_READ_LOOKUP)
    bool prev_pad = false, after_n = false;   // after_n: this walk does not advance over an N, so what follows one is not where the slab says

    template <bool EMIT>
    __device__ inline void op(int64_t adv, uint8_t ch, uint32_t read, clair_op_t *ops, uint32_t *op_elem, uint32_t elem0) {
        int code = -1;
        switch (ch) {
        case 'S': soft += adv; qp += adv; break;
        case 'M': case '=': case 'X': code = CLAIR_OP_M; break;
        case 'I': code = CLAIR_OP_I; break;
        case 'D': code = CLAIR_OP_D; break;
        case 'N': rlen += adv; after_n = after_n || adv > 0; break;
        default: break;
        }
        if (code >= 0) {
            if (adv > 0) {
                const int64_t len = adv > 0x3fffffff ? 0x3fffffff : adv;
                if (EMIT) {
                    ops[n_ops] = clair_op_t{read, (uint32_t)len << 2 | (uint32_t)code, (int32_t)rp, (uint32_t)qp};
                    op_elem[n_ops] = elem0 + (uint32_t)elems;
                }
                if (code != CLAIR_OP_M && (prev_pad || after_n)) pad_mask |= 1u << (n_ops < 31 ? n_ops : 31);
                ++n_ops;
                elems += (uint64_t)len;
                if (code != CLAIR_OP_M && rp == 0) lead = true;       // tallied at POS - 1 by the candidate search (EVC :326-336)
            } else if (code != CLAIR_OP_M) {
                zero = true;
            }
            if (code != CLAIR_OP_I) { rp += adv; rlen += adv; }
            if (code != CLAIR_OP_D) qp += adv;
        }
        total += adv;
        prev_pad = adv == 0 || !(ch == 'M' || ch == '=' || ch == 'X' || ch == 'I' || ch == 'D' || ch == 'N' || ch == 'S');
    }
};

// walks a CIGAR; EMIT writes the kept operations
template <bool EMIT>
__device__ inline CigarWalk walk_cigar(const uint8_t *cg, uint32_t cl, uint32_t read, clair_op_t *ops, uint32_t *op_elem, uint32_t elem0) {
    int64_t adv = 0;
    CigarWalk w;
    for (uint32_t i = 0; i < cl; ++i) {
        const uint8_t ch = cg[i];
        if (ch >= '0' && ch <= '9') { adv = adv * 10 + (ch - '0'); if (adv > ((int64_t)1 << 40)) adv = (int64_t)1 << 40; continue; }
        w.op<EMIT>(adv, ch, read, ops, op_elem, elem0);
        adv = 0;
    }
    return w;
}

__device__ inline bool text_int(const uint8_t *s, uint32_t len, int64_t *out) {     // [+-]digits, at most 18 of them (host_sampack.cpp)
    uint32_t i = 0;
    bool neg = false;
    if (i < len && (s[i] == '-' || s[i] == '+')) { neg = s[i] == '-'; ++i; }
    if (i == len || len - i > 18) return false;
    int64_t x = 0;
    for (; i < len; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        x = x * 10 + (s[i] - '0');
    }
    *out = neg ? -x : x;
    return true;
}

__global__ __launch_bounds__(256) void fe_text_lines_kernel(const uint8_t *text, const int64_t *newline, int64_t n_lines, TextOptions opt, TextLine *lines,
                                                            uint8_t *is_candidate, TextState *state) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_lines) return;
    TextLine out{};
    is_candidate[k] = 0;
    const int64_t begin = k == 0 ? 0 : newline[k - 1] + 1, end = newline[k];
    uint32_t col[10], len[10];
    int n = 0;
    int64_t p = begin;
    while (p < end && n < 10) {
        while (p < end && text_space(text[p])) ++p;
        if (p >= end) break;
        const int64_t q = token_end(text, p, end);
        col[n] = (uint32_t)p;
        len[n] = (uint32_t)(q - p);
        ++n;
        p = q;
    }
    bool bad = n == 0;
    if (!bad && text[col[0]] == '@') { lines[k] = out; return; }            // header line
    bad = bad || n < 10;
    int64_t flag = 0, pos1 = 0, mq = 0;
    bad = bad || !text_int(text + col[1], len[1], &flag) || !text_int(text + col[3], len[3], &pos1) || !text_int(text + col[4], len[4], &mq);
    if (bad) {                                                                // the host packer names the line and the column
        atomicMin(&state->malformed, (uint32_t)(k + 1));
        lines[k] = out;
        return;
    }
    bool same_ctg = (int)len[2] == opt.ctg_len;
    for (int i = 0; same_ctg && i < opt.ctg_len; ++i) same_ctg = text[col[2] + i] == opt.ctg[i];
    const CigarWalk w = walk_cigar<false>(text + col[5], len[5], 0, nullptr, nullptr, 0);
    const bool evc_ok = same_ctg && mq >= opt.evc_min_mq && !(len[5] == 1 && text[col[5]] == '*') && !(1.0 - (double)w.soft / (double)(w.total + 1) < 0.55);
    bool in_region = true;
    if (opt.pile_start >= 0 && opt.pile_end >= 0) {
        const int64_t end1 = pos1 + (w.rlen > 0 ? w.rlen : 1) - 1;            // bam_endpos
        in_region = same_ctg && pos1 <= opt.pile_end && end1 >= opt.pile_start;
    }
    const bool candidate = in_region && mq >= opt.pile_min_mq;
    out.pos0 = pos1 - 1;
    out.cigar_off = col[5]; out.cigar_len = len[5];
    out.seq_off = col[9]; out.seq_len = len[9];
    out.n_ops = w.n_ops;
    out.n_elem = w.elems > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)w.elems;
    out.flags = ((flag & 16) ? CLAIR_READ_REVERSE : 0) | (evc_ok ? CLAIR_READ_EVC : 0) | (candidate ? TL_CANDIDATE : 0) | (w.zero ? TL_ZERO_INDEL : 0)
                | (w.lead ? TL_LEAD_INDEL : 0)
                | ((w.rp > (int64_t)len[9] + 100000 - 64 || w.rp > 0x7fffff00 || w.qp > 0x7fffff00) ? TL_LONG_SPAN : 0);
    lines[k] = out;
    is_candidate[k] = candidate ? 1 : 0;
}

// --dcov: the rank of a pileup read among those of its start position = its index among the candidates minus the lower bound of its
// position (start positions ascend; where they do not, CLAIR_FE_UNSORTED sends the run to the host anyway)
__global__ __launch_bounds__(256) void fe_text_dcov_kernel(TextLine *lines, const int64_t *cand, int64_t n_cand, int dcov, TextState carry) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_cand) return;
    TextLine &ln = lines[cand[j]];
    const int64_t pos = ln.pos0;
    int64_t a = 0, b = j;                                                     // first candidate with this start position
    while (a < b) { const int64_t mid = (a + b) >> 1; if (lines[cand[mid]].pos0 < pos) a = mid + 1; else b = mid; }
    int64_t depth_cap = j - a;
    if (a == 0 && pos == carry.prev_pos) depth_cap += carry.depth_cap + 1;   // the run began in an earlier chunk (or is the scripts' initial previous_position = 0)
    uint32_t fl = ln.flags;
    if (depth_cap < dcov) fl |= CLAIR_READ_PILE | (depth_cap == 0 ? CLAIR_READ_FLUSH : 0);
    ln.flags = fl;
}

__global__ __launch_bounds__(256) void fe_text_keep_kernel(const TextLine *lines, int64_t n_lines, uint8_t *keep) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_lines) return;
    keep[k] = (lines[k].flags & (CLAIR_READ_EVC | CLAIR_READ_PILE | TL_LOOKUP)) ? 1 : 0;
}

// one workgroup: exclusive sums of the kept lines' operation and element counts, sortedness, counters, the state for the next chunk
__global__ __launch_bounds__(256) void fe_text_offsets_kernel(const TextLine *lines, int64_t n_lines, const int64_t *kept, int64_t n_kept, const int64_t *cand, int64_t n_cand,
                                                              uint32_t *op0, uint32_t *elem0, uint32_t *seq0, uint64_t *totals, TextState carry, TextState *state) {
    __shared__ uint64_t s_ops, s_elems;
    __shared__ uint32_t s_anom, s_reach;
    __shared__ unsigned long long s_evc, s_pile;
    __shared__ unsigned long long s_last_evc;                                 // 1 + index (among the kept lines) of the last one the candidate search accepts
    if (threadIdx.x == 0) { s_ops = 0; s_elems = 0; s_anom = 0; s_reach = 0; s_evc = 0; s_pile = 0; s_last_evc = 0; }
    __syncthreads();
    uint64_t carry_ops = 0, carry_elems = 0, carry_seq = 0;
    uint32_t anom = 0, reach = 0;                 // reach: the longest alignment in elements (no reference span is longer)
    unsigned long long evc = 0, pile = 0;
    for (int64_t at = 0; at < n_kept; at += 256) {
        const int64_t i = at + threadIdx.x;
        uint32_t a = 0, b = 0, c = 0;
        if (i < n_kept) {
            const TextLine ln = lines[kept[i]];
            a = ln.n_ops;
            b = ln.n_elem;
            c = (ln.seq_len + 3u) & ~3u;          // the alignment's bases in the packed buffer: a whole number of dwords
            reach = max(reach, b);
            const int64_t before = i > 0 ? lines[kept[i - 1]].pos0 : (carry.have_last ? carry.last_pos : ln.pos0);
            if (ln.pos0 < before) anom |= CLAIR_FE_UNSORTED;
            if ((ln.flags & TL_ZERO_INDEL) && (ln.flags & CLAIR_READ_EVC)) anom |= CLAIR_FE_ZERO_INDEL;
            if (((ln.flags & TL_LONG_SPAN) && (ln.flags & (CLAIR_READ_EVC | CLAIR_READ_PILE))) || (ln.flags & TL_OFFSETS)) anom |= CLAIR_FE_LONG_SPAN;
            if (ln.flags & CLAIR_READ_EVC) {
                atomicMax(&s_last_evc, (unsigned long long)(i + 1));
                if (ln.flags & TL_LEAD_INDEL) {                                // rare: look back over the run of equal start positions for an accepted alignment
                    bool earlier = false;
                    int64_t j = i - 1;
                    for (; j >= 0; --j) {
                        const TextLine &b4 = lines[kept[j]];
                        if (b4.pos0 != ln.pos0) break;
                        if (b4.flags & CLAIR_READ_EVC) { earlier = true; break; }
                    }
                    if (!earlier && j < 0 && carry.have_evc_last && carry.evc_last_pos == ln.pos0) earlier = true;   // the run began in an earlier chunk
                    if (earlier) anom |= CLAIR_FE_LEAD_INDEL;
                }
            }
            evc += (ln.flags & CLAIR_READ_EVC) ? 1 : 0;
            pile += (ln.flags & CLAIR_READ_PILE) ? 1 : 0;
        }
        uint32_t ta, tb, tc;
        using Sum = SumScan<uint32_t, uint32_t>;
        const uint32_t ea = clair_scan::block_exclusive<Sum>(a, &ta);
        const uint32_t eb = clair_scan::block_exclusive<Sum>(b, &tb);
        const uint32_t ec = clair_scan::block_exclusive<Sum>(c, &tc);
        if (i < n_kept) { op0[i] = (uint32_t)(carry_ops + ea); elem0[i] = (uint32_t)(carry_elems + eb); seq0[i] = (uint32_t)(carry_seq + ec); }
        carry_ops += ta;
        carry_elems += tb;
        carry_seq += tc;
    }
    atomicOr(&s_anom, anom);
    atomicMax(&s_reach, reach);
    atomicAdd(&s_evc, evc);
    atomicAdd(&s_pile, pile);
    __syncthreads();
    if (threadIdx.x == 0) {
        totals[0] = carry_ops;
        totals[1] = carry_elems;
        totals[2] = s_reach;
        totals[3] = n_kept ? (uint64_t)lines[kept[0]].pos0 : 0;       // where the slab begins (the kept lines are sorted, or CLAIR_FE_UNSORTED is raised)
        totals[4] = carry_seq;                                        // bytes of the packed bases
        TextState st = carry;
        st.anomalies = carry.anomalies | s_anom;
        st.malformed = state->malformed;
        st.lines = carry.lines + n_lines;
        st.evc_reads = carry.evc_reads + (int64_t)s_evc;
        st.pile_reads = carry.pile_reads + (int64_t)s_pile;
        if (n_kept) { st.last_pos = lines[kept[n_kept - 1]].pos0; st.have_last = 1; }
        if (s_last_evc) { st.evc_last_pos = lines[kept[s_last_evc - 1]].pos0; st.have_evc_last = 1; }
        if (n_cand) {                                                         // previous_position / depthCap after the last pileup candidate
            const int64_t pos = lines[cand[n_cand - 1]].pos0;
            int64_t a = 0, b = n_cand - 1;
            while (a < b) { const int64_t mid = (a + b) >> 1; if (lines[cand[mid]].pos0 < pos) a = mid + 1; else b = mid; }
            int64_t depth_cap = n_cand - 1 - a;
            if (a == 0 && pos == carry.prev_pos) depth_cap += carry.depth_cap + 1;
            st.prev_pos = pos;
            st.depth_cap = depth_cap;
        }
        *state = st;
    }
}

// The SEQ column of every kept line into the slab's packed buffer: a wave per alignment, a dword per lane and step.  The source starts at any
// byte of the text: two aligned dwords and v_alignbyte give the four bytes from there (the text buffer is allocated 16 bytes longer than the text).
__global__ __launch_bounds__(256) void fe_text_seq_kernel(const uint8_t *text, const TextLine *lines, const int64_t *kept, int64_t n_kept, const uint32_t *seq0, uint8_t *seq) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_kept) return;
    const int lane = threadIdx.x & 63;
    const TextLine ln = lines[kept[i]];
    const uint32_t n_dw = (ln.seq_len + 3u) >> 2;
    const uint32_t *src = (const uint32_t *)(text + (ln.seq_off & ~3u));
    const uint32_t shift = ln.seq_off & 3u;
    uint32_t *dst = (uint32_t *)(seq + seq0[i]);
    for (uint32_t k = (uint32_t)lane; k < n_dw; k += 64) {
        const uint32_t lo = src[k], hi = src[k + 1];
        dst[k] = __builtin_amdgcn_alignbyte(hi, lo, shift);
    }
}

// ---- BAM records decoded on the device (clair_frontend_bam_options / _add_bam): the binary twin of the text path above ------------------
// The host inflates BGZF and walks the records' block_size fields (hostsrc/host_bam.cpp); the chunk comes here as it was inflated, with the
// start of every record.  fe_bam_records_kernel decodes a record into the TextLine the text path fills for the line `samtools view` would
// print for it, and applies the view's own filter first (-F 2316, the contig, the region, and `-s` where clair_frontend_bam_subsample asked
// for it: subsample_core.h); the records the view drops are compacted out
// before anything counts lines, so that --dcov, the kept lines, the counters and the slab are the text path's kernels on the same lines.
// Records start at any byte: fields are read as two aligned dwords and v_alignbyte (the buffer is allocated 16 bytes longer).
struct BamOptions {
    int tid;
    int64_t region_lo, region_hi;        // 1-based inclusive, what `samtools view <bam> ctg:lo-hi` selects; -1 -1: the whole contig
    uint32_t seed;                       // clair_frontend_bam_subsample: what `samtools view -s` adds to the view (subsample_core.h); frac <= 0: off
    double frac;
};
constexpr uint16_t BAM_VIEW_FILTER = 2316;

__device__ inline uint32_t bam_u32(const uint8_t *base, uint64_t off) {
    const uint32_t *w = (const uint32_t *)(base + (off & ~(uint64_t)3));
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(off & 3));
}

__device__ inline uint8_t bam_cigar_letter(uint32_t op) {
    switch (op) {
    case 0: return 'M'; case 1: return 'I'; case 2: return 'D'; case 3: return 'N'; case 4: return 'S';
    case 5: return 'H'; case 6: return 'P'; case 7: return '='; case 8: return 'X'; case 9: return 'B';
    default: return '?';
    }
}

// the binary CIGAR at `off` (n operations) through the text walker's rules
template <bool EMIT>
__device__ inline CigarWalk walk_cigar_bam(const uint8_t *rec, uint64_t off, uint32_t n, uint32_t read, clair_op_t *ops, uint32_t *op_elem, uint32_t elem0) {
    CigarWalk w;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = bam_u32(rec, off + 4ull * i);
        w.op<EMIT>((int64_t)(c >> 4), bam_cigar_letter(c & 15), read, ops, op_elem, elem0);
    }
    return w;
}

// the records as csrc/bam_record_core.h reads them: single bytes as they lie, 32-bit values as every other field here
struct BamBytes {
    const uint8_t *rec;
    __device__ uint32_t byte(uint64_t at) const { return rec[at]; }
    __device__ uint32_t le32(uint64_t at) const { return bam_u32(rec, at); }
};

// subsample_hash of the read name at `off`: n bytes, or up to an earlier NUL.  A dword at a time like every other field, never a byte load
// near the end of the buffer; the bytes of a dword go through the shared rule one by one.
__device__ inline uint32_t bam_name_hash(const uint8_t *rec, uint64_t off, uint32_t n) {
    uint32_t h = 0;
    for (uint32_t i = 0; i < n; i += 4) {
        const uint32_t w = bam_u32(rec, off + i), left = n - i;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint8_t c = (uint8_t)(w >> (8 * j));
            if (j >= left || c == 0) return h;
            h = subsample_hash(&c, 1, h);
        }
    }
    return h;
}

// one thread per record: all[k] = the line the text path would have parsed, pass[k] = 1 when `samtools view -F 2316 <bam> <region>` prints it
__global__ __launch_bounds__(256) void fe_bam_records_kernel(const uint8_t *rec, int64_t len, const int64_t *offsets, int64_t n, TextOptions opt, BamOptions bo,
                                                             TextLine *all, uint8_t *pass, TextState *state) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    TextLine out{};
    pass[k] = 0;
    const int64_t at = offsets[k];
    bool bad = at < 0 || at + 36 > len;
    uint32_t block_size = 0, l_read_name = 0, mq = 0, n_cigar = 0, flag = 0;
    int32_t ref_id = 0, pos0 = 0, l_seq = 0;
    if (!bad) {
        block_size = bam_u32(rec, at);
        bad = block_size < 32 || at + 4 + (int64_t)block_size > len;
    }
    if (!bad) {
        ref_id = (int32_t)bam_u32(rec, at + 4);
        pos0 = (int32_t)bam_u32(rec, at + 8);
        const uint32_t w3 = bam_u32(rec, at + 12), w4 = bam_u32(rec, at + 16);
        l_read_name = w3 & 0xff;
        mq = (w3 >> 8) & 0xff;
        n_cigar = w4 & 0xffff;
        flag = w4 >> 16;
        l_seq = (int32_t)bam_u32(rec, at + 20);
        bad = clair_rec::sizes_verdict(block_size, l_read_name, n_cigar, l_seq) != clair_rec::SIZES_OK;
    }
    if (bad) {                                                                // the host renderer on the same records names the field
        atomicMin(&state->malformed, (uint32_t)(k + 1));
        all[k] = out;
        return;
    }
    const uint64_t name_off = (uint64_t)at + 36, cigar_stored = name_off + l_read_name, seq_off = cigar_stored + 4ull * n_cigar;
    const uint64_t rec_end = (uint64_t)at + 4 + block_size;
    uint64_t cigar_off = cigar_stored;
    uint32_t n_ops_cigar = n_cigar;
    if (n_cigar > 0 && ref_id >= 0 && pos0 >= 0) {
        const uint32_t c0 = bam_u32(rec, cigar_stored);
        if ((c0 & 15) == 4 && (c0 >> 4) == (uint32_t)l_seq)                  // rare: look for CG:B:I (a stored CIGAR of more than 65 535 operations)
            clair_rec::real_cigar(BamBytes{rec}, seq_off + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq, rec_end, n_cigar, &cigar_off, &n_ops_cigar);
    }
    const CigarWalk w = walk_cigar_bam<false>(rec, cigar_off, n_ops_cigar, 0, nullptr, nullptr, 0);
    const int64_t pos1 = (int64_t)pos0 + 1;
    bool view = (flag & BAM_VIEW_FILTER) == 0 && ref_id == bo.tid;
    if (view && bo.region_lo >= 0 && bo.region_hi >= 0) {
        const int64_t end1 = pos1 + (w.rlen > 0 ? w.rlen : 1) - 1;          // bam_endpos
        view = pos1 <= bo.region_hi && end1 >= bo.region_lo;
    }
    if (view && bo.frac > 0.0) view = subsample_keeps(bam_name_hash(rec, name_off, l_read_name - 1), bo.seed, bo.frac);
    if (!view) { all[k] = out; return; }
    const uint32_t seq_len = l_seq > 0 ? (uint32_t)l_seq : 1u;               // SEQ '*' is one byte of text
    const bool evc_ok = (int64_t)mq >= opt.evc_min_mq && n_ops_cigar > 0 && !(1.0 - (double)w.soft / (double)(w.total + 1) < 0.55);
    bool in_region = true;
    if (opt.pile_start >= 0 && opt.pile_end >= 0) {
        const int64_t end1 = pos1 + (w.rlen > 0 ? w.rlen : 1) - 1;
        in_region = pos1 <= opt.pile_end && end1 >= opt.pile_start;
    }
    const bool candidate = in_region && (int64_t)mq >= opt.pile_min_mq;
    out.pos0 = pos0;
    out.cigar_off = (uint32_t)cigar_off; out.cigar_len = n_ops_cigar;
    out.seq_off = (uint32_t)seq_off; out.seq_len = seq_len;
    out.n_ops = w.n_ops;
    out.n_elem = w.elems > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)w.elems;
    out.flags = ((flag & 16) ? CLAIR_READ_REVERSE : 0) | (evc_ok ? CLAIR_READ_EVC : 0) | (candidate ? TL_CANDIDATE : 0) | (w.zero ? TL_ZERO_INDEL : 0)
                | (w.lead ? TL_LEAD_INDEL : 0) | (l_seq == 0 ? TL_BAM_NOSEQ : 0) | ((opt.lookup && n_ops_cigar > 0) ? TL_LOOKUP : 0)
                | ((w.rp > (int64_t)seq_len + 100000 - 64 || w.rp > 0x7fffff00 || w.qp > 0x7fffff00) ? TL_LONG_SPAN : 0)
                | ((w.rp > 0x7fffff00 || w.qp > 0x7fffff00) ? TL_OFFSETS : 0);
    out.pad_mask = opt.lookup ? w.pad_mask : 0;
    all[k] = out;
    pass[k] = 1;
}

// the records the view prints, in order: from here on they are the text path's lines
__global__ __launch_bounds__(256) void fe_bam_gather_kernel(const TextLine *all, const int64_t *shown, int64_t n_lines, TextLine *lines, uint8_t *is_candidate) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_lines) return;
    const TextLine ln = all[shown[j]];
    lines[j] = ln;
    is_candidate[j] = (ln.flags & TL_CANDIDATE) ? 1 : 0;
}

// the kept lines' alignments and their operations into the slab, from the text (`src` the text) or from the records (BAM: `src` the records)
template <bool BAM>
__global__ __launch_bounds__(256) void fe_emit_kernel(const uint8_t *src, const TextLine *lines, const int64_t *kept, int64_t n_kept, const uint32_t *op0,
                                                      const uint32_t *elem0, const uint32_t *seq0, clair_read_t *reads, clair_op_t *ops, uint32_t *op_elem,
                                                      uint64_t total_ops, uint64_t total_elems) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) op_elem[total_ops] = (uint32_t)total_elems;
    if (i >= n_kept) return;
    const TextLine ln = lines[kept[i]];
    if (BAM) (void)walk_cigar_bam<true>(src, ln.cigar_off, ln.cigar_len, (uint32_t)i, ops + op0[i], op_elem + op0[i], elem0[i]);
    else (void)walk_cigar<true>(src + ln.cigar_off, ln.cigar_len, (uint32_t)i, ops + op0[i], op_elem + op0[i], elem0[i]);
    clair_read_t r;
    r.pos0 = ln.pos0;
    r.seq0 = seq0[i];
    r.seq_len = ln.seq_len;
    r.op0 = op0[i];
    r.n_ops = ln.n_ops;
    r.flags = (ln.flags & (CLAIR_READ_REVERSE | CLAIR_READ_EVC | CLAIR_READ_PILE | CLAIR_READ_FLUSH)) | ((ln.flags & TL_LOOKUP) ? CLAIR_READ_LOOKUP : 0);
    r.reserved = (ln.flags & TL_LOOKUP) ? ln.pad_mask : 0;
    reads[i] = r;
}

// "=ACMGRSVTWYHKDBN" eight letters to a word: a 4-bit code to its letter without a table in memory
constexpr uint64_t pack8(const char *s) { uint64_t v = 0; for (int i = 7; i >= 0; --i) v = v << 8 | (uint8_t)s[i]; return v; }
constexpr uint64_t NT16_LO = pack8("=ACMGRSV"), NT16_HI = pack8("TWYHKDBN");
__device__ inline uint32_t nt16_letter(uint32_t c) { return (uint32_t)(((c & 8) ? NT16_HI : NT16_LO) >> ((c & 7) * 8)) & 0xff; }

// The 4-bit SEQ of every kept record into the slab's packed buffer as the letters `samtools view` prints: a wave per alignment, per lane and
// step two packed bytes in (bases 4k .. 4k+3), one dword out.  An odd l_seq leaves its padding nibble in the alignment's pad bytes.
__global__ __launch_bounds__(256) void fe_bam_seq_kernel(const uint8_t *rec, const TextLine *lines, const int64_t *kept, int64_t n_kept, const uint32_t *seq0, uint8_t *seq) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_kept) return;
    const int lane = threadIdx.x & 63;
    const TextLine ln = lines[kept[i]];
    uint32_t *dst = (uint32_t *)(seq + seq0[i]);
    if (ln.flags & TL_BAM_NOSEQ) { if (lane == 0) dst[0] = '*'; return; }
    const uint32_t n_dw = (ln.seq_len + 3u) >> 2;
    for (uint32_t k = (uint32_t)lane; k < n_dw; k += 64) {
        const uint32_t two = bam_u32(rec, (uint64_t)ln.seq_off + 2ull * k);
        dst[k] = nt16_letter((two >> 4) & 15) | nt16_letter(two & 15) << 8 | nt16_letter((two >> 12) & 15) << 16 | nt16_letter((two >> 8) & 15) << 24;
    }
}

}  // namespace

// what depends on the candidate list: replaced as a whole when the candidates are fixed again
struct CandidateBuffers {
    DeviceBuffer centre;                         // int64_t
    // windows
    DeviceBuffer ins;                            // uint32_t
    DeviceBuffer before_sum, prefix_block_sum;   // unsigned long long: running sum of `before` (pass 2 per operation)
    DeviceBuffer late;                           // uint32_t, --stop_consider_left_edge only
    DeviceBuffer tuple_diff;                     // int
    DeviceBuffer keep;                           // uint8_t
    DeviceBuffer window_tuples;                  // uint64_t
    DeviceBuffer kept;                           // int64_t
    DeviceBuffer block_sum;                      // uint32_t
    DeviceBuffer counts, out_centre, out_refseq; // short4, int64_t, uint8_t: sized by the kept windows of the last build
    // the paired training set over those windows (train_set.hip: clair_frontend_pair)
    DeviceBuffer ts_flags, ts_kept;              // uint8_t [3][windows + 1]: at a truth position, usable, kept non-variant; int64_t: indices of the kept windows
    DeviceBuffer ts_block_sum, ts_total;         // uint32_t
    DeviceBuffer ts_centre, ts_refseq, ts_labels, ts_in_set;   // per kept row: int64_t, uint8_t [34], uint8_t [4], uint8_t
    DeviceBuffer ts_stage;                       // the rows clair_frontend_train_set_counts gathers before they go to the host
    int64_t ts_n_kept = -1;
};

// what the last clair_frontend_gvcf_blocks call computed (gvcf.hip), kept so that a second call with the same arguments and room for the
// records only copies them
struct GvcfHeld {
    bool valid = false;
    int cost[3] = {0, 0, 0};
    uint8_t bands[CLAIR_GVCF_GQ_VALUES] = {};
    std::vector<int64_t> iv;             // starts, then ends
    int64_t n_blocks = 0;
    DeviceBuffer records, cls, totals, intervals;
    hipEvent_t began = nullptr, ended = nullptr;      // around the launches of the last computation (clair_frontend_gvcf_device_ms)
    float device_ms = -1.0f;
    ~GvcfHeld() { if (began) (void)hipEventDestroy(began); if (ended) (void)hipEventDestroy(ended); }
};

struct clair_frontend {
    int device = 0;
    hipStream_t stream = nullptr;
    Region g{};
    DeviceBuffer ref, pq, misc, anomalies;       // what `g` points into
    std::deque<Slab> slabs;                      // (a deque: a slab never moves)
    // candidates
    DeviceBuffer flags;                  // uint8_t per position
    DeviceBuffer before;                 // uint32_t, n + 1
    DeviceBuffer block_sum;              // uint32_t
    DeviceBuffer total;                  // uint32_t [2]: candidates, kept windows
    int64_t n_candidates = -1;
    DeviceBuffer bed;                    // int64_t
    std::unique_ptr<CandidateBuffers> cand{new CandidateBuffers};
    int64_t n_windows = -1;
    // text parsed on the device (clair_frontend_text_options / _add_text)
    bool text_ready = false;
    TextOptions text_opt{};
    DeviceBuffer ctg;
    TextState text_state{};
    DeviceBuffer d_text_state;           // TextState
    bool bam_mode = false;               // clair_frontend_bam_options was called last: records come through _add_bam
    BamOptions bam_opt{};
    DeviceBuffer span;                   // uint32_t: the longest reference reach of the slab being tallied (fe_slab_span_kernel)
    DeviceBuffer d2, fold;               // unsigned long long; --stop_consider_left_edge, pass 2 per operation: tuples per window as second differences over positions
    bool pass2_per_base = false;         // CLAIR_AMD_FE_PASS2=base when the handle was created: --stop_consider_left_edge's pass 2 by fe_windows_per_base_kernel
    bool tally_per_base = false;         // CLAIR_AMD_FE_TALLY=atomic when the handle was created: pass 1 by fe_tally_kernel (one device atomic per base)
    // the indel look-up (indel_lookup.hip): queries, hits per query, tables; sized by the largest call so far
    DeviceBuffer lk_pos, lk_views, lk_count, lk_hits, lk_entries, lk_n, lk_depth, lk_status;
    std::deque<SlabHostCopy> lk_host;    // slabs copied back for the host fallback, once each (a slab never changes)
    GvcfHeld gvcf;
    std::string error;

    SlabView view(const Slab &s) const {
        return SlabView{s.reads.as<clair_read_t>(), s.ops.as<clair_op_t>(), s.op_elem.as<uint32_t>(), s.seq.as<uint8_t>(), s.tuples.as<uint64_t>(),
                        (uint32_t)s.n_ops, (uint32_t)s.n_elem};
    }
};

namespace {

inline HipFail fe_fail(clair_frontend *f) { return {f ? f->error : g_fe_error}; }

inline unsigned blocks_for(int64_t n, int64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// flags[n] -> how many are set (block sums left scanned in block_sum for scan_write)
template <typename Flags> void launch_count(clair_frontend *f, Flags flags, int64_t n, uint32_t *block_sum, uint32_t *d_count) {
    const unsigned nb = blocks_for(n, SCAN_BLOCK);
    if (n > 0) hipLaunchKernelGGL((clair_scan::totals_kernel<Flags, SCAN_ITEMS>), dim3(nb), dim3(256), 0, f->stream, flags, n, block_sum);
    hipLaunchKernelGGL((clair_scan::walk_kernel<SumScan<uint32_t, uint32_t>, false>), dim3(1), dim3(256), 0, f->stream, SumScan<uint32_t, uint32_t>{block_sum}, (int64_t)nb,
                       block_sum, d_count);
}
int scan_count(clair_frontend *f, const uint8_t *flags, int64_t n, uint32_t *block_sum, uint32_t *d_count, int64_t *count, bool newlines = false) {
    if (newlines) launch_count(f, ScanNewlines{{flags}}, n, block_sum, d_count);
    else launch_count(f, ScanFlags{{flags}}, n, block_sum, d_count);
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    uint32_t total = 0;
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(&total, d_count, sizeof total, hipMemcpyDeviceToHost, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    *count = total;
    return 0;
}

// after scan_count: prefix[n + 1] (optional) and the list of flagged indices (+ list_base)
int scan_write(clair_frontend *f, const uint8_t *flags, int64_t n, uint32_t *block_sum, const uint32_t *d_count, uint32_t *prefix, int64_t *list,
               int64_t list_base, bool newlines = false) {
    // entry n of the prefix is written by the thread that owns index n: cover it with one more (empty) item
    const unsigned nb = blocks_for(n, SCAN_BLOCK), nbw = blocks_for(n + 1, SCAN_BLOCK);
    if (nbw > nb) CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(block_sum + nb, d_count, sizeof(uint32_t), hipMemcpyDeviceToDevice, f->stream));
    const WriteCompact w{prefix, list, list_base};
    const uint32_t *prefix_of_blocks = block_sum;
    if (newlines) hipLaunchKernelGGL((clair_scan::write_kernel<ScanNewlines, SCAN_ITEMS, WriteCompact>), dim3(nbw), dim3(256), 0, f->stream, ScanNewlines{{flags}}, n, prefix_of_blocks, w);
    else hipLaunchKernelGGL((clair_scan::write_kernel<ScanFlags, SCAN_ITEMS, WriteCompact>), dim3(nbw), dim3(256), 0, f->stream, ScanFlags{{flags}}, n, prefix_of_blocks, w);
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    return 0;
}

// v[n] -> its seeded inclusive running sum in 64 bits (w.out may be v); block_sum: one entry per SCAN_BLOCK items
template <typename L>
void running_sum(clair_frontend *f, decltype(L::v) v, int64_t n, unsigned long long *block_sum, const WriteRunning &w) {
    const unsigned nb = blocks_for(n, SCAN_BLOCK);
    hipLaunchKernelGGL((clair_scan::totals_kernel<L, SCAN_ITEMS>), dim3(nb), dim3(256), 0, f->stream, L{v}, n, block_sum);
    hipLaunchKernelGGL((clair_scan::walk_kernel<ScanU64, false>), dim3(1), dim3(256), 0, f->stream, ScanU64{block_sum}, (int64_t)nb, block_sum, (unsigned long long *)nullptr);
    hipLaunchKernelGGL((clair_scan::write_kernel<L, SCAN_ITEMS, WriteRunning>), dim3(nb), dim3(256), 0, f->stream, L{v}, n, (const unsigned long long *)block_sum, w);
}

void free_candidates(clair_frontend *f) {
    f->cand.reset(new CandidateBuffers);
    f->n_candidates = -1;
    f->n_windows = -1;
}

// after the flags are set: the candidate list, its per-position prefix, and room for the windows
int finish_candidates(clair_frontend *f, int64_t *n_candidates) {
    free_candidates(f);
    int64_t n = 0;
    if (scan_count(f, f->flags.as<uint8_t>(), f->g.n, f->block_sum.as<uint32_t>(), f->total.as<uint32_t>(), &n)) return 1;
    CLAIR_HIP_TRY(fe_fail(f), f->cand->centre.ensure((size_t)n * sizeof(int64_t)));
    if (scan_write(f, f->flags.as<uint8_t>(), f->g.n, f->block_sum.as<uint32_t>(), f->total.as<uint32_t>(), f->before.as<uint32_t>(), f->cand->centre.as<int64_t>(), f->g.lo + 1))
        return 1;
    f->n_candidates = n;
    *n_candidates = n;
    return 0;
}

// the bed intervals of the contig for membership only (shared/interval_tree.py:30-32, 45-57): sorted, empty intervals widened by one, merged; on the
// device in f->bed until the next call
int upload_bed(clair_frontend *f, const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, const int64_t **d_start, const int64_t **d_end, int64_t *n_merged) {
    std::vector<std::pair<int64_t, int64_t>> iv;
    for (int64_t i = 0; i < n_bed; ++i) iv.emplace_back(bed_start[i], bed_end[i] == bed_start[i] ? bed_end[i] + 1 : bed_end[i]);
    std::sort(iv.begin(), iv.end());
    std::vector<int64_t> st, en;
    for (auto &x : iv) {
        if (x.second <= x.first) continue;
        if (!st.empty() && x.first <= en.back()) en.back() = std::max(en.back(), x.second);
        else { st.push_back(x.first); en.push_back(x.second); }
    }
    const size_t m = st.size();
    CLAIR_HIP_TRY(fe_fail(f), f->bed.ensure(2 * m * sizeof(int64_t)));
    int64_t *d_bed = f->bed.as<int64_t>();
    if (m) {
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(d_bed, st.data(), m * sizeof(int64_t), hipMemcpyHostToDevice));
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(d_bed + m, en.data(), m * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    *d_start = d_bed;
    *d_end = d_bed + m;
    *n_merged = (int64_t)m;
    return 0;
}

// a slab of these sizes, owned by the handle from here on, its tuples zeroed (on the stream)
int new_slab(clair_frontend *f, int64_t n_reads, int64_t n_ops, int64_t n_elem, int64_t seq_bytes, Slab **out) {
    f->slabs.emplace_back();
    f->gvcf.valid = false;               // the tallies are about to change
    Slab &d = f->slabs.back();
    d.n_reads = n_reads; d.n_ops = n_ops; d.n_elem = n_elem; d.seq_bytes = seq_bytes;
    CLAIR_HIP_TRY(fe_fail(f), d.reads.ensure((size_t)n_reads * sizeof(clair_read_t)));
    CLAIR_HIP_TRY(fe_fail(f), d.ops.ensure((size_t)n_ops * sizeof(clair_op_t)));
    CLAIR_HIP_TRY(fe_fail(f), d.op_elem.ensure(((size_t)n_ops + 1) * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), d.seq.ensure((size_t)std::max<int64_t>(seq_bytes, 16)));
    CLAIR_HIP_TRY(fe_fail(f), d.tuples.ensure((size_t)n_reads * sizeof(uint64_t)));
    CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(d.tuples.p, 0, (size_t)n_reads * sizeof(uint64_t), f->stream));
    *out = &d;
    return 0;
}

// the part of clair_frontend_create that can fail on the device (the caller destroys the handle then)
int frontend_init(clair_frontend *f, const char *ref_seq, int64_t ref_len) {
    auto failed = [](const char *what, hipError_t err) { return err != hipSuccess && fe_fail(nullptr)("%s failed: %s", what, hipGetErrorString(err)); };
    if (failed("hipSetDevice", hipSetDevice(f->device))) return 1;
    if (failed("hipStreamCreate", hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking))) return 1;
    Region &g = f->g;
    if (failed("hipMalloc(reference)", f->ref.ensure((size_t)ref_len))) return 1;
    if (failed("hipMemcpy(reference)", hipMemcpy(f->ref.p, ref_seq, (size_t)ref_len, hipMemcpyHostToDevice))) return 1;
    const size_t table = (size_t)g.n * 32;
    if (failed("hipMalloc(read-base counters)", f->pq.ensure(table))) return 1;
    if (failed("hipMalloc(counts)", f->misc.ensure(table))) return 1;
    if (failed("hipMalloc", f->anomalies.ensure(sizeof(uint32_t)))) return 1;
    if (failed("hipMalloc(flags)", f->flags.ensure((size_t)g.n + 1))) return 1;
    if (failed("hipMalloc(prefix)", f->before.ensure(((size_t)g.n + 1) * sizeof(uint32_t)))) return 1;
    if (failed("hipMalloc", f->block_sum.ensure(((size_t)blocks_for(g.n + 1, SCAN_BLOCK) + 1) * sizeof(uint32_t)))) return 1;
    if (failed("hipMalloc", f->total.ensure(2 * sizeof(uint32_t)))) return 1;
    g.ref = f->ref.as<uint8_t>();
    g.pq = f->pq.as<unsigned long long>();
    g.misc = f->misc.as<uint32_t>();
    g.anomalies = f->anomalies.as<uint32_t>();
    (void)hipMemsetAsync(g.pq, 0, table, f->stream);
    (void)hipMemsetAsync(g.misc, 0, table, f->stream);
    (void)hipMemsetAsync(g.anomalies, 0, sizeof(uint32_t), f->stream);
    return failed("hipMemset", hipStreamSynchronize(f->stream)) ? 1 : 0;
}

}  // namespace

extern "C" {

const char *clair_frontend_last_error(const clair_frontend_t *f) { return f ? f->error.c_str() : g_fe_error.c_str(); }

int clair_frontend_create(int device, const char *ref_seq, int64_t ref_len, int64_t reference_start_0_based, int64_t span_lo, int64_t span_hi,
                          clair_frontend_t **out) {
    if (!out) return fe_fail(nullptr)("out is NULL");
    *out = nullptr;
    if (!ref_seq || ref_len < 0) return fe_fail(nullptr)("reference sequence missing");
    if (span_hi <= span_lo) return fe_fail(nullptr)("empty span [%lld, %lld)", (long long)span_lo, (long long)span_hi);
    if (span_hi - span_lo > ((int64_t)1 << 32) - 8192) return fe_fail(nullptr)("span of %lld positions is beyond one front end (2^32)", (long long)(span_hi - span_lo));
    if (hip_device_check(fe_fail(nullptr), device, "the front end runs on an MI355X only (the host code is clair_host_evc_* / clair_host_pileup_*)")) return 1;
    clair_frontend *f = new clair_frontend;
    { const char *t = getenv("CLAIR_AMD_FE_TALLY"); f->tally_per_base = t && !strcmp(t, "atomic"); }
    { const char *t = getenv("CLAIR_AMD_FE_PASS2"); f->pass2_per_base = t && !strcmp(t, "base"); }
    f->device = device;
    f->g.lo = span_lo;
    f->g.n = span_hi - span_lo;
    f->g.ref0 = reference_start_0_based;
    f->g.ref_len = ref_len;
    if (frontend_init(f, ref_seq, ref_len)) {
        clair_frontend_destroy(f);
        return 1;
    }
    *out = f;
    return 0;
}

void clair_frontend_destroy(clair_frontend_t *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    const hipStream_t stream = f->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete f;                                   // every buffer goes with its owner, after the work on the stream is done ...
    if (stream) (void)hipStreamDestroy(stream); // ... and before the stream is
}

__global__ void fe_flag_kernel(Region g, uint32_t bits) { atomicOr(g.anomalies, bits); }

// Pass 1 over one slab.  The tiled kernel wherever its assumptions hold (fewer alignments in the slab than a 21-bit counter holds, so that a
// tile's counters cannot carry into their neighbours); CLAIR_AMD_FE_TALLY=atomic keeps the per-base kernel (tests compare the two, bit for bit).
// [p_first, p_reach): reference positions the slab may touch (a generous guess is fine, see fe_tally_tile_kernel).
static int launch_tally(clair_frontend *f, const Slab &d, int64_t p_first, int64_t p_reach, bool sorted = true) {
    if (!d.n_elem) return 0;
    if (f->tally_per_base || d.n_reads >= (int64_t)PQ_MASK || !sorted) {   // the tiled kernel finds a tile's alignments by bisection over their starts
        hipLaunchKernelGGL(fe_tally_kernel, dim3(blocks_for(d.n_elem, 256)), dim3(256), 0, f->stream, f->g, f->view(d));
        return 0;
    }
    CLAIR_HIP_TRY(fe_fail(f), f->span.ensure(sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->span.p, 0, sizeof(uint32_t), f->stream));
    hipLaunchKernelGGL(fe_slab_span_kernel, dim3(blocks_for(d.n_reads, 256)), dim3(256), 0, f->stream, f->view(d), (uint32_t)d.n_reads, f->span.as<uint32_t>());
    const int64_t n_tiles = (f->g.n + TT_POS - 1) / TT_POS;
    const int64_t tile0 = std::min(std::max<int64_t>((p_first - f->g.lo) / TT_POS - (p_first < f->g.lo ? 1 : 0), 0), n_tiles - 1);
    const int64_t tile1 = std::min(std::max<int64_t>((p_reach - f->g.lo) / TT_POS, tile0), n_tiles - 1);
    hipLaunchKernelGGL(fe_tally_tile_kernel, dim3((unsigned)(tile1 - tile0 + 1)), dim3(TT_THREADS), 0, f->stream, f->g, f->view(d), (uint32_t)d.n_reads, f->span.as<const uint32_t>(), tile0);
    return 0;
}

// freed on every way out
struct DeviceTemp {
    std::vector<void *> p;
    ~DeviceTemp() { for (void *x : p) (void)hipFree(x); }
    hipError_t get(void **out, size_t bytes) { hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 16)); if (e == hipSuccess) p.push_back(*out); return e; }
};

// The lines of one chunk, parsed from text (clair_frontend_add_text) or decoded from BAM records and compacted to those the view prints
// (clair_frontend_add_bam), in lines[0 .. n_lines) with is_cand set -> --dcov, the kept lines, their offsets and the counters, the slab
// (operations and bases from `src`: the text, or the records when `bam`), its tally.  Returns 2 with *malformed = 1 + the index of the
// first malformed line / record.
static int pack_lines(clair_frontend *f, DeviceTemp &tmp, const uint8_t *src, bool bam, TextLine *lines, uint8_t *is_cand, int64_t n_lines, uint32_t *d_count,
               const TextState &carry, uint32_t *malformed) {
    int64_t *cand = nullptr, *kept = nullptr;
    uint8_t *keep = nullptr;
    uint32_t *line_sum = nullptr;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&keep, (size_t)n_lines + 1));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&line_sum, ((size_t)blocks_for(n_lines + 1, SCAN_BLOCK) + 2) * sizeof(uint32_t)));
    int64_t n_cand = 0, n_kept = 0;
    if (scan_count(f, is_cand, n_lines, line_sum, d_count + 1, &n_cand)) return 1;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&cand, (size_t)n_cand * sizeof(int64_t)));
    if (scan_write(f, is_cand, n_lines, line_sum, d_count + 1, nullptr, cand, 0)) return 1;
    if (n_cand) hipLaunchKernelGGL(fe_text_dcov_kernel, dim3(blocks_for(n_cand, 256)), dim3(256), 0, f->stream, lines, (const int64_t *)cand, n_cand, f->text_opt.dcov, carry);
    hipLaunchKernelGGL(fe_text_keep_kernel, dim3(blocks_for(n_lines, 256)), dim3(256), 0, f->stream, (const TextLine *)lines, n_lines, keep);
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    if (scan_count(f, keep, n_lines, line_sum, d_count + 2, &n_kept)) return 1;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&kept, (size_t)n_kept * sizeof(int64_t)));
    if (scan_write(f, keep, n_lines, line_sum, d_count + 2, nullptr, kept, 0)) return 1;
    uint32_t *op0 = nullptr, *elem0 = nullptr, *seq0 = nullptr;
    uint64_t *d_totals = nullptr;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&op0, (size_t)n_kept * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&elem0, (size_t)n_kept * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&seq0, (size_t)n_kept * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&d_totals, 5 * sizeof(uint64_t)));
    hipLaunchKernelGGL(fe_text_offsets_kernel, dim3(1), dim3(256), 0, f->stream, (const TextLine *)lines, n_lines, (const int64_t *)kept, n_kept, (const int64_t *)cand, n_cand,
                       op0, elem0, seq0, d_totals, carry, f->d_text_state.as<TextState>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    uint64_t totals[5] = {0, 0, 0, 0, 0};
    TextState after{};
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(&after, f->d_text_state.p, sizeof after, hipMemcpyDeviceToHost, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    if (after.malformed != 0xffffffffu) {
        *malformed = after.malformed;
        return 2;
    }
    if (totals[0] > 0xfffffff0ull || totals[1] > 0xfffffff0ull || totals[4] > 0xfffffff0ull) return fe_fail(f)("chunk too dense for 32-bit offsets: feed smaller chunks");
    after.malformed = 0;
    f->text_state = after;
    if (n_kept == 0 || totals[0] == 0) return 0;
    Slab *slab = nullptr;
    if (new_slab(f, n_kept, (int64_t)totals[0], (int64_t)totals[1], (int64_t)totals[4], &slab)) return 1;    // the bases only: the text itself is released when this call returns
    const Slab &d = *slab;
    const auto emit = bam ? fe_emit_kernel<true> : fe_emit_kernel<false>;       // same arguments; `src` is the records or the text
    const auto seq = bam ? fe_bam_seq_kernel : fe_text_seq_kernel;
    hipLaunchKernelGGL(emit, dim3(blocks_for(n_kept, 256)), dim3(256), 0, f->stream, src, (const TextLine *)lines, (const int64_t *)kept, n_kept, (const uint32_t *)op0,
                       (const uint32_t *)elem0, (const uint32_t *)seq0, d.reads.as<clair_read_t>(), d.ops.as<clair_op_t>(), d.op_elem.as<uint32_t>(), totals[0], totals[1]);
    hipLaunchKernelGGL(seq, dim3(blocks_for(n_kept, 4)), dim3(256), 0, f->stream, src, (const TextLine *)lines, (const int64_t *)kept, n_kept, (const uint32_t *)seq0,
                       d.seq.as<uint8_t>());
    // the tiled tally bisects over the slab's start positions: once the packer has seen a start go backwards (this slab or an earlier
    // one: the word is cumulative, and a start below the previous slab's last is exactly such a case) the per-base kernel is used, as
    // clair_frontend_add_reads does -- an unsorted slab is flagged AND tallied correctly on both entry points
    if (launch_tally(f, d, (int64_t)totals[3], after.last_pos + (int64_t)totals[2], !(after.anomalies & CLAIR_FE_UNSORTED))) return 1;
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    return 0;
}

int clair_frontend_add_reads(clair_frontend_t *f, const clair_read_t *reads, int64_t n_reads, const clair_op_t *ops, int64_t n_ops,
                             const uint32_t *op_elem, const uint8_t *seq, int64_t seq_bytes) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (n_reads < 0 || n_ops < 0 || seq_bytes < 0) return fe_fail(f)("negative slab size");
    if (n_reads == 0 || n_ops == 0) return 0;
    if (!reads || !ops || !op_elem || (!seq && seq_bytes > 0)) return fe_fail(f)("NULL slab array");
    if (n_ops > 0xfffffff0ll || seq_bytes > 0xfffffff0ll) return fe_fail(f)("slab too large for 32-bit offsets");
    if (f->n_candidates >= 0) return fe_fail(f)("reads cannot be added after the candidates were fixed");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    Slab *slab = nullptr;
    if (new_slab(f, n_reads, n_ops, op_elem[n_ops], seq_bytes, &slab)) return 1;
    const Slab &d = *slab;
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d.reads.p, reads, (size_t)n_reads * sizeof(clair_read_t), hipMemcpyHostToDevice, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d.ops.p, ops, (size_t)n_ops * sizeof(clair_op_t), hipMemcpyHostToDevice, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d.op_elem.p, op_elem, ((size_t)n_ops + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, f->stream));
    if (seq_bytes) CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d.seq.p, seq, (size_t)seq_bytes, hipMemcpyHostToDevice, f->stream));
    {   // where the slab lies, for the grid of the tiled tally: first and last start, the longest reach (host arrays: one look at every alignment's last operation)
        int64_t p_first = reads[0].pos0, p_last = reads[0].pos0, reach = 0;
        bool sorted = true;
        for (int64_t i = 0; i < n_reads; ++i) {
            sorted &= reads[i].pos0 >= p_last;      // p_last is still the largest start among 0 .. i-1
            p_first = std::min(p_first, reads[i].pos0);
            p_last = std::max(p_last, reads[i].pos0);
            if (reads[i].n_ops && (int64_t)reads[i].op0 + reads[i].n_ops <= n_ops) {
                const clair_op_t &o = ops[reads[i].op0 + reads[i].n_ops - 1];
                reach = std::max(reach, (int64_t)o.ref_off + (int64_t)(o.code_len >> 2));
            }
        }
        // Starts that decrease inside a slab (a direct caller of this entry point; the packers raise the same bit themselves): the tallies stay
        // right -- the per-base kernel does not care about order -- and the caller hears about it like about every other thing the reference's
        // scripts would have treated differently (they stop at the first such line): CLAIR_FE_UNSORTED in the anomaly word.
        if (!sorted) hipLaunchKernelGGL(fe_flag_kernel, dim3(1), dim3(1), 0, f->stream, f->g, (uint32_t)CLAIR_FE_UNSORTED);
        if (launch_tally(f, d, p_first, p_last + reach, sorted)) return 1;
    }
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    // the caller's arrays may be reused as soon as this returns (the packer's slab is reset): wait for the copies
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    return 0;
}

int clair_frontend_text_options(clair_frontend_t *f, const char *ctg_name, int dcov, int evc_min_mq, int pile_min_mq, int64_t pile_start, int64_t pile_end) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!ctg_name) return fe_fail(f)("contig name missing");
    if (!f->slabs.empty() && f->text_ready) return fe_fail(f)("text options cannot change once text was added");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    const size_t n = strlen(ctg_name);
    CLAIR_HIP_TRY(fe_fail(f), f->ctg.ensure(n));
    if (n) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(f->ctg.p, ctg_name, n, hipMemcpyHostToDevice));
    CLAIR_HIP_TRY(fe_fail(f), f->d_text_state.ensure(sizeof(TextState)));
    const bool have_region = pile_start >= 0 && pile_end >= 0;
    f->text_opt = TextOptions{f->ctg.as<uint8_t>(), (int)n, dcov, evc_min_mq, pile_min_mq, have_region ? pile_start : -1, have_region ? pile_end : -1, 0};
    f->text_state = TextState{};
    f->text_ready = true;
    return 0;
}

// returns 2 (not 1) when a line of the text is malformed: clair_host_sampack_feed on the same text names the line and the column
int clair_frontend_add_text(clair_frontend_t *f, const char *sam, int64_t len) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!f->text_ready) return fe_fail(f)("call clair_frontend_text_options first");
    if (f->bam_mode) return fe_fail(f)("clair_frontend_bam_options was called: records come through clair_frontend_add_bam");
    if (len < 0 || (len > 0 && !sam)) return fe_fail(f)("bad text");
    if (len == 0) return 0;
    if (len > 0x7ffffff0ll) return fe_fail(f)("text chunk of %lld bytes: at most 2 GB at a time", (long long)len);
    if (sam[len - 1] != '\n') return fe_fail(f)("the text must end at a line end");
    if (f->n_candidates >= 0) return fe_fail(f)("reads cannot be added after the candidates were fixed");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    DeviceTemp tmp;
    uint8_t *d_text = nullptr;
    uint32_t *block_sum = nullptr, *d_count = nullptr;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&d_text, (size_t)len + 16));            // fe_text_seq_kernel reads whole dwords
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&block_sum, ((size_t)blocks_for(len + 1, SCAN_BLOCK) + 2) * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&d_count, 4 * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d_text, sam, (size_t)len, hipMemcpyHostToDevice, f->stream));
    int64_t n_lines = 0;
    if (scan_count(f, d_text, len, block_sum, d_count, &n_lines, true)) return 1;
    int64_t *newline = nullptr;
    TextLine *lines = nullptr;
    uint8_t *is_cand = nullptr;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&newline, (size_t)n_lines * sizeof(int64_t)));
    if (scan_write(f, d_text, len, block_sum, d_count, nullptr, newline, 0, true)) return 1;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&lines, (size_t)n_lines * sizeof(TextLine)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&is_cand, (size_t)n_lines + 1));
    TextState carry = f->text_state;
    carry.malformed = 0xffffffffu;
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(f->d_text_state.p, &carry, sizeof carry, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(fe_text_lines_kernel, dim3(blocks_for(n_lines, 256)), dim3(256), 0, f->stream, (const uint8_t *)d_text, (const int64_t *)newline, n_lines,
                       f->text_opt, lines, is_cand, f->d_text_state.as<TextState>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    uint32_t malformed = 0;
    const int rc = pack_lines(f, tmp, d_text, false, lines, is_cand, n_lines, d_count, carry, &malformed);
    if (rc == 2)
        fe_fail(f)("line %u of this chunk (%lld lines before it) is not an alignment line the scripts accept: clair_host_sampack_feed on the same text names "
                   "the column", malformed - 1, (long long)f->text_state.lines);
    return rc;
}

int clair_frontend_bam_options(clair_frontend_t *f, int tid, int dcov, int evc_min_mq, int pile_min_mq, int64_t pile_start, int64_t pile_end,
                               int64_t region_lo, int64_t region_hi) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (tid < 0) return fe_fail(f)("reference id %d", tid);
    if (!f->slabs.empty() && f->text_ready) return fe_fail(f)("BAM options cannot change once records were added");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CLAIR_HIP_TRY(fe_fail(f), f->d_text_state.ensure(sizeof(TextState)));
    const bool have_pile = pile_start >= 0 && pile_end >= 0, have_region = region_lo >= 0 && region_hi >= 0;
    f->text_opt = TextOptions{nullptr, 0, dcov, evc_min_mq, pile_min_mq, have_pile ? pile_start : -1, have_pile ? pile_end : -1, 0};
    f->bam_opt = BamOptions{tid, have_region ? region_lo : -1, have_region ? region_hi : -1};
    f->text_state = TextState{};
    f->text_ready = true;
    f->bam_mode = true;
    return 0;
}

int clair_frontend_bam_subsample(clair_frontend_t *f, int64_t seed, double frac) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!f->text_ready || !f->bam_mode) return fe_fail(f)("call clair_frontend_bam_options first");
    if (f->text_state.lines) return fe_fail(f)("the subsample option cannot change once records were added");
    if (seed < 0 || seed > 0xffffffffll) return fe_fail(f)("subsample seed %lld: 0 .. 4294967295", (long long)seed);
    f->bam_opt.seed = (uint32_t)seed;
    f->bam_opt.frac = frac > 0.0 ? frac : 0.0;
    return 0;
}

int clair_frontend_bam_lookup(clair_frontend_t *f, int keep) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!f->text_ready || !f->bam_mode) return fe_fail(f)("call clair_frontend_bam_options first");
    if (f->text_state.lines) return fe_fail(f)("the look-up option cannot change once records were added");
    f->text_opt.lookup = keep != 0;
    return 0;
}

// returns 2 (not 1) when a record is malformed: the error names its index in this chunk (clair_host_bam_render on the same records says what)
int clair_frontend_add_bam(clair_frontend_t *f, const uint8_t *records, int64_t len, const int64_t *offsets, int64_t n_records) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!f->text_ready || !f->bam_mode) return fe_fail(f)("call clair_frontend_bam_options first");
    if (len < 0 || n_records < 0 || (n_records > 0 && (!records || !offsets))) return fe_fail(f)("bad record chunk");
    if (n_records == 0) return 0;
    if (len > 0x7ffffff0ll) return fe_fail(f)("record chunk of %lld bytes: at most 2 GB at a time", (long long)len);
    if (n_records > 0xfffffff0ll) return fe_fail(f)("%lld records in one chunk", (long long)n_records);
    if (f->n_candidates >= 0) return fe_fail(f)("reads cannot be added after the candidates were fixed");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    DeviceTemp tmp;
    uint8_t *d_rec = nullptr, *pass = nullptr, *is_cand = nullptr;
    int64_t *d_off = nullptr, *shown = nullptr;
    uint32_t *rec_sum = nullptr, *d_count = nullptr;
    TextLine *all = nullptr, *lines = nullptr;
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&d_rec, (size_t)len + 16));               // fields and bases are read as whole dwords
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&d_off, (size_t)n_records * sizeof(int64_t)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&all, (size_t)n_records * sizeof(TextLine)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&pass, (size_t)n_records + 1));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&rec_sum, ((size_t)blocks_for(n_records + 1, SCAN_BLOCK) + 2) * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&d_count, 4 * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d_rec, records, (size_t)len, hipMemcpyHostToDevice, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d_off, offsets, (size_t)n_records * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
    TextState carry = f->text_state;
    carry.malformed = 0xffffffffu;
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(f->d_text_state.p, &carry, sizeof carry, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(fe_bam_records_kernel, dim3(blocks_for(n_records, 256)), dim3(256), 0, f->stream, (const uint8_t *)d_rec, len, (const int64_t *)d_off,
                       n_records, f->text_opt, f->bam_opt, all, pass, f->d_text_state.as<TextState>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    int64_t n_lines = 0;                                                  // the records the view prints
    if (scan_count(f, pass, n_records, rec_sum, d_count + 3, &n_lines)) return 1;
    uint32_t malformed = 0;
    int rc = 0;
    if (n_lines == 0) {                                                   // nothing for the text path's kernels: the state is the carry's
        TextState after{};
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(&after, f->d_text_state.p, sizeof after, hipMemcpyDeviceToHost, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
        if (after.malformed != 0xffffffffu) { malformed = after.malformed; rc = 2; }
    } else {
        CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&shown, (size_t)n_lines * sizeof(int64_t)));
        if (scan_write(f, pass, n_records, rec_sum, d_count + 3, nullptr, shown, 0)) return 1;
        CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&lines, (size_t)n_lines * sizeof(TextLine)));
        CLAIR_HIP_TRY(fe_fail(f), tmp.get((void **)&is_cand, (size_t)n_lines + 1));
        hipLaunchKernelGGL(fe_bam_gather_kernel, dim3(blocks_for(n_lines, 256)), dim3(256), 0, f->stream, (const TextLine *)all, (const int64_t *)shown, n_lines,
                           lines, is_cand);
        CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
        rc = pack_lines(f, tmp, d_rec, true, lines, is_cand, n_lines, d_count, carry, &malformed);
    }
    if (rc == 2) fe_fail(f)("record %u of this chunk is not a well-formed BAM record", malformed - 1);
    return rc;
}

int clair_frontend_text_stats(clair_frontend_t *f, int64_t *stats) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!stats) return fe_fail(f)("stats is NULL");
    stats[0] = f->text_state.lines;
    stats[1] = f->text_state.evc_reads;
    stats[2] = f->text_state.pile_reads;
    stats[3] = (int64_t)f->text_state.anomalies;
    return 0;
}

int clair_frontend_slab_reads(clair_frontend_t *f, int64_t slab, struct clair_read *reads, int64_t capacity, int64_t *n_reads) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (slab < 0 || slab >= (int64_t)f->slabs.size()) return fe_fail(f)("slab %lld out of range [0, %lld)", (long long)slab, (long long)f->slabs.size());
    if (!n_reads) return fe_fail(f)("n_reads is NULL");
    const Slab &s = f->slabs[(size_t)slab];
    *n_reads = s.n_reads;
    if (!reads) return 0;
    if (capacity < s.n_reads) return fe_fail(f)("room for %lld alignments, the slab holds %lld", (long long)capacity, (long long)s.n_reads);
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(reads, s.reads.p, (size_t)s.n_reads * sizeof(clair_read_t), hipMemcpyDeviceToHost));
    return 0;
}

int clair_frontend_find_candidates(clair_frontend_t *f, double min_coverage, double threshold, int64_t ctg_start, int64_t ctg_end,
                                   const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, int64_t *n_candidates) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!n_candidates) return fe_fail(f)("n_candidates is NULL");
    if (n_bed > 0 && (!bed_start || !bed_end)) return fe_fail(f)("bed intervals missing");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CandidateRule rule{min_coverage, threshold, ctg_start >= 0 && ctg_end >= 0 ? ctg_start : -1, ctg_end, nullptr, nullptr, n_bed < 0 ? -1 : 0};
    if (n_bed > 0 && upload_bed(f, bed_start, bed_end, n_bed, &rule.bed_start, &rule.bed_end, &rule.n_bed)) return 1;
    hipLaunchKernelGGL(fe_candidate_flags_kernel, dim3(blocks_for(f->g.n, 256)), dim3(256), 0, f->stream, f->g, rule, f->flags.as<uint8_t>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    return finish_candidates(f, n_candidates);
}

int clair_frontend_set_candidates(clair_frontend_t *f, const int64_t *positions, int64_t n_positions, int64_t *n_candidates) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!n_candidates || (n_positions > 0 && !positions) || n_positions < 0) return fe_fail(f)("bad candidate list");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    for (int64_t i = 1; i < n_positions; ++i)
        if (positions[i] <= positions[i - 1]) {     // the sequential code keeps list order (CreateTensor.py:86-109); this path needs it ascending
            uint32_t bit = CLAIR_FE_CANDIDATES, cur = 0;
            CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(&cur, f->g.anomalies, sizeof cur, hipMemcpyDeviceToHost));
            cur |= bit;
            CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(f->g.anomalies, &cur, sizeof cur, hipMemcpyHostToDevice));
            break;
        }
    CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->flags.p, 0, (size_t)f->g.n + 1, f->stream));
    if (n_positions) {
        DeviceBuffer d_pos;
        CLAIR_HIP_TRY(fe_fail(f), d_pos.ensure((size_t)n_positions * sizeof(int64_t)));
        hipError_t err = hipMemcpyAsync(d_pos.p, positions, (size_t)n_positions * sizeof(int64_t), hipMemcpyHostToDevice, f->stream);
        if (err == hipSuccess) {
            hipLaunchKernelGGL(fe_given_flags_kernel, dim3(blocks_for(n_positions, 256)), dim3(256), 0, f->stream, d_pos.as<const int64_t>(), n_positions, f->g.lo, f->g.n,
                               f->flags.as<uint8_t>());
            err = hipStreamSynchronize(f->stream);
        }
        CLAIR_HIP_TRY(fe_fail(f), err);
    }
    return finish_candidates(f, n_candidates);
}

int clair_frontend_get_candidates(clair_frontend_t *f, int64_t *positions) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (f->n_candidates < 0) return fe_fail(f)("no candidates yet: call clair_frontend_find_candidates / _set_candidates first");
    if (f->n_candidates && !positions) return fe_fail(f)("positions is NULL");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    if (f->n_candidates) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(positions, f->cand->centre.p, (size_t)f->n_candidates * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int clair_frontend_build_windows(clair_frontend_t *f, int min_coverage, int drop_non_iupac_centre, int64_t *n_windows) {
    return clair_frontend_build_windows_ex(f, min_coverage, drop_non_iupac_centre, 1, n_windows);
}

int clair_frontend_build_windows_ex(clair_frontend_t *f, int min_coverage, int drop_non_iupac_centre, int consider_left_edge, int64_t *n_windows) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!n_windows) return fe_fail(f)("n_windows is NULL");
    if (f->n_candidates < 0) return fe_fail(f)("no candidates yet: call clair_frontend_find_candidates / _set_candidates first");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    const int64_t nc = f->n_candidates, room = std::max<int64_t>(nc, 1);
    CandidateBuffers &cb = *f->cand;
    CLAIR_HIP_TRY(fe_fail(f), cb.ins.ensure((size_t)room * N_QUAD * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.keep.ensure((size_t)room + 1));
    CLAIR_HIP_TRY(fe_fail(f), cb.window_tuples.ensure((size_t)room * sizeof(uint64_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.kept.ensure((size_t)room * sizeof(int64_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.block_sum.ensure(((size_t)blocks_for(room + 1, SCAN_BLOCK) + 1) * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(cb.ins.p, 0, cb.ins.bytes, f->stream));
    if (!consider_left_edge) {
        CLAIR_HIP_TRY(fe_fail(f), cb.late.ensure((size_t)room * N_POS * LATE_ROW * sizeof(uint32_t)));
        CLAIR_HIP_TRY(fe_fail(f), cb.tuple_diff.ensure(((size_t)room + 1) * sizeof(int)));
        CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(cb.late.p, 0, cb.late.bytes, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(cb.tuple_diff.p, 0, cb.tuple_diff.bytes, f->stream));
    }
    uint32_t *late = consider_left_edge ? nullptr : cb.late.as<uint32_t>();
    const int64_t *centre = cb.centre.as<int64_t>();
    uint64_t *window_tuples = cb.window_tuples.as<uint64_t>();
    const bool per_op = consider_left_edge || !f->pass2_per_base;
    const int64_t m2 = f->g.n + 2;
    if (per_op && nc) {      // the running sum of the candidate prefix: what lets pass 2 go operation by operation
        const int64_t m = f->g.n + 1;
        CLAIR_HIP_TRY(fe_fail(f), cb.before_sum.ensure((size_t)m * sizeof(unsigned long long)));
        CLAIR_HIP_TRY(fe_fail(f), cb.prefix_block_sum.ensure(((size_t)blocks_for(m2, SCAN_BLOCK) + 1) * sizeof(unsigned long long)));
        running_sum<ScanU32>(f, f->before.as<uint32_t>(), m, cb.prefix_block_sum.as<unsigned long long>(), WriteRunning{cb.before_sum.as<unsigned long long>(), nullptr, 0, 0});
        if (!consider_left_edge) {
            CLAIR_HIP_TRY(fe_fail(f), f->d2.ensure((size_t)m2 * sizeof(unsigned long long)));
            CLAIR_HIP_TRY(fe_fail(f), f->fold.ensure(2 * sizeof(unsigned long long)));
            CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->d2.p, 0, f->d2.bytes, f->stream));
            CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->fold.p, 0, f->fold.bytes, f->stream));
        }
    }
    unsigned long long *d2 = f->d2.as<unsigned long long>();
    Candidates c{centre, f->before.as<uint32_t>(), cb.ins.as<uint32_t>(), cb.before_sum.as<unsigned long long>(), late,
                 consider_left_edge ? nullptr : cb.tuple_diff.as<int>(), d2, f->fold.as<unsigned long long>()};
    for (Slab &s : f->slabs) {
        CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(s.tuples.p, 0, (size_t)s.n_reads * sizeof(uint64_t), f->stream));
        if (!s.n_elem || !nc) continue;
        if (consider_left_edge) hipLaunchKernelGGL(fe_windows_per_op_kernel, dim3(blocks_for(s.n_ops, 256)), dim3(256), 0, f->stream, f->g, f->view(s), c);
        else if (per_op) {
            hipLaunchKernelGGL(fe_windows_per_op_noleft_kernel, dim3(blocks_for(s.n_ops, 256)), dim3(256), 0, f->stream, f->g, f->view(s), c);
            hipLaunchKernelGGL(fe_late_starters_kernel, dim3(blocks_for(s.n_reads, 256)), dim3(256), 0, f->stream, f->g, f->view(s), c, (uint32_t)s.n_reads);
        } else hipLaunchKernelGGL(fe_windows_per_base_kernel, dim3(blocks_for(s.n_elem, 256)), dim3(256), 0, f->stream, f->g, f->view(s), c);
    }
    if (nc && late && per_op) {          // second differences -> first differences -> tuples per centre value -> per window
        for (int second = 0; second < 2; ++second)
            running_sum<ScanU64>(f, d2, m2, cb.prefix_block_sum.as<unsigned long long>(), WriteRunning{d2, f->fold.as<unsigned long long>(), second, f->g.lo});
        hipLaunchKernelGGL(fe_window_totals_at_kernel, dim3(blocks_for(nc, 256)), dim3(256), 0, f->stream, (const unsigned long long *)d2, centre, nc, f->g.lo, f->g.n, window_tuples);
    }
    WindowRule rule{min_coverage, drop_non_iupac_centre, late};
    if (nc && late && !per_op)           // per-base pass 2: tuples per window = the (signed) running sum of its range additions, by one workgroup
        hipLaunchKernelGGL((clair_scan::walk_kernel<ScanInt, true>), dim3(1), dim3(256), 0, f->stream, ScanInt{cb.tuple_diff.as<const int>()}, nc, (long long *)window_tuples,
                           (long long *)nullptr);
    if (nc) hipLaunchKernelGGL(fe_window_flags_kernel, dim3(blocks_for(nc, 256)), dim3(256), 0, f->stream, f->g, centre, nc, rule, cb.keep.as<uint8_t>(), window_tuples);
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    int64_t kept = 0;
    uint32_t *d_kept_total = f->total.as<uint32_t>() + 1;
    if (scan_count(f, cb.keep.as<uint8_t>(), nc, cb.block_sum.as<uint32_t>(), d_kept_total, &kept)) return 1;
    if (scan_write(f, cb.keep.as<uint8_t>(), nc, cb.block_sum.as<uint32_t>(), d_kept_total, nullptr, cb.kept.as<int64_t>(), 0)) return 1;
    // + one engine batch of slack is the caller's business: clair_submit_ex reads exactly n windows
    CLAIR_HIP_TRY(fe_fail(f), cb.counts.ensure((size_t)kept * WINDOW_VALUES * sizeof(int16_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.out_centre.ensure((size_t)kept * sizeof(int64_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.out_refseq.ensure((size_t)kept * 34));
    if (kept)
        hipLaunchKernelGGL(fe_assemble_kernel, dim3(blocks_for(kept * N_QUAD, 256)), dim3(256), 0, f->stream, f->g, centre, cb.kept.as<const int64_t>(), kept,
                           cb.ins.as<const uint32_t>(), (const uint32_t *)late, cb.counts.as<short4>(), cb.out_centre.as<int64_t>(), cb.out_refseq.as<uint8_t>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    f->n_windows = kept;
    cb.ts_n_kept = -1;           // a paired set is one of the windows it was made over
    *n_windows = kept;
    return 0;
}

int clair_frontend_window_info(clair_frontend_t *f, int64_t first, int64_t n, int64_t *centres, char *refseq) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (f->n_windows < 0) return fe_fail(f)("no windows yet: call clair_frontend_build_windows first");
    if (first < 0 || n < 0 || first + n > f->n_windows) return fe_fail(f)("windows [%lld, %lld) out of range [0, %lld)", (long long)first, (long long)(first + n), (long long)f->n_windows);
    if (n == 0) return 0;
    if (!centres || !refseq) return fe_fail(f)("NULL output pointer");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(centres, f->cand->out_centre.as<int64_t>() + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(refseq, f->cand->out_refseq.as<uint8_t>() + first * 34, (size_t)n * 34, hipMemcpyDeviceToHost));
    return 0;
}

int clair_frontend_window_counts(clair_frontend_t *f, int64_t first, int64_t n, int16_t *counts) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (f->n_windows < 0) return fe_fail(f)("no windows yet: call clair_frontend_build_windows first");
    if (first < 0 || n < 0 || first + n > f->n_windows) return fe_fail(f)("windows [%lld, %lld) out of range [0, %lld)", (long long)first, (long long)(first + n), (long long)f->n_windows);
    if (n == 0) return 0;
    if (!counts) return fe_fail(f)("NULL output pointer");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(counts, f->cand->counts.as<const int16_t>() + first * WINDOW_VALUES, (size_t)n * WINDOW_VALUES * sizeof(int16_t), hipMemcpyDeviceToHost));
    return 0;
}

const int16_t *clair_frontend_counts_device(clair_frontend_t *f, int64_t first) {
    if (!f || f->n_windows < 0 || first < 0 || first > f->n_windows) return nullptr;
    return f->cand->counts.as<const int16_t>() + first * WINDOW_VALUES;
}

int clair_frontend_budget_inputs(clair_frontend_t *f, int64_t slab, uint64_t *read_tuples, int64_t *centres, uint64_t *window_tuples) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (f->n_windows < 0) return fe_fail(f)("no windows yet: call clair_frontend_build_windows first");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    if (read_tuples) {
        if (slab < 0 || slab >= (int64_t)f->slabs.size()) return fe_fail(f)("slab %lld out of range [0, %lld)", (long long)slab, (long long)f->slabs.size());
        const Slab &s = f->slabs[(size_t)slab];
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(read_tuples, s.tuples.p, (size_t)s.n_reads * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (centres && f->n_candidates) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(centres, f->cand->centre.p, (size_t)f->n_candidates * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (window_tuples && f->n_candidates) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(window_tuples, f->cand->window_tuples.p, (size_t)f->n_candidates * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int clair_frontend_stats(clair_frontend_t *f, int64_t *stats) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!stats) return fe_fail(f)("stats is NULL");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    uint32_t bits = 0;
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(&bits, f->g.anomalies, sizeof bits, hipMemcpyDeviceToHost));
    int64_t reads = 0, elems = 0;
    for (const Slab &s : f->slabs) { reads += s.n_reads; elems += s.n_elem; }
    stats[0] = (int64_t)(bits | f->text_state.anomalies);
    stats[1] = (int64_t)f->slabs.size();
    stats[2] = reads;
    stats[3] = elems;
    stats[4] = f->n_candidates;
    stats[5] = f->n_windows;
    return 0;
}

}  // extern "C"

// the indel look-up over the resident slabs: its kernels and clair_frontend_indel_table (part of this translation unit: it works on the handle's slabs)
#include "indel_lookup.hip"

// the training-set builder over the tallies and the windows: clair_frontend_sample_candidates / _pair / _train_set_* (part of this translation unit too)
#include "train_set.hip"

// the gVCF stage over the tallies: reference-confidence blocks banded by a segmented scan, clair_frontend_position_tallies / _gvcf_blocks (part of this
// translation unit as well: the tallies are this handle's tables)
#include "gvcf.hip"
