// The indel look-up on the device (include/clair_amd.h: clair_frontend_indel_table; the table is defined in include/clair_reads.h).
// Included at the end of frontend.hip: it works on the slabs that handle keeps in HBM.
//
// The reference asks pysam, one pileup per call, for "the most frequent inserted / deleted sequence right after this position"
// (clair/call_var.py:102-170, asked at :498-565 and :805-823).  Here all the positions a batch asks about go down in ONE call:
//   fe_lookup_scatter_kernel  a thread per operation of every slab: an M / D adds to the covering depth of the queries it lies over; an
//                             I / D that counts (indel_lookup_core.h: clair_lookup_indel_counts) bisects the sorted query positions and, on
//                             a hit, appends (rank of its alignment, slab, operation) to that query's hit list;
//   fe_lookup_group_kernel    a wave per query: hash of every hit's key, for every hit the first-ranked hit with the same hash and how many
//                             there are, a full compare of every hit with that one (a hash alone decides nothing: one mismatch hands
//                             the query to the host code), the distinct keys written in the order they were first seen.
// A query with more than LK_HITS hits, or with a hash collision, is marked CLAIR_LOOKUP_HITS and answered by the host code of
// indel_lookup_core.h over the slabs copied back -- the same bytes, just slower.  Integer work on a few thousand operations per query at
// most: nothing here is tuned beyond staying off the host.
#include "indel_lookup_core.h"

namespace {

constexpr int LK_HITS = 512;               // hits kept per query
constexpr int LK_QUERIES = 4096;           // queries per launch: LK_QUERIES * LK_HITS * 16 bytes of hit list (32 MB)

struct LookupHit { uint32_t rank, slab, op, pad; };

__device__ inline int64_t lk_lower(const int64_t *pos, int nq, int64_t p) {
    int a = 0, b = nq;
    while (a < b) { const int m = (a + b) >> 1; if (pos[m] < p) a = m + 1; else b = m; }
    return a;
}

__global__ __launch_bounds__(256) void fe_lookup_scatter_kernel(SlabView s, uint32_t n_reads, uint32_t seq_bytes, uint32_t rank0, uint32_t slab, const int64_t *pos, int nq,
                                                                uint32_t *count, LookupHit *hits, int32_t *depth) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= s.n_ops) return;
    const clair_op_t op = s.ops[j];
    if (op.read >= n_reads) return;
    const clair_read_t r = s.reads[op.read];
    if (!(r.flags & CLAIR_READ_LOOKUP)) return;
    const uint32_t code = op.code_len & 3u, len = op.code_len >> 2;
    if (code != CLAIR_OP_I) {              // covers the columns [start, start + len): the queries p with p - 1 among them (at most nq steps)
        const int64_t start = r.pos0 + (int64_t)op.ref_off;
        for (int64_t q = lk_lower(pos, nq, start + 1); q < nq && pos[q] <= start + (int64_t)len; ++q) atomicAdd(&depth[q], 1);
    }
    int64_t p1 = 0;
    if (!clair_lookup_indel_counts(r, s.ops, (int64_t)s.n_ops, (int64_t)seq_bytes, (int64_t)j, &p1)) return;
    const int64_t q = lk_lower(pos, nq, p1);
    if (q >= nq || pos[q] != p1) return;
    const uint32_t at = atomicAdd(&count[q], 1u);
    if (at < (uint32_t)LK_HITS) hits[q * LK_HITS + at] = LookupHit{rank0 + op.read, slab, j, 0u};      // beyond: the count says so, the host code answers
}

struct LookupKey { const uint8_t *bases; uint32_t meta; };      // meta = length << 8 | (1: insertion, 2: deletion); bases of an insertion only

__device__ inline LookupKey lk_key(const SlabView *views, const LookupHit &h) {
    const SlabView &v = views[h.slab];
    const clair_op_t op = v.ops[h.op];
    const clair_read_t r = v.reads[op.read];
    const bool ins = (op.code_len & 3u) == CLAIR_OP_I;
    return LookupKey{ins ? v.seq + r.seq0 + op.q_off : nullptr, (op.code_len >> 2) << 8 | (ins ? 1u : 2u)};
}

__global__ __launch_bounds__(64) void fe_lookup_group_kernel(const SlabView *views, const uint32_t *count, const LookupHit *hits, int nq, int capacity,
                                                             clair_indel_entry_t *entries, int32_t *n_entries, uint32_t *status) {
    __shared__ unsigned long long hash_l[LK_HITS];
    __shared__ uint32_t rank_l[LK_HITS], same_l[LK_HITS];
    __shared__ uint16_t first_l[LK_HITS];          // index of the first-ranked hit with this hit's hash
    __shared__ uint32_t n_rep, collided;
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= nq) return;
    const uint32_t c = count[q];
    if (c > (uint32_t)LK_HITS) {                   // (uniform: the whole wave leaves)
        if (lane == 0) { status[q] = CLAIR_LOOKUP_HITS; n_entries[q] = 0; }
        return;
    }
    if (lane == 0) { n_rep = 0; collided = 0; }
    const LookupHit *mine = hits + (size_t)q * LK_HITS;
    for (uint32_t i = (uint32_t)lane; i < c; i += 64) {
        const LookupHit h = mine[i];
        const LookupKey k = lk_key(views, h);
        unsigned long long x = 0xcbf29ce484222325ull ^ k.meta;      // FNV-1a over the key
        x *= 0x100000001b3ull;
        if (k.bases)
            for (uint32_t b = 0; b < (k.meta >> 8); ++b) { x ^= clair_lookup_upper(k.bases[b]); x *= 0x100000001b3ull; }
        hash_l[i] = x;
        rank_l[i] = h.rank;
    }
    __syncthreads();
    for (uint32_t i = (uint32_t)lane; i < c; i += 64) {
        const unsigned long long x = hash_l[i];
        uint32_t same = 0, first = i;
        for (uint32_t j = 0; j < c; ++j)
            if (hash_l[j] == x) { ++same; if (rank_l[j] < rank_l[first]) first = j; }
        same_l[i] = same;
        first_l[i] = (uint16_t)first;
        if (first == i) atomicAdd(&n_rep, 1u);
        else {                                     // equal hash: equal key?
            const LookupKey a = lk_key(views, mine[i]), b = lk_key(views, mine[first]);
            bool equal = a.meta == b.meta;
            if (equal && a.bases)
                for (uint32_t t = 0; t < (a.meta >> 8); ++t) equal = equal && clair_lookup_upper(a.bases[t]) == clair_lookup_upper(b.bases[t]);
            if (!equal) atomicOr(&collided, 1u);
        }
    }
    __syncthreads();
    if (collided) {
        if (lane == 0) { status[q] = CLAIR_LOOKUP_HITS; n_entries[q] = 0; }
        return;
    }
    const uint32_t reps = n_rep;
    if (lane == 0) { n_entries[q] = (int32_t)reps; status[q] = reps > (uint32_t)capacity ? (uint32_t)CLAIR_LOOKUP_ENTRIES : 0u; }
    for (uint32_t i = (uint32_t)lane; i < c; i += 64) {
        if (first_l[i] != i) continue;
        uint32_t at = 0;                           // distinct keys first seen before this one
        for (uint32_t j = 0; j < c; ++j) at += (first_l[j] == j && rank_l[j] < rank_l[i]) ? 1u : 0u;
        if (at >= (uint32_t)capacity) continue;
        const LookupKey k = lk_key(views, mine[i]);
        const uint32_t len = k.meta >> 8;
        uint32_t *out = (uint32_t *)(entries + (size_t)q * (size_t)capacity + at);      // 16 dwords: sign, length | count | first_rank | 50 bases | pad
        out[0] = (k.bases ? 0x01u : 0xffu) | len << 8;
        out[1] = same_l[i];
        out[2] = rank_l[i];
        for (uint32_t w = 3; w < 16; ++w) {
            uint32_t v = 0;
            for (uint32_t t = 0; t < 4; ++t) {
                const uint32_t b = w * 4 + t - 12;
                if (k.bases && b < len) v |= (uint32_t)clair_lookup_upper(k.bases[b]) << (8 * t);
            }
            out[w] = v;
        }
    }
}

// a buffer of the handle that only ever grows (the work on the stream is done whenever a call returns)
hipError_t lk_room(DeviceBuffer &b, size_t bytes) { return b.bytes >= bytes ? hipSuccess : b.ensure(bytes); }

// The queries the device handed over, on the host.  The slabs come back once per handle (a slab never changes once it is there) and stay
// for the next such call; stderr says when they are copied, because it is the slow path: a region's alignments cross the link.  Only the
// queries marked CLAIR_LOOKUP_HITS are answered here; every other one keeps the device's answer.
int lookup_on_host(clair_frontend *f, const int64_t *positions, int64_t n, const uint8_t *only, clair_indel_entry_t *entries, int capacity, int32_t *n_entries,
                   int32_t *depth, uint32_t *status) {
    size_t copied = 0;
    while (f->lk_host.size() < f->slabs.size()) {
        const Slab &d = f->slabs[f->lk_host.size()];
        SlabHostCopy c;
        c.reads.resize((size_t)d.n_reads); c.ops.resize((size_t)d.n_ops); c.seq.resize((size_t)d.seq_bytes);
        if (d.n_reads) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(c.reads.data(), d.reads.p, c.reads.size() * sizeof(clair_read_t), hipMemcpyDeviceToHost));
        if (d.n_ops) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(c.ops.data(), d.ops.p, c.ops.size() * sizeof(clair_op_t), hipMemcpyDeviceToHost));
        if (d.seq_bytes) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(c.seq.data(), d.seq.p, c.seq.size(), hipMemcpyDeviceToHost));
        copied += c.reads.size() * sizeof(clair_read_t) + c.ops.size() * sizeof(clair_op_t) + c.seq.size();
        f->lk_host.push_back(std::move(c));
    }
    int64_t handed = 0;
    for (int64_t q = 0; q < n; ++q) handed += only[q] ? 1 : 0;
    if (copied)
        fprintf(stderr, "indel look-up: %lld of %lld positions handed to the host code (more than 512 hits or a hash collision); "
                        "slabs copied back once (%.1f MB)\n", (long long)handed, (long long)n, (double)copied / 1e6);
    std::vector<ClairLookupSlab> slabs(f->slabs.size());
    for (size_t s = 0; s < slabs.size(); ++s) {
        const SlabHostCopy &c = f->lk_host[s];
        slabs[s] = ClairLookupSlab{c.reads.data(), (int64_t)c.reads.size(), c.ops.data(), (int64_t)c.ops.size(), c.seq.data(), (int64_t)c.seq.size()};
    }
    clair_indel_table_core(slabs.data(), (int64_t)slabs.size(), positions, n, only, entries, capacity, n_entries, depth, status);
    return 0;
}

}  // namespace

extern "C" int clair_frontend_indel_table(clair_frontend_t *f, const int64_t *positions, int64_t n, clair_indel_entry_t *entries, int capacity, int32_t *n_entries,
                                          int32_t *depth, uint32_t *status) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (n < 0 || capacity < 1 || capacity > 65536) return fe_fail(f)("indel table: %lld positions, capacity %d (1 .. 65536)", (long long)n, capacity);
    if (n == 0) return 0;
    if (!positions || !entries || !n_entries || !depth || !status) return fe_fail(f)("indel table: NULL array");
    for (int64_t q = 1; q < n; ++q)
        if (positions[q] <= positions[q - 1]) return fe_fail(f)("indel table: positions must ascend strictly (entry %lld)", (long long)q);
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    const size_t n_slabs = f->slabs.size();
    std::vector<SlabView> views(n_slabs);
    for (size_t s = 0; s < n_slabs; ++s) views[s] = f->view(f->slabs[s]);
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_views, std::max<size_t>(n_slabs, 1) * sizeof(SlabView)));
    if (n_slabs) CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(f->lk_views.p, views.data(), n_slabs * sizeof(SlabView), hipMemcpyHostToDevice, f->stream));
    const size_t room = (size_t)std::min<int64_t>(n, LK_QUERIES);
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_pos, room * sizeof(int64_t)));
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_count, room * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_hits, room * LK_HITS * sizeof(LookupHit)));
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_entries, room * (size_t)capacity * sizeof(clair_indel_entry_t)));
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_n, room * sizeof(int32_t)));
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_depth, room * sizeof(int32_t)));
    CLAIR_HIP_TRY(fe_fail(f), lk_room(f->lk_status, room * sizeof(uint32_t)));
    bool handed_over = false;
    for (int64_t q0 = 0; q0 < n; q0 += LK_QUERIES) {
        const int nq = (int)std::min<int64_t>(n - q0, LK_QUERIES);
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(f->lk_pos.p, positions + q0, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->lk_count.p, 0, (size_t)nq * sizeof(uint32_t), f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->lk_depth.p, 0, (size_t)nq * sizeof(int32_t), f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(f->lk_entries.p, 0, (size_t)nq * (size_t)capacity * sizeof(clair_indel_entry_t), f->stream));
        uint32_t rank0 = 0;
        for (size_t s = 0; s < n_slabs; ++s) {
            const Slab &d = f->slabs[s];
            if (d.n_ops)
                hipLaunchKernelGGL(fe_lookup_scatter_kernel, dim3(blocks_for(d.n_ops, 256)), dim3(256), 0, f->stream, views[s], (uint32_t)d.n_reads, (uint32_t)d.seq_bytes, rank0,
                                   (uint32_t)s, f->lk_pos.as<const int64_t>(), nq, f->lk_count.as<uint32_t>(), f->lk_hits.as<LookupHit>(), f->lk_depth.as<int32_t>());
            rank0 += (uint32_t)d.n_reads;
        }
        hipLaunchKernelGGL(fe_lookup_group_kernel, dim3((unsigned)nq), dim3(64), 0, f->stream, f->lk_views.as<const SlabView>(), f->lk_count.as<const uint32_t>(),
                           f->lk_hits.as<const LookupHit>(), nq, capacity, f->lk_entries.as<clair_indel_entry_t>(), f->lk_n.as<int32_t>(), f->lk_status.as<uint32_t>());
        CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(entries + (size_t)q0 * (size_t)capacity, f->lk_entries.p, (size_t)nq * (size_t)capacity * sizeof(clair_indel_entry_t), hipMemcpyDeviceToHost, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(n_entries + q0, f->lk_n.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(depth + q0, f->lk_depth.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(status + q0, f->lk_status.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
        for (int i = 0; i < nq; ++i) handed_over = handed_over || (status[q0 + i] & CLAIR_LOOKUP_HITS);
    }
    if (handed_over) {
        std::vector<uint8_t> only((size_t)n);
        for (int64_t q = 0; q < n; ++q) only[(size_t)q] = (status[q] & CLAIR_LOOKUP_HITS) ? 1 : 0;
        if (lookup_on_host(f, positions, n, only.data(), entries, capacity, n_entries, depth, status)) return 1;
        for (int64_t q = 0; q < n; ++q)
            if (only[(size_t)q]) status[q] |= CLAIR_LOOKUP_HITS;          // the caller may want to know
    }
    return 0;
}
