// The gVCF stage on the device (docs/gvcf.md): reference-confidence blocks from the candidate search's tallies, which are still in HBM after
// find_candidates.  Part of frontend.hip's translation unit (it reads that handle's tables), like indel_lookup.hip and train_set.hip.
//
//   gv_class_kernel     one byte per table position: 255 outside the allowed set (bisection over the intervals), else the GQ band of the
//                       position under the rule of gvcf_core.h, bit 7 set where the position opens its allowed interval
//   the device-wide scan of device_scan.h under GvScan: the running value (gvcf_core.h: clair_gvcf_run) holds the heads seen, the head's
//                       offset, minimum and sum of DP, minimum GQ and the three minimum PLs since the last block head.  item() applies the
//                       rule to the tables again (the "recompute" layout: no per-position record is stored, only the class byte); the
//                       walk over the workgroup totals also yields the number of heads = blocks, before the records are allocated
//   GvWriteBlocks       the thread that owns a block's LAST position writes its record, at index (heads seen) - 1
// No atomics anywhere: every record has one writer.
namespace clair_gv {

constexpr int ITEMS = 8, TILE = 256 * ITEMS;        // positions per thread and per workgroup of the scan (clair_amd/gvcf.py: SCAN_TILE)
constexpr uint8_t OUTSIDE = 255, FIRST = 0x80;

__device__ inline void tallies_at(const Region &g, int64_t t, uint32_t n[7]) {
    const ulonglong2 w01 = *(const ulonglong2 *)(g.pq + t * 4), w23 = *(const ulonglong2 *)(g.pq + t * 4 + 2);
    const uint4 hi4 = *(const uint4 *)(g.misc + t * 8 + 4);
    n[0] = pq_field(w01.x, 2); n[1] = pq_field(w01.y, 2); n[2] = pq_field(w23.x, 2); n[3] = pq_field(w23.y, 2);
    n[4] = hi4.y; n[5] = hi4.z; n[6] = hi4.w;
}

__device__ inline clair_gvcf_site site_at(const Region &g, int64_t t, const clair_gvcf_costs &c) {
    uint32_t n[7];
    tallies_at(g, t, n);
    const int64_t i = g.lo + t - g.ref0;
    return clair_gvcf_rule(n, i >= 0 && i < g.ref_len ? clair_gvcf_ref_index(g.ref[i]) : -1, c);
}

__global__ __launch_bounds__(256) void gv_tallies_kernel(Region g, int64_t first, int64_t n, uint32_t *out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    uint32_t v[7];
    tallies_at(g, first + k, v);
    for (int j = 0; j < 7; ++j) out[k * 7 + j] = v[j];
}

__global__ __launch_bounds__(256) void gv_class_kernel(Region g, clair_gvcf_costs c, clair_gvcf_bands bands, const int64_t *iv_start, const int64_t *iv_end, int64_t n_iv,
                                                       uint8_t *cls) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= g.n) return;
    bool first = false;
    uint8_t v = OUTSIDE;
    if (clair_gvcf_allowed(iv_start, iv_end, n_iv, g.lo + t, &first)) v = (uint8_t)(bands.of[site_at(g, t, c).gq] | (first ? FIRST : 0));
    cls[t] = v;
}

struct GvScan {
    using T = clair_gvcf_run;
    Region g;
    clair_gvcf_costs c;
    const uint8_t *cls;
    static __device__ inline T identity() { return clair_gvcf_run_identity(); }
    static __device__ inline T join(const T &a, const T &b) { return clair_gvcf_run_join(a, b); }
    static __device__ inline T up(const T &x, int d) {
        T y;
        y.heads = __shfl_up(x.heads, d, 64); y.start = __shfl_up(x.start, d, 64); y.min_dp = __shfl_up(x.min_dp, d, 64); y.gq = __shfl_up(x.gq, d, 64);
        y.sum_dp = __shfl_up(x.sum_dp, d, 64);
        for (int k = 0; k < 3; ++k) y.pl[k] = __shfl_up(x.pl[k], d, 64);
        y.pad = 0;
        return y;
    }
    // a head: the first position of an allowed interval, or one whose band differs from that of the position before it
    __device__ inline bool head(int64_t i) const {
        const uint8_t v = cls[i];
        if (v == OUTSIDE) return false;
        return (v & FIRST) || i == 0 || cls[i - 1] == OUTSIDE || (cls[i - 1] & 0x7f) != (v & 0x7f);
    }
    __device__ inline bool last(int64_t i) const { return cls[i] != OUTSIDE && (i + 1 >= g.n || cls[i + 1] == OUTSIDE || head(i + 1)); }
    __device__ inline T item(int64_t i) const {
        if (cls[i] == OUTSIDE) return identity();
        return clair_gvcf_run_of(site_at(g, i, c), head(i), (uint32_t)i);
    }
};

struct GvWriteBlocks {
    static constexpr int PAST_END = 0;
    clair_gvcf_block_t *out;
    int64_t n_blocks;
    static __device__ inline clair_gvcf_run seed() { return clair_gvcf_run_identity(); }
    __device__ inline void write(const GvScan &p, int64_t i, int64_t, const clair_gvcf_run &before, const clair_gvcf_run &item) const {
        if (!p.last(i)) return;
        const clair_gvcf_run v = clair_gvcf_run_join(before, item);
        const int64_t k = (int64_t)v.heads - 1;
        if (k >= 0 && k < n_blocks) out[k] = clair_gvcf_block_of(v, p.g.lo, (uint32_t)i);      // (the bound holds by construction: the count is the scan's own)
    }
};

}  // namespace clair_gv

extern "C" {

int clair_frontend_position_tallies(clair_frontend_t *f, int64_t first, int64_t n, uint32_t *out) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (n < 0 || first < f->g.lo || first + n > f->g.lo + f->g.n) {
        fe_fail(f)("positions [%lld, %lld) lie outside the tables [%lld, %lld)", (long long)first, (long long)(first + n), (long long)f->g.lo, (long long)(f->g.lo + f->g.n));
        return 2;
    }
    if (n == 0) return 0;
    if (!out) return fe_fail(f)("NULL output pointer");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    DeviceBuffer d;
    CLAIR_HIP_TRY(fe_fail(f), d.ensure((size_t)n * 7 * sizeof(uint32_t)));
    hipLaunchKernelGGL(clair_gv::gv_tallies_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, f->stream, f->g, first - f->g.lo, n, d.as<uint32_t>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(out, d.p, (size_t)n * 7 * sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    return 0;
}

int clair_frontend_gvcf_blocks(clair_frontend_t *f, int c_match, int c_err, int c_half, const uint8_t *band_of_gq, const int64_t *iv_start, const int64_t *iv_end,
                               int64_t n_iv, clair_gvcf_block_t *out, int64_t capacity, int64_t *n_blocks) {
    using namespace clair_gv;
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!n_blocks) return fe_fail(f)("n_blocks is NULL");
    const Region &g = f->g;
    char verdict[320];
    if (clair_gvcf_check_arguments(c_match, c_err, c_half, band_of_gq, iv_start, iv_end, n_iv, g.lo, g.n, verdict, sizeof verdict)) {
        fe_fail(f)("%s", verdict);
        return 2;
    }
    if (capacity < 0 || (capacity > 0 && !out)) { fe_fail(f)("gvcf: room for %lld records at a NULL pointer", (long long)capacity); return 2; }
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    {   // tables that may be incomplete are not banded: the host twin walks the alignments itself
        uint32_t bits = 0;
        CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(&bits, g.anomalies, sizeof bits, hipMemcpyDeviceToHost));
        bits |= f->text_state.anomalies;
        if (bits) {
            fe_fail(f)("gvcf: the front end reported anomaly bits 0x%x (CLAIR_FE_*): its tallies may be incomplete, the host twin (clair_host_gvcf_*) runs instead", bits);
            return 3;
        }
    }
    GvcfHeld &h = f->gvcf;
    const int cost[3] = {c_match, c_err, c_half};
    bool same = h.valid && !memcmp(h.cost, cost, sizeof cost) && !memcmp(h.bands, band_of_gq, sizeof h.bands) && h.iv.size() == (size_t)(2 * n_iv);
    if (same && n_iv) same = !memcmp(h.iv.data(), iv_start, (size_t)n_iv * sizeof(int64_t)) && !memcmp(h.iv.data() + n_iv, iv_end, (size_t)n_iv * sizeof(int64_t));
    if (!same) {
        h.valid = false;
        memcpy(h.cost, cost, sizeof cost);
        memcpy(h.bands, band_of_gq, sizeof h.bands);
        h.iv.assign(iv_start, iv_start + n_iv);
        h.iv.insert(h.iv.end(), iv_end, iv_end + n_iv);
        h.n_blocks = 0;
        h.device_ms = 0.0f;
        if (n_iv) {
            const int64_t nb = (g.n + TILE - 1) / TILE;
            CLAIR_HIP_TRY(fe_fail(f), h.intervals.ensure((size_t)(2 * n_iv) * sizeof(int64_t)));
            CLAIR_HIP_TRY(fe_fail(f), h.cls.ensure((size_t)g.n + 1));
            CLAIR_HIP_TRY(fe_fail(f), h.totals.ensure((size_t)(nb + 1) * sizeof(clair_gvcf_run)));
            CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(h.intervals.p, h.iv.data(), h.iv.size() * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
            if (!h.began) CLAIR_HIP_TRY(fe_fail(f), hipEventCreate(&h.began));
            if (!h.ended) CLAIR_HIP_TRY(fe_fail(f), hipEventCreate(&h.ended));
            CLAIR_HIP_TRY(fe_fail(f), hipEventRecord(h.began, f->stream));
            const clair_gvcf_costs c{c_match, c_err, c_half};
            clair_gvcf_bands bands;
            memcpy(bands.of, band_of_gq, sizeof bands.of);
            const int64_t *d_iv = h.intervals.as<int64_t>();
            hipLaunchKernelGGL(gv_class_kernel, dim3(blocks_for(g.n, 256)), dim3(256), 0, f->stream, g, c, bands, d_iv, d_iv + n_iv, n_iv, h.cls.as<uint8_t>());
            const GvScan scan{g, c, h.cls.as<uint8_t>()};
            clair_gvcf_run *totals = h.totals.as<clair_gvcf_run>();
            const clair_scan::Stored<GvScan> stored{scan, totals};
            hipLaunchKernelGGL((clair_scan::totals_kernel<GvScan, ITEMS>), dim3((unsigned)nb), dim3(256), 0, f->stream, scan, g.n, totals);
            hipLaunchKernelGGL((clair_scan::walk_kernel<clair_scan::Stored<GvScan>, false>), dim3(1), dim3(256), 0, f->stream, stored, nb, totals, totals + nb);
            CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
            clair_gvcf_run grand;
            CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(&grand, totals + nb, sizeof grand, hipMemcpyDeviceToHost, f->stream));
            CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
            h.n_blocks = (int64_t)grand.heads;
            CLAIR_HIP_TRY(fe_fail(f), h.records.ensure((size_t)std::max<int64_t>(h.n_blocks, 1) * sizeof(clair_gvcf_block_t)));
            hipLaunchKernelGGL((clair_scan::write_kernel<GvScan, ITEMS, GvWriteBlocks>), dim3((unsigned)nb), dim3(256), 0, f->stream, scan, g.n,
                               (const clair_gvcf_run *)totals, GvWriteBlocks{h.records.as<clair_gvcf_block_t>(), h.n_blocks});
            CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
            CLAIR_HIP_TRY(fe_fail(f), hipEventRecord(h.ended, f->stream));
            CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
            CLAIR_HIP_TRY(fe_fail(f), hipEventElapsedTime(&h.device_ms, h.began, h.ended));
        }
        h.valid = true;
    }
    *n_blocks = h.n_blocks;
    if (capacity >= h.n_blocks && h.n_blocks > 0)
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(out, h.records.p, (size_t)h.n_blocks * sizeof(clair_gvcf_block_t), hipMemcpyDeviceToHost));
    return 0;
}

int clair_frontend_gvcf_device_ms(clair_frontend_t *f, double *ms) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!ms) return fe_fail(f)("ms is NULL");
    if (!f->gvcf.valid) return fe_fail(f)("no blocks yet: call clair_frontend_gvcf_blocks first");
    *ms = (double)f->gvcf.device_ms;
    return 0;
}

}  // extern "C"
