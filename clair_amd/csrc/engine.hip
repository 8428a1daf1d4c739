// C ABI of the MI355X engine (include/clair_amd.h): host side -- weight packing, workspaces,
// streams, launch sequence, timing.  gfx950 only; no CPU fallback: every entry point fails
// loudly when no HIP device is present.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>
#include <ctype.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.hip.h"
#include "dense.hip.h"
#include "decode.hip.h"
#include "evaluate.hip.h"
#include "ensemble.hip.h"
#include "gemm_split.hip.h"
#include "lstm32.hip.h"
#include "lstm32_pair.hip.h"
#include "lstm2_fused.hip.h"
#include "sites.hip.h"
#include "device_buffer.h"
#include "weight_images.h"

using namespace clair;

namespace {

thread_local std::string g_create_error;
thread_local std::string *g_error_sink = nullptr;   // the staging worker: failures go to the slot they belong to, clair_wait reports them

// the kernels' constants the weight images depend on (weight_images.h)
constexpr LayerSizes LAYER_SIZES = {T_POS, F_IN, HID, L3_UNITS, L4_UNITS, L5_UNITS, L34_GROUPS, L34_KS, L34_CH, L32_X_SHIFT};

struct TimedLaunch {
    int kernel;
    hipEvent_t start, stop;
};

// A LANE is what one forward pass in flight needs: a HIP stream for its kernels and the inter-kernel workspaces.  Three or four lanes fill
// the chip (clair_engine_create: as many as the process has hardware queues to spare).
struct Lane {
    hipStream_t stream = nullptr;
    DeviceBuffer zx;          // float: fragment-major x-projection, reused by both layers
    DeviceBuffer a1;          // unsigned short [2][33][max_pad][256] fp16: LSTM1 output as its 2-way split
    DeviceBuffer a2;          // float: LSTM2 output, channel-group-major: [32 groups of 8 features][33][n_pad][8]
    DeviceBuffer l4part;      // float [8 splits][max_pad rounded to 64][192] split-K partials in the accumulator layout (dense.hip.h)
    DeviceBuffer fuse_flags;  // unsigned, lstm2_fused.hip.h: [2][max_pad/32][33][8] ticket words, one error word, one claim word per workgroup (only with the fused launch)
    unsigned fuse_ticket = 0;         // ticket of the last fused forward pass on this lane
    int last_n_pad = 0;
    std::mutex order;         // one forward pass is enqueued at a time (the submitting thread and the staging worker both enqueue)
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> free_events;
    // forward passes enqueued with the fused layer-2 launch since the lane's error word was last read: what recover_fused re-runs
    struct FusedRun { const float *x; float *out; int n; int slot; };   // slot: the submit it belongs to, -1 for clair_run_resident
    std::vector<FusedRun> fused_runs;
};

// A SLOT is one submit in flight at the host boundary: its input and output buffers on both sides of the link and a stream of its own for
// the transfers, so that the copy engines move batch i+1 in and batch i-1 out while the lanes compute batch i.  Slot s computes on lane
// s % lanes; the kernels of the slots that share a lane run back to back on the lane's stream (with as many slots as
// lanes every lane idles while its only slot is on the link -- 3.9 M candidates/s of 7.5).
struct Slot {
    int lane = 0;
    hipStream_t cin = nullptr, cout = nullptr;   // the streams the batch comes in on and the results go out on (copy_mode: whose they are)
    hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_out = nullptr;   // input on the device / forward pass (and decode) finished / results on the host
    DeviceBuffer d_x;         // float [max_pad][1056]
    DeviceBuffer d_out;       // float [max_pad][90]
    PinnedBuffer h_out;       // float [max_batch][90], then (h_word_offset) the fused launch's error word
    PinnedBuffer h_x;         // float [max_batch][1056], allocated on first use
    DeviceBuffer d_counts;    // short [max_pad][1056] raw counts, allocated on first use
    DeviceBuffer d_records;   // candidates copied with the caller's stride (binary tensor records as they lie), clair_submit_ex
    PinnedBuffer h_counts;    // short [max_batch][1056]: staging of a caller's pageable count buffer (as h_x is for float input)
    // device decode (clair_submit_ex): the candidates' centre bytes in, call records out; allocated together on first use
    DeviceBuffer d_centre; PinnedBuffer h_centre;   // unsigned char [max_pad][2], pinned twin
    DeviceBuffer d_calls; PinnedBuffer h_calls;     // clair_call_t [max_pad], pinned twin
    clair_call_t *o_calls = nullptr;                // caller's array of the pending submit (NULL: no decode requested)
    // device scoring (clair_submit_eval, clair_eval): the candidates' true indices, allocated on first use
    DeviceBuffer d_labels; PinnedBuffer h_labels;   // unsigned char [max_pad][4], pinned twin
    // ensemble calling (clair_submit_ensemble, clair_ensemble_average): the running sums of ensemble.hip.h, allocated on first use
    DeviceBuffer d_acc;       // double [max_pad][90]
    // ensemble across BAMs (clair_submit_sites, clair_sites_add_rows): the candidates' reference windows on their way into the site table
    DeviceBuffer d_seq; PinnedBuffer h_seq;         // unsigned char [max_pad][33], pinned twin
    // pending host outputs of a submit
    float *o_gt21 = nullptr, *o_gt = nullptr, *o_l1 = nullptr, *o_l2 = nullptr;
    int pending_n = 0;
    bool refetch = false;     // a fused-launch recovery re-ran this slot's pass after its outputs had been fetched: fetch them again
    // hand-over to the staging worker: 0 = nothing queued, 1 = queued, 2 = enqueued on the device, 3 = failed (message in worker_error)
    int staged = 0;
    std::string worker_error;
};

// One checkpoint on the device: the tensors as the caller handed them over and the images the kernels read (weight_images.h).  A handle
// has one (image 0: clair_set_tensor, clair_finalize_weights) unless clair_ensemble_models asked for more.
struct ModelWeights {
    bool ready = false;
    std::vector<float> host_tensors[CLAIR_T_COUNT];
    DeviceBuffer bx1, bx2;    // float: gate-scaled biases [2][512] of the two layers
    DeviceBuffer wh1s, wh2s, wx1s, w4s, w3s;   // unsigned short: fp16 split MFMA fragment images (lstm32.hip.h, dense.hip.h)
    DeviceBuffer wx2s;        // unsigned short [8][2][1024][32] fp16 planes of the gate-scaled Wx2
    DeviceBuffer b4;          // float
    DeviceBuffer w5s, whs;    // unsigned short: fp16 split A fragments of the L5 branches and the heads (dense.hip.h: tail_kernel)
    DeviceBuffer b5, bh;      // float
    int w4_shift = 0;          // the W4 image is W4 * 2^w4_shift (finalize_model)
    int w3_shift = 0;          // the (W3 | b3) image is the tensor * 2^w3_shift
    int w5_shift[4] = {0, 0, 0, 0}, wh_shift[4] = {0, 0, 0, 0};   // per-branch power-of-two image shifts of those tensors
};

}  // namespace

// The site table of ensemble calling across BAMs (sites.hip.h; include/clair_amd.h: clair_sites_*).  It belongs to the engine handle: its
// kernels run on the handle's lanes, its errors are the handle's, and what is left of it goes with the handle.
struct clair_sites {
    clair_engine *e = nullptr;
    int64_t n_sites = 0, capacity = 0;      // rows in use / allocated
    DeviceBuffer key, count, acc, x, centre, seq;       // per row: int64, int, double [90], float [1056], 2 bytes, 33 bytes
    DeviceBuffer idx_key[2], idx_row[2];                // (key, row) sorted by key; `cur` is the one in use
    int cur = 0;
    // the current source
    int64_t src_n = -1;                                 // its positions (-1: no source begun)
    DeviceBuffer pos, lb, is_new, before, row_of;       // int64 [n], int64 [n], uint32 [n], uint32 [n + 1], int64 [n]
    DeviceBuffer overflow;                              // int: a site was given a 65th row
    // after clair_sites_finish
    bool finished = false;
    int64_t n_out = 0;
    DeviceBuffer keep, out_before, out_row, out_key, out_count, out_seq, avg;   // uint32 [n_sites], uint32 [n_sites + 1]; int64, int64, int, [33], float [90] per output
    DeviceBuffer gathered;                              // clair_sites_windows: the windows of a range, dense
    SiteRows rows() const { return SiteRows{key.as<int64_t>(), count.as<int>(), acc.as<double>(), x.as<float>(), centre.as<unsigned char>(), seq.as<unsigned char>()}; }
};

struct clair_engine {
    int device = 0;
    int max_batch = 0;
    int max_pad = 0;
    unsigned timing_mask = 0;   // bit k: kernel id k is bracketed by HIP events (clair_timing_enable)
    int lstm2_pair = -1;       // LSTM2 as two tiles per workgroup (lstm32_pair.hip.h): -1 = from 64 tiles (2048 candidates) on, where it wins
                               // 1-2 % (profiles/r02_lstm2_pair_by_batch.txt; at 1024 the kernel's own latency, 128 vs 81 us, costs 5 %); CLAIR_AMD_LSTM2_PAIR=0/1 forces
    std::atomic<int> lstm2_fused{0};       // layer 2 as ONE launch, projection and recurrence side by side (lstm2_fused.hip.h).  OPT-IN since round 5
                               // (CLAIR_AMD_LSTM2_FUSED=1): its zx hand-off is ordered by the L2 of ONE XCD -- the producer's stores retired into it, then
                               // its ticket -- which is how the hardware works and what every launch checks its placement for, but it is not a release
                               // the HIP memory model has a name for, and the release it does have (buffer_wbl2 per publication) costs more than the
                               // launch saves (0.5 us per write-back and XCD; even one per (direction, t) group leaves the launch
                               // slower than the two it replaces).  The default path of every handle is therefore the two launches, ordered by the
                               // stream.  What the fused launch bought on one- and two-slot handles: 104 us instead of 47 + 78 at batch 1024.
    int fused_groups = 4;      // projection workgroup groups per XCD inside the fused launch (CLAIR_AMD_FUSED_GROUPS)
    int64_t fused_launches = 0;   // fused launches of this handle so far
    int64_t fused_fault_at = 0;   // test hook CLAIR_AMD_FUSED_FAULT=k: the k-th fused launch finds logical id 0 already claimed (the kernel
                                  // raises its error word itself) and its a2 is poisoned afterwards, so only a real re-run gives right outputs
    int fused_recoveries = 0;     // passes re-run on the two-launch path after a fused launch raised its error word
    int proj2_groups = 8;      // persistent workgroup groups per XCD of the projection GEMM: 8 XCDs x 4 gate tiles x groups workgroups (see clair_engine_create)
    bool l34_stamps = false;   // CLAIR_AMD_L34_STAMPS=1: l3l4_kernel writes its per-wave phase clocks into the (dead) zx workspace for clair_debug_read(5)
    bool tap_l3 = false;   // CLAIR_AMD_TAP_L3=1: l3l4_kernel also writes l3 into the (dead) zx workspace for clair_debug_read(4)
    std::string error;
    std::list<PinnedBuffer> pinned;                  // page-locked host buffers handed to the caller (clair_pinned_alloc)
    mutable std::mutex pinned_mu;                    // the staging workers look buffers up while the caller may allocate another
    std::vector<Slot> slots;
    std::vector<std::unique_ptr<Lane>> lanes;
    std::vector<hipStream_t> copy_streams;   // owned here; the slots point into it
    int copy_mode = 3;                  // CLAIR_AMD_COPY_STREAMS=slot|two|lane|in (0, 1, 2, 3): see clair_engine_create
    bool convert_on_lane = true;        // CLAIR_AMD_CONVERT=copy: the int16 -> float32 conversion behind the copy on the incoming stream instead of on the lane
    bool d2h_kernel = true;             // CLAIR_AMD_D2H=sdma: results fetched by the copy engine instead of written to page-locked host memory by a kernel
    // the staging worker (clair_submit* on pageable memory): the copy of the caller's batch into page-locked memory and the enqueue of its
    // transfers and kernels run on this thread, so that the submitting thread is free after a few microseconds, as the reference's
    // predict thread leaves load and output to two others (clair/call_var.py:1331-1352)
    struct Request {
        const void *input; bool counts; int64_t stride; int n;
        const uint8_t *centre; clair_call_t *calls; float *gt21, *gt, *l1, *l2;
        const uint8_t *labels = nullptr;   // clair_submit_eval: [n][4] true indices, scored behind the forward pass
        int models = 0;                    // clair_submit_ensemble: this many forward passes, one per weight image, averaged (0: image 0 alone, as it is)
        clair_sites *sites = nullptr;      // clair_submit_sites: the passes are folded into this table's rows of candidates [sites_first, sites_first + n) of its source
        int64_t sites_first = 0;
        const uint8_t *seq = nullptr;      // their reference windows, [n][33]
    };
    int staging_threads = 2;            // CLAIR_AMD_STAGING_THREADS (0: everything on the submitting thread): a 4.3 MB batch takes one core ~100 us
                                        // to copy, 75 % of the 135 us the GPU needs for it
    std::vector<std::thread> workers;
    std::mutex wmu;
    std::condition_variable wcv, wdone;
    std::deque<std::pair<int, Request>> wqueue;
    bool wstop = false;
    // weight images: models[0] is the handle's own checkpoint; clair_ensemble_models adds up to CLAIR_ENSEMBLE_MAX_MODELS - 1 more
    std::vector<std::unique_ptr<ModelWeights>> models;
    DeviceBuffer eval_counts; // unsigned long long [CLAIR_EVAL_COUNTS] confusion counters of evaluate.hip.h, allocated by the first clair_eval_* call
    std::list<std::unique_ptr<clair_sites>> tables;   // site tables of clair_sites_create not yet destroyed
    double ms_sum[CLAIR_K_COUNT] = {0};
    int64_t launches[CLAIR_K_COUNT] = {0};
};

namespace {

int fail(clair_engine *e, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g_error_sink) *g_error_sink = buf; else if (e) e->error = buf; else g_create_error = buf;
    return 1;
}

#define HIP_TRY(e, call)                                                                        \
    do {                                                                                        \
        hipError_t err__ = (call);                                                              \
        if (err__ != hipSuccess)                                                                \
            return fail((e), "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

// a weight image to the device, into an allocation of its own size
template <typename T> int upload(clair_engine *e, DeviceBuffer &dst, const std::vector<T> &src) {
    dst.reset();
    HIP_TRY(e, dst.ensure(src.size() * sizeof(T)));
    HIP_TRY(e, hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

hipEvent_t get_event(Lane &l) {
    if (!l.free_events.empty()) {
        hipEvent_t ev = l.free_events.back();
        l.free_events.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
}

struct KernelTimer {
    clair_engine *e; Lane &l; int id; hipEvent_t start = nullptr, stop = nullptr;
    KernelTimer(clair_engine *e_, Lane &l_, int id_) : e(e_), l(l_), id(id_) {
        if ((e->timing_mask >> id) & 1u) { start = get_event(l); stop = get_event(l); (void)hipEventRecord(start, l.stream); }
    }
    ~KernelTimer() {
        if (start) { (void)hipEventRecord(stop, l.stream); l.timed.push_back({id, start, stop}); }
    }
};

int quiesce(clair_engine *e);

int drain_timers(clair_engine *e) {
    if (quiesce(e)) return 1;           // nothing is being enqueued (and timed) while the lists are read
    for (auto &lp : e->lanes) {
        Lane &l = *lp;
        HIP_TRY(e, hipStreamSynchronize(l.stream));
        for (auto &t : l.timed) {
            float ms = 0.f;
            HIP_TRY(e, hipEventElapsedTime(&ms, t.start, t.stop));
            e->ms_sum[t.kernel] += ms;
            e->launches[t.kernel] += 1;
            l.free_events.push_back(t.start);
            l.free_events.push_back(t.stop);
        }
        l.timed.clear();
    }
    return 0;
}

bool fused_possible(const clair_engine *e) { return e->lstm2_fused == 1; }
bool use_lstm2_fused(const clair_engine *e, int ntiles) {   // pairs of tiles share a 64-row activation tile: even tile counts only
    if ((ntiles & 1) || !fused_possible(e)) return false;
    return e->lstm2_fused == 1 || (ntiles >= 16 && ntiles <= 64);   // 512 .. 2048 candidates: beyond, every kernel fills the chip by itself and
                                                                    // 128 projection workgroups are too few (batch 4096, one slot: 6.6 against 7.2 M/s)
}
size_t fuse_words(int max_pad) { return (size_t)2 * (max_pad / 32) * T_POS * 8; }                  // ticket words of the zx blocks
size_t fuse_claims(const clair_engine *e) { return (size_t)32 * e->fused_groups + 32 * ((e->max_pad / 64 + 7) / 8); }   // one per workgroup of the largest launch
bool use_lstm2_pair(const clair_engine *e, int ntiles) { return e->lstm2_pair < 0 ? ntiles >= 64 : e->lstm2_pair == 1; }

// Enqueue the forward pass for n candidates whose input is at x_dev ([n_pad][1056], rows >= n
// zero or any finite value) writing packed outputs to out_dev ([n][90]).
int enqueue_forward(clair_engine *e, Lane &l, const ModelWeights &w, const float *x_dev, float *out_dev, int n, int slot_index) {
    const int n_pad = (n + 31) & ~31;
    const int ntiles = n_pad / L32_TILE;
    const int m_rows = T_POS * n_pad;
    l.last_n_pad = n_pad;
    {   // LSTM1 with its input projection fused in (no separate GEMM, no zx round trip), fp16 split products
        KernelTimer kt(e, l, CLAIR_K_LSTM1);
        Lstm32Args a{x_dev, w.wx1s.as<unsigned short>(), w.bx1.as<float>(), nullptr, w.wh1s.as<unsigned short>(), l.a1.as<unsigned short>(), nullptr, n_pad, ntiles, -1};
        hipLaunchKernelGGL((lstm32_kernel<true>), dim3(ntiles * 2), dim3(256), 0, l.stream, a);
    }
    if (use_lstm2_fused(e, ntiles)) {   // layer 2 in one launch: projection and recurrence side by side, zx through L2 (lstm2_fused.hip.h)
        KernelTimer kt(e, l, CLAIR_K_LSTM2);
        const int groups = e->fused_groups;
        if (++l.fuse_ticket == 0) l.fuse_ticket = 1;   // (a wrapped ticket could meet a 4-billion-passes-old word; the words are zero at most once)
        Lstm2FusedArgs a{GemmSplitArgs{l.a1.as<unsigned short>(), w.wx2s.as<unsigned short>(), w.bx2.as<float>(), l.zx.as<float>(), n_pad, ntiles, m_rows, groups},
                         Lstm32Args{nullptr, nullptr, nullptr, l.zx.as<float>(), w.wh2s.as<unsigned short>(), nullptr, l.a2.as<float>(), n_pad, ntiles, -1},
                         FuseArgs{l.fuse_flags.as<unsigned>(), l.fuse_ticket, l.fuse_flags.as<unsigned>() + fuse_words(e->max_pad) + 1, l.fuse_flags.as<unsigned>() + fuse_words(e->max_pad)}, 32 * groups};
        const int consumers = 32 * ((ntiles / 2 + 7) / 8);
        const bool fault = ++e->fused_launches == e->fused_fault_at;
        if (fault) HIP_TRY(e, hipMemsetD32Async((hipDeviceptr_t)a.f.claims, (int)l.fuse_ticket, 1, l.stream));
        hipLaunchKernelGGL(lstm2_fused_kernel, dim3(32 * groups + consumers), dim3(256), 0, l.stream, a);
        if (fault) HIP_TRY(e, hipMemsetAsync(l.a2.as<float>(), 0x7f, (size_t)T_POS * n_pad * 256 * sizeof(float), l.stream));
        l.fused_runs.push_back({x_dev, out_dev, n, slot_index});
    } else {
        {   // LSTM2 input projection on the fp16 matrix cores, fp32-grade via the 2-way split; weight-stationary persistent workgroups
            KernelTimer kt(e, l, CLAIR_K_PROJ2);
            const int x_tiles = (m_rows + GS_ROWS - 1) / GS_ROWS;
            const int groups = std::min(e->proj2_groups, (x_tiles + 7) / 8);
            GemmSplitArgs a{l.a1.as<unsigned short>(), w.wx2s.as<unsigned short>(), w.bx2.as<float>(), l.zx.as<float>(), n_pad, ntiles, m_rows, groups};
            hipLaunchKernelGGL(gemm_split_kernel, dim3(32 * groups), dim3(256), 0, l.stream, a);
        }
        {
            KernelTimer kt(e, l, CLAIR_K_LSTM2);
            if (use_lstm2_pair(e, ntiles)) {
                Lstm32PairArgs a{l.zx.as<float>(), w.wh2s.as<unsigned short>(), l.a2.as<float>(), n_pad, ntiles};
                hipLaunchKernelGGL(lstm32_pair_kernel, dim3(((ntiles + 1) / 2) * 2), dim3(256), 0, l.stream, a);
            } else {
                Lstm32Args a{nullptr, nullptr, nullptr, l.zx.as<float>(), w.wh2s.as<unsigned short>(), nullptr, l.a2.as<float>(), n_pad, ntiles, -1};
                hipLaunchKernelGGL((lstm32_kernel<false>), dim3(ntiles * 2), dim3(256), 0, l.stream, a);
            }
        }
    }
    {   // L3 (slice dense) + L4 (split-K 8: a workgroup walks the four channel groups of its split), fused
        KernelTimer kt(e, l, CLAIR_K_L4);
        L3L4Args a{l.a2.as<float>(), w.w3s.as<unsigned short>(), w.w4s.as<unsigned short>(), l.l4part.as<float>(), n_pad, std::ldexp(1.0f, -w.w3_shift), e->tap_l3 ? l.zx.as<float>() : nullptr,
                   e->l34_stamps ? l.zx.as<unsigned long long>() : nullptr};   // zx is dead by now
        hipLaunchKernelGGL(l3l4_kernel, dim3(l34_grid((n_pad + L34_CAND - 1) / L34_CAND)), dim3(L34_THREADS), 0, l.stream, a);
    }
    {
        KernelTimer kt(e, l, CLAIR_K_TAIL);
        TailArgs a{l.l4part.as<float>(), w.b4.as<float>(), w.w5s.as<unsigned short>(), w.b5.as<float>(), w.whs.as<unsigned short>(), w.bh.as<float>(), out_dev, n_pad, n, std::ldexp(1.0f, -w.w4_shift) / L34_ACT_SCALE, {}, {}};
        for (int k = 0; k < 4; ++k) {
            a.l5_scale[k] = std::ldexp(1.0f, -w.w5_shift[k]) / TAIL_ACT_SCALE;
            a.head_scale[k] = std::ldexp(1.0f, -w.wh_shift[k]) / TAIL_ACT_SCALE;
        }
        hipLaunchKernelGGL(tail_kernel, dim3(n_pad / TAIL_TILE), dim3(TAIL_THREADS), 0, l.stream, a);
    }
    HIP_TRY(e, hipGetLastError());
    return 0;
}

// A slot's page-locked input buffer exists from its first use -- by a staging worker (pageable float input) or by the caller
// (clair_slot_input), whichever comes first: one allocation, under the lock the look-ups below take.
int ensure_slot_input(clair_engine *e, Slot &s) {
    std::lock_guard<std::mutex> g(e->pinned_mu);
    HIP_TRY(e, s.h_x.ensure((size_t)e->max_batch * CLAIR_INPUT_FLOATS * sizeof(float)));
    return 0;
}

// The other buffers a slot has from their first use on (each keeps what it has once it has it): raw counts on the device and the
// page-locked staging of a caller's pageable ones; records as they lie, `span` bytes of them, grown when a batch needs more, then to what
// a full batch of this stride takes; the decode's centre bytes and call records, and the scoring's true indices, on both sides of the link.
int ensure_slot_counts(clair_engine *e, Slot &s) { HIP_TRY(e, s.d_counts.ensure((size_t)e->max_pad * CLAIR_INPUT_FLOATS * sizeof(short))); return 0; }
int ensure_slot_counts_staging(clair_engine *e, Slot &s) { HIP_TRY(e, s.h_counts.ensure((size_t)e->max_batch * CLAIR_INPUT_FLOATS * sizeof(short))); return 0; }
int ensure_slot_records(clair_engine *e, Slot &s, size_t span, size_t stride) {
    if (s.d_records.bytes < span) HIP_TRY(e, s.d_records.ensure(std::max(span, (size_t)e->max_batch * stride)));
    return 0;
}
int ensure_slot_decode(clair_engine *e, Slot &s) {
    HIP_TRY(e, s.d_centre.ensure((size_t)e->max_pad * 2));
    HIP_TRY(e, s.h_centre.ensure((size_t)e->max_batch * 2));
    HIP_TRY(e, s.d_calls.ensure((size_t)e->max_pad * sizeof(clair_call_t)));
    HIP_TRY(e, s.h_calls.ensure((size_t)e->max_batch * sizeof(clair_call_t)));
    return 0;
}
int ensure_slot_labels(clair_engine *e, Slot &s) {
    HIP_TRY(e, s.d_labels.ensure((size_t)e->max_pad * 4));
    HIP_TRY(e, s.h_labels.ensure((size_t)e->max_batch * 4));
    return 0;
}

// does [p, p + len) lie inside a buffer of clair_pinned_alloc?  (then the DMA engine can read it directly)
bool in_pinned(const clair_engine *e, const void *p, size_t len) {
    std::lock_guard<std::mutex> g(e->pinned_mu);
    for (const auto &b : e->pinned)
        if ((const char *)p >= b.as<char>() && (const char *)p + len <= b.as<char>() + b.bytes) return true;
    return false;
}

// memory of this process's HIP devices (hipMalloc), as opposed to anything the host allocated
bool is_device_pointer(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice;
}

// n candidates of `row` bytes each, `stride` bytes apart in the caller's buffer (0: dense), into a dense staging buffer
void gather_rows(void *dst, const void *src, int n, size_t row, int64_t stride) {
    if (stride == 0 || (size_t)stride == row) { memcpy(dst, src, (size_t)n * row); return; }
    for (int i = 0; i < n; ++i) memcpy((char *)dst + (size_t)i * row, (const char *)src + (size_t)i * (size_t)stride, row);
}

// The decode of the slot's batch on the device (decode.hip.h): probabilities in d_out + window in d_x + centre bytes -> call records.
int enqueue_decode(clair_engine *e, Lane &l, Slot &s, int n) {
    KernelTimer kt(e, l, CLAIR_K_DECODE);
    DecodeArgs a{s.d_x.as<float>(), s.d_out.as<float>(), s.d_centre.as<unsigned char>(), s.d_calls.as<clair_call_t>(), n};
    hipLaunchKernelGGL(decode_kernel, dim3((n + 3) / 4), dim3(256), 0, l.stream, a);
    HIP_TRY(e, hipGetLastError());
    return 0;
}

// The scoring of the slot's batch on the device (evaluate.hip.h): probabilities in d_out + true indices -> the handle's counter block.
// It has no id in enum clair_kernel_id (callers size arrays by CLAIR_K_COUNT), so clair_kernel_times does not see it.
static_assert(EVAL_COUNTS == CLAIR_EVAL_COUNTS, "evaluate.hip.h and include/clair_amd.h disagree on the counter block");
int enqueue_eval(clair_engine *e, Lane &l, Slot &s, int n) {
    EvalArgs a{s.d_out.as<float>(), s.d_labels.as<unsigned char>(), e->eval_counts.as<unsigned long long>(), n};
    hipLaunchKernelGGL(eval_kernel, dim3((n + EVAL_CAND - 1) / EVAL_CAND), dim3(256), 0, l.stream, a);
    HIP_TRY(e, hipGetLastError());
    return 0;
}

// The averaging step of ensemble calling (ensemble.hip.h) behind one of the K forward passes of the slot's batch: d_out -> the slot's sums, or
// (last) sums -> d_out.  No id in enum clair_kernel_id, like the scoring.
int ensure_slot_ensemble(clair_engine *e, Slot &s) { HIP_TRY(e, s.d_acc.ensure((size_t)e->max_pad * OUT_FLOATS * sizeof(double))); return 0; }
int enqueue_ensemble(clair_engine *e, Lane &l, Slot &s, int n, int models, bool first, bool last) {
    EnsembleArgs a{s.d_out.as<float>(), s.d_acc.as<double>(), n * OUT_FLOATS / 2, models, first ? 1 : 0, last ? 1 : 0};
    hipLaunchKernelGGL(ensemble_kernel, dim3((a.n_pairs + 255) / 256), dim3(256), 0, l.stream, a);
    HIP_TRY(e, hipGetLastError());
    return 0;
}

// The site table's steps behind a forward pass of the slot's batch (sites.hip.h): window, centre and seq into the rows that are new, then d_out
// into the rows' sums.  `first`: where the batch begins in the table's current source.  No id in enum clair_kernel_id, like the averaging.
int ensure_slot_sites(clair_engine *e, Slot &s) {
    HIP_TRY(e, s.d_seq.ensure((size_t)e->max_pad * SITE_SEQ));
    HIP_TRY(e, s.h_seq.ensure((size_t)e->max_batch * SITE_SEQ));
    return 0;
}
int enqueue_sites_adopt(clair_engine *e, Lane &l, Slot &s, clair_sites *t, int64_t first, int n, bool with_x) {
    hipLaunchKernelGGL(sites_adopt_kernel, dim3((n + 3) / 4), dim3(256), 0, l.stream, t->rows(), t->row_of.as<int64_t>() + first, n,
                       with_x ? s.d_x.as<float>() : nullptr, s.d_centre.as<unsigned char>(), s.d_seq.as<unsigned char>());
    HIP_TRY(e, hipGetLastError());
    return 0;
}
int enqueue_sites_accumulate(clair_engine *e, Lane &l, Slot &s, clair_sites *t, int64_t first, int n) {
    const int n_pairs = n * OUT_FLOATS / 2;
    hipLaunchKernelGGL(sites_accumulate_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, l.stream, t->rows(), t->row_of.as<int64_t>() + first, n_pairs,
                       s.d_out.as<float>(), t->overflow.as<int>());
    HIP_TRY(e, hipGetLastError());
    return 0;
}

// the counter block exists (zeroed) from the first call that needs it
int ensure_eval_counts(clair_engine *e) {
    if (!e->eval_counts.p) {
        HIP_TRY(e, e->eval_counts.ensure((size_t)CLAIR_EVAL_COUNTS * sizeof(unsigned long long)));
        HIP_TRY(e, hipMemset(e->eval_counts.p, 0, (size_t)CLAIR_EVAL_COUNTS * sizeof(unsigned long long)));
        HIP_TRY(e, hipStreamSynchronize(nullptr));   // a memset of device memory may return before it ran; the lanes' streams do not wait for the null stream
    }
    return 0;
}

// true indices in range?  (evaluate.hip.h indexes its histogram with them)
int check_labels(clair_engine *e, const uint8_t *labels, int n) {
    for (int i = 0; i < n; ++i) {
        const uint8_t *l = labels + (size_t)i * 4;
        if (l[0] >= CLAIR_GT21 || l[1] >= CLAIR_GENOTYPE || l[2] >= CLAIR_INDEL_LEN || l[3] >= CLAIR_INDEL_LEN)
            return fail(e, "label of candidate %d out of range: gt21 %d (< 21), genotype %d (< 3), lengths %d %d (< 33)", i, l[0], l[1], l[2], l[3]);
    }
    return 0;
}

// lstm2_fused.hip.h hands zx over through the L2 of the XCD its workgroups find themselves on; if the placement rule it relies on
// did not hold (a logical id claimed twice, a wait that ran out) a workgroup raised the word behind the slot's tickets and the
// results of the slot's fused passes cannot be trusted.  The reference never drops a batch (clair/call_var.py:1331-1352), so
// neither does this: the fused launch is switched off for the rest of the handle's life, the affected passes are enqueued again
// on the two-launch path (same arithmetic, bit-identical outputs) and the caller sees success; stderr gets one line.
// Called with the lane's order lock held; waits for the lane first.  Slots other than `current` whose pass was re-run fetch their
// outputs again when they are waited for (Slot::refetch).
int recover_fused(clair_engine *e, Lane &l, int current) {
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    HIP_TRY(e, hipMemsetAsync(l.fuse_flags.as<unsigned>() + fuse_words(e->max_pad), 0, sizeof(unsigned), l.stream));
    if (e->lstm2_fused != 0)
        fprintf(stderr, "clair_amd: the fused layer-2 launch found its blocks placed differently from what it assumes (a logical id claimed twice, or "
                        "a bounded wait that ran out); re-running %d pass(es) on the two-launch path and keeping it for this handle\n", (int)l.fused_runs.size());
    e->lstm2_fused = 0;
    std::vector<Lane::FusedRun> runs;
    runs.swap(l.fused_runs);
    for (const auto &r : runs) {
        if (enqueue_forward(e, l, *e->models[0], r.x, r.out, r.n, r.slot)) return 1;   // (a handle with the fused launch runs no ensembles)
        if (r.slot >= 0 && r.slot != current) e->slots[r.slot].refetch = true;
        ++e->fused_recoveries;
    }
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    return 0;
}

int check_fused_placement(clair_engine *e) {
    for (auto &lp : e->lanes) {
        Lane &l = *lp;
        if (!l.fuse_flags.p) continue;
        std::lock_guard<std::mutex> g(l.order);
        if (!l.fused_runs.empty()) {
            unsigned bad = 0;
            HIP_TRY(e, hipMemcpy(&bad, l.fuse_flags.as<unsigned>() + fuse_words(e->max_pad), sizeof bad, hipMemcpyDeviceToHost));
            if (bad && recover_fused(e, l, -1)) return 1;
        }
        l.fused_runs.clear();
    }
    return 0;
}

// raw counts -> network input (clair/utils.py:96-98): one (position, row) quad of four channels per thread
__global__ __launch_bounds__(256) void counts_to_input_kernel(const short4 *counts, f32x4 *x, int n_quads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_quads) return;
    const short4 c = counts[i];
    const float c0 = (float)c.x;
    x[i] = (f32x4){c0, (float)c.y - c0, (float)c.z - c0, (float)c.w - c0};
}

// the same for candidates `stride` bytes apart (binary tensor records copied as they lie): quad i = candidate i / 264, quad i % 264 of it
__global__ __launch_bounds__(256) void counts_to_input_strided_kernel(const char *base, size_t stride, f32x4 *x, int n_quads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_quads) return;
    const int cand = i / (CLAIR_INPUT_FLOATS / 4), q = i - cand * (CLAIR_INPUT_FLOATS / 4);
    const short4 c = *(const short4 *)(base + (size_t)cand * stride + (size_t)q * 8);
    const float c0 = (float)c.x;
    x[i] = (f32x4){c0, (float)c.y - c0, (float)c.z - c0, (float)c.w - c0};
}


// Where the fused launch's error word lives in a slot's page-locked output buffer, in floats: the first 16-byte boundary past the
// last uint4 the result kernel below may write for a full batch (it copies the probabilities as WHOLE vectors: for an odd n the last
// one reaches 8 bytes past n * 360), so that neither that vector nor the end of the allocation can touch the word.
inline size_t h_word_offset(int max_batch) { return ((((size_t)max_batch * OUT_FLOATS * sizeof(float) + 15) / 16) * 16) / sizeof(float); }
inline size_t h_out_floats(int max_batch) { return h_word_offset(max_batch) + 4; }

// results of a forward pass (and decode) to the slot's page-locked buffers, written by the GPU itself: no copy engine, no queue switch
__global__ __launch_bounds__(256) void results_to_host_kernel(const uint4 *out, uint4 *h_out, int out_vec, const uint4 *calls, uint4 *h_calls, int call_vec,
                                                             const unsigned *word, unsigned *h_word) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < out_vec) h_out[i] = out[i];
    else if (i - out_vec < call_vec) h_calls[i - out_vec] = calls[i - out_vec];
    if (i == 0 && word) *h_word = *word;
}

// The way back: call records, probabilities and the fused launch's error word into the slot's page-locked buffers, on the slot's
// outgoing stream (which may be the lane's own), then the event clair_wait sleeps on.
int enqueue_results(clair_engine *e, Lane &l, Slot &s, int n, bool calls, bool probs) {
    unsigned *word = l.fuse_flags.p ? l.fuse_flags.as<unsigned>() + fuse_words(e->max_pad) : nullptr;
    unsigned *h_word = (unsigned *)(s.h_out.as<float>() + h_word_offset(e->max_batch));
    if (e->d2h_kernel) {
        const int out_vec = probs ? (n * OUT_FLOATS * (int)sizeof(float) + 15) / 16 : 0, call_vec = calls ? n * (int)sizeof(clair_call_t) / 16 : 0;
        hipLaunchKernelGGL(results_to_host_kernel, dim3((std::max(out_vec + call_vec, 1) + 255) / 256), dim3(256), 0, s.cout, s.d_out.as<uint4>(), s.h_out.as<uint4>(), out_vec,
                           s.d_calls.as<uint4>(), s.h_calls.as<uint4>(), call_vec, word, h_word);
    } else {
        if (calls) HIP_TRY(e, hipMemcpyAsync(s.h_calls.p, s.d_calls.p, (size_t)n * sizeof(clair_call_t), hipMemcpyDeviceToHost, s.cout));
        if (probs) HIP_TRY(e, hipMemcpyAsync(s.h_out.p, s.d_out.p, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyDeviceToHost, s.cout));
        if (word) HIP_TRY(e, hipMemcpyAsync(h_word, word, sizeof(unsigned), hipMemcpyDeviceToHost, s.cout));
    }
    HIP_TRY(e, hipEventRecord(s.ev_out, s.cout));
    return 0;
}

// Everything one submit puts on the device, in order: the batch over the link on the slot's copy stream (through page-locked staging
// when the caller's memory is pageable), the forward pass (and the decode) on the slot's lane once the batch has arrived, the results
// back over the link once the lane is done.  Runs on the submitting thread or on the staging worker.
int enqueue_request(clair_engine *e, int slot_index, const clair_engine::Request &q) {
    Slot &s = e->slots[slot_index];
    Lane &l = *e->lanes[s.lane];
    const int n = q.n, n_pad = (n + 31) & ~31;
    const bool want_probs = q.gt21 != nullptr;
    const bool same_in = s.cin == l.stream, same_out = s.cout == l.stream;     // copy_mode "lane": copies in line with the kernels, no events
    std::unique_lock<std::mutex> whole(l.order, std::defer_lock);
    if (same_in) whole.lock();
    // A caller's buffer from clair_pinned_alloc (or the slot's own input buffer) is read by the DMA engine where it lies: no pass over
    // the batch on any host thread.  Anything else goes through the slot's page-locked staging buffer.
    const size_t row_bytes = CLAIR_INPUT_FLOATS * (q.counts ? sizeof(short) : sizeof(float));
    const size_t stride = q.stride ? (size_t)q.stride : row_bytes;
    const size_t span = (size_t)(n - 1) * stride + row_bytes;
    const float *own_input;
    { std::lock_guard<std::mutex> g(e->pinned_mu); own_input = s.h_x.as<float>(); }
    const bool direct = (q.input == (const void *)own_input && own_input && stride == row_bytes && !q.counts) || in_pinned(e, q.input, span);
    const bool on_device = !direct && is_device_pointer(q.input);   // e.g. the windows of clair_frontend_build_windows: no copy at all
    if (on_device && !q.counts) return fail(e, "a device pointer is taken for int16 counts only");
    enum { NONE, DENSE, STRIDED } convert = NONE;                    // the int16 -> float32 kernel the lane runs first
    const char *convert_from = nullptr;
    if (q.counts) {
        if (!on_device && ensure_slot_counts(e, s)) return 1;
        if (on_device) {
            convert = STRIDED; convert_from = (const char *)q.input;
        } else if (direct && stride != row_bytes) {   // records as they lie: ONE contiguous copy of the span, the conversion kernel skips what lies between the counts
            if (ensure_slot_records(e, s, span, stride)) return 1;
            HIP_TRY(e, hipMemcpyAsync(s.d_records.p, q.input, span, hipMemcpyHostToDevice, s.cin));
            convert = STRIDED; convert_from = s.d_records.as<char>();
        } else {
            const void *src = q.input;
            if (!direct) {
                if (ensure_slot_counts_staging(e, s)) return 1;
                gather_rows(s.h_counts.p, q.input, n, row_bytes, q.stride);
                src = s.h_counts.p;
            }
            HIP_TRY(e, hipMemcpyAsync(s.d_counts.p, src, (size_t)n * row_bytes, hipMemcpyHostToDevice, s.cin));
            convert = DENSE; convert_from = s.d_counts.as<char>();
        }
    } else if (direct && stride != row_bytes) {
        HIP_TRY(e, hipMemcpy2DAsync(s.d_x.p, row_bytes, q.input, stride, row_bytes, (size_t)n, hipMemcpyHostToDevice, s.cin));
    } else {
        const void *src = q.input;
        if (!direct) {
            if (ensure_slot_input(e, s)) return 1;
            gather_rows(s.h_x.p, q.input, n, row_bytes, q.stride);
            src = s.h_x.p;
        }
        HIP_TRY(e, hipMemcpyAsync(s.d_x.p, src, (size_t)n * row_bytes, hipMemcpyHostToDevice, s.cin));
    }
    if (n_pad > n)
        HIP_TRY(e, hipMemsetAsync(s.d_x.as<float>() + (size_t)n * CLAIR_INPUT_FLOATS, 0, (size_t)(n_pad - n) * CLAIR_INPUT_FLOATS * sizeof(float), s.cin));
    if (q.calls) {
        if (ensure_slot_decode(e, s)) return 1;
        memcpy(s.h_centre.p, q.centre, (size_t)n * 2);
        HIP_TRY(e, hipMemcpyAsync(s.d_centre.p, s.h_centre.p, (size_t)n * 2, hipMemcpyHostToDevice, s.cin));
    }
    if (q.models && !q.sites && ensure_slot_ensemble(e, s)) return 1;
    if (q.sites) {
        if (ensure_slot_decode(e, s) || ensure_slot_sites(e, s)) return 1;
        memcpy(s.h_centre.p, q.centre, (size_t)n * 2);
        memcpy(s.h_seq.p, q.seq, (size_t)n * SITE_SEQ);
        HIP_TRY(e, hipMemcpyAsync(s.d_centre.p, s.h_centre.p, (size_t)n * 2, hipMemcpyHostToDevice, s.cin));
        HIP_TRY(e, hipMemcpyAsync(s.d_seq.p, s.h_seq.p, (size_t)n * SITE_SEQ, hipMemcpyHostToDevice, s.cin));
    }
    if (q.labels) {
        if (ensure_slot_labels(e, s)) return 1;
        memcpy(s.h_labels.p, q.labels, (size_t)n * 4);
        HIP_TRY(e, hipMemcpyAsync(s.d_labels.p, s.h_labels.p, (size_t)n * 4, hipMemcpyHostToDevice, s.cin));
    }
    // int16 counts -> the float32 tensor.  On the LANE, in front of LSTM1 (default): a kernel of 1 056 small workgroups on the incoming stream has to
    // find CUs of its own among lanes whose recurrent workgroups hold whole CUs (one wave per SIMD, every register), and now and then it waits for
    // them long enough to leave a lane without input -- 5.3-5.5 instead of 7.2-7.6 M candidates/s in one run out of four (profiles/r04_convert_stream.txt);
    // on the lane it costs its own ~4 us per pass and nothing else.  CLAIR_AMD_CONVERT=copy puts it back behind the copy.
    auto launch_convert = [&](hipStream_t st) {
        const int n_quads = n * (CLAIR_INPUT_FLOATS / 4);
        if (convert == DENSE)
            hipLaunchKernelGGL(counts_to_input_kernel, dim3((n_quads + 255) / 256), dim3(256), 0, st, (const short4 *)convert_from, s.d_x.as<f32x4>(), n_quads);
        else if (convert == STRIDED)
            hipLaunchKernelGGL(counts_to_input_strided_kernel, dim3((n_quads + 255) / 256), dim3(256), 0, st, convert_from, stride, s.d_x.as<f32x4>(), n_quads);
    };
    const bool convert_on_lane = e->convert_on_lane && !same_in;
    if (!convert_on_lane) launch_convert(s.cin);
    if (!same_in) HIP_TRY(e, hipEventRecord(s.ev_in, s.cin));
    {
        std::unique_lock<std::mutex> g(l.order, std::defer_lock);
        if (!same_in) g.lock();
        if (!same_in) HIP_TRY(e, hipStreamWaitEvent(l.stream, s.ev_in, 0));
        if (convert_on_lane) launch_convert(l.stream);
        if (q.sites) {    // K passes over the same input back to back, each folded into the table's rows; the first brings the new rows their windows
            for (int k = 0; k < q.models; ++k) {
                if (enqueue_forward(e, l, *e->models[k], s.d_x.as<float>(), s.d_out.as<float>(), n, slot_index)) return 1;
                if (k == 0 && enqueue_sites_adopt(e, l, s, q.sites, q.sites_first, n, true)) return 1;
                if (enqueue_sites_accumulate(e, l, s, q.sites, q.sites_first, n)) return 1;
            }
        } else if (q.models) {   // K passes over the same input back to back, each folded into the slot's sums; the last leaves the averaged rows in d_out
            for (int k = 0; k < q.models; ++k) {
                if (enqueue_forward(e, l, *e->models[k], s.d_x.as<float>(), s.d_out.as<float>(), n, slot_index)) return 1;
                if (enqueue_ensemble(e, l, s, n, q.models, k == 0, k == q.models - 1)) return 1;
            }
        } else if (enqueue_forward(e, l, *e->models[0], s.d_x.as<float>(), s.d_out.as<float>(), n, slot_index)) return 1;
        if (q.calls && enqueue_decode(e, l, s, n)) return 1;
        if (q.labels && enqueue_eval(e, l, s, n)) return 1;
        if (same_out) return enqueue_results(e, l, s, n, q.calls != nullptr, want_probs);      // in line with the kernels, under the lane's lock
        HIP_TRY(e, hipEventRecord(s.ev_done, l.stream));
    }
    HIP_TRY(e, hipStreamWaitEvent(s.cout, s.ev_done, 0));
    return enqueue_results(e, l, s, n, q.calls != nullptr, want_probs);
}

void staging_worker(clair_engine *e) {
    (void)hipSetDevice(e->device);
    for (;;) {
        std::pair<int, clair_engine::Request> job;
        {
            std::unique_lock<std::mutex> g(e->wmu);
            e->wcv.wait(g, [&] { return e->wstop || !e->wqueue.empty(); });
            if (e->wqueue.empty()) return;            // stop asked for and nothing left to do
            job = e->wqueue.front();
            e->wqueue.pop_front();
        }
        g_error_sink = &e->slots[job.first].worker_error;   // `error` belongs to the caller's threads
        const int rc = enqueue_request(e, job.first, job.second);
        g_error_sink = nullptr;
        {
            std::lock_guard<std::mutex> g(e->wmu);
            e->slots[job.first].staged = rc ? 3 : 2;
        }
        e->wdone.notify_all();
    }
}

// Validates a request on the caller's thread, then hands it to the staging worker when the caller's memory has to be copied first
// (the worker does the copy AND the enqueue) or enqueues it right here.
int submit_request(clair_engine *e, int slot, const clair_engine::Request &q) {
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    if (s.pending_n) return fail(e, "slot %d still has a pending submit; call clair_wait first", slot);
    s.o_gt21 = q.gt21; s.o_gt = q.gt; s.o_l1 = q.l1; s.o_l2 = q.l2;
    s.o_calls = q.calls;
    s.refetch = false;
    if (!e->workers.empty()) {
        {
            std::lock_guard<std::mutex> g(e->wmu);
            s.staged = 1;
            e->wqueue.emplace_back(slot, q);
        }
        e->wcv.notify_one();
    } else {
        s.staged = 0;
        if (enqueue_request(e, slot, q)) return 1;
    }
    s.pending_n = q.n;
    return 0;
}

// the staging worker has nothing queued and every stream of the handle is idle
int quiesce(clair_engine *e) {
    {
        std::unique_lock<std::mutex> g(e->wmu);
        e->wdone.wait(g, [&] { for (auto &s : e->slots) if (s.staged == 1) return false; return true; });
    }
    for (auto st : e->copy_streams) HIP_TRY(e, hipStreamSynchronize(st));
    for (auto &lp : e->lanes) HIP_TRY(e, hipStreamSynchronize(lp->stream));
    return 0;
}

int check_slot(clair_engine *e, int slot, bool need_weights = true) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (slot < 0 || slot >= (int)e->slots.size()) return fail(e, "slot %d out of range [0,%d)", slot, (int)e->slots.size());
    if (need_weights && !e->models[0]->ready) return fail(e, "weights not loaded: call clair_set_tensor for all tensors, then clair_finalize_weights");
    return 0;
}

int check_n(clair_engine *e, int n) {
    if (n < 1 || n > e->max_batch) return fail(e, "n=%d out of range [1,%d]", n, e->max_batch);
    return 0;
}

// What the four submit entry points ask of a request, in the order they have always asked it: the slot, the weights, n, then
// `pointers_ok` with the entry point's own message (which pointers it insists on is its own business), the probability arrays (all four
// or none) and the stride.
int check_request(clair_engine *e, int slot, const clair_engine::Request &q, bool pointers_ok, const char *pointers_message) {
    if (check_slot(e, slot) || check_n(e, q.n)) return 1;
    if (!pointers_ok) return fail(e, "%s", pointers_message);
    if ((q.gt21 || q.gt || q.l1 || q.l2) && !(q.gt21 && q.gt && q.l1 && q.l2)) return fail(e, "the four probability arrays come together or not at all");
    return 0;
}
int check_stride(clair_engine *e, const clair_engine::Request &q) {
    if (q.stride != 0 && q.stride < (int64_t)(CLAIR_INPUT_FLOATS * (q.counts ? sizeof(short) : sizeof(float))))
        return fail(e, "input stride of %lld bytes is shorter than one candidate", (long long)q.stride);
    return 0;
}

// clair_set_tensor / clair_finalize_weights for weight image `model` (0: the handle's own checkpoint)
int set_model_tensor(clair_engine *e, int model, int id, const float *host, int64_t count) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (model < 0 || model >= (int)e->models.size()) return fail(e, "model %d out of range [0,%d): call clair_ensemble_models first", model, (int)e->models.size());
    if (id < 0 || id >= CLAIR_T_COUNT) return fail(e, "tensor id %d out of range", id);
    if (!host) return fail(e, "tensor %d: host pointer is NULL", id);
    if (count != TENSOR_COUNT[id]) return fail(e, "tensor %d: got %lld floats, expected %lld", id, (long long)count, (long long)TENSOR_COUNT[id]);
    ModelWeights &w = *e->models[model];
    w.host_tensors[id].assign(host, host + count);
    w.ready = false;
    return 0;
}

int finalize_model(clair_engine *e, int model) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (model < 0 || model >= (int)e->models.size()) return fail(e, "model %d out of range [0,%d): call clair_ensemble_models first", model, (int)e->models.size());
    ModelWeights &w = *e->models[model];
    for (int i = 0; i < CLAIR_T_COUNT; ++i)
        if ((int64_t)w.host_tensors[i].size() != TENSOR_COUNT[i]) return fail(e, "tensor %d has not been set", i);
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    const WeightImages m = build_weight_images(LAYER_SIZES, w.host_tensors);
    if (upload(e, w.bx1, m.bx1) || upload(e, w.bx2, m.bx2) || upload(e, w.wx2s, m.wx2s) || upload(e, w.wh1s, m.wh1s) || upload(e, w.wh2s, m.wh2s) ||
        upload(e, w.wx1s, m.wx1s) || upload(e, w.w3s, m.w3s) || upload(e, w.w4s, m.w4s) || upload(e, w.b4, m.b4) || upload(e, w.w5s, m.w5s) ||
        upload(e, w.whs, m.whs) || upload(e, w.b5, m.b5) || upload(e, w.bh, m.bh)) return 1;
    w.w3_shift = m.w3_shift;
    w.w4_shift = m.w4_shift;
    for (int k = 0; k < 4; ++k) { w.w5_shift[k] = m.w5_shift[k]; w.wh_shift[k] = m.wh_shift[k]; }
    w.ready = true;
    return 0;
}

// The packed [n][90] rows the kernels exchange, from and to the four arrays callers hold: 21 | 3 | 33 | 33 floats (HEAD_SIZE).
static_assert(HEAD_SIZE[0] + HEAD_SIZE[1] + HEAD_SIZE[2] + HEAD_SIZE[3] == OUT_FLOATS, "the four heads fill a packed row");
void pack_rows(float *rows, const float *const (&heads)[4], int n) {
    for (int i = 0; i < n; ++i) {
        float *row = rows + (size_t)i * OUT_FLOATS;
        for (int k = 0; k < 4; row += HEAD_SIZE[k], ++k) memcpy(row, heads[k] + (size_t)i * HEAD_SIZE[k], HEAD_SIZE[k] * sizeof(float));
    }
}
void unpack_rows(const float *rows, float *const (&heads)[4], int n) {
    for (int i = 0; i < n; ++i) {
        const float *row = rows + (size_t)i * OUT_FLOATS;
        for (int k = 0; k < 4; row += HEAD_SIZE[k], ++k) memcpy(heads[k] + (size_t)i * HEAD_SIZE[k], row, HEAD_SIZE[k] * sizeof(float));
    }
}

}  // namespace

extern "C" {

int clair_abi_version(void) { return CLAIR_ABI_VERSION; }

int clair_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int clair_device_pci_bus_id(int device, char *buf, int len) {
    if (!buf || len < 16) return fail(nullptr, "clair_device_pci_bus_id: buffer of at least 16 bytes needed");
    buf[0] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return fail(nullptr, "clair_device_pci_bus_id: no HIP device %d (%d visible)", device, n);
    if (hipDeviceGetPCIBusId(buf, len, device) != hipSuccess) { buf[0] = 0; return fail(nullptr, "hipDeviceGetPCIBusId(%d) failed", device); }
    for (char *c = buf; *c; ++c) *c = (char)tolower((unsigned char)*c);      // sysfs spells the hexadecimal digits in lower case
    return 0;
}

const char *clair_last_error(const clair_engine_t *e) { return e ? e->error.c_str() : g_create_error.c_str(); }

int clair_engine_create(int device, int max_batch, int n_slots, clair_engine_t **out) {
    if (!out) return fail(nullptr, "out is NULL");
    *out = nullptr;
    if (max_batch < 1 || max_batch > (1 << 20)) return fail(nullptr, "max_batch %d out of range [1, 2^20]", max_batch);
    if (n_slots < 1 || n_slots > 64) return fail(nullptr, "n_slots %d out of range [1,64]", n_slots);
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev <= 0)
        return fail(nullptr, "no HIP device available (hipGetDeviceCount: %s); the MI355X engine has no CPU fallback",
                    hipGetErrorString(err));
    if (device < 0 || device >= ndev) return fail(nullptr, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(nullptr, hipSetDevice(device));
    clair_engine *e = new clair_engine();
    e->device = device;
    e->max_batch = max_batch;
    e->max_pad = (max_batch + 31) & ~31;
    { const char *t = getenv("CLAIR_AMD_TAP_L3"); e->tap_l3 = t && t[0] == '1'; }
    { const char *t = getenv("CLAIR_AMD_L34_STAMPS"); e->l34_stamps = !e->tap_l3 && t && t[0] == '1'; }
    // A handle with one slot runs its kernels alone: the projection GEMM takes every CU (8 XCDs x 4 gate tiles x 8 groups).  With
    // batches in flight on several slots the 64-workgroup recurrent kernels of the other slots hold whole CUs for ~80 us; a
    // 256-workgroup persistent GEMM then runs its last 64 workgroups as a second round on a quarter of the chip.  Four groups (128
    // workgroups) pack beside two recurrent kernels: +4 % whole-pipeline throughput at 3 slots (profiles/r01_microbench.txt).
    // Lanes.  The runtime gives a process four hardware queues: FOUR forward passes in flight when nothing else needs one (a handle of up to four
    // slots: clair_run_resident, clair_predict -- 8.05 against 7.89 M candidates/s with three, profiles/r04_lanes_sweep.txt; a fifth stream shares a
    // queue with one of the four and sets the whole pipeline back, 6.5 M/s); THREE plus the incoming copy stream for a handle with more slots than
    // that, i.e. one that is fed from the host with batches in flight on the link (four lanes there: 6.2 against 7.3 M/s).
    int n_lanes = n_slots <= 4 ? n_slots : 3;
    { const char *t = getenv("CLAIR_AMD_LANES"); if (t && atoi(t) > 0) n_lanes = std::min(atoi(t), n_slots); }
    e->proj2_groups = n_lanes >= 4 ? 3 : (n_lanes > 1 ? 4 : 8);       // four lanes: 96 workgroups (8.00 against 7.91 M/s with 128, profiles/r04_lanes_sweep.txt)
    { const char *t = getenv("CLAIR_AMD_PROJ2_GROUPS"); if (t && atoi(t) > 0) e->proj2_groups = atoi(t); }
    { const char *t = getenv("CLAIR_AMD_LSTM2_FUSED"); if (t && (t[0] == '0' || t[0] == '1')) e->lstm2_fused = t[0] - '0'; }
    { const char *t = getenv("CLAIR_AMD_FUSED_GROUPS"); if (t && atoi(t) > 0 && atoi(t) <= 8) e->fused_groups = atoi(t); }
    { const char *t = getenv("CLAIR_AMD_LSTM2_PAIR"); if (t && (t[0] == '0' || t[0] == '1')) e->lstm2_pair = t[0] - '0'; }
    { const char *t = getenv("CLAIR_AMD_FUSED_FAULT"); if (t && atoll(t) > 0) e->fused_fault_at = atoll(t); }
    { const char *t = getenv("CLAIR_AMD_STAGING_THREADS"); if (t && atoi(t) >= 0 && atoi(t) <= 16) e->staging_threads = atoi(t); }
    { const char *t = getenv("CLAIR_AMD_ASYNC_STAGING"); if (t && t[0] == '0') e->staging_threads = 0; }
    { const char *t = getenv("CLAIR_AMD_COPY_STREAMS"); if (t) e->copy_mode = !strcmp(t, "slot") ? 0 : !strcmp(t, "two") ? 1 : !strcmp(t, "lane") ? 2 : 3; }
    { const char *t = getenv("CLAIR_AMD_D2H"); if (t) e->d2h_kernel = !strcmp(t, "kernel"); }
    { const char *t = getenv("CLAIR_AMD_CONVERT"); if (t) e->convert_on_lane = strcmp(t, "copy") != 0; }
    e->models.emplace_back(new ModelWeights());
    for (int i = 0; i < n_lanes; ++i) e->lanes.emplace_back(new Lane());
    e->slots = std::vector<Slot>(n_slots);   // (a Slot owns its buffers and does not move)
    const size_t mp = e->max_pad;
    hipError_t r = hipSuccess;
    for (auto &lp : e->lanes) {
        Lane &l = *lp;
        if (r == hipSuccess) r = hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking);
        if (r == hipSuccess) r = l.zx.ensure((size_t)T_POS * mp * 1024 * sizeof(float));
        if (r == hipSuccess) r = l.a1.ensure(((size_t)2 * T_POS * mp * 256 + 128 * 256) * sizeof(unsigned short));   // + slack rows read (never used) by gemm_split's ragged last tile
        if (r == hipSuccess) r = l.a2.ensure((size_t)T_POS * mp * 256 * sizeof(float));
        if (r == hipSuccess) r = l.l4part.ensure((size_t)L4_SPLITS * ((mp + L34_CAND - 1) / L34_CAND * L34_CAND) * L4_UNITS * sizeof(float));
        if (r == hipSuccess && fused_possible(e)) {
            const size_t words = fuse_words(e->max_pad) + 1 + fuse_claims(e);   // tickets | error word | claims
            r = l.fuse_flags.ensure(words * sizeof(unsigned));
            if (r == hipSuccess) r = hipMemset(l.fuse_flags.p, 0, words * sizeof(unsigned));
        }
    }
    for (size_t i = 0; i < e->slots.size(); ++i) {
        Slot &s = e->slots[i];
        s.lane = (int)(i % e->lanes.size());
        if (e->copy_mode == 0) {            // a stream per slot for both directions
            hipStream_t st = nullptr;
            if (r == hipSuccess) r = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (r == hipSuccess) e->copy_streams.push_back(st);
            s.cin = s.cout = st;
        } else if (e->copy_mode == 1) {     // one stream for everything that comes in, one for everything that goes out
            while (r == hipSuccess && e->copy_streams.size() < 2) {
                hipStream_t st = nullptr;
                r = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
                if (r == hipSuccess) e->copy_streams.push_back(st);
            }
            if (r == hipSuccess) { s.cin = e->copy_streams[0]; s.cout = e->copy_streams[1]; }
        } else if (e->copy_mode == 2) {     // on the lane's own stream, in line with its kernels
            s.cin = s.cout = e->lanes[s.lane]->stream;
        } else {                            // ONE stream for everything that comes in; the results leave on the lane's own stream
            if (r == hipSuccess && e->copy_streams.empty()) {
                hipStream_t st = nullptr;
                r = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
                if (r == hipSuccess) e->copy_streams.push_back(st);
            }
            if (r == hipSuccess) { s.cin = e->copy_streams[0]; s.cout = e->lanes[s.lane]->stream; }
        }
        if (r == hipSuccess) r = hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming);
        if (r == hipSuccess) r = s.d_x.ensure(mp * CLAIR_INPUT_FLOATS * sizeof(float));
        if (r == hipSuccess) r = hipMemset(s.d_x.p, 0, mp * CLAIR_INPUT_FLOATS * sizeof(float));
        if (r == hipSuccess) r = s.d_out.ensure(mp * OUT_FLOATS * sizeof(float));
        if (r == hipSuccess) r = s.h_out.ensure(h_out_floats(max_batch) * sizeof(float));   // + the fused launch's error word
    }
    if (r != hipSuccess) {
        fail(nullptr, "allocating workspaces for max_batch=%d, %d slot(s) failed: %s", max_batch, n_slots, hipGetErrorString(r));
        clair_engine_destroy(e);
        return 1;
    }
    for (int i = 0; i < e->staging_threads; ++i) e->workers.emplace_back(staging_worker, e);
    *out = e;
    return 0;
}

void clair_engine_destroy(clair_engine_t *e) {
    if (!e) return;
    if (!e->workers.empty()) {
        { std::lock_guard<std::mutex> g(e->wmu); e->wstop = true; }
        e->wcv.notify_all();
        for (auto &t : e->workers) t.join();
    }
    (void)hipSetDevice(e->device);
    for (auto &lp : e->lanes) if (lp->stream) (void)hipStreamSynchronize(lp->stream);
    for (auto st : e->copy_streams) (void)hipStreamSynchronize(st);
    std::vector<hipStream_t> streams = e->copy_streams;
    for (auto &s : e->slots) {
        if (s.ev_out) (void)hipEventSynchronize(s.ev_out);
        for (hipEvent_t ev : {s.ev_in, s.ev_done, s.ev_out}) if (ev) (void)hipEventDestroy(ev);
    }
    for (auto &lp : e->lanes) {
        if (!lp->stream) continue;
        for (auto &t : lp->timed) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
        for (auto ev : lp->free_events) (void)hipEventDestroy(ev);
        streams.push_back(lp->stream);
    }
    delete e;                                            // every buffer goes with its owner
    for (auto st : streams) (void)hipStreamDestroy(st);
}

int clair_set_tensor(clair_engine_t *e, int id, const float *host, int64_t count) { return set_model_tensor(e, 0, id, host, count); }

int clair_finalize_weights(clair_engine_t *e) { return finalize_model(e, 0); }

int clair_submit(clair_engine_t *e, int slot, const float *x, int n, float *gt21, float *genotype, float *l1, float *l2) {
    const clair_engine::Request q{x, false, 0, n, nullptr, nullptr, gt21, genotype, l1, l2};
    if (check_request(e, slot, q, x && gt21 && genotype && l1 && l2, "NULL input/output pointer")) return 1;
    return submit_request(e, slot, q);
}

int clair_submit_counts(clair_engine_t *e, int slot, const int16_t *counts, int n, float *gt21, float *genotype, float *l1, float *l2) {
    const clair_engine::Request q{counts, true, 0, n, nullptr, nullptr, gt21, genotype, l1, l2};
    if (check_request(e, slot, q, counts && gt21 && genotype && l1 && l2, "NULL input/output pointer")) return 1;
    return submit_request(e, slot, q);
}

int clair_slot_input(clair_engine_t *e, int slot, float **x_pinned) {
    if (check_slot(e, slot)) return 1;
    if (!x_pinned) return fail(e, "x_pinned is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    if (ensure_slot_input(e, s)) return 1;
    *x_pinned = s.h_x.as<float>();
    return 0;
}

int clair_wait(clair_engine_t *e, int slot) {
    if (check_slot(e, slot, false)) return 1;      // what a submit needs it has checked itself; clair_submit_site_calls needs no weights
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    Lane &l = *e->lanes[s.lane];
    const int n = s.pending_n;
    if (s.staged) {     // handed to the staging worker: it has enqueued the batch by the time this returns
        std::unique_lock<std::mutex> g(e->wmu);
        e->wdone.wait(g, [&] { return s.staged != 1; });
        const bool failed = s.staged == 3;
        s.staged = 0;
        if (failed) {
            g.unlock();
            (void)hipStreamSynchronize(s.cout);
            s.pending_n = 0; s.o_calls = nullptr;
            e->error = s.worker_error;
            return 1;
        }
    }
    if (n) HIP_TRY(e, hipEventSynchronize(s.ev_out));
    bool again = s.refetch;
    s.refetch = false;
    if (l.fuse_flags.p) {
        std::lock_guard<std::mutex> g(l.order);
        unsigned bad;
        memcpy(&bad, s.h_out.as<float>() + h_word_offset(e->max_batch), sizeof bad);
        bool mine = false;
        for (const auto &r : l.fused_runs) mine = mine || r.slot == slot;
        if (n && bad && mine) {   // re-run on the two-launch path (d_x still holds the input), fetch the outputs again
            if (recover_fused(e, l, slot)) { s.pending_n = 0; return 1; }
            again = true;
        }
        l.fused_runs.erase(std::remove_if(l.fused_runs.begin(), l.fused_runs.end(), [slot](const Lane::FusedRun &r) { return r.slot == slot; }), l.fused_runs.end());
    }
    if (n && again) {
        std::lock_guard<std::mutex> g(l.order);
        if (s.o_calls) {
            if (enqueue_decode(e, l, s, n)) { s.pending_n = 0; return 1; }
            HIP_TRY(e, hipMemcpyAsync(s.h_calls.p, s.d_calls.p, (size_t)n * sizeof(clair_call_t), hipMemcpyDeviceToHost, l.stream));
        }
        if (s.o_gt21) HIP_TRY(e, hipMemcpyAsync(s.h_out.p, s.d_out.p, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyDeviceToHost, l.stream));
        HIP_TRY(e, hipStreamSynchronize(l.stream));
    }
    if (s.o_gt21) unpack_rows(s.h_out.as<float>(), {s.o_gt21, s.o_gt, s.o_l1, s.o_l2}, n);
    if (s.o_calls) memcpy(s.o_calls, s.h_calls.p, (size_t)n * sizeof(clair_call_t));
    s.o_calls = nullptr;
    s.pending_n = 0;
    return 0;
}

// The pipelined call with the decode on the device: input as float32 tensor (input_is_counts == 0) or raw int16 counts; calls != NULL
// asks for the call records (centre: [n][2] bytes, required then); the four probability arrays are optional then (all or none).
int clair_submit_ex(clair_engine_t *e, int slot, const void *input, int input_is_counts, int64_t input_stride_bytes, int n, const uint8_t *centre,
                    clair_call_t *calls, float *gt21, float *genotype, float *l1, float *l2) {
    const clair_engine::Request q{input, input_is_counts != 0, input_stride_bytes, n, centre, calls, gt21, genotype, l1, l2};
    if (check_request(e, slot, q, input != nullptr, "NULL input pointer")) return 1;
    if (!(gt21 || genotype || l1 || l2) && !calls) return fail(e, "nothing asked for: neither call records nor probabilities");
    if (calls && !centre) return fail(e, "call records need the candidates' centre bytes");
    if (check_stride(e, q)) return 1;
    return submit_request(e, slot, q);
}

// The decode alone, on probabilities the caller already has (call_var's --input_probabilities path, clair/call_var.py:1276-1309): synchronous.
int clair_decode(clair_engine_t *e, int slot, const float *x, const float *gt21, const float *genotype, const float *l1, const float *l2, int n,
                 const uint8_t *centre, clair_call_t *calls) {
    if (check_slot(e, slot, false) || check_n(e, n)) return 1;
    if (!x || !gt21 || !genotype || !l1 || !l2 || !centre || !calls) return fail(e, "NULL input/output pointer");
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    if (s.pending_n) return fail(e, "slot %d still has a pending submit; call clair_wait first", slot);
    if (ensure_slot_decode(e, s)) return 1;
    pack_rows(s.h_out.as<float>(), {gt21, genotype, l1, l2}, n);
    memcpy(s.h_centre.p, centre, (size_t)n * 2);
    Lane &l = *e->lanes[s.lane];
    std::lock_guard<std::mutex> g(l.order);
    HIP_TRY(e, hipMemcpyAsync(s.d_x.p, x, (size_t)n * CLAIR_INPUT_FLOATS * sizeof(float), hipMemcpyHostToDevice, l.stream));
    HIP_TRY(e, hipMemcpyAsync(s.d_out.p, s.h_out.p, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyHostToDevice, l.stream));
    HIP_TRY(e, hipMemcpyAsync(s.d_centre.p, s.h_centre.p, (size_t)n * 2, hipMemcpyHostToDevice, l.stream));
    if (enqueue_decode(e, l, s, n)) return 1;
    HIP_TRY(e, hipMemcpyAsync(s.h_calls.p, s.d_calls.p, (size_t)n * sizeof(clair_call_t), hipMemcpyDeviceToHost, l.stream));
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    memcpy(calls, s.h_calls.p, (size_t)n * sizeof(clair_call_t));
    return 0;
}

// -- scoring against truth labels on the device (evaluate.hip.h; clair/evaluate.py:87-129) --------------------------------------
int clair_eval_reset(clair_engine_t *e) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    if (ensure_eval_counts(e)) return 1;
    HIP_TRY(e, hipMemset(e->eval_counts.p, 0, (size_t)CLAIR_EVAL_COUNTS * sizeof(unsigned long long)));
    HIP_TRY(e, hipStreamSynchronize(nullptr));
    return 0;
}

int clair_submit_eval(clair_engine_t *e, int slot, const void *input, int input_is_counts, int64_t input_stride_bytes, int n, const uint8_t *labels,
                      float *gt21, float *genotype, float *l1, float *l2) {
    clair_engine::Request q{input, input_is_counts != 0, input_stride_bytes, n, nullptr, nullptr, gt21, genotype, l1, l2};
    q.labels = labels;
    if (check_request(e, slot, q, input && labels, "NULL input or label pointer") || check_stride(e, q)) return 1;
    // a fused layer-2 launch (opt-in) may be re-run after the fact (recover_fused), which would count its batch twice
    if (fused_possible(e)) return fail(e, "clair_submit_eval runs on the two-launch layer-2 path only: unset CLAIR_AMD_LSTM2_FUSED");
    if (check_labels(e, labels, n)) return 1;
    HIP_TRY(e, hipSetDevice(e->device));
    if (ensure_eval_counts(e)) return 1;
    return submit_request(e, slot, q);
}

// The scoring alone, on probabilities the caller holds: synchronous, needs no weights (the twin of clair_decode).
int clair_eval(clair_engine_t *e, int slot, const float *gt21, const float *genotype, const float *l1, const float *l2, const uint8_t *labels, int n) {
    if (check_slot(e, slot, false) || check_n(e, n)) return 1;
    if (!gt21 || !genotype || !l1 || !l2 || !labels) return fail(e, "NULL input pointer");
    if (check_labels(e, labels, n)) return 1;
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    if (s.pending_n) return fail(e, "slot %d still has a pending submit; call clair_wait first", slot);
    if (ensure_eval_counts(e) || ensure_slot_labels(e, s)) return 1;
    pack_rows(s.h_out.as<float>(), {gt21, genotype, l1, l2}, n);
    memcpy(s.h_labels.p, labels, (size_t)n * 4);
    Lane &l = *e->lanes[s.lane];
    std::lock_guard<std::mutex> g(l.order);
    HIP_TRY(e, hipMemcpyAsync(s.d_out.p, s.h_out.p, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyHostToDevice, l.stream));
    HIP_TRY(e, hipMemcpyAsync(s.d_labels.p, s.h_labels.p, (size_t)n * 4, hipMemcpyHostToDevice, l.stream));
    if (enqueue_eval(e, l, s, n)) return 1;
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    return 0;
}

int clair_eval_read(clair_engine_t *e, int64_t *counts) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (!counts) return fail(e, "counts is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    if (ensure_eval_counts(e)) return 1;
    HIP_TRY(e, hipMemcpy(counts, e->eval_counts.p, (size_t)CLAIR_EVAL_COUNTS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

// -- ensemble calling: K checkpoints over one batch, averaged on the device (ensemble.hip.h; clair/post_processing/ensemble.py:10-75) ----
int clair_ensemble_models(clair_engine_t *e, int models) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (models < 1 || models > CLAIR_ENSEMBLE_MAX_MODELS) return fail(e, "clair_ensemble_models: %d models, 1 .. %d", models, CLAIR_ENSEMBLE_MAX_MODELS);
    if (fused_possible(e)) return fail(e, "ensemble calling runs on the two-launch layer-2 path only: unset CLAIR_AMD_LSTM2_FUSED");
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;           // nothing in flight reads an image that goes away
    while ((int)e->models.size() > models) e->models.pop_back();
    while ((int)e->models.size() < models) e->models.emplace_back(new ModelWeights());
    return 0;
}

int clair_ensemble_set_tensor(clair_engine_t *e, int model, int tensor_id, const float *host, int64_t count) { return set_model_tensor(e, model, tensor_id, host, count); }

int clair_ensemble_finalize_weights(clair_engine_t *e, int model) { return finalize_model(e, model); }

int clair_submit_ensemble(clair_engine_t *e, int slot, const void *input, int input_is_counts, int64_t input_stride_bytes, int n, const uint8_t *centre,
                          clair_call_t *calls, float *gt21, float *genotype, float *l1, float *l2) {
    clair_engine::Request q{input, input_is_counts != 0, input_stride_bytes, n, centre, calls, gt21, genotype, l1, l2};
    if (check_request(e, slot, q, input != nullptr, "NULL input pointer")) return 1;
    if (!(gt21 || genotype || l1 || l2) && !calls) return fail(e, "nothing asked for: neither call records nor probabilities");
    if (calls && !centre) return fail(e, "call records need the candidates' centre bytes");
    if (check_stride(e, q)) return 1;
    // a fused layer-2 launch (opt-in) may be re-run after the fact (recover_fused), and a re-run knows one weight image
    if (fused_possible(e)) return fail(e, "clair_submit_ensemble runs on the two-launch layer-2 path only: unset CLAIR_AMD_LSTM2_FUSED");
    q.models = (int)e->models.size();
    for (int k = 0; k < q.models; ++k)
        if (!e->models[k]->ready) return fail(e, "weights of model %d not loaded: clair_ensemble_set_tensor for all tensors, then clair_ensemble_finalize_weights", k);
    return submit_request(e, slot, q);
}

// The averaging alone, on probabilities the caller holds: synchronous, needs no weights (the twin of clair_decode and clair_eval).
int clair_ensemble_average(clair_engine_t *e, int slot, const float *probs, int models, int n, float *out) {
    if (check_slot(e, slot, false) || check_n(e, n)) return 1;
    if (models < 1 || models > CLAIR_ENSEMBLE_MAX_MODELS) return fail(e, "clair_ensemble_average: %d models, 1 .. %d", models, CLAIR_ENSEMBLE_MAX_MODELS);
    if (!probs || !out) return fail(e, "NULL input/output pointer");
    if (fused_possible(e)) return fail(e, "clair_ensemble_average is not available on a handle with the fused layer-2 launch: unset CLAIR_AMD_LSTM2_FUSED");
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    if (s.pending_n) return fail(e, "slot %d still has a pending submit; call clair_wait first", slot);
    if (ensure_slot_ensemble(e, s)) return 1;
    const size_t row_bytes = (size_t)n * OUT_FLOATS * sizeof(float);
    Lane &l = *e->lanes[s.lane];
    std::lock_guard<std::mutex> g(l.order);
    for (int k = 0; k < models; ++k) {
        HIP_TRY(e, hipMemcpyAsync(s.d_out.p, (const char *)probs + (size_t)k * row_bytes, row_bytes, hipMemcpyHostToDevice, l.stream));
        if (enqueue_ensemble(e, l, s, n, models, k == 0, k == models - 1)) return 1;
    }
    HIP_TRY(e, hipMemcpyAsync(out, s.d_out.p, row_bytes, hipMemcpyDeviceToHost, l.stream));
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    return 0;
}

// -- ensemble across BAMs: the site table (sites.hip.h; clair/post_processing/ensemble.py:10-75 over runs whose sites differ) ----------------
namespace {

// a buffer grown to new_bytes with its first old_bytes kept
int grow_buffer(clair_engine *e, DeviceBuffer &b, size_t old_bytes, size_t new_bytes) {
    DeviceBuffer fresh;
    HIP_TRY(e, fresh.ensure(new_bytes));
    if (old_bytes) HIP_TRY(e, hipMemcpy(fresh.p, b.p, old_bytes, hipMemcpyDeviceToDevice));
    std::swap(b.p, fresh.p);
    std::swap(b.bytes, fresh.bytes);
    return 0;
}

int check_sites(clair_sites *t, const char *what, bool open_only) {
    if (!t) return fail(nullptr, "%s: the site table is NULL", what);
    if (open_only && t->finished) return fail(t->e, "%s: the site table has been finished: it takes no more rows", what);
    return 0;
}

int check_source_range(clair_sites *t, const char *what, int64_t first, int64_t n) {
    if (t->src_n < 0) return fail(t->e, "%s: no source begun: call clair_sites_begin_source first", what);
    if (first < 0 || n < 1 || first > t->src_n - n) return fail(t->e, "%s: rows [%lld, %lld) lie outside the current source of %lld", what, (long long)first,
                                                                (long long)(first + n), (long long)t->src_n);
    return 0;
}

int check_output_range(clair_sites *t, const char *what, int64_t first, int64_t n) {
    if (!t->finished) return fail(t->e, "%s: call clair_sites_finish first", what);
    if (first < 0 || n < 0 || first > t->n_out - n) return fail(t->e, "%s: rows [%lld, %lld) lie outside the output list of %lld", what, (long long)first,
                                                                (long long)(first + n), (long long)t->n_out);
    return 0;
}

int read_overflow(clair_sites *t, const char *what) {
    int flag = 0;
    HIP_TRY(t->e, hipMemcpy(&flag, t->overflow.p, sizeof flag, hipMemcpyDeviceToHost));
    if (flag) return fail(t->e, "%s: a site was given more than %d rows", what, SITE_MAX_ROWS);
    return 0;
}

}  // namespace

int clair_sites_create(clair_engine_t *e, clair_sites_t **out) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (!out) return fail(e, "out is NULL");
    if (fused_possible(e)) return fail(e, "clair_sites_create: the site table runs on the two-launch layer-2 path only: unset CLAIR_AMD_LSTM2_FUSED");
    HIP_TRY(e, hipSetDevice(e->device));
    std::unique_ptr<clair_sites> t(new clair_sites());
    t->e = e;
    HIP_TRY(e, t->overflow.ensure(sizeof(int)));
    HIP_TRY(e, hipMemset(t->overflow.p, 0, sizeof(int)));
    HIP_TRY(e, hipStreamSynchronize(nullptr));
    *out = t.get();
    e->tables.push_back(std::move(t));
    return 0;
}

void clair_sites_destroy(clair_sites_t *t) {
    if (!t) return;
    clair_engine *e = t->e;
    (void)hipSetDevice(e->device);
    (void)quiesce(e);
    e->tables.remove_if([t](const std::unique_ptr<clair_sites> &p) { return p.get() == t; });
}

int clair_sites_begin_source(clair_sites_t *t, const int64_t *positions, int64_t n, int64_t *n_new) {
    if (check_sites(t, "clair_sites_begin_source", true)) return 1;
    clair_engine *e = t->e;
    if (n < 0 || n > INT32_MAX || (n > 0 && !positions)) return fail(e, "clair_sites_begin_source: bad arguments");
    for (int64_t i = 1; i < n; ++i)
        if (positions[i] <= positions[i - 1])
            return fail(e, "clair_sites_begin_source: positions are not strictly ascending (%lld after %lld at %lld)", (long long)positions[i], (long long)positions[i - 1], (long long)i);
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;                     // every slot drained: nothing in flight reads row_of or the rows that move
    Lane &l = *e->lanes[0];
    std::lock_guard<std::mutex> g(l.order);
    uint32_t fresh = 0;
    if (n > 0) {
        const int64_t ns = t->n_sites;
        HIP_TRY(e, t->pos.ensure((size_t)n * sizeof(int64_t)));
        HIP_TRY(e, t->lb.ensure((size_t)n * sizeof(int64_t)));
        HIP_TRY(e, t->row_of.ensure((size_t)n * sizeof(int64_t)));
        HIP_TRY(e, t->is_new.ensure((size_t)n * sizeof(uint32_t)));
        HIP_TRY(e, t->before.ensure((size_t)(n + 1) * sizeof(uint32_t)));
        HIP_TRY(e, hipMemcpyAsync(t->pos.p, positions, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, l.stream));
        hipLaunchKernelGGL(sites_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, l.stream, t->pos.as<int64_t>(), n, t->idx_key[t->cur].as<int64_t>(),
                           t->idx_row[t->cur].as<int64_t>(), ns, t->lb.as<int64_t>(), t->is_new.as<uint32_t>(), t->row_of.as<int64_t>());
        hipLaunchKernelGGL(sites_scan_kernel, dim3(1), dim3(256), 0, l.stream, t->is_new.as<uint32_t>(), n, t->before.as<uint32_t>());
        HIP_TRY(e, hipGetLastError());
        HIP_TRY(e, hipMemcpyAsync(&fresh, t->before.as<uint32_t>() + n, sizeof fresh, hipMemcpyDeviceToHost, l.stream));
        HIP_TRY(e, hipStreamSynchronize(l.stream));
        if (ns + fresh > t->capacity) {           // room for every position of the source, so that a source of known sites never grows anything
            const size_t from = (size_t)ns, to = (size_t)(ns + n);
            if (grow_buffer(e, t->key, from * sizeof(int64_t), to * sizeof(int64_t)) || grow_buffer(e, t->count, from * sizeof(int), to * sizeof(int)) ||
                grow_buffer(e, t->acc, from * OUT_FLOATS * sizeof(double), to * OUT_FLOATS * sizeof(double)) ||
                grow_buffer(e, t->x, from * SITE_X * sizeof(float), to * SITE_X * sizeof(float)) || grow_buffer(e, t->centre, from * 2, to * 2) ||
                grow_buffer(e, t->seq, from * SITE_SEQ, to * SITE_SEQ)) return 1;
            for (int k = 0; k < 2; ++k) {
                const size_t keep = k == t->cur ? from * sizeof(int64_t) : 0;
                if (grow_buffer(e, t->idx_key[k], keep, to * sizeof(int64_t)) || grow_buffer(e, t->idx_row[k], keep, to * sizeof(int64_t))) return 1;
            }
            t->capacity = (int64_t)to;
        }
        if (fresh) {
            const int other = t->cur ^ 1;
            hipLaunchKernelGGL(sites_assign_kernel, dim3((unsigned)((n + ns + 255) / 256)), dim3(256), 0, l.stream, t->pos.as<int64_t>(), n, t->lb.as<int64_t>(),
                               t->is_new.as<uint32_t>(), t->before.as<uint32_t>(), t->idx_key[t->cur].as<int64_t>(), t->idx_row[t->cur].as<int64_t>(), ns,
                               t->idx_key[other].as<int64_t>(), t->idx_row[other].as<int64_t>(), t->row_of.as<int64_t>(), t->key.as<int64_t>(), t->count.as<int>());
            HIP_TRY(e, hipGetLastError());
            HIP_TRY(e, hipMemsetAsync(t->acc.as<double>() + (size_t)ns * OUT_FLOATS, 0, (size_t)fresh * OUT_FLOATS * sizeof(double), l.stream));
            // window, centre and seq of a new row are zeros until a run brings its own (clair_sites_add_rows may bring none)
            HIP_TRY(e, hipMemsetAsync(t->x.as<float>() + (size_t)ns * SITE_X, 0, (size_t)fresh * SITE_X * sizeof(float), l.stream));
            HIP_TRY(e, hipMemsetAsync(t->centre.as<unsigned char>() + (size_t)ns * 2, 0, (size_t)fresh * 2, l.stream));
            HIP_TRY(e, hipMemsetAsync(t->seq.as<unsigned char>() + (size_t)ns * SITE_SEQ, 0, (size_t)fresh * SITE_SEQ, l.stream));
            HIP_TRY(e, hipStreamSynchronize(l.stream));
            t->cur = other;
            t->n_sites = ns + fresh;
        }
    }
    t->src_n = n;
    if (n_new) *n_new = fresh;
    return 0;
}

int clair_submit_sites(clair_engine_t *e, int slot, clair_sites_t *t, int64_t first, const void *input, int input_is_counts, int64_t input_stride_bytes, int n,
                       const uint8_t *centre, const uint8_t *seq) {
    if (check_sites(t, "clair_submit_sites", true)) return 1;
    if (e != t->e) return fail(e, "clair_submit_sites: the site table belongs to another engine");
    clair_engine::Request q{input, input_is_counts != 0, input_stride_bytes, n, centre, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (check_request(e, slot, q, input && centre && seq, "NULL input, centre or seq pointer") || check_stride(e, q)) return 1;
    if (check_source_range(t, "clair_submit_sites", first, n)) return 1;
    if (fused_possible(e)) return fail(e, "clair_submit_sites runs on the two-launch layer-2 path only: unset CLAIR_AMD_LSTM2_FUSED");
    q.models = (int)e->models.size();
    for (int k = 0; k < q.models; ++k)
        if (!e->models[k]->ready) return fail(e, "weights of model %d not loaded: clair_ensemble_set_tensor for all tensors, then clair_ensemble_finalize_weights", k);
    q.sites = t;
    q.sites_first = first;
    q.seq = seq;
    return submit_request(e, slot, q);
}

// One run's rows alone, on probabilities the caller holds: synchronous, needs no weights (the twin of clair_ensemble_average).  x, centre
// and seq (each optional) are what the rows that are new take along, as after the first pass of clair_submit_sites.
int clair_sites_add_rows(clair_engine_t *e, clair_sites_t *t, int64_t first, const float *probs, int n, const float *x, const uint8_t *centre, const uint8_t *seq) {
    if (check_sites(t, "clair_sites_add_rows", true)) return 1;
    if (e != t->e) return fail(e, "clair_sites_add_rows: the site table belongs to another engine");
    if (check_slot(e, 0, false) || check_n(e, n)) return 1;
    if (!probs) return fail(e, "NULL input pointer");
    if (check_source_range(t, "clair_sites_add_rows", first, n)) return 1;
    if (fused_possible(e)) return fail(e, "clair_sites_add_rows is not available on a handle with the fused layer-2 launch: unset CLAIR_AMD_LSTM2_FUSED");
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[0];
    if (s.pending_n) return fail(e, "slot 0 still has a pending submit; call clair_wait first");
    if (ensure_slot_decode(e, s) || ensure_slot_sites(e, s)) return 1;
    Lane &l = *e->lanes[s.lane];
    std::lock_guard<std::mutex> g(l.order);
    HIP_TRY(e, hipMemcpyAsync(s.d_out.p, probs, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyHostToDevice, l.stream));
    if (x) HIP_TRY(e, hipMemcpyAsync(s.d_x.p, x, (size_t)n * SITE_X * sizeof(float), hipMemcpyHostToDevice, l.stream));
    // rows without a centre or a seq of their own take zeros
    if (centre) HIP_TRY(e, hipMemcpyAsync(s.d_centre.p, centre, (size_t)n * 2, hipMemcpyHostToDevice, l.stream));
    else HIP_TRY(e, hipMemsetAsync(s.d_centre.p, 0, (size_t)n * 2, l.stream));
    if (seq) HIP_TRY(e, hipMemcpyAsync(s.d_seq.p, seq, (size_t)n * SITE_SEQ, hipMemcpyHostToDevice, l.stream));
    else HIP_TRY(e, hipMemsetAsync(s.d_seq.p, 0, (size_t)n * SITE_SEQ, l.stream));
    if (enqueue_sites_adopt(e, l, s, t, first, n, x != nullptr) || enqueue_sites_accumulate(e, l, s, t, first, n)) return 1;
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    return read_overflow(t, "clair_sites_add_rows");
}

int clair_sites_finish(clair_sites_t *t, int min_count, int order, int64_t *n_out) {
    if (check_sites(t, "clair_sites_finish", false)) return 1;
    clair_engine *e = t->e;
    if (order != CLAIR_SITES_ORDER_CHAIN && order != CLAIR_SITES_ORDER_POSITION) return fail(e, "clair_sites_finish: order %d is neither chain (0) nor position (1)", order);
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    if (read_overflow(t, "clair_sites_finish")) return 1;
    Lane &l = *e->lanes[0];
    std::lock_guard<std::mutex> g(l.order);
    const int64_t ns = t->n_sites;
    uint32_t kept = 0;
    if (ns > 0) {
        const int64_t *idx_row = order == CLAIR_SITES_ORDER_POSITION ? t->idx_row[t->cur].as<int64_t>() : nullptr;
        const unsigned blocks = (unsigned)((ns + 255) / 256);
        HIP_TRY(e, t->keep.ensure((size_t)ns * sizeof(uint32_t)));
        HIP_TRY(e, t->out_before.ensure((size_t)(ns + 1) * sizeof(uint32_t)));
        // a site is a position some run produced: a row begun but never fed (count 0) is none, whatever the minimum
        hipLaunchKernelGGL(sites_keep_kernel, dim3(blocks), dim3(256), 0, l.stream, t->count.as<int>(), idx_row, ns, std::max(min_count, 1), t->keep.as<uint32_t>());
        hipLaunchKernelGGL(sites_scan_kernel, dim3(1), dim3(256), 0, l.stream, t->keep.as<uint32_t>(), ns, t->out_before.as<uint32_t>());
        HIP_TRY(e, hipGetLastError());
        HIP_TRY(e, hipMemcpyAsync(&kept, t->out_before.as<uint32_t>() + ns, sizeof kept, hipMemcpyDeviceToHost, l.stream));
        HIP_TRY(e, hipStreamSynchronize(l.stream));
        if (kept) {
            HIP_TRY(e, t->out_row.ensure((size_t)kept * sizeof(int64_t)));
            HIP_TRY(e, t->out_key.ensure((size_t)kept * sizeof(int64_t)));
            HIP_TRY(e, t->out_count.ensure((size_t)kept * sizeof(int)));
            HIP_TRY(e, t->out_seq.ensure((size_t)kept * SITE_SEQ));
            HIP_TRY(e, t->avg.ensure((size_t)kept * OUT_FLOATS * sizeof(float)));
            hipLaunchKernelGGL(sites_compact_kernel, dim3(blocks), dim3(256), 0, l.stream, t->rows(), idx_row, ns, t->keep.as<uint32_t>(), t->out_before.as<uint32_t>(),
                               t->out_row.as<int64_t>(), t->out_key.as<int64_t>(), t->out_count.as<int>(), t->out_seq.as<unsigned char>());
            const int64_t n_values = (int64_t)kept * OUT_FLOATS;
            hipLaunchKernelGGL(sites_average_kernel, dim3((unsigned)((n_values + 255) / 256)), dim3(256), 0, l.stream, t->rows(), t->out_row.as<int64_t>(), n_values,
                               t->avg.as<float>());
            HIP_TRY(e, hipGetLastError());
            HIP_TRY(e, hipStreamSynchronize(l.stream));
        }
    }
    t->finished = true;
    t->n_out = kept;
    if (n_out) *n_out = kept;
    return 0;
}

int clair_sites_info(clair_sites_t *t, int64_t first, int64_t n, int64_t *positions, int32_t *counts, uint8_t *seq) {
    if (check_sites(t, "clair_sites_info", false) || check_output_range(t, "clair_sites_info", first, n)) return 1;
    clair_engine *e = t->e;
    HIP_TRY(e, hipSetDevice(e->device));
    if (n == 0) return 0;
    if (positions) HIP_TRY(e, hipMemcpy(positions, t->out_key.as<int64_t>() + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (counts) HIP_TRY(e, hipMemcpy(counts, t->out_count.as<int>() + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (seq) HIP_TRY(e, hipMemcpy(seq, t->out_seq.as<unsigned char>() + (size_t)first * SITE_SEQ, (size_t)n * SITE_SEQ, hipMemcpyDeviceToHost));
    return 0;
}

int clair_sites_rows(clair_sites_t *t, int64_t first, int64_t n, float *out) {
    if (check_sites(t, "clair_sites_rows", false) || check_output_range(t, "clair_sites_rows", first, n)) return 1;
    clair_engine *e = t->e;
    if (n > 0 && !out) return fail(e, "clair_sites_rows: out is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (n > 0) HIP_TRY(e, hipMemcpy(out, t->avg.as<float>() + (size_t)first * OUT_FLOATS, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int clair_sites_windows(clair_sites_t *t, int64_t first, int64_t n, float *x) {
    if (check_sites(t, "clair_sites_windows", false) || check_output_range(t, "clair_sites_windows", first, n)) return 1;
    clair_engine *e = t->e;
    if (n > INT32_MAX || (n > 0 && !x)) return fail(e, "clair_sites_windows: bad arguments");
    if (n == 0) return 0;
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    Lane &l = *e->lanes[0];
    std::lock_guard<std::mutex> g(l.order);
    if (t->gathered.bytes < (size_t)n * SITE_X * sizeof(float)) HIP_TRY(e, t->gathered.ensure((size_t)n * SITE_X * sizeof(float)));
    hipLaunchKernelGGL(sites_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, l.stream, t->rows(), t->out_row.as<int64_t>(), t->avg.as<float>(), first, (int)n,
                       t->gathered.as<float>(), (unsigned char *)nullptr, (float *)nullptr);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(x, t->gathered.p, (size_t)n * SITE_X * sizeof(float), hipMemcpyDeviceToHost, l.stream));
    HIP_TRY(e, hipStreamSynchronize(l.stream));
    return 0;
}

// The decode of entries [first, first + n) of the output list: a gather into the slot, then what clair_submit_ensemble leaves behind its
// last pass -- decode_kernel and the result copy, unchanged.  Pair with clair_wait(slot).
int clair_submit_site_calls(clair_engine_t *e, int slot, clair_sites_t *t, int64_t first, int n, clair_call_t *calls, float *gt21, float *genotype, float *l1, float *l2) {
    if (check_sites(t, "clair_submit_site_calls", false)) return 1;
    if (e != t->e) return fail(e, "clair_submit_site_calls: the site table belongs to another engine");
    if (check_slot(e, slot, false) || check_n(e, n)) return 1;
    if ((gt21 || genotype || l1 || l2) && !(gt21 && genotype && l1 && l2)) return fail(e, "the four probability arrays come together or not at all");
    if (!gt21 && !calls) return fail(e, "nothing asked for: neither call records nor probabilities");
    if (check_output_range(t, "clair_submit_site_calls", first, n)) return 1;
    if (fused_possible(e)) return fail(e, "clair_submit_site_calls runs on the two-launch layer-2 path only: unset CLAIR_AMD_LSTM2_FUSED");
    HIP_TRY(e, hipSetDevice(e->device));
    Slot &s = e->slots[slot];
    if (s.pending_n) return fail(e, "slot %d still has a pending submit; call clair_wait first", slot);
    if (ensure_slot_decode(e, s)) return 1;
    Lane &l = *e->lanes[s.lane];
    s.o_gt21 = gt21; s.o_gt = genotype; s.o_l1 = l1; s.o_l2 = l2;
    s.o_calls = calls;
    s.refetch = false;
    s.staged = 0;
    const bool same_out = s.cout == l.stream;
    {
        std::lock_guard<std::mutex> g(l.order);
        hipLaunchKernelGGL(sites_gather_kernel, dim3((n + 3) / 4), dim3(256), 0, l.stream, t->rows(), t->out_row.as<int64_t>(), t->avg.as<float>(), first, n, s.d_x.as<float>(),
                           s.d_centre.as<unsigned char>(), s.d_out.as<float>());
        HIP_TRY(e, hipGetLastError());
        if (calls && enqueue_decode(e, l, s, n)) return 1;
        if (same_out) { if (enqueue_results(e, l, s, n, calls != nullptr, gt21 != nullptr)) return 1; }
        else HIP_TRY(e, hipEventRecord(s.ev_done, l.stream));
    }
    if (!same_out) {
        HIP_TRY(e, hipStreamWaitEvent(s.cout, s.ev_done, 0));
        if (enqueue_results(e, l, s, n, calls != nullptr, gt21 != nullptr)) return 1;
    }
    s.pending_n = n;
    return 0;
}

int clair_predict(clair_engine_t *e, const float *x, int n, float *gt21, float *genotype, float *l1, float *l2) {
    if (clair_submit(e, 0, x, n, gt21, genotype, l1, l2)) return 1;
    return clair_wait(e, 0);
}

int clair_dataset_alloc(clair_engine_t *e, int64_t N, void **x_dev, void **out_dev) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (N < 1 || !x_dev || !out_dev) return fail(e, "bad arguments to clair_dataset_alloc");
    HIP_TRY(e, hipSetDevice(e->device));
    // +max_pad rows of zeroed slack so the last (padded) tile of a run never reads past the end
    const size_t rows = (size_t)N + e->max_pad;
    HIP_TRY(e, hipMalloc(x_dev, rows * CLAIR_INPUT_FLOATS * sizeof(float)));
    HIP_TRY(e, hipMemset(*x_dev, 0, rows * CLAIR_INPUT_FLOATS * sizeof(float)));
    HIP_TRY(e, hipMalloc(out_dev, rows * OUT_FLOATS * sizeof(float)));
    HIP_TRY(e, hipMemset(*out_dev, 0, rows * OUT_FLOATS * sizeof(float)));
    return 0;
}

int clair_dataset_free(clair_engine_t *e, void *x_dev, void *out_dev) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipDeviceSynchronize());
    HIP_TRY(e, hipFree(x_dev));
    HIP_TRY(e, hipFree(out_dev));
    return 0;
}

int clair_dataset_upload(clair_engine_t *e, void *x_dev, int64_t first, const float *x_host, int64_t n) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpy((float *)x_dev + (size_t)first * CLAIR_INPUT_FLOATS, x_host, (size_t)n * CLAIR_INPUT_FLOATS * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int clair_dataset_download(clair_engine_t *e, const void *out_dev, int64_t first, float *out_host, int64_t n) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpy(out_host, (const float *)out_dev + (size_t)first * OUT_FLOATS, (size_t)n * OUT_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int clair_run_resident(clair_engine_t *e, int slot, const void *x_dev, void *out_dev, int64_t first, int n) {
    if (check_slot(e, slot) || check_n(e, n)) return 1;
    HIP_TRY(e, hipSetDevice(e->device));
    Lane &l = *e->lanes[e->slots[slot].lane];
    std::lock_guard<std::mutex> g(l.order);
    return enqueue_forward(e, l, *e->models[0], (const float *)x_dev + (size_t)first * CLAIR_INPUT_FLOATS, (float *)out_dev + (size_t)first * OUT_FLOATS, n, -1);
}

int clair_sync(clair_engine_t *e) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    return check_fused_placement(e);
}

int clair_timing_enable(clair_engine_t *e, int on) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (drain_timers(e)) return 1;
    e->timing_mask = on == 0 ? 0u : (on == 1 ? ~0u : (unsigned)on);
    return 0;
}

int clair_kernel_times(clair_engine_t *e, double *ms_sum, int64_t *launches) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (drain_timers(e)) return 1;
    for (int k = 0; k < CLAIR_K_COUNT; ++k) {
        if (ms_sum) ms_sum[k] = e->ms_sum[k];
        if (launches) launches[k] = e->launches[k];
    }
    return 0;
}

int clair_timing_reset(clair_engine_t *e) {
    if (!e) return fail(nullptr, "engine is NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    if (drain_timers(e)) return 1;
    for (int k = 0; k < CLAIR_K_COUNT; ++k) { e->ms_sum[k] = 0; e->launches[k] = 0; }
    return 0;
}

int clair_kernel_workgroups(clair_engine_t *e, int n, int *workgroups) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (!workgroups) return fail(e, "workgroups is NULL");
    if (n < 1 || n > e->max_batch) return fail(e, "n %d out of range [1,%d]", n, e->max_batch);
    const int n_pad = (n + 31) & ~31, ntiles = n_pad / 32;
    const int x_tiles = (T_POS * n_pad + GS_ROWS - 1) / GS_ROWS;
    for (int k = 0; k < CLAIR_K_COUNT; ++k) workgroups[k] = 0;
    workgroups[CLAIR_K_LSTM1] = ntiles * 2;
    workgroups[CLAIR_K_LSTM2] = use_lstm2_pair(e, ntiles) ? ((ntiles + 1) / 2) * 2 : ntiles * 2;
    workgroups[CLAIR_K_PROJ2] = 32 * std::min(e->proj2_groups, (x_tiles + 7) / 8);
    if (use_lstm2_fused(e, ntiles)) {   // one launch: the projection workgroups first, then the recurrent ones
        workgroups[CLAIR_K_LSTM2] = 32 * e->fused_groups + 32 * ((ntiles / 2 + 7) / 8);
        workgroups[CLAIR_K_PROJ2] = 0;
    }
    workgroups[CLAIR_K_L4] = l34_grid((n_pad + L34_CAND - 1) / L34_CAND);
    workgroups[CLAIR_K_TAIL] = n_pad / TAIL_TILE;
    workgroups[CLAIR_K_DECODE] = (n + 3) / 4;       // launched only by clair_submit_ex with call records asked for
    return 0;
}

int clair_pinned_alloc(clair_engine_t *e, int64_t bytes, void **ptr) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (!ptr || bytes < 1) return fail(e, "bad arguments to clair_pinned_alloc");
    HIP_TRY(e, hipSetDevice(e->device));
    std::list<PinnedBuffer> one(1);
    HIP_TRY(e, one.front().ensure((size_t)bytes));
    *ptr = one.front().p;
    std::lock_guard<std::mutex> g(e->pinned_mu);
    e->pinned.splice(e->pinned.end(), one);
    return 0;
}

int clair_pinned_free(clair_engine_t *e, void *ptr) {
    if (!e) return fail(nullptr, "engine is NULL");
    bool known = false;
    {
        std::lock_guard<std::mutex> g(e->pinned_mu);
        for (const auto &b : e->pinned) known |= b.p == ptr;
    }
    if (!known) return fail(e, "clair_pinned_free: not a buffer of clair_pinned_alloc");
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;   // no copy may still be reading it (and no staging worker is looking it up)
    std::lock_guard<std::mutex> g(e->pinned_mu);
    e->pinned.remove_if([ptr](const PinnedBuffer &b) { return b.p == ptr; });   // released with its entry
    return 0;
}

int clair_engine_counter(clair_engine_t *e, int which, int64_t *value) {
    if (!e) return fail(nullptr, "engine is NULL");
    if (!value) return fail(e, "value is NULL");
    switch (which) {
        case 0: *value = e->fused_launches; return 0;
        case 1: *value = e->fused_recoveries; return 0;
        default: return fail(e, "clair_engine_counter: unknown counter %d", which);
    }
}

int clair_debug_read(clair_engine_t *e, int slot, int which, float *host, int64_t count) {
    if (check_slot(e, slot)) return 1;
    HIP_TRY(e, hipSetDevice(e->device));
    if (quiesce(e)) return 1;
    Lane &l = *e->lanes[e->slots[slot].lane];
    const float *src = nullptr;
    int64_t avail = 0;
    const int64_t np = l.last_n_pad;
    if (which == 1) {   // LSTM1 output lives as two fp16 planes: hand back their fp32 sum
        avail = (int64_t)T_POS * np * 256;
        if (count > avail) return fail(e, "clair_debug_read: asked %lld floats, tap 1 holds %lld", (long long)count, (long long)avail);
        std::vector<unsigned short> planes((size_t)2 * avail);
        HIP_TRY(e, hipMemcpy(planes.data(), l.a1.p, planes.size() * sizeof(unsigned short), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < count; ++i) host[i] = f16_value(planes[i]) + f16_value(planes[avail + i]);
        return 0;
    }
    if (which == 2) {   // LSTM2 output lives channel-group-major [32][33][n_pad][8] (lstm32.hip.h): hand it back as [33][n_pad][256]
        avail = (int64_t)T_POS * np * 256;
        if (count > avail) return fail(e, "clair_debug_read: asked %lld floats, tap 2 holds %lld", (long long)count, (long long)avail);
        std::vector<float> raw((size_t)avail);
        HIP_TRY(e, hipMemcpy(raw.data(), l.a2.p, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < count; ++i) {
            const int64_t t = i / (np * 256), n = (i / 256) % np, c = i % 256;
            host[i] = raw[(size_t)((((c / 8) * T_POS + t) * np + n) * 8 + c % 8)];
        }
        return 0;
    }
    switch (which) {
        case 4: if (!e->tap_l3) return fail(e, "clair_debug_read: tap 4 needs CLAIR_AMD_TAP_L3=1 at engine creation");
                src = l.zx.as<float>(); avail = np * L3_OUT; break;
        case 5: if (!e->l34_stamps) return fail(e, "clair_debug_read: tap 5 needs CLAIR_AMD_L34_STAMPS=1 at engine creation");
                src = l.zx.as<float>(); avail = ((np + L34_CAND - 1) / L34_CAND) * L4_SPLITS * 8 * 16 * 2; break;   // uint64 pairs of floats
        case 3: {   // split-K partials live in the accumulator layout (dense.hip.h): hand them back as [8 splits][n_pad][192] in W4's own units
            avail = (int64_t)L4_SPLITS * np * L4_UNITS;
            if (count > avail) return fail(e, "clair_debug_read: asked %lld floats, tap 3 holds %lld", (long long)count, (long long)avail);
            const int64_t nblk = (np + L34_CAND - 1) / L34_CAND;
            std::vector<float> raw((size_t)L4_SPLITS * nblk * L34_CAND * L4_UNITS);
            HIP_TRY(e, hipMemcpy(raw.data(), l.l4part.p, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
            const float inv = std::ldexp(1.0f, -e->models[0]->w4_shift) / L34_ACT_SCALE;
            for (int64_t i = 0; i < count; ++i) {
                const int64_t cg = i / (np * L4_UNITS), n = (i / L4_UNITS) % np, col = i % L4_UNITS;
                const int64_t blk = n / 64, row = n % 64, mb = row / 32, a = (row % 32) / 8, hq = (row % 8) / 4, r = row % 4;
                const int64_t nh = col / 96, nb = (col % 96) / 32, l32 = col % 32;
                host[i] = raw[(size_t)((((((cg * nblk + blk) * 2 + nh) * 6 + mb * 3 + nb) * 4 + a) * 64 + hq * 32 + l32) * 4 + r)] * inv;
            }
            return 0;
        }
        default: return fail(e, "clair_debug_read: unknown tap %d", which);
    }
    if (count > avail) return fail(e, "clair_debug_read: asked %lld floats, tap %d holds %lld", (long long)count, which, (long long)avail);
    HIP_TRY(e, hipMemcpy(host, src, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
