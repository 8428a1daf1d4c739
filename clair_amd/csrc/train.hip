// Training on the device (include/clair_amd.h: clair_train_*; docs/train.md): forward pass with the gates kept, losses, backward pass and the
// optimizer, all float32.  A trainer is its own handle: it needs no engine and shares nothing with the inference kernels, which read fp16-split
// weight images and keep no gates.
//
// Layout.  The 22 tensors of enum clair_tensor_id lie back to back in one flat vector per set (weights, gradients, Adam m | momentum, Adam v).
// Activations of a micro-batch of n rows are time-major: a1, a2 [33][n][256] (fw | bw halves), gates z [dir][33][n][512] (i|c~|f|o, turned into
// their pre-activation gradients in place by the backward pass), cell states c [dir][33][n][128].
//
// The recurrence is one GEMM launch (z_t += h_prev . K_h) and one pointwise launch per step and direction, forward and backward: 264 small
// launches per pass and layer pair.  Everything else is tgemm (csrc/train_gemm.hip.h), the kernels of csrc/train_kernels.hip.h and the accuracy
// count of csrc/train_accuracy.hip.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/clair_amd.h"
#include "device_buffer.h"
#include "hip_status.h"
#include "train_accuracy.hip.h"
#include "train_gemm.hip.h"
#include "train_kernels.hip.h"

using namespace clair_train;

namespace {

std::string g_train_error;

constexpr int N_TENSORS = 22;
constexpr int64_t TENSOR_COUNT[N_TENSORS] = {160 * 512, 512, 160 * 512, 512, 384 * 512, 512, 384 * 512, 512, 256 * 33 * 30, 256 * 30, 7680 * 192, 192,
                                             4 * 192 * 96, 4 * 96, 96 * 21, 21, 96 * 3, 3, 96 * 33, 33, 96 * 33, 33};
constexpr int HEAD_OFF[4] = {0, 21, 24, 57}, HEAD_SIZE[4] = {21, 3, 33, 33};
constexpr int MAX_MICRO_BATCH = 4096;
constexpr int MASK_WIDTH[6] = {T_STEPS * 256, 192, 96, 96, 96, 96};      // per row: LSTM2, L4, L5_1..4

}  // namespace

struct clair_trainer {
    int device = 0, cap = 0, optimizer = 0, loss = 0;
    hipStream_t stream = nullptr;
    int64_t offset[N_TENSORS + 1] = {0};
    int64_t n_params = 0, step = 0, seed = 0;
    float beta1_power = 1.f, beta2_power = 1.f;           // Adam's beta^t, multiplied up in float32 as TensorFlow's own variables are
    double task_weights[5] = {1, 1, 1, 1, 1};
    double class_weights[90];
    double rates[6] = {0.5, 0.5, 0.2, 0.2, 0.2, 0.2};
    int last_n = 0, last_training = 0;
    DeviceBuffer sets[4];                                  // weights, gradients, m | momentum, v
    DeviceBuffer x, xt, z1, c1, a1, z2, c2, a2, a2d, da2, da1, dhrec, dc, l3, dl3, y4, d4, dd4, y5, d5, dd5, lg, probs, dz;
    DeviceBuffer m_lstm2, m4, m5, labels, row_loss, sums, partial, stats, tp;
    DeviceBuffer dbg_a, dbg_b, dbg_bias, dbg_c;            // operands of clair_train_debug_gemm / _debug_column_sum, allocated on their first call
    std::string error;
};

namespace {

inline HipFail train_fail(clair_trainer *t) { return {t ? t->error : g_train_error}; }

inline dim3 blocks_for(int64_t count) { return dim3((unsigned)((count + 255) / 256)); }
#define LAUNCH(t, kernel, count, ...)                                                        \
    do {                                                                                     \
        if ((count) > 0) {                                                                   \
            hipLaunchKernelGGL(kernel, blocks_for(count), dim3(256), 0, (t)->stream, __VA_ARGS__); \
            CLAIR_HIP_TRY(train_fail(t), hipGetLastError());                                 \
        }                                                                                    \
    } while (0)

int train_init(clair_trainer *t) {
    CLAIR_HIP_TRY(train_fail(nullptr), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(nullptr), hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    for (int i = 0; i < N_TENSORS; ++i) t->offset[i + 1] = t->offset[i] + TENSOR_COUNT[i];
    t->n_params = t->offset[N_TENSORS];
    for (DeviceBuffer &b : t->sets) {
        CLAIR_HIP_TRY(train_fail(nullptr), b.ensure((size_t)t->n_params * 4));
        // on the handle's own stream: it does not wait for the null stream, where a hipMemset could still be clearing the weights after
        // the first clair_train_set_tensor has written them
        CLAIR_HIP_TRY(train_fail(nullptr), hipMemsetAsync(b.p, 0, (size_t)t->n_params * 4, t->stream));
    }
    CLAIR_HIP_TRY(train_fail(nullptr), hipStreamSynchronize(t->stream));
    const size_t cap = (size_t)t->cap, F = sizeof(float);
    struct { DeviceBuffer *b; size_t per_row; } plan[] = {
        {&t->x, T_STEPS * 32 * F}, {&t->xt, T_STEPS * 32 * F},
        {&t->z1, 2 * T_STEPS * 512 * F}, {&t->c1, 2 * T_STEPS * HID * F}, {&t->a1, T_STEPS * 256 * F},
        {&t->z2, 2 * T_STEPS * 512 * F}, {&t->c2, 2 * T_STEPS * HID * F}, {&t->a2, T_STEPS * 256 * F},
        {&t->a2d, T_STEPS * 256 * F}, {&t->da2, T_STEPS * 256 * F}, {&t->da1, T_STEPS * 256 * F},
        {&t->dhrec, HID * F}, {&t->dc, HID * F}, {&t->l3, 7680 * F}, {&t->dl3, 7680 * F},
        {&t->y4, 192 * F}, {&t->d4, 192 * F}, {&t->dd4, 192 * F}, {&t->y5, 384 * F}, {&t->d5, 384 * F}, {&t->dd5, 384 * F},
        {&t->lg, 90 * F}, {&t->probs, 90 * F}, {&t->dz, 90 * F},
        {&t->m_lstm2, T_STEPS * 256}, {&t->m4, 192}, {&t->m5, 384}, {&t->labels, 4}, {&t->row_loss, 4 * sizeof(double)},
    };
    for (auto &e : plan) CLAIR_HIP_TRY(train_fail(nullptr), e.b->ensure(cap * e.per_row));
    CLAIR_HIP_TRY(train_fail(nullptr), t->sums.ensure(4 * sizeof(double)));
    CLAIR_HIP_TRY(train_fail(nullptr), t->partial.ensure(2 * RED_BLOCKS * sizeof(double)));
    CLAIR_HIP_TRY(train_fail(nullptr), t->stats.ensure(3 * sizeof(double)));
    CLAIR_HIP_TRY(train_fail(nullptr), t->tp.ensure(4 * sizeof(int64_t)));
    for (double &w : t->class_weights) w = 1.0;
    return 0;
}

GemmArgs gemm(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, float *C, int64_t scm, int M, int N, int K,
              const float *bias = nullptr, int accumulate = 0) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = bias;
    g.M = M; g.N = N; g.K = K;
    g.sam = sam; g.sak = sak; g.sbk = sbk; g.sbn = sbn; g.scm = scm; g.scn = 1;
    g.accumulate = accumulate;
    return g;
}

int column_sum(clair_trainer *t, const float *x, int64_t rows, int cols, int64_t ld, float *out, int d = 1, int s1 = 1, int s2 = 0) {
    hipLaunchKernelGGL(column_sum_kernel, dim3((cols + 31) / 32), dim3(256), 0, t->stream, x, rows, cols, ld, out, d, s1, s2);
    CLAIR_HIP_TRY(train_fail(t), hipGetLastError());
    return 0;
}

struct Lstm {                   // one layer's buffers and tensors
    int kernel_id[2], in;
    float *z, *c, *a;
};

Lstm lstm_of(clair_trainer *t, int layer) {
    if (layer == 1) return Lstm{{CLAIR_T_LSTM1_FW_KERNEL, CLAIR_T_LSTM1_BW_KERNEL}, 32, t->z1.as<float>(), t->c1.as<float>(), t->a1.as<float>()};
    return Lstm{{CLAIR_T_LSTM2_FW_KERNEL, CLAIR_T_LSTM2_BW_KERNEL}, 256, t->z2.as<float>(), t->c2.as<float>(), t->a2.as<float>()};
}

// X [33 * n][in] time-major -> a [33][n][256]; gates and cell states of every step are kept
int lstm_forward(clair_trainer *t, int layer, const float *X, int n) {
    const Lstm L = lstm_of(t, layer);
    const float *P = t->sets[0].as<float>();
    for (int dir = 0; dir < 2; ++dir) {
        const float *K = P + t->offset[L.kernel_id[dir]], *bias = P + t->offset[L.kernel_id[dir] + 1];
        float *z = L.z + (int64_t)dir * T_STEPS * n * 512, *c = L.c + (int64_t)dir * T_STEPS * n * HID, *a = L.a + dir * HID;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(X, L.in, 1, K, 512, 1, z, 512, T_STEPS * n, 512, L.in, bias)));
        for (int s = 0; s < T_STEPS; ++s) {
            const int tt = dir == 0 ? s : T_STEPS - 1 - s, prev = dir == 0 ? tt - 1 : tt + 1;
            float *zt = z + (int64_t)tt * n * 512;
            if (s > 0)
                CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(a + (int64_t)prev * n * 256, 256, 1, K + (int64_t)L.in * 512, 512, 1, zt, 512, n, 512, HID, nullptr, 1)));
            LAUNCH(t, lstm_step_forward_kernel, (int64_t)n * HID, zt, s > 0 ? c + (int64_t)prev * n * HID : nullptr, c + (int64_t)tt * n * HID,
                   a + (int64_t)tt * n * 256, 256, n);
        }
    }
    return 0;
}

// dA [33][n][256]: gradient wrt the layer's output.  Adds the kernel and bias gradients; dX [33 * n][in] (or nullptr) gets both directions' sum.
int lstm_backward(clair_trainer *t, int layer, const float *X, const float *dA, float *dX, int n) {
    const Lstm L = lstm_of(t, layer);
    const float *P = t->sets[0].as<float>();
    float *G = t->sets[1].as<float>();
    float *dhrec = t->dhrec.as<float>(), *dc = t->dc.as<float>();
    for (int dir = 0; dir < 2; ++dir) {
        const float *K = P + t->offset[L.kernel_id[dir]];
        const float *Kh = K + (int64_t)L.in * 512;
        float *z = L.z + (int64_t)dir * T_STEPS * n * 512, *c = L.c + (int64_t)dir * T_STEPS * n * HID;
        const float *a = L.a + dir * HID;
        for (int s = 0; s < T_STEPS; ++s) {            // the reverse of the direction's own order
            const int tt = dir == 0 ? T_STEPS - 1 - s : s, prev = dir == 0 ? tt - 1 : tt + 1;
            const bool has_prev = s < T_STEPS - 1;
            float *zt = z + (int64_t)tt * n * 512;
            LAUNCH(t, lstm_step_backward_kernel, (int64_t)n * HID, zt, c + (int64_t)tt * n * HID, has_prev ? c + (int64_t)prev * n * HID : nullptr,
                   dA + (int64_t)tt * n * 256 + dir * HID, 256, s > 0 ? dhrec : nullptr, dc, s == 0 ? 1 : 0, n);
            if (has_prev) CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(zt, 512, 1, Kh, 1, 512, dhrec, HID, n, HID, 512)));      // dz_t . K_h^T
        }
        float *dK = G + t->offset[L.kernel_id[dir]];
        // dK = [x_t ; h_prev]^T . dz over all (t, n) rows: the x rows, then the h rows (the first step of the direction has no h_prev)
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(X, 1, L.in, z, 512, 1, dK, 512, L.in, 512, T_STEPS * n, nullptr, 1)));
        const float *h_prev = dir == 0 ? a : a + (int64_t)n * 256;
        const float *dz_next = dir == 0 ? z + (int64_t)n * 512 : z;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(h_prev, 1, 256, dz_next, 512, 1, dK + (int64_t)L.in * 512, 512, HID, 512, (T_STEPS - 1) * n, nullptr, 1)));
        if (column_sum(t, z, (int64_t)T_STEPS * n, 512, 512, G + t->offset[L.kernel_id[dir] + 1])) return 1;
        if (dX) CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(z, 512, 1, K, 1, 512, dX, L.in, T_STEPS * n, L.in, 512, nullptr, dir)));
    }
    return 0;
}

struct DropoutSelu { float a, b; uint32_t threshold; };
DropoutSelu dropout_selu_constants(double rate) {
    const double keep = 1.0 - rate, alpha = DROPOUT_SELU_ALPHA;
    const double a = std::sqrt(1.0 / (keep * ((1.0 - keep) * alpha * alpha + 1.0)));
    return DropoutSelu{(float)a, (float)(-a * (1.0 - keep) * alpha), (uint32_t)std::llround(keep * 16777216.0)};
}

int run_accumulate(clair_trainer *t, int n, int64_t first_row, int training, double *losses) {
    const float *P = t->sets[0].as<float>();
    float *G = t->sets[1].as<float>();
    const int64_t *off = t->offset;
    // ---- forward ----
    LAUNCH(t, transpose_x_kernel, (int64_t)n * T_STEPS * 32, t->x.as<float>(), t->xt.as<float>(), n);
    if (lstm_forward(t, 1, t->xt.as<float>(), n)) return 1;
    if (lstm_forward(t, 2, t->a1.as<float>(), n)) return 1;
    const int64_t a_count = (int64_t)T_STEPS * n * 256;
    const bool drop2 = training && t->rates[0] > 0.0;
    const float inv_keep2 = (float)(1.0 / (1.0 - t->rates[0]));
    float *a2d = drop2 ? t->a2d.as<float>() : t->a2.as<float>();
    if (drop2)
        LAUNCH(t, dropout_forward_kernel, a_count, t->a2.as<float>(), a2d, t->m_lstm2.as<uint8_t>(), n, 256, first_row, mask_key(t->seed, t->step, 0),
               (uint32_t)std::llround((1.0 - t->rates[0]) * 16777216.0), inv_keep2);
    else if (training)
        CLAIR_HIP_TRY(train_fail(t), hipMemsetAsync(t->m_lstm2.p, 1, (size_t)a_count, t->stream));
    // L3 "ntc,ctu->nuc": a batch over the 256 channels; output column u * 256 + c
    {
        GemmArgs g = gemm(a2d, 256, (int64_t)n * 256, P + off[CLAIR_T_L3_KERNEL], 30, 1, t->l3.as<float>(), 7680, n, 30, T_STEPS, P + off[CLAIR_T_L3_BIAS]);
        g.scn = 256; g.ba = 1; g.bb = T_STEPS * 30; g.bc = 1; g.bbias = 30;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, g, 256));
    }
    LAUNCH(t, selu_kernel, (int64_t)n * 7680, t->l3.as<float>(), (int64_t)n * 7680);
    CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->l3.as<float>(), 7680, 1, P + off[CLAIR_T_L4_KERNEL], 192, 1, t->y4.as<float>(), 192, n, 192, 7680, P + off[CLAIR_T_L4_BIAS])));
    const DropoutSelu k4 = dropout_selu_constants(t->rates[1]);
    LAUNCH(t, selu_dropout_forward_kernel, (int64_t)n * 192, t->y4.as<float>(), t->d4.as<float>(), t->m4.as<uint8_t>(), n, 192, first_row,
           mask_key(t->seed, t->step, 1), k4.threshold, k4.a, k4.b, training);
    {
        GemmArgs g = gemm(t->d4.as<float>(), 192, 1, P + off[CLAIR_T_L5_KERNEL], 96, 1, t->y5.as<float>(), 96, n, 96, 192, P + off[CLAIR_T_L5_BIAS]);
        g.bb = 192 * 96; g.bc = (int64_t)n * 96; g.bbias = 96;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, g, 4));
    }
    DropoutSelu k5[4];
    for (int k = 0; k < 4; ++k) {
        k5[k] = dropout_selu_constants(t->rates[2 + k]);
        const int64_t at = (int64_t)k * n * 96;
        LAUNCH(t, selu_dropout_forward_kernel, (int64_t)n * 96, t->y5.as<float>() + at, t->d5.as<float>() + at, t->m5.as<uint8_t>() + at, n, 96, first_row,
               mask_key(t->seed, t->step, 2 + k), k5[k].threshold, k5[k].a, k5[k].b, training);
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->d5.as<float>() + at, 96, 1, P + off[CLAIR_T_HEAD_GT21_KERNEL + 2 * k], HEAD_SIZE[k], 1, t->lg.as<float>() + HEAD_OFF[k], 90,
                                            n, HEAD_SIZE[k], 96, P + off[CLAIR_T_HEAD_GT21_BIAS + 2 * k])));
    }
    LAUNCH(t, selu_kernel, (int64_t)n * 90, t->lg.as<float>(), (int64_t)n * 90);
    {
        LossArgs a{};
        a.lg = t->lg.as<float>(); a.labels = t->labels.as<uint8_t>(); a.probs = t->probs.as<float>(); a.row_loss = t->row_loss.as<double>();
        a.dz = t->dz.as<float>();
        for (int c = 0; c < 90; ++c) a.class_weights[c] = t->class_weights[c];
        for (int k = 0; k < 4; ++k) a.task_weights[k] = t->task_weights[k];
        a.n = n; a.focal = t->loss == 0; a.training = training;
        LAUNCH(t, loss_kernel, (int64_t)n * 4, a);
        hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, t->stream, t->row_loss.as<double>(), n, t->sums.as<double>());
        CLAIR_HIP_TRY(train_fail(t), hipGetLastError());
    }
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(losses, t->sums.p, 4 * sizeof(double), hipMemcpyDeviceToHost, t->stream));
    if (!training) {
        CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
        return 0;
    }
    // ---- backward ----
    float *dz = t->dz.as<float>();
    for (int k = 0; k < 4; ++k) {
        const int64_t at = (int64_t)k * n * 96;
        const int hk = CLAIR_T_HEAD_GT21_KERNEL + 2 * k;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->d5.as<float>() + at, 1, 96, dz + HEAD_OFF[k], 90, 1, G + off[hk], HEAD_SIZE[k], 96, HEAD_SIZE[k], n, nullptr, 1)));
        if (column_sum(t, dz + HEAD_OFF[k], n, HEAD_SIZE[k], 90, G + off[hk + 1])) return 1;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(dz + HEAD_OFF[k], 90, 1, P + off[hk], 1, HEAD_SIZE[k], t->dd5.as<float>() + at, 96, n, 96, HEAD_SIZE[k])));
        LAUNCH(t, selu_dropout_backward_kernel, (int64_t)n * 96, t->dd5.as<float>() + at, t->y5.as<float>() + at, t->m5.as<uint8_t>() + at, (int64_t)n * 96, k5[k].a);
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->d4.as<float>(), 1, 192, t->dd5.as<float>() + at, 96, 1, G + off[CLAIR_T_L5_KERNEL] + (int64_t)k * 192 * 96, 96, 192, 96, n,
                                            nullptr, 1)));
        if (column_sum(t, t->dd5.as<float>() + at, n, 96, 96, G + off[CLAIR_T_L5_BIAS] + k * 96)) return 1;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->dd5.as<float>() + at, 96, 1, P + off[CLAIR_T_L5_KERNEL] + (int64_t)k * 192 * 96, 1, 96, t->dd4.as<float>(), 192, n, 192, 96,
                                            nullptr, k > 0)));
    }
    LAUNCH(t, selu_dropout_backward_kernel, (int64_t)n * 192, t->dd4.as<float>(), t->y4.as<float>(), t->m4.as<uint8_t>(), (int64_t)n * 192, k4.a);
    CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->l3.as<float>(), 1, 7680, t->dd4.as<float>(), 192, 1, G + off[CLAIR_T_L4_KERNEL], 192, 7680, 192, n, nullptr, 1)));
    if (column_sum(t, t->dd4.as<float>(), n, 192, 192, G + off[CLAIR_T_L4_BIAS])) return 1;
    CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, gemm(t->dd4.as<float>(), 192, 1, P + off[CLAIR_T_L4_KERNEL], 1, 192, t->dl3.as<float>(), 7680, n, 7680, 192)));
    LAUNCH(t, selu_backward_kernel, (int64_t)n * 7680, t->dl3.as<float>(), t->l3.as<float>(), (int64_t)n * 7680);
    {   // L3: dW[c][t][u] += sum_n a2d[t][n][c] dz3[n][u*256+c];  da2d[t][n][c] = sum_u dz3[n][u*256+c] W[c][t][u];  db[c][u] += sum_n dz3
        GemmArgs g = gemm(a2d, (int64_t)n * 256, 256, t->dl3.as<float>(), 7680, 256, G + off[CLAIR_T_L3_KERNEL], 30, T_STEPS, 30, n, nullptr, 1);
        g.ba = 1; g.bb = 1; g.bc = T_STEPS * 30;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, g, 256));
        GemmArgs h = gemm(t->dl3.as<float>(), 7680, 256, P + off[CLAIR_T_L3_KERNEL], 1, 30, t->da2.as<float>(), 256, n, T_STEPS, 30);
        h.scn = (int64_t)n * 256; h.ba = 1; h.bb = T_STEPS * 30; h.bc = 1;
        CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, h, 256));
        if (column_sum(t, t->dl3.as<float>(), n, 7680, 7680, G + off[CLAIR_T_L3_BIAS], 256, 1, 30)) return 1;
    }
    if (drop2) LAUNCH(t, dropout_backward_kernel, a_count, t->da2.as<float>(), t->m_lstm2.as<uint8_t>(), a_count, inv_keep2);
    if (lstm_backward(t, 2, t->a1.as<float>(), t->da2.as<float>(), t->da1.as<float>(), n)) return 1;
    if (lstm_backward(t, 1, t->xt.as<float>(), t->da1.as<float>(), nullptr, n)) return 1;
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

}  // namespace

extern "C" {

const char *clair_train_last_error(const clair_trainer_t *t) { return t ? t->error.c_str() : g_train_error.c_str(); }

int clair_train_create(int device, int micro_batch, int optimizer, int loss, clair_trainer_t **out) {
    if (!out) return train_fail(nullptr)("out is NULL");
    *out = nullptr;
    if (micro_batch < 1 || micro_batch > MAX_MICRO_BATCH) return train_fail(nullptr)("micro_batch %d: 1 .. %d", micro_batch, MAX_MICRO_BATCH);
    if (optimizer < 0 || optimizer > 1) return train_fail(nullptr)("optimizer %d: 0 (Adam) or 1 (SGDM)", optimizer);
    if (loss < 0 || loss > 1) return train_fail(nullptr)("loss %d: 0 (focal loss) or 1 (cross entropy)", loss);
    if (hip_device_check(train_fail(nullptr), device, "training runs on an MI355X only")) return 1;
    clair_trainer *t = new clair_trainer;
    t->device = device; t->cap = micro_batch; t->optimizer = optimizer; t->loss = loss;
    if (train_init(t)) {
        clair_train_destroy(t);
        return 1;
    }
    *out = t;
    return 0;
}

void clair_train_destroy(clair_trainer_t *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    hipStream_t stream = t->stream;
    delete t;                                   // the buffers go with it, before the stream
    if (stream) (void)hipStreamDestroy(stream);
}

static int tensor_range(clair_trainer *t, const char *what, int set, int tensor_id, const void *host, int64_t count) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (set < 0 || set > 3) return train_fail(t)("%s: set %d: 0 weights, 1 gradients, 2 Adam m | momentum, 3 Adam v", what, set);
    if (tensor_id < 0 || tensor_id >= N_TENSORS) return train_fail(t)("%s: tensor id %d out of range [0,%d)", what, tensor_id, N_TENSORS);
    if (!host) return train_fail(t)("%s: host is NULL", what);
    if (count != TENSOR_COUNT[tensor_id]) return train_fail(t)("%s: tensor %d has %lld elements, got %lld", what, tensor_id, (long long)TENSOR_COUNT[tensor_id], (long long)count);
    return 0;
}

int clair_train_set_tensor(clair_trainer_t *t, int set, int tensor_id, const float *host, int64_t count) {
    if (tensor_range(t, "clair_train_set_tensor", set, tensor_id, host, count)) return 1;
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(t->sets[set].as<float>() + t->offset[tensor_id], host, (size_t)count * 4, hipMemcpyHostToDevice, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_get_tensor(clair_trainer_t *t, int set, int tensor_id, float *host, int64_t count) {
    if (tensor_range(t, "clair_train_get_tensor", set, tensor_id, host, count)) return 1;
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(host, t->sets[set].as<float>() + t->offset[tensor_id], (size_t)count * 4, hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_config(clair_trainer_t *t, const double *task_loss_weights, const double *class_weights, const double *dropout_rates, int64_t seed) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (dropout_rates)
        for (int i = 0; i < 6; ++i)
            if (!(dropout_rates[i] >= 0.0 && dropout_rates[i] < 1.0)) return train_fail(t)("dropout rate %d is %g: 0 <= rate < 1", i, dropout_rates[i]);
    if (task_loss_weights) for (int i = 0; i < 5; ++i) t->task_weights[i] = task_loss_weights[i];
    if (class_weights) for (int i = 0; i < 90; ++i) t->class_weights[i] = class_weights[i];
    if (dropout_rates) for (int i = 0; i < 6; ++i) t->rates[i] = dropout_rates[i];
    t->seed = seed;
    return 0;
}

int clair_train_zero_grad(clair_trainer_t *t) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemsetAsync(t->sets[1].p, 0, (size_t)t->n_params * 4, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_accumulate(clair_trainer_t *t, const float *x, const uint8_t *labels, int n, int64_t first_row, int training, double *losses) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (n < 1 || n > t->cap) return train_fail(t)("%d rows in a micro-batch: 1 .. micro_batch = %d", n, t->cap);
    if (!x || !labels || !losses) return train_fail(t)("NULL argument");
    if (first_row < 0) return train_fail(t)("first_row %lld is negative", (long long)first_row);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k)
            if (labels[i * 4 + k] >= HEAD_SIZE[k]) return train_fail(t)("row %d: label %d of head %d: 0 .. %d", i, labels[i * 4 + k], k, HEAD_SIZE[k] - 1);
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(t->x.p, x, (size_t)n * T_STEPS * 32 * 4, hipMemcpyHostToDevice, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(t->labels.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, t->stream));
    t->last_n = 0;
    if (run_accumulate(t, n, first_row, training ? 1 : 0, losses)) return 1;
    t->last_n = n;
    t->last_training = training ? 1 : 0;
    return 0;
}

int clair_train_step(clair_trainer_t *t, double learning_rate, double l2_lambda, double *stats) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (!stats) return train_fail(t)("stats is NULL");
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    Segments segs;
    for (int i = 0; i < N_TENSORS; ++i) segs.end[i] = t->offset[i + 1];
    float *w = t->sets[0].as<float>(), *g = t->sets[1].as<float>();
    hipLaunchKernelGGL(regularize_norm_kernel, dim3(RED_BLOCKS), dim3(256), 0, t->stream, w, g, t->n_params, segs, (float)(t->task_weights[4] * l2_lambda),
                       t->partial.as<double>());
    CLAIR_HIP_TRY(train_fail(t), hipGetLastError());
    hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(64), 0, t->stream, t->partial.as<double>(), t->stats.as<double>());
    CLAIR_HIP_TRY(train_fail(t), hipGetLastError());
    t->step += 1;
    if (t->optimizer == 0) {
        const float lr = (float)learning_rate;
        t->beta1_power *= 0.9f;
        t->beta2_power *= 0.999f;
        const float lr_t = lr * std::sqrt(1.f - t->beta2_power) / (1.f - t->beta1_power);
        LAUNCH(t, adam_kernel, t->n_params, w, g, t->sets[2].as<float>(), t->sets[3].as<float>(), t->n_params, t->stats.as<double>(), lr_t);
    } else {
        LAUNCH(t, momentum_kernel, t->n_params, w, g, t->sets[2].as<float>(), t->n_params, t->stats.as<double>(), (float)learning_rate);
    }
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(stats, t->stats.p, 2 * sizeof(double), hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_read_mask(clair_trainer_t *t, int layer, uint8_t *host, int64_t count) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (layer < 0 || layer > 5) return train_fail(t)("mask layer %d: 0 LSTM2, 1 L4, 2..5 L5_1..4", layer);
    if (!host) return train_fail(t)("host is NULL");
    if (!t->last_n || !t->last_training) return train_fail(t)("no training accumulate to read masks of");
    const int64_t want = (int64_t)t->last_n * MASK_WIDTH[layer];
    if (count != want) return train_fail(t)("mask of layer %d has %lld bytes for %d rows, got %lld", layer, (long long)want, t->last_n, (long long)count);
    const uint8_t *src = layer == 0 ? t->m_lstm2.as<uint8_t>() : layer == 1 ? t->m4.as<uint8_t>() : t->m5.as<uint8_t>() + (int64_t)(layer - 2) * t->last_n * 96;
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(host, src, (size_t)count, hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_probabilities(clair_trainer_t *t, float *out) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (!out) return train_fail(t)("out is NULL");
    if (!t->last_n) return train_fail(t)("no accumulate to read probabilities of");
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(out, t->probs.p, (size_t)t->last_n * 90 * 4, hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_accuracy(clair_trainer_t *t, int64_t *tp) {
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (!tp) return train_fail(t)("tp is NULL");
    if (!t->last_n) return train_fail(t)("no accumulate to count the accuracy of");
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    CLAIR_HIP_TRY(train_fail(t), hipMemsetAsync(t->tp.p, 0, 4 * sizeof(int64_t), t->stream));
    LAUNCH(t, accuracy_kernel, t->last_n, t->probs.as<float>(), t->labels.as<uint8_t>(), t->last_n, t->tp.as<unsigned long long>());
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(tp, t->tp.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

}  // extern "C"

// ---- kernel taps for tests (include/clair_amd.h): these checks are all that stands between a test's typo and an access outside a buffer ----
namespace {

constexpr int64_t DEBUG_MAX_DIM = 1 << 20, DEBUG_MAX_BATCH = 65535, DEBUG_MAX_COUNT = 1 << 28;     // (extent - 1) * stride < 2^56: no index sum below can overflow

int debug_range(clair_trainer *t, const char *what, const char *name, int64_t v, int64_t lo, int64_t hi) {
    if (v < lo || v > hi) return train_fail(t)("%s: %s is %lld: %lld .. %lld", what, name, (long long)v, (long long)lo, (long long)hi);
    return 0;
}

// the operand's largest element index, the sum over (extent - 1) * stride of its three axes, must lie inside its `count` elements
int debug_operand(clair_trainer *t, const char *what, const char *name, const void *host, int64_t count, const int64_t (&extent)[3], const int64_t (&stride)[3],
                  const char *const (&stride_name)[3]) {
    if (!host) return train_fail(t)("%s: %s is NULL", what, name);
    if (count < 1 || count > DEBUG_MAX_COUNT) return train_fail(t)("%s: %s has %lld elements: 1 .. %lld", what, name, (long long)count, (long long)DEBUG_MAX_COUNT);
    int64_t last = 0;
    for (int i = 0; i < 3; ++i) {
        if (stride[i] < 0 || stride[i] > DEBUG_MAX_COUNT)
            return train_fail(t)("%s: %s: stride %s is %lld: 0 .. %lld", what, name, stride_name[i], (long long)stride[i], (long long)DEBUG_MAX_COUNT);
        last += (extent[i] - 1) * stride[i];
    }
    if (last >= count) return train_fail(t)("%s: %s: the largest element index %lld is outside its %lld elements", what, name, (long long)last, (long long)count);
    return 0;
}

int debug_upload(clair_trainer *t, DeviceBuffer &buf, const float *host, int64_t count) {
    CLAIR_HIP_TRY(train_fail(t), buf.ensure((size_t)count * 4));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(buf.p, host, (size_t)count * 4, hipMemcpyHostToDevice, t->stream));
    return 0;
}

}  // namespace

extern "C" {

int clair_train_debug_gemm(clair_trainer_t *t, const float *a, int64_t a_count, const float *b, int64_t b_count, const float *bias, int64_t bias_count,
                           float *c, int64_t c_count, const int64_t *dims, const int64_t *strides) {
    const char *what = "clair_train_debug_gemm";
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (!dims) return train_fail(t)("%s: dims is NULL", what);
    if (!strides) return train_fail(t)("%s: strides is NULL", what);
    const int64_t M = dims[0], N = dims[1], K = dims[2], batch = dims[3], accumulate = dims[4];
    if (debug_range(t, what, "M", M, 1, DEBUG_MAX_DIM) || debug_range(t, what, "N", N, 1, DEBUG_MAX_DIM) || debug_range(t, what, "K", K, 1, DEBUG_MAX_DIM) ||
        debug_range(t, what, "batch", batch, 1, DEBUG_MAX_BATCH) || debug_range(t, what, "accumulate", accumulate, 0, 1))
        return 1;
    const int64_t sam = strides[0], sak = strides[1], sbk = strides[2], sbn = strides[3], scm = strides[4], scn = strides[5], ba = strides[6], bb = strides[7],
                  bc = strides[8], bbias = strides[9];
    if (debug_operand(t, what, "A", a, a_count, {M, K, batch}, {sam, sak, ba}, {"sam", "sak", "ba"})) return 1;
    if (debug_operand(t, what, "B", b, b_count, {K, N, batch}, {sbk, sbn, bb}, {"sbk", "sbn", "bb"})) return 1;
    if (debug_operand(t, what, "C", c, c_count, {M, N, batch}, {scm, scn, bc}, {"scm", "scn", "bc"})) return 1;
    if (!bias && bias_count != 0) return train_fail(t)("%s: bias is NULL with bias_count %lld", what, (long long)bias_count);
    if (bias ? debug_operand(t, what, "bias", bias, bias_count, {N, batch, 1}, {1, bbias, 0}, {"1", "bbias", "0"}) : debug_range(t, what, "bbias", bbias, 0, DEBUG_MAX_COUNT))
        return 1;
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    if (debug_upload(t, t->dbg_a, a, a_count) || debug_upload(t, t->dbg_b, b, b_count) || debug_upload(t, t->dbg_c, c, c_count)) return 1;
    if (bias && debug_upload(t, t->dbg_bias, bias, bias_count)) return 1;
    GemmArgs g = gemm(t->dbg_a.as<float>(), sam, sak, t->dbg_b.as<float>(), sbk, sbn, t->dbg_c.as<float>(), scm, (int)M, (int)N, (int)K,
                      bias ? t->dbg_bias.as<float>() : nullptr, (int)accumulate);
    g.scn = scn; g.ba = ba; g.bb = bb; g.bc = bc; g.bbias = bbias;
    CLAIR_HIP_TRY(train_fail(t), tgemm(t->stream, g, (int)batch));
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(c, t->dbg_c.p, (size_t)c_count * 4, hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

int clair_train_debug_column_sum(clair_trainer_t *t, const float *x, int64_t x_count, int64_t rows, int cols, int64_t ld, float *out, int64_t out_count,
                                 int d, int s1, int s2) {
    const char *what = "clair_train_debug_column_sum";
    if (!t) return train_fail(nullptr)("trainer handle is NULL");
    if (debug_range(t, what, "rows", rows, 1, DEBUG_MAX_COUNT) || debug_range(t, what, "cols", cols, 1, DEBUG_MAX_DIM) || debug_range(t, what, "d", d, 1, DEBUG_MAX_COUNT))
        return 1;
    if (debug_operand(t, what, "x", x, x_count, {rows, cols, 1}, {ld, 1, 0}, {"ld", "1", "0"})) return 1;
    // column j goes to (j / d) * s1 + (j % d) * s2: no j has a larger quotient than cols - 1 or a larger remainder than min(d, cols) - 1
    if (debug_operand(t, what, "out", out, out_count, {(cols - 1) / d + 1, d < cols ? d : cols, 1}, {s1, s2, 0}, {"s1", "s2", "0"})) return 1;
    CLAIR_HIP_TRY(train_fail(t), hipSetDevice(t->device));
    if (debug_upload(t, t->dbg_a, x, x_count) || debug_upload(t, t->dbg_c, out, out_count)) return 1;
    if (column_sum(t, t->dbg_a.as<float>(), rows, cols, ld, t->dbg_c.as<float>(), d, s1, s2)) return 1;
    CLAIR_HIP_TRY(train_fail(t), hipMemcpyAsync(out, t->dbg_c.p, (size_t)out_count * 4, hipMemcpyDeviceToHost, t->stream));
    CLAIR_HIP_TRY(train_fail(t), hipStreamSynchronize(t->stream));
    return 0;
}

}  // extern "C"
