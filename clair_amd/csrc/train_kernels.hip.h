// The elementwise, loss and optimizer kernels of the training path (csrc/train.hip).  Everything is float32 except the loss and its row sums
// and the optimizer's sums of squares, which are float64; column_sum_kernel (the bias gradients) sums in float32, as tgemm does (docs/train.md
// holds both to the float32 oracle's error up to 150 rows).  Every reduction has a fixed order and none uses atomics: the same inputs give
// the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "train_set_core.h"

namespace clair_train {

constexpr int T_STEPS = 33, HID = 128;
constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f, SELU_SCALE = 1.0507009873554804934193349852946f;
constexpr double DROPOUT_SELU_ALPHA = -1.7580993408473766;      // clair/selu.py:39

// ---- dropout masks: a counter-based hash of (seed, optimizer step, layer) -> key, then (row of the whole batch, element) ----------------
__host__ __device__ inline uint64_t mix64(uint64_t z) { return clair_mix64(z); }     // train_set_core.h: the training-set draws hash with it too
inline uint64_t mask_key(int64_t seed, int64_t step, int layer) { return mix64(mix64((uint64_t)seed) ^ mix64((uint64_t)step * 8 + (uint64_t)layer)); }
// kept when the 24-bit draw is below keep * 2^24
__device__ inline uint8_t mask_bit(uint64_t key, int64_t row, int64_t elem, uint32_t threshold) {
    return (uint32_t)(mix64(mix64(key + (uint64_t)row) + (uint64_t)elem) >> 40) < threshold ? 1 : 0;
}

__device__ inline float selu_f(float x) { return SELU_SCALE * (x >= 0.f ? x : SELU_ALPHA * (expf(x) - 1.f)); }
// the derivative from the OUTPUT y = selu(x): scale where x >= 0, y + scale * alpha below.  For x in (-6e-8, 0) expf(x) - 1 rounds to -0, so
// y = -0 tests as >= 0 and the derivative returned is scale instead of scale * alpha (1.758): a measure-zero sliver of pre-activations, kept
// in exchange for storing the activation alone.
__device__ inline float selu_grad_from_y(float y) { return y >= 0.f ? SELU_SCALE : y + SELU_SCALE * SELU_ALPHA; }
__device__ inline float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

#define TRAIN_INDEX(count)                                                       \
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;         \
    if (idx >= (count)) return

// x [n][33][32] -> xt [33][n][32]
__global__ void transpose_x_kernel(const float *x, float *xt, int n) {
    TRAIN_INDEX((int64_t)n * T_STEPS * 32);
    const int f = idx & 31;
    const int64_t r = idx >> 5;
    const int t = r % T_STEPS;
    const int64_t i = r / T_STEPS;
    xt[((int64_t)t * n + i) * 32 + f] = x[idx];
}

// one LSTM step forward: z [n][512] pre-activations (i|c~|f|o) -> activated gates in place, c_t, h_t (row stride ldh)
__global__ void lstm_step_forward_kernel(float *z, const float *c_prev, float *c_out, float *h_out, int ldh, int n) {
    TRAIN_INDEX((int64_t)n * HID);
    const int j = idx & (HID - 1);
    const int64_t row = idx >> 7;
    float *g = z + row * 4 * HID;
    const float i = sigmoid_f(g[j]), cc = tanhf(g[HID + j]), f = sigmoid_f(g[2 * HID + j]), o = sigmoid_f(g[3 * HID + j]);
    const float c = (c_prev ? f * c_prev[idx] : 0.f) + i * cc;
    g[j] = i; g[HID + j] = cc; g[2 * HID + j] = f; g[3 * HID + j] = o;
    c_out[idx] = c;
    h_out[row * ldh + j] = o * tanhf(c);
}

// one LSTM step backward: gates [n][512] activated -> dz in place.  dh = dh_above (+ dh_rec); dc carries c's gradient to the step before.
__global__ void lstm_step_backward_kernel(float *gates, const float *c_t, const float *c_prev, const float *dh_above, int ldh, const float *dh_rec,
                                          float *dc, int first, int n) {
    TRAIN_INDEX((int64_t)n * HID);
    const int j = idx & (HID - 1);
    const int64_t row = idx >> 7;
    float *g = gates + row * 4 * HID;
    const float i = g[j], cc = g[HID + j], f = g[2 * HID + j], o = g[3 * HID + j];
    const float dh = dh_above[row * ldh + j] + (dh_rec ? dh_rec[idx] : 0.f);
    const float tc = tanhf(c_t[idx]);
    const float dct = dh * o * (1.f - tc * tc) + (first ? 0.f : dc[idx]);
    g[j] = dct * cc * i * (1.f - i);
    g[HID + j] = dct * i * (1.f - cc * cc);
    g[2 * HID + j] = c_prev ? dct * c_prev[idx] * f * (1.f - f) : 0.f;
    g[3 * HID + j] = dh * tc * o * (1.f - o);
    dc[idx] = dct * f;
}

// tf.layers.dropout on a [33][n][width] tensor: out = x * mask / keep, the mask bytes kept for the backward
__global__ void dropout_forward_kernel(const float *x, float *out, uint8_t *mask, int n, int width, int64_t first_row, uint64_t key, uint32_t threshold,
                                       float inv_keep) {
    TRAIN_INDEX((int64_t)T_STEPS * n * width);
    const int c = idx % width;
    const int64_t r = idx / width;
    const int64_t i = r % n;
    const int t = r / n;
    const uint8_t m = mask_bit(key, first_row + i, (int64_t)t * width + c, threshold);
    mask[idx] = m;
    out[idx] = m ? x[idx] * inv_keep : 0.f;
}
__global__ void dropout_backward_kernel(float *d, const uint8_t *mask, int64_t count, float inv_keep) {
    TRAIN_INDEX(count);
    d[idx] = mask[idx] ? d[idx] * inv_keep : 0.f;
}

__global__ void selu_kernel(float *z, int64_t count) {
    TRAIN_INDEX(count);
    z[idx] = selu_f(z[idx]);
}
// d (gradient wrt y = selu(z)) -> gradient wrt z, in place
__global__ void selu_backward_kernel(float *d, const float *y, int64_t count) {
    TRAIN_INDEX(count);
    d[idx] *= selu_grad_from_y(y[idx]);
}

// y = selu(z) in place, then dropout_selu (clair/selu.py:39-74): d = a * (y * mask + alpha' * (1 - mask)) + b on [n][width]
__global__ void selu_dropout_forward_kernel(float *y, float *d, uint8_t *mask, int n, int width, int64_t first_row, uint64_t key, uint32_t threshold, float a,
                                            float b, int training) {
    TRAIN_INDEX((int64_t)n * width);
    const float v = selu_f(y[idx]);
    y[idx] = v;
    if (!training) { d[idx] = v; return; }
    const uint8_t m = mask_bit(key, first_row + idx / width, idx % width, threshold);
    mask[idx] = m;
    d[idx] = a * (m ? v : (float)DROPOUT_SELU_ALPHA) + b;
}
// dd (gradient wrt the dropout output) -> gradient wrt z, in place: a * mask * dd * selu'(z)
__global__ void selu_dropout_backward_kernel(float *dd, const float *y, const uint8_t *mask, int64_t count, float a) {
    TRAIN_INDEX(count);
    dd[idx] = mask[idx] ? a * dd[idx] * selu_grad_from_y(y[idx]) : 0.f;
}

// ---- loss: per row and head the softmax of the SELU'd logits, the loss and d loss / d z (z = the head's pre-activation) -----------------
struct LossArgs {
    const float *lg;            // [n][90] selu(z)
    const uint8_t *labels;      // [n][4]
    float *probs;               // [n][90]
    double *row_loss;           // [n][4]
    float *dz;                  // [n][90], written when training
    double class_weights[90];
    double task_weights[4];
    int n, focal, training;
};
__global__ void loss_kernel(LossArgs a) {
    TRAIN_INDEX((int64_t)a.n * 4);
    const int head = idx & 3;
    const int64_t row = idx >> 2;
    const int off = head == 0 ? 0 : head == 1 ? 21 : head == 2 ? 24 : 57;
    const int size = head == 0 ? 21 : head == 1 ? 3 : 33;
    const float *lg = a.lg + row * 90 + off;
    const int y = a.labels[idx];
    double p[33], gp[33];
    double top = lg[0];
    for (int c = 1; c < size; ++c) top = lg[c] > top ? (double)lg[c] : top;
    double sum = 0.0;
    for (int c = 0; c < size; ++c) { p[c] = exp((double)lg[c] - top); sum += p[c]; }
    double loss = 0.0, dot = 0.0;
    for (int c = 0; c < size; ++c) {
        const double pc = p[c] / sum;
        p[c] = pc;
        a.probs[row * 90 + off + c] = (float)pc;
        double g = 0.0;
        if (a.focal) {          // clair/model.py:784-805, gamma 2, clip to [1e-8, 1]; the clip passes no gradient outside its range
            if (c == y) {
                const double q = 1.0 - pc, cl = pc < 1e-8 ? 1e-8 : pc;
                loss -= q * q * log(cl);
                g = 2.0 * q * log(cl) - (pc >= 1e-8 ? q * q / pc : 0.0);
            } else {
                const double q = 1.0 - pc, cl = q < 1e-8 ? 1e-8 : q;
                loss -= pc * pc * log(cl);
                g = -2.0 * pc * log(cl) + (q >= 1e-8 ? pc * pc / q : 0.0);
            }
        } else if (c == y) {    // clair/model.py:247-263
            const double w = a.class_weights[off + c];
            loss -= w * log(pc + 1e-10);
            g = -w / (pc + 1e-10);
        }
        gp[c] = g;
        dot += g * pc;
    }
    a.row_loss[idx] = loss;
    if (!a.training) return;
    for (int c = 0; c < size; ++c) {
        const double dlg = p[c] * (gp[c] - dot) * a.task_weights[head];
        a.dz[row * 90 + off + c] = (float)dlg * selu_grad_from_y(lg[c]);
    }
}

// sums[4] = per-head sums of row_loss [n][4], one workgroup, fixed order
__global__ __launch_bounds__(256) void loss_reduce_kernel(const double *row_loss, int n, double *sums) {
    __shared__ double part[256];
    const int head = threadIdx.x & 3, lane = threadIdx.x >> 2;      // 64 lanes per head
    double s = 0.0;
    for (int64_t r = lane; r < n; r += 64) s += row_loss[r * 4 + head];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int step = 128; step >= 4; step >>= 1) {
        if (threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x < 4) sums[threadIdx.x] = part[threadIdx.x];
}

// out[(j / d) * s1 + (j % d) * s2] += sum over rows of x[row * ld + j], j < cols: 32 columns per workgroup, 8 float32 partial sums per column
__global__ __launch_bounds__(256) void column_sum_kernel(const float *x, int64_t rows, int cols, int64_t ld, float *out, int d, int s1, int s2) {
    __shared__ float part[8][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + cx;
    float s = 0.f;
    if (j < cols)
        for (int64_t r = ry; r < rows; r += 8) s += x[r * ld + j];
    part[ry][cx] = s;
    __syncthreads();
    if (ry == 0 && j < cols) {
        float total = part[0][cx];
        for (int k = 1; k < 8; ++k) total += part[k][cx];
        out[(j / d) * s1 + (j % d) * s2] += total;
    }
}

// ---- optimizer ----------------------------------------------------------------------------------------------------------------------
struct Segments {               // the 22 tensors inside the flat parameter vector
    int64_t end[22];            // one past the tensor's last element
};
// the tensor idx lies in, searched on from tensor t (a thread's indices only grow); kernels have the even ids of enum clair_tensor_id
__device__ inline int tensor_of(const Segments &s, int64_t idx, int t) {
    while (t < 21 && idx >= s.end[t]) ++t;
    return t;
}

constexpr int RED_BLOCKS = 512;
// g += coef * w on kernel tensors; partial[2 * block + 0] = sum w^2 over kernels, [.. + 1] = sum g^2 (after the addition) over all
__global__ __launch_bounds__(256) void regularize_norm_kernel(const float *w, float *g, int64_t count, Segments segs, float coef, double *partial) {
    __shared__ double p0[256], p1[256];
    const int64_t chunk = (count + RED_BLOCKS - 1) / RED_BLOCKS;
    const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < count ? lo + chunk : count;
    double s0 = 0.0, s1 = 0.0;
    int tensor = 0;
    for (int64_t idx = lo + threadIdx.x; idx < hi; idx += 256) {
        float gv = g[idx];
        tensor = tensor_of(segs, idx, tensor);
        if ((tensor & 1) == 0) {
            const float wv = w[idx];
            s0 += (double)wv * wv;
            gv += coef * wv;
            g[idx] = gv;
        }
        s1 += (double)gv * gv;
    }
    p0[threadIdx.x] = s0; p1[threadIdx.x] = s1;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (threadIdx.x < step) { p0[threadIdx.x] += p0[threadIdx.x + step]; p1[threadIdx.x] += p1[threadIdx.x + step]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = p0[0]; partial[2 * blockIdx.x + 1] = p1[0]; }
}
// stats[0] = l2 loss (sum w^2 / 2), stats[1] = global norm, stats[2] = the clip factor 5 / max(norm, 5)
__global__ void norm_finish_kernel(const double *partial, double *stats) {
    if (threadIdx.x || blockIdx.x) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < RED_BLOCKS; ++b) { s0 += partial[2 * b]; s1 += partial[2 * b + 1]; }
    const double norm = sqrt(s1);
    stats[0] = 0.5 * s0;
    stats[1] = norm;
    stats[2] = 5.0 / (norm > 5.0 ? norm : 5.0);
}
// tf.train.AdamOptimizer (ApplyAdam): m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= lr_t * m / (sqrt(v) + eps)
__global__ void adam_kernel(float *w, const float *g, float *m, float *v, int64_t count, const double *stats, float lr_t) {
    TRAIN_INDEX(count);
    const float gv = g[idx] * (float)stats[2];
    const float mv = m[idx] + (gv - m[idx]) * (1.f - 0.9f);
    const float vv = v[idx] + (gv * gv - v[idx]) * (1.f - 0.999f);
    m[idx] = mv;
    v[idx] = vv;
    w[idx] -= (mv * lr_t) / (sqrtf(vv) + 1e-8f);
}
// tf.train.MomentumOptimizer(momentum 0.9): acc = 0.9 acc + g; w -= lr * acc
__global__ void momentum_kernel(float *w, const float *g, float *acc, int64_t count, const double *stats, float lr) {
    TRAIN_INDEX(count);
    const float a = acc[idx] * 0.9f + g[idx] * (float)stats[2];
    acc[idx] = a;
    w[idx] -= lr * a;
}

}  // namespace clair_train
