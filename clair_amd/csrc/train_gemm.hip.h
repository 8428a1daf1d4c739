// tgemm: the one strided-batched float32 GEMM of the training path (csrc/train.hip), on v_mfma_f32_32x32x2_f32.
//
//   C[b] (+)= op(A[b]) . op(B[b]) (+ bias[b][col])
//
// Every operand is addressed by element strides, so a transposed operand is only another pair of strides and the slice-dense layer L3
// ("ntc,ctu->nuc", its output column u*256+c) is a batch over c with strides.  A 64x64 block of C per workgroup of four waves, each wave one
// 32x32 tile; K goes through LDS 16 at a time.  Elements outside M, N or K are read as zeros and never written, so any M, N, K is exact.
// The K order of every output element is fixed (k ascending, one fused multiply-add per k), no split-K and no atomics: the same inputs give
// the same bits.  Untuned on purpose (docs/train.md): no software pipelining, scalar global loads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace clair_train {

struct GemmArgs {
    const float *A, *B, *bias;      // bias: per output column, or nullptr
    float *C;
    int M, N, K;
    int64_t sam, sak;               // A(m, k) = A[m * sam + k * sak]
    int64_t sbk, sbn;               // B(k, n) = B[k * sbk + n * sbn]
    int64_t scm, scn;               // C(m, n) = C[m * scm + n * scn]
    int64_t ba, bb, bc, bbias;      // per-batch offsets
    int accumulate;                 // C += A.B instead of C = A.B
};

constexpr int TG_M = 64, TG_N = 64, TG_K = 16, TG_LD = 68;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__global__ __launch_bounds__(256) void tgemm_kernel(GemmArgs g) {
    __shared__ float As[TG_K][TG_LD];       // [k][m]
    __shared__ float Bs[TG_K][TG_LD];       // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * TG_M, n0 = blockIdx.x * TG_N;
    const int64_t b = blockIdx.z;
    const float *A = g.A + b * g.ba, *B = g.B + b * g.bb;
    float *C = g.C + b * g.bc;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const bool a_kfast = g.sak == 1, b_nfast = g.sbn == 1;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < g.K; k0 += TG_K) {
        for (int p = 0; p < 4; ++p) {
            int m, k;
            if (a_kfast) { k = tid & 15; m = (tid >> 4) + 16 * p; } else { m = tid & 63; k = (tid >> 6) + 4 * p; }
            const int gm = m0 + m;
            int gk = k0 + k;
            As[k][m] = (gm < g.M && gk < g.K) ? A[(int64_t)gm * g.sam + (int64_t)gk * g.sak] : 0.f;
            int n;
            if (b_nfast) { n = tid & 63; k = (tid >> 6) + 4 * p; } else { k = tid & 15; n = (tid >> 4) + 16 * p; }
            const int gn = n0 + n;
            gk = k0 + k;
            Bs[k][n] = (gn < g.N && gk < g.K) ? B[(int64_t)gk * g.sbk + (int64_t)gn * g.sbn] : 0.f;
        }
        __syncthreads();
        for (int kk = 0; kk < TG_K; kk += 2) {
            const float a = As[kk + (lane >> 5)][wm + (lane & 31)];
            const float bv = Bs[kk + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = n0 + wn + (lane & 31);
    if (col >= g.N) return;
    const float bias = g.bias ? g.bias[b * g.bbias + col] : 0.f;
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= g.M) continue;
        float *c = C + (int64_t)row * g.scm + (int64_t)col * g.scn;
        const float v = acc[r] + bias;
        *c = g.accumulate ? *c + v : v;
    }
}

inline hipError_t tgemm(hipStream_t s, const GemmArgs &g, int batch = 1) {
    if (g.M <= 0 || g.N <= 0 || batch <= 0) return hipSuccess;
    dim3 grid((g.N + TG_N - 1) / TG_N, (g.M + TG_M - 1) / TG_M, batch);
    hipLaunchKernelGGL(tgemm_kernel, grid, dim3(256), 0, s, g);
    return hipGetLastError();
}

}  // namespace clair_train
