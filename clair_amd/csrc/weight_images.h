// The engine's weight images: the 22 tensors of a checkpoint (include/clair_amd.h: enum clair_tensor_id) packed into the layouts the
// kernels read them in.  Plain C++17 for the host: no HIP type appears here, engine.hip uploads what build_weight_images returns, and a
// host compiler with _Float16 can build and compare the images without a GPU.
//
// The layer constants the images depend on live with the kernels that own them (common.hip.h, dense.hip.h, lstm32.hip.h: device
// headers); the engine hands them in as a LayerSizes.
#pragma once
#include "../../include/clair_amd.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace clair {

struct LayerSizes {
    int t_pos, f_in, hid, l3_units, l4_units, l5_units;   // common.hip.h
    int l34_groups, l34_ks, l34_ch;                      // dense.hip.h: the W4 fragments of l3l4_kernel
    int l32_x_shift;                                     // lstm32.hip.h: L32_X_SHIFT
};

// outputs of the four heads: the 21 | 3 | 33 | 33 floats of a packed row, the columns of the head kernels
constexpr int HEAD_SIZE[4] = {CLAIR_GT21, CLAIR_GENOTYPE, CLAIR_INDEL_LEN, CLAIR_INDEL_LEN};

// floats per tensor, by clair_tensor_id
constexpr int64_t TENSOR_COUNT[CLAIR_T_COUNT] = {
    160 * 512, 512, 160 * 512, 512, 384 * 512, 512, 384 * 512, 512, 256 * 33 * 30, 256 * 30,
    7680 * 192, 192, 4 * 192 * 96, 4 * 96, 96 * HEAD_SIZE[0], HEAD_SIZE[0], 96 * HEAD_SIZE[1], HEAD_SIZE[1],
    96 * HEAD_SIZE[2], HEAD_SIZE[2], 96 * HEAD_SIZE[3], HEAD_SIZE[3]};

// host-side 2-way fp16 split (round to nearest even; _Float16 conversions are IEEE on the host compiler too)
inline unsigned short f16_bits(_Float16 h) { unsigned short u; memcpy(&u, &h, 2); return u; }
inline float f16_value(unsigned short u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }
inline void split2_host(float x, unsigned short &hi, unsigned short &lo) {
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    hi = f16_bits(h);
    lo = f16_bits(l);
}

// Factor folded into every LSTM gate column (and bias) so the MFMA result is the exp2 argument of the
// gate's activation (lstm32.hip.h): columns are i | c~ | f | o, 128 each.
inline float gate_scale(int col512) {
    const float L2E = 1.44269504088896340736f;
    return ((col512 >> 7) == 1) ? 2.0f * L2E : -L2E;
}

// Gate-row order of the recurrent kernels (lstm32.hip.h): row rho = 8a + 4h' + c of block b of wave w is
// gate c (i | c~ | f | o) of hidden unit 32w + 8b + 4h' + a, i.e. column c*128 + unit of the reference's [K][512] kernel.
inline int gate_col(int w, int b, int rho) {
    const int a = rho >> 3, hq = (rho >> 2) & 1, c = rho & 3;
    return c * 128 + 32 * w + 8 * b + 4 * hq + a;
}

// Power-of-two image shift of a tensor: puts its largest magnitude into [2^13, 2^14).  A freshly initialised W4 has sigma = 0.011 and a
// trained one may be smaller still, i.e. residuals below the fp16 normal range -- the low plane would keep them to 3e-8 ABSOLUTE
// only (common.hip.h); the kernel that consumes the product multiplies by 2^-shift (exact).
inline int image_shift(float vmax) {
    if (!(vmax > 0.0f) || !std::isfinite(vmax)) return 0;
    int ex = 0;
    (void)std::frexp(vmax, &ex);              // vmax = m * 2^ex, m in [0.5, 1)
    return std::max(-20, std::min(40, 14 - ex));
}
inline float max_abs(const float *v, size_t n, float vmax = 0.0f) {
    for (size_t i = 0; i < n; ++i) vmax = std::max(vmax, std::fabs(v[i]));
    return vmax;
}

// An image of MFMA operand fragments as a 2-way fp16 split: [frag][plane][lane][8], plane 0 = fp16(v), plane 1 = fp16(v - plane 0);
// zero where nothing is put.  The packers below say which fragment is which; this is the only place that knows the rest.
struct SplitImage {
    std::vector<unsigned short> data;
    explicit SplitImage(size_t frags) : data(frags * 2 * 64 * 8, 0) {}
    void put(size_t frag, int lane, int j, float v) {
        unsigned short hi, lo;
        split2_host(v, hi, lo);
        const size_t base = ((frag * 2) * 64 + lane) * 8 + j;
        data[base] = hi;
        data[base + 64 * 8] = lo;
    }
};

// gate-scaled bias of both directions in gate-row order: [dir][wave][b][rho]  (= [..][a][h'][c] accumulator quads)
inline std::vector<float> pack_bias32(const std::vector<float> &fb, const std::vector<float> &bb) {
    std::vector<float> out(1024);
    for (int d = 0; d < 2; ++d)
        for (int w = 0; w < 4; ++w)
            for (int b = 0; b < 4; ++b)
                for (int rho = 0; rho < 32; ++rho) {
                    const int col = gate_col(w, b, rho);
                    out[((d * 4 + w) * 4 + b) * 32 + rho] = (d ? bb : fb)[col] * gate_scale(col);
                }
    return out;
}

// fp16 2-way split A fragments of W^T for v_mfma_f32_32x32x16_f16: [dir][wave][b][kk][plane][lane][8]:
// W[k0 + 16*kk + 8*(lane/32) + j][gate_col(w, b, lane%32)] * gate_scale, kk < nkk
// `pow2` is an extra power-of-two factor on the image (exact): see L32_X_SHIFT in lstm32.hip.h
inline std::vector<unsigned short> pack_wt32(const std::vector<float> &fw, const std::vector<float> &bw, int k0, int nkk, float pow2 = 1.0f) {
    SplitImage out((size_t)2 * 4 * 4 * nkk);
    for (int d = 0; d < 2; ++d) {
        const std::vector<float> &src = d ? bw : fw;
        for (int w = 0; w < 4; ++w)
            for (int b = 0; b < 4; ++b)
                for (int kk = 0; kk < nkk; ++kk)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int col = gate_col(w, b, lane & 31), k = k0 + 16 * kk + 8 * (lane >> 5) + j;
                            out.put(((size_t)(d * 4 + w) * 4 + b) * nkk + kk, lane, j, src[(size_t)k * 512 + col] * gate_scale(col) * pow2);
                        }
    }
    return out.data;
}

// Wx2^T (gate-scaled, gate-row order) as A fragments of the weight-stationary projection GEMM (gemm_split.hip.h):
// [gate tile][wm][mi][kk][plane][lane][8]
inline std::vector<unsigned short> pack_wx2(const std::vector<float> &fw, const std::vector<float> &bw) {
    SplitImage out((size_t)8 * 2 * 2 * 16);
    for (int gt = 0; gt < 8; ++gt)
        for (int wm = 0; wm < 2; ++wm)
            for (int mi = 0; mi < 2; ++mi)
                for (int kk = 0; kk < 16; ++kk)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int R = gt * 128 + wm * 64 + mi * 32 + (lane & 31), k = 16 * kk + 8 * (lane >> 5) + j;
                            const int d = R >> 9, col = gate_col((R >> 7) & 3, (R >> 5) & 3, R & 31);
                            out.put((((size_t)gt * 2 + wm) * 2 + mi) * 16 + kk, lane, j, (d ? bw : fw)[(size_t)k * 512 + col] * gate_scale(col));
                        }
    return out.data;
}

// L3 A fragments (dense.hip.h: l3l4_kernel): (W3[c]^T | b3[c]) * 2^shift as fp16 split, [c][kk][plane][lane][8]: row u = lane%32,
// k = 16kk + 8(lane/32) + j: t for k < 33, the bias at k = 33 (the activation operand carries 1.0 there), zero beyond and for u >= 30
inline std::vector<unsigned short> pack_w3(const LayerSizes &L, const std::vector<float> &W3, const std::vector<float> &b3, int &shift) {
    shift = image_shift(max_abs(b3.data(), b3.size(), max_abs(W3.data(), W3.size())));
    const float pow2 = std::ldexp(1.0f, shift);
    SplitImage out((size_t)256 * 3);
    for (int c = 0; c < 256; ++c)
        for (int kk = 0; kk < 3; ++kk)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int u = lane & 31, k = 16 * kk + 8 * (lane >> 5) + j;
                    float v = 0.0f;
                    if (u < L.l3_units && k < L.t_pos) v = W3[((size_t)c * L.t_pos + k) * L.l3_units + u];
                    else if (u < L.l3_units && k == L.t_pos) v = b3[(size_t)c * L.l3_units + u];
                    out.put((size_t)c * 3 + kk, lane, j, v * pow2);
                }
    return out.data;
}

// W4 as fp16 split B fragments of the fused L3/L4 kernel (dense.hip.h): [cg][ks][nb][plane][lane][8]: row (2ks + lane/32)*256 + cg*8 + j
// of W4 * 2^shift, column nb*32 + lane%32; the kernel that reduces the split-K partials multiplies by 2^-shift.
inline std::vector<unsigned short> pack_w4(const LayerSizes &L, const std::vector<float> &W4, int &shift) {
    shift = image_shift(max_abs(W4.data(), W4.size()));
    const float pow2 = std::ldexp(1.0f, shift);
    SplitImage out((size_t)L.l34_groups * L.l34_ks * 6);
    for (int cg = 0; cg < L.l34_groups; ++cg)
        for (int ks = 0; ks < L.l34_ks; ++ks)
            for (int nb = 0; nb < 6; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int u = 2 * ks + (lane >> 5), col = nb * 32 + (lane & 31);
                        out.put(((size_t)cg * L.l34_ks + ks) * 6 + nb, lane, j, W4[((size_t)u * 256 + cg * L.l34_ch + j) * L.l4_units + col] * pow2);
                    }
    return out.data;
}

// tail A fragments (dense.hip.h: tail_kernel): W5_k^T as fp16 split, [branch][ks][nb][plane][lane][8], each branch shifted by its own
// power of two
inline std::vector<unsigned short> pack_w5(const LayerSizes &L, const std::vector<float> &W5all, int (&shift)[4]) {
    SplitImage out((size_t)4 * 12 * 3);
    for (int k5 = 0; k5 < 4; ++k5) {
        const float *W5 = W5all.data() + (size_t)k5 * L.l4_units * L.l5_units;
        shift[k5] = image_shift(max_abs(W5, (size_t)L.l4_units * L.l5_units));
        const float p5 = std::ldexp(1.0f, shift[k5]);
        for (int ks = 0; ks < 12; ++ks)
            for (int nb = 0; nb < 3; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int k = 16 * ks + 8 * (lane >> 5) + j, n = nb * 32 + (lane & 31);
                        out.put(((size_t)k5 * 12 + ks) * 3 + nb, lane, j, W5[(size_t)k * L.l5_units + n] * p5);
                    }
    }
    return out.data;
}

// the same for the heads: Wh_k^T, [head][ks][nb][plane][lane][8], columns beyond the head's size zero; their biases as [head][64]
inline std::vector<unsigned short> pack_wh(const std::vector<float> *tensors, int (&shift)[4], std::vector<float> &bh) {
    SplitImage out((size_t)4 * 6 * 2);
    bh.assign(4 * 64, 0.0f);
    for (int k5 = 0; k5 < 4; ++k5) {
        const std::vector<float> &Wh = tensors[CLAIR_T_HEAD_GT21_KERNEL + 2 * k5], &b = tensors[CLAIR_T_HEAD_GT21_BIAS + 2 * k5];
        shift[k5] = image_shift(max_abs(Wh.data(), Wh.size()));
        const float ph = std::ldexp(1.0f, shift[k5]);
        for (int ks = 0; ks < 6; ++ks)
            for (int nb = 0; nb < 2; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int k = 16 * ks + 8 * (lane >> 5) + j, c = nb * 32 + (lane & 31);
                        if (c < HEAD_SIZE[k5]) out.put(((size_t)k5 * 6 + ks) * 2 + nb, lane, j, Wh[(size_t)k * HEAD_SIZE[k5] + c] * ph);
                    }
        for (int j = 0; j < HEAD_SIZE[k5]; ++j) bh[k5 * 64 + j] = b[j];
    }
    return out.data;
}

// Everything clair_finalize_weights uploads, and the shifts the launches undo.
struct WeightImages {
    std::vector<float> bx1, bx2;                 // gate-scaled biases [2][512] of the two LSTM layers
    std::vector<unsigned short> wh1s, wh2s, wx1s;   // recurrent weights of both layers and layer 1's x part (lstm32.hip.h)
    std::vector<unsigned short> wx2s;            // layer 2's x part (gemm_split.hip.h)
    std::vector<unsigned short> w3s, w4s;        // dense.hip.h: l3l4_kernel
    std::vector<unsigned short> w5s, whs;        // dense.hip.h: tail_kernel
    std::vector<float> b4, b5, bh;
    int w3_shift = 0, w4_shift = 0, w5_shift[4] = {0, 0, 0, 0}, wh_shift[4] = {0, 0, 0, 0};
};

// T: the CLAIR_T_COUNT tensors, each of its TENSOR_COUNT
inline WeightImages build_weight_images(const LayerSizes &L, const std::vector<float> *T) {
    WeightImages m;
    m.bx1 = pack_bias32(T[CLAIR_T_LSTM1_FW_BIAS], T[CLAIR_T_LSTM1_BW_BIAS]);
    m.bx2 = pack_bias32(T[CLAIR_T_LSTM2_FW_BIAS], T[CLAIR_T_LSTM2_BW_BIAS]);
    m.wx2s = pack_wx2(T[CLAIR_T_LSTM2_FW_KERNEL], T[CLAIR_T_LSTM2_BW_KERNEL]);
    m.wh1s = pack_wt32(T[CLAIR_T_LSTM1_FW_KERNEL], T[CLAIR_T_LSTM1_BW_KERNEL], L.f_in, 8);
    m.wh2s = pack_wt32(T[CLAIR_T_LSTM2_FW_KERNEL], T[CLAIR_T_LSTM2_BW_KERNEL], 2 * L.hid, 8);
    m.wx1s = pack_wt32(T[CLAIR_T_LSTM1_FW_KERNEL], T[CLAIR_T_LSTM1_BW_KERNEL], 0, 2, (float)(1 << L.l32_x_shift));
    m.w3s = pack_w3(L, T[CLAIR_T_L3_KERNEL], T[CLAIR_T_L3_BIAS], m.w3_shift);
    m.w4s = pack_w4(L, T[CLAIR_T_L4_KERNEL], m.w4_shift);
    m.b4 = T[CLAIR_T_L4_BIAS];
    m.w5s = pack_w5(L, T[CLAIR_T_L5_KERNEL], m.w5_shift);
    m.b5 = T[CLAIR_T_L5_BIAS];
    m.whs = pack_wh(T, m.wh_shift, m.bh);
    return m;
}

}  // namespace clair
