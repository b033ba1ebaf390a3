// The VALU convs: every forward and data-gradient conv the implicit GEMM does not take -- the 2-channel colour 1x1 convs (networks.py:98-105,
// 233-240), the 1-channel minibatch-stddev plane (networks.py:174-176) and the generic direct conv -- and run_thin, which launches what
// thin_route (conv_thin_route.h) chose and decides nothing.  (Their weight gradients: conv_wgrad.hip.)
#include "conv_device.h"
#include "conv_thin_route.h"

namespace gs {

// Bias and activation behind the kernels that take the activation as a run-time argument (direct, single): the arithmetic of gs_bias_act_fwd
// (elementwise.hip), on the fp32 sum.  As a pass behind the kernel the same two steps read a bf16 result back: the sum was rounded to bf16
// BEFORE the bias went in, and where sum and bias cancel that rounding is many times the size of the result's own.
__device__ inline float bias_act_rt(float v, const float* __restrict__ bias, int oc, int act) {
    if (bias) v += bias[oc];
    if (act == GS_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
    if (act == GS_ACT_TANH) v = tanhf(v);
    return v;
}

// ------------------------------------------------------------------------- direct gather conv
// y[n][oy][ox][oc0..oc0+OCV) = act(alpha * sum_{tap,ic} x[n][iy][ix][ic] * wp[tap][oc][ic] + bias[oc])   (wp fp32; bias optional, OC floats)
template <typename T, int OCV, int VEC>
__global__ void conv_direct_kernel(const T* __restrict__ x, const float* __restrict__ wp, T* __restrict__ y, int mode,
                                   int ks, int N, int Hi, int Wi, int IC, int OC, int Ho, int Wo, float alpha, const float* __restrict__ bias, int act) {
    const int ngrp = OC / OCV;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)N * Ho * Wo * ngrp;
    if (idx >= total) return;
    const int g = idx % ngrp;
    long pix = idx / ngrp;
    const int ox = pix % Wo;
    pix /= Wo;
    const int oy = pix % Ho;
    const int n = pix / Ho;
    const int oc = g * OCV;
    float acc[OCV];
#pragma unroll
    for (int v = 0; v < OCV; ++v) acc[v] = 0.f;
    for (int ky = 0; ky < ks; ++ky) {
        int iy;
        if (!tap_input(mode, ks, oy, ky, Hi, iy)) continue;
        for (int kx = 0; kx < ks; ++kx) {
            int ix;
            if (!tap_input(mode, ks, ox, kx, Wi, ix)) continue;
            const T* xp = x + (((long)n * Hi + iy) * Wi + ix) * IC;
            const float* wr = wp + ((long)(ky * ks + kx) * OC + oc) * IC;
            if (VEC == 4) {
                for (int ic = 0; ic < IC; ic += 4) {
                    float xv[4];
                    ld4(xp + ic, xv);
#pragma unroll
                    for (int v = 0; v < OCV; ++v) {
                        const float4 wv = *reinterpret_cast<const float4*>(wr + (long)v * IC + ic);
                        acc[v] += xv[0] * wv.x + xv[1] * wv.y + xv[2] * wv.z + xv[3] * wv.w;
                    }
                }
            } else {
                for (int ic = 0; ic < IC; ++ic) {
                    const float xv = DT<T>::ld(xp + ic);
#pragma unroll
                    for (int v = 0; v < OCV; ++v) acc[v] += xv * wr[(long)v * IC + ic];
                }
            }
        }
    }
    T* yp = y + (((long)n * Ho + oy) * Wo + ox) * OC + oc;
    if (OCV == 4) {
        float o[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) o[v] = bias_act_rt(acc[v < OCV ? v : 0] * alpha, bias, oc + (v < OCV ? v : 0), act);
        st4(yp, o);
    } else {
#pragma unroll
        for (int v = 0; v < OCV; ++v) DT<T>::st(yp + v, bias_act_rt(acc[v] * alpha, bias, oc + v, act));
    }
}

// ------------------------------------------------------------------ thin 1x1 convolutions
// The colour blocks (ops.py:237-243 with a [1,1,C,2] / [1,1,2,C] kernel) are pure streaming: 64 bytes in and 4 out per
// pixel, or the reverse.  One lane per 16 bytes of the wide side keeps every access coalesced; the bias / activation
// epilogue of the block is applied in the same pass.
// The activation of a streaming kernel is a TEMPLATE parameter: as a run-time argument the three-way choice (tanhf's own branches
// included) was compiled into the pixel loop once per output VALUE -- ~6 scalar branches per value in thin_expand_kernel's hot loop
// (hipcc -S), 23 us for the 67 MB of the top-level colour block where the write rate allows ~14.
template <int ACT> __device__ inline float thin_act(float v) {
    if constexpr (ACT == GS_ACT_LRELU) return fmaxf(v, 0.2f * v);
    else if constexpr (ACT == GS_ACT_TANH) return fast_tanh(v);
    else return v;
}
// few -> many channels: y[p][oc] = act(alpha * sum_ic x[p][ic] wp[oc][ic] + bias[oc]),  IC <= 4, OC % Wide::N == 0, 256 % (OC / N) == 0.
// A thread keeps its Wide::N output channels (weights + bias in registers) and strides over pixels.
template <typename T, int IC, int ACT, bool MASKED>
// `mask` (MASKED, y's shape): y *= mask_act'(.) through that activation output -- the second-order pass of the R1 penalty runs the colour
// block forward on a cotangent and the next node's first step is that multiplication (gs_conv_fwd_mask)
__global__ __launch_bounds__(256) void thin_expand_kernel(const T* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                                                          T* __restrict__ y, long P, int OC, float alpha,
                                                          const T* __restrict__ mask = nullptr, int mask_act = 0, unsigned* __restrict__ bits = nullptr) {
    // `bits` (bf16 leaky relu, OC % 32 == 0): the sign words of the result behind it (include/gansynth_hip.h, GS_ACT_WRITE_BITS) -- a lane's 8 channels
    // are one byte of the pixel's word, the four lanes of a 32-channel tile are a DPP quad
    constexpr int WN = Wide<T>::N;
    const int groups = OC / WN;
    const int oc0 = (threadIdx.x % groups) * WN;
    float wr[WN][IC], br[WN];
    {   // this lane's WN x IC weights and WN biases: contiguous floats, fetched as 16-byte vectors (a scalar load each made the prologue of
        // a block cost as much as its pixels: 22.8 us at 4096 blocks, 51 us at 16384, scripts/bench_thin.py)
        typedef float f4_t __attribute__((ext_vector_type(4)));
        float flat[WN * IC];
        if constexpr ((WN * IC) % 4 == 0) {
#pragma unroll
            for (int q = 0; q < WN * IC / 4; ++q) {
                const f4_t t = *reinterpret_cast<const f4_t*>(wp + (long)oc0 * IC + 4 * q);
                flat[4 * q] = t.x; flat[4 * q + 1] = t.y; flat[4 * q + 2] = t.z; flat[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < WN * IC; ++q) flat[q] = wp[(long)oc0 * IC + q];
        }
#pragma unroll
        for (int v = 0; v < WN; ++v)
#pragma unroll
            for (int i = 0; i < IC; ++i) wr[v][i] = flat[v * IC + i] * alpha;
#pragma unroll
        for (int q = 0; q < WN / 4; ++q) {
            f4_t t = {0.f, 0.f, 0.f, 0.f};
            if (bias) t = *reinterpret_cast<const f4_t*>(bias + oc0 + 4 * q);
            br[4 * q] = t.x; br[4 * q + 1] = t.y; br[4 * q + 2] = t.z; br[4 * q + 3] = t.w;
        }
    }
    const long ppb = 256 / groups;  // pixels per block pass
    const long stride = (long)gridDim.x * ppb;
    long pix = (long)blockIdx.x * ppb + threadIdx.x / groups;
    auto one = [&](long px, const float* xv) __attribute__((always_inline)) {
        float o[WN];
        // two output channels per instruction (v_pk_fma_f32 / v_pk_mul_f32): the kernel's time IS its VALU count -- 50 instructions per 16
        // bytes stored with scalar arithmetic (hipcc split every multiply-add into a packed multiply and an add), ~30 like this
        typedef float f2_t __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int v = 0; v < WN; v += 2) {
            f2_t a = {br[v], br[v + 1]};
#pragma unroll
            for (int i = 0; i < IC; ++i) {
                const f2_t xx = {xv[i], xv[i]}, ww = {wr[v][i], wr[v + 1][i]};
                a = __builtin_elementwise_fma(xx, ww, a);
            }
            if constexpr (ACT == GS_ACT_LRELU) {
                const f2_t t = a * 0.2f;
                o[v] = fmaxf(a.x, t.x);
                o[v + 1] = fmaxf(a.y, t.y);
            } else {
                o[v] = thin_act<ACT>(a.x);
                o[v + 1] = thin_act<ACT>(a.y);
            }
        }
        if constexpr (MASKED) {
            float mv[WN];
            ld_wide<T>(mask + px * OC + oc0, mv);
#pragma unroll
            for (int v = 0; v < WN; ++v) o[v] *= mask_act == GS_ACT_LRELU ? (mv[v] > 0.f ? 1.f : 0.2f) : (mask_act == GS_ACT_TANH ? 1.f - mv[v] * mv[v] : 1.f);
        }
        if constexpr (ACT == GS_ACT_LRELU && !MASKED && sizeof(T) == 2) {
            if (bits) {
                uint4 v;
                v.x = pack_bf16x2(o[0], o[1]); v.y = pack_bf16x2(o[2], o[3]); v.z = pack_bf16x2(o[4], o[5]); v.w = pack_bf16x2(o[6], o[7]);
                *reinterpret_cast<uint4*>(y + px * OC + oc0) = v;
                const unsigned b8 = ((int)(v.x << 16) > 0 ? 1u : 0u) | ((int)v.x >= 0x10000 ? 2u : 0u) | ((int)(v.y << 16) > 0 ? 4u : 0u) | ((int)v.y >= 0x10000 ? 8u : 0u) |
                                    ((int)(v.z << 16) > 0 ? 16u : 0u) | ((int)v.z >= 0x10000 ? 32u : 0u) | ((int)(v.w << 16) > 0 ? 64u : 0u) | ((int)v.w >= 0x10000 ? 128u : 0u);
                const int piece = (oc0 >> 3) & 3;   // 16-byte piece of the tile: channels 8 piece .. -> byte 2 (piece & 1) + (piece >> 1) of the word
                unsigned word = b8 << (8 * (2 * (piece & 1) + (piece >> 1)));
                word |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)word, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
                word |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)word, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
                if (piece == 0) bits[(px * OC + oc0) >> 5] = word;
                return;
            }
        }
        st_wide<T>(y + px * OC + oc0, o);
    };
    auto ldpix = [&](long px, float* xv) __attribute__((always_inline)) {
        if constexpr (IC == 2 && sizeof(T) == 2) {   // both colour channels of a pixel in one 4-byte load
            const unsigned u = *reinterpret_cast<const unsigned*>(x + px * 2);
            xv[0] = __uint_as_float(u << 16);
            xv[1] = __uint_as_float(u & 0xffff0000u);
        } else {
#pragma unroll
            for (int i = 0; i < IC; ++i) xv[i] = DT<T>::ld(x + px * IC + i);
        }
    };
    for (; pix + 3 * stride < P; pix += 4 * stride) {   // four pixels per trip (loads first)
        float xv[4][IC];
#pragma unroll
        for (int k = 0; k < 4; ++k) ldpix(pix + k * stride, xv[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) one(pix + k * stride, xv[k]);
    }
    for (; pix < P; pix += stride) {
        float xv[IC];
        ldpix(pix, xv);
        one(pix, xv);
    }
}

// The same map as a DATA GRADIENT continued through the pixel norm and activation of the block that produced the conv's input
// (gs_conv_bwd_data_pnbwd for the colour block, networks.py:98-104): g[p][oc] = alpha * sum_ic x[p][ic] wp[oc][ic] is the gradient
// w.r.t. pixel_norm(z); out = (r (g - z r^2 mean_c(z g)) + addend) * act'(z), r = rsqrt(mean_c z^2 + eps).  The OC / Wide::N lanes of
// a pixel are neighbours in the wave: two xor-shuffle folds give the pixel's sums.  One pass instead of thin_expand + a 4-tensor norm pass.
template <typename T, int IC>
__global__ __launch_bounds__(256) void thin_expand_pnbwd_kernel(const T* __restrict__ x, const float* __restrict__ wp, const T* __restrict__ z,
                                                                const T* __restrict__ addend, T* __restrict__ y, long P, int OC, float alpha, float eps, int act) {
    constexpr int WN = Wide<T>::N;
    const int groups = OC / WN;   // a power of two <= 64 dividing 256 (checked by the launcher)
    const int oc0 = (threadIdx.x % groups) * WN;
    float wr[WN][IC];
#pragma unroll
    for (int v = 0; v < WN; ++v)
#pragma unroll
        for (int i = 0; i < IC; ++i) wr[v][i] = wp[(long)(oc0 + v) * IC + i] * alpha;
    const long ppb = 256 / groups;
    const long stride = (long)gridDim.x * ppb;
    const long npass = (P + stride - 1) / stride;   // same trip count for every lane (shuffles)
    const float inv_c = 1.f / (float)OC;
    for (long k = 0; k < npass; ++k) {
        const long pix = (long)blockIdx.x * ppb + threadIdx.x / groups + k * stride;
        const long px = pix < P ? pix : P - 1;      // (clamped: loads and shuffles stay unconditional)
        float xv[IC], zv[WN], av[WN], g[WN];
        if constexpr (IC == 2 && sizeof(T) == 2) {
            const unsigned u = *reinterpret_cast<const unsigned*>(x + px * 2);
            xv[0] = __uint_as_float(u << 16);
            xv[1] = __uint_as_float(u & 0xffff0000u);
        } else {
#pragma unroll
            for (int i = 0; i < IC; ++i) xv[i] = DT<T>::ld(x + px * IC + i);
        }
        ld_wide<T>(z + px * OC + oc0, zv);
        if (addend) ld_wide<T>(addend + px * OC + oc0, av);
        float ssq = 0.f, szg = 0.f;
#pragma unroll
        for (int v = 0; v < WN; ++v) {
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < IC; ++i) a += xv[i] * wr[v][i];
            g[v] = a;
            ssq += zv[v] * zv[v];
            szg += zv[v] * a;
        }
        ssq = group_sum(ssq, groups);
        szg = group_sum(szg, groups);
        const float r = rsqrtf(ssq * inv_c + eps);
        const float m = szg * inv_c * r * r;
        float out[WN];
#pragma unroll
        for (int v = 0; v < WN; ++v) {
            float t = r * (g[v] - zv[v] * m);
            if (addend) t += av[v];
            out[v] = act == GS_ACT_LRELU ? (zv[v] > 0.f ? t : 0.2f * t) : t;
        }
        if (pix < P) st_wide<T>(y + pix * OC + oc0, out);
    }
}

// many -> few channels: a pixel is read by L = IC / Wide::N lanes (a power of two <= 64), partial dots are folded with
// xor-shuffles, lane 0 of the group writes the OC <= 4 results.  Weights stay in registers across the pixel loop.
// LC: the lanes per pixel as a compile-time constant (4: the 32-channel bf16 colour block; 8: 64 bf16 / 32 fp32 channels; 0: any power of
// two, run-time) -- with a run-time lane count the folds are loops of ds_bpermute round trips through the LDS pipe, with a constant one
// they unroll into DPP moves.
template <typename T, int OC, int ACT, int LC>
__global__ __launch_bounds__(256) void thin_reduce_kernel(const T* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                                                          T* __restrict__ y, long P, int IC, float alpha) {
    constexpr int WN = Wide<T>::N;
    const int L = LC ? LC : IC / WN;
    const int l = threadIdx.x % L;
    float wr[OC][WN];
#pragma unroll
    for (int v = 0; v < OC; ++v)
#pragma unroll
        for (int i = 0; i < WN; ++i) wr[v][i] = wp[v * IC + l * WN + i] * alpha;
    const long ppb = 256 / L;
    const long npass = (P + (long)gridDim.x * ppb - 1) / ((long)gridDim.x * ppb);  // same trip count for every lane (shuffles)
    float bv[OC];
#pragma unroll
    for (int v = 0; v < OC; ++v) bv[v] = bias ? bias[v] : 0.f;
    auto fold = [&](float* a) __attribute__((always_inline)) {
        // VALU only (DPP inside a row, permlane swaps across rows; gs_common.h: a __shfl_xor is a ds_bpermute whatever its offset)
#pragma unroll
        for (int v = 0; v < OC; ++v) a[v] = group_sum(a[v], LC != 0 ? LC : L);
    };
    auto finish = [&](long pix, float* a) __attribute__((always_inline)) {
        fold(a);
        if (pix < P && l == 0) {
            if constexpr (OC == 2 && sizeof(T) == 2) {   // both colour channels of a pixel in one 4-byte store
                *reinterpret_cast<unsigned*>(y + pix * 2) = pack_bf16x2(thin_act<ACT>(a[0] + bv[0]), thin_act<ACT>(a[1] + bv[1]));
            } else {
#pragma unroll
                for (int v = 0; v < OC; ++v) DT<T>::st(y + pix * OC + v, thin_act<ACT>(a[v] + bv[v]));
            }
        }
    };
    constexpr int U = 4;   // pixels per trip: their loads go out together
    long k = 0;
    for (; k + U <= npass; k += U) {
        float xv[U][WN], a[U][OC];
        long pix[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pix[u] = ((k + u) * gridDim.x + blockIdx.x) * ppb + threadIdx.x / L;
            ld_wide<T>(x + (pix[u] < P ? pix[u] : 0) * IC + l * WN, xv[u]);   // (clamped: the loads stay unconditional)
        }
        if constexpr (LC == U) {
            // after the folds each of the pixel's LC lanes holds the sums of all U pixels of the trip: lane l finishes pixel l -- bias,
            // activation (a tanh on the generator's colour block) and the store run ONCE per lane instead of U times on a quarter of them
            float mine[OC];
            long mypix = pix[0];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int v = 0; v < OC; ++v) {
                    a[u][v] = 0.f;
#pragma unroll
                    for (int i = 0; i < WN; ++i) a[u][v] += xv[u][i] * wr[v][i];
                }
                fold(a[u]);
#pragma unroll
                for (int v = 0; v < OC; ++v) mine[v] = (u == 0 || l == u) ? a[u][v] : mine[v];
                mypix = l == u ? pix[u] : mypix;
            }
            if (mypix < P) {
                if constexpr (OC == 2 && sizeof(T) == 2) {
                    *reinterpret_cast<unsigned*>(y + mypix * 2) = pack_bf16x2(thin_act<ACT>(mine[0] + bv[0]), thin_act<ACT>(mine[1] + bv[1]));
                } else {
#pragma unroll
                    for (int v = 0; v < OC; ++v) DT<T>::st(y + mypix * OC + v, thin_act<ACT>(mine[v] + bv[v]));
                }
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int v = 0; v < OC; ++v) {
                a[u][v] = 0.f;
#pragma unroll
                for (int i = 0; i < WN; ++i) a[u][v] += xv[u][i] * wr[v][i];
            }
            finish(pix[u], a[u]);
        }
    }
    for (; k < npass; ++k) {
        const long pix = (k * gridDim.x + blockIdx.x) * ppb + threadIdx.x / L;
        float a[OC];
#pragma unroll
        for (int v = 0; v < OC; ++v) a[v] = 0.f;
        if (pix < P) {
            float xv[WN];
            ld_wide<T>(x + pix * IC + l * WN, xv);
#pragma unroll
            for (int v = 0; v < OC; ++v)
#pragma unroll
                for (int i = 0; i < WN; ++i) a[v] += xv[i] * wr[v][i];
        }
        finish(pix, a);
    }
}

// one output channel, many input channels, any tap geometry (the data gradient of the minibatch-stddev plane of the last
// discriminator block): a wave per output pixel, lanes over the input channels.
template <typename T>
__global__ __launch_bounds__(256) void thin_single_kernel(const T* __restrict__ x, const float* __restrict__ wp, T* __restrict__ y, int mode,
                                                          int ks, int N, int Hi, int Wi, int IC, int Ho, int Wo, float alpha,
                                                          const float* __restrict__ bias, int act) {
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pix >= (long)N * Ho * Wo) return;
    const int ox = pix % Wo;
    const int oy = (pix / Wo) % Ho;
    const int n = pix / ((long)Wo * Ho);
    float a = 0.f;
    for (int ky = 0; ky < ks; ++ky) {
        int iy;
        if (!tap_input(mode, ks, oy, ky, Hi, iy)) continue;
        for (int kx = 0; kx < ks; ++kx) {
            int ix;
            if (!tap_input(mode, ks, ox, kx, Wi, ix)) continue;
            const T* xp = x + (((long)n * Hi + iy) * Wi + ix) * IC;
            const float* wr = wp + (long)(ky * ks + kx) * IC;
            for (int ic = lane; ic < IC; ic += 64) a += DT<T>::ld(xp + ic) * wr[ic];
        }
    }
    a = wave_sum(a);
    if (lane == 0) DT<T>::st(y + pix, bias_act_rt(a * alpha, bias, 0, act));
}

// the same for 3x3 kernels with IC a multiple of 256: a lane owns 4 consecutive channels per 256-channel block and ALL its loads (9 taps x
// IC / 256 blocks, inputs and weights) are issued before the first multiply -- the generic kernel above walks 9 x IC / 64 dependent
// load pairs (11.6 us for the 256-channel stddev-plane gradient at 2 x 16: a pure latency chain)
template <typename T, int NB>
__global__ __launch_bounds__(256) void thin_single3_kernel(const T* __restrict__ x, const float* __restrict__ wp, T* __restrict__ y, int mode,
                                                           int N, int Hi, int Wi, int Ho, int Wo, float alpha, const float* __restrict__ bias, int act) {
    constexpr int IC = 256 * NB;
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pix >= (long)N * Ho * Wo) return;
    const int ox = pix % Wo;
    const int oy = (pix / Wo) % Ho;
    const int n = pix / ((long)Wo * Ho);
    float xv[9][NB][4];
    float4 wv[9][NB];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t % 3;
        int iy, ix;
        const bool oky = tap_input(mode, 3, oy, ky, Hi, iy), okx = tap_input(mode, 3, ox, kx, Wi, ix);
        const bool ok = oky && okx;
        const T* xp = x + (((long)n * Hi + (ok ? iy : 0)) * Wi + (ok ? ix : 0)) * IC + 4 * lane;   // (clamped: the loads stay unconditional)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            ld4(xp + 256 * b, xv[t][b]);
            wv[t][b] = ok ? *reinterpret_cast<const float4*>(wp + (long)t * IC + 256 * b + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) a += xv[t][b][0] * wv[t][b].x + xv[t][b][1] * wv[t][b].y + xv[t][b][2] * wv[t][b].z + xv[t][b][3] * wv[t][b].w;
    a = wave_sum(a);
    if (lane == 0) DT<T>::st(y + pix, bias_act_rt(a * alpha, bias, 0, act));
}

// ------------------------------------------------------------------------------- the launcher
// One launch: the kernel, template arguments and grid of the route, the operands of the call.  The epilogue operands go in only where the route
// says the kernel takes them.
template <typename T>
static bool launch_thin(const ThinRoute& r, const ThinArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)r.grid), block(256);
    const T* x = reinterpret_cast<const T*>(a.x);
    T* y = reinterpret_cast<T*>(a.y);
    const float* rt_bias = r.epilogue_fused ? a.bias : nullptr;   // (direct, single: a.act is the norm's activation where the epilogue is not theirs)
    const int rt_act = r.epilogue_fused ? a.act : GS_ACT_NONE;
    switch (r.kernel) {
    case GS_THIN_EXPAND:
        return with_constant<1, 2, 3, 4>(r.C, [&](auto ic) {
            return with_constant<GS_ACT_NONE, GS_ACT_LRELU, GS_ACT_TANH>(r.ACT, [&](auto act) {
                return with_constant<0, 1>(r.MASKED, [&](auto masked) {
                    hipLaunchKernelGGL((thin_expand_kernel<T, decltype(ic)::value, decltype(act)::value, decltype(masked)::value != 0>), grid, block, 0, st, x, a.wp, a.bias, y,
                                       a.P, a.OCk, a.alpha, r.mask_fused ? reinterpret_cast<const T*>(a.mask) : nullptr, a.mask_act, r.bits_fused ? a.bits : nullptr);
                    return true;
                });
            });
        });
    case GS_THIN_REDUCE:
        return with_constant<1, 2, 3, 4>(r.C, [&](auto oc) {
            return with_constant<GS_ACT_NONE, GS_ACT_LRELU, GS_ACT_TANH>(r.ACT, [&](auto act) {
                return with_constant<4, 8, 0>(r.LC, [&](auto lc) {
                    hipLaunchKernelGGL((thin_reduce_kernel<T, decltype(oc)::value, decltype(act)::value, decltype(lc)::value>), grid, block, 0, st, x, a.wp, a.bias, y, a.P, a.ICk,
                                       a.alpha);
                    return true;
                });
            });
        });
    case GS_THIN_EXPAND_PNBWD:
        return with_constant<1, 2, 3, 4>(r.C, [&](auto ic) {
            hipLaunchKernelGGL((thin_expand_pnbwd_kernel<T, decltype(ic)::value>), grid, block, 0, st, x, a.wp, reinterpret_cast<const T*>(a.z), reinterpret_cast<const T*>(a.addend),
                               y, a.P, a.OCk, a.alpha, a.eps, a.act);
            return true;
        });
    case GS_THIN_SINGLE3:
        hipLaunchKernelGGL((thin_single3_kernel<T, 1>), grid, block, 0, st, x, a.wp, y, a.mode, a.N, a.Hi, a.Wi, a.Ho, a.Wo, a.alpha, rt_bias, rt_act);
        return true;
    case GS_THIN_SINGLE:
        hipLaunchKernelGGL((thin_single_kernel<T>), grid, block, 0, st, x, a.wp, y, a.mode, a.ks, a.N, a.Hi, a.Wi, a.ICk, a.Ho, a.Wo, a.alpha, rt_bias, rt_act);
        return true;
    case GS_THIN_DIRECT:
        return with_constant<4, 2, 1>(r.OCV, [&](auto ocv) {
            return with_constant<4, 1>(r.VEC, [&](auto vec) {
                hipLaunchKernelGGL((conv_direct_kernel<T, decltype(ocv)::value, decltype(vec)::value>), grid, block, 0, st, x, a.wp, y, a.mode, a.ks, a.N, a.Hi, a.Wi, a.ICk, a.OCk,
                                   a.Ho, a.Wo, a.alpha, rt_bias, rt_act);
                return true;
            });
        });
    }
    return false;
}

int run_thin(const ThinRoute& r, const ThinArgs& a, hipStream_t st) {
    bool compiled = false;
    GS_DISPATCH_DTYPE(a.dtype, compiled = launch_thin<T>(r, a, st));
    if (!compiled) return fail(GS_ERR_UNSUPPORTED, "conv thin: no instantiation of kernel %d with C=%d ACT=%d MASKED=%d LC=%d OCV=%d VEC=%d", r.kernel, r.C, r.ACT, r.MASKED, r.LC, r.OCV, r.VEC);
    GS_CHECK_LAUNCH();
    return 0;
}
}  // namespace gs
