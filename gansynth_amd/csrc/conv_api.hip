// C-ABI entry points of the conv family + the generic direct (VALU) kernels used for the
// channel counts the MFMA implicit GEMM does not take: the 2-channel colour 1x1 convs
// (networks.py:98-105, 233-240) and the 1-channel minibatch-stddev plane (networks.py:174-176).
#include "conv_shared.h"
#include <utility>
#include <vector>

namespace gs {


// from conv_igemm.hip / conv_wgrad.hip
bool igemm_supported(int ic, int oc, int dtype);
bool igemm_norm_fused(int mode, int N, int Hb, int Wb, int IC, int OC, int dtype, int want);
int igemm_config(int mode, int N, int Hb, int Wb, int IC, int OC, int dtype, int want, int* out);
int igemm_table(int index, int* out);
extern "C" int gs_pixel_norm_bwd_bwd_fused(const void* gg, const void* g, const void* x, void* out, void* out_g, int64_t p, int c, float eps, int pre_act,
                                           int dtype, void* stream);
size_t igemm_prep_bytes(int ic, int oc, int dtype);
int run_igemm(int mode, int variant, const void* x, const float* w_hwio, void* y, int N, int Hi, int Wi, int ICk,
              int OCk, int w_ci, int w_co, int Hb, int Wb, float alpha, const float* bias, int act, int dtype, int w_prepared,
              void* ws, size_t ws_bytes, hipStream_t st, const void* mask = nullptr, int mask_act = 0, void* y2 = nullptr, float pn_eps = 0.f,
              const void* addend = nullptr, int normbwd = 0);
extern "C" int gs_pixel_norm_bwd_fused(const void* g, const void* x, const void* addend, void* gx, int64_t p, int c, float eps, int pre_act, int post_act, int dtype,
                                       void* stream);
size_t wgrad_mfma_bytes(int mode, int dtype, int N, int Hb, int Wb, int IC, int OC);
int run_wgrad_mfma(int mode, const WgradSrcs& srcs, int nsrc, float* gw, float* gb, int N, int Hi, int Wi, int IC, int OC, int Hb,
                   int Wb, float alpha, int transpose, int accumulate, int dtype, void* ws, size_t ws_bytes, hipStream_t st,
                   GsWgradReduce* defer = nullptr);
void wgrad_sk_job_geometry(int mode, int N, SkJob& q);
void wgrad_sk_plan(int mode, SkGroup& g);
size_t wgrad_sk_bytes(const SkGroup& g);
int run_wgrad_sk(int mode, const SkGroup& g, void* ws, size_t ws_bytes, hipStream_t st);

// ------------------------------------------------------------------------- direct gather conv
// y[n][oy][ox][oc0..oc0+OCV) = alpha * sum_{tap,ic} x[n][iy][ix][ic] * wp[tap][oc][ic]   (wp fp32)
template <typename T, int OCV, int VEC>
__global__ void conv_direct_kernel(const T* __restrict__ x, const float* __restrict__ wp, T* __restrict__ y, int mode,
                                   int ks, int N, int Hi, int Wi, int IC, int OC, int Ho, int Wo, float alpha) {
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
        if (mode == MODE_S1) iy = oy + ky - (ks >> 1);
        else if (mode == MODE_S2) iy = 2 * oy + ky;
        else { const int d = oy - ky; if (d < 0 || (d & 1)) continue; iy = d >> 1; }
        if (iy < 0 || iy >= Hi) continue;
        for (int kx = 0; kx < ks; ++kx) {
            int ix;
            if (mode == MODE_S1) ix = ox + kx - (ks >> 1);
            else if (mode == MODE_S2) ix = 2 * ox + kx;
            else { const int d = ox - kx; if (d < 0 || (d & 1)) continue; ix = d >> 1; }
            if (ix < 0 || ix >= Wi) continue;
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
        for (int v = 0; v < 4; ++v) o[v] = acc[v < OCV ? v : 0] * alpha;
        st4(yp, o);
    } else {
#pragma unroll
        for (int v = 0; v < OCV; ++v) DT<T>::st(yp + v, acc[v] * alpha);
    }
}

template <typename T>
static int launch_direct(const T* x, const float* wp, T* y, int mode, int ks, int N, int Hi, int Wi, int IC, int OC,
                         int Ho, int Wo, float alpha, hipStream_t st) {
    const int ocv = OC % 4 == 0 ? 4 : (OC % 2 == 0 ? 2 : 1);
    const int vec = IC % 4 == 0 ? 4 : 1;
    const long total = (long)N * Ho * Wo * (OC / ocv);
    dim3 grid(cdiv(total, 256)), block(256);
#define GS_DL(OCVV, VECV)                                                                                              \
    hipLaunchKernelGGL((conv_direct_kernel<T, OCVV, VECV>), grid, block, 0, st, x, wp, y, mode, ks, N, Hi, Wi, IC, OC, Ho, \
                       Wo, alpha)
    if (ocv == 4 && vec == 4) GS_DL(4, 4);
    else if (ocv == 4) GS_DL(4, 1);
    else if (ocv == 2 && vec == 4) GS_DL(2, 4);
    else if (ocv == 2) GS_DL(2, 1);
    else if (vec == 4) GS_DL(1, 4);
    else GS_DL(1, 1);
#undef GS_DL
    GS_CHECK_LAUNCH();
    return 0;
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
static bool thin_expand_pnbwd_ok(int ks, int ICk, int OCk, int dtype) {
    const int wn = dtype == GS_F32 ? 4 : 8;
    if (ks != 1 || ICk < 1 || ICk > 4 || OCk % wn != 0) return false;
    const int groups = OCk / wn;
    return groups >= 1 && groups <= 64 && (groups & (groups - 1)) == 0;
}
// x: the thin gradient [P][ICk], wp: fp32 [OCk][ICk] (bwd-data layout of the 1x1 kernel), z / addend / y: [P][OCk]
static int run_thin_expand_pnbwd(const void* x, const float* wp, const void* z, const void* addend, void* y, long P, int ICk, int OCk, float alpha, float eps, int act,
                                 int dtype, hipStream_t st) {
    const int wn = dtype == GS_F32 ? 4 : 8;
    long nb = cdiv(P * (OCk / wn), 256);
    if (nb > 4096) nb = 4096;
    const unsigned grid = (unsigned)nb;
#define GS_TEP(TT, ICV) hipLaunchKernelGGL((thin_expand_pnbwd_kernel<TT, ICV>), dim3(grid), dim3(256), 0, st, (const TT*)x, wp, (const TT*)z, (const TT*)addend, (TT*)y, P, OCk, alpha, eps, act)
#define GS_TEP_ALL(TT) do { if (ICk == 1) GS_TEP(TT, 1); else if (ICk == 2) GS_TEP(TT, 2); else if (ICk == 3) GS_TEP(TT, 3); else GS_TEP(TT, 4); } while (0)
    GS_DISPATCH_DTYPE(dtype, GS_TEP_ALL(T));
#undef GS_TEP_ALL
#undef GS_TEP
    GS_CHECK_LAUNCH();
    return 0;
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
                                                          int ks, int N, int Hi, int Wi, int IC, int Ho, int Wo, float alpha) {
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pix >= (long)N * Ho * Wo) return;
    const int ox = pix % Wo;
    const int oy = (pix / Wo) % Ho;
    const int n = pix / ((long)Wo * Ho);
    float a = 0.f;
    for (int ky = 0; ky < ks; ++ky) {
        int iy;
        if (mode == MODE_S1) iy = oy + ky - (ks >> 1);
        else if (mode == MODE_S2) iy = 2 * oy + ky;
        else { const int d = oy - ky; if (d < 0 || (d & 1)) continue; iy = d >> 1; }
        if (iy < 0 || iy >= Hi) continue;
        for (int kx = 0; kx < ks; ++kx) {
            int ix;
            if (mode == MODE_S1) ix = ox + kx - (ks >> 1);
            else if (mode == MODE_S2) ix = 2 * ox + kx;
            else { const int d = ox - kx; if (d < 0 || (d & 1)) continue; ix = d >> 1; }
            if (ix < 0 || ix >= Wi) continue;
            const T* xp = x + (((long)n * Hi + iy) * Wi + ix) * IC;
            const float* wr = wp + (long)(ky * ks + kx) * IC;
            for (int ic = lane; ic < IC; ic += 64) a += DT<T>::ld(xp + ic) * wr[ic];
        }
    }
    a = wave_sum(a);
    if (lane == 0) DT<T>::st(y + pix, a * alpha);
}

// the same for 3x3 kernels with IC a multiple of 256: a lane owns 4 consecutive channels per 256-channel block and ALL its loads (9 taps x
// IC / 256 blocks, inputs and weights) are issued before the first multiply -- the generic kernel above walks 9 x IC / 64 dependent
// load pairs (11.6 us for the 256-channel stddev-plane gradient at 2 x 16: a pure latency chain)
template <typename T, int NB>
__global__ __launch_bounds__(256) void thin_single3_kernel(const T* __restrict__ x, const float* __restrict__ wp, T* __restrict__ y, int mode,
                                                           int N, int Hi, int Wi, int Ho, int Wo, float alpha) {
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
        bool ok = true;
        if (mode == MODE_S1) { iy = oy + ky - 1; ix = ox + kx - 1; }
        else if (mode == MODE_S2) { iy = 2 * oy + ky; ix = 2 * ox + kx; }
        else {
            const int dy = oy - ky, dx = ox - kx;
            ok = dy >= 0 && dx >= 0 && !(dy & 1) && !(dx & 1);
            iy = dy >> 1; ix = dx >> 1;
        }
        ok = ok && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
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
    if (lane == 0) DT<T>::st(y + pix, a * alpha);
}

// direct conv through the fp32 prepped weights living in ws; *fused is set when bias / act went into the same pass
static int run_direct(int mode, int ks, int variant, const void* x, const float* w_hwio, void* y, int N, int Hi, int Wi,
                      int ICk, int OCk, int w_ci, int w_co, int Ho, int Wo, float alpha, int dtype, int w_prepared, void* ws,
                      size_t ws_bytes, hipStream_t st, const float* bias = nullptr, int act = GS_ACT_NONE, bool* fused = nullptr,
                      const void* mask = nullptr, int mask_act = 0, bool* mask_fused = nullptr, unsigned* bits_out = nullptr, bool* bits_done = nullptr) {
    const long total = (long)ks * ks * w_ci * w_co;
    if (ws_bytes < (size_t)total * 4) return fail(GS_ERR_WORKSPACE, "conv direct: workspace %zu < %zu", ws_bytes, (size_t)total * 4);
    float* wp = reinterpret_cast<float*>(ws);
    if (!w_prepared) {
        hipLaunchKernelGGL((weight_prep_kernel<float>), dim3(cdiv(total, 256)), dim3(256), 0, st, w_hwio, wp, ks * ks, w_ci, w_co, variant);
        GS_CHECK_LAUNCH();
    }
    if (fused) *fused = false;
    const long P = (long)N * Ho * Wo;
    const int wn = dtype == GS_F32 ? 4 : 8;
    if (ks == 1 && mode == MODE_S1 && ICk <= 4 && OCk % wn == 0 && 256 % (OCk / wn) == 0) {   // colour -> features
        long nb = cdiv(P * (OCk / wn), 256);
        // (2048 blocks: 18.5 us for the 67 MB of the top level against 19.4 at 4096 and 23.0 at 8192 -- every block pays the weight prologue)
        static const long te_cap = getenv("GS_THIN_EXPAND_BLOCKS") ? atol(getenv("GS_THIN_EXPAND_BLOCKS")) : 2048;
        if (nb > te_cap) nb = te_cap;
        const unsigned grid = (unsigned)nb;
        unsigned* te_bits = (bits_out && bits_done && !mask && act == GS_ACT_LRELU && dtype == GS_BF16 && OCk % 32 == 0) ? bits_out : nullptr;
        if (te_bits) *bits_done = true;
#define GS_TE(TT, ICV, ACTV, MK) hipLaunchKernelGGL((thin_expand_kernel<TT, ICV, ACTV, MK>), dim3(grid), dim3(256), 0, st, (const TT*)x, wp, bias, (TT*)y, P, OCk, alpha, (const TT*)mask, mask_act, te_bits)
#define GS_TE_ACT(TT, ICV)                                                                                               \
    do {                                                                                                                 \
        if (mask) {   /* (masked: a forward on a cotangent -- the activation, if any, is applied by the slower generic form) */ \
            if (act == GS_ACT_NONE) GS_TE(TT, ICV, GS_ACT_NONE, true);                                                   \
            else if (act == GS_ACT_LRELU) GS_TE(TT, ICV, GS_ACT_LRELU, true);                                            \
            else GS_TE(TT, ICV, GS_ACT_TANH, true);                                                                      \
        } else if (act == GS_ACT_LRELU) GS_TE(TT, ICV, GS_ACT_LRELU, false);                                             \
        else if (act == GS_ACT_TANH) GS_TE(TT, ICV, GS_ACT_TANH, false);                                                 \
        else GS_TE(TT, ICV, GS_ACT_NONE, false);                                                                         \
    } while (0)
#define GS_TE_ALL(TT) do { if (ICk == 1) GS_TE_ACT(TT, 1); else if (ICk == 2) GS_TE_ACT(TT, 2); else if (ICk == 3) GS_TE_ACT(TT, 3); else GS_TE_ACT(TT, 4); } while (0)
        GS_DISPATCH_DTYPE(dtype, GS_TE_ALL(T));
#undef GS_TE_ALL
#undef GS_TE_ACT
#undef GS_TE
        GS_CHECK_LAUNCH();
        if (mask_fused) *mask_fused = mask != nullptr;
        if (fused) *fused = true;
        else if (bias || act != GS_ACT_NONE) return fail(GS_ERR_ARG, "conv direct: epilogue requested without a fused flag");
        return 0;
    }
    const int lanes = ICk / wn;
    if (ks == 1 && mode == MODE_S1 && OCk <= 4 && ICk % wn == 0 && lanes <= 64 && (lanes & (lanes - 1)) == 0) {  // features -> colour
        long nb = cdiv(P * lanes, 256);
        static const long tr_cap = getenv("GS_THIN_REDUCE_BLOCKS") ? atol(getenv("GS_THIN_REDUCE_BLOCKS")) : 4096;
        if (nb > tr_cap) nb = tr_cap;
        const unsigned grid = (unsigned)nb;
#define GS_TRL(TT, OCV, ACTV, LV) hipLaunchKernelGGL((thin_reduce_kernel<TT, OCV, ACTV, LV>), dim3(grid), dim3(256), 0, st, (const TT*)x, wp, bias, (TT*)y, P, ICk, alpha)
#define GS_TR(TT, OCV, ACTV) do { if (lanes == 4) GS_TRL(TT, OCV, ACTV, 4); else if (lanes == 8) GS_TRL(TT, OCV, ACTV, 8); else GS_TRL(TT, OCV, ACTV, 0); } while (0)
#define GS_TR_ACT(TT, OCV) do { if (act == GS_ACT_LRELU) GS_TR(TT, OCV, GS_ACT_LRELU); else if (act == GS_ACT_TANH) GS_TR(TT, OCV, GS_ACT_TANH); else GS_TR(TT, OCV, GS_ACT_NONE); } while (0)
#define GS_TR_ALL(TT) do { if (OCk == 1) GS_TR_ACT(TT, 1); else if (OCk == 2) GS_TR_ACT(TT, 2); else if (OCk == 3) GS_TR_ACT(TT, 3); else GS_TR_ACT(TT, 4); } while (0)
        GS_DISPATCH_DTYPE(dtype, GS_TR_ALL(T));
#undef GS_TR_ALL
#undef GS_TR_ACT
#undef GS_TR
#undef GS_TRL
        GS_CHECK_LAUNCH();
        if (fused) *fused = true;
        return 0;
    }
    if (OCk == 1 && ICk == 256 && ks == 3) {
        GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((thin_single3_kernel<T, 1>), dim3((unsigned)cdiv(P, 4)), dim3(256), 0, st, (const T*)x, wp, (T*)y, mode,
                                                    N, Hi, Wi, Ho, Wo, alpha));
        GS_CHECK_LAUNCH();
        return 0;
    }
    if (OCk == 1 && ICk >= 64) {
        GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((thin_single_kernel<T>), dim3((unsigned)cdiv(P, 4)), dim3(256), 0, st, (const T*)x, wp, (T*)y, mode,
                                                    ks, N, Hi, Wi, ICk, Ho, Wo, alpha));
        GS_CHECK_LAUNCH();
        return 0;
    }
    GS_DISPATCH_DTYPE(dtype, return launch_direct<T>(reinterpret_cast<const T*>(x), wp, reinterpret_cast<T*>(y), mode, ks,
                                                     N, Hi, Wi, ICk, OCk, Ho, Wo, alpha, st));
}

// ------------------------------------------------------------------ batched weight re-layout
// which operand a map's entry point builds: (variant of weight_prep_kernel, fp32 storage for the direct kernels / T for MFMA)
__device__ __host__ inline void prep_plan(int map, int ci, int co, int ksize, int dtype, int* variant, bool* store_f32) {
    const int bk = dtype == GS_F32 ? 16 : 32;
    bool mfma;
    if (map == GS_PREP_CONV_FWD || map == GS_PREP_CONVT_FWD) {
        *variant = 0;
        mfma = ksize == 3 && ci % bk == 0 && co % 32 == 0;
    } else if (map == GS_PREP_CONV_BWD_DATA) {   // stride 1: flipped taps; stride 2: transposed-conv walk (set by the caller)
        *variant = 1;
        mfma = ksize == 3 && co % bk == 0 && ci % 32 == 0;
    } else {
        *variant = 2;
        mfma = co % bk == 0 && ci % 32 == 0;
    }
    *store_f32 = !mfma || dtype == GS_F32;
}
// One 64 x 64 (ci x co) tile of one tap per trip, staged through LDS so that both sides move whole 256-byte rows: the forward operand
// is the TRANSPOSE of the stored [ci][co] slab (a thread-per-element gather read it with a stride of co floats: 31 us per launch for the
// ~20 MB of a network, now bandwidth-bound); the data-gradient operands are (tap-flipped) copies.
static __global__ __launch_bounds__(256) void weight_prep_batch_kernel(const GsPrepDesc* __restrict__ descs) {
    __shared__ float tile[64][65];
    const GsPrepDesc d = descs[blockIdx.y];
    int variant;
    bool f32;
    prep_plan(d.map, d.ci, d.co, d.ksize, d.dtype, &variant, &f32);
    if (d.map == GS_PREP_CONV_BWD_DATA && d.stride == 2) variant = 2;
    const int taps = d.ksize * d.ksize, ci = d.ci, co = d.co;
    const int tci = (ci + 63) >> 6, tco = (co + 63) >> 6;
    const int ntiles = taps * tci * tco;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // 16 x 16 threads, 4 consecutive elements each
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int t = tl / (tci * tco), r = tl % (tci * tco);
        const int i0 = (r / tco) * 64, o0 = (r % tco) * 64;
        const float* src = d.w_hwio + (long)t * ci * co;
        if (variant == 0) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // rows i0 + ty + 16 k, columns o0 + 4 tx ..
                const int i = i0 + ty + 16 * k, o = o0 + 4 * tx;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (i < ci) {
                    if (o + 3 < co && (co & 3) == 0) { const float4 q = *reinterpret_cast<const float4*>(src + (long)i * co + o); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
                    else { for (int e = 0; e < 4; ++e) if (o + e < co) v[e] = src[(long)i * co + o + e]; }
                }
                for (int e = 0; e < 4; ++e) tile[ty + 16 * k][4 * tx + e] = v[e];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // output rows o0 + ty + 16 k, 4 consecutive input channels i0 + 4 tx ..
                const int o = o0 + ty + 16 * k, i = i0 + 4 * tx;
                if (o >= co) continue;
                float v[4];
                for (int e = 0; e < 4; ++e) v[e] = tile[4 * tx + e][ty + 16 * k];
                const long dst = ((long)t * co + o) * ci + i;
                if (i + 3 < ci && (ci & 3) == 0) {
                    if (f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.ws) + dst) = make_float4(v[0], v[1], v[2], v[3]);
                    else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(d.ws) + dst) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (i + e < ci) {
                            if (f32) reinterpret_cast<float*>(d.ws)[dst + e] = v[e];
                            else reinterpret_cast<bf16_t*>(d.ws)[dst + e] = f32_to_bf16(v[e]);
                        }
                }
            }
        } else {
            const int tt = variant == 1 ? taps - 1 - t : t;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + ty + 16 * k, o = o0 + 4 * tx;
                if (i >= ci) continue;
                const long so = (long)i * co + o, dst = (long)tt * ci * co + so;
                if (o + 3 < co && (co & 3) == 0) {
                    const float4 q = *reinterpret_cast<const float4*>(src + so);
                    if (f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.ws) + dst) = q;
                    else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(d.ws) + dst) = make_uint2(pack_bf16x2(q.x, q.y), pack_bf16x2(q.z, q.w));
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (o + e < co) {
                            if (f32) reinterpret_cast<float*>(d.ws)[dst + e] = src[so + e];
                            else reinterpret_cast<bf16_t*>(d.ws)[dst + e] = f32_to_bf16(src[so + e]);
                        }
                }
            }
        }
    }
}

extern "C" int gs_weight_prep_batch(const GsPrepDesc* descs, int n, void* stream) {
    GS_CHECK_ARG(descs != nullptr && n > 0 && n <= 65535, "weight_prep_batch: bad args");
    hipLaunchKernelGGL(weight_prep_batch_kernel, dim3(48, n), dim3(256), 0, as_stream(stream), descs);
    GS_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ direct weight gradient
// part[slice][t][ic][oc] = sum over the slice's output pixels of x[in(p,t)][ic] * gy[p][oc]
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_direct_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                                                                float* __restrict__ part, int mode, int ks, int N, int Hi,
                                                                int Wi, int IC, int OC, int Hb, int Wb, long E, long npix,
                                                                long pps) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const long e = (long)blockIdx.x * 64 + (tid & 63);
    const int sub = tid >> 6;
    const int slice = blockIdx.y;
    float acc = 0.f;
    if (e < E) {
        const int oc = e % OC;
        const int ic = (e / OC) % IC;
        const int t = e / ((long)IC * OC);
        const int ky = t / ks, kx = t % ks;
        const long p0 = (long)slice * pps;
        long p1 = p0 + pps;
        if (p1 > npix) p1 = npix;
        // (branch-free body, clamped addresses: unrolled, the loads of four pixels are in flight together -- with a `continue` per pixel the
        //  loop was a chain of dependent load pairs: 10 us for the 256 pixels of the stddev-plane conv at 2 x 16)
#pragma unroll 4
        for (long p = p0 + sub; p < p1; p += 4) {
            const int px = (int)(p % Wb);
            const long q = p / Wb;
            const int py = (int)(q % Hb);
            const int n = (int)(q / Hb);
            int iy, ix;
            if (mode == MODE_S1) { iy = py + ky - (ks >> 1); ix = px + kx - (ks >> 1); }
            else { iy = 2 * py + ky; ix = 2 * px + kx; }
            const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
            const float xv = DT<T>::ld(x + (((long)n * Hi + (ok ? iy : 0)) * Wi + (ok ? ix : 0)) * IC + ic);
            const float gv = DT<T>::ld(gy + p * OC + oc);
            acc += ok ? xv * gv : 0.f;
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (sub == 0 && e < E) part[(long)slice * E + e] = red[tid] + red[tid + 64] + red[tid + 128] + red[tid + 192];
}

// ------------------------------------------------------------- thin 1x1 weight gradient
// The colour convs have 2 channels on one side: gw = sum_p wide[p][C] (x) thin[p][2].  One streaming pass:
// C/4 lanes per pixel hold 4 wide channels x 2 thin values = 8 accumulators, pixel lanes reduce through LDS.
// WIDE_IS_X: x is the wide tensor (gw[c][j], Cout = 2), else gy is (gw[j][c], Cin = 2).
template <typename T, bool WIDE_IS_X>
__global__ __launch_bounds__(256) void thin_wgrad_kernel(const T* __restrict__ wide, const T* __restrict__ thin, float* __restrict__ part,
                                                         int C, long npix, long pps) {
    __shared__ float red[256 * 8];
    const int quads = C >> 2;
    const int rpi = 256 / quads;  // pixel lanes per iteration
    const int q = threadIdx.x % quads, r = threadIdx.x / quads;
    const long p0 = (long)blockIdx.x * pps;
    long p1 = p0 + pps;
    if (p1 > npix) p1 = npix;
    float acc[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    if (r < rpi) {
        long p = p0 + r;
        for (; p + 3 * rpi < p1; p += 4 * rpi) {   // four pixels per trip: their loads are in flight together
            float w4[4][4], t[4][2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ld4(wide + (p + k * rpi) * C + q * 4, w4[k]);
                t[k][0] = DT<T>::ld(thin + (p + k * rpi) * 2);
                t[k][1] = DT<T>::ld(thin + (p + k * rpi) * 2 + 1);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[e][0] += w4[k][e] * t[k][0]; acc[e][1] += w4[k][e] * t[k][1]; }
        }
        for (; p < p1; p += rpi) {
            float w4[4];
            ld4(wide + p * C + q * 4, w4);
            const float t0 = DT<T>::ld(thin + p * 2), t1 = DT<T>::ld(thin + p * 2 + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e][0] += w4[e] * t0; acc[e][1] += w4[e] * t1; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[threadIdx.x * 8 + e * 2] = acc[e][0]; red[threadIdx.x * 8 + e * 2 + 1] = acc[e][1]; }
    __syncthreads();
    if (threadIdx.x < quads) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < rpi; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += red[(k * quads + threadIdx.x) * 8 + e];
        float* out = part + (long)blockIdx.x * C * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = threadIdx.x * 4 + e;
            if (WIDE_IS_X) { out[c * 2] = s[e * 2]; out[c * 2 + 1] = s[e * 2 + 1]; }
            else { out[c] = s[e * 2]; out[C + c] = s[e * 2 + 1]; }
        }
    }
}

static size_t wgrad_direct_bytes(int mode, int ks, int dtype, int N, int Hb, int Wb, int IC, int OC) {
    const WgradPlan p = wgrad_plan(mode, ks, dtype, N, Hb, Wb, IC, OC);
    return align256((size_t)p.ws_slices * ks * ks * IC * OC * 4);
}

static int run_wgrad_direct(int mode, int ks, const void* x, const void* gy, float* gw, int N, int Hi, int Wi, int IC,
                            int OC, int Hb, int Wb, float alpha, int transpose, int accumulate, int dtype, void* ws, size_t ws_bytes,
                            hipStream_t st, GsWgradReduce* defer = nullptr) {
    const WgradPlan p = wgrad_plan(mode, ks, dtype, N, Hb, Wb, IC, OC);
    if (p.family > WG_THIN) return fail(GS_ERR_UNSUPPORTED, "conv wgrad direct: %d -> %d channels belong to the MFMA kernels", IC, OC);
    const long ns = p.nslices, pps = p.pps;
    const long npix = (long)N * Hb * Wb;
    const long E = (long)ks * ks * IC * OC;
    if (p.family == WG_THIN) {
        const int C = IC == 2 ? OC : IC;
        if (ws_bytes < (size_t)ns * E * 4) return fail(GS_ERR_WORKSPACE, "conv wgrad thin: workspace too small (%zu)", ws_bytes);
        float* tpart = reinterpret_cast<float*>(ws);
        if (!p.ot) {
            GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((thin_wgrad_kernel<T, false>), dim3((unsigned)ns), dim3(256), 0, st,
                                                        reinterpret_cast<const T*>(gy), reinterpret_cast<const T*>(x), tpart, C, npix, pps));
        } else {
            GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((thin_wgrad_kernel<T, true>), dim3((unsigned)ns), dim3(256), 0, st,
                                                        reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(gy), tpart, C, npix, pps));
        }
        GS_CHECK_LAUNCH();
        wgrad_reduce_launch(tpart, gw, nullptr, (int)ns, 1, IC, OC, alpha, transpose, accumulate, st, defer);
        GS_CHECK_LAUNCH();
        return 0;
    }
    if (ws_bytes < (size_t)ns * E * 4) return fail(GS_ERR_WORKSPACE, "conv wgrad direct: workspace too small (%zu)", ws_bytes);
    float* part = reinterpret_cast<float*>(ws);
    dim3 grid(cdiv(E, 64), (unsigned)ns);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv_wgrad_direct_kernel<T>), grid, dim3(256), 0, st,
                                                reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(gy), part, mode,
                                                ks, N, Hi, Wi, IC, OC, Hb, Wb, E, npix, pps));
    GS_CHECK_LAUNCH();
    wgrad_reduce_launch(part, gw, nullptr, (int)ns, ks * ks, IC, OC, alpha, transpose, accumulate, st, defer);
    GS_CHECK_LAUNCH();
    return 0;
}

static int check_conv(const GsConv* c) {
    GS_CHECK_ARG(c != nullptr, "conv: no layer descriptor");
    GS_CHECK_ARG(c->n > 0 && c->h > 0 && c->w > 0 && c->ci > 0 && c->co > 0, "conv: non-positive dim");
    GS_CHECK_ARG(!c->transposed || (c->ksize == 3 && c->stride == 2), "conv: a transposed layer is 3x3 stride 2 (got %dx%d stride %d)", c->ksize, c->ksize, c->stride);
    GS_CHECK_ARG(c->ksize == 1 || c->ksize == 3, "conv: ksize %d not in {1,3}", c->ksize);
    GS_CHECK_ARG(c->stride == 1 || (c->stride == 2 && c->ksize == 3), "conv: stride %d unsupported with ksize %d", c->stride, c->ksize);
    GS_CHECK_ARG(c->stride == 1 || c->transposed || (c->h % 2 == 0 && c->w % 2 == 0), "conv: stride 2 needs even h,w (got %d,%d)", c->h, c->w);
    GS_CHECK_ARG(c->dtype == GS_F32 || c->dtype == GS_BF16, "conv: bad dtype %d", c->dtype);
    return 0;
}

// ---- THE relabelling: a layer and one of its three maps -> the roles the kernels know.  A transposed conv is the stride-2 conv with its two
// sides swapped, so every map of either kind is one of MODE_S1 / MODE_S2 / MODE_T2 over (ICk -> OCk) channels, reading Hi x Wi and walking
// the base grid Hb x Wb (the smaller side of a strided map).  Every entry point below, plan_jobs and the *_is_fused queries take their
// geometry from here and nowhere else (a valid layer is assumed: check_conv first).
struct ConvRole {
    int mode;         // MODE_*
    int variant;      // weight_prep_kernel's (fwd / bwd_data)
    int ICk, OCk;     // channels the kernel contracts / produces; bwd_weight: its input side / gradient side
    int Hi, Wi;       // what the kernel reads (bwd_weight: its input side)
    int Hb, Wb;       // base grid
    int Ho, Wo;       // what the kernel writes: the base grid, twice it in MODE_T2
    int swapped;      // bwd_weight of a transposed layer: x and gy change places and gw is stored transposed
};
static ConvRole conv_role(const GsConv& c, int map) {
    const int s = c.stride;
    ConvRole r;
    memset(&r, 0, sizeof(r));
    const bool up = c.transposed != 0;
    if (map == GS_CONV_BWD_DATA) {
        r.ICk = c.co; r.OCk = c.ci;
        if (up) { r.mode = MODE_S2; r.variant = 2; r.Hi = 2 * c.h; r.Wi = 2 * c.w; r.Hb = c.h; r.Wb = c.w; }
        else if (s == 2) { r.mode = MODE_T2; r.variant = 2; r.Hi = r.Hb = c.h / 2; r.Wi = r.Wb = c.w / 2; }
        else { r.mode = MODE_S1; r.variant = 1; r.Hi = r.Hb = c.h; r.Wi = r.Wb = c.w; }
    } else if (map == GS_CONV_BWD_WEIGHT && up) {   // the stride-2 conv from the big side to the small one
        r.mode = MODE_S2; r.swapped = 1;
        r.ICk = c.co; r.OCk = c.ci; r.Hi = 2 * c.h; r.Wi = 2 * c.w; r.Hb = c.h; r.Wb = c.w;
    } else {                                         // fwd, and the plain conv's bwd_weight
        r.mode = up ? MODE_T2 : (s == 2 ? MODE_S2 : MODE_S1);
        r.ICk = c.ci; r.OCk = c.co; r.Hi = c.h; r.Wi = c.w;
        r.Hb = up ? c.h : c.h / s; r.Wb = up ? c.w : c.w / s;
    }
    const int f = r.mode == MODE_T2 ? 2 : 1;
    r.Ho = f * r.Hb; r.Wo = f * r.Wb;
    return r;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_channel_sum_workspace_bytes(int64_t p, int c);
extern "C" int gs_channel_sum(const void* g, float* out, int64_t p, int c, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
extern "C" int gs_bias_act_fwd(const void* x, const float* bias, void* y, int64_t p, int c, int act, int dtype, void* stream);   // the epilogue of the shapes without the MFMA kernel
extern "C" int gs_act_bwd(const void* g, const void* y, void* gx, int64_t numel, int act, int dtype, void* stream);

extern "C" size_t gs_conv_workspace_bytes(const GsConv* c, int which) {
    if (check_conv(c)) return 0;
    if (which != GS_CONV_BWD_WEIGHT) return align256((size_t)c->ksize * c->ksize * c->ci * c->co * 4);   // the re-laid weight
    const ConvRole r = conv_role(*c, GS_CONV_BWD_WEIGHT);
    const size_t wg = wgrad_plan(r.mode, c->ksize, c->dtype, c->n, r.Hb, r.Wb, r.ICk, r.OCk).family >= WG_F32
                          ? wgrad_mfma_bytes(r.mode, c->dtype, c->n, r.Hb, r.Wb, r.ICk, r.OCk)
                          : wgrad_direct_bytes(r.mode, c->ksize, c->dtype, c->n, r.Hb, r.Wb, r.ICk, r.OCk);
    if (c->transposed) return wg;   // (no bias)
    const size_t cs = align256(gs_channel_sum_workspace_bytes((int64_t)c->n * r.Hb * r.Wb, c->co));   // bias-gradient fallback of gs_conv_bwd_weight
    return wg > cs ? wg : cs;
}

static int mask_fuse_min_channels() {
    static const int v = [] { const char* e = getenv("GS_MASK_FUSE_MIN_CI"); return e ? atoi(e) : 32; }();   // (env: measurement knob)
    return v;
}
static bool mask_act_ok(int a) { return a == GS_ACT_LRELU || a == GS_ACT_TANH || a == GS_ACT_LRELU_BITS; }

// y_norm (optional): y_norm = pixel_norm(act(conv + bias)) as well -- fused into the conv epilogue where the tile owns all channels of a
// pixel, a separate pass otherwise; y (the activation itself) may then be NULL
extern "C" int gs_conv_fwd(const GsConv* c, const void* x, const float* w_hwio, const float* bias, int act, void* y, void* y_norm, float eps, void* stream) {
    if (int e = check_conv(c)) return e;
    const bool want_bits = (act & GS_ACT_WRITE_BITS) != 0;   // (the caller's y has room for the sign bits behind it: include/gansynth_hip.h)
    act &= ~GS_ACT_WRITE_BITS;
    GS_CHECK_ARG(act == GS_ACT_NONE || act == GS_ACT_LRELU || act == GS_ACT_TANH, "conv_fwd: bad activation %d", act);
    GS_CHECK_ARG(!want_bits || (act == GS_ACT_LRELU && c->dtype == GS_BF16 && c->co % 32 == 0 && y && !c->transposed),
                 "conv_fwd: sign bits go with a plain conv's bf16 leaky-relu result of 32 k channels");
    GS_CHECK_ARG(y || y_norm, "conv_fwd: no output");
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    if (c->ksize == 3 && igemm_supported(r.ICk, r.OCk, c->dtype) && act != GS_ACT_TANH)
        return run_igemm(r.mode, r.variant, x, w_hwio, y, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, bias, act | (want_bits ? GS_ACT_WRITE_BITS : 0),
                         c->dtype, c->w_prepared, c->ws, c->ws_bytes, st, nullptr, 0, y_norm, eps);
    void* z = y ? y : y_norm;
    const int64_t P = (int64_t)c->n * r.Ho * r.Wo;
    bool fused = false;
    bool bits_done = false;
    unsigned* bits_out = (want_bits && !y_norm) ? reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(y) + (size_t)P * c->co) : nullptr;
    if (int e = run_direct(r.mode, c->ksize, r.variant, x, w_hwio, z, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Ho, r.Wo, c->alpha, c->dtype, c->w_prepared, c->ws,
                           c->ws_bytes, st, bias, act, &fused, nullptr, 0, nullptr, bits_out, &bits_done))
        return e;
    if (!fused && (bias || act != GS_ACT_NONE))
        if (int e = gs_bias_act_fwd(z, bias, z, P, c->co, act, c->dtype, stream)) return e;
    if (y_norm)
        if (int e = gs_pixel_norm_fwd(z, y_norm, P, c->co, eps, c->dtype, stream)) return e;
    if (want_bits && !bits_done) return gs_pack_act_bits(y, P, c->co, c->dtype, stream);   // (direct kernels other than the colour block's)
    return 0;
}

// y = conv(x, w) * mask_act'(.) through `mask` (an activation OUTPUT of y's shape): the second-order pass of the R1 penalty runs
// the discriminator's convs forward on cotangents and multiplies each result by the derivative of the activation that follows
// the conv; in the epilogue on the MFMA path (see gs_conv_bwd_data), in place after the conv otherwise
extern "C" int gs_conv_fwd_mask(const GsConv* c, const void* x, const float* w_hwio, const void* mask, int mask_act, void* y, void* stream) {
    if (int e = check_conv(c)) return e;
    if (c->transposed) return fail(GS_ERR_UNSUPPORTED, "conv_fwd_mask: no masked forward of a transposed layer");
    GS_CHECK_ARG(mask == nullptr || mask_act_ok(mask_act), "conv_fwd_mask: bad activation %d", mask_act);
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    const bool mfma = c->ksize == 3 && igemm_supported(r.ICk, r.OCk, c->dtype);
    const bool fused = mask != nullptr && c->co >= mask_fuse_min_channels() && mfma;
    int rc;
    const int bits_act = mask_act;   // (only the MFMA epilogue reads the sign bits; every other path reads the values they stand behind)
    if (mask_act == GS_ACT_LRELU_BITS) mask_act = GS_ACT_LRELU;
    if (mfma)
        rc = run_igemm(r.mode, r.variant, x, w_hwio, y, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared, c->ws,
                       c->ws_bytes, st, fused ? mask : nullptr, bits_act);
    else {   // (the colour block's streaming kernel applies the mask itself; the other direct kernels leave it to the pass below)
        bool epi = false, mdone = false;
        rc = run_direct(r.mode, c->ksize, r.variant, x, w_hwio, y, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Ho, r.Wo, c->alpha, c->dtype, c->w_prepared, c->ws, c->ws_bytes,
                        st, nullptr, GS_ACT_NONE, &epi, mask, mask_act, &mdone);
        if (rc || !mask || mdone) return rc;
    }
    if (rc || !mask || fused) return rc;
    return gs_act_bwd(y, mask, y, (int64_t)c->n * r.Ho * r.Wo * c->co, mask_act, c->dtype, stream);
}

// gx = bwd_data(gy, w) * mask_act'(.) through `mask` (the activation OUTPUT that was the layer's input; NULL: plain)
extern "C" int gs_conv_bwd_data(const GsConv* c, const void* gy, const float* w_hwio, const void* mask, int mask_act, void* gx, void* stream) {
    if (int e = check_conv(c)) return e;
    if (c->transposed && mask) return fail(GS_ERR_UNSUPPORTED, "conv_bwd_data: no masked data gradient of a transposed layer");
    GS_CHECK_ARG(mask == nullptr || mask_act_ok(mask_act), "conv_bwd_data: bad activation %d", mask_act);
    const int bits_act = mask_act;   // (see gs_conv_fwd_mask)
    if (mask_act == GS_ACT_LRELU_BITS) mask_act = GS_ACT_LRELU;
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_BWD_DATA);
    int rc;
    // In the epilogue the mask costs one more read of gx's size; with the mask vectors fetched ahead of the epilogue arithmetic
    // (conv_igemm.hip) that beats the separate in-place pass on every MFMA-path layer, the HBM-bound 32-channel top included
    // (+1.6 % on the step against fusing from 64 channels up).
    bool fused = mask != nullptr && c->ci >= mask_fuse_min_channels();
    if (c->ksize == 3 && igemm_supported(r.ICk, r.OCk, c->dtype))
        rc = run_igemm(r.mode, r.variant, gy, w_hwio, gx, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared, c->ws,
                       c->ws_bytes, st, fused ? mask : nullptr, bits_act);
    else {
        rc = run_direct(r.mode, c->ksize, r.variant, gy, w_hwio, gx, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Ho, r.Wo, c->alpha, c->dtype, c->w_prepared, c->ws, c->ws_bytes, st);
        fused = false;
    }
    if (rc || !mask || fused) return rc;
    return gs_act_bwd(gx, mask, gx, (int64_t)c->n * r.Ho * r.Wo * c->ci, mask_act, c->dtype, stream);   // shapes without the MFMA kernel: in place
}

// the (x, gy) pairs of one launch, as the kernels want them; for the transposed conv the roles of the two sides swap
static WgradSrcs make_srcs(const void* const* xs, const void* const* gys, int nsrc, int n_per, const int* ns, unsigned bias_mask, bool swap, int* total) {
    WgradSrcs s;
    memset(&s, 0, sizeof(s));
    int end = 0;
    for (int i = 0; i < GS_WGRAD_MAX_SRC; ++i) {
        if (i < nsrc) {
            s.x[i] = swap ? gys[i] : xs[i];
            s.gy[i] = swap ? xs[i] : gys[i];
            end += ns ? ns[i] : n_per;
        }
        s.n_end[i] = end;
    }
    s.bias_mask = bias_mask;
    *total = end;
    return s;
}

// One layer's weight gradient from several (x, gy) pairs in one launch: gw (+)= sum_s bwd_weight(xs[s], gys[s]); pair s has ns[s] images
// (ns NULL: c.n each) and bit s of bias_mask says whether it contributes to gb (ignored when gb is NULL).  The layer then costs one set of
// block partials and one slice reduction instead of one per pair.  `pending` (NULL = reduce at once): see GsWgradReduce.  c.ws is sized by
// gs_conv_workspace_bytes(GS_CONV_BWD_WEIGHT) for the total image count.
static int wgrad_layer(const GsConv& c, const void* const* xs, const void* const* gys, const int* ns, int nsrc, unsigned bias_mask, float* gw_hwio, float* gb,
                       int accumulate, GsWgradReduce* pending, void* stream) {
    if (int e = check_conv(&c)) return e;
    GS_CHECK_ARG(!(c.transposed && gb), "conv_bwd_weight: a transposed layer has no bias gradient");
    GS_CHECK_ARG(xs && gys && nsrc >= 1 && nsrc <= GS_WGRAD_MAX_SRC, "conv_bwd_weight: %d sources (1..%d)", nsrc, GS_WGRAD_MAX_SRC);
    for (int i = 0; i < nsrc; ++i) GS_CHECK_ARG(xs[i] && gys[i], "conv_bwd_weight: null source %d", i);
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(c, GS_CONV_BWD_WEIGHT);
    const WgradPlan lp = wgrad_plan(r.mode, c.ksize, c.dtype, c.n, r.Hb, r.Wb, r.ICk, r.OCk);   // (family and bias form: functions of the layer, not of n)
    const bool mfma = lp.family >= WG_F32;
    if (pending) memset(pending, 0, sizeof(*pending));
    if (!gb) bias_mask = 0;
    if (nsrc > 1 && !(mfma && (!gb || lp.fused_bias))) {
        // shapes without the multi-source kernels: one call per source (the first applies `accumulate`, the rest add)
        for (int i = 0; i < nsrc; ++i) {
            GsConv one = c;
            if (ns) one.n = ns[i];
            const int rc = wgrad_layer(one, xs + i, gys + i, nullptr, 1, 1u, gw_hwio, ((bias_mask >> i) & 1u) ? gb : nullptr, i == 0 ? accumulate : 1, nullptr, stream);
            if (rc) return rc;
        }
        return 0;
    }
    const bool fused_bias = bias_mask && lp.fused_bias;
    // the channel-sum fallback of the bias gradient reuses ws: such calls cannot leave their partials pending
    GsWgradReduce* defer = (bias_mask && !fused_bias) ? nullptr : pending;
    int rc;
    const int n0 = ns ? ns[0] : c.n;   // (the single-source paths below)
    if (mfma) {
        int total = 0;
        const WgradSrcs srcs = make_srcs(xs, gys, nsrc, c.n, ns, bias_mask, r.swapped != 0, &total);
        rc = run_wgrad_mfma(r.mode, srcs, nsrc, gw_hwio, fused_bias ? gb : nullptr, total, r.Hi, r.Wi, r.ICk, r.OCk, r.Hb, r.Wb, c.alpha, r.swapped, accumulate, c.dtype, c.ws,
                            c.ws_bytes, st, defer);
    } else {
        rc = run_wgrad_direct(r.mode, c.ksize, r.swapped ? gys[0] : xs[0], r.swapped ? xs[0] : gys[0], gw_hwio, n0, r.Hi, r.Wi, r.ICk, r.OCk, r.Hb, r.Wb, c.alpha, r.swapped,
                              accumulate, c.dtype, c.ws, c.ws_bytes, st, defer);
    }
    if (rc || !bias_mask || fused_bias) return rc;
    // shapes without the fused path: the plain channel sum (stream-ordered after the kernels above, same workspace)
    return gs_channel_sum(gys[0], gb, (int64_t)n0 * r.Hb * r.Wb, c.co, accumulate, c.dtype, c.ws, c.ws_bytes, stream);
}

extern "C" int gs_conv_bwd_weight(const GsConv* c, const void* x, const void* gy, float* gw_hwio, float* gb, int accumulate, void* stream) {
    if (int e = check_conv(c)) return e;
    return wgrad_layer(*c, &x, &gy, nullptr, 1, 1u, gw_hwio, gb, accumulate, nullptr, stream);
}

// many pending slice reductions in a handful of launches: up to GS_REDUCE_BATCH entries per launch, a new launch whenever an
// entry adds into a gradient that the current launch already touches (list order = summation order).  `pending`: host array
static int wgrad_reduce_batch(const GsWgradReduce* pending, int n, void* stream) {
    GS_CHECK_ARG(n >= 0 && (n == 0 || pending), "wgrad_reduce_batch: bad args");
    hipStream_t st = as_stream(stream);
    ReduceBatch b;
    int cnt = 0;
    long gx = 0;   // blocks of the entry that needs most (64 element quads per block with 4 slice lanes, 16 with 16: see the kernel)
    auto flush = [&]() {
        if (cnt == 0) return;
        wgrad_reduce_batch_launch(b, cnt, gx, st);
        cnt = 0;
        gx = 0;
    };
    for (int i = 0; i < n; ++i) {
        const GsWgradReduce& d = pending[i];
        if (d.nslices <= 0) continue;   // nothing pending for this call
        GS_CHECK_ARG(d.partials && d.gw && d.taps > 0 && d.ic > 0 && d.oc > 0 && (((long)d.taps * d.ic * d.oc) & 3) == 0 && (!d.gb || (d.oc & 3) == 0),
                     "wgrad_reduce_batch: entry %d is not a pending reduction", i);
        bool clash = cnt == GS_REDUCE_BATCH;
        for (int j = 0; j < cnt && !clash; ++j) clash = b.e[j].gw == d.gw || (d.gb && b.e[j].gb == d.gb);
        if (clash) flush();
        b.e[cnt++] = d;
        const long pstride = (long)d.taps * d.ic * d.oc + (d.gb ? d.oc : 0);
        const long epb = 256 / wgrad_fold_lanes(d.nslices);
        const long blocks = (pstride / 4 + epb - 1) / epb;
        if (blocks > gx) gx = blocks;
    }
    flush();
    GS_CHECK_LAUNCH();
    return 0;
}

// ---- all weight gradients of a backward pass in one call (gs_conv_wgrad_jobs): the layers the 64 x 64-tile bf16 kernel takes are
// grouped by its instantiation (the conv mode) and each group runs as ONE stream-K launch + one fold (conv_shared.h); every
// other layer goes through wgrad_layer above, its slice reduction left pending, and one wgrad_reduce_batch folds
// those at the end.  Workspace: the largest group (groups run one after the other on the stream) + the sum of the per-layer needs.
namespace gs {
struct JobPlan {
    std::vector<std::pair<int, SkGroup>> groups;   // (conv mode, group), in launch order
    std::vector<GsWgradJob> single;               // jobs on the per-layer path (one source each where the layer has no multi-source kernel)
    std::vector<size_t> single_off;               // their workspace offsets
    std::vector<std::vector<int>> group_jobs;      // per group: the index in the caller's list of each of its jobs (gs_conv_wgrad_jobs_plan)
    std::vector<std::pair<int, int>> single_src;   // per single job: (index in the caller's list, source it was split off for or -1)
    size_t group_bytes = 0, total_bytes = 0;
};
static GsConv job_conv(const GsWgradJob& jb, int n) {   // the job's layer, with n images
    GsConv c;
    memset(&c, 0, sizeof(c));
    c.n = n; c.h = jb.h; c.w = jb.w; c.ci = jb.ci; c.co = jb.co; c.ksize = jb.ksize; c.stride = jb.stride; c.transposed = jb.transposed;
    c.dtype = jb.dtype; c.alpha = jb.alpha;
    return c;
}
static int job_check(const GsWgradJob& jb, int idx) {
    GS_CHECK_ARG(jb.nsrc >= 1 && jb.nsrc <= GS_WGRAD_MAX_SRC && jb.gw, "conv_wgrad_jobs: job %d has %d sources (1..%d) / no output", idx, jb.nsrc, GS_WGRAD_MAX_SRC);
    for (int i = 0; i < jb.nsrc; ++i) GS_CHECK_ARG(jb.x[i] && jb.gy[i] && jb.n[i] > 0, "conv_wgrad_jobs: job %d, null or empty source %d", idx, i);
    GS_CHECK_ARG(!jb.transposed || (jb.ksize == 3 && jb.stride == 2 && !jb.gb), "conv_wgrad_jobs: job %d: the transposed conv is 3x3 stride 2 without bias", idx);
    GS_CHECK_ARG(jb.gw_ci_stride == 0 || (jb.gw_ci_stride >= jb.ci && !jb.transposed), "conv_wgrad_jobs: job %d: bad gw_ci_stride %d", idx, jb.gw_ci_stride);
    const GsConv c = job_conv(jb, jb.n[0]);
    return check_conv(&c);
}
static int job_total_images(const GsWgradJob& jb) {
    int t = 0;
    for (int i = 0; i < jb.nsrc; ++i) t += jb.n[i];
    return t;
}
static int plan_jobs(const GsWgradJob* jobs, int njobs, JobPlan& plan) {
    static const bool no_sk = getenv("GS_NO_WGRAD_GROUPS") != nullptr;   // measurement knob: everything on the per-layer path
    int open_idx[3] = {-1, -1, -1};   // conv mode -> index of the group still accepting jobs
    for (int i = 0; i < njobs; ++i) {
        const GsWgradJob& jb = jobs[i];
        if (int e = job_check(jb, i)) return e;
        const int total = job_total_images(jb);
        const ConvRole r = conv_role(job_conv(jb, total), GS_CONV_BWD_WEIGHT);
        const WgradPlan lp = wgrad_plan(r.mode, jb.ksize, jb.dtype, total, r.Hb, r.Wb, r.ICk, r.OCk);
        if (!no_sk && lp.family == WG_TILE64) {
            int gi = open_idx[r.mode];
            if (gi >= 0) {   // a full group, or one that already adds into this gradient, is closed (launch order = summation order)
                const SkGroup& og = plan.groups[gi].second;
                bool close = og.njobs == GS_SK_MAX_JOBS;
                for (int j = 0; j < og.njobs && !close; ++j) close = og.job[j].gw == jb.gw || (jb.gb && og.job[j].gb == jb.gb);
                if (close) gi = -1;
            }
            if (gi < 0) {
                SkGroup ng;
                memset(&ng, 0, sizeof(ng));
                plan.groups.push_back(std::make_pair(r.mode, ng));
                plan.group_jobs.push_back(std::vector<int>());
                gi = (int)plan.groups.size() - 1;
                open_idx[r.mode] = gi;
            }
            SkGroup& g = plan.groups[gi].second;
            SkJob& q = g.job[g.njobs++];
            plan.group_jobs[gi].push_back(i);
            int tot = 0;
            q.srcs = make_srcs(jb.x, jb.gy, jb.nsrc, 0, jb.n, jb.gb ? jb.bias_mask : 0u, r.swapped != 0, &tot);
            q.gw = jb.gw; q.gb = jb.gb; q.alpha = jb.alpha; q.transpose = r.swapped; q.accumulate = jb.accumulate;
            q.Hi = r.Hi; q.Wi = r.Wi; q.IC = r.ICk; q.OC = r.OCk; q.Hb = r.Hb; q.Wb = r.Wb;
            q.ICld = jb.gw_ci_stride > 0 ? jb.gw_ci_stride : r.ICk;
            wgrad_sk_job_geometry(r.mode, total, q);
        } else {
            // layers without a multi-source kernel (direct / thin kernels, fp32 bias sums): one single-source job per pair, each with its own
            // partials so that every slice reduction can stay pending
            const bool multi = lp.family >= WG_F32 && (!jb.gb || lp.fused_bias);
            if (jb.nsrc == 1 || multi) {
                plan.single.push_back(jb);
                plan.single_src.push_back(std::make_pair(i, -1));
            } else {
                for (int sidx = 0; sidx < jb.nsrc; ++sidx) {
                    GsWgradJob one = jb;
                    one.nsrc = 1;
                    one.x[0] = jb.x[sidx]; one.gy[0] = jb.gy[sidx]; one.n[0] = jb.n[sidx];
                    one.bias_mask = (jb.bias_mask >> sidx) & 1u;
                    if (!one.bias_mask) one.gb = nullptr;
                    if (sidx > 0) one.accumulate = 1;
                    plan.single.push_back(one);
                    plan.single_src.push_back(std::make_pair(i, sidx));
                }
            }
        }
    }
    for (auto& kg : plan.groups) {
        wgrad_sk_plan(kg.first, kg.second);
        const size_t b = wgrad_sk_bytes(kg.second);
        if (b > plan.group_bytes) plan.group_bytes = b;
    }
    size_t off = plan.group_bytes;
    for (const GsWgradJob& jb : plan.single) {
        const GsConv c = job_conv(jb, job_total_images(jb));
        plan.single_off.push_back(off);
        off += gs_conv_workspace_bytes(&c, GS_CONV_BWD_WEIGHT);
    }
    plan.total_bytes = off;
    return 0;
}
}  // namespace gs

extern "C" size_t gs_conv_wgrad_jobs_workspace_bytes(const GsWgradJob* jobs, int njobs) {
    if (!jobs || njobs <= 0) return 0;
    JobPlan plan;
    if (plan_jobs(jobs, njobs, plan)) return 0;
    return plan.total_bytes;
}

extern "C" int gs_conv_wgrad_jobs(const GsWgradJob* jobs, int njobs, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs), "conv_wgrad_jobs: bad args");
    if (njobs == 0) return 0;
    JobPlan plan;
    if (int e = plan_jobs(jobs, njobs, plan)) return e;
    if (ws_bytes < plan.total_bytes) return fail(GS_ERR_WORKSPACE, "conv_wgrad_jobs: workspace %zu < %zu", ws_bytes, plan.total_bytes);
    hipStream_t st = as_stream(stream);
    for (auto& kg : plan.groups)
        if (int e = run_wgrad_sk(kg.first, kg.second, ws, plan.group_bytes, st)) return e;
    std::vector<GsWgradReduce> pend;
    for (size_t k = 0; k < plan.single.size(); ++k) {
        const GsWgradJob& jb = plan.single[k];
        GsConv c = job_conv(jb, jb.n[0]);
        c.ws = reinterpret_cast<unsigned char*>(ws) + plan.single_off[k];
        c.ws_bytes = (k + 1 < plan.single.size() ? plan.single_off[k + 1] : plan.total_bytes) - plan.single_off[k];
        GsWgradReduce d;
        memset(&d, 0, sizeof(d));
        if (int rc = wgrad_layer(c, jb.x, jb.gy, jb.n, jb.nsrc, jb.bias_mask, jb.gw, jb.gb, jb.accumulate, &d, stream)) return rc;
        if (jb.gw_ci_stride > jb.ci) {   // a channel-slice target: only the pending (batched) fold knows the row stride
            if (d.nslices <= 0 || d.transpose) return fail(GS_ERR_UNSUPPORTED, "conv_wgrad_jobs: a %d -> %d layer cannot add into a channel slice", jb.ci, jb.co);
            d.ic_ld = jb.gw_ci_stride;
        }
        if (d.nslices > 0) pend.push_back(d);
    }
    if (!pend.empty()) return wgrad_reduce_batch(pend.data(), (int)pend.size(), stream);
    return 0;
}

// Second-order pass (the mode-seeking term differentiates the generator's backward, models.py:60): the forward conv applied to a cotangent gives
// t = the gradient w.r.t. u = act'(z) pixel_norm_bwd(g, z), the first-order backward of the block whose activation z and incoming gradient g
// are given.  Both gradients of that node in the conv's epilogue (h = t act'(z)):
//   out_g = pixel_norm_bwd(h, z)                 (w.r.t. g)          out_z = d<h, pixel_norm_bwd(g, z)>/dz      (w.r.t. z)
// where a tile owns all channels of a pixel; otherwise the conv into out_g and gs_pixel_norm_bwd_bwd_fused (out_g in place).
extern "C" int gs_conv_fwd_pnbwdbwd(const GsConv* c, const void* x, const float* w_hwio, const void* g, const void* z, int act, float eps, void* out_g, void* out_z,
                                    void* stream) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(g && z && out_g && out_z && (act == GS_ACT_NONE || act == GS_ACT_LRELU), "conv_fwd_pnbwdbwd: g, z and both outputs are required, activation none or leaky relu (got %d)", act);
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    if (c->ksize == 3 && igemm_supported(r.ICk, r.OCk, c->dtype))
        return run_igemm(r.mode, r.variant, x, w_hwio, out_g, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared, c->ws,
                         c->ws_bytes, as_stream(stream), z, act, out_z, eps, g, 2);
    if (int e = gs_conv_fwd(c, x, w_hwio, nullptr, GS_ACT_NONE, out_g, nullptr, 0.f, stream)) return e;
    return gs_pixel_norm_bwd_bwd_fused(out_g, g, z, out_z, out_g, (int64_t)c->n * r.Ho * r.Wo, c->co, eps, act, c->dtype, stream);
}
// 1 when that call runs as one launch for the layer
extern "C" int gs_conv_fwd_pnbwdbwd_is_fused(const GsConv* c) {
    if (check_conv(c) || c->ksize != 3 || !(c->transposed || c->stride == 1)) return 0;
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    return igemm_norm_fused(r.mode, c->n, r.Hb, r.Wb, r.ICk, r.OCk, c->dtype, IGEMM_NORM_BWD2) ? 1 : 0;
}

// Data gradient of a conv whose INPUT was y = pixel_norm(z), z = act(...) the previous block's activation (networks.py:41-93: every
// generator block ends conv -> leaky_relu -> pixel_norm), continued through that norm and activation in the conv's epilogue:
//   gx = (pixel_norm_bwd(B^T(gy, w), z) + addend) * act'(z)       (addend: optional second gradient into z, same shape)
// i.e. the gradient w.r.t. the previous block's pre-activation in ONE pass.  The epilogue form exists where a tile owns every channel of a
// pixel (the 32- / 64-channel layers -- where the bytes are); other shapes run the plain data gradient and gs_pixel_norm_bwd_fused in place.
extern "C" int gs_conv_bwd_data_pnbwd(const GsConv* c, const void* gy, const float* w_hwio, const void* z, const void* addend, int act, float eps, void* gx, void* stream) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(z && gx && (act == GS_ACT_NONE || act == GS_ACT_LRELU), "conv_bwd_data_pnbwd: z is required, activation none or leaky relu (got %d)", act);
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_BWD_DATA);
    const bool epilogue_map = c->transposed || c->stride == 1;   // (the stride-2 conv's data gradient, MODE_T2, has no norm epilogue)
    if (epilogue_map && c->ksize == 3 && igemm_supported(r.ICk, r.OCk, c->dtype))
        return run_igemm(r.mode, r.variant, gy, w_hwio, gx, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared, c->ws,
                         c->ws_bytes, st, z, act, nullptr, eps, addend, 1);
    if (c->stride == 1 && thin_expand_pnbwd_ok(c->ksize, r.ICk, r.OCk, c->dtype)) {   // the colour block (few -> many channels as a gradient): streaming, one pass
        const long total = (long)c->ci * c->co;
        if (c->ws_bytes < (size_t)total * 4) return fail(GS_ERR_WORKSPACE, "conv_bwd_data_pnbwd: workspace %zu < %zu", c->ws_bytes, (size_t)total * 4);
        float* wp = reinterpret_cast<float*>(c->ws);
        if (!c->w_prepared) {
            hipLaunchKernelGGL((weight_prep_kernel<float>), dim3(cdiv(total, 256)), dim3(256), 0, st, w_hwio, wp, 1, c->ci, c->co, 1);
            GS_CHECK_LAUNCH();
        }
        return run_thin_expand_pnbwd(gy, wp, z, addend, gx, (long)c->n * r.Ho * r.Wo, r.ICk, r.OCk, c->alpha, eps, act, c->dtype, st);
    }
    if (int e = gs_conv_bwd_data(c, gy, w_hwio, nullptr, 0, gx, stream)) return e;
    return gs_pixel_norm_bwd_fused(gx, z, addend, gx, (int64_t)c->n * r.Ho * r.Wo, c->ci, eps, GS_ACT_NONE, act, c->dtype, stream);
}
// 1 when the call above runs as ONE launch for the layer (the epilogue form), 0 when it is the conv + the norm's backward in place
extern "C" int gs_conv_bwd_data_pnbwd_is_fused(const GsConv* c) {
    if (check_conv(c) || !(c->transposed || c->stride == 1)) return 0;
    const ConvRole r = conv_role(*c, GS_CONV_BWD_DATA);
    if (c->ksize == 1) return thin_expand_pnbwd_ok(1, r.ICk, r.OCk, c->dtype) ? 1 : 0;
    return igemm_norm_fused(r.mode, c->n, r.Hb, r.Wb, r.ICk, r.OCk, c->dtype, IGEMM_NORM_BWD) ? 1 : 0;
}
// Which implicit-GEMM configuration a 3x3 layer runs with (kernel-role shape: hb x wb the base grid, ic -> oc the kernel's channels; mode 0 stride
// 1, 1 stride 2, 2 transposed; want: the epilogue asked for, 0 none, 1 pixel norm, 2 / 3 its first- / second-order backward).  Host arithmetic
// only -- no launch, no device needed.  out_cfg[10]: A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC, then 1 if that configuration is compiled.
extern "C" int gs_conv_igemm_config(int mode, int n, int hb, int wb, int ic, int oc, int dtype, int want, int* out_cfg) {
    return igemm_config(mode, n, hb, wb, ic, oc, dtype, want, out_cfg);
}
// Row `index` of the table of compiled implicit-GEMM kernels (conv_igemm.hip: GS_IGEMM_CONFIGS), for tests that want one case per kernel.  Host
// only.  out11: mode, bf16_only, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC; GS_ERR_ARG past the last row.
extern "C" int gs_conv_igemm_table(int index, int* out11) { return igemm_table(index, out11); }

// ---- what the weight-gradient entry points WOULD launch, asked without launching (host arithmetic on wgrad_plan / plan_jobs, the structs the
// launchers themselves read; no device needed: the CU count then defaults to 256).  tests/test_wgrad_cover_*.py key their cases by these answers.
static void layer_plan_ints(const GsConv& c, int* out) {   // c.n: images of all sources
    const ConvRole r = conv_role(c, GS_CONV_BWD_WEIGHT);
    const WgradPlan p = wgrad_plan(r.mode, c.ksize, c.dtype, c.n, r.Hb, r.Wb, r.ICk, r.OCk);
    const int v[GS_WGRAD_PLAN_INTS] = {p.family, p.mode, p.tw, p.ot, r.swapped, r.ICk, r.OCk, r.Hb, r.Wb, p.ntiles, p.nslices, p.fold, p.batch_lanes,
                                       p.fused_bias, p.tiles_x, p.tiles_y};
    memcpy(out, v, sizeof(v));
}
extern "C" int gs_conv_wgrad_plan(const GsConv* c, int* out) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(out != nullptr, "conv_wgrad_plan: no output");
    layer_plan_ints(*c, out);
    return 0;
}
extern "C" int gs_conv_wgrad_jobs_plan(const GsWgradJob* jobs, int njobs, int* out, int out_len) {
    GS_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs) && out && out_len >= 2, "conv_wgrad_jobs_plan: bad args");
    JobPlan plan;
    if (njobs > 0)
        if (int e = plan_jobs(jobs, njobs, plan)) return e;
    std::vector<int> v;
    v.push_back((int)plan.groups.size());
    v.push_back((int)plan.single.size());
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const SkGroup& g = plan.groups[gi].second;
        const int head[5] = {plan.groups[gi].first, g.njobs, g.total_units, g.total_runs, g.nblocks};
        v.insert(v.end(), head, head + 5);
        for (int j = 0; j < g.njobs; ++j) {
            const int row[5] = {plan.group_jobs[gi][j], g.job[j].unit_base, g.job[j].run_base, g.job[j].ntiles, g.job[j].nct};
            v.insert(v.end(), row, row + 5);
        }
    }
    for (size_t k = 0; k < plan.single.size(); ++k) {
        int row[2 + GS_WGRAD_PLAN_INTS] = {plan.single_src[k].first, plan.single_src[k].second};
        layer_plan_ints(job_conv(plan.single[k], job_total_images(plan.single[k])), row + 2);
        v.insert(v.end(), row, row + 2 + GS_WGRAD_PLAN_INTS);
    }
    if ((int)v.size() > out_len) return fail(GS_ERR_ARG, "conv_wgrad_jobs_plan: %d ints needed, room for %d", (int)v.size(), out_len);
    memcpy(out, v.data(), v.size() * sizeof(int));
    return (int)v.size();
}
