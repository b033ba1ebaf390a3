// Pitch classifier (reference networks.py:293-413, a pre-activation ResNet-34 with group normalisation and weight standardisation)
// for GANSynth.evaluate: the operators the GAN itself never uses.  Inference only; the 3x3 convs go through the implicit-GEMM family
// (gs_conv_fwd), the logits through gs_dense_fwd.  Every reduction here runs in a fixed order with no float
// atomics, so two runs on the same input are bit-identical.
#include <math.h>

#include "gs_common.h"
#include "gs_prof.h"
#include "classifier_shared.h"

namespace gs {

enum { PROF_STEM_POOL = 40, PROF_PROJ = 41, PROF_GN_STATS = 42, PROF_GN_APPLY = 43, PROF_HEAD = 44, PROF_WS = 45, PROF_POOL = 46 };

// value as the next kernel will read it back from a T buffer
template <typename T> __device__ inline float stored(float v);
template <> __device__ inline float stored<float>(float v) { return v; }
template <> __device__ inline float stored<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// ------------------------------------------------------------------------------------------ weight standardisation (ops.py:53-66)
// (classifier_shared.h: weight_std_block; a one-off per loaded weight set -- training standardises every weight in one launch,
// classifier_bwd.hip)
__global__ __launch_bounds__(WS_CH * WS_RL) void weight_std_kernel(const float* __restrict__ w, float* __restrict__ out, int fan, int co, float eps) {
    __shared__ double red[WS_CH * WS_RL];
    weight_std_block(w, out, nullptr, fan, co, eps, blockIdx.x, red);
}

// ------------------------------------------------------------------------------------------------------ stem conv + max pool
// conv 7x7 stride 2, 2 -> 64 channels, bias, TF SAME on an even input (2 rows / columns of zeros before, 3 after), then max pool
// 3x3 stride 2 SAME (0 before, 1 after, the padding never wins: -inf).  A block owns a tile of STEM_PR x STEM_PC pool outputs: it
// computes the (2 PR + 1) x (2 PC + 1) stem pixels under them into LDS (the last row / column is the neighbour tile's first: 1.29x
// recompute) and pools from there, so the stem output (4 MB per image in bf16) never goes to memory.  Lane = output channel; the 98
// weights of a channel stay in VGPRs, the input patch in LDS (every lane reads the same pair: a broadcast).  y_stem (optional)
// receives the stem pixels this tile owns, for tests.
constexpr int STEM_PR = 2, STEM_PC = 16;
constexpr int STEM_SR = 2 * STEM_PR + 1, STEM_SC = 2 * STEM_PC + 1;   // stem rows / columns a tile computes
constexpr int STEM_IR = 2 * STEM_SR + 5, STEM_IC = 2 * STEM_SC + 5;   // input rows / columns under them

template <typename T>
__global__ __launch_bounds__(256) void stem_pool_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                        T* __restrict__ y_stem, T* __restrict__ y_pool, int H, int W) {
    __shared__ float2 xin[STEM_IR * STEM_IC];
    __shared__ float st[STEM_SR * STEM_SC * 64];
    const int Hs = H / 2, Ws = W / 2, Hp = Hs / 2, Wp = Ws / 2;
    const int n = blockIdx.z, py0 = blockIdx.y * STEM_PR, px0 = blockIdx.x * STEM_PC;
    const int sy0 = 2 * py0, sx0 = 2 * px0;          // first stem pixel of the tile
    const int iy0 = 2 * sy0 - 2, ix0 = 2 * sx0 - 2;  // first input pixel under it (SAME: 2 before)
    const T* xn = x + (long)n * H * W * 2;
    for (int i = threadIdx.x; i < STEM_IR * STEM_IC; i += 256) {
        const int r = i / STEM_IC, c = i % STEM_IC;
        const int iy = iy0 + r, ix = ix0 + c;
        float2 v = make_float2(0.f, 0.f);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const T* p = xn + ((long)iy * W + ix) * 2;
            v = make_float2(DT<T>::ld(p), DT<T>::ld(p + 1));
        }
        xin[i] = v;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float wr[98];
#pragma unroll
    for (int k = 0; k < 98; ++k) wr[k] = w[k * 64 + lane];
    const float b = bias ? bias[lane] : 0.f;
    __syncthreads();
    for (int q = wv; q < STEM_SR * STEM_SC; q += 4) {
        const int ly = q / STEM_SC, lx = q % STEM_SC;
        const int sy = sy0 + ly, sx = sx0 + lx;
        float v = -INFINITY;
        if (sy < Hs && sx < Ws) {
            float acc = b;
#pragma unroll
            for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float2 xv = xin[(2 * ly + ky) * STEM_IC + 2 * lx + kx];
                    acc = fmaf(xv.x, wr[(ky * 7 + kx) * 2], acc);
                    acc = fmaf(xv.y, wr[(ky * 7 + kx) * 2 + 1], acc);
                }
            v = stored<T>(acc);
            if (y_stem && ly < 2 * STEM_PR && lx < 2 * STEM_PC) DT<T>::st(y_stem + (((long)n * Hs + sy) * Ws + sx) * 64 + lane, acc);
        }
        st[q * 64 + lane] = v;
    }
    __syncthreads();
    if (!y_pool) return;
    for (int q = wv; q < STEM_PR * STEM_PC; q += 4) {
        const int pr = q / STEM_PC, pc = q % STEM_PC;
        const int py = py0 + pr, px = px0 + pc;
        if (py >= Hp || px >= Wp) continue;
        float m = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, st[((2 * pr + dy) * STEM_SC + 2 * pc + dx) * 64 + lane]);
        DT<T>::st(y_pool + (((long)n * Hp + py) * Wp + px) * 64 + lane, m);
    }
}

// ------------------------------------------------------------------------------------------- standalone max pool (ops.py:308-316)
// 3x3 stride 2 SAME on an even input: window rows 2 oy .. 2 oy + 2 clipped to the input (the clipped row is padding that never wins)
template <typename T>
__global__ __launch_bounds__(256) void max_pool_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)n * Ho * Wo * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long p = i / C;
        const int ox = (int)(p % Wo); p /= Wo;
        const int oy = (int)(p % Ho);
        const int b = (int)(p / Ho);
        float m = -INFINITY;
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = 2 * oy + dy;
            if (iy >= H) break;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = 2 * ox + dx;
                if (ix >= W) break;
                m = fmaxf(m, DT<T>::ld(x + (((long)b * H + iy) * W + ix) * C + c));
            }
        }
        DT<T>::st(y + i, m);
    }
}

// ---------------------------------------------------------------------------------- 1x1 projection shortcut, stride 1 or 2
// y[n][oy][ox][:] = x[n][s oy][s ox][:] @ w[ci][co] (TF SAME pads nothing for a 1x1 kernel), no bias.  A GEMM of M = output pixels,
// K = ci, N = co on the VALU in 64 x 64 tiles, 4 x 4 outputs per thread, K staged through LDS 32 at a time (the projections are
// ~0.5 % of the network's flops).
template <typename T>
__global__ __launch_bounds__(256) void conv1x1_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y, int H, int W,
                                                      int CI, int CO, int stride, long M) {
    __shared__ float xs[32][64 + 4];
    __shared__ float wsm[32][64];
    const int Ho = H / stride, Wo = W / stride;
    const long m0 = (long)blockIdx.x * 64;
    const int n0 = blockIdx.y * 64;
    const int tm = threadIdx.x / 16, tn = threadIdx.x % 16;
    float acc[4][4] = {};
    // loader: thread -> (pixel row, 8 consecutive k)
    const int lr = threadIdx.x / 4, lk = (threadIdx.x % 4) * 8;
    const long m = m0 + lr;
    const T* src = nullptr;
    if (m < M) {
        const int ox = (int)(m % Wo);
        const long q = m / Wo;
        const int oy = (int)(q % Ho);
        const long b = q / Ho;
        src = x + ((b * H + (long)stride * oy) * W + (long)stride * ox) * CI;
    }
    for (int k0 = 0; k0 < CI; k0 += 32) {
        float v[8];
        if (src) { ld4(src + k0 + lk, *reinterpret_cast<float(*)[4]>(v)); ld4(src + k0 + lk + 4, *reinterpret_cast<float(*)[4]>(v + 4)); }
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xs[lk + e][lr] = v[e];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = threadIdx.x + e * 256;   // 2048 weights: 32 rows x 64 columns
            wsm[i / 64][i % 64] = w[(long)(k0 + i / 64) * CO + n0 + i % 64];
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&xs[k][tm * 4]);
            const float4 bb = *reinterpret_cast<const float4*>(&wsm[k][tn * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long mm = m0 + tm * 4 + i;
        if (mm < M) st4(y + mm * CO + n0 + tn * 4, acc[i]);
    }
}

// ---------------------------------------------------------------------------------------------- group normalisation (ops.py:120-146)
// Statistics per (image, group) over H * W * C / G values.  Pass 1: a block walks one slice of one image's pixels, every thread keeps
// a Welford (mean, M2) for its 4 channels, the threads of a group are merged (Chan) in a fixed order into one partial per (slice,
// group).  Pass 2: one thread per (image, group) merges the slices in order -> stats [n][G] = (mean, 1 / sqrt(var + eps)).
// ADD: x + addend is the value (the residual sum of a block), written to `sum` as it is read -- the sum is the next block's input and
// shortcut, so it is stored once, here, and the add has no pass of its own.
struct GnPart { float n, mean, m2; };

__device__ inline void chan_merge(float& na, float& ma, float& m2a, float nb, float mb, float m2b) {
    const float nn = na + nb;
    if (nb == 0.f) return;
    const float d = mb - ma;
    const float f = nb / nn;
    ma += d * f;
    m2a += m2b + d * d * na * f;
    na = nn;
}

template <typename T, bool ADD>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* __restrict__ x, const T* __restrict__ addend, T* __restrict__ sum,
                                                         GnPart* __restrict__ part, int HW, int C, int G, int S, int pps) {
    __shared__ float sm_mean[256 * 4], sm_m2[256 * 4], sm_n[256];
    const int cv = C / 4, R = 256 / cv;
    const int v4 = threadIdx.x % cv, r = threadIdx.x / cv;
    const int n = blockIdx.y, s = blockIdx.x;
    const int p0 = s * pps;
    const int p1 = min(HW, p0 + pps);
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    float k = 0.f;
    if (r < R) {
        for (int p = p0 + r; p < p1; p += R) {
            const long off = ((long)n * HW + p) * C + v4 * 4;
            float v[4];
            ld4(x + off, v);
            if constexpr (ADD) {
                float a[4];
                ld4(addend + off, a);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += a[e];
                st4(sum + off, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = stored<T>(v[e]);
            }
            k += 1.f;
            const float inv = 1.f / k;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[e] - mean[e];
                mean[e] += d * inv;
                m2[e] += d * (v[e] - mean[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sm_mean[threadIdx.x * 4 + e] = mean[e]; sm_m2[threadIdx.x * 4 + e] = m2[e]; }
    sm_n[threadIdx.x] = k;
    __syncthreads();
    if (threadIdx.x < G) {
        const int g = threadIdx.x, cg = C / G;
        float na = 0.f, ma = 0.f, m2a = 0.f;
        for (int rr = 0; rr < R; ++rr)
            for (int c = g * cg; c < (g + 1) * cg; ++c) {
                const int t = rr * cv + c / 4;
                chan_merge(na, ma, m2a, sm_n[t], sm_mean[t * 4 + (c & 3)], sm_m2[t * 4 + (c & 3)]);
            }
        part[((long)n * S + s) * G + g] = GnPart{na, ma, m2a};
    }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const GnPart* __restrict__ part, float* __restrict__ stats, int N, int G, int S, float eps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * G) return;
    const int n = i / G, g = i % G;
    float na = 0.f, ma = 0.f, m2a = 0.f;
    for (int s = 0; s < S; ++s) {
        const GnPart q = part[((long)n * S + s) * G + g];
        chan_merge(na, ma, m2a, q.n, q.mean, q.m2);
    }
    const float var = na > 0.f ? m2a / na : 0.f;
    stats[2 * i] = ma;
    stats[2 * i + 1] = 1.f / sqrtf(var + eps);
}

// y = [relu]((x - mean) * rstd * gamma + beta), 4 channels per thread
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, T* __restrict__ y, long nvec, int HW, int C, int G, int relu) {
    const int cv = C / 4, cg = C / G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const int c0 = (int)(i % cv) * 4;
        const long img = (i / cv) / HW;
        float v[4];
        ld4(x + i * 4, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            const float* sg = stats + (img * G + c / cg) * 2;
            const float sc = sg[1] * gamma[c];
            float t = (v[e] - sg[0]) * sc + beta[c];
            v[e] = relu ? fmaxf(t, 0.f) : t;
        }
        st4(y + i * 4, v);
    }
}

// head: features[n][c] = mean over the H * W pixels of relu(group_norm(x)); 64 channels per block (lane = channel), the 4 waves take
// every 4th pixel and their sums meet in LDS in wave order
template <typename T>
__global__ __launch_bounds__(256) void gn_relu_mean_kernel(const T* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ out, int HW, int C, int G) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.y, c = blockIdx.x * 64 + lane;
    const float* sg = stats + ((long)n * G + c / (C / G)) * 2;
    const float sc = sg[1] * gamma[c], sh = beta[c] - sg[0] * sc;
    float acc = 0.f;
    for (int p = wv; p < HW; p += 4) acc += fmaxf(fmaf(DT<T>::ld(x + ((long)n * HW + p) * C + c), sc, sh), 0.f);
    red[wv][lane] = acc;
    __syncthreads();
    if (wv == 0) out[(long)n * C + c] = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (float)HW;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_weight_standardize(const float* w, float* out, int fan_in, int co, float eps, void* stream) {
    GS_CHECK_ARG(w && out && fan_in > 0 && co > 0, "weight_standardize: bad args");
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, 5.0 * fan_in * co, 3.0 * fan_in * co * 4, PROF_WS, 1, 1, 1, fan_in, co, 0, 0);
    hipLaunchKernelGGL(weight_std_kernel, dim3(cdiv(co, WS_CH)), dim3(WS_CH * WS_RL), 0, st, w, out, fan_in, co, eps);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_resnet_stem_pool(const void* x, const float* w, const float* bias, void* y_stem, void* y_pool, int n, int h, int w_, int co,
                                   int dtype, void* stream) {
    GS_CHECK_ARG(x && w && (y_stem || y_pool), "resnet_stem_pool: x, w and an output are required");
    GS_CHECK_ARG(n > 0 && h > 0 && w_ > 0 && h % 4 == 0 && w_ % 4 == 0, "resnet_stem_pool: input %d x %d (positive multiples of 4)", h, w_);
    GS_CHECK_ARG(co == 64, "resnet_stem_pool: %d output channels (64)", co);
    GS_CHECK_ARG(n <= 65535, "resnet_stem_pool: batch %d", n);
    hipStream_t st = as_stream(stream);
    const int Hp = h / 4, Wp = w_ / 4;
    const double esz = dtype == GS_F32 ? 4.0 : 2.0;
    const double spx = (double)n * (h / 2) * (w_ / 2);
    ProfScope ps(st, 2.0 * 98 * 64 * spx, esz * ((double)n * h * w_ * 2 + (double)n * Hp * Wp * 64 + (y_stem ? spx * 64 : 0.0)) + 98 * 64 * 4,
                 PROF_STEM_POOL, n, Hp, Wp, 2, co, y_stem ? 1 : 0, y_pool ? 1 : 0);
    dim3 grid(cdiv(Wp, STEM_PC), cdiv(Hp, STEM_PR), n);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((stem_pool_kernel<T>), grid, dim3(256), 0, st, (const T*)x, w, bias, (T*)y_stem, (T*)y_pool, h, w_));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_max_pool2d(const void* x, void* y, int n, int h, int w, int c, int dtype, void* stream) {
    GS_CHECK_ARG(x && y && n > 0 && c > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "max_pool2d: bad args (even h, w)");
    hipStream_t st = as_stream(stream);
    const long total = (long)n * (h / 2) * (w / 2) * c;
    const double esz = dtype == GS_F32 ? 4.0 : 2.0;
    ProfScope ps(st, 9.0 * total, esz * ((double)n * h * w * c + total), PROF_POOL, n, h / 2, w / 2, c, c, 0, 0);
    long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((max_pool_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, (T*)y, n, h, w, c));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_conv1x1_fwd(const void* x, const float* w, void* y, int n, int h, int w_, int ci, int co, int stride, int dtype, void* stream) {
    GS_CHECK_ARG(x && w && y && n > 0 && h > 0 && w_ > 0, "conv1x1_fwd: bad args");
    GS_CHECK_ARG(stride == 1 || (stride == 2 && h % 2 == 0 && w_ % 2 == 0), "conv1x1_fwd: stride %d on %d x %d", stride, h, w_);
    GS_CHECK_ARG(ci % 32 == 0 && co % 64 == 0, "conv1x1_fwd: %d -> %d channels (multiples of 32 -> 64)", ci, co);
    GS_CHECK_ARG(dtype == GS_F32 || dtype == GS_BF16, "conv1x1_fwd: bad dtype %d", dtype);
    hipStream_t st = as_stream(stream);
    const long M = (long)n * (h / stride) * (w_ / stride);
    GS_CHECK_ARG((M + 63) / 64 < (1L << 31), "conv1x1_fwd: too many pixels");
    const double esz = dtype == GS_F32 ? 4.0 : 2.0;
    ProfScope ps(st, 2.0 * M * ci * co, esz * (double)M * (ci + co) + 4.0 * ci * co, PROF_PROJ, n, h / stride, w_ / stride, ci, co, stride, 0);
    dim3 grid((unsigned)cdiv(M, 64), co / 64);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv1x1_kernel<T>), grid, dim3(256), 0, st, (const T*)x, w, (T*)y, h, w_, ci, co, stride, M));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_group_norm_workspace_bytes(int n, int hw, int c, int groups) {
    if (n <= 0 || hw <= 0 || c < 4 || groups <= 0) return 0;
    int S, pps;
    gn_geometry(n, hw, c, &S, &pps);
    return (size_t)n * S * groups * sizeof(GnPart);
}

extern "C" int gs_group_norm_stats(const void* x, const void* addend, void* sum, float* stats, int n, int hw, int c, int groups, float eps,
                                   int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_gn(n, hw, c, groups, dtype)) return e;
    GS_CHECK_ARG(x && stats && (!addend || sum), "group_norm_stats: x, stats (and sum with an addend) are required");
    GS_CHECK_ARG(n <= 65535, "group_norm_stats: batch %d", n);
    int S, pps;
    gn_geometry(n, hw, c, &S, &pps);
    if (ws_bytes < gs_group_norm_workspace_bytes(n, hw, c, groups) || !ws) return fail(GS_ERR_WORKSPACE, "group_norm_stats: workspace too small (%zu)", ws_bytes);
    hipStream_t st = as_stream(stream);
    const double esz = dtype == GS_F32 ? 4.0 : 2.0, numel = (double)n * hw * c;
    ProfScope ps(st, (addend ? 6.0 : 5.0) * numel, esz * numel * (addend ? 3.0 : 1.0) + 8.0 * n * groups, PROF_GN_STATS, n, hw, 1, c, groups,
                 addend ? 1 : 0, 0);
    GnPart* part = reinterpret_cast<GnPart*>(ws);
    dim3 grid(S, n);
    if (addend) {
        GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gn_partial_kernel<T, true>), grid, dim3(256), 0, st, (const T*)x, (const T*)addend, (T*)sum,
                                                    part, hw, c, groups, S, pps));
    } else {
        GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gn_partial_kernel<T, false>), grid, dim3(256), 0, st, (const T*)x, (const T*)nullptr, (T*)nullptr,
                                                    part, hw, c, groups, S, pps));
    }
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(cdiv((long)n * groups, 256)), dim3(256), 0, st, part, stats, n, groups, S, eps);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_group_norm_apply(const void* x, const float* stats, const float* gamma, const float* beta, void* y, int n, int hw, int c, int groups,
                                   int relu, int dtype, void* stream) {
    if (int e = check_gn(n, hw, c, groups, dtype)) return e;
    GS_CHECK_ARG(x && stats && gamma && beta && y, "group_norm_apply: null argument");
    hipStream_t st = as_stream(stream);
    const long nvec = (long)n * hw * (c / 4);
    const double esz = dtype == GS_F32 ? 4.0 : 2.0, numel = (double)n * hw * c;
    ProfScope ps(st, 3.0 * numel, 2.0 * esz * numel, PROF_GN_APPLY, n, hw, 1, c, groups, relu, 0);
    long blocks = (nvec + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gn_apply_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, stats, gamma, beta, (T*)y,
                                                nvec, hw, c, groups, relu));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_group_norm_relu_mean(const void* x, const float* stats, const float* gamma, const float* beta, float* features, int n, int hw, int c,
                                       int groups, int dtype, void* stream) {
    if (int e = check_gn(n, hw, c, groups, dtype)) return e;
    GS_CHECK_ARG(x && stats && gamma && beta && features, "group_norm_relu_mean: null argument");
    GS_CHECK_ARG(c % 64 == 0 && n <= 65535, "group_norm_relu_mean: %d channels (a multiple of 64), batch %d", c, n);
    hipStream_t st = as_stream(stream);
    const double esz = dtype == GS_F32 ? 4.0 : 2.0, numel = (double)n * hw * c;
    ProfScope ps(st, 3.0 * numel, esz * numel + 4.0 * n * c, PROF_HEAD, n, hw, 1, c, groups, 0, 0);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gn_relu_mean_kernel<T>), dim3(c / 64, n), dim3(256), 0, st, (const T*)x, stats, gamma, beta, features,
                                                hw, c, groups));
    GS_CHECK_LAUNCH();
    return 0;
}
