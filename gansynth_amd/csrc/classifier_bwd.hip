// Training the pitch classifier (reference models.py:253-299): the backward of the operators of classifier.hip, softmax cross-entropy
// and TF's momentum update.  The 3x3 convs and the logits layer go through gs_conv_bwd_data / gs_conv_bwd_weight /
// gs_dense_bwd_* on the standardised weights with alpha = 1.  Every reduction runs in a fixed order with no float atomics: two runs
// on the same input are bit-identical, as the forward is.
#include <math.h>

#include "gs_common.h"
#include "gs_prof.h"
#include "classifier_shared.h"

namespace gs {

enum { PROF_GN_BWD = 50, PROF_HEAD_BWD = 51, PROF_WS_BATCH = 52, PROF_WS_BWD = 53, PROF_POOL_BWD = 54, PROF_STEM_WGRAD = 55,
       PROF_PROJ_BWD_DATA = 56, PROF_PROJ_BWD_WEIGHT = 57, PROF_XENT = 58, PROF_MOMENTUM = 59 };

// ------------------------------------------------------------------------------------------------- fold of split-K partials
// out[i] (+)= sum_s part[s][i], i < N: 64 elements per block, 4 slice lanes each (s = lane, lane + 4, ... in order), the lanes meet in
// LDS as (0 + 1) + (2 + 3).  The first n1 elements go to out1, the rest to out2 (a weight gradient and its bias gradient).
__global__ __launch_bounds__(256) void fold_partials_kernel(const float* __restrict__ part, int S, long N, float* __restrict__ out1, long n1,
                                                            float* __restrict__ out2, int accumulate) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + e;
    float a = 0.f;
    if (i < N)
        for (int s = sl; s < S; s += 4) a += part[(long)s * N + i];
    red[sl][e] = a;
    __syncthreads();
    if (sl == 0 && i < N) {
        const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        float* dst = i < n1 ? out1 + i : out2 + (i - n1);
        *dst = accumulate ? *dst + v : v;
    }
}

static void launch_fold(const float* part, int S, long N, float* out1, long n1, float* out2, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(fold_partials_kernel, dim3(cdiv(N, 64)), dim3(256), 0, st, part, S, N, out1, n1, out2, accumulate);
}

// -------------------------------------------------------------------------------------- group norm + ReLU backward (ops.py:120-146)
// y = relu(gamma xh + beta), xh = (x - mean) rstd per (image, group).  With g' = gy [gamma xh + beta > 0] (the mask recomputed with
// the forward's own expression):
//   dbeta = sum g', dgamma = sum g' xh,  dx = rstd (gamma g' - mean_g(gamma g') - xh mean_g(gamma g' xh)) [+ addend]
// Pass 1 (gnb_partial): a block walks one slice of one image's pixels (the slices of the statistics), a thread sums g' and g' xh for
//   its 4 channels, the pixel rows of the block meet in an LDS tree -> part [n][S][c][2].
// Pass 2 (gnb_finalize): per (image, 64 channels) the slices are merged (4 lanes, then a tree) -> chs [n][c][2]; contracted with gamma
//   over a group's channels -> gm [n][G][2], the two group means.
// Pass 3 (gnb_param): dgamma, dbeta = chs folded over the images in order.
// Pass 4 (gnb_dx): the element-wise formula; `addend` is the identity-shortcut gradient of a pre-activation block, so the residual
//   add needs no pass of its own in the backward either.
// HEAD: the upstream gradient is d features [n][c] / HW at every pixel (the backward of gs_group_norm_relu_mean) and the mask uses that
// kernel's expression.
template <typename T, bool HEAD>
__global__ __launch_bounds__(256) void gnb_partial_kernel(const T* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const T* __restrict__ gy, const float* __restrict__ gf,
                                                          float* __restrict__ part, int HW, int C, int G, int S, int pps, float inv_hw) {
    __shared__ float sm[256 * 8];
    const int cv = C / 4, R = 256 / cv, cg = C / G;   // (cv * R == 256: both powers of two)
    const int v4 = threadIdx.x % cv, r = threadIdx.x / cv;
    const int n = blockIdx.y, s = blockIdx.x;
    const int p0 = s * pps;
    const int p1 = min(HW, p0 + pps);
    const int c0 = v4 * 4;
    float mean[4], rstd[4], sc[4], bt[4], gh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = c0 + e;
        const float* sg = stats + ((long)n * G + c / cg) * 2;
        mean[e] = sg[0];
        rstd[e] = sg[1];
        sc[e] = sg[1] * gamma[c];
        bt[e] = HEAD ? beta[c] - sg[0] * sc[e] : beta[c];
        gh[e] = HEAD ? gf[(long)n * C + c] * inv_hw : 0.f;
    }
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = p0 + r; p < p1; p += R) {
        const long off = ((long)n * HW + p) * C + c0;
        float v[4], g[4];
        ld4(x + off, v);
        if constexpr (!HEAD) ld4(gy + off, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = HEAD ? fmaf(v[e], sc[e], bt[e]) : (v[e] - mean[e]) * sc[e] + bt[e];
            const float gp = t > 0.f ? (HEAD ? gh[e] : g[e]) : 0.f;
            s1[e] += gp;
            s2[e] += gp * ((v[e] - mean[e]) * rstd[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sm[threadIdx.x * 8 + e] = s1[e]; sm[threadIdx.x * 8 + 4 + e] = s2[e]; }
    __syncthreads();
    for (int h = R / 2; h > 0; h >>= 1) {
        if (r < h)
#pragma unroll
            for (int k = 0; k < 8; ++k) sm[threadIdx.x * 8 + k] += sm[(threadIdx.x + h * cv) * 8 + k];
        __syncthreads();
    }
    if (r == 0) {
        float* dst = part + (((long)n * S + s) * C + c0) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { dst[2 * e] = sm[threadIdx.x * 8 + e]; dst[2 * e + 1] = sm[threadIdx.x * 8 + 4 + e]; }
    }
}

__global__ __launch_bounds__(256) void gnb_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma, float* __restrict__ chs,
                                                           float* __restrict__ gm, int HW, int C, int G, int S) {
    __shared__ float r1[4][64], r2[4][64];
    const int ch = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int n = blockIdx.y, cb = blockIdx.x * 64, c = cb + ch;
    const bool ok = c < C;
    float a = 0.f, b = 0.f;
    if (ok)
        for (int s = sl; s < S; s += 4) {
            const float2 q = *reinterpret_cast<const float2*>(part + (((long)n * S + s) * C + c) * 2);
            a += q.x;
            b += q.y;
        }
    r1[sl][ch] = a;
    r2[sl][ch] = b;
    __syncthreads();
    if (sl == 0) {
        a = (r1[0][ch] + r1[1][ch]) + (r1[2][ch] + r1[3][ch]);
        b = (r2[0][ch] + r2[1][ch]) + (r2[2][ch] + r2[3][ch]);
        if (ok) { chs[((long)n * C + c) * 2] = a; chs[((long)n * C + c) * 2 + 1] = b; }
        const float gmm = ok ? gamma[c] : 0.f;
        r1[1][ch] = gmm * a;
        r2[1][ch] = gmm * b;
    }
    __syncthreads();
    const int cg = C / G;                          // <= 64 (checked by the entry point)
    const int here = (C < 64 ? C : 64) / cg;       // groups of this block
    if (threadIdx.x < here) {
        float u = 0.f, w = 0.f;
        for (int k = 0; k < cg; ++k) { u += r1[1][threadIdx.x * cg + k]; w += r2[1][threadIdx.x * cg + k]; }
        const float inv = 1.f / ((float)cg * (float)HW);
        const int g = cb / cg + threadIdx.x;
        gm[((long)n * G + g) * 2] = u * inv;
        gm[((long)n * G + g) * 2 + 1] = w * inv;
    }
}

__global__ __launch_bounds__(256) void gnb_param_kernel(const float* __restrict__ chs, float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int C,
                                                        int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, b = 0.f;
    for (int n = 0; n < N; ++n) { a += chs[((long)n * C + c) * 2]; b += chs[((long)n * C + c) * 2 + 1]; }
    dbeta[c] = accumulate ? dbeta[c] + a : a;
    dgamma[c] = accumulate ? dgamma[c] + b : b;
}

template <typename T, bool HEAD>
__global__ __launch_bounds__(256) void gnb_dx_kernel(const T* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const T* __restrict__ gy, const float* __restrict__ gf,
                                                     const float* __restrict__ gm, const T* __restrict__ addend, T* __restrict__ dx, long nvec, int HW,
                                                     int C, int G, float inv_hw) {
    const int cv = C / 4, cg = C / G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const int c0 = (int)(i % cv) * 4;
        const long img = (i / cv) / HW;
        float v[4], g[4], a[4], o[4];
        ld4(x + i * 4, v);
        if constexpr (!HEAD) ld4(gy + i * 4, g);
        if (addend) ld4(addend + i * 4, a);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            const float* sg = stats + (img * G + c / cg) * 2;
            const float* mg = gm + (img * G + c / cg) * 2;
            const float sc = sg[1] * gamma[c];
            const float t = HEAD ? fmaf(v[e], sc, beta[c] - sg[0] * sc) : (v[e] - sg[0]) * sc + beta[c];
            const float up = HEAD ? gf[img * C + c] * inv_hw : g[e];
            const float gp = t > 0.f ? up : 0.f;
            const float xh = (v[e] - sg[0]) * sg[1];
            float d = sg[1] * (gamma[c] * gp - mg[0] - xh * mg[1]);
            if (addend) d += a[e];
            o[e] = d;
        }
        st4(dx + i * 4, o);
    }
}

static size_t gn_bwd_ws_floats(int n, int hw, int c, int groups) {
    int S, pps;
    gn_geometry(n, hw, c, &S, &pps);
    return ((size_t)n * S * c + (size_t)n * c + (size_t)n * groups) * 2;
}

template <bool HEAD>
static int gn_bwd_launch(const void* x, const float* stats, const float* gamma, const float* beta, const void* gy, const float* gf, const void* addend,
                         void* dx, float* dgamma, float* dbeta, int n, int hw, int c, int groups, int accumulate, int dtype, void* ws, size_t ws_bytes,
                         void* stream) {
    if (int e = check_gn(n, hw, c, groups, dtype)) return e;
    GS_CHECK_ARG(x && stats && gamma && beta && (HEAD ? (const void*)gf : gy) && dx && dgamma && dbeta, "group_norm_relu_bwd: null argument");
    GS_CHECK_ARG(c / groups <= 64 && n <= 65535, "group_norm_relu_bwd: %d channels per group (at most 64), batch %d", c / groups, n);
    if (!ws || ws_bytes < gn_bwd_ws_floats(n, hw, c, groups) * sizeof(float)) return fail(GS_ERR_WORKSPACE, "group_norm_relu_bwd: workspace too small (%zu)", ws_bytes);
    int S, pps;
    gn_geometry(n, hw, c, &S, &pps);
    float* part = reinterpret_cast<float*>(ws);
    float* chs = part + (size_t)n * S * c * 2;
    float* gm = chs + (size_t)n * c * 2;
    hipStream_t st = as_stream(stream);
    const double esz = dtype == GS_F32 ? 4.0 : 2.0, numel = (double)n * hw * c;
    // x twice, gy twice (once for the head: it has none), the addend, dx
    ProfScope ps(st, 16.0 * numel, esz * numel * ((HEAD ? 3.0 : 5.0) + (addend ? 1.0 : 0.0)), HEAD ? PROF_HEAD_BWD : PROF_GN_BWD, n, hw, 1, c, groups,
                 addend ? 1 : 0, 0);
    const float inv_hw = 1.f / (float)hw;
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gnb_partial_kernel<T, HEAD>), dim3(S, n), dim3(256), 0, st, (const T*)x, stats, gamma, beta, (const T*)gy, gf,
                                                part, hw, c, groups, S, pps, inv_hw));
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(gnb_finalize_kernel, dim3(cdiv(c, 64), n), dim3(256), 0, st, part, gamma, chs, gm, hw, c, groups, S);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(gnb_param_kernel, dim3(cdiv(c, 256)), dim3(256), 0, st, chs, dgamma, dbeta, n, c, accumulate);
    GS_CHECK_LAUNCH();
    const long nvec = (long)n * hw * (c / 4);
    long blocks = (nvec + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gnb_dx_kernel<T, HEAD>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, stats, gamma, beta,
                                                (const T*)gy, gf, gm, (const T*)addend, (T*)dx, nvec, hw, c, groups, inv_hw));
    GS_CHECK_LAUNCH();
    return 0;
}

// --------------------------------------------------------------------------------- weight standardisation, every weight in one launch
// blockIdx.y = weight (a row of the descriptor table in device memory), blockIdx.x = block of WS_CH channels (blocks past a narrow
// weight's channels leave at once).  Forward: weight_std_block, the body of gs_weight_standardize (bit-identical), and 1 / sqrt(var + eps)
// per channel for the backward.  Backward, per output channel over the fan_in rows:
//   dW = (dWh - mean(dWh) - Wh mean(dWh Wh)) rstd;  dWh is cleared behind the read (the next step's convs add into it from zero).
__global__ __launch_bounds__(WS_CH * WS_RL) void weight_std_batch_kernel(const GsWsDesc* __restrict__ descs, float eps) {
    __shared__ double red[WS_CH * WS_RL];
    const GsWsDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x * WS_CH >= d.co) return;
    weight_std_block(d.w, d.out, d.rstd, d.fan_in, d.co, eps, blockIdx.x, red);
}

__global__ __launch_bounds__(WS_CH * WS_RL) void weight_std_bwd_batch_kernel(const GsWsDesc* __restrict__ descs) {
    __shared__ double red[WS_CH * WS_RL];
    const GsWsDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x * WS_CH >= d.co) return;
    const int ch = threadIdx.x % WS_CH, rl = threadIdx.x / WS_CH;
    const int c = blockIdx.x * WS_CH + ch, fan = d.fan_in, co = d.co;
    const bool ok = c < co;
    double s1 = 0.0, s2 = 0.0;
    if (ok)
        for (int i = rl; i < fan; i += WS_RL) {
            const double g = d.gout[(long)i * co + c];
            s1 += g;
            s2 += g * d.out[(long)i * co + c];
        }
    const double m1 = ws_block_sum(s1, red) / fan;
    const double m2 = ws_block_sum(s2, red) / fan;
    if (ok) {
        const double r = d.rstd[c];
        for (int i = rl; i < fan; i += WS_RL) {
            const long o = (long)i * co + c;
            d.gw[o] = (float)((d.gout[o] - m1 - d.out[o] * m2) * r);
            d.gout[o] = 0.f;
        }
    }
}

// -------------------------------------------------------------------------------------------- max pool backward (ops.py:308-316)
// 3x3 stride 2, TF SAME on any h, w (pad total max((ceil(n / 2) - 1) 2 + 3 - n, 0), the smaller half before: 0 / 1 on an even size,
// 1 / 1 on an odd one).  Gather form: a thread owns one input element, visits the (at most 2 x 2) windows that contain it, finds each
// window's first maximum in row-major order and takes the window's gradient when that is its own element.
template <typename T>
__global__ __launch_bounds__(256) void max_pool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ gx, int n, int H, int W, int C) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int ph = max((Ho - 1) * 2 + 3 - H, 0) / 2, pw = max((Wo - 1) * 2 + 3 - W, 0) / 2;
    const long total = (long)n * H * W * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long p = i / C;
        const int ix = (int)(p % W); p /= W;
        const int iy = (int)(p % H);
        const long b = p / H;
        const T* xb = x + b * H * W * C + c;
        const int ty = iy + ph, tx = ix + pw;
        const int oy0 = max(0, (ty - 1) / 2), oy1 = min(Ho - 1, ty / 2);
        const int ox0 = max(0, (tx - 1) / 2), ox1 = min(Wo - 1, tx / 2);
        float acc = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                float best = -INFINITY;
                int by = -1, bx = -1;
                for (int dy = 0; dy < 3; ++dy) {
                    const int yy = 2 * oy - ph + dy;
                    if (yy < 0 || yy >= H) continue;
                    for (int dx = 0; dx < 3; ++dx) {
                        const int xx = 2 * ox - pw + dx;
                        if (xx < 0 || xx >= W) continue;
                        const float v = DT<T>::ld(xb + ((long)yy * W + xx) * C);
                        if (v > best) { best = v; by = yy; bx = xx; }
                    }
                }
                if (by == iy && bx == ix) acc += DT<T>::ld(gy + ((b * Ho + oy) * Wo + ox) * C + c);
            }
        DT<T>::st(gx + i, acc);
    }
}

// ------------------------------------------------------------------------------------------------- stem weight gradient
// dW [7][7][2][64] = sum over n, stem pixels of x patch (x) g, db [64] = sum g: a GEMM of M = 98, N = 64, K = n * (h / 2) * (w / 2)
// on the fp32 VALU.  Lane = output channel, the 98 (+ 1 bias) accumulators of a channel stay in VGPRs; a block walks tiles of one stem
// row x STEMB_TW columns (tile b, b + blocks, ...: split K), the input patch of a tile goes through LDS (every lane reads the same pair:
// a broadcast), each of the 4 waves takes every 4th pixel.  The waves' sums meet in LDS in wave order -> one partial per block, folded
// by fold_partials_kernel.
constexpr int STEMB_TW = 32, STEMB_IC = 2 * STEMB_TW + 5, STEMB_MAXB = 1024;

template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ gs_, float* __restrict__ part, int N, int H, int W,
                                                         int ntiles) {
    __shared__ float2 xin[7 * STEMB_IC];
    __shared__ float red[99 * 64];
    const int Hs = H / 2, Ws = W / 2, tiles_x = (Ws + STEMB_TW - 1) / STEMB_TW;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc[98];
#pragma unroll
    for (int k = 0; k < 98; ++k) acc[k] = 0.f;
    float accb = 0.f;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = t % tiles_x;
        const int q = t / tiles_x;
        const int sy = q % Hs, n = q / Hs;
        const int sx0 = tx * STEMB_TW;
        const int iy0 = 2 * sy - 2, ix0 = 2 * sx0 - 2;   // SAME on an even input: 2 before
        const T* xn = x + (long)n * H * W * 2;
        __syncthreads();   // (the previous tile's readers are done)
        for (int i = threadIdx.x; i < 7 * STEMB_IC; i += 256) {
            const int r = i / STEMB_IC, c = i % STEMB_IC;
            const int iy = iy0 + r, ix = ix0 + c;
            float2 v = make_float2(0.f, 0.f);
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                const T* p = xn + ((long)iy * W + ix) * 2;
                v = make_float2(DT<T>::ld(p), DT<T>::ld(p + 1));
            }
            xin[i] = v;
        }
        __syncthreads();
        for (int lx = wv; lx < STEMB_TW; lx += 4) {
            const int sx = sx0 + lx;
            if (sx >= Ws) break;
            const float g = DT<T>::ld(gs_ + (((long)n * Hs + sy) * Ws + sx) * 64 + lane);
            accb += g;
#pragma unroll
            for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float2 xv = xin[ky * STEMB_IC + 2 * lx + kx];
                    acc[(ky * 7 + kx) * 2] = fmaf(xv.x, g, acc[(ky * 7 + kx) * 2]);
                    acc[(ky * 7 + kx) * 2 + 1] = fmaf(xv.y, g, acc[(ky * 7 + kx) * 2 + 1]);
                }
        }
    }
    for (int w = 1; w < 4; ++w) {   // waves 1, 2, 3 added into wave 0, in this order
        __syncthreads();
        if (wv == w) {
#pragma unroll
            for (int k = 0; k < 98; ++k) red[k * 64 + lane] = acc[k];
            red[98 * 64 + lane] = accb;
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int k = 0; k < 98; ++k) acc[k] += red[k * 64 + lane];
            accb += red[98 * 64 + lane];
        }
    }
    if (wv == 0) {
        float* dst = part + (long)blockIdx.x * 99 * 64;
#pragma unroll
        for (int k = 0; k < 98; ++k) dst[k * 64 + lane] = acc[k];
        dst[98 * 64 + lane] = accb;
    }
}

static int stem_wgrad_blocks(int n, int h, int w) {
    const long tiles = (long)n * (h / 2) * cdiv(w / 2, STEMB_TW);
    return (int)(tiles < STEMB_MAXB ? tiles : STEMB_MAXB);
}

// ------------------------------------------------------------------------------------ 1x1 projection backward, stride 1 or 2
// Data: gx[n][s oy][s ox][:] (+)= gy[n][oy][ox][:] @ w^T -- the forward's 64 x 64 tiles with the weight read transposed and the result
// rows written to (added into) the sampled pixels; every gx element belongs to one thread.
template <typename T>
__global__ __launch_bounds__(256) void conv1x1_bwd_data_kernel(const T* __restrict__ gy, const float* __restrict__ w, T* __restrict__ gx, int H, int W,
                                                               int CI, int CO, int stride, long M, int accumulate) {
    __shared__ float xs[32][64 + 4];
    __shared__ float wsm[32][64 + 1];
    const int Ho = H / stride, Wo = W / stride;
    const long m0 = (long)blockIdx.x * 64;
    const int n0 = blockIdx.y * 64;   // first input channel of the tile
    const int tm = threadIdx.x / 16, tn = threadIdx.x % 16;
    float acc[4][4] = {};
    const int lr = threadIdx.x / 4, lk = (threadIdx.x % 4) * 8;
    const long m = m0 + lr;
    const T* src = m < M ? gy + m * CO : nullptr;
    for (int k0 = 0; k0 < CO; k0 += 32) {
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
            const int i = threadIdx.x + e * 256;   // 2048 weights: 64 input channels x 32 output channels, k fastest (contiguous in w)
            wsm[i % 32][i / 32] = w[(long)(n0 + i / 32) * CO + k0 + i % 32];
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&xs[k][tm * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w};
            float bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = wsm[k][tn * 4 + j];
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
        if (mm >= M) continue;
        const int ox = (int)(mm % Wo);
        const long q = mm / Wo;
        const int oy = (int)(q % Ho);
        const long b = q / Ho;
        T* dst = gx + ((b * H + (long)stride * oy) * W + (long)stride * ox) * CI + n0 + tn * 4;
        if (accumulate) {
            float o[4];
            ld4(dst, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += acc[i][j];
            st4(dst, o);
        } else {
            st4(dst, acc[i]);
        }
    }
}

// Weight: dW [ci][co] = sum_m x[pixel(m)][ci] gy[m][co], a GEMM with K = M output pixels: 64 x 64 tiles of dW, the pixels split over
// blockIdx.z (rows_per_split each, a multiple of 32), 32 pixels at a time through LDS -> part [split][ci][co], folded in order.
template <typename T>
__global__ __launch_bounds__(256) void conv1x1_bwd_weight_kernel(const T* __restrict__ x, const T* __restrict__ gy, float* __restrict__ part, int H, int W,
                                                                 int CI, int CO, int stride, long M, long rows_per_split) {
    __shared__ float xs[32][64];
    __shared__ float gsm[32][64];
    const int Ho = H / stride, Wo = W / stride;
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const long mb = (long)blockIdx.z * rows_per_split;
    const long me = mb + rows_per_split < M ? mb + rows_per_split : M;
    const int tm = threadIdx.x / 16, tn = threadIdx.x % 16;
    const int lr = threadIdx.x / 8, lc = (threadIdx.x % 8) * 8;
    float acc[4][4] = {};
    for (long mc = mb; mc < me; mc += 32) {
        const long m = mc + lr;
        float a[8], g[8];
        if (m < me) {
            const int ox = (int)(m % Wo);
            const long q = m / Wo;
            const int oy = (int)(q % Ho);
            const long b = q / Ho;
            const T* xp = x + ((b * H + (long)stride * oy) * W + (long)stride * ox) * CI + i0 + lc;
            const T* gp = gy + m * CO + j0 + lc;
            ld4(xp, *reinterpret_cast<float(*)[4]>(a)); ld4(xp + 4, *reinterpret_cast<float(*)[4]>(a + 4));
            ld4(gp, *reinterpret_cast<float(*)[4]>(g)); ld4(gp + 4, *reinterpret_cast<float(*)[4]>(g + 4));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { a[e] = 0.f; g[e] = 0.f; }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) { xs[lr][lc + e] = a[e]; gsm[lr][lc + e] = g[e]; }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const float4 av4 = *reinterpret_cast<const float4*>(&xs[k][tm * 4]);
            const float4 bv4 = *reinterpret_cast<const float4*>(&gsm[k][tn * 4]);
            const float av[4] = {av4.x, av4.y, av4.z, av4.w}, bv[4] = {bv4.x, bv4.y, bv4.z, bv4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
    }
    float* dst = part + (long)blockIdx.z * CI * CO;
#pragma unroll
    for (int i = 0; i < 4; ++i) st4(dst + (long)(i0 + tm * 4 + i) * CO + j0 + tn * 4, acc[i]);
}

static void conv1x1_wgrad_split(long M, int ci, int co, int* splits, long* rows) {
    const int tiles = (ci / 64) * (co / 64);
    long ks = 512 / tiles;
    if (ks < 1) ks = 1;
    const long chunks = (M + 31) / 32;
    if (ks > chunks) ks = chunks;
    *rows = ((chunks + ks - 1) / ks) * 32;
    *splits = (int)((M + *rows - 1) / *rows);
}

// ------------------------------------------------------------------------------------------------------ softmax cross-entropy
// tf.losses.softmax_cross_entropy (mean over the batch) + its gradient + the count of rows whose argmax matches the labels' (first
// maximum, as tf.argmax), one block: a thread walks whole rows, the row losses meet in an LDS tree in double.  Sized for a training
// batch: up to 256 rows it is one row per thread and latency-bound (40 us at 64 x 61); beyond that the time grows with n / 256.
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits, const float* __restrict__ labels, float* __restrict__ loss,
                                                           float* __restrict__ dlogits, int* __restrict__ correct, int N, int C) {
    __shared__ double rl[256];
    __shared__ int rc[256];
    double lsum = 0.0;
    int hits = 0;
    const float inv_n = 1.f / (float)N;
    for (int r = threadIdx.x; r < N; r += 256) {
        const float* z = logits + (long)r * C;
        const float* y = labels + (long)r * C;
        float zmax = -INFINITY, ymax = -INFINITY;
        int zi = 0, yi = 0;
        for (int c = 0; c < C; ++c) {
            if (z[c] > zmax) { zmax = z[c]; zi = c; }
            if (y[c] > ymax) { ymax = y[c]; yi = c; }
        }
        float se = 0.f, ysum = 0.f, yz = 0.f;
        for (int c = 0; c < C; ++c) {
            se += expf(z[c] - zmax);
            ysum += y[c];
            yz += y[c] * (z[c] - zmax);
        }
        const float lse = logf(se);
        lsum += (double)(lse * ysum - yz);
        hits += zi == yi ? 1 : 0;
        if (dlogits) {
            const float inv = 1.f / se;
            for (int c = 0; c < C; ++c) dlogits[(long)r * C + c] = (expf(z[c] - zmax) * inv * ysum - y[c]) * inv_n;
        }
    }
    rl[threadIdx.x] = lsum;
    rc[threadIdx.x] = hits;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { rl[threadIdx.x] += rl[threadIdx.x + h]; rc[threadIdx.x] += rc[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(rl[0] / N);
        correct[0] = rc[0];
    }
}

// ------------------------------------------------------------------------------ tf.train.MomentumOptimizer over a flat fp32 buffer
// One pass: g += wd v on [decay_lo, decay_hi) (the L2 term of the loss), accum = momentum accum + g, then
//   Nesterov: v -= lr g + lr momentum accum;  plain: v -= lr accum;   g cleared behind it when zero_grad.
// The same pass sums v^2 of the decayed range at the PRE-update values (double, per thread, then a block tree) -> one partial per block;
// a one-block launch adds the partials in a tree -> l2[0] = sum v^2 / 2.  4 elements per thread and step.
constexpr int MOM_MAXB = 1024;

__global__ __launch_bounds__(256) void momentum_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ accum, long n4, long lo, long hi,
                                                       float wd, float lr, float momentum, int nesterov, int zero_grad, double* __restrict__ partial) {
    __shared__ double red[256];
    double sq = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float v[4], gr[4], a[4];
        ld4(p + i * 4, v);
        ld4(g + i * 4, gr);
        ld4(accum + i * 4, a);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = i * 4 + e;
            if (k >= lo && k < hi) {
                sq += (double)v[e] * (double)v[e];
                gr[e] = fmaf(wd, v[e], gr[e]);
            }
            a[e] = fmaf(momentum, a[e], gr[e]);
            v[e] -= nesterov ? lr * gr[e] + lr * momentum * a[e] : lr * a[e];
            gr[e] = 0.f;
        }
        st4(p + i * 4, v);
        st4(accum + i * 4, a);
        if (zero_grad) st4(g + i * 4, gr);
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void momentum_l2_kernel(const double* __restrict__ partial, int nb, float* __restrict__ l2) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) l2[0] = (float)(0.5 * red[0]);
}

static int momentum_blocks(int64_t n) {
    const long b = (n / 4 + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > MOM_MAXB ? MOM_MAXB : b));
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_group_norm_bwd_workspace_bytes(int n, int hw, int c, int groups) {
    if (n <= 0 || hw <= 0 || c < 4 || groups <= 0) return 0;
    return gn_bwd_ws_floats(n, hw, c, groups) * sizeof(float);
}

extern "C" int gs_group_norm_relu_bwd(const void* x, const float* stats, const float* gamma, const float* beta, const void* gy, const void* addend, void* dx,
                                      float* dgamma, float* dbeta, int n, int hw, int c, int groups, int accumulate, int dtype, void* ws, size_t ws_bytes,
                                      void* stream) {
    return gn_bwd_launch<false>(x, stats, gamma, beta, gy, nullptr, addend, dx, dgamma, dbeta, n, hw, c, groups, accumulate, dtype, ws, ws_bytes, stream);
}

extern "C" int gs_group_norm_relu_mean_bwd(const void* x, const float* stats, const float* gamma, const float* beta, const float* gfeatures, void* dx,
                                           float* dgamma, float* dbeta, int n, int hw, int c, int groups, int accumulate, int dtype, void* ws,
                                           size_t ws_bytes, void* stream) {
    return gn_bwd_launch<true>(x, stats, gamma, beta, nullptr, gfeatures, nullptr, dx, dgamma, dbeta, n, hw, c, groups, accumulate, dtype, ws, ws_bytes,
                               stream);
}

extern "C" int gs_weight_standardize_batch(const GsWsDesc* descs, int n, int max_co, float eps, void* stream) {
    GS_CHECK_ARG(descs && n > 0 && n <= 65535 && max_co > 0, "weight_standardize_batch: bad args");
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, 0.0, 0.0, PROF_WS_BATCH, n, 1, 1, 0, max_co, 0, 0);
    hipLaunchKernelGGL(weight_std_batch_kernel, dim3(cdiv(max_co, WS_CH), n), dim3(WS_CH * WS_RL), 0, st, descs, eps);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_weight_standardize_bwd_batch(const GsWsDesc* descs, int n, int max_co, void* stream) {
    GS_CHECK_ARG(descs && n > 0 && n <= 65535 && max_co > 0, "weight_standardize_bwd_batch: bad args");
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, 0.0, 0.0, PROF_WS_BWD, n, 1, 1, 0, max_co, 0, 0);
    hipLaunchKernelGGL(weight_std_bwd_batch_kernel, dim3(cdiv(max_co, WS_CH), n), dim3(WS_CH * WS_RL), 0, st, descs);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_max_pool2d_bwd(const void* x, const void* gy, void* gx, int n, int h, int w, int c, int dtype, void* stream) {
    GS_CHECK_ARG(x && gy && gx && n > 0 && c > 0 && h > 0 && w > 0, "max_pool2d_bwd: bad args");
    GS_CHECK_ARG(dtype == GS_F32 || dtype == GS_BF16, "max_pool2d_bwd: bad dtype %d", dtype);
    hipStream_t st = as_stream(stream);
    const long total = (long)n * h * w * c;
    const double esz = dtype == GS_F32 ? 4.0 : 2.0;
    ProfScope ps(st, 10.0 * total, esz * (2.0 * total + (double)n * ((h + 1) / 2) * ((w + 1) / 2) * c), PROF_POOL_BWD, n, h, w, c, c, 0, 0);
    long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((max_pool_bwd_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, (const T*)gy, (T*)gx, n, h, w, c));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_resnet_stem_bwd_weight_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h < 4 || w < 4) return 0;
    return (size_t)stem_wgrad_blocks(n, h, w) * 99 * 64 * sizeof(float);
}

extern "C" int gs_resnet_stem_bwd_weight(const void* x, const void* gstem, float* gw, float* gb, int n, int h, int w_, int co, int accumulate, int dtype,
                                         void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(x && gstem && gw && gb, "resnet_stem_bwd_weight: null argument");
    GS_CHECK_ARG(n > 0 && h > 0 && w_ > 0 && h % 4 == 0 && w_ % 4 == 0, "resnet_stem_bwd_weight: input %d x %d (positive multiples of 4)", h, w_);
    GS_CHECK_ARG(co == 64, "resnet_stem_bwd_weight: %d output channels (64)", co);
    GS_CHECK_ARG(dtype == GS_F32 || dtype == GS_BF16, "resnet_stem_bwd_weight: bad dtype %d", dtype);
    GS_CHECK_ARG((long)n * (h / 2) * cdiv(w_ / 2, STEMB_TW) < (1L << 31), "resnet_stem_bwd_weight: too many pixels");
    if (!ws || ws_bytes < gs_resnet_stem_bwd_weight_workspace_bytes(n, h, w_)) return fail(GS_ERR_WORKSPACE, "resnet_stem_bwd_weight: workspace too small (%zu)", ws_bytes);
    hipStream_t st = as_stream(stream);
    const int nb = stem_wgrad_blocks(n, h, w_);
    const int ntiles = (int)((long)n * (h / 2) * cdiv(w_ / 2, STEMB_TW));
    const double esz = dtype == GS_F32 ? 4.0 : 2.0, spx = (double)n * (h / 2) * (w_ / 2);
    ProfScope ps(st, 2.0 * 98 * 64 * spx, esz * ((double)n * h * w_ * 2 + spx * 64) + 99.0 * 64 * 4, PROF_STEM_WGRAD, n, h / 2, w_ / 2, 2, co, 0, 0);
    float* part = reinterpret_cast<float*>(ws);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((stem_wgrad_kernel<T>), dim3(nb), dim3(256), 0, st, (const T*)x, (const T*)gstem, part, n, h, w_, ntiles));
    GS_CHECK_LAUNCH();
    launch_fold(part, nb, 99L * 64, gw, 98L * 64, gb, accumulate, st);
    GS_CHECK_LAUNCH();
    return 0;
}

static int check_conv1x1_bwd(const char* who, int n, int h, int w_, int ci, int co, int stride, int dtype) {
    GS_CHECK_ARG(n > 0 && h > 0 && w_ > 0, "%s: bad sizes", who);
    GS_CHECK_ARG(stride == 1 || (stride == 2 && h % 2 == 0 && w_ % 2 == 0), "%s: stride %d on %d x %d", who, stride, h, w_);
    GS_CHECK_ARG(ci % 64 == 0 && co % 64 == 0 && ci > 0 && co > 0, "%s: %d -> %d channels (multiples of 64)", who, ci, co);
    GS_CHECK_ARG(dtype == GS_F32 || dtype == GS_BF16, "%s: bad dtype %d", who, dtype);
    GS_CHECK_ARG(((long)n * (h / stride) * (w_ / stride) + 63) / 64 < (1L << 31), "%s: too many pixels", who);
    return 0;
}

extern "C" int gs_conv1x1_bwd_data(const void* gy, const float* w, void* gx, int n, int h, int w_, int ci, int co, int stride, int accumulate, int dtype,
                                   void* stream) {
    GS_CHECK_ARG(gy && w && gx, "conv1x1_bwd_data: null argument");
    if (int e = check_conv1x1_bwd("conv1x1_bwd_data", n, h, w_, ci, co, stride, dtype)) return e;
    hipStream_t st = as_stream(stream);
    const long M = (long)n * (h / stride) * (w_ / stride);
    const double esz = dtype == GS_F32 ? 4.0 : 2.0;
    ProfScope ps(st, 2.0 * M * ci * co, esz * (double)M * (co + ci * (accumulate ? 2 : 1)) + 4.0 * ci * co, PROF_PROJ_BWD_DATA, n, h / stride, w_ / stride, ci,
                 co, stride, 0);
    if (!accumulate && stride != 1) {   // the pixels the stride skips receive no gradient
        if (hipMemsetAsync(gx, 0, (size_t)((double)n * h * w_ * ci * esz), st) != hipSuccess) return fail(GS_ERR_HIP, "conv1x1_bwd_data: memset failed");
    }
    dim3 grid((unsigned)cdiv(M, 64), ci / 64);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv1x1_bwd_data_kernel<T>), grid, dim3(256), 0, st, (const T*)gy, w, (T*)gx, h, w_, ci, co, stride, M, accumulate));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_conv1x1_bwd_weight_workspace_bytes(int n, int h, int w_, int ci, int co, int stride) {
    if (n <= 0 || h <= 0 || w_ <= 0 || ci <= 0 || co <= 0 || ci % 64 || co % 64 || (stride != 1 && stride != 2)) return 0;
    int splits;
    long rows;
    conv1x1_wgrad_split((long)n * (h / stride) * (w_ / stride), ci, co, &splits, &rows);
    return (size_t)splits * ci * co * sizeof(float);
}

extern "C" int gs_conv1x1_bwd_weight(const void* x, const void* gy, float* gw, int n, int h, int w_, int ci, int co, int stride, int accumulate, int dtype,
                                     void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(x && gy && gw, "conv1x1_bwd_weight: null argument");
    if (int e = check_conv1x1_bwd("conv1x1_bwd_weight", n, h, w_, ci, co, stride, dtype)) return e;
    if (!ws || ws_bytes < gs_conv1x1_bwd_weight_workspace_bytes(n, h, w_, ci, co, stride)) return fail(GS_ERR_WORKSPACE, "conv1x1_bwd_weight: workspace too small (%zu)", ws_bytes);
    hipStream_t st = as_stream(stream);
    const long M = (long)n * (h / stride) * (w_ / stride);
    int splits;
    long rows;
    conv1x1_wgrad_split(M, ci, co, &splits, &rows);
    const double esz = dtype == GS_F32 ? 4.0 : 2.0;
    ProfScope ps(st, 2.0 * M * ci * co, esz * (double)M * (ci + co) + 4.0 * ci * co, PROF_PROJ_BWD_WEIGHT, n, h / stride, w_ / stride, ci, co, stride, 0);
    float* part = reinterpret_cast<float*>(ws);
    dim3 grid(ci / 64, co / 64, splits);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv1x1_bwd_weight_kernel<T>), grid, dim3(256), 0, st, (const T*)x, (const T*)gy, part, h, w_, ci, co, stride, M, rows));
    GS_CHECK_LAUNCH();
    launch_fold(part, splits, (long)ci * co, gw, (long)ci * co, gw, accumulate, st);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_softmax_xent(const float* logits, const float* labels, float* loss, float* dlogits, int* correct, int n, int c, void* stream) {
    GS_CHECK_ARG(logits && labels && loss && correct && n > 0 && c > 0, "softmax_xent: bad args");
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, 8.0 * n * c, 12.0 * n * c, PROF_XENT, n, 1, 1, c, c, 0, 0);
    hipLaunchKernelGGL(softmax_xent_kernel, dim3(1), dim3(256), 0, st, logits, labels, loss, dlogits, correct, n, c);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_momentum_workspace_bytes(int64_t n) {
    return n > 0 ? (size_t)momentum_blocks(n) * sizeof(double) : 0;
}

extern "C" int gs_momentum_tf_step(float* p, float* g, float* accum, int64_t n, int64_t decay_lo, int64_t decay_hi, float weight_decay, float lr,
                                   float momentum, int nesterov, int zero_grad, float* l2, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(p && g && accum && n > 0 && n % 4 == 0, "momentum_tf_step: p, g, accum and a multiple of 4 elements (got %ld)", (long)n);
    GS_CHECK_ARG(decay_lo >= 0 && decay_lo <= decay_hi && decay_hi <= n, "momentum_tf_step: decayed range [%ld, %ld) of %ld", (long)decay_lo, (long)decay_hi, (long)n);
    if (!ws || ws_bytes < gs_momentum_workspace_bytes(n)) return fail(GS_ERR_WORKSPACE, "momentum_tf_step: workspace too small (%zu)", ws_bytes);
    hipStream_t st = as_stream(stream);
    const int nb = momentum_blocks(n);
    ProfScope ps(st, 6.0 * n, (zero_grad ? 24.0 : 20.0) * n, PROF_MOMENTUM, 1, 1, 1, 0, 0, nesterov, 0);
    double* partial = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(momentum_kernel, dim3(nb), dim3(256), 0, st, p, g, accum, (long)(n / 4), (long)decay_lo, (long)decay_hi, weight_decay, lr, momentum,
                       nesterov, zero_grad, partial);
    GS_CHECK_LAUNCH();
    if (l2) {
        hipLaunchKernelGGL(momentum_l2_kernel, dim3(1), dim3(256), 0, st, partial, nb, l2);
        GS_CHECK_LAUNCH();
    }
    return 0;
}
