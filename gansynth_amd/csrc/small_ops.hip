// Small-tensor kernels of the PGGAN hot path: embedding (ops.py:204-218) and minibatch stddev (ops.py:336-348) with their first/second-order
// gradients, and the GAN losses (models.py:39-65).  All tiny; none is MFMA work.  (The dense layers: dense.hip.)
// (Which batch-stddev instantiation a shape runs -- VN -- and its blocks: elementwise_route.h, the route the elementwise kernels share.)
#include "elementwise_route.h"

namespace gs {

// ------------------------------------------------------------------------------ embedding
template <typename T>
__global__ void embedding_fwd_kernel(const int64_t* __restrict__ idx, const float* __restrict__ w, T* __restrict__ y, int b, int rows, int units, float alpha) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b * units) return;
    const int r = e / units, u = e % units;
    long k = idx[r];
    if (k < 0) k = 0;
    if (k >= rows) k = rows - 1;
    DT<T>::st(y + e, w[k * units + u] * alpha);
}
// the same gather with the row index taken from the one-hot input itself (ops.py:204-218 gathers by tf.argmax of it): block b scans its
// label row for the first maximum, writes it to idx_out[b] (the backward's scatter index) and gathers -- no separate argmax launch
template <typename T>
__global__ __launch_bounds__(256) void embedding_onehot_fwd_kernel(const T* __restrict__ labels, const float* __restrict__ w, T* __restrict__ y, int64_t* __restrict__ idx_out,
                                                                    int rows, int units, float alpha) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int b = blockIdx.x, t = threadIdx.x;
    float best = -INFINITY;
    int bi = rows;
    for (int k = t; k < rows; k += 256) {   // (ascending k per thread: the first maximum wins)
        const float v = DT<T>::ld(labels + (long)b * rows + k);
        if (v > best) { best = v; bi = k; }
    }
    sv[t] = best; si[t] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const float v = sv[t + o];
            const int i = si[t + o];
            if (v > sv[t] || (v == sv[t] && i < si[t])) { sv[t] = v; si[t] = i; }
        }
        __syncthreads();
    }
    int k = si[0];
    if (k >= rows) k = 0;
    if (t == 0) idx_out[b] = k;
    for (int u = t; u < units; u += 256) DT<T>::st(y + (long)b * units + u, w[(long)k * units + u] * alpha);
}
// gw[row][u] = alpha * sum_{b: idx[b]==row} gy[b][u]  (gather form: deterministic, no atomics)
template <typename T>
__global__ void embedding_bwd_kernel(const int64_t* __restrict__ idx, const T* __restrict__ gy, float* __restrict__ gw, int b, int rows, int units, float alpha) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * units) return;
    const int r = e / units, u = e % units;
    float s = 0.f;
    for (int k = 0; k < b; ++k)
        if (idx[k] == r) s += DT<T>::ld(gy + (long)k * units + u);
    gw[e] = s * alpha;
}

// -------------------------------------------------------------------------- batch stddev
// x [b][hw][c] (channels-last), groups of 4: column j in [0, M=b/4) holds samples j, j+M, j+2M, j+3M.
// One block per column j (M = 2 at batch 8: a latency chain, not a bandwidth problem): 1024 threads, VN = 16 bytes of
// positions per thread and member (VN = 1: scalar fallback for odd sizes), so that the 4 x 8192 values of the model's 2x16x256
// block are one trip of four independent 16-byte loads per thread.
template <typename T, int VN> __device__ inline void bs_ld(const T* p, float* o) {
    if constexpr (VN == 1) o[0] = DT<T>::ld(p); else ld_wide<T>(p, o);
}
template <typename T, int VN> __device__ inline void bs_st(T* p, const float* o) {
    if constexpr (VN == 1) DT<T>::st(p, o[0]); else st_wide<T>(p, o);
}
template <typename T, int VN>
__device__ inline void bs_load(const T* x, int M, int j, long pos, long npos, float (&v)[4][VN]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) bs_ld<T, VN>(x + ((long)(i * M + j)) * npos + pos, v[i]);
}
constexpr int BS_NT = 1024;

template <typename T, int VN>
__global__ __launch_bounds__(BS_NT) void batch_stddev_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int M, int hw, int c, float eps) {
    __shared__ float red[BS_NT / 64];
    const int j = blockIdx.x;
    const long npos = (long)hw * c;
    float s = 0.f;
    for (long pos = (long)threadIdx.x * VN; pos < npos; pos += (long)BS_NT * VN) {
        float v[4][VN];
        bs_load<T, VN>(x, M, j, pos, npos, v);
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float mu = 0.25f * (v[0][e] + v[1][e] + v[2][e] + v[3][e]);
            float var = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) var += (v[i][e] - mu) * (v[i][e] - mu);
            s += sqrtf(0.25f * var + eps);
        }
    }
    s = block_sum<BS_NT>(s, red) / (float)npos;
    for (int k = threadIdx.x; k < 4 * hw; k += BS_NT) {
        const int i = k / hw, p = k % hw;
        DT<T>::st(y + (long)(i * M + j) * hw + p, s);
    }
}

// gx_i = gs_j * d_i / (4 sigma N) (+ addend_i),  gs_j = sum over members/pixels of gy
// addend (optional): the OTHER gradient into x -- x feeds the statistic and the conv beside it (networks.py:174-176), the sum of the two
// gradients is formed here instead of by one more pass
template <typename T, int VN>
__global__ __launch_bounds__(BS_NT) void batch_stddev_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ x, const T* __restrict__ addend,
                                                                 T* __restrict__ gx, int M, int hw, int c, float eps) {
    __shared__ float red[BS_NT / 64];
    const int j = blockIdx.x;
    const long npos = (long)hw * c;
    float g = 0.f;
    for (int k = threadIdx.x; k < 4 * hw; k += BS_NT) g += DT<T>::ld(gy + (long)((k / hw) * M + j) * hw + (k % hw));
    g = block_sum<BS_NT>(g, red);
    const float coef = g / (4.f * (float)npos);
    for (long pos = (long)threadIdx.x * VN; pos < npos; pos += (long)BS_NT * VN) {
        float v[4][VN], o[4][VN];
        bs_load<T, VN>(x, M, j, pos, npos, v);
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float mu = 0.25f * (v[0][e] + v[1][e] + v[2][e] + v[3][e]);
            float var = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) var += (v[i][e] - mu) * (v[i][e] - mu);
            const float inv = coef / sqrtf(0.25f * var + eps);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i][e] = (v[i][e] - mu) * inv;
        }
        if (addend) {
            bs_load<T, VN>(addend, M, j, pos, npos, v);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < VN; ++e) o[i][e] += v[i][e];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) bs_st<T, VN>(gx + ((long)(i * M + j)) * npos + pos, o[i]);
    }
}

// F = sum_pos gs_j/(4N) * S/sigma,  S = sum_i ggx_i d_i
//   ggy (every member / pixel of column j) = sum_pos S / (4 sigma N)
//   gx2_k = gs_j/(4N) * [ (ggx_k - mean_i ggx_i)/sigma - S d_k / (4 sigma^3) ]
template <typename T, int VN>
__global__ __launch_bounds__(BS_NT) void batch_stddev_bwd_bwd_kernel(const T* __restrict__ ggx, const T* __restrict__ gy, const T* __restrict__ x,
                                                                     T* __restrict__ ggy, T* __restrict__ gx2, int M, int hw, int c, float eps) {
    __shared__ float red[BS_NT / 64];
    const int j = blockIdx.x;
    const long npos = (long)hw * c;
    float g = 0.f;
    for (int k = threadIdx.x; k < 4 * hw; k += BS_NT) g += DT<T>::ld(gy + (long)((k / hw) * M + j) * hw + (k % hw));
    g = block_sum<BS_NT>(g, red);
    const float coef = g / (4.f * (float)npos);
    float t = 0.f;
    for (long pos = (long)threadIdx.x * VN; pos < npos; pos += (long)BS_NT * VN) {
        float v[4][VN], gg[4][VN], o[4][VN];
        bs_load<T, VN>(x, M, j, pos, npos, v);
        bs_load<T, VN>(ggx, M, j, pos, npos, gg);
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            const float mu = 0.25f * (v[0][e] + v[1][e] + v[2][e] + v[3][e]);
            const float gm = 0.25f * (gg[0][e] + gg[1][e] + gg[2][e] + gg[3][e]);
            float var = 0.f, S = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) { var += (v[i][e] - mu) * (v[i][e] - mu); S += gg[i][e] * (v[i][e] - mu); }
            const float sig = sqrtf(0.25f * var + eps);
            t += S / sig;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i][e] = coef * ((gg[i][e] - gm) / sig - S * (v[i][e] - mu) / (4.f * sig * sig * sig));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) bs_st<T, VN>(gx2 + ((long)(i * M + j)) * npos + pos, o[i]);
    }
    t = block_sum<BS_NT>(t, red) / (4.f * (float)npos);
    for (int k = threadIdx.x; k < 4 * hw; k += BS_NT) DT<T>::st(ggy + (long)((k / hw) * M + j) * hw + (k % hw), t);
}

// ------------------------------------------------------------------------------ GAN losses
// The loss algebra of models.py:39-65 on [N] / [N, C] tensors was ~50 torch launches per iteration (casts, products, sums,
// softplus, mean and their autograd mirror images); here each loss is ONE single-block launch that also writes the gradients of
// the mean w.r.t. its inputs (the backward of the autograd node then only scales them by the incoming scalar).
__device__ inline float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }       // tf.nn.softplus
__device__ inline float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// L_D = mean_i [ softplus(-r_i) + softplus(f_i) + pen_i ],  r_i / f_i = sum_c logits[i][c] * labels[i][c] (one-hot labels:
// tf.gather_nd(logits, tf.where(labels)), models.py:39-40).  g_real = d L_D / d real_logits etc.
template <typename T>
__global__ __launch_bounds__(256) void gan_d_loss_kernel(const T* __restrict__ rl, const T* __restrict__ fl, const T* __restrict__ lab,
                                                         const float* __restrict__ pen, float pen_w, int n, int c, float* __restrict__ loss,
                                                         T* __restrict__ g_real, T* __restrict__ g_fake, float* __restrict__ g_pen) {
    __shared__ float red[4];
    __shared__ float sr[1024], sf[1024];
    const float inv_n = 1.f / (float)n;
    float part = 0.f;
    // a WAVE per sample, its lanes over the classes (a thread per sample walked the 61 classes as one chain of dependent loads: 8-11 us for
    // 16 samples)
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < n; i += 4) {
        float r = 0.f, f = 0.f;
        for (int k = lane; k < c; k += 64) {
            const float l = DT<T>::ld(lab + (long)i * c + k);
            if (rl) r += DT<T>::ld(rl + (long)i * c + k) * l;
            if (fl) f += DT<T>::ld(fl + (long)i * c + k) * l;
        }
        r = wave_sum(r);
        f = wave_sum(f);
        if (lane == 0) {
            // (either half of the sum may be absent: the two halves of a discriminator run that keeps its real and its fake pass on two
            //  streams are two launches, each with its own partial mean -- the gradients are the same numbers either way)
            part += (rl ? softplus_f(-r) : 0.f) + (fl ? softplus_f(f) : 0.f) + (pen ? pen_w * pen[i] : 0.f);
            if (g_pen) g_pen[i] = pen_w * inv_n;
            sr[i] = -sigmoid_f(-r) * inv_n;   // d mean / d r_i
            sf[i] = sigmoid_f(f) * inv_n;     // d mean / d f_i
        }
    }
    const float tot = block_sum<256>(part, red);
    if (threadIdx.x == 0) loss[0] = tot * inv_n;
    __syncthreads();
    for (int e = threadIdx.x; e < n * c; e += 256) {
        const float l = DT<T>::ld(lab + e);
        if (rl) DT<T>::st(g_real + e, sr[e / c] * l);
        if (fl) DT<T>::st(g_fake + e, sf[e / c] * l);
    }
}

// L_G = mean_i [ softplus(-f_i) + w / (s_i + eps) ],  s_i = sum((d sum(G(z)) / d z_i)^2) (models.py:57-64); g_s = d L_G / d s.
template <typename T>
__global__ __launch_bounds__(256) void gan_g_loss_kernel(const T* __restrict__ fl, const T* __restrict__ lab, const float* __restrict__ ssq, float w,
                                                         float eps, int n, int c, float* __restrict__ loss, T* __restrict__ g_fake,
                                                         float* __restrict__ g_ssq) {
    __shared__ float red[4];
    __shared__ float sf[1024];
    const float inv_n = 1.f / (float)n;
    float part = 0.f;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < n; i += 4) {   // a wave per sample (see gan_d_loss_kernel)
        float f = 0.f;
        if (fl) for (int k = lane; k < c; k += 64) f += DT<T>::ld(fl + (long)i * c + k) * DT<T>::ld(lab + (long)i * c + k);
        f = wave_sum(f);
        if (lane == 0) {
            if (fl) part += softplus_f(-f);   // (absent: the mode-seeking half alone, see gan_d_loss_kernel)
            sf[i] = -sigmoid_f(-f) * inv_n;
            if (ssq) {
                const float d = ssq[i] + eps;
                part += w / d;
                g_ssq[i] = -w / (d * d) * inv_n;
            }
        }
    }
    const float tot = block_sum<256>(part, red);
    if (threadIdx.x == 0) loss[0] = tot * inv_n;
    __syncthreads();
    if (fl) for (int e = threadIdx.x; e < n * c; e += 256) DT<T>::st(g_fake + e, sf[e / c] * DT<T>::ld(lab + e));
}

}  // namespace gs

using namespace gs;

extern "C" int gs_gan_d_loss(const void* real_logits, const void* fake_logits, const void* labels, const float* penalty, float penalty_weight, int n, int c,
                             float* loss, void* g_real, void* g_fake, float* g_penalty, int dtype, void* stream) {
    GS_CHECK_ARG(n > 0 && n <= 1024 && c > 0 && (real_logits || fake_logits) && labels && loss && (!real_logits || g_real) && (!fake_logits || g_fake),
                 "gan_d_loss: bad args (batch %d <= 1024)", n);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gan_d_loss_kernel<T>), dim3(1), dim3(256), 0, as_stream(stream), (const T*)real_logits, (const T*)fake_logits,
                                                (const T*)labels, penalty, penalty_weight, n, c, loss, (T*)g_real, (T*)g_fake, penalty ? g_penalty : nullptr));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_gan_g_loss(const void* fake_logits, const void* labels, const float* sumsq, float weight, float eps, int n, int c, float* loss,
                             void* g_fake, float* g_sumsq, int dtype, void* stream) {
    GS_CHECK_ARG(n > 0 && n <= 1024 && c > 0 && (fake_logits || sumsq) && (!fake_logits || (labels && g_fake)) && loss && (!sumsq || g_sumsq),
                 "gan_g_loss: bad args (batch %d <= 1024)", n);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gan_g_loss_kernel<T>), dim3(1), dim3(256), 0, as_stream(stream), (const T*)fake_logits, (const T*)labels, sumsq,
                                                weight, eps, n, c, loss, (T*)g_fake, g_sumsq));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_embedding_fwd(const int64_t* idx, const float* w, void* y, int b, int rows, int units, float alpha, int dtype, void* stream) {
    GS_CHECK_ARG(b > 0 && rows > 0 && units > 0, "embedding_fwd: bad args");
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((embedding_fwd_kernel<T>), dim3(cdiv((long)b * units, 256)), dim3(256), 0, as_stream(stream), idx, w, (T*)y, b, rows, units, alpha));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_embedding_onehot_fwd(const void* labels, const float* w, void* y, int64_t* idx_out, int b, int rows, int units, float alpha, int dtype, void* stream) {
    GS_CHECK_ARG(b > 0 && rows > 0 && units > 0 && labels && w && y && idx_out, "embedding_onehot_fwd: bad args");
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((embedding_onehot_fwd_kernel<T>), dim3(b), dim3(256), 0, as_stream(stream), (const T*)labels, w, (T*)y, idx_out, rows, units, alpha));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_embedding_bwd(const int64_t* idx, const void* gy, float* gw, int b, int rows, int units, float alpha, int dtype, void* stream) {
    GS_CHECK_ARG(b > 0 && rows > 0 && units > 0, "embedding_bwd: bad args");
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((embedding_bwd_kernel<T>), dim3(cdiv((long)rows * units, 256)), dim3(256), 0, as_stream(stream), idx, (const T*)gy, gw, b, rows, units, alpha));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_batch_stddev_fwd(const void* x, void* y, int b, int hw, int c, float eps, int dtype, void* stream) {
    EwRoute r;
    if (int e = ew_plan("batch_stddev_fwd", GS_EW_OP_BATCH_STDDEV_FWD, dtype, hw, c, b, 0, &r)) return e;
    GS_DISPATCH_DTYPE(dtype, {
        if (r.E == Wide<T>::N) hipLaunchKernelGGL((batch_stddev_fwd_kernel<T, Wide<T>::N>), dim3(r.grid_x), dim3(BS_NT), 0, as_stream(stream), (const T*)x, (T*)y, b / 4, hw, c, eps);
        else hipLaunchKernelGGL((batch_stddev_fwd_kernel<T, 1>), dim3(r.grid_x), dim3(BS_NT), 0, as_stream(stream), (const T*)x, (T*)y, b / 4, hw, c, eps);
    });
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_batch_stddev_bwd(const void* gy, const void* x, const void* addend, void* gx, int b, int hw, int c, float eps, int dtype, void* stream) {
    EwRoute r;
    if (int e = ew_plan("batch_stddev_bwd", GS_EW_OP_BATCH_STDDEV_BWD, dtype, hw, c, b, 0, &r)) return e;
    GS_DISPATCH_DTYPE(dtype, {
        if (r.E == Wide<T>::N) hipLaunchKernelGGL((batch_stddev_bwd_kernel<T, Wide<T>::N>), dim3(r.grid_x), dim3(BS_NT), 0, as_stream(stream), (const T*)gy, (const T*)x, (const T*)addend, (T*)gx, b / 4, hw, c, eps);
        else hipLaunchKernelGGL((batch_stddev_bwd_kernel<T, 1>), dim3(r.grid_x), dim3(BS_NT), 0, as_stream(stream), (const T*)gy, (const T*)x, (const T*)addend, (T*)gx, b / 4, hw, c, eps);
    });
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_batch_stddev_bwd_bwd(const void* ggx, const void* gy, const void* x, void* ggy, void* gx2, int b, int hw, int c, float eps, int dtype, void* stream) {
    EwRoute r;
    if (int e = ew_plan("batch_stddev_bwd_bwd", GS_EW_OP_BATCH_STDDEV_BWD_BWD, dtype, hw, c, b, 0, &r)) return e;
    GS_DISPATCH_DTYPE(dtype, {
        if (r.E == Wide<T>::N) hipLaunchKernelGGL((batch_stddev_bwd_bwd_kernel<T, Wide<T>::N>), dim3(r.grid_x), dim3(BS_NT), 0, as_stream(stream), (const T*)ggx, (const T*)gy, (const T*)x, (T*)ggy, (T*)gx2, b / 4, hw, c, eps);
        else hipLaunchKernelGGL((batch_stddev_bwd_bwd_kernel<T, 1>), dim3(r.grid_x), dim3(BS_NT), 0, as_stream(stream), (const T*)ggx, (const T*)gy, (const T*)x, (T*)ggy, (T*)gx2, b / 4, hw, c, eps);
    });
    GS_CHECK_LAUNCH();
    return 0;
}
