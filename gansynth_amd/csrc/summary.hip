// TensorBoard summaries: quantise images to 8-bit planes and audio to 16-bit PCM on the device, so that a summary step copies
// bytes, not activations, to the host (models.py:131-161 of the reference: tf.summary.image / tf.summary.audio, max_outputs = 4).
//
// Images: tf.summary.image's rule for float input, per image and per channel plane (see include/gansynth_hip.h).  Two launches, no
// atomics: `summary_minmax_kernel` leaves one (min, max) pair per (plane, slab) in the workspace, `summary_image_u8_kernel` folds its
// plane's pairs in one wave and quantises its slab.  min / max are exact, so neither the slab size nor the fold order shows in the result.
// The arithmetic is fp32 with the multiply and the add rounded separately: a fused multiply-add moves pixels across truncation boundaries.
#include "gs_common.h"

namespace gs {

constexpr int SUM_NT = 256;          // threads per block
constexpr int SUM_SLAB = 2048;       // pixels of one plane per block (a multiple of every pack width)

// pixels per thread and step: one 16-byte load per channel for fp32, one 16-byte load in all for bf16
template <typename T, int C> struct Pack { static constexpr int PX = (sizeof(T) == 2 && C == 1) ? 8 : 4; };

__device__ inline bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// PX consecutive pixels of one image, channels interleaved -> v[c][i]; `src` is 16-byte aligned
template <typename T, int C, int PX> __device__ inline void load_pixels(const T* src, float (&v)[C][PX]) {
    constexpr int W = Wide<T>::N;
    float raw[PX * C];
#pragma unroll
    for (int k = 0; k < PX * C / W; ++k) ld_wide<T>(src + k * W, raw + k * W);
#pragma unroll
    for (int i = 0; i < PX; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][i] = raw[i * C + c];
}

// Whether image `img` (its input at x, its planes at out) takes the packed path: block-uniform, decided from the addresses
template <typename T, int C> __device__ inline bool packed_ok(const T* x, const unsigned char* out, long p) {
    constexpr int PX = Pack<T, C>::PX;
    bool ok = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#pragma unroll
    for (int c = 0; c < C; ++c) ok = ok && ((reinterpret_cast<uintptr_t>(out + c * p) & (PX - 1)) == 0);
    return ok;
}

// grid (slabs, n).  ws[((img * C + c) * slabs + slab) * 2 + {0, 1}] = min, max of the finite values of the slab (+inf, -inf when it has none)
template <typename T, int C>
__global__ __launch_bounds__(SUM_NT) void summary_minmax_kernel(const T* __restrict__ x, const unsigned char* out, float* __restrict__ ws, long p) {
    constexpr int PX = Pack<T, C>::PX;
    const int slab = blockIdx.x, slabs = gridDim.x, img = blockIdx.y;
    const T* xi = x + (size_t)img * p * C;
    const long p0 = (long)slab * SUM_SLAB;
    const long p1 = p0 + SUM_SLAB < p ? p0 + SUM_SLAB : p;
    float lo[C], hi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
    long scalar_from = p0;
    if (packed_ok<T, C>(xi, out + (size_t)img * C * p, p)) {   // (the same split as the quantising launch: nothing depends on it here)
        const long packs = (p1 - p0) / PX;
        for (long q = threadIdx.x; q < packs; q += SUM_NT) {
            float v[C][PX];
            load_pixels<T, C, PX>(xi + (p0 + q * PX) * C, v);
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (finite_f32(v[c][i])) { lo[c] = fminf(lo[c], v[c][i]); hi[c] = fmaxf(hi[c], v[c][i]); }
        }
        scalar_from = p0 + packs * PX;
    }
    for (long q = scalar_from + threadIdx.x; q < p1; q += SUM_NT)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = DT<T>::ld(xi + q * C + c);
            if (finite_f32(v)) { lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
        }
    __shared__ float part[SUM_NT / 64][C][2];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        lo[c] = wave_extreme<false>(lo[c]);
        hi[c] = wave_extreme<true>(hi[c]);
        if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][c][0] = lo[c]; part[threadIdx.x >> 6][c][1] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        float l = part[0][c][0], h = part[0][c][1];
#pragma unroll
        for (int w = 1; w < SUM_NT / 64; ++w) { l = fminf(l, part[w][c][0]); h = fmaxf(h, part[w][c][1]); }
        *reinterpret_cast<float2*>(ws + (((size_t)img * C + c) * slabs + slab) * 2) = make_float2(l, h);
    }
}

// tf.summary.image's scale and offset of a plane from its finite range
__device__ inline void plane_scale(float lo, float hi, float& scale, float& offset) {
    if (lo < 0.f) {
        const float m = fmaxf(fabsf(lo), fabsf(hi));
        scale = m < 1e-6f ? 0.f : __fdiv_rn(127.f, m);
        offset = 128.f;
    } else {
        scale = hi < 1e-6f ? 0.f : __fdiv_rn(255.f, hi);
        offset = 0.f;
    }
}

// fl(fl(v * scale) + offset), truncated.  __fmul_rn / __fadd_rn are plain operators in hipcc's headers and were contracted into one
// v_fma_f32 here (seen in the ISA): the operators are written out under the pragma, which is what keeps the two roundings apart.
__device__ inline unsigned int quantise_u8(float v, float scale, float offset) {
#pragma clang fp contract(off)
    if (!finite_f32(v)) return 255u;
    const float t = v * scale;
    const float r = t + offset;
    return (unsigned int)(int)r;   // 0 <= r < 256 by construction of scale and offset; the conversion truncates
}

// grid (slabs, n).  out[(img * C + c) * p + pixel]
template <typename T, int C>
__global__ __launch_bounds__(SUM_NT) void summary_image_u8_kernel(const T* __restrict__ x, unsigned char* __restrict__ out,
                                                                  const float* __restrict__ ws, long p) {
    constexpr int PX = Pack<T, C>::PX;
    const int slab = blockIdx.x, slabs = gridDim.x, img = blockIdx.y;
    __shared__ float so[C][2];
    if (threadIdx.x < 64) {   // one wave folds the partials of this image's planes
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* w = ws + ((size_t)img * C + c) * slabs * 2;
            float lo = INFINITY, hi = -INFINITY;
            for (int s = threadIdx.x; s < slabs; s += 64) {
                const float2 lh = *reinterpret_cast<const float2*>(w + (size_t)s * 2);
                lo = fminf(lo, lh.x);
                hi = fmaxf(hi, lh.y);
            }
            lo = wave_extreme<false>(lo);
            hi = wave_extreme<true>(hi);
            if (threadIdx.x == 0) plane_scale(lo, hi, so[c][0], so[c][1]);
        }
    }
    __syncthreads();
    float scale[C], offset[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { scale[c] = so[c][0]; offset[c] = so[c][1]; }
    const T* xi = x + (size_t)img * p * C;
    unsigned char* oi = out + (size_t)img * C * p;
    const long p0 = (long)slab * SUM_SLAB;
    const long p1 = p0 + SUM_SLAB < p ? p0 + SUM_SLAB : p;
    long scalar_from = p0;
    if (packed_ok<T, C>(xi, oi, p)) {
        const long packs = (p1 - p0) / PX;
        for (long q = threadIdx.x; q < packs; q += SUM_NT) {
            const long px = p0 + q * PX;
            float v[C][PX];
            load_pixels<T, C, PX>(xi + px * C, v);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                unsigned int w[PX / 4];
#pragma unroll
                for (int k = 0; k < PX / 4; ++k)
                    w[k] = quantise_u8(v[c][4 * k], scale[c], offset[c]) | (quantise_u8(v[c][4 * k + 1], scale[c], offset[c]) << 8) |
                           (quantise_u8(v[c][4 * k + 2], scale[c], offset[c]) << 16) | (quantise_u8(v[c][4 * k + 3], scale[c], offset[c]) << 24);
                unsigned char* dst = oi + c * p + px;
                if constexpr (PX == 8) *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
                else *reinterpret_cast<unsigned int*>(dst) = w[0];
            }
        }
        scalar_from = p0 + packs * PX;
    }
    for (long q = scalar_from + threadIdx.x; q < p1; q += SUM_NT)
#pragma unroll
        for (int c = 0; c < C; ++c) oi[c * p + q] = (unsigned char)quantise_u8(DT<T>::ld(xi + q * C + c), scale[c], offset[c]);
}

// ------------------------------------------------------------------------------------------------ audio
// (quantise_s16, TF's FloatToInt16Sample, lives in gs_common.h: the note mixdown of synth.hip quantises by the same rule)
constexpr int AUD_STEPS = 4;   // packs per thread

// grid (blocks, n): row `blockIdx.y` of x (stride in elements) -> row of out (contiguous)
template <typename T>
__global__ __launch_bounds__(SUM_NT) void summary_audio_s16_kernel(const T* __restrict__ x, short* __restrict__ out, long l, long stride) {
    constexpr int W = Wide<T>::N;
    const T* xr = x + (size_t)blockIdx.y * stride;
    short* orow = out + (size_t)blockIdx.y * l;
    const long span = (long)SUM_NT * W * AUD_STEPS;
    const long s0 = (long)blockIdx.x * span;
    const long s1 = s0 + span < l ? s0 + span : l;
    long scalar_from = s0;
    if ((reinterpret_cast<uintptr_t>(xr) & 15) == 0 && (reinterpret_cast<uintptr_t>(orow) & (2 * W - 1)) == 0) {   // block-uniform
        const long packs = (s1 - s0) / W;
        for (long q = threadIdx.x; q < packs; q += SUM_NT) {
            float v[W];
            ld_wide<T>(xr + s0 + q * W, v);
            unsigned int w[W / 2];
#pragma unroll
            for (int k = 0; k < W / 2; ++k)
                w[k] = ((unsigned int)quantise_s16(v[2 * k]) & 0xffffu) | ((unsigned int)quantise_s16(v[2 * k + 1]) << 16);
            short* dst = orow + s0 + q * W;
            if constexpr (W == 8) *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            else *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
        }
        scalar_from = s0 + packs * W;
    }
    for (long q = scalar_from + threadIdx.x; q < s1; q += SUM_NT) orow[q] = (short)quantise_s16(DT<T>::ld(xr + q));
}

static inline long image_slabs(long p) { return (p + SUM_SLAB - 1) / SUM_SLAB; }

}  // namespace gs

using namespace gs;

extern "C" size_t gs_summary_image_u8_workspace_bytes(int n, int64_t p, int c) {
    if (n <= 0 || p <= 0 || (c != 1 && c != 2)) return 0;
    return (size_t)n * c * image_slabs(p) * 2 * sizeof(float);
}

extern "C" int gs_summary_image_u8(const void* x, uint8_t* out, int n, int64_t p, int c, int dtype, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(c == 1 || c == 2, "summary_image_u8: channels must be 1 or 2 (got %d)", c);
    GS_CHECK_ARG(n > 0 && n <= 65535 && p > 0 && image_slabs(p) <= 0x7fffffffL, "summary_image_u8: bad shape n=%d p=%lld", n, (long long)p);
    GS_CHECK_ARG(x && out, "summary_image_u8: null pointer");
    GS_CHECK_ARG(ws && ws_bytes >= gs_summary_image_u8_workspace_bytes(n, p, c) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                 "summary_image_u8: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, gs_summary_image_u8_workspace_bytes(n, p, c));
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)image_slabs(p), (unsigned)n);
    GS_DISPATCH_DTYPE(dtype, {
        const T* xt = static_cast<const T*>(x);
        if (c == 1) {
            hipLaunchKernelGGL((summary_minmax_kernel<T, 1>), grid, dim3(SUM_NT), 0, st, xt, out, static_cast<float*>(ws), (long)p);
            hipLaunchKernelGGL((summary_image_u8_kernel<T, 1>), grid, dim3(SUM_NT), 0, st, xt, out, static_cast<const float*>(ws), (long)p);
        } else {
            hipLaunchKernelGGL((summary_minmax_kernel<T, 2>), grid, dim3(SUM_NT), 0, st, xt, out, static_cast<float*>(ws), (long)p);
            hipLaunchKernelGGL((summary_image_u8_kernel<T, 2>), grid, dim3(SUM_NT), 0, st, xt, out, static_cast<const float*>(ws), (long)p);
        }
    });
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_summary_audio_s16(const void* x, int16_t* out, int n, int64_t l, int64_t row_stride, int dtype, void* stream) {
    GS_CHECK_ARG(n > 0 && n <= 65535 && l > 0 && row_stride >= l, "summary_audio_s16: bad shape n=%d l=%lld stride=%lld", n, (long long)l,
                 (long long)row_stride);
    GS_CHECK_ARG(x && out, "summary_audio_s16: null pointer");
    hipStream_t st = as_stream(stream);
    GS_DISPATCH_DTYPE(dtype, {
        const long span = (long)SUM_NT * Wide<T>::N * AUD_STEPS;
        GS_CHECK_ARG((l + span - 1) / span <= 0x7fffffffL, "summary_audio_s16: row too long");
        const dim3 grid((unsigned)((l + span - 1) / span), (unsigned)n);
        hipLaunchKernelGGL((summary_audio_s16_kernel<T>), grid, dim3(SUM_NT), 0, st, static_cast<const T*>(x), out, (long)l, (long)row_stride);
    });
    GS_CHECK_LAUNCH();
    return 0;
}
