// The finishing stage of a rendered clip, once for every producer (clip_finish.h): gs_note_mix, gs_note_mix_stereo, gs_stereo_finish,
// gs_resample and gs_fftconv all end here.  The rules -- one peak a clip, the quotient by __fdiv_rn only when the peak exceeds 1, TF's
// FloatToInt16Sample -- are stated in include/gansynth_hip.h and DESIGN.md "Note sequences".
//
// A second launch after the producer's, like gs_summary_image_u8: every block folds its clip's block maxima with all its threads (a minute
// at 48 kHz leaves thousands; a maximum over values that are never NaN is exact, so the fold order does not show), then scales and
// quantises its own CLIP_TILE samples of every channel, 16 bytes per lane where the bases allow and sample by sample otherwise.
#include "clip_finish.h"

namespace gs {

static inline long clip_tiles(long n) { return (n + CLIP_TILE - 1) / CLIP_TILE; }

// grid (tiles of n, or 1 when only the peak is wanted; clips).  x = x / peak when `normalize` and peak > 1 (else untouched); pcm from x
template <int CH>
__global__ __launch_bounds__(CLIP_NT) void clip_finish_kernel(float* __restrict__ x, long row_stride, short* __restrict__ pcm, float* __restrict__ peak_out,
                                                              const float* __restrict__ block_max, int n_max, long n, int normalize) {
    const int clip = blockIdx.y;
    float m = 0.f;
    for (int s = threadIdx.x; s < n_max; s += CLIP_NT) m = fmaxf(m, block_max[(size_t)clip * n_max + s]);
    const float peak = block_max_of<CLIP_NT>(m);
    if (blockIdx.x == 0 && threadIdx.x == 0 && peak_out != nullptr) peak_out[clip] = peak;
    const bool scale = normalize != 0 && peak > 1.f;
    if (!scale && pcm == nullptr) return;
    float* xc[CH];
    uintptr_t bases = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        xc[c] = x + ((size_t)clip * CH + c) * row_stride;
        bases |= reinterpret_cast<uintptr_t>(xc[c]);
    }
    short* __restrict__ q = pcm != nullptr ? pcm + (size_t)clip * n * CH : nullptr;
    const long tile_begin = (long)blockIdx.x * CLIP_TILE;
    const long tile_end = tile_begin + CLIP_TILE < n ? tile_begin + CLIP_TILE : n;
    const bool wide = (bases & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & (8 * CH - 1)) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < CLIP_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * CLIP_NT + threadIdx.x) * 4;
        if (t0 + 4 <= tile_end && wide) {
            float v[CH][4];
#pragma unroll
            for (int c = 0; c < CH; ++c) ld4(xc[c] + t0, v[c]);
            if (scale) {
#pragma unroll
                for (int c = 0; c < CH; ++c) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[c][j] = __fdiv_rn(v[c][j], peak);
                    st4(xc[c] + t0, v[c]);
                }
            }
            if (q != nullptr) {   // 4 * CH interleaved values, two a dword: value i is sample i / CH of channel i % CH
                unsigned int p[2 * CH];
#pragma unroll
                for (int i = 0; i < 2 * CH; ++i)
                    p[i] = ((unsigned int)quantise_s16(v[(2 * i) % CH][(2 * i) / CH]) & 0xffffu) |
                           ((unsigned int)quantise_s16(v[(2 * i + 1) % CH][(2 * i + 1) / CH]) << 16);
                if constexpr (CH == 1) *reinterpret_cast<uint2*>(q + t0) = make_uint2(p[0], p[1]);
                else *reinterpret_cast<uint4*>(q + 2 * t0) = make_uint4(p[0], p[1], p[2], p[3]);
            }
        } else {
            for (int j = 0; j < 4; ++j) {
                const long t = t0 + j;
                if (t >= tile_end) break;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    float v = xc[c][t];
                    if (scale) { v = __fdiv_rn(v, peak); xc[c][t] = v; }
                    if (q != nullptr) q[CH * t + c] = (short)quantise_s16(v);
                }
            }
        }
    }
}

// grid (tiles of n).  block_max[blockIdx.x] = max |x[c * row_stride + t]| over the tile's t < n and every c
template <int CH>
__global__ __launch_bounds__(CLIP_NT) void clip_block_max_kernel(const float* __restrict__ x, long n, long row_stride, float* __restrict__ block_max) {
    const long tile_begin = (long)blockIdx.x * CLIP_TILE;
    const long tile_end = tile_begin + CLIP_TILE < n ? tile_begin + CLIP_TILE : n;
    uintptr_t bases = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) bases |= reinterpret_cast<uintptr_t>(x + (size_t)c * row_stride);
    const bool wide = (bases & 15) == 0;   // block-uniform
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < CLIP_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * CLIP_NT + threadIdx.x) * 4;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float* __restrict__ xc = x + (size_t)c * row_stride;
            if (t0 + 4 <= tile_end && wide) {
                float v[4];
                ld4(xc + t0, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) m = fmaxf(m, fabsf(v[j]));
            } else {
                for (int j = 0; j < 4; ++j)
                    if (t0 + j < tile_end) m = fmaxf(m, fabsf(xc[t0 + j]));
            }
        }
    }
    publish_block_max<CLIP_NT>(m, block_max + blockIdx.x);
}

void launch_clip_finish(float* x, int ch, int rows, long n, long row_stride, short* pcm, float* peak, const float* block_max, int n_max,
                        int normalize, hipStream_t st) {
    const dim3 grid((normalize != 0 || pcm != nullptr) ? (unsigned)clip_tiles(n) : 1u, (unsigned)rows);
    if (ch == 1)
        hipLaunchKernelGGL(clip_finish_kernel<1>, grid, dim3(CLIP_NT), 0, st, x, row_stride, pcm, peak, block_max, n_max, n, normalize);
    else
        hipLaunchKernelGGL(clip_finish_kernel<2>, grid, dim3(CLIP_NT), 0, st, x, row_stride, pcm, peak, block_max, n_max, n, normalize);
}

void launch_clip_block_max(const float* x, long n, long row_stride, float* block_max, hipStream_t st) {
    hipLaunchKernelGGL(clip_block_max_kernel<2>, dim3((unsigned)clip_tiles(n)), dim3(CLIP_NT), 0, st, x, n, row_stride, block_max);
}

}  // namespace gs
