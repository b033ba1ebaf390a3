// The finishing stage of every rendered clip (clip_finish.hip): its producer -- the note mixes of synth.hip, resample.hip, fftconv.hip --
// leaves the samples together with one |max| per block (publish_block_max); the finish folds those into a peak, divides by it when
// `normalize` and peak > 1, and quantises to 16-bit PCM.  gs_stereo_finish, for a clip that no producer left, takes the maxima first.
#pragma once
#include "gs_common.h"

namespace gs {

constexpr int CLIP_NT = 256;                      // threads per block
constexpr int CLIP_STEPS = 4;                     // 4-sample packs per lane
constexpr int CLIP_TILE = CLIP_NT * 4 * CLIP_STEPS;

// the maximum of every thread's m (each a chain of fmaxf from 0: never NaN) over a block of NT threads, in every thread.  Once per kernel.
template <int NT>
__device__ inline float block_max_of(float m) {
    m = wave_extreme<true>(m);
    __shared__ float part[NT / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = part[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = fmaxf(r, part[w]);
    return r;
}

// a producer's last step: the block's |max| from every lane's, into its slot of the workspace
template <int NT>
__device__ inline void publish_block_max(float m, float* __restrict__ slot) {
    const float r = block_max_of<NT>(m);
    if (threadIdx.x == 0) *slot = r;
}

// the minimum counterparts (limiter.hip: the deepest gain; every thread's m a chain of fminf from +inf over values that are never NaN)
template <int NT>
__device__ inline float block_min_of(float m) {
    m = wave_extreme<false>(m);
    __shared__ float part[NT / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = part[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = fminf(r, part[w]);
    return r;
}

template <int NT>
__device__ inline void publish_block_min(float m, float* __restrict__ slot) {
    const float r = block_min_of<NT>(m);
    if (threadIdx.x == 0) *slot = r;
}

// Finishes `rows` clips of `ch` channels (1 or 2) IN PLACE: channel c of clip r is the n samples at x + (r * ch + c) * row_stride.
// block_max: n_max maxima per clip (over all its channels: ONE peak a clip), clip r's at block_max + r * n_max; peak[r] = their fold.
// pcm: clip r's n * ch values at pcm + r * n * ch, the channels interleaved.  pcm / peak may be null; the caller skips the call when
// nothing is asked for.  One launch.
void launch_clip_finish(float* x, int ch, int rows, long n, long row_stride, short* pcm, float* peak, const float* block_max, int n_max,
                        int normalize, hipStream_t st);

// for a two-channel clip that no producer left: block_max[b] = max |x[c * row_stride + t]| over tile b's t < n and both c, (n + CLIP_TILE - 1) / CLIP_TILE slots
void launch_clip_block_max(const float* x, long n, long row_stride, float* block_max, hipStream_t st);

}  // namespace gs
