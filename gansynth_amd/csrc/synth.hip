// Note sequences: the mixdown of many generated notes into one clip, with envelopes, peak normalisation and 16-bit PCM, on the device
// (GANSynth.synthesize; the rules are this project's own and are stated in include/gansynth_hip.h and DESIGN.md "Note sequences").
//
// Gather form, no atomics.  A block owns MIX_TILE consecutive output samples -- 4 per lane and step, MIX_STEPS steps, the accumulators
// in registers -- and looks up the notes that reach into them: the table is sorted by onset and no note is longer than `length`, so the
// candidates are the contiguous index range with onset in (tile_begin - length, tile_end), found by two binary searches that one wave
// runs once per block.  Every candidate is validated and clipped to the tile; a sample adds its notes in ascending table order, so the
// result is a function of the table alone.  Wave rows are read dword by dword (t - onset is not 16-byte aligned in general), the output
// leaves with 16 bytes per lane, the tail of `total` goes sample by sample.
// Two launches, like gs_summary_image_u8: `note_mix_kernel` leaves the mix in `out` and one |max| per block in the workspace,
// `note_mix_finish_kernel` folds the block maxima in one wave per block (a maximum is exact: the fold order does not show), then
// scales and quantises its own tile.
#include "gs_common.h"
#include "clip_finish.h"

namespace gs {

constexpr int MIX_NT = 256;                     // threads per block
constexpr int MIX_STEPS = 4;                    // 4-sample packs per lane
constexpr int MIX_TILE = MIX_NT * 4 * MIX_STEPS;
static_assert(MIX_TILE == GS_MIX_TILE, "include/gansynth_hip.h states the tile");
static_assert(sizeof(GsMixNote) == 24, "GsMixNote is 24 bytes (gansynth_amd/_lib.py mirrors it)");

static inline long mix_blocks(long total) { return (total + MIX_TILE - 1) / MIX_TILE; }

// first index in [0, n) whose onset is >= x (n when there is none); the table is sorted by onset
__device__ inline int first_onset_at_or_after(const GsMixNote* __restrict__ notes, int n, long x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (notes[mid].onset < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (blocks).  out[t] = mix[t] for the tile's t < total; block_max[blockIdx.x] = max |mix[t]| over them
__global__ __launch_bounds__(MIX_NT) void note_mix_kernel(const float* __restrict__ waves, int rows, long length, long row_stride,
                                                          const GsMixNote* __restrict__ notes, int n_notes, long total,
                                                          float* __restrict__ out, float* __restrict__ block_max) {
#pragma clang fp contract(off)
    const long tile_begin = (long)blockIdx.x * MIX_TILE;
    const long tile_end = tile_begin + MIX_TILE < total ? tile_begin + MIX_TILE : total;
    __shared__ int range[2];
    if (threadIdx.x < 64) {   // one wave searches (every lane the same, uniform loads), lane 0 publishes
        const int first = first_onset_at_or_after(notes, n_notes, tile_begin - length + 1);
        const int last = first_onset_at_or_after(notes, n_notes, tile_end);
        if (threadIdx.x == 0) { range[0] = first; range[1] = last; }
    }
    __syncthreads();
    const int first = range[0], last = range[1];

    float acc[MIX_STEPS][4];
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[u][j] = 0.f;

    for (int i = first; i < last; ++i) {
        const GsMixNote nt = notes[i];
        const long span = (long)nt.hold + (long)nt.release;
        // a bad table must not fault (the Python layer refuses these; an unsorted table can bring any onset here)
        if (nt.row < 0 || nt.row >= rows || nt.hold < 1 || nt.release < 0 || span > length || nt.onset < 0 || nt.onset >= tile_end) continue;
        const long a = nt.onset > tile_begin ? nt.onset : tile_begin;                       // the note clipped to the tile (and so to total)
        const long b = nt.onset + span < tile_end ? nt.onset + span : tile_end;
        if (a >= b) continue;
        const float* __restrict__ w = waves + (size_t)nt.row * row_stride;
        const float inv = __fdiv_rn(1.f, (float)(nt.release + 1));
#pragma unroll
        for (int u = 0; u < MIX_STEPS; ++u) {
            const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
            if (t0 + 4 <= a || t0 >= b) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long t = t0 + j;
                if (t < a || t >= b) continue;
                const long k = t - nt.onset;                                                // 0 <= k < span <= length
                const float env = k < nt.hold ? 1.f : (float)(nt.release - (int)(k - nt.hold)) * inv;
                const float ge = nt.gain * env;
                acc[u][j] = acc[u][j] + ge * w[k];
            }
        }
    }

    float m = 0.f;
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
        if (t0 + 4 <= tile_end && wide) {
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, fabsf(acc[u][j]));
            st4(out + t0, acc[u]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + j < tile_end) { m = fmaxf(m, fabsf(acc[u][j])); out[t0 + j] = acc[u][j]; }
        }
    }
    m = wave_extreme<true>(m);
    __shared__ float part[MIX_NT / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = part[0];
#pragma unroll
        for (int w = 1; w < MIX_NT / 64; ++w) r = fmaxf(r, part[w]);
        block_max[blockIdx.x] = r;
    }
}

// grid (blocks of launch 1, or 1 when only the peak is wanted).  out = mix / peak when `normalize` and peak > 1 (else untouched); pcm from out
__global__ __launch_bounds__(MIX_NT) void note_mix_finish_kernel(float* __restrict__ out, short* __restrict__ pcm, float* __restrict__ peak_out,
                                                                 const float* __restrict__ block_max, int blocks, long total, int normalize) {
    __shared__ float sp;
    if (threadIdx.x < 64) {   // one wave folds every block's maximum
        float m = 0.f;
        for (int s = threadIdx.x; s < blocks; s += 64) m = fmaxf(m, block_max[s]);
        m = wave_extreme<true>(m);
        if (threadIdx.x == 0) sp = m;
    }
    __syncthreads();
    const float peak = sp;
    if (blockIdx.x == 0 && threadIdx.x == 0 && peak_out != nullptr) *peak_out = peak;
    const bool scale = normalize != 0 && peak > 1.f;
    if (!scale && pcm == nullptr) return;
    const long tile_begin = (long)blockIdx.x * MIX_TILE;
    const long tile_end = tile_begin + MIX_TILE < total ? tile_begin + MIX_TILE : total;
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(pcm) & 7) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
        if (t0 + 4 <= tile_end && wide) {
            float v[4];
            ld4(out + t0, v);
            if (scale) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = __fdiv_rn(v[j], peak);
                st4(out + t0, v);
            }
            if (pcm != nullptr)
                *reinterpret_cast<uint2*>(pcm + t0) =
                    make_uint2(((unsigned int)quantise_s16(v[0]) & 0xffffu) | ((unsigned int)quantise_s16(v[1]) << 16),
                               ((unsigned int)quantise_s16(v[2]) & 0xffffu) | ((unsigned int)quantise_s16(v[3]) << 16));
        } else {
            for (int j = 0; j < 4; ++j) {
                const long t = t0 + j;
                if (t >= tile_end) break;
                float v = out[t];
                if (scale) { v = __fdiv_rn(v, peak); out[t] = v; }
                if (pcm != nullptr) pcm[t] = (short)quantise_s16(v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- two channels
// The same gather with two gains per note: a block owns MIX_TILE samples of BOTH channels (2 x 16 accumulators a lane), every wave sample is
// loaded once and enters both sums, and the block's |max| is over both -- one peak for the clip, so that normalising cannot move the
// stereo image.  Operation for operation a channel is note_mix_kernel's sum with that channel's gain.
static_assert(sizeof(GsMixNoteStereo) == 32, "GsMixNoteStereo is 32 bytes (gansynth_amd/_lib.py mirrors it)");

__device__ inline int first_onset_at_or_after(const GsMixNoteStereo* __restrict__ notes, int n, long x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (notes[mid].onset < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the block's |max| from every lane's: one per block into block_max[blockIdx.x]
__device__ inline void publish_block_max(float m, float* __restrict__ block_max) {
    m = wave_extreme<true>(m);
    __shared__ float part[MIX_NT / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = part[0];
#pragma unroll
        for (int w = 1; w < MIX_NT / 64; ++w) r = fmaxf(r, part[w]);
        block_max[blockIdx.x] = r;
    }
}

// grid (blocks).  out[c * out_stride + t] = mix_c[t] for the tile's t < total; block_max[blockIdx.x] = max |mix_c[t]| over them and both c
__global__ __launch_bounds__(MIX_NT) void note_mix_stereo_kernel(const float* __restrict__ waves, int rows, long length, long row_stride,
                                                                 const GsMixNoteStereo* __restrict__ notes, int n_notes, long total,
                                                                 float* __restrict__ out, long out_stride, float* __restrict__ block_max) {
#pragma clang fp contract(off)
    const long tile_begin = (long)blockIdx.x * MIX_TILE;
    const long tile_end = tile_begin + MIX_TILE < total ? tile_begin + MIX_TILE : total;
    __shared__ int range[2];
    if (threadIdx.x < 64) {   // one wave searches (every lane the same, uniform loads), lane 0 publishes
        const int first = first_onset_at_or_after(notes, n_notes, tile_begin - length + 1);
        const int last = first_onset_at_or_after(notes, n_notes, tile_end);
        if (threadIdx.x == 0) { range[0] = first; range[1] = last; }
    }
    __syncthreads();
    const int first = range[0], last = range[1];

    float acc_l[MIX_STEPS][4], acc_r[MIX_STEPS][4];
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_l[u][j] = acc_r[u][j] = 0.f;

    for (int i = first; i < last; ++i) {
        const GsMixNoteStereo nt = notes[i];
        const long span = (long)nt.hold + (long)nt.release;
        // a bad table must not fault: the note is judged before an address is formed from it (as in note_mix_kernel)
        if (nt.row < 0 || nt.row >= rows || nt.hold < 1 || nt.release < 0 || span > length || nt.onset < 0 || nt.onset >= tile_end) continue;
        const long a = nt.onset > tile_begin ? nt.onset : tile_begin;                       // the note clipped to the tile (and so to total)
        const long b = nt.onset + span < tile_end ? nt.onset + span : tile_end;
        if (a >= b) continue;
        const float* __restrict__ w = waves + (size_t)nt.row * row_stride;
        const float inv = __fdiv_rn(1.f, (float)(nt.release + 1));
#pragma unroll
        for (int u = 0; u < MIX_STEPS; ++u) {
            const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
            if (t0 + 4 <= a || t0 >= b) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long t = t0 + j;
                if (t < a || t >= b) continue;
                const long k = t - nt.onset;                                                // 0 <= k < span <= length
                const float env = k < nt.hold ? 1.f : (float)(nt.release - (int)(k - nt.hold)) * inv;
                const float s = w[k];                                                       // loaded once, used on both sides
                const float ge_l = nt.gain_l * env;
                const float ge_r = nt.gain_r * env;
                acc_l[u][j] = acc_l[u][j] + ge_l * s;
                acc_r[u][j] = acc_r[u][j] + ge_r * s;
            }
        }
    }

    float m = 0.f;
    float* __restrict__ out_r = out + out_stride;
    const bool wide = ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(out_r)) & 15) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
        if (t0 + 4 <= tile_end && wide) {
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, fmaxf(fabsf(acc_l[u][j]), fabsf(acc_r[u][j])));
            st4(out + t0, acc_l[u]);
            st4(out_r + t0, acc_r[u]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + j < tile_end) {
                    m = fmaxf(m, fmaxf(fabsf(acc_l[u][j]), fabsf(acc_r[u][j])));
                    out[t0 + j] = acc_l[u][j];
                    out_r[t0 + j] = acc_r[u][j];
                }
        }
    }
    publish_block_max(m, block_max);
}

// grid (blocks).  block_max[blockIdx.x] = max |x[c * row_stride + t]| over the tile's t < n and both c (gs_stereo_finish: a clip the mix did not leave)
__global__ __launch_bounds__(MIX_NT) void stereo_block_max_kernel(const float* __restrict__ x, long n, long row_stride, float* __restrict__ block_max) {
    const long tile_begin = (long)blockIdx.x * MIX_TILE;
    const long tile_end = tile_begin + MIX_TILE < n ? tile_begin + MIX_TILE : n;
    const float* __restrict__ x_r = x + row_stride;
    const bool wide = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_r)) & 15) == 0;   // block-uniform
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
        if (t0 + 4 <= tile_end && wide) {
            float l[4], r[4];
            ld4(x + t0, l);
            ld4(x_r + t0, r);
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, fmaxf(fabsf(l[j]), fabsf(r[j])));
        } else {
            for (int j = 0; j < 4; ++j)
                if (t0 + j < tile_end) m = fmaxf(m, fmaxf(fabsf(x[t0 + j]), fabsf(x_r[t0 + j])));
        }
    }
    publish_block_max(m, block_max);
}

// grid (blocks of the launch before, or 1 when only the peak is wanted).  Both rows of x divided by the ONE peak when `normalize` and
// peak > 1 (else untouched); pcm[t][c] from x.  The second stage of gs_note_mix_stereo and of gs_stereo_finish alike.
__global__ __launch_bounds__(MIX_NT) void stereo_finish_kernel(float* __restrict__ x, long row_stride, short* __restrict__ pcm, float* __restrict__ peak_out,
                                                               const float* __restrict__ block_max, int blocks, long total, int normalize) {
    __shared__ float sp;
    if (threadIdx.x < 64) {   // one wave folds every block's maximum
        float m = 0.f;
        for (int s = threadIdx.x; s < blocks; s += 64) m = fmaxf(m, block_max[s]);
        m = wave_extreme<true>(m);
        if (threadIdx.x == 0) sp = m;
    }
    __syncthreads();
    const float peak = sp;
    if (blockIdx.x == 0 && threadIdx.x == 0 && peak_out != nullptr) *peak_out = peak;
    const bool scale = normalize != 0 && peak > 1.f;
    if (!scale && pcm == nullptr) return;
    const long tile_begin = (long)blockIdx.x * MIX_TILE;
    const long tile_end = tile_begin + MIX_TILE < total ? tile_begin + MIX_TILE : total;
    float* __restrict__ x_r = x + row_stride;
    const bool wide = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_r) | reinterpret_cast<uintptr_t>(pcm)) & 15) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
        if (t0 + 4 <= tile_end && wide) {
            float l[4], r[4];
            ld4(x + t0, l);
            ld4(x_r + t0, r);
            if (scale) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { l[j] = __fdiv_rn(l[j], peak); r[j] = __fdiv_rn(r[j], peak); }
                st4(x + t0, l);
                st4(x_r + t0, r);
            }
            if (pcm != nullptr) {   // four interleaved (left, right) pairs: 16 bytes
                unsigned int p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = ((unsigned int)quantise_s16(l[j]) & 0xffffu) | ((unsigned int)quantise_s16(r[j]) << 16);
                *reinterpret_cast<uint4*>(pcm + 2 * t0) = make_uint4(p[0], p[1], p[2], p[3]);
            }
        } else {
            for (int j = 0; j < 4; ++j) {
                const long t = t0 + j;
                if (t >= tile_end) break;
                float l = x[t], r = x_r[t];
                if (scale) {
                    l = __fdiv_rn(l, peak);
                    r = __fdiv_rn(r, peak);
                    x[t] = l;
                    x_r[t] = r;
                }
                if (pcm != nullptr) { pcm[2 * t] = (short)quantise_s16(l); pcm[2 * t + 1] = (short)quantise_s16(r); }
            }
        }
    }
}

void launch_clip_finish(float* x, int rows, long n, long row_stride, short* pcm, float* peak, const float* block_max, int n_max, int normalize,
                        hipStream_t st) {
    const unsigned grid = (normalize != 0 || pcm != nullptr) ? (unsigned)mix_blocks(n) : 1u;
    if (rows == 1)
        hipLaunchKernelGGL(note_mix_finish_kernel, dim3(grid), dim3(MIX_NT), 0, st, x, pcm, peak, block_max, n_max, n, normalize);
    else
        hipLaunchKernelGGL(stereo_finish_kernel, dim3(grid), dim3(MIX_NT), 0, st, x, row_stride, pcm, peak, block_max, n_max, n, normalize);
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_note_mix_stereo_workspace_bytes(int64_t total) {
    if (total <= 0) return 0;
    return (size_t)mix_blocks((long)total) * sizeof(float);
}

extern "C" int gs_note_mix_stereo(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNoteStereo* notes, int n_notes,
                                  int64_t total, int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes,
                                  void* stream) {
    GS_CHECK_ARG(n_notes > 0, "note_mix_stereo: n_notes must be positive (got %d)", n_notes);
    GS_CHECK_ARG(total > 0, "note_mix_stereo: total must be positive (got %lld)", (long long)total);
    GS_CHECK_ARG(rows > 0, "note_mix_stereo: rows must be positive (got %d)", rows);
    GS_CHECK_ARG(length > 0, "note_mix_stereo: length must be positive (got %lld)", (long long)length);
    GS_CHECK_ARG(row_stride >= length, "note_mix_stereo: row_stride %lld is below length %lld", (long long)row_stride, (long long)length);
    GS_CHECK_ARG(out_stride >= total, "note_mix_stereo: out_stride %lld is below total %lld", (long long)out_stride, (long long)total);
    GS_CHECK_ARG(waves && notes && out, "note_mix_stereo: null pointer (waves, notes and out are required)");
    GS_CHECK_ARG(mix_blocks((long)total) <= 0x7fffffffL && length <= 0x7fffffffL, "note_mix_stereo: clip or note too long (total %lld, length %lld)",
                 (long long)total, (long long)length);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(notes) & 7) == 0, "note_mix_stereo: misaligned pointer (notes must be 8-byte aligned)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(waves) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(peak) & 3) == 0, "note_mix_stereo: misaligned pointer (waves, out and peak must be 4-byte aligned)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(pcm) & 1) == 0, "note_mix_stereo: misaligned pointer (pcm must be 2-byte aligned)");
    GS_CHECK_ARG(ws && ws_bytes >= gs_note_mix_stereo_workspace_bytes(total) && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "note_mix_stereo: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, gs_note_mix_stereo_workspace_bytes(total));
    hipStream_t st = as_stream(stream);
    const int blocks = (int)mix_blocks((long)total);
    float* block_max = static_cast<float*>(ws);
    hipLaunchKernelGGL(note_mix_stereo_kernel, dim3((unsigned)blocks), dim3(MIX_NT), 0, st, waves, rows, (long)length, (long)row_stride, notes, n_notes,
                       (long)total, out, (long)out_stride, block_max);
    if (normalize != 0 || pcm != nullptr || peak != nullptr)
        hipLaunchKernelGGL(stereo_finish_kernel, dim3((unsigned)((normalize != 0 || pcm != nullptr) ? blocks : 1)), dim3(MIX_NT), 0, st, out,
                           (long)out_stride, reinterpret_cast<short*>(pcm), peak, static_cast<const float*>(block_max), blocks, (long)total, normalize);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_stereo_finish_workspace_bytes(int64_t n) { return gs_note_mix_stereo_workspace_bytes(n); }

extern "C" int gs_stereo_finish(float* x, int64_t n, int64_t row_stride, int normalize, int16_t* pcm, float* peak, void* ws, size_t ws_bytes,
                                void* stream) {
    GS_CHECK_ARG(n > 0, "stereo_finish: n must be positive (got %lld)", (long long)n);
    GS_CHECK_ARG(row_stride >= n, "stereo_finish: row_stride %lld is below n %lld", (long long)row_stride, (long long)n);
    GS_CHECK_ARG(x != nullptr, "stereo_finish: null pointer (x is required)");
    GS_CHECK_ARG(mix_blocks((long)n) <= 0x7fffffffL, "stereo_finish: clip too long (n %lld)", (long long)n);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(peak) & 3) == 0,
                 "stereo_finish: misaligned pointer (x and peak must be 4-byte aligned)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(pcm) & 1) == 0, "stereo_finish: misaligned pointer (pcm must be 2-byte aligned)");
    GS_CHECK_ARG(ws && ws_bytes >= gs_stereo_finish_workspace_bytes(n) && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "stereo_finish: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, gs_stereo_finish_workspace_bytes(n));
    if (normalize == 0 && pcm == nullptr && peak == nullptr) return 0;   // nothing is asked for
    hipStream_t st = as_stream(stream);
    const int blocks = (int)mix_blocks((long)n);
    float* block_max = static_cast<float*>(ws);
    hipLaunchKernelGGL(stereo_block_max_kernel, dim3((unsigned)blocks), dim3(MIX_NT), 0, st, static_cast<const float*>(x), (long)n, (long)row_stride,
                       block_max);
    hipLaunchKernelGGL(stereo_finish_kernel, dim3((unsigned)((normalize != 0 || pcm != nullptr) ? blocks : 1)), dim3(MIX_NT), 0, st, x,
                       (long)row_stride, reinterpret_cast<short*>(pcm), peak, static_cast<const float*>(block_max), blocks, (long)n, normalize);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_note_mix_workspace_bytes(int64_t total) {
    if (total <= 0) return 0;
    return (size_t)mix_blocks((long)total) * sizeof(float);
}

extern "C" int gs_note_mix(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNote* notes, int n_notes, int64_t total,
                           int normalize, float* out, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(n_notes > 0, "note_mix: n_notes must be positive (got %d)", n_notes);
    GS_CHECK_ARG(total > 0, "note_mix: total must be positive (got %lld)", (long long)total);
    GS_CHECK_ARG(rows > 0, "note_mix: rows must be positive (got %d)", rows);
    GS_CHECK_ARG(length > 0, "note_mix: length must be positive (got %lld)", (long long)length);
    GS_CHECK_ARG(row_stride >= length, "note_mix: row_stride %lld is below length %lld", (long long)row_stride, (long long)length);
    GS_CHECK_ARG(waves && notes && out, "note_mix: null pointer (waves, notes and out are required)");
    GS_CHECK_ARG(mix_blocks((long)total) <= 0x7fffffffL && length <= 0x7fffffffL, "note_mix: clip or note too long (total %lld, length %lld)",
                 (long long)total, (long long)length);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(notes) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(pcm) & 1) == 0, "note_mix: misaligned pointer");
    GS_CHECK_ARG(ws && ws_bytes >= gs_note_mix_workspace_bytes(total) && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "note_mix: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, gs_note_mix_workspace_bytes(total));
    hipStream_t st = as_stream(stream);
    const int blocks = (int)mix_blocks((long)total);
    float* block_max = static_cast<float*>(ws);
    hipLaunchKernelGGL(note_mix_kernel, dim3((unsigned)blocks), dim3(MIX_NT), 0, st, waves, rows, (long)length, (long)row_stride, notes, n_notes,
                       (long)total, out, block_max);
    if (normalize != 0 || pcm != nullptr || peak != nullptr)
        hipLaunchKernelGGL(note_mix_finish_kernel, dim3((unsigned)((normalize != 0 || pcm != nullptr) ? blocks : 1)), dim3(MIX_NT), 0, st, out,
                           reinterpret_cast<short*>(pcm), peak, static_cast<const float*>(block_max), blocks, (long)total, normalize);
    GS_CHECK_LAUNCH();
    return 0;
}
