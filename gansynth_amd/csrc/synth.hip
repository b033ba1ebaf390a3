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

}  // namespace gs

using namespace gs;

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
