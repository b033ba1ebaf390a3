// Note sequences: the mixdown of many generated notes into one clip of one or two channels, with envelopes, on the device
// (GANSynth.synthesize; the rules are this project's own and are stated in include/gansynth_hip.h and DESIGN.md "Note sequences").
//
// Gather form, no atomics.  A block owns MIX_TILE consecutive output samples of every channel -- 4 per lane and step, MIX_STEPS steps,
// the accumulators in registers -- and looks up the notes that reach into them: the table is sorted by onset and no note is longer than
// `length`, so the candidates are the contiguous index range with onset in (tile_begin - length, tile_end), found by two binary searches
// that one wave runs once per block.  Every candidate is validated and clipped to the tile; a sample adds its notes in ascending table
// order, so the result is a function of the table alone.  Wave rows are read dword by dword (t - onset is not 16-byte aligned in general),
// the output leaves with 16 bytes per lane, the tail of `total` goes sample by sample.
// ONE kernel for GsMixNote (one gain, one channel) and GsMixNoteStereo (two gains, two channels): a wave sample is loaded once and enters
// every channel's sum with that channel's gain, so a stereo channel IS the mono sum, and the block's |max| is over all channels -- one
// peak for the clip, so that normalising cannot move the stereo image.
// Two launches, like gs_summary_image_u8: `note_mix_kernel` leaves the mix in `out` and one |max| per block in the workspace, the finish
// of clip_finish.hip folds them, then scales and quantises.
#include <type_traits>

#include "gs_common.h"
#include "clip_finish.h"
#include "mix_shared.h"   // the tile, the onset search and the host checks, shared with mix_curves.hip

namespace gs {

static_assert(MIX_TILE == CLIP_TILE, "gs_stereo_finish sizes the workspace of launch_clip_block_max by mix_blocks");
static_assert(sizeof(GsMixNote) == 24, "GsMixNote is 24 bytes (gansynth_amd/_lib.py mirrors it)");
static_assert(sizeof(GsMixNoteStereo) == 32, "GsMixNoteStereo is 32 bytes (gansynth_amd/_lib.py mirrors it)");

// the channels of a note struct and the gain of channel c
template <class Note> constexpr int mix_channels = std::is_same<Note, GsMixNoteStereo>::value ? 2 : 1;
__device__ inline float mix_gain(const GsMixNote& nt, int) { return nt.gain; }
__device__ inline float mix_gain(const GsMixNoteStereo& nt, int c) { return c == 0 ? nt.gain_l : nt.gain_r; }

// grid (blocks).  out[c * out_stride + t] = mix_c[t] for the tile's t < total (one channel: out_stride is not read);
// block_max[blockIdx.x] = max |mix_c[t]| over them and every c
template <class Note>
__global__ __launch_bounds__(MIX_NT) void note_mix_kernel(const float* __restrict__ waves, int rows, long length, long row_stride,
                                                          const Note* __restrict__ notes, int n_notes, long total, float* __restrict__ out,
                                                          long out_stride, float* __restrict__ block_max) {
#pragma clang fp contract(off)
    constexpr int CH = mix_channels<Note>;
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

    float acc[CH][MIX_STEPS][4];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int u = 0; u < MIX_STEPS; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c][u][j] = 0.f;

    for (int i = first; i < last; ++i) {
        const Note nt = notes[i];
        const long span = (long)nt.hold + (long)nt.release;
        // a bad table must not fault: the note is judged before an address is formed from it (the Python layer refuses these; an
        // unsorted table can bring any onset here)
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
                const float s = w[k];                                                       // loaded once, used by every channel
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const float ge = mix_gain(nt, c) * env;
                    acc[c][u][j] = acc[c][u][j] + ge * s;
                }
            }
        }
    }

    float m = 0.f;
    uintptr_t bases = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) bases |= reinterpret_cast<uintptr_t>(out + (size_t)c * out_stride);
    const bool wide = (bases & 15) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < MIX_STEPS; ++u) {
        const long t0 = tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float* __restrict__ oc = out + (size_t)c * out_stride;
            if (t0 + 4 <= tile_end && wide) {
#pragma unroll
                for (int j = 0; j < 4; ++j) m = fmaxf(m, fabsf(acc[c][u][j]));
                st4(oc + t0, acc[c][u]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t0 + j < tile_end) { m = fmaxf(m, fabsf(acc[c][u][j])); oc[t0 + j] = acc[c][u][j]; }
            }
        }
    }
    publish_block_max<MIX_NT>(m, block_max + blockIdx.x);
}

// both mixes: the checks, the kernel, the finish when anything of it is asked for
template <class Note>
static int note_mix(const char* name, const float* waves, int rows, int64_t length, int64_t row_stride, const Note* notes, int n_notes, int64_t total,
                    int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream) {
    constexpr int CH = mix_channels<Note>;
    const int code = check_mix(name, CH, waves, rows, length, row_stride, notes, n_notes, total, out, out_stride, pcm, peak, ws, ws_bytes);
    if (code != 0) return code;
    hipStream_t st = as_stream(stream);
    const int blocks = (int)mix_blocks((long)total);
    float* block_max = static_cast<float*>(ws);
    hipLaunchKernelGGL(note_mix_kernel<Note>, dim3((unsigned)blocks), dim3(MIX_NT), 0, st, waves, rows, (long)length, (long)row_stride, notes, n_notes,
                       (long)total, out, (long)out_stride, block_max);
    if (normalize != 0 || pcm != nullptr || peak != nullptr)
        launch_clip_finish(out, CH, 1, (long)total, (long)out_stride, reinterpret_cast<short*>(pcm), peak, block_max, blocks, normalize, st);
    GS_CHECK_LAUNCH();
    return 0;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_note_mix_workspace_bytes(int64_t total) {
    if (total <= 0) return 0;
    return (size_t)mix_blocks((long)total) * sizeof(float);
}

extern "C" int gs_note_mix(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNote* notes, int n_notes, int64_t total,
                           int normalize, float* out, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream) {
    return note_mix("note_mix", waves, rows, length, row_stride, notes, n_notes, total, normalize, out, total, pcm, peak, ws, ws_bytes, stream);
}

extern "C" size_t gs_note_mix_stereo_workspace_bytes(int64_t total) { return gs_note_mix_workspace_bytes(total); }

extern "C" int gs_note_mix_stereo(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNoteStereo* notes, int n_notes,
                                  int64_t total, int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes,
                                  void* stream) {
    return note_mix("note_mix_stereo", waves, rows, length, row_stride, notes, n_notes, total, normalize, out, out_stride, pcm, peak, ws, ws_bytes,
                    stream);
}

extern "C" size_t gs_stereo_finish_workspace_bytes(int64_t n) { return gs_note_mix_workspace_bytes(n); }

extern "C" int gs_stereo_finish(float* x, int64_t n, int64_t row_stride, int normalize, int16_t* pcm, float* peak, void* ws, size_t ws_bytes,
                                void* stream) {
    GS_CHECK_ARG(n > 0, "stereo_finish: n must be positive (got %lld)", (long long)n);
    GS_CHECK_ARG(row_stride >= n, "stereo_finish: row_stride %lld is below n %lld", (long long)row_stride, (long long)n);
    GS_CHECK_ARG(x != nullptr, "stereo_finish: null pointer (x is required)");
    GS_CHECK_ARG(mix_blocks((long)n) <= 0x7fffffffL, "stereo_finish: clip too long (n %lld)", (long long)n);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(peak) & 3) == 0,
                 "stereo_finish: misaligned pointer (x and peak must be 4-byte aligned)");
    const int code = check_clip_out("stereo_finish", pcm, ws, ws_bytes, (long)n);
    if (code != 0) return code;
    if (normalize == 0 && pcm == nullptr && peak == nullptr) return 0;   // nothing is asked for
    hipStream_t st = as_stream(stream);
    float* block_max = static_cast<float*>(ws);
    launch_clip_block_max(x, (long)n, (long)row_stride, block_max, st);
    launch_clip_finish(x, 2, 1, (long)n, (long)row_stride, reinterpret_cast<short*>(pcm), peak, block_max, (int)mix_blocks((long)n), normalize, st);
    GS_CHECK_LAUNCH();
    return 0;
}
