// Controller curves: the note mixdown of synth.hip with a gain that is a function of clip time (GANSynth.synthesize with controllers;
// the rules are this project's own and are stated in include/gansynth_hip.h and DESIGN.md "Controllers").
//
// synth.hip's gather form, no atomics: a block owns MIX_TILE consecutive samples of every channel, the accumulators in registers, and
// finds its candidate notes by two binary searches on the onsets.  A note names a curve (its part's); the curve's value depends on
// (curve, t) and not on the note, and the note loop is block-uniform, so a lane keeps the curve values of its 16 samples -- per channel --
// in registers and evaluates them again only when the next valid candidate names another curve.  That evaluation: in the curve's range of
// `points` (clamped into [0, n_points) before anything is read) every wave finds the last point at or before the tile's first sample by a
// 64-way search, every thread brings one point from there on into LDS, and a lane searches that window for each of its four packs and
// walks on through the pack's four samples (a tile that needs more than 256 points of one curve searches global memory instead).
// A one-point curve costs one uniform load.  The finish (peak, quotient, PCM) is clip_finish.hip's, as for the other mixes.
#include "gs_common.h"
#include "clip_finish.h"
#include "mix_shared.h"

#pragma clang fp contract(off)

namespace gs {

static_assert(MIX_TILE == CLIP_TILE, "the finish folds one |max| per mix tile");
static_assert(sizeof(GsMixNoteCurve) == 32, "GsMixNoteCurve is 32 bytes (gansynth_amd/_lib.py mirrors it)");
static_assert(sizeof(GsCurvePoint) == 16, "GsCurvePoint is 16 bytes (gansynth_amd/_lib.py mirrors it)");

// first index in [lo, hi) whose pos is > t (hi when there is none); every index read lies in [lo, hi), whatever the positions hold
__device__ inline int first_pos_after(const GsCurvePoint* __restrict__ points, int lo, int hi, long t) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (points[mid].pos <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first_pos_after by one wave, 64 probes a round: three dependent rounds for 20000 points where the binary search takes fifteen.  The
// result is the same in every lane; with positions out of order it is some index of [lo, hi], and every index read lies in [lo, hi).
__device__ inline int first_pos_after_wave(const GsCurvePoint* __restrict__ points, int lo, int hi, long t) {
    const int lane = threadIdx.x & 63;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const long probe = (long)lo + (long)lane * step;
        const bool before = probe < hi && points[probe].pos <= t;       // (sorted: true for the first `count` lanes)
        const int count = __popcll(__ballot(before));
        if (count == 0) { hi = lo; break; }
        const long top = (long)lo + (long)count * step;                 // the answer lies in (lo + (count - 1) step, min(top, hi)]
        lo = lo + (count - 1) * step + 1;
        hi = top < hi ? (int)top : hi;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// The curve over points[lo, hi) (0 <= lo < hi <= n_points) at the four samples t0 .. t0 + 3, per channel, in the stated fp32 order.
// [s0, s1] (lo <= s0 <= s1 <= hi) holds, for every t of the tile, the first index whose pos is > t.
template <int CH>
__device__ inline void curve_pack(const GsCurvePoint* __restrict__ points, int lo, int hi, int s0, int s1, long t0, float (&cv)[CH][4]) {
#pragma clang fp contract(off)
    int k = first_pos_after(points, s0, s1, t0);
    int held = -1;                       // the k whose segment is in the registers below
    bool flat = true;
    long p0 = 0;
    float inv = 0.f, v0[CH], dv[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) { v0[c] = 0.f; dv[c] = 0.f; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long t = t0 + j;
        while (k < s1 && points[k].pos <= t) ++k;                // (k < s1 <= hi: the index read is inside the range)
        if (k != held) {
            held = k;
            // the segment [k - 1, k]; before the first point and from the last one on the curve is constant
            const int i0 = k - 1 < lo ? lo : k - 1;             // in [lo, hi)
            const int i1 = k < hi ? k : hi - 1;                  // in [lo, hi)
            const GsCurvePoint a = points[i0], b = points[i1];
            const long d = b.pos - a.pos;
            flat = i0 == i1 || k - 1 < lo || d <= 0;             // a zero-length (or backward) segment is never divided by
            p0 = a.pos;
            inv = flat ? 0.f : __fdiv_rn(1.f, (float)d);
            v0[0] = a.v_l;
            dv[0] = b.v_l - a.v_l;
            if (CH == 2) { v0[CH - 1] = a.v_r; dv[CH - 1] = b.v_r - a.v_r; }
        }
        const float x = (float)(t - p0) * inv;
#pragma unroll
        for (int c = 0; c < CH; ++c) cv[c][j] = flat ? v0[c] : v0[c] + x * dv[c];
    }
}

// grid (blocks).  out[c * out_stride + t] = mix_c[t] for the tile's t < total (one channel: out_stride is not read);
// block_max[blockIdx.x] = max |mix_c[t]| over them and every c
template <int CH>
__global__ __launch_bounds__(MIX_NT) void note_mix_curves_kernel(const float* __restrict__ waves, int rows, long length, long row_stride,
                                                                 const GsMixNoteCurve* __restrict__ notes, int n_notes,
                                                                 const GsCurvePoint* __restrict__ points, int n_points,
                                                                 const int* __restrict__ first_point, int n_curves, long total,
                                                                 float* __restrict__ out, long out_stride, float* __restrict__ block_max) {
#pragma clang fp contract(off)
    const long tile_begin = (long)blockIdx.x * MIX_TILE;
    const long tile_end = tile_begin + MIX_TILE < total ? tile_begin + MIX_TILE : total;
    __shared__ int range[2];
    __shared__ GsCurvePoint window[MIX_NT];   // the current curve's points around the tile, one a thread
    if (threadIdx.x < 64) {   // one wave searches (every lane the same, uniform loads), lane 0 publishes
        const int first = first_onset_at_or_after(notes, n_notes, tile_begin - length + 1);
        const int last = first_onset_at_or_after(notes, n_notes, tile_end);
        if (threadIdx.x == 0) { range[0] = first; range[1] = last; }
    }
    __syncthreads();
    const int first = range[0], last = range[1];

    float acc[CH][MIX_STEPS][4], cv[MIX_STEPS][CH][4];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int u = 0; u < MIX_STEPS; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[c][u][j] = 0.f; cv[u][c][j] = 0.f; }
    int current = -1;   // the curve whose values cv holds (block-uniform)

    for (int i = first; i < last; ++i) {
        const GsMixNoteCurve nt = notes[i];
        const long span = (long)nt.hold + (long)nt.release;
        // a bad table must not fault: the note is judged before an address is formed from it
        if (nt.row < 0 || nt.row >= rows || nt.hold < 1 || nt.release < 0 || span > length || nt.onset < 0 || nt.onset >= tile_end ||
            nt.curve < 0 || nt.curve >= n_curves) continue;
        const long a = nt.onset > tile_begin ? nt.onset : tile_begin;                       // the note clipped to the tile (and so to total)
        const long b = nt.onset + span < tile_end ? nt.onset + span : tile_end;
        if (a >= b) continue;
        if (nt.curve != current) {   // block-uniform: another part's curve over this lane's 16 samples
            current = nt.curve;
            int lo = first_point[nt.curve], hi = first_point[nt.curve + 1];                // 0 <= curve < n_curves: first_point has n_curves + 1 entries
            lo = lo < 0 ? 0 : (lo > n_points - 1 ? n_points - 1 : lo);                      // clamped: 0 <= lo < hi <= n_points, whatever the table says
            hi = hi > n_points ? n_points : hi;
            hi = hi < lo + 1 ? lo + 1 : hi;
            if (hi - lo == 1) {                                                             // a constant: one uniform load
                const GsCurvePoint p = points[lo];
#pragma unroll
                for (int u = 0; u < MIX_STEPS; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        cv[u][0][j] = p.v_l;
                        if (CH == 2) cv[u][CH - 1][j] = p.v_r;
                    }
            } else {
                // the points that matter inside the tile start with the last one at or before its first sample: every wave finds it,
                // every thread brings one point from there on into LDS, and the lanes search there
                const long tile_last = tile_begin + MIX_TILE - 1;
                const int s0 = first_pos_after_wave(points, lo, hi, tile_begin);
                const int base = s0 - 1 < lo ? lo : s0 - 1;                                 // in [lo, hi)
                const int held = hi - base < MIX_NT ? hi - base : MIX_NT;                   // 1 .. MIX_NT points of the window count
                __syncthreads();                                                            // (the lanes are done with the window before)
                window[threadIdx.x] = points[base + ((int)threadIdx.x < held ? (int)threadIdx.x : held - 1)];
                __syncthreads();
                if (base + held == hi || window[MIX_NT - 1].pos > tile_last) {              // block-uniform: the window holds all the tile needs
#pragma unroll
                    for (int u = 0; u < MIX_STEPS; ++u)
                        curve_pack<CH>(window, 0, held, 0, held, tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4, cv[u]);
                } else {                                                                    // more than MIX_NT points in one tile: from global memory
                    const int s1 = first_pos_after(points, s0, hi, tile_last);
#pragma unroll
                    for (int u = 0; u < MIX_STEPS; ++u)
                        curve_pack<CH>(points, lo, hi, s0, s1, tile_begin + ((long)u * MIX_NT + threadIdx.x) * 4, cv[u]);
                }
            }
        }
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
                const float ge = nt.gain * env;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const float g = ge * cv[u][c][j];
                    acc[c][u][j] = acc[c][u][j] + g * s;
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

}  // namespace gs

using namespace gs;

extern "C" size_t gs_note_mix_curves_workspace_bytes(int64_t total) {
    if (total <= 0) return 0;
    return (size_t)mix_blocks((long)total) * sizeof(float);
}

extern "C" int gs_note_mix_curves(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNoteCurve* notes, int n_notes,
                                  const GsCurvePoint* points, int n_points, const int32_t* first, int n_curves, int channels, int64_t total,
                                  int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream) {
    const char* name = "note_mix_curves";
    GS_CHECK_ARG(channels == 1 || channels == 2, "%s: channels must be 1 or 2 (got %d)", name, channels);
    GS_CHECK_ARG(n_points > 0, "%s: n_points must be positive (got %d)", name, n_points);
    GS_CHECK_ARG(n_curves > 0, "%s: n_curves must be positive (got %d)", name, n_curves);
    GS_CHECK_ARG(points && first, "%s: null pointer (points and first are required)", name);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(points) & 7) == 0, "%s: misaligned pointer (points must be 8-byte aligned)", name);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(first) & 3) == 0, "%s: misaligned pointer (first must be 4-byte aligned)", name);
    // the stereo mix's conditions for either channel count (one channel: out is one row, out_stride is not read)
    const int64_t stride = channels == 1 ? total : out_stride;
    const int code = check_mix(name, 2, waves, rows, length, row_stride, notes, n_notes, total, out, stride, pcm, peak, ws, ws_bytes);
    if (code != 0) return code;
    hipStream_t st = as_stream(stream);
    const int blocks = (int)mix_blocks((long)total);
    float* block_max = static_cast<float*>(ws);
    if (channels == 1)
        hipLaunchKernelGGL(note_mix_curves_kernel<1>, dim3((unsigned)blocks), dim3(MIX_NT), 0, st, waves, rows, (long)length, (long)row_stride, notes,
                           n_notes, points, n_points, first, n_curves, (long)total, out, (long)stride, block_max);
    else
        hipLaunchKernelGGL(note_mix_curves_kernel<2>, dim3((unsigned)blocks), dim3(MIX_NT), 0, st, waves, rows, (long)length, (long)row_stride, notes,
                           n_notes, points, n_points, first, n_curves, (long)total, out, (long)stride, block_max);
    if (normalize != 0 || pcm != nullptr || peak != nullptr)
        launch_clip_finish(out, channels, 1, (long)total, (long)stride, reinterpret_cast<short*>(pcm), peak, block_max, blocks, normalize, st);
    GS_CHECK_LAUNCH();
    return 0;
}
