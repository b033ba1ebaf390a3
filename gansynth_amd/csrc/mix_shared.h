// What the note mixes share (synth.hip: gs_note_mix, gs_note_mix_stereo; mix_curves.hip: gs_note_mix_curves): the tile, the search of
// the onsets, and the host checks of their arguments.
#pragma once
#include "gs_common.h"

namespace gs {

constexpr int MIX_NT = 256;                     // threads per block
constexpr int MIX_STEPS = 4;                    // 4-sample packs per lane
constexpr int MIX_TILE = MIX_NT * 4 * MIX_STEPS;
static_assert(MIX_TILE == GS_MIX_TILE, "include/gansynth_hip.h states the tile");

static inline long mix_blocks(long total) { return (total + MIX_TILE - 1) / MIX_TILE; }

// first index in [0, n) whose onset is >= x (n when there is none); the table is sorted by onset
template <class Note>
__device__ inline int first_onset_at_or_after(const Note* __restrict__ notes, int n, long x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (notes[mid].onset < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------------------- host: the checks
// the pointer part of every entry point here: the PCM and the workspace of one |max| per tile of n samples
static inline int check_clip_out(const char* name, const void* pcm, const void* ws, size_t ws_bytes, long n) {
    const size_t need = (size_t)mix_blocks(n) * sizeof(float);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(pcm) & 1) == 0, "%s: misaligned pointer (pcm must be 2-byte aligned)", name);
    GS_CHECK_ARG(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 3) == 0, "%s: workspace too small or misaligned (%zu bytes, need %zu)",
                 name, ws_bytes, need);
    return 0;
}

// what gs_note_mix and gs_note_mix_stereo ask of their arguments, under the entry point's `name` (ch 1 or 2; out_stride is read for 2)
static inline int check_mix(const char* name, int ch, const float* waves, int rows, int64_t length, int64_t row_stride, const void* notes,
                            int n_notes, int64_t total, const float* out, int64_t out_stride, const void* pcm, const float* peak, const void* ws,
                            size_t ws_bytes) {
    GS_CHECK_ARG(n_notes > 0, "%s: n_notes must be positive (got %d)", name, n_notes);
    GS_CHECK_ARG(total > 0, "%s: total must be positive (got %lld)", name, (long long)total);
    GS_CHECK_ARG(rows > 0, "%s: rows must be positive (got %d)", name, rows);
    GS_CHECK_ARG(length > 0, "%s: length must be positive (got %lld)", name, (long long)length);
    GS_CHECK_ARG(row_stride >= length, "%s: row_stride %lld is below length %lld", name, (long long)row_stride, (long long)length);
    GS_CHECK_ARG(ch == 1 || out_stride >= total, "%s: out_stride %lld is below total %lld", name, (long long)out_stride, (long long)total);
    GS_CHECK_ARG(waves && notes && out, "%s: null pointer (waves, notes and out are required)", name);
    GS_CHECK_ARG(mix_blocks((long)total) <= 0x7fffffffL && length <= 0x7fffffffL, "%s: clip or note too long (total %lld, length %lld)", name,
                 (long long)total, (long long)length);
    if (ch == 1) {   // (the one-channel entry point names no pointer and does not look at waves and peak)
        GS_CHECK_ARG((reinterpret_cast<uintptr_t>(notes) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(pcm) & 1) == 0, "%s: misaligned pointer", name);
    } else {
        GS_CHECK_ARG((reinterpret_cast<uintptr_t>(notes) & 7) == 0, "%s: misaligned pointer (notes must be 8-byte aligned)", name);
        GS_CHECK_ARG((reinterpret_cast<uintptr_t>(waves) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(peak) & 3) == 0, "%s: misaligned pointer (waves, out and peak must be 4-byte aligned)", name);
    }
    return check_clip_out(name, pcm, ws, ws_bytes, (long)total);
}

}  // namespace gs
