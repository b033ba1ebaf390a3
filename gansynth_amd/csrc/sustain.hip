// Sustain: notes held past the generated length (GANSynth.synthesize with sustain; the rule is this project's own and is stated in
// include/gansynth_hip.h and DESIGN.md "Sustain").  Two launches ahead of the mix, which stays what it is:
//
// gs_loop_search: a 256-lane block owns SUS_LAGS consecutive lags of one note (grid: lag tiles x notes).  It stages the window
// x[a .. a + W) and the span x[a + m0 .. a + m0 + SUS_LAGS - 1 + W) in LDS, zero-filled past the row's end, and lane l correlates the
// window with the span at its own lag m0 + l: per four taps one 16-byte broadcast read of the window and four dword reads of the span
// (consecutive over the wave: no bank conflict), eight FMAs into four chains of S_ab and four of S_bb by tap index mod 4.  S_aa is the
// block's own sum over the staged window (a chain per lane, then the fixed tree of block_sum), so there is no second launch and no
// workspace.  A fixed order and no atomics: two calls agree bit for bit.
//
// gs_note_sustain: a 256-lane block owns SUS_TILE consecutive outputs of one job (grid: tiles x jobs), four consecutive ones per lane.
// A lane takes (k - b) mod m once, in 64 bits, and steps it; an output reads at most two source samples, and the four leave as one
// 16-byte store where the destination allows it.  Every operation rounded on its own (contract off): bit for bit the fp32 restatement.
#include <math.h>

#include "gs_common.h"

namespace gs {

constexpr int SUS_NT = 256;                              // threads per block (both kernels)
constexpr int SUS_LAGS = GS_SUSTAIN_LAG_TILE;            // lags per block: one per lane
constexpr int SUS_MAX_W = GS_SUSTAIN_MAX_WINDOW;
constexpr int SUS_SPAN = SUS_LAGS + SUS_MAX_W;           // staged span: xs[s] = x[a + m0 + s], s < SUS_LAGS - 1 + W (rounded up to 4)
constexpr int SUS_TILE = GS_SUSTAIN_TILE;
static_assert(SUS_LAGS == SUS_NT, "one lag per lane");
static_assert(SUS_TILE == SUS_NT * 4, "four outputs per lane");
static_assert(SUS_MAX_W % 4 == 0, "the window is staged as whole float4s");
static_assert((SUS_MAX_W + SUS_SPAN) * sizeof(float) < 34 * 1024, "window and span stay under 34 KB of LDS");
static_assert(sizeof(GsLoopNote) == 24, "GsLoopNote is 24 bytes (gansynth_amd/_lib.py mirrors it)");
static_assert(sizeof(GsSustainJob) == 32, "GsSustainJob is 32 bytes (gansynth_amd/_lib.py mirrors it)");

// grid (lag tiles, notes).  scores[note * scores_stride + (m - m_min)] for the tile's m <= m_max
__global__ __launch_bounds__(SUS_NT) void loop_search_kernel(const float* __restrict__ waves, int rows, long length, long row_stride,
                                                             const GsLoopNote* __restrict__ notes, float* __restrict__ scores,
                                                             long scores_stride) {
    __shared__ __attribute__((aligned(16))) float ws[SUS_MAX_W];
    __shared__ __attribute__((aligned(16))) float xs[SUS_SPAN];
    __shared__ float red[SUS_NT / 64];
    const GsLoopNote nt = notes[blockIdx.y];
    // a bad table must not fault: the note is judged before an address is formed from it (block-uniform: the whole block leaves)
    if (nt.row < 0 || nt.row >= rows || nt.a < 0 || nt.m_min < 1 || nt.m_max < nt.m_min || nt.window < 1 || nt.window > SUS_MAX_W ||
        (long)nt.a + (long)nt.m_max + (long)nt.window > length || (long)nt.m_max - (long)nt.m_min + 1 > scores_stride) return;
    const long lag0 = (long)blockIdx.x * SUS_LAGS;       // the tile's first lag, relative to m_min
    if (lag0 > (long)nt.m_max - (long)nt.m_min) return;
    const int W = nt.window, W4 = W & ~3;
    const float* __restrict__ xr = waves + (size_t)nt.row * row_stride;
    const long base = (long)nt.a + (long)nt.m_min + lag0; // the source index of xs[0]: <= a + m_max < length

    float aa = 0.f;
    for (int i = threadIdx.x; i < ((W + 3) & ~3); i += SUS_NT) {   // a + i < a + W <= length; zeros round the window up to a float4
        const float v = i < W ? xr[nt.a + i] : 0.f;
        ws[i] = v;
        aa = fmaf(v, v, aa);
    }
    const int span = SUS_LAGS - 1 + W;                   // <= SUS_SPAN - 1
    for (int s = threadIdx.x; s < span; s += SUS_NT) {
        const long i = base + s;
        xs[s] = i < length ? xr[i] : 0.f;                // the zero fill: lags past m_max never see the stride padding or another row
    }
    const float s_aa = block_sum<SUS_NT>(aa, red);       // (its barriers also publish ws and xs)

    const float* __restrict__ xl = xs + threadIdx.x;     // xl[i] = x[a + m + i] for this lane's lag m
    float ab[4] = {0.f, 0.f, 0.f, 0.f}, bb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < W4; i += 4) {
        const float4 w = *reinterpret_cast<const float4*>(ws + i);
        const float s0 = xl[i], s1 = xl[i + 1], s2 = xl[i + 2], s3 = xl[i + 3];
        ab[0] = fmaf(w.x, s0, ab[0]); bb[0] = fmaf(s0, s0, bb[0]);
        ab[1] = fmaf(w.y, s1, ab[1]); bb[1] = fmaf(s1, s1, bb[1]);
        ab[2] = fmaf(w.z, s2, ab[2]); bb[2] = fmaf(s2, s2, bb[2]);
        ab[3] = fmaf(w.w, s3, ab[3]); bb[3] = fmaf(s3, s3, bb[3]);
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {                        // the last W mod 4 taps, into their own chains
        if (W4 + e < W) {
            const float s = xl[W4 + e];
            ab[e] = fmaf(ws[W4 + e], s, ab[e]);
            bb[e] = fmaf(s, s, bb[e]);
        }
    }
    const float s_ab = (ab[0] + ab[1]) + (ab[2] + ab[3]);
    const float s_bb = (bb[0] + bb[1]) + (bb[2] + bb[3]);
    const float prod = s_aa * s_bb;
    const long lag = lag0 + threadIdx.x;
    if (lag <= (long)nt.m_max - (long)nt.m_min)          // lag < scores_stride
        scores[(size_t)blockIdx.y * scores_stride + lag] = prod == 0.f ? 0.f : s_ab / sqrtf(prod);
}

// grid (tiles, jobs).  waves[dst_row][j] = y[offset + j] for the tile's j < count
__global__ __launch_bounds__(SUS_NT) void note_sustain_kernel(float* __restrict__ waves, int rows, long length, long row_stride,
                                                              const GsSustainJob* __restrict__ jobs) {
#pragma clang fp contract(off)
    const GsSustainJob jb = jobs[blockIdx.y];
    const long j0 = (long)blockIdx.x * SUS_TILE + (long)threadIdx.x * 4;
    // a bad table must not fault: the job is judged before an address is formed from it (block-uniform up to the tile's end)
    if (jb.src_row < 0 || jb.src_row >= rows || jb.dst_row < 0 || jb.dst_row >= rows || jb.src_row == jb.dst_row || jb.count < 1 ||
        (long)jb.count > length || jb.offset < 0 || jb.a < 0 || jb.m < 1 || jb.xfade < 0 ||
        (long)jb.a + (long)jb.m + (long)jb.xfade > length || j0 >= (long)jb.count) return;
    const float* __restrict__ x = waves + (size_t)jb.src_row * row_stride;
    float* __restrict__ out = waves + (size_t)jb.dst_row * row_stride;
    const long b = (long)jb.a + (long)jb.m, m = jb.m;
    const float inv = __fdiv_rn(1.f, (float)(jb.xfade + 1));
    long k = jb.offset + j0;                              // offset < 2^63 - length is the caller's; the Python layer stops at 2^62
    // p < m fits 32 bits and stays there: (float)(p + 1) is then one conversion.  As a 64-bit integer it is normalised by a 64-bit
    // shift whose amount hipcc put into the last VGPR of the wave's allocation (v15 of 16), and that shift now and then came back
    // with another amount on the MI355X -- w off by a power of two in one wave of some ten thousand (DESIGN.md "Sustain").
    int p = k >= b ? (int)((k - b) % m) : 0;              // (before b: p is 0 when k reaches b)
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e, ++k) {
        if (k < b) {                                      // 0 <= k < b <= length
            v[e] = x[k];
            continue;
        }
        const float xa = x[jb.a + p];                     // a + p < a + m = b <= length
        if (p < jb.xfade) {
            const float w = (float)(p + 1) * inv;
            v[e] = (1.f - w) * x[b + p] + w * xa;         // b + p < b + xfade <= length
        } else {
            v[e] = xa;
        }
        p = p + 1 == jb.m ? 0 : p + 1;                    // p + 1 <= m: no overflow
    }
    if (j0 + 4 <= (long)jb.count && (reinterpret_cast<uintptr_t>(out + j0) & 15) == 0) {
        st4(out + j0, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < (long)jb.count) out[j0 + e] = v[e];
    }
}

static int check_sustain(const char* name, const void* waves, int rows, int64_t length, int64_t row_stride, const void* table, int n,
                         unsigned table_align) {
    GS_CHECK_ARG(n > 0 && n <= 65535, "%s: the table must hold 1 to 65535 entries (got %d)", name, n);
    GS_CHECK_ARG(rows > 0, "%s: rows must be positive (got %d)", name, rows);
    GS_CHECK_ARG(length > 0 && length <= GS_SUSTAIN_MAX_LENGTH, "%s: length must be in [1, 2^30] (got %lld)", name, (long long)length);
    GS_CHECK_ARG(row_stride >= length, "%s: row_stride %lld is below length %lld", name, (long long)row_stride, (long long)length);
    GS_CHECK_ARG(waves != nullptr && table != nullptr, "%s: null pointer (waves and the table are required)", name);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(waves) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & (table_align - 1)) == 0,
                 "%s: misaligned pointer (waves: 4 bytes, the table: %u)", name, table_align);
    return 0;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_loop_search(const float* waves, int rows, int64_t length, int64_t row_stride, const GsLoopNote* notes, int n_notes,
                              float* scores, int64_t scores_stride, void* stream) {
    const char* name = "loop_search";
    const int code = check_sustain(name, waves, rows, length, row_stride, notes, n_notes, 4);
    if (code != 0) return code;
    GS_CHECK_ARG(scores_stride > 0 && scores_stride <= (1 << 24), "%s: scores_stride must be in [1, 2^24] (got %lld)", name,
                 (long long)scores_stride);
    GS_CHECK_ARG(scores != nullptr && (reinterpret_cast<uintptr_t>(scores) & 3) == 0, "%s: scores is null or off 4 bytes", name);
    const long tiles = ((long)scores_stride + SUS_LAGS - 1) / SUS_LAGS;
    hipLaunchKernelGGL(loop_search_kernel, dim3((unsigned)tiles, (unsigned)n_notes), dim3(SUS_NT), 0, as_stream(stream), waves, rows,
                       (long)length, (long)row_stride, notes, scores, (long)scores_stride);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_note_sustain(float* waves, int rows, int64_t length, int64_t row_stride, const GsSustainJob* jobs, int n_jobs, void* stream) {
    const char* name = "note_sustain";
    const int code = check_sustain(name, waves, rows, length, row_stride, jobs, n_jobs, 8);
    if (code != 0) return code;
    const long tiles = ((long)length + SUS_TILE - 1) / SUS_TILE;
    hipLaunchKernelGGL(note_sustain_kernel, dim3((unsigned)tiles, (unsigned)n_jobs), dim3(SUS_NT), 0, as_stream(stream), waves, rows,
                       (long)length, (long)row_stride, jobs);
    GS_CHECK_LAUNCH();
    return 0;
}
