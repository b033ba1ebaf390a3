// True peak: the 4x oversampled peak detector of a rendered clip (gansynth_amd/true_peak.py, kernels.true_peak; the rule is this project's own
// and is stated in include/gansynth_hip.h and DESIGN.md "True peak").  e[t] = max over the rows of max(|x[t]|, |z[4t]| .. |z[4t + 3]|) with z
// what gs_resample would write for the design 1 -> 4 (68 taps a phase) -- but the 4x signal never leaves the registers.
//
// 272 FMAs per sample and row against 4 bytes read: the fp32 vector pipe binds, so the kernel is built around the FMA's operands.
//   * A block owns TP_TILE = 2048 consecutive samples of ALL rows and stages them with the halo (33 before, 34 after; 0 outside [0, n)) in
//     LDS once: the inner loop has no bounds test.
//   * A lane owns TP_S = 8 consecutive samples x 4 phases = 32 accumulators, each ONE chain over k ascending (a fixed order: two calls agree
//     bit for bit; the independent chains hide the FMA's latency).  Two phases of a sample share a register pair and one v_pk_fma_f32: the
//     coefficient pair comes from a scalar register pair, the sample is taken on both halves (op_sel) -- 1088 packed FMAs a lane and row.
//   * The taps run in 17 chunks of 4.  A chunk needs the 11 samples x[t0 - 33 + 4c .. + 10] of its lane: a window of registers that slides by
//     ONE 16-byte LDS read a chunk (19 ds_read_b128 per lane and row for 2176 FMAs).  Lane l reads at 32 l bytes: the 16 lanes of a
//     ds_read_b128 group cover 128 dwords, two to a bank -- 2-way, 8 LDS cycles an instruction, 152 a wave and row against 4352 VALU cycles.
//   * The 16 coefficients of a chunk, T[0..3][4c .. 4c + 3], are wave-uniform: read through the constant path into scalar registers (four
//     16-byte loads from a __restrict__ const pointer at uniform addresses, paired by s_mov), and an FMA takes its coefficients from there.
//     No lane loads one.
//   * The chunk loop is a real loop (window and coefficients are read one chunk ahead): see the note at the loop.
//   true_peak_kernel<ROWS>   grid (tiles): stage, filter, env (16 bytes a lane where env is 16-byte aligned), one |max| of e a block
//   true_peak_fold_kernel    grid (1): the fold of those slots (maxima of values that are never NaN: exact in any order)
#include <math.h>

#include "clip_finish.h"
#include "gs_common.h"

namespace gs {

constexpr int TP_NT = 256;                         // threads per block
constexpr int TP_S = 8;                            // consecutive samples a lane owns
constexpr int TP_TILE = TP_NT * TP_S;              // samples a block owns
constexpr int TP_TAPS = GS_TRUE_PEAK_TAPS;
constexpr int TP_UP = GS_TRUE_PEAK_OVERSAMPLE;
constexpr int TP_ROW = GS_RESAMPLE_ROW(TP_TAPS);   // floats per row of the device table
constexpr int TP_BEFORE = TP_TAPS / 2 - 1;         // 33: the halo before the tile (34 after)
constexpr int TP_CHUNKS = TP_TAPS / 4;
constexpr int TP_SPAN = TP_TILE + TP_TAPS;         // floats of a row in LDS: TP_TILE + 67 are read as samples, one more by the last 16-byte read
static_assert(TP_TILE == GS_TRUE_PEAK_TILE && TP_TAPS % 4 == 0 && TP_ROW == TP_TAPS && TP_UP == 4 && TP_S % 4 == 0, "the kernel is written for this design");

typedef float f32x2 __attribute__((ext_vector_type(2)));

static inline long tp_tiles(long n) { return (n + TP_TILE - 1) / TP_TILE; }

// grid (tiles of n).  env[t] = e[t] for the tile's t < n (env may be null); block_max[b] = max of e over them
template <int ROWS>
__global__ __launch_bounds__(TP_NT) void true_peak_kernel(const float* __restrict__ table, const float* __restrict__ x, long n, long row_stride,
                                                          float* __restrict__ env, float* __restrict__ block_max) {
    __shared__ __attribute__((aligned(16))) float xs[ROWS][TP_SPAN];   // xs[r][j] = x[r][tile_begin - 33 + j], 0 outside [0, n)
    const long tile_begin = (long)blockIdx.x * TP_TILE;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const float* __restrict__ xr = x + (size_t)r * row_stride;
        for (int j = threadIdx.x; j < TP_SPAN; j += TP_NT) {
            const long t = tile_begin - TP_BEFORE + j;
            xs[r][j] = (t >= 0 && t < n) ? xr[t] : 0.f;
        }
    }
    __syncthreads();

    float e[TP_S];
#pragma unroll
    for (int s = 0; s < TP_S; ++s) e[s] = 0.f;
#pragma unroll 1
    for (int r = 0; r < ROWS; ++r) {
        const float* xl = xs[r] + threadIdx.x * TP_S;   // xl[i] = x[t0 - 33 + i] for the lane's first sample t0; 32-byte aligned
        f32x2 acc[TP_S][TP_UP / 2];                     // acc[s][q]: the phases 2q and 2q + 1 of sample s, one register pair
#pragma unroll
        for (int s = 0; s < TP_S; ++s)
#pragma unroll
            for (int q = 0; q < TP_UP / 2; ++q) acc[s][q] = f32x2{0.f, 0.f};
        float win[TP_S + 4];                            // in chunk c: win[i] = xl[4c + i]
#pragma unroll
        for (int i = 0; i < TP_S; i += 4) ld4(xl + i, *reinterpret_cast<float(*)[4]>(win + i));
#pragma unroll
        for (int s = 0; s < TP_S; ++s) e[s] = fmaxf(e[s], fabsf(xl[TP_BEFORE + s]));                        // |x[t0 + s]|
        float nxt[4], co[TP_UP][4];                     // the window's next four samples and T[p][4c + kk] (uniform), read a chunk ahead
        ld4(xl + TP_S, nxt);
#pragma unroll
        for (int p = 0; p < TP_UP; ++p) ld4(table + p * TP_ROW, co[p]);
        // the chunk loop is NOT unrolled: unrolled, the scheduler lines up each accumulator's whole 68-tap chain back to back, every FMA waits
        // for the one before it, and the kernel runs at a third of the FMA rate (measured).  A loop body keeps the 16 accumulators interleaved.
#pragma unroll 1
        for (int c = 0; c < TP_CHUNKS; ++c) {
#pragma unroll
            for (int i = 0; i < 4; ++i) win[TP_S + i] = nxt[i];
            const int cn = c + 1 < TP_CHUNKS ? c + 1 : c;   // (the last chunk reads its own again: in bounds, not used)
            float con[TP_UP][4];
            ld4(xl + 4 * cn + TP_S, nxt);
#pragma unroll
            for (int p = 0; p < TP_UP; ++p) ld4(table + p * TP_ROW + 4 * cn, con[p]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int s = 0; s < TP_S; ++s)
#pragma unroll
                    for (int q = 0; q < TP_UP / 2; ++q)   // x[t0 + s - 33 + k], k = 4c + kk: one v_pk_fma_f32, the sample on both halves
                        acc[s][q] = __builtin_elementwise_fma(f32x2{co[2 * q][kk], co[2 * q + 1][kk]}, f32x2{win[s + kk], win[s + kk]}, acc[s][q]);
#pragma unroll
            for (int i = 0; i < TP_S; ++i) win[i] = win[i + 4];
#pragma unroll
            for (int p = 0; p < TP_UP; ++p)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) co[p][kk] = con[p][kk];
        }
#pragma unroll
        for (int s = 0; s < TP_S; ++s)
#pragma unroll
            for (int q = 0; q < TP_UP / 2; ++q) e[s] = fmaxf(fmaxf(e[s], fabsf(acc[s][q].x)), fabsf(acc[s][q].y));
    }

    const long t0 = tile_begin + (long)threadIdx.x * TP_S;
    float m = 0.f;
#pragma unroll
    for (int s = 0; s < TP_S; ++s)
        if (t0 + s < n) m = fmaxf(m, e[s]);            // (a sample from n on is no part of the clip: the filter's tail there is not measured)
    if (env != nullptr) {
        if ((reinterpret_cast<uintptr_t>(env) & 15) == 0 && t0 + TP_S <= n) {
#pragma unroll
            for (int s = 0; s < TP_S; s += 4) st4(env + t0 + s, *reinterpret_cast<const float(*)[4]>(e + s));
        } else {
#pragma unroll
            for (int s = 0; s < TP_S; ++s)
                if (t0 + s < n) env[t0 + s] = e[s];
        }
    }
    publish_block_max<TP_NT>(m, block_max + blockIdx.x);
}

// grid (1).  peak = max of block_max[0 .. tiles)
__global__ __launch_bounds__(TP_NT) void true_peak_fold_kernel(const float* __restrict__ block_max, int tiles, float* __restrict__ peak) {
    float mx = 0.f;
    for (int s = threadIdx.x; s < tiles; s += TP_NT) mx = fmaxf(mx, block_max[s]);
    mx = block_max_of<TP_NT>(mx);
    if (threadIdx.x == 0) *peak = mx;
}

static bool tp_shape_ok(int rows, int64_t n) { return (rows == 1 || rows == 2) && n > 0 && n <= GS_TRUE_PEAK_MAX_N; }
static size_t tp_ws_bytes(int64_t n) { return ((size_t)tp_tiles((long)n) * sizeof(float) + 15) & ~(size_t)15; }

}  // namespace gs

using namespace gs;

extern "C" size_t gs_true_peak_workspace_bytes(int rows, int64_t n) {
    if (!tp_shape_ok(rows, n)) return 0;
    return tp_ws_bytes(n);
}

extern "C" int gs_true_peak(const float* table_dev, const float* x, int rows, int64_t n, int64_t row_stride, float* env, float* peak, void* ws,
                            size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(rows == 1 || rows == 2, "true_peak: rows must be 1 or 2 (got %d)", rows);
    GS_CHECK_ARG(n > 0 && n <= GS_TRUE_PEAK_MAX_N, "true_peak: n must be in [1, 2^40] (got %lld)", (long long)n);
    GS_CHECK_ARG(row_stride >= n, "true_peak: row_stride %lld is below n %lld", (long long)row_stride, (long long)n);
    GS_CHECK_ARG(table_dev && x, "true_peak: null pointer (table and x are required)");
    GS_CHECK_ARG(env || peak, "true_peak: null pointer (env and peak cannot both be left out)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(table_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(env) & 3) == 0 && (reinterpret_cast<uintptr_t>(peak) & 3) == 0,
                 "true_peak: misaligned pointer (table: 16 bytes, x / env / peak: 4)");
    const size_t need = tp_ws_bytes(n);
    GS_CHECK_ARG(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "true_peak: workspace too small or misaligned (%zu bytes, need %zu)",
                 ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int tiles = (int)tp_tiles((long)n);
    float* block_max = static_cast<float*>(ws);
    with_constant<1, 2>(rows, [&](auto rows_c) {
        hipLaunchKernelGGL((true_peak_kernel<decltype(rows_c)::value>), dim3((unsigned)tiles), dim3(TP_NT), 0, st, table_dev, x, (long)n, (long)row_stride, env,
                           block_max);
        return true;
    });
    if (peak != nullptr) hipLaunchKernelGGL(true_peak_fold_kernel, dim3(1), dim3(TP_NT), 0, st, static_cast<const float*>(block_max), tiles, peak);
    GS_CHECK_LAUNCH();
    return 0;
}
