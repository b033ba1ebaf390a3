// Output rates: the rational-ratio, Kaiser-windowed-sinc resampler behind GANSynth.synthesize / generate(sample_rate=...) and
// spectral_ops.resample (the rule is this project's own and is stated in include/gansynth_hip.h and DESIGN.md "Output rates").
//
// Host: the design (gcd, up, down, taps) and the coefficient table, in double, rounded once to fp32.
// Device, two launches like gs_note_mix.  `resample_kernel`: a 256-lane block owns RS_TILE consecutive outputs of one row.  Their input
// indices floor(j * down / up) - taps/2 + 1 + k cover one contiguous span of at most (RS_TILE - 1) * down / up + 1 + taps samples, which
// the block stages in LDS once -- the zero fill beyond the row's two ends happens there, so the inner loop has no bounds test and never
// sees the stride padding or a neighbouring row.  The 64-bit part of the index arithmetic is done once per block (q0, r0 of the tile's
// first output); a lane's own offset and phase follow from r0 + l * down in 32 bits.  A lane reads its tap row from the table (rows
// padded to 16 bytes: GS_RESAMPLE_ROW) as float4, the samples from LDS, and sums into four chains by k mod 4, folded at the end -- a
// fixed order, so two calls agree bit for bit.  One |max| per block goes to the workspace.
// The finish of clip_finish.hip, one clip a row: every block folds its row's block maxima (a maximum is exact), then scales and quantises
// its own tile.
#include <math.h>

#include "clip_finish.h"
#include "gs_common.h"

namespace gs {

constexpr int RS_NT = 256;        // threads per block
constexpr int RS_PER_LANE = 2;    // outputs per lane of the filter (RS_NT apart: the stores of a wave stay contiguous)
constexpr int RS_TILE = RS_NT * RS_PER_LANE;
static_assert(RS_TILE == GS_RESAMPLE_TILE, "include/gansynth_hip.h states the tile");

static inline long rs_tiles(long n_out) { return (n_out + RS_TILE - 1) / RS_TILE; }
static inline int rs_row(int taps) { return GS_RESAMPLE_ROW(taps); }
// the largest span of input samples a tile needs: its last output starts at most ((up - 1) + (RS_TILE - 1) * down) / up behind its first
static inline long rs_span(int up, int down, int taps) { return ((long)(up - 1) + (long)(RS_TILE - 1) * down) / up + taps; }

// grid (tiles, rows), dynamic LDS: rs_span floats.  out[row][j] = y[j]; block_max[row * tiles + tile] = max |y[j]| over the tile
__global__ __launch_bounds__(RS_NT) void resample_kernel(const float* __restrict__ x, long n_in, long row_stride, const float* __restrict__ table,
                                                         int up, int down, int taps, long n_out, int tiles, float* __restrict__ out,
                                                         float* __restrict__ block_max) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int row = blockIdx.y;
    const long j0 = (long)blockIdx.x * RS_TILE;
    const long jd = j0 * down;                       // (block-uniform; < 2^63: the entry point bounds n_in * up)
    const long q0 = jd / up;
    const unsigned r0 = (unsigned)(jd - q0 * up);
    const long base = q0 - taps / 2 + 1;             // the input index of xs[0]; negative at the row's head
    const int span = (int)((r0 + (unsigned)(RS_TILE - 1) * (unsigned)down) / (unsigned)up) + taps;   // <= rs_span(up, down, taps)
    const float* __restrict__ xr = x + (size_t)row * row_stride;
    for (int s = threadIdx.x; s < span; s += RS_NT) {
        const long i = base + s;
        xs[s] = (i >= 0 && i < n_in) ? xr[i] : 0.f;
    }
    __syncthreads();

    const int tp = GS_RESAMPLE_ROW(taps);
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < RS_PER_LANE; ++u) {
        const int l = u * RS_NT + threadIdx.x;
        const long j = j0 + l;
        if (j >= n_out) continue;
        const unsigned a = r0 + (unsigned)l * (unsigned)down;      // (j * down) - q0 * up: below 2^32 (down <= 16 * up <= 2^14)
        const unsigned off = a / (unsigned)up, p = a - off * (unsigned)up;
        const float4* __restrict__ c4 = reinterpret_cast<const float4*>(table + (size_t)p * tp);
        const float* xl = xs + off;                                // xl[k] = x[i0 - taps/2 + 1 + k]; off + taps <= span
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int k = 0;
        for (; k + 4 <= taps; k += 4) {
            const float4 c = c4[k >> 2];
            acc[0] = fmaf(c.x, xl[k], acc[0]);
            acc[1] = fmaf(c.y, xl[k + 1], acc[1]);
            acc[2] = fmaf(c.z, xl[k + 2], acc[2]);
            acc[3] = fmaf(c.w, xl[k + 3], acc[3]);
        }
        if (k < taps) {   // taps is even: two left (the row's padding is not multiplied: a sample there may be anything)
            const float4 c = c4[k >> 2];
            acc[0] = fmaf(c.x, xl[k], acc[0]);
            acc[1] = fmaf(c.y, xl[k + 1], acc[1]);
        }
        const float y = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        out[(size_t)row * n_out + j] = y;
        m = fmaxf(m, fabsf(y));
    }
    publish_block_max<RS_NT>(m, block_max + (size_t)row * tiles + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------- host: the design
static long rs_gcd(long a, long b) {
    while (b != 0) { const long t = a % b; a = b; b = t; }
    return a;
}

// the design of (rate_in, rate_out), or a refusal with its message
static int rs_design(int rate_in, int rate_out, GsResample* d) {
    GS_CHECK_ARG(rate_in > 0 && rate_out > 0, "resample: rates must be positive (got %d -> %d)", rate_in, rate_out);
    GS_CHECK_ARG(rate_in != rate_out, "resample: equal rates (%d): nothing to convert", rate_in);
    const long g = rs_gcd(rate_in, rate_out);
    const long up = rate_out / g, down = rate_in / g;
    GS_CHECK_ARG(up <= GS_RESAMPLE_MAX_UP, "resample: %d -> %d needs up = %ld phases, more than %d", rate_in, rate_out, up, GS_RESAMPLE_MAX_UP);
    const double c = GS_RESAMPLE_ROLLOFF * (up < down ? (double)up / (double)down : 1.0);
    const double half = ceil((double)GS_RESAMPLE_ZEROS / c);
    GS_CHECK_ARG(2.0 * half <= (double)GS_RESAMPLE_MAX_TAPS, "resample: %d -> %d needs taps = %.0f, more than %d", rate_in, rate_out, 2.0 * half,
                 GS_RESAMPLE_MAX_TAPS);
    d->rate_in = rate_in; d->rate_out = rate_out;
    d->up = (int32_t)up; d->down = (int32_t)down;
    d->taps = 2 * (int32_t)half; d->zeros = GS_RESAMPLE_ZEROS;
    return 0;
}

// a caller's descriptor is what rs_design gives for its rates
static int rs_check(const GsResample* r) {
    GS_CHECK_ARG(r != nullptr, "resample: null descriptor");
    GsResample d;
    const int code = rs_design(r->rate_in, r->rate_out, &d);
    if (code != 0) return code;
    GS_CHECK_ARG(r->up == d.up && r->down == d.down && r->taps == d.taps && r->zeros == d.zeros,
                 "resample: descriptor (up %d, down %d, taps %d, zeros %d) does not follow from its rates %d -> %d (up %d, down %d, taps %d, zeros %d)",
                 r->up, r->down, r->taps, r->zeros, r->rate_in, r->rate_out, d.up, d.down, d.taps, d.zeros);
    return 0;
}

// I0 by its power series sum ((x/2)^2k / (k!)^2): every term positive, converged to the last bit of the double sum
static double rs_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

static double rs_h(double u, double c) {
    const double pi = 3.14159265358979323846;
    const double a = c * u / (double)GS_RESAMPLE_ZEROS;
    if (!(fabs(a) < 1.0)) return 0.0;
    const double t = pi * c * u;
    const double sinc = t == 0.0 ? 1.0 : sin(t) / t;
    return c * sinc * rs_i0(GS_RESAMPLE_BETA * sqrt(1.0 - a * a)) / rs_i0(GS_RESAMPLE_BETA);
}

}  // namespace gs

using namespace gs;

extern "C" int gs_resample_design(int rate_in, int rate_out, GsResample* out) {
    GS_CHECK_ARG(out != nullptr, "resample_design: null descriptor");
    return rs_design(rate_in, rate_out, out);
}

extern "C" int64_t gs_resample_out_len(const GsResample* r, int64_t n_in) {
    const int code = rs_check(r);
    if (code != 0) return code;
    GS_CHECK_ARG(n_in > 0 && n_in <= GS_RESAMPLE_MAX_N, "resample: n_in must be in [1, 2^40] (got %lld)", (long long)n_in);
    return (n_in * r->up + r->down - 1) / r->down;
}

extern "C" size_t gs_resample_table_bytes(const GsResample* r, int device_layout) {
    if (rs_check(r) != 0) return 0;
    return (size_t)r->up * (size_t)(device_layout ? rs_row(r->taps) : r->taps) * sizeof(float);
}

extern "C" int gs_resample_table(const GsResample* r, int device_layout, float* table_host) {
    const int code = rs_check(r);
    if (code != 0) return code;
    GS_CHECK_ARG(table_host != nullptr, "resample_table: null table");
    const int taps = r->taps, stride = device_layout ? rs_row(taps) : taps;
    const double c = GS_RESAMPLE_ROLLOFF * (r->up < r->down ? (double)r->up / (double)r->down : 1.0);
    for (int p = 0; p < r->up; ++p) {
        float* t = table_host + (size_t)p * stride;
        for (int k = 0; k < taps; ++k) t[k] = (float)rs_h((double)p / (double)r->up + (double)(taps / 2 - 1 - k), c);
        for (int k = taps; k < stride; ++k) t[k] = 0.f;
    }
    return 0;
}

extern "C" size_t gs_resample_workspace_bytes(const GsResample* r, int rows, int64_t n_in) {
    if (rows <= 0) { fail(GS_ERR_ARG, "resample: rows must be positive (got %d)", rows); return 0; }
    const int64_t n_out = gs_resample_out_len(r, n_in);
    if (n_out <= 0) return 0;
    return (size_t)rows * (size_t)rs_tiles((long)n_out) * sizeof(float);
}

extern "C" int gs_resample(const GsResample* r, const float* table_dev, const float* x, int rows, int64_t n_in, int64_t row_stride, int normalize,
                           float* out, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream) {
    const int code = rs_check(r);
    if (code != 0) return code;
    GS_CHECK_ARG(rows > 0 && rows <= 65535, "resample: rows must be in [1, 65535] (got %d)", rows);
    GS_CHECK_ARG(n_in > 0 && n_in <= GS_RESAMPLE_MAX_N, "resample: n_in must be in [1, 2^40] (got %lld)", (long long)n_in);
    GS_CHECK_ARG(row_stride >= n_in, "resample: row_stride %lld is below n_in %lld", (long long)row_stride, (long long)n_in);
    GS_CHECK_ARG(x && out && table_dev, "resample: null pointer (x, out and table are required)");
    const long n_out = (long)((n_in * r->up + r->down - 1) / r->down);
    const long tiles = rs_tiles(n_out);
    GS_CHECK_ARG(tiles <= 0x7fffffffL, "resample: row too long (n_out %ld)", n_out);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(table_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(pcm) & 1) == 0 &&
                 (reinterpret_cast<uintptr_t>(peak) & 3) == 0, "resample: misaligned pointer (table: 16 bytes, x / out / peak: 4, pcm: 2)");
    const size_t need = (size_t)rows * (size_t)tiles * sizeof(float);
    GS_CHECK_ARG(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "resample: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    float* block_max = static_cast<float*>(ws);
    const size_t lds = (size_t)rs_span(r->up, r->down, r->taps) * sizeof(float);   // <= 36 KB at the largest supported ratio
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(RS_NT), lds, st, x, (long)n_in, (long)row_stride, table_dev,
                       (int)r->up, (int)r->down, (int)r->taps, n_out, (int)tiles, out, block_max);
    if (normalize != 0 || pcm != nullptr || peak != nullptr)
        launch_clip_finish(out, 1, rows, n_out, n_out, reinterpret_cast<short*>(pcm), peak, block_max, (int)tiles, normalize, st);
    GS_CHECK_LAUNCH();
    return 0;
}
