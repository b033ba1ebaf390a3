// Pitch bend: the per-note time-warp resampler ahead of the mix (GANSynth.synthesize with bend; the rule is this project's own and is
// stated in include/gansynth_hip.h and DESIGN.md "Pitch bend").
//
// Host: the coefficient table (a Kaiser-windowed sinc sampled WARP_Q times per zero crossing), in double, rounded once to fp32.
// Device, one launch: a 256-lane block owns WARP_TILE consecutive outputs of one bent note (grid: tiles x notes).  The block evaluates
// the read position of its first and of its last output once (float64, block-uniform), stages the table (32 KB) and the span of the
// source row between them -- widened by the longest filter on either side, zero-filled beyond the row's two ends -- in LDS, and every
// lane then evaluates its own outputs: the curve's segment by a binary search between the tile's first and last segment (found once per
// block, in global memory: a curve may have any number of points inside a tile), the position in float64, and from `f` and `c` on fp32:
// an interpolated table read and one FMA per tap, summed into four chains by tap index mod 4 and folded at the end -- a fixed order, no
// atomics, so two calls agree bit for bit.  The tap loop has no bounds test: a lane's offset into the staged span is clamped to the span.
#include <math.h>

#include "gs_common.h"

namespace gs {

constexpr int WARP_NT = 256;                            // threads per block
constexpr int WARP_PER_LANE = 4;                        // outputs per lane (WARP_NT apart: the stores of a wave stay contiguous)
constexpr int WARP_TILE = WARP_NT * WARP_PER_LANE;
constexpr int WARP_Z = GS_WARP_ZEROS, WARP_Q = GS_WARP_Q;
constexpr int WARP_ZQ = WARP_Z * WARP_Q;                // the table's last index
constexpr int WARP_HALF = WARP_Z * 4;                   // taps on either side at the lowest cutoff (ratio 4): 128
constexpr int WARP_SPAN = WARP_TILE * 4 + 2 * WARP_HALF + 4;   // staged samples: xs[s] = x[n_first - WARP_HALF + s]
constexpr int WARP_TABLE = GS_WARP_TABLE_FLOATS;        // T[0 .. ZQ], the zero that follows, padding to 16 bytes
static_assert(WARP_TILE == GS_WARP_TILE, "include/gansynth_hip.h states the tile");
static_assert(WARP_TABLE >= WARP_ZQ + 2 && WARP_TABLE % 4 == 0, "the table, its trailing zero, whole float4s");
static_assert(sizeof(GsWarpNote) == 24, "GsWarpNote is 24 bytes (gansynth_amd/_lib.py mirrors it)");
static_assert(sizeof(GsWarpPoint) == 24, "GsWarpPoint is 24 bytes (gansynth_amd/_lib.py mirrors it)");

// first index in [lo, hi) whose pos is > t (hi when there is none); every index read lies in [lo, hi), whatever the positions hold
__device__ inline int warp_first_after(const GsWarpPoint* __restrict__ points, int lo, int hi, double t) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (points[mid].pos <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ inline double warp_ratio(double r) { return fmin(fmax(r, 0.25), 4.0); }   // (NaN: 0.25)

// Phi(t) and the ratio at t over the curve points[lo, hi) (0 <= lo < hi <= n_points); k = the first index of [lo, hi] whose pos is > t.
// Every operation rounded on its own, in the order of the header (no FMA).
__device__ inline void warp_phi(const GsWarpPoint* __restrict__ points, int lo, int hi, int k, double t, double* phi, double* ratio) {
#pragma clang fp contract(off)
    const int i0 = k - 1 < lo ? lo : k - 1;              // in [lo, hi): before the first point the first one, extended flat
    const int i1 = k < hi ? k : hi - 1;                   // in [lo, hi)
    const GsWarpPoint a = points[i0], b = points[i1];
    const double ra = warp_ratio(a.ratio), rb = warp_ratio(b.ratio);
    const double d = t - a.pos, dp = b.pos - a.pos;
    if (i0 == i1 || k - 1 < lo || !(dp > 0.0)) {          // outside the points, or a segment of length <= 0: constant, nothing divided
        *phi = a.cum + ra * d;
        *ratio = ra;
    } else {
        const double dr = rb - ra;
        *phi = a.cum + ra * d + dr * d * d / (2.0 * dp);
        *ratio = ra + dr * d / dp;
    }
}

// grid (tiles, notes).  waves[dst_row][k] = bent[k] for the tile's k < count
__global__ __launch_bounds__(WARP_NT) void note_warp_kernel(float* __restrict__ waves, int rows, long length, long row_stride,
                                                            const GsWarpNote* __restrict__ notes, const GsWarpPoint* __restrict__ points,
                                                            const int* __restrict__ first_point, int n_curves, int n_points,
                                                            const float* __restrict__ table) {
    __shared__ __attribute__((aligned(16))) float ts[WARP_TABLE];
    __shared__ __attribute__((aligned(16))) float xs[WARP_SPAN];
    const GsWarpNote nt = notes[blockIdx.y];
    const long k0 = (long)blockIdx.x * WARP_TILE;
    // a bad table must not fault: the note is judged before an address is formed from it (block-uniform: the whole block leaves)
    if (nt.src_row < 0 || nt.src_row >= rows || nt.dst_row < 0 || nt.dst_row >= rows || nt.src_row == nt.dst_row || nt.count < 1 ||
        (long)nt.count > length || nt.onset < 0 || nt.curve < 0 || nt.curve >= n_curves || k0 >= (long)nt.count) return;
    const long k1 = k0 + WARP_TILE < (long)nt.count ? k0 + WARP_TILE : (long)nt.count;    // the tile's outputs: [k0, k1)
    int lo = first_point[nt.curve], hi = first_point[nt.curve + 1];                        // 0 <= curve < n_curves: first has n_curves + 1 entries
    lo = lo < 0 ? 0 : (lo > n_points - 1 ? n_points - 1 : lo);                              // clamped: 0 <= lo < hi <= n_points, whatever the table says
    hi = hi > n_points ? n_points : hi;
    hi = hi < lo + 1 ? lo + 1 : hi;

    // block-uniform, float64: Phi at the onset, the tile's segment range [s0, s1], the positions of its first and last output
    const double q_max = (double)(length + WARP_HALF);   // from there on every tap of every cutoff reads the zero fill
    const double t_on = (double)nt.onset;
    double phi_on, phi, r_unused;
    warp_phi(points, lo, hi, warp_first_after(points, lo, hi, t_on), t_on, &phi_on, &r_unused);
    const int s0 = warp_first_after(points, lo, hi, (double)(nt.onset + k0));
    const int s1 = warp_first_after(points, s0, hi, (double)(nt.onset + k1 - 1));
    warp_phi(points, lo, hi, s0, (double)(nt.onset + k0), &phi, &r_unused);
    const long n_first = (long)floor(fmin(fmax(phi - phi_on, 0.0), q_max));                 // (NaN: 0)
    warp_phi(points, lo, hi, s1, (double)(nt.onset + k1 - 1), &phi, &r_unused);
    const long n_last = (long)floor(fmin(fmax(phi - phi_on, 0.0), q_max));
    long rel_max = n_last - n_first;                      // a curve as the header asks for it: 0 <= rel_max <= 4 * (WARP_TILE - 1) + 1
    rel_max = rel_max < 0 ? 0 : (rel_max > 4L * WARP_TILE ? 4L * WARP_TILE : rel_max);
    const int span = (int)rel_max + 2 * WARP_HALF + 1;    // <= WARP_SPAN; a lane reads xs[rel + 1 .. rel + 2 * WARP_HALF], rel <= rel_max

    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(table);
    for (int s = threadIdx.x; s < WARP_TABLE / 4; s += WARP_NT) reinterpret_cast<float4*>(ts)[s] = t4[s];
    const float* __restrict__ xr = waves + (size_t)nt.src_row * row_stride;
    const long base = n_first - WARP_HALF;                // the source index of xs[0]; negative at the row's head
    for (int s = threadIdx.x; s < span; s += WARP_NT) {
        const long i = base + s;
        xs[s] = (i >= 0 && i < length) ? xr[i] : 0.f;     // the zero fill: the tap loop never sees the stride padding or another row
    }
    __syncthreads();

    float* __restrict__ out = waves + (size_t)nt.dst_row * row_stride;
#pragma unroll 1
    for (int u = 0; u < WARP_PER_LANE; ++u) {
        const long k = k0 + u * WARP_NT + threadIdx.x;
        if (k >= k1) continue;
        const double t = (double)(nt.onset + k);
        double r;
        warp_phi(points, lo, hi, warp_first_after(points, s0, s1, t), t, &phi, &r);
        const double q = fmin(fmax(phi - phi_on, 0.0), q_max);
        const double nq = floor(q);
        const float f = (float)(q - nq);
        const float c = (float)fmin(1.0, 1.0 / r);        // r in [0.25, 4]: c in [0.25, 1]
        long rel = (long)nq - n_first;
        rel = rel < 0 ? 0 : (rel > rel_max ? rel_max : rel);   // (no change for a curve as the header asks for it)
        // taps j = i - n in [-w + 1, w], w = ceil(Z / c) <= WARP_HALF: every tap of |c (j - f)| < Z, and beyond it exact zeros
        int w = (int)ceilf((float)WARP_Z / c);
        w = w > WARP_HALF ? WARP_HALF : ((w + 1) & ~1);   // even, so that the window is whole groups of four taps
        const float* xl = xs + rel + WARP_HALF;           // xl[j] = x[n + j]
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = -w + 1; j <= w; j += 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = fminf(c * fabsf((float)(j + e) - f) * (float)WARP_Q, (float)WARP_ZQ);
                const int m = (int)a;                      // 0 .. ZQ; ts[ZQ + 1] is the zero that follows the table
                const float fr = a - (float)m;
                const float t0 = ts[m], t1 = ts[m + 1];
                const float h = c * (t0 + fr * (t1 - t0));
                acc[e] = fmaf(h, xl[j + e], acc[e]);
            }
        }
        out[k] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
}

// I0 by its power series sum ((x/2)^2k / (k!)^2): every term positive, converged to the last bit of the double sum
static double warp_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_note_warp_table_bytes(void) { return (size_t)WARP_TABLE * sizeof(float); }

extern "C" int gs_note_warp_table(float* table_host) {
    GS_CHECK_ARG(table_host != nullptr, "note_warp_table: null table");
    const double pi = 3.14159265358979323846;
    const double i0b = warp_i0(GS_WARP_BETA);
    for (int m = 0; m <= WARP_ZQ; ++m) {
        if (m % WARP_Q == 0) {                             // exact: 1 at the centre, 0 at the sinc's zero crossings
            table_host[m] = m == 0 ? 1.f : 0.f;
            continue;
        }
        const double x = (double)m / (double)WARP_Q, a = (double)m / (double)WARP_ZQ;
        table_host[m] = (float)(sin(pi * x) / (pi * x) * warp_i0(GS_WARP_BETA * sqrt(1.0 - a * a)) / i0b);
    }
    for (int m = WARP_ZQ + 1; m < WARP_TABLE; ++m) table_host[m] = 0.f;
    return 0;
}

extern "C" int gs_note_warp(float* waves, int rows, int64_t length, int64_t row_stride, const GsWarpNote* notes, int n_notes,
                            const GsWarpPoint* points, const int32_t* first, int n_curves, int n_points, const float* table_dev, void* stream) {
    const char* name = "note_warp";
    GS_CHECK_ARG(n_notes > 0 && n_notes <= 65535, "%s: n_notes must be in [1, 65535] (got %d)", name, n_notes);
    GS_CHECK_ARG(rows > 0, "%s: rows must be positive (got %d)", name, rows);
    GS_CHECK_ARG(length > 0 && length <= GS_WARP_MAX_LENGTH, "%s: length must be in [1, 2^30] (got %lld)", name, (long long)length);
    GS_CHECK_ARG(row_stride >= length, "%s: row_stride %lld is below length %lld", name, (long long)row_stride, (long long)length);
    GS_CHECK_ARG(n_curves > 0, "%s: n_curves must be positive (got %d)", name, n_curves);
    GS_CHECK_ARG(n_points > 0, "%s: n_points must be positive (got %d)", name, n_points);
    GS_CHECK_ARG(waves && notes && points && first && table_dev, "%s: null pointer (waves, notes, points, first and table are required)", name);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(waves) & 3) == 0 && (reinterpret_cast<uintptr_t>(notes) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(points) & 7) == 0 && (reinterpret_cast<uintptr_t>(first) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(table_dev) & 15) == 0,
                 "%s: misaligned pointer (table: 16 bytes, notes / points: 8, waves / first: 4)", name);
    const long tiles = ((long)length + WARP_TILE - 1) / WARP_TILE;
    hipLaunchKernelGGL(note_warp_kernel, dim3((unsigned)tiles, (unsigned)n_notes), dim3(WARP_NT), 0, as_stream(stream), waves, rows, (long)length,
                       (long)row_stride, notes, points, first, n_curves, n_points, table_dev);
    GS_CHECK_LAUNCH();
    return 0;
}
