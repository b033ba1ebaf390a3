// BS.1770 K-weighted hop energies: the meter of a rendered clip (gansynth_amd/loudness.py, kernels.loudness_energy; the rule is stated in
// include/gansynth_hip.h and DESIGN.md "Loudness").  K-weighting is two biquads in cascade -- a fourth-order recurrence with poles at
// radius 0.995 -- over the whole row; the exact recurrence is kept, no block restarts at rest from a halo.  It is linear: with s the four
// state numbers of the cascade (transposed direct form II) and A the 4x4 matrix one silent sample applies to them, k samples from the
// state s end in  A^k s + (their end from rest).  So a tile is a hop (one block, the hop's samples in LDS, its energy a block reduction),
// a lane owns `chunk` consecutive samples of it, and the states are carried as float64 sums of matrix powers:
//
//   loud_ends_kernel<CAP>    grid (hops, rows): every lane runs its chunk from rest; a block scan carries the ends across the lanes ->
//                            the hop's end from rest, Z[r][j]
//   loud_carry_kernel        grid (rows): the same scan over the hops, 256 at a time, with A^hop -> the state every hop starts in, S[r][j]
//   loud_energy_kernel<CAP>  grid (hops, rows): the ends from rest again, the scan seeded with S[r][j] -> the state every chunk starts in;
//                            every lane runs its chunk from it and sums the squares; the block's sum in a fixed tree -> energy[r][j]
//
// The scan (loud_scan) is Hillis-Steele over the 256 lanes: v[i] += P^(2^k) v[i - 2^k], k = 0 .. 7, with the eight powers of P = A^chunk
// (or A^hop) from the descriptor; a seed enters as P times itself added to lane 0.  Values only ever flow to higher lanes and later
// hops, so a NaN reaches nothing before it, and no lane reads another row.
// Everything after the fp32 load runs in float64: the filter, the carry, the squares and their sum -- one rounding to fp32, at the store.
// gfx950 issues v_fma_f64 at the fp32 rate, the kernel is bound by its dependent chain per sample and not by the register file, and the
// error against the float64 rule is then the final rounding (DESIGN.md "Loudness" has the figures).
// Loads: the hop's samples from its first 16-byte boundary on as 16-byte packs, whatever the row base and the hop's offset (the LDS
// image is shifted by the same 0 .. 3 floats, so a pack is one ds_write_b128), sample by sample before that boundary and at the tail.  A
// lane reads its chunk at a stride of `chunk` dwords, which the design keeps odd: ds_read_b32 without a bank conflict.
#include <math.h>

#include "gs_common.h"

namespace gs {

constexpr int LD_NT = 256;
constexpr int LD_STEPS = GS_LOUDNESS_STEPS;   // log2(LD_NT)
static_assert((1 << LD_STEPS) == LD_NT, "the scan covers the block");
constexpr int LD_CAP_SMALL = 4800;            // a hop at up to 48 kHz: 19 KB of LDS a block
constexpr int LD_CAP_LARGE = 19200;           // at up to GS_LOUDNESS_MAX_RATE: 77 KB
static_assert(LD_CAP_LARGE * 10 == GS_LOUDNESS_MAX_RATE, "the large instantiation holds the longest hop");

struct LoudCoef { double b1[3], a1[2], b2[3], a2[2]; };   // both sections, a0 = 1
struct LoudMats { double m[LD_STEPS][16]; };               // P^(2^k), row-major
struct LoudMat { double m[16]; };

// one sample through both sections (transposed direct form II); s: the four state numbers
__device__ inline double loud_step(const LoudCoef& c, double x, double (&s)[4]) {
    const double y1 = c.b1[0] * x + s[0];
    s[0] = c.b1[1] * x - c.a1[0] * y1 + s[1];
    s[1] = c.b1[2] * x - c.a1[1] * y1;
    const double y2 = c.b2[0] * y1 + s[2];
    s[2] = c.b2[1] * y1 - c.a2[0] * y2 + s[3];
    s[3] = c.b2[2] * y1 - c.a2[1] * y2;
    return y2;
}

__device__ inline void loud_matvec_add(const double* __restrict__ m, const double (&v)[4], double (&acc)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += m[4 * r] * v[0] + m[4 * r + 1] * v[1] + m[4 * r + 2] * v[2] + m[4 * r + 3] * v[3];
}

// v[i] <- sum over k <= i of P^(i - k) v[k] over the block's lanes; buf: 4 * LD_NT doubles of LDS, free on entry and on return
__device__ inline void loud_scan(const LoudMats& pw, double (&v)[4], double* buf) {
    const int i = threadIdx.x;
#pragma unroll
    for (int k = 0; k < LD_STEPS; ++k) {
#pragma unroll
        for (int c = 0; c < 4; ++c) buf[c * LD_NT + i] = v[c];
        __syncthreads();
        if (i >= (1 << k)) {
            double u[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) u[c] = buf[c * LD_NT + i - (1 << k)];
            loud_matvec_add(pw.m[k], u, v);
        }
        __syncthreads();
    }
}

// every lane's v to every lane: -> lane `from`'s (from in [0, LD_NT))
__device__ inline void loud_fetch(const double (&v)[4], int from, double (&got)[4], double* buf) {
#pragma unroll
    for (int c = 0; c < 4; ++c) buf[c * LD_NT + threadIdx.x] = v[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) got[c] = buf[c * LD_NT + from];
    __syncthreads();
}

// the hop's samples src[0 .. hop) into LDS: -> xs with xs[t] = src[t] (barrier passed).  lds: 16-byte aligned, hop + 3 floats.
__device__ inline const float* loud_stage(const float* __restrict__ src, int hop, float* lds) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);     // floats past a 16-byte boundary
    float* xs = lds + mis;
    const int head = min((4 - mis) & 3, hop);
    const int packs = (hop - head) >> 2;
    if ((int)threadIdx.x < head) xs[threadIdx.x] = src[threadIdx.x];
    for (int p = threadIdx.x; p < packs; p += LD_NT)                        // (mis + head) % 4 == 0: both sides on 16 bytes
        *reinterpret_cast<float4*>(xs + head + 4 * p) = *reinterpret_cast<const float4*>(src + head + 4 * p);
    for (int t = head + 4 * packs + threadIdx.x; t < hop; t += LD_NT) xs[t] = src[t];
    __syncthreads();
    return xs;
}

// the lane's chunk from the state s: s becomes its end; -> the sum of the squared outputs
__device__ inline double loud_run(const LoudCoef& c, const float* xs, int begin, int count, double (&s)[4]) {
    double acc = 0.0;
    for (int k = 0; k < count; ++k) {
        const double y = loud_step(c, (double)xs[begin + k], s);
        acc += y * y;
    }
    return acc;
}

// What both hop kernels share.  The lane's chunk is [begin, begin + count) of the hop: `chunk` samples for the lanes below last = lanes - 1,
// the remaining `rem` for lane `last`, none above.  -> start: the state lane i's chunk starts in when the hop starts in `seed`; z: the
// lane's end from rest.
__device__ inline const float* loud_chunk_starts(const float* __restrict__ x, long row_stride, int hop, int chunk, const LoudCoef& coef,
                                                 const LoudMats& chunk_pow, const double (&seed)[4], float* lds, double* buf, int& begin,
                                                 int& count, double (&z)[4], double (&start)[4]) {
    const float* src = x + (size_t)blockIdx.y * row_stride + (size_t)blockIdx.x * hop;
    const float* xs = loud_stage(src, hop, lds);
    const int i = threadIdx.x;
    const int last = (hop + chunk - 1) / chunk - 1;
    begin = i <= last ? i * chunk : hop;
    count = i < last ? chunk : (i == last ? hop - begin : 0);
#pragma unroll
    for (int c = 0; c < 4; ++c) z[c] = 0.0;
    loud_run(coef, xs, begin, count, z);
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = i < last ? z[c] : 0.0;           // only whole chunks enter the scan: its matrix is A^chunk
    if (i == 0 && last > 0) loud_matvec_add(chunk_pow.m[0], seed, v);
    loud_scan(chunk_pow, v, buf);                                        // v: the state at the end of chunk i, for i < last
    loud_fetch(v, i > 0 ? i - 1 : 0, start, buf);
    if (i == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) start[c] = seed[c];
    }
    return xs;
}

// grid (hops, rows).  Z[(r * hops + j) * 4 ..]: the state hop j of row r ends in when it starts at rest
template <int CAP>
__global__ __launch_bounds__(LD_NT) void loud_ends_kernel(const float* __restrict__ x, long row_stride, int hop, int chunk, LoudCoef coef,
                                                          LoudMats chunk_pow, LoudMat rem_pow, double* __restrict__ Z) {
    __shared__ __attribute__((aligned(16))) float lds[CAP + 4];
    __shared__ double buf[4 * LD_NT];
    const double rest[4] = {0.0, 0.0, 0.0, 0.0};
    int begin, count;
    double z[4], start[4];
    loud_chunk_starts(x, row_stride, hop, chunk, coef, chunk_pow, rest, lds, buf, begin, count, z, start);
    if ((int)threadIdx.x == (hop + chunk - 1) / chunk - 1) {             // the last chunk: rem samples from `start`
        loud_matvec_add(rem_pow.m, start, z);
        double* out = Z + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = z[c];
    }
}

// grid (rows).  S[(r * hops + j) * 4 ..]: the state hop j of row r starts in (rest for j = 0), from Z and the powers of A^hop
__global__ __launch_bounds__(LD_NT) void loud_carry_kernel(const double* __restrict__ Z, double* __restrict__ S, long hops, LoudMats hop_pow) {
    __shared__ double buf[4 * LD_NT];
    const int i = threadIdx.x;
    const double* zr = Z + (size_t)blockIdx.x * hops * 4;
    double* sr = S + (size_t)blockIdx.x * hops * 4;
    double carry[4] = {0.0, 0.0, 0.0, 0.0};                              // the state the tile's first hop starts in
    for (long t0 = 0; t0 < hops; t0 += LD_NT) {
        const long j = t0 + i;
        double v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = j < hops ? zr[j * 4 + c] : 0.0;
        if (i == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sr[t0 * 4 + c] = carry[c];
            loud_matvec_add(hop_pow.m[0], carry, v);
        }
        loud_scan(hop_pow, v, buf);                                      // v: the state hop j ends in
        if (i < LD_NT - 1 && j + 1 < hops) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sr[(j + 1) * 4 + c] = v[c];
        }
        loud_fetch(v, LD_NT - 1, carry, buf);
    }
}

// grid (hops, rows).  energy[r * energy_stride + j]: the sum of the squared K-weighted samples of hop j of row r
template <int CAP>
__global__ __launch_bounds__(LD_NT) void loud_energy_kernel(const float* __restrict__ x, long row_stride, int hop, int chunk, LoudCoef coef,
                                                            LoudMats chunk_pow, const double* __restrict__ S, float* __restrict__ energy,
                                                            long energy_stride) {
    __shared__ __attribute__((aligned(16))) float lds[CAP + 4];
    __shared__ double buf[4 * LD_NT];
    const double* sj = S + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
    const double seed[4] = {sj[0], sj[1], sj[2], sj[3]};
    int begin, count;
    double z[4], start[4];
    const float* xs = loud_chunk_starts(x, row_stride, hop, chunk, coef, chunk_pow, seed, lds, buf, begin, count, z, start);
    buf[threadIdx.x] = loud_run(coef, xs, begin, count, start);
    __syncthreads();
#pragma unroll
    for (int w = LD_NT / 2; w >= 1; w >>= 1) {                           // a fixed tree: two calls are bit-identical
        if ((int)threadIdx.x < w) buf[threadIdx.x] += buf[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) energy[(size_t)blockIdx.y * energy_stride + blockIdx.x] = (float)buf[0];
}

// ---------------------------------------------------------------------------------------------------------------- host: the design
static void loud_matmul(const double* a, const double* b, double* out) {
    double t[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += a[4 * r + k] * b[4 * k + c];
            t[4 * r + c] = acc;
        }
    memcpy(out, t, sizeof(t));
}

static void loud_matpow(const double* a, long e, double* out) {         // binary powering, e >= 0
    double base[16], acc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    memcpy(base, a, sizeof(base));
    for (; e > 0; e >>= 1) {
        if (e & 1) loud_matmul(acc, base, acc);
        loud_matmul(base, base, base);
    }
    memcpy(out, acc, sizeof(acc));
}

// the bilinear forms of include/gansynth_hip.h; shelf: the first section, else the high-pass
static void loud_section(int rate, double f0, double q, bool shelf, double* b, double* a) {
    const double k = tan(M_PI * f0 / (double)rate);
    const double a0 = 1.0 + k / q + k * k;
    if (shelf) {
        const double vh = pow(10.0, 3.999843853973347 / 20.0), vb = pow(vh, 0.4996667741545416);
        b[0] = (vh + vb * k / q + k * k) / a0;
        b[1] = 2.0 * (k * k - vh) / a0;
        b[2] = (vh - vb * k / q + k * k) / a0;
    } else {
        b[0] = 1.0, b[1] = -2.0, b[2] = 1.0;
    }
    a[0] = 1.0;
    a[1] = 2.0 * (k * k - 1.0) / a0;
    a[2] = (1.0 - k / q + k * k) / a0;
}

static bool loud_rate_ok(int rate) { return rate >= GS_LOUDNESS_MIN_RATE && rate <= GS_LOUDNESS_MAX_RATE; }

static void loud_design(int rate, GsLoudness* d) {
    memset(d, 0, sizeof(*d));
    d->rate = rate;
    d->hop = (int)floor(0.1 * (double)rate + 0.5);
    d->chunk = ((d->hop + LD_NT - 1) / LD_NT) | 1;
    d->lanes = (d->hop + d->chunk - 1) / d->chunk;
    d->rem = d->hop - (d->lanes - 1) * d->chunk;
    loud_section(rate, 1681.974450955533, 0.7071752369554196, true, d->b1, d->a1);
    loud_section(rate, 38.13547087602444, 0.5003270373238773, false, d->b2, d->a2);
    // one silent sample on (s1[0], s1[1], s2[0], s2[1]): loud_step with x = 0
    const double a[16] = {-d->a1[1], 1, 0, 0,
                          -d->a1[2], 0, 0, 0,
                          d->b2[1] - d->a2[1] * d->b2[0], 0, -d->a2[1], 1,
                          d->b2[2] - d->a2[2] * d->b2[0], 0, -d->a2[2], 0};
    loud_matpow(a, d->chunk, d->chunk_pow[0]);
    loud_matpow(a, d->hop, d->hop_pow[0]);
    loud_matpow(a, d->rem, d->rem_pow);
    for (int k = 1; k < LD_STEPS; ++k) {
        loud_matmul(d->chunk_pow[k - 1], d->chunk_pow[k - 1], d->chunk_pow[k]);
        loud_matmul(d->hop_pow[k - 1], d->hop_pow[k - 1], d->hop_pow[k]);
    }
}

// a descriptor is taken only as gs_loudness_design leaves it: every number of it follows from the rate
static bool loud_design_ok(const GsLoudness* d) {
    if (d == nullptr || !loud_rate_ok(d->rate)) return false;
    GsLoudness want;
    loud_design(d->rate, &want);
    return memcmp(&want, d, sizeof(want)) == 0;
}

static bool loud_shape_ok(int rows, int64_t n) { return (rows == 1 || rows == 2) && n > 0 && n <= GS_LOUDNESS_MAX_N; }
static size_t loud_ws_bytes(int rows, int64_t hops) { return (size_t)rows * (size_t)(hops > 0 ? hops : 1) * 2 * 4 * sizeof(double); }

}  // namespace gs

using namespace gs;

extern "C" int gs_loudness_design(int rate, GsLoudness* out) {
    GS_CHECK_ARG(out != nullptr, "loudness_design: null descriptor");
    GS_CHECK_ARG(loud_rate_ok(rate), "loudness_design: rate must be in [%d, %d] (got %d)", GS_LOUDNESS_MIN_RATE, GS_LOUDNESS_MAX_RATE, rate);
    loud_design(rate, out);
    return 0;
}

extern "C" int64_t gs_loudness_hops(const GsLoudness* d, int64_t n) {
    if (!loud_design_ok(d)) return fail(GS_ERR_ARG, "loudness_hops: the descriptor does not follow from its rate (gs_loudness_design fills it)");
    GS_CHECK_ARG(n > 0 && n <= GS_LOUDNESS_MAX_N, "loudness_hops: n must be in [1, 2^40] (got %lld)", (long long)n);
    return n / d->hop;
}

extern "C" size_t gs_loudness_workspace_bytes(const GsLoudness* d, int rows, int64_t n) {
    if (!loud_design_ok(d) || !loud_shape_ok(rows, n)) return 0;
    return loud_ws_bytes(rows, n / d->hop);
}

extern "C" int gs_loudness(const GsLoudness* d, const float* x, int rows, int64_t n, int64_t row_stride, float* energy, int64_t energy_stride,
                           void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(loud_design_ok(d), "loudness: the descriptor does not follow from its rate (gs_loudness_design fills it)");
    GS_CHECK_ARG(rows == 1 || rows == 2, "loudness: rows must be 1 or 2 (got %d)", rows);
    GS_CHECK_ARG(n > 0 && n <= GS_LOUDNESS_MAX_N, "loudness: n must be in [1, 2^40] (got %lld)", (long long)n);
    GS_CHECK_ARG(row_stride >= n, "loudness: row_stride %lld is below n %lld", (long long)row_stride, (long long)n);
    const int64_t hops = n / d->hop;
    GS_CHECK_ARG(energy_stride >= hops, "loudness: energy_stride %lld is below the %lld hops of n", (long long)energy_stride, (long long)hops);
    GS_CHECK_ARG(x && energy, "loudness: null pointer (x and energy are required)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(energy) & 3) == 0,
                 "loudness: misaligned pointer (x / energy: 4 bytes)");
    const size_t need = loud_ws_bytes(rows, hops);
    GS_CHECK_ARG(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "loudness: workspace too small or misaligned (%zu bytes, need %zu)",
                 ws_bytes, need);
    if (hops == 0) return 0;   // no complete hop: nothing is measured, nothing is written
    hipStream_t st = as_stream(stream);
    double* Z = static_cast<double*>(ws);
    double* S = Z + (size_t)rows * (size_t)hops * 4;
    LoudCoef coef;
    for (int i = 0; i < 3; ++i) coef.b1[i] = d->b1[i], coef.b2[i] = d->b2[i];
    for (int i = 0; i < 2; ++i) coef.a1[i] = d->a1[i + 1], coef.a2[i] = d->a2[i + 1];
    LoudMats chunk_pow, hop_pow;
    LoudMat rem_pow;
    memcpy(chunk_pow.m, d->chunk_pow, sizeof(chunk_pow.m));
    memcpy(hop_pow.m, d->hop_pow, sizeof(hop_pow.m));
    memcpy(rem_pow.m, d->rem_pow, sizeof(rem_pow.m));
    const dim3 grid((unsigned)hops, (unsigned)rows);
    const int hop = d->hop, chunk = d->chunk;
    with_constant<LD_CAP_SMALL, LD_CAP_LARGE>(hop <= LD_CAP_SMALL ? LD_CAP_SMALL : LD_CAP_LARGE, [&](auto cap_c) {
        constexpr int CAP = decltype(cap_c)::value;
        hipLaunchKernelGGL((loud_ends_kernel<CAP>), grid, dim3(LD_NT), 0, st, x, (long)row_stride, hop, chunk, coef, chunk_pow, rem_pow, Z);
        hipLaunchKernelGGL(loud_carry_kernel, dim3((unsigned)rows), dim3(LD_NT), 0, st, static_cast<const double*>(Z), S, (long)hops, hop_pow);
        hipLaunchKernelGGL((loud_energy_kernel<CAP>), grid, dim3(LD_NT), 0, st, x, (long)row_stride, hop, chunk, coef, chunk_pow,
                           static_cast<const double*>(S), energy, (long)energy_stride);
        return true;
    });
    GS_CHECK_LAUNCH();
    return 0;
}
