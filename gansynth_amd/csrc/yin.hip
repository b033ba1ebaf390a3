// YIN fundamental-frequency tracker (de Cheveigne & Kawahara 2002, steps 1-5) for gansynth_amd/pitch.py, metrics.f0_pitch_accuracy_device and
// GANSynth.evaluate(f0=True); the rules are stated in include/gansynth_hip.h and DESIGN.md "Pitch tracking on the device", and tests/yin_ref.py
// restates them in float64 numpy.  No float atomics; two calls write the same bits, and gs_yin_track writes the bits of gs_yin_pick after
// gs_yin_difference because the three kernels run the same two device functions.
//
// One block of four waves owns one frame of one row.
//   yin_difference_block   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2 in the direct form, on the vector ALU (the energy-plus-cross-correlation form
//     cancels without a relative bound, and so does the matrix pipe's accumulation), and the frame power.
//     * The W + L - 1 samples of the frame are staged once in LDS (scalar loads: a row may start at any 4-byte alignment).
//     * A thread owns YN_R = 8 consecutive lags tau0 .. tau0 + 7, tau0 = 8 (thread % GP); GP = 64 lanes cover L <= 512, GP = 128 the rest, and the
//       256 / GP groups of lanes split the j range between them in runs of whole chunks (wave-uniform).  A chunk is YN_U = 4 consecutive j: one
//       ds_read_b128 of x[j .. j + 3] (one address a wave: a broadcast) and one of the four NEW values of the thread's window
//       x[j + tau0 + 8 .. + 11]; the other eight are still in registers from the chunks before (a window of 12 registers that rotates by four a
//       chunk: the loop body is three chunks, so that no value is ever moved).  Two 16-byte LDS reads feed 32 subtract / FMA pairs.
//     * Every lag's chain runs over j ascending inside its group's run; the groups' partial sums meet in LDS and are added in group order.  A sum
//       of W non-negative terms in this fixed order: within (W + 8) 2^-24, relative, of the exact value.  d(0) is a sum of exact zeros.
//     * The chains are scalar v_sub_f32 / v_fmac_f32 (build.sh: -fno-slp-vectorize; the generated loop has no v_pk_*): a packed pair would
//       have to hold two lags whose windows are one sample apart, and a register pair cannot be re-cut a sample further on without moves
//       (DESIGN.md has the reasoning and the measured rate).
//   yin_pick_block   rules 2-4 in float64 on the frame's d in LDS: lane 0 adds S(tau) = d(1) + ... + d(tau) sequentially (the result must not
//     depend on a scan tree), every thread turns its S into c(tau) = d(tau) tau / S(tau) (the product is exact: 24 + 10 bits), the first tau
//     under the threshold is an integer atomicMin in LDS, the fallback argmin a (value, index) tree with the lower index on a tie, and lane 0
//     walks down to the local minimum and fits the parabola.
//   yin_difference_kernel / yin_pick_kernel / yin_track_kernel   grid (rows * frames)
#include <limits.h>
#include <math.h>

#include "gs_common.h"

namespace gs {

constexpr int YN_NT = 256;       // threads per block
constexpr int YN_R = 8;          // consecutive lags a thread owns
constexpr int YN_U = 4;          // consecutive j of a chunk
constexpr int YN_WIN = YN_R + YN_U;   // registers of the rotating window
static_assert(YN_WIN % YN_U == 0 && YN_U == 4 && YN_R % 4 == 0, "the window rotates by whole 16-byte reads");
static_assert(GS_YIN_MAX_LAGS <= YN_NT / 2 * YN_R, "two groups of 128 lanes cover the lags");

// the LDS image of a block, in bytes from its (16-byte aligned) start: the doubles first
struct YinLds {
    int lq;        // L rounded up to 4
    int xs_n;      // floats of the staged frame: W + L - 1 samples, then zeros up to what the last lag thread's window reads
    int gp;        // lanes that share the lags: 64 or 128
    int c, redv, redi, dl, xs, psum;   // offsets
    int bytes;
};
__host__ __device__ inline YinLds yin_lds(int W, int L, bool difference) {
    YinLds s;
    s.lq = (L + 3) & ~3;
    s.xs_n = (W + L + 8 + 3) & ~3;
    s.gp = L <= 64 * YN_R ? 64 : 128;
    s.c = 0;                                   // double[lq]: S, then c
    s.redv = s.c + s.lq * 8;                   // double[YN_NT]
    s.redi = s.redv + YN_NT * 8;               // int[YN_NT]
    s.dl = s.redi + YN_NT * 4;                 // float[lq]
    s.xs = s.dl + s.lq * 4;                    // float[xs_n]
    s.psum = s.xs + (difference ? s.xs_n * 4 : 0);   // float[YN_NT * YN_R]: [group][gp * YN_R]
    s.bytes = s.psum + (difference ? YN_NT * YN_R * 4 : 0);
    return s;
}

// one chunk, PH = (chunk - first chunk) % 3: acc[k] += (x[j + u + tau0 + k] - x[j + u])^2 for u = 0 .. 3 in this order
template <int PH>
__device__ inline void yin_chunk(const float* __restrict__ xs, int j, int tau0, float (&win)[YN_WIN], float (&acc)[YN_R]) {
    float xj[4], nw[4];
    ld4(xs + j, xj);
    ld4(xs + j + tau0 + YN_R, nw);
#pragma unroll
    for (int e = 0; e < 4; ++e) win[(YN_R + YN_U * PH + e) % YN_WIN] = nw[e];
#pragma unroll
    for (int u = 0; u < YN_U; ++u)
#pragma unroll
        for (int k = 0; k < YN_R; ++k) {
            const float t = win[(YN_U * PH + k + u) % YN_WIN] - xj[u];
            acc[k] = fmaf(t, t, acc[k]);
        }
}

// frame = the frame's first sample.  Leaves d(0 .. L) in dl and returns the frame power (in every thread).  Ends with a barrier.
__device__ inline float yin_difference_block(const float* __restrict__ frame, int W, int L, const YinLds& s, unsigned char* lds) {
    float* xs = reinterpret_cast<float*>(lds + s.xs);
    float* psum = reinterpret_cast<float*>(lds + s.psum);
    float* dl = reinterpret_cast<float*>(lds + s.dl);
    const int tid = threadIdx.x;
    float pp = 0.f;
    for (int i = tid; i < s.xs_n; i += YN_NT) {
        const float v = i < W + L - 1 ? frame[i] : 0.f;
        xs[i] = v;
        if (i < W) pp = fmaf(v, v, pp);
    }
    const float power = block_sum<YN_NT>(pp, reinterpret_cast<float*>(lds + s.redv)) / (float)W;   // (its barriers also publish xs)

    const int parts = YN_NT / s.gp;
    const int group = tid / s.gp, tau0 = (tid & (s.gp - 1)) * YN_R;   // (group: wave-uniform)
    const int chunks = W / YN_U;
    const int per = (chunks + parts - 1) / parts;
    const int c0 = group * per, c1 = c0 + per < chunks ? c0 + per : chunks;
    float acc[YN_R];
#pragma unroll
    for (int k = 0; k < YN_R; ++k) acc[k] = 0.f;
    if (tau0 < L) {
        if (c0 < c1) {
            float win[YN_WIN];
            {
                float a[4], b[4];
                ld4(xs + YN_U * c0 + tau0, a);
                ld4(xs + YN_U * c0 + tau0 + 4, b);
#pragma unroll
                for (int e = 0; e < 4; ++e) { win[e] = a[e]; win[4 + e] = b[e]; win[8 + e] = 0.f; }
            }
            int c = c0;
            for (; c + 3 <= c1; c += 3) {
                yin_chunk<0>(xs, YN_U * c, tau0, win, acc);
                yin_chunk<1>(xs, YN_U * c + YN_U, tau0, win, acc);
                yin_chunk<2>(xs, YN_U * c + 2 * YN_U, tau0, win, acc);
            }
            if (c < c1) yin_chunk<0>(xs, YN_U * c, tau0, win, acc);
            if (c + 1 < c1) yin_chunk<1>(xs, YN_U * c + YN_U, tau0, win, acc);
        }
        if (group == parts - 1)   // the j past the last whole chunk: at most three
            for (int j = chunks * YN_U; j < W; ++j) {
                const float xj = xs[j];
#pragma unroll
                for (int k = 0; k < YN_R; ++k) {
                    const float t = xs[j + tau0 + k] - xj;
                    acc[k] = fmaf(t, t, acc[k]);
                }
            }
    }
    {
        float lo[4] = {acc[0], acc[1], acc[2], acc[3]}, hi[4] = {acc[4], acc[5], acc[6], acc[7]};
        st4(psum + group * s.gp * YN_R + tau0, lo);
        st4(psum + group * s.gp * YN_R + tau0 + 4, hi);
    }
    __syncthreads();
    for (int lag = tid; lag < L; lag += YN_NT) {
        float sum = psum[lag];
        for (int q = 1; q < parts; ++q) sum += psum[q * s.gp * YN_R + lag];
        dl[lag] = sum;
    }
    __syncthreads();
    return power;
}

// rules 2-4 on dl[0 .. L); the results are valid in thread 0.  Starts after a barrier that published dl.
__device__ inline void yin_pick_block(int L, int tau_min, double threshold, const YinLds& s, unsigned char* lds, int& lag, double& period, double& aper) {
    const float* dl = reinterpret_cast<const float*>(lds + s.dl);
    double* c = reinterpret_cast<double*>(lds + s.c);
    double* redv = reinterpret_cast<double*>(lds + s.redv);
    int* redi = reinterpret_cast<int*>(lds + s.redi);
    const int tid = threadIdx.x, hi = L - 2;
    if (tid == 0) {
        double sum = 0.0;
        for (int tau = 1; tau < L; ++tau) {   // sequential, ascending: S(tau)
            sum += (double)dl[tau];
            c[tau] = sum;
        }
        redi[0] = INT_MAX;
    }
    __syncthreads();
    for (int tau = tid; tau < L; tau += YN_NT) {
        const double sum = tau > 0 ? c[tau] : 0.0;
        c[tau] = sum == 0.0 ? 1.0 : ((double)dl[tau] * (double)tau) / sum;
    }
    __syncthreads();
    int first = INT_MAX;
    for (int tau = tau_min + tid; tau <= hi; tau += YN_NT)
        if (c[tau] < threshold) {
            first = tau;
            break;
        }
    if (first != INT_MAX) atomicMin(&redi[0], first);
    __syncthreads();
    first = redi[0];
    __syncthreads();
    if (first == INT_MAX) {   // (block-uniform) nothing under the threshold: the argmin, the lower index on a tie
        double best = INFINITY;
        int at = INT_MAX;
        for (int tau = tau_min + tid; tau <= hi; tau += YN_NT)
            if (c[tau] < best) {
                best = c[tau];
                at = tau;
            }
        redv[tid] = best;
        redi[tid] = at;
        __syncthreads();
        for (int half = YN_NT / 2; half > 0; half >>= 1) {
            if (tid < half) {
                const double v = redv[tid + half];
                const int i = redi[tid + half];
                if (v < redv[tid] || (v == redv[tid] && i < redi[tid])) {
                    redv[tid] = v;
                    redi[tid] = i;
                }
            }
            __syncthreads();
        }
        first = redi[0];
        if (first == INT_MAX) first = tau_min;   // (only a frame of NaN gets here)
    } else if (tid == 0) {
        while (first + 1 <= hi && c[first + 1] < c[first]) ++first;
    }
    if (tid == 0) {
        const double cm = c[first - 1], c0 = c[first], cp = c[first + 1];
        const double den = cm - 2.0 * c0 + cp;
        double off = 0.0;
        if (den > 0.0) {
            off = 0.5 * (cm - cp) / den;
            off = off < -1.0 ? -1.0 : off > 1.0 ? 1.0 : off;
        }
        lag = first;
        period = (double)first + off;
        aper = c0;
    }
}

__global__ __launch_bounds__(YN_NT) void yin_difference_kernel(const float* __restrict__ x, size_t ldx, int frames, int W, int L, int hop, float* __restrict__ d,
                                                               float* __restrict__ power) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const YinLds s = yin_lds(W, L, true);
    const size_t row = blockIdx.x / (unsigned)frames, f = blockIdx.x % (unsigned)frames;
    const float p = yin_difference_block(x + row * ldx + f * (size_t)hop, W, L, s, lds);
    const float* dl = reinterpret_cast<const float*>(lds + s.dl);
    float* out = d + (size_t)blockIdx.x * L;
    for (int lag = threadIdx.x; lag < L; lag += YN_NT) out[lag] = dl[lag];
    if (threadIdx.x == 0) power[blockIdx.x] = p;
}

__global__ __launch_bounds__(YN_NT) void yin_pick_kernel(const float* __restrict__ d, int L, int tau_min, double threshold, int* __restrict__ lag,
                                                         double* __restrict__ period, double* __restrict__ aper) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const YinLds s = yin_lds(L, L, false);
    float* dl = reinterpret_cast<float*>(lds + s.dl);
    const float* in = d + (size_t)blockIdx.x * L;
    for (int i = threadIdx.x; i < L; i += YN_NT) dl[i] = in[i];
    __syncthreads();
    int at = 0;
    double per = 0.0, ap = 0.0;
    yin_pick_block(L, tau_min, threshold, s, lds, at, per, ap);
    if (threadIdx.x == 0) {
        lag[blockIdx.x] = at;
        period[blockIdx.x] = per;
        aper[blockIdx.x] = ap;
    }
}

__global__ __launch_bounds__(YN_NT) void yin_track_kernel(const float* __restrict__ x, size_t ldx, int frames, int W, int L, int hop, int tau_min, double threshold,
                                                          int* __restrict__ lag, double* __restrict__ period, double* __restrict__ aper, float* __restrict__ power) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const YinLds s = yin_lds(W, L, true);
    const size_t row = blockIdx.x / (unsigned)frames, f = blockIdx.x % (unsigned)frames;
    const float p = yin_difference_block(x + row * ldx + f * (size_t)hop, W, L, s, lds);
    int at = 0;
    double per = 0.0, ap = 0.0;
    yin_pick_block(L, tau_min, threshold, s, lds, at, per, ap);
    if (threadIdx.x == 0) {
        lag[blockIdx.x] = at;
        period[blockIdx.x] = per;
        aper[blockIdx.x] = ap;
        power[blockIdx.x] = p;
    }
}


}  // namespace gs

using namespace gs;

#define YN_CHECK_FRAME(what)                                                                                                              \
    GS_CHECK_ARG(L >= 4 && L <= GS_YIN_MAX_LAGS, what ": L must be in [4, %d] (got %d)", GS_YIN_MAX_LAGS, L);                              \
    GS_CHECK_ARG(W >= L && W <= GS_YIN_MAX_WINDOW, what ": W must be in [L, %d] (got %d, L %d)", GS_YIN_MAX_WINDOW, W, L);                 \
    GS_CHECK_ARG(hop >= 1, what ": hop must be positive (got %d)", hop);                                                                  \
    GS_CHECK_ARG(n >= (int64_t)W + L, what ": n %lld is below W + L = %d", (long long)n, W + L)

#define YN_CHECK_ROWS(what, frames)                                                                                                       \
    GS_CHECK_ARG(rows >= 1, what ": rows must be positive (got %lld)", (long long)rows);                                                  \
    GS_CHECK_ARG(rows <= (int64_t)INT_MAX / (frames), what ": rows %lld x %lld frames exceed 2^31 - 1 blocks", (long long)rows, (long long)(frames))

#define YN_CHECK_PICK(what)                                                                                                               \
    GS_CHECK_ARG(tau_min >= 2, what ": tau_min must be at least 2 (got %d)", tau_min);                                                    \
    GS_CHECK_ARG(L >= tau_min + 2 && L <= GS_YIN_MAX_LAGS, what ": L must be in [tau_min + 2, %d] (got %d, tau_min %d)", GS_YIN_MAX_LAGS, L, tau_min)

static int64_t yn_frames(int64_t n, int W, int L, int hop) { return (n - W - L) / hop + 1; }

extern "C" int64_t gs_yin_frames(int64_t n, int W, int L, int hop) {
    const int code = [&]() -> int {
        YN_CHECK_FRAME("yin_frames");
        return 0;
    }();
    return code ? 0 : yn_frames(n, W, L, hop);
}

extern "C" int gs_yin_difference(const float* x, int64_t ldx, int64_t rows, int64_t n, int W, int L, int hop, float* d, float* power, void* stream) {
    YN_CHECK_FRAME("yin_difference");
    GS_CHECK_ARG(ldx >= n, "yin_difference: ldx %lld is below n %lld", (long long)ldx, (long long)n);
    const int64_t frames = yn_frames(n, W, L, hop);
    GS_CHECK_ARG(frames <= INT_MAX, "yin_difference: n %lld gives more than 2^31 - 1 frames", (long long)n);
    YN_CHECK_ROWS("yin_difference", frames);
    GS_CHECK_ARG(x && d && power, "yin_difference: null pointer (x, d and power are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(d, 4) && aligned(power, 4), "yin_difference: misaligned pointer (x, d and power: 4 bytes)");
    const YinLds s = yin_lds(W, L, true);
    hipLaunchKernelGGL(yin_difference_kernel, dim3((unsigned)(rows * frames)), dim3(YN_NT), (size_t)s.bytes, as_stream(stream), x, (size_t)ldx, (int)frames, W, L, hop,
                       d, power);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_yin_pick(const float* d, int64_t rows, int64_t frames, int L, int tau_min, double threshold, int32_t* lag, double* period, double* aperiodicity,
                           void* stream) {
    YN_CHECK_PICK("yin_pick");
    GS_CHECK_ARG(frames >= 1 && frames <= INT_MAX, "yin_pick: F must be in [1, 2^31 - 1] (got %lld)", (long long)frames);
    YN_CHECK_ROWS("yin_pick", frames);
    GS_CHECK_ARG(d && lag && period && aperiodicity, "yin_pick: null pointer (d, lag, period and aperiodicity are required)");
    GS_CHECK_ARG(aligned(d, 4) && aligned(lag, 4) && aligned(period, 8) && aligned(aperiodicity, 8),
                 "yin_pick: misaligned pointer (d and lag: 4 bytes; period and aperiodicity: 8)");
    const YinLds s = yin_lds(L, L, false);
    hipLaunchKernelGGL(yin_pick_kernel, dim3((unsigned)(rows * frames)), dim3(YN_NT), (size_t)s.bytes, as_stream(stream), d, L, tau_min, threshold, lag, period,
                       aperiodicity);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_yin_track(const float* x, int64_t ldx, int64_t rows, int64_t n, int W, int L, int hop, int tau_min, double threshold, int32_t* lag, double* period,
                            double* aperiodicity, float* power, void* stream) {
    YN_CHECK_PICK("yin_track");
    YN_CHECK_FRAME("yin_track");
    GS_CHECK_ARG(ldx >= n, "yin_track: ldx %lld is below n %lld", (long long)ldx, (long long)n);
    const int64_t frames = yn_frames(n, W, L, hop);
    GS_CHECK_ARG(frames <= INT_MAX, "yin_track: n %lld gives more than 2^31 - 1 frames", (long long)n);
    YN_CHECK_ROWS("yin_track", frames);
    GS_CHECK_ARG(x && lag && period && aperiodicity && power, "yin_track: null pointer (x, lag, period, aperiodicity and power are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(lag, 4) && aligned(power, 4) && aligned(period, 8) && aligned(aperiodicity, 8),
                 "yin_track: misaligned pointer (x, lag and power: 4 bytes; period and aperiodicity: 8)");
    const YinLds s = yin_lds(W, L, true);
    hipLaunchKernelGGL(yin_track_kernel, dim3((unsigned)(rows * frames)), dim3(YN_NT), (size_t)s.bytes, as_stream(stream), x, (size_t)ldx, (int)frames, W, L, hop,
                       tau_min, threshold, lag, period, aperiodicity, power);
    GS_CHECK_LAUNCH();
    return 0;
}
