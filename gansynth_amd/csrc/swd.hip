// Sliced Wasserstein distance between Laplacian-pyramid patches (gansynth_amd/swd.py, metrics.sliced_wasserstein_distance_device; the rules are
// this project's own and are stated in include/gansynth_hip.h and DESIGN.md "SWD on the device").  fp32 values, double sums, fixed orders, no
// float atomics: two calls agree bit for bit.  No sort or scan library is used.
//   swd_down_kernel<T>      G_{l+1} = the 5x5 binomial filter of G_l at the even rows and columns (mirror border), a thread per output pixel,
//                           both channels; rows first ((((k0 x0 + k1 x1) + k2 x2) + k3 x3) + k4 x4), then the five row sums the same way
//   swd_lap_kernel<T>       Lap_l = G_l - up(G_{l+1}): the taps of the zero-stuffed image that fall on an even index (three on an even row or
//                           column, two on an odd one), in ascending order, rows first
//   swd_widen_kernel<T>     Lap_{L-1} = G_{L-1}
//   swd_patches_kernel      a thread per descriptor value
//   swd_moments_kernel      grid (blocks): a block's contiguous share of the buffer, per channel sum and sum of squares in double, a fixed tree
//   swd_fold_kernel         grid (1): the blocks' partials in block order, a fixed tree; for the moments also mean and standard deviation
//   swd_project_kernel      a block owns 128 rows, normalised on the way into LDS as a[k][row]; the directions come through LDS 32 at a time; a
//                           thread holds 4 rows x 4 directions, each ONE chain of 98 FMAs over k ascending (the fp32 vector pipe: K = 98
//                           is no multiple of an MFMA's K and the rule fixes the order of the sum)
//   swd_sort_tile_kernel    grid (tiles, rows): a tile of GS_SWD_SORT_TILE values as order-preserving unsigned keys in LDS, a bitonic network
//                           over the power of two that covers the tile's values; the padding (the largest key) sorts behind them and is not written
//   swd_merge_kernel        grid (chunks of 2048 outputs, rows): one pass that merges neighbouring sorted runs; a block finds its share of
//                           both runs by two merge-path searches, stages it in LDS, every thread merges 8 outputs from its own diagonal
//   swd_l1_kernel           grid (blocks): sum |a - b| of a contiguous share in double, a fixed tree; then swd_fold_kernel
#include <math.h>

#include "gs_common.h"

namespace gs {

constexpr int SW_NT = 256;
constexpr int SW_TILE = GS_SWD_SORT_TILE;
constexpr int SW_MC = 2048;                   // outputs a block of a merge pass owns
constexpr int SW_PER = SW_MC / SW_NT;         // ... and a thread of it
constexpr int SW_D = GS_SWD_DESC;             // 98
constexpr int SW_PP = GS_SWD_PATCHES;         // 128
constexpr int PJ_ROWS = 128, PJ_DIRS = 32;    // rows a block of the projection owns, directions per round
constexpr int PJ_LD = PJ_ROWS + 1;            // floats between two k of a[k][row]: the staging writes (consecutive k) hit distinct banks
constexpr int SW_MAX_BLOCKS = 1024;           // partials of a two-stage sum, at most
static_assert(SW_TILE % SW_MC == 0 && (SW_TILE & (SW_TILE - 1)) == 0, "a merge block's outputs lie inside one pair of runs");
static_assert((SW_D * PJ_LD + SW_D * PJ_DIRS) * 4 <= 65536, "the projection's two LDS arrays");

// the mirror without the edge sample: d c b | a b c d | c b a
__device__ inline int mirror(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

template <typename T>
__global__ __launch_bounds__(SW_NT) void swd_down_kernel(const T* __restrict__ in, long b, int h, int w, float* __restrict__ out) {
    const int ho = h / 2, wo = w / 2;
    const long total = b * ho * wo;
    const float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    for (long i = (long)blockIdx.x * SW_NT + threadIdx.x; i < total; i += (long)gridDim.x * SW_NT) {
        const int xo = (int)(i % wo);
        const long r = i / wo;
        const int yo = (int)(r % ho);
        const T* __restrict__ base = in + (size_t)(r / ho) * h * w * 2;
        float v0 = 0.f, v1 = 0.f;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const T* __restrict__ row = base + (size_t)mirror(2 * yo + dy - 2, h) * w * 2;
            float h0 = 0.f, h1 = 0.f;
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) {
                const T* p = row + (size_t)mirror(2 * xo + dx - 2, w) * 2;
                h0 = dx == 0 ? K[0] * DT<T>::ld(p) : fmaf(K[dx], DT<T>::ld(p), h0);
                h1 = dx == 0 ? K[0] * DT<T>::ld(p + 1) : fmaf(K[dx], DT<T>::ld(p + 1), h1);
            }
            v0 = dy == 0 ? K[0] * h0 : fmaf(K[dy], h0, v0);
            v1 = dy == 0 ? K[0] * h1 : fmaf(K[dy], h1, v1);
        }
        out[2 * i] = v0;
        out[2 * i + 1] = v1;
    }
}

// the taps of 4 x the filter on the zero-stuffed axis of n2 samples that fall on a stuffed (even) index: -> their number; index into the coarse axis, weight
__device__ inline int up_taps(int y, int n2, int (&idx)[3], float (&wt)[3]) {
    const float K[5] = {0.125f, 0.5f, 0.75f, 0.5f, 0.125f};
    int c = 0;
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
        const int p = mirror(y + d, n2);
        if (!(p & 1) && c < 3) { idx[c] = p >> 1; wt[c] = K[d + 2]; ++c; }
    }
    return c;
}

template <typename T>
__global__ __launch_bounds__(SW_NT) void swd_lap_kernel(const T* __restrict__ fine, const float* __restrict__ coarse, long b, int h, int w, float* __restrict__ out) {
    const int hc = h / 2, wc = w / 2;
    const long total = b * h * w;
    for (long i = (long)blockIdx.x * SW_NT + threadIdx.x; i < total; i += (long)gridDim.x * SW_NT) {
        const int x = (int)(i % w);
        const long r = i / w;
        const int y = (int)(r % h);
        const float* __restrict__ base = coarse + (size_t)(r / h) * hc * wc * 2;
        int iy[3], ix[3];
        float wy[3], wx[3];
        const int ny = up_taps(y, h, iy, wy), nx = up_taps(x, w, ix, wx);
        float v0 = 0.f, v1 = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a >= ny) continue;
            const float* __restrict__ row = base + (size_t)iy[a] * wc * 2;
            float h0 = 0.f, h1 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= nx) continue;
                h0 = c == 0 ? wx[0] * row[2 * ix[0]] : fmaf(wx[c], row[2 * ix[c]], h0);
                h1 = c == 0 ? wx[0] * row[2 * ix[0] + 1] : fmaf(wx[c], row[2 * ix[c] + 1], h1);
            }
            v0 = a == 0 ? wy[0] * h0 : fmaf(wy[a], h0, v0);
            v1 = a == 0 ? wy[0] * h1 : fmaf(wy[a], h1, v1);
        }
        out[2 * i] = DT<T>::ld(fine + 2 * i) - v0;
        out[2 * i + 1] = DT<T>::ld(fine + 2 * i + 1) - v1;
    }
}

template <typename T>
__global__ __launch_bounds__(SW_NT) void swd_widen_kernel(const T* __restrict__ in, long count, float* __restrict__ out) {
    for (long i = (long)blockIdx.x * SW_NT + threadIdx.x; i < count; i += (long)gridDim.x * SW_NT) out[i] = DT<T>::ld(in + i);
}

// desc[row_offset + img * 128 + p][(c * 7 + dy) * 7 + dx] = level[img][ys + dy][xs + dx][c]; a corner outside the level is moved inside it
__global__ __launch_bounds__(SW_NT) void swd_patches_kernel(const float* __restrict__ level, long b, int h, int w, const int* __restrict__ ys,
                                                            const int* __restrict__ xs, float* __restrict__ desc, long row_offset) {
    const long total = b * SW_PP * SW_D;
    for (long i = (long)blockIdx.x * SW_NT + threadIdx.x; i < total; i += (long)gridDim.x * SW_NT) {
        const long row = i / SW_D;
        const int k = (int)(i % SW_D);
        const int c = k / 49, dy = (k % 49) / 7, dx = k % 7;
        int y0 = ys[row], x0 = xs[row];
        y0 = y0 < 0 ? 0 : (y0 > h - 7 ? h - 7 : y0);
        x0 = x0 < 0 ? 0 : (x0 > w - 7 ? w - 7 : x0);
        desc[(size_t)(row_offset + row) * SW_D + k] = level[(((size_t)(row / SW_PP) * h + y0 + dy) * w + x0 + dx) * 2 + c];
    }
}

// the sum over the block in thread 0 (block_tree_f64's fixed tree); sm: SW_NT doubles, shared by a kernel's calls
__device__ inline double block_tree_sum(double v, double* sm) {
    __syncthreads();   // (the array may still be read from the call before)
    return block_tree_f64<SW_NT>(v, sm);
}

// part[block][4] = sum c0, sum of squares c0, sum c1, sum of squares c1 over the block's share [block * share, ...) of the count values
__global__ __launch_bounds__(SW_NT) void swd_moments_kernel(const float* __restrict__ desc, long count, long share, double* __restrict__ part) {
    __shared__ double sm[SW_NT];
    const long begin = (long)blockIdx.x * share, end = begin + share < count ? begin + share : count;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long i = begin + threadIdx.x; i < end; i += SW_NT) {
        const double v = (double)desc[i];
        const int c = (i % SW_D) >= 49 ? 2 : 0;
        s[c] += v;
        s[c + 1] = fma(v, v, s[c + 1]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double total = block_tree_sum(s[q], sm);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * 4 + q] = total;
    }
}

// out[q] = the sum of part[.][q] in block order (a thread's share ascending, then a fixed tree); with m > 0 (the moments): out = per channel
// (sum, sum of squares, mean, population standard deviation) for m values a channel
__global__ __launch_bounds__(SW_NT) void swd_fold_kernel(const double* __restrict__ part, int blocks, int cols, long m, double* __restrict__ out) {
    __shared__ double sm[SW_NT];
    __shared__ double tot[4];
    for (int q = 0; q < cols; ++q) {
        double s = 0.0;
        for (int i = threadIdx.x; i < blocks; i += SW_NT) s += part[(size_t)i * cols + q];
        const double total = block_tree_sum(s, sm);
        if (threadIdx.x == 0) tot[q] = total;
    }
    if (threadIdx.x != 0) return;
    if (m <= 0) {
        for (int q = 0; q < cols; ++q) out[q] = tot[q];
        return;
    }
    for (int c = 0; c < 2; ++c) {
        const double mean = tot[2 * c] / (double)m;
        const double var = tot[2 * c + 1] / (double)m - mean * mean;
        out[4 * c] = tot[2 * c];
        out[4 * c + 1] = tot[2 * c + 1];
        out[4 * c + 2] = mean;
        out[4 * c + 3] = var > 0.0 ? sqrt(var) : 0.0;
    }
}

// out[dir][row] = sum over k ascending of ((desc[row][k] - mean_c) / std_c) * dirs[k][dir], mean and std rounded once to fp32
__global__ __launch_bounds__(SW_NT) void swd_project_kernel(const float* __restrict__ desc, long n, const double* __restrict__ moments,
                                                            const float* __restrict__ dirs, int ndir, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float as[SW_D * PJ_LD];
    __shared__ __attribute__((aligned(16))) float ds[SW_D * PJ_DIRS];
    const int tid = threadIdx.x, rl = tid & 31, dg = tid >> 5;
    const long row0 = (long)blockIdx.x * PJ_ROWS;
    const float mean[2] = {(float)moments[2], (float)moments[6]}, sd[2] = {(float)moments[3], (float)moments[7]};
    for (int f = tid; f < PJ_ROWS * SW_D; f += SW_NT) {
        const int r = f / SW_D, k = f % SW_D;
        const int c = k >= 49;
        as[k * PJ_LD + r] = row0 + r < n ? (desc[(size_t)row0 * SW_D + f] - mean[c]) / sd[c] : 0.f;
    }
    for (int c0 = 0; c0 < ndir; c0 += PJ_DIRS) {
        __syncthreads();   // the round before is consumed (and, the first time, as is written)
        for (int f = tid; f < SW_D * PJ_DIRS; f += SW_NT) {
            const int k = f / PJ_DIRS, j = f % PJ_DIRS;
            ds[f] = c0 + j < ndir ? dirs[(size_t)k * ndir + c0 + j] : 0.f;
        }
        __syncthreads();
        float acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] = 0.f;
#pragma unroll 2
        for (int k = 0; k < SW_D; ++k) {
            float a[4], d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = as[k * PJ_LD + rl + 32 * j];
            ld4(ds + k * PJ_DIRS + dg * 4, d);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(a[j], d[e], acc[j][e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int dir = c0 + dg * 4 + e;
            if (dir >= ndir) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long row = row0 + rl + 32 * j;
                if (row < n) out[(size_t)dir * n + row] = acc[j][e];
            }
        }
    }
}

// a float as an unsigned key of the same order (-0 below +0; every finite value and both infinities below 0xffffffff, the padding)
__device__ inline unsigned key_of(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

__global__ __launch_bounds__(SW_NT) void swd_sort_tile_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
    __shared__ unsigned s[SW_TILE];
    const size_t at = (size_t)blockIdx.y * n + (size_t)blockIdx.x * SW_TILE;
    const long left = n - (long)blockIdx.x * SW_TILE;
    const int valid = left < SW_TILE ? (int)left : SW_TILE;
    int P = 2;
    while (P < valid) P <<= 1;   // (block-uniform; at most SW_TILE)
    for (int i = threadIdx.x; i < P; i += SW_NT) s[i] = i < valid ? key_of(in[at + i]) : 0xffffffffu;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < P / 2; i += SW_NT) {
                const int l = ((i & ~(j - 1)) << 1) | (i & (j - 1)), r = l | j;
                const unsigned a = s[l], b = s[r];
                if ((a > b) == ((l & k) == 0)) { s[l] = b; s[r] = a; }
            }
        }
    __syncthreads();
    for (int i = threadIdx.x; i < valid; i += SW_NT) out[at + i] = float_of(s[i]);
}

// how many of the first d values of merge(A, B) come from A (A first on ties).  Reads A[m], B[d - 1 - m] only inside both runs.
template <typename FA, typename FB>
__device__ inline long merge_path(FA&& a_key, long la, FB&& b_key, long lb, long d) {
    long lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const long m = (lo + hi) >> 1;
        if (a_key(m) <= b_key(d - 1 - m)) lo = m + 1; else hi = m;
    }
    return lo;
}

// one pass: out = the runs of `run` values of in, merged two and two (a last run without a partner is copied)
__global__ __launch_bounds__(SW_NT) void swd_merge_kernel(const float* __restrict__ in, float* __restrict__ out, long n, long run) {
    __shared__ unsigned sk[SW_MC];
    __shared__ unsigned so[SW_MC];
    __shared__ long split[2];
    const size_t rowat = (size_t)blockIdx.y * n;
    const long o0 = (long)blockIdx.x * SW_MC;
    const long base = o0 / (2 * run) * (2 * run);
    const long la = n - base < run ? n - base : run;
    const long lb = n - base - la < run ? n - base - la : run;   // (0 without a partner)
    const float* __restrict__ A = in + rowat + base;
    const float* __restrict__ B = A + la;
    const long d0 = o0 - base, d1 = d0 + SW_MC < la + lb ? d0 + SW_MC : la + lb;
    if (threadIdx.x < 2)
        split[threadIdx.x] = merge_path([&](long i) { return key_of(A[i]); }, la, [&](long i) { return key_of(B[i]); }, lb, threadIdx.x ? d1 : d0);
    __syncthreads();
    const long a0 = split[0], a1 = split[1], b0 = d0 - a0, b1 = d1 - a1;
    const int na = (int)(a1 - a0), nb = (int)(b1 - b0), cnt = na + nb;   // cnt = d1 - d0 <= SW_MC
    for (int i = threadIdx.x; i < na; i += SW_NT) sk[i] = key_of(A[a0 + i]);
    for (int i = threadIdx.x; i < nb; i += SW_NT) sk[na + i] = key_of(B[b0 + i]);
    __syncthreads();
    const int dd = threadIdx.x * SW_PER < cnt ? threadIdx.x * SW_PER : cnt;
    int ia = (int)merge_path([&](long i) { return sk[i]; }, na, [&](long i) { return sk[na + i]; }, nb, dd);
    int ib = dd - ia;
#pragma unroll
    for (int j = 0; j < SW_PER; ++j)
        if (dd + j < cnt) {
            const bool take_a = ib >= nb || (ia < na && sk[ia] <= sk[na + ib]);
            so[dd + j] = take_a ? sk[ia] : sk[na + ib];
            ia += take_a;
            ib += !take_a;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += SW_NT) out[rowat + o0 + i] = float_of(so[i]);
}

__global__ __launch_bounds__(SW_NT) void swd_l1_kernel(const float* __restrict__ a, const float* __restrict__ b, long count, long share, double* __restrict__ part) {
    __shared__ double sm[SW_NT];
    const long begin = (long)blockIdx.x * share, end = begin + share < count ? begin + share : count;
    double s = 0.0;
    for (long i = begin + threadIdx.x; i < end; i += SW_NT) s += fabs((double)a[i] - (double)b[i]);
    const double total = block_tree_sum(s, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------------------- host arithmetic
static int sw_levels(long h, long w) {
    if (h < 16 || w < 16 || h > GS_SWD_MAX_SIDE || w > GS_SWD_MAX_SIDE) return 0;
    int levels = 0;
    while ((h < w ? h : w) >= 16) {
        ++levels;
        if ((h < w ? h : w) / 2 < 16) break;   // the last level: it is not halved
        if ((h | w) & 1) return 0;             // an odd size on the way down
        h /= 2;
        w /= 2;
    }
    return (h >= 7 && w >= 7) ? levels : 0;
}
static bool sw_batch_ok(int64_t b) { return b >= 1 && b <= GS_SWD_MAX_BATCH; }
// floats of the levels 1 .. L-1 of b images (the Gaussian pyramid the Laplacian one is made from)
static size_t sw_gauss_floats(int64_t b, int h, int w, int levels) {
    size_t total = 0;
    for (int l = 1; l < levels; ++l) total += (size_t)b * (h >> l) * (w >> l) * 2;
    return total;
}
static int sw_blocks(int64_t count) {   // of a two-stage sum over count values: at least 2048 values a block
    const int64_t blocks = (count + 2047) / 2048;
    return (int)(blocks < SW_MAX_BLOCKS ? blocks : SW_MAX_BLOCKS);
}
static bool sw_rows_n_ok(int64_t rows, int64_t n) { return rows >= 1 && rows <= GS_SWD_MAX_ROWS && n >= 1 && n <= GS_SWD_MAX_N; }
static size_t sw_round16(size_t v) { return (v + 15) & ~(size_t)15; }
static size_t sw_ws_bytes(int stage, int64_t a, int64_t b, int64_t c) {
    switch (stage) {
        case GS_SWD_STAGE_PYRAMID: {
            const int levels = (b > 0 && c > 0 && b <= GS_SWD_MAX_SIDE && c <= GS_SWD_MAX_SIDE) ? sw_levels(b, c) : 0;
            if (!sw_batch_ok(a) || levels == 0) return 0;
            return sw_round16(sw_gauss_floats(a, (int)b, (int)c, levels) * sizeof(float) + 16);
        }
        case GS_SWD_STAGE_MOMENTS:
            if (a < 1 || a > GS_SWD_MAX_N) return 0;
            return sw_round16((size_t)sw_blocks(a * SW_D) * 4 * sizeof(double));
        case GS_SWD_STAGE_SORT:
            if (!sw_rows_n_ok(a, b)) return 0;
            return b > SW_TILE ? sw_round16((size_t)a * b * sizeof(float)) : 16;
        case GS_SWD_STAGE_L1:
            if (!sw_rows_n_ok(a, b)) return 0;
            return sw_round16((size_t)sw_blocks(a * b) * sizeof(double));
        default: return 0;
    }
}
static unsigned sw_grid(int64_t threads) {
    const int64_t blocks = (threads + SW_NT - 1) / SW_NT;
    return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace gs

using namespace gs;

#define SW_CHECK_WS(what, need) \
    GS_CHECK_ARG(ws && ws_bytes >= (need) && aligned(ws, 16), what ": workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, (size_t)(need))

extern "C" int gs_swd_levels(int h, int w) { return sw_levels(h, w); }

extern "C" size_t gs_swd_workspace_bytes(int stage, int64_t a, int64_t b, int64_t c) { return sw_ws_bytes(stage, a, b, c); }

extern "C" int gs_swd_pyramid(const void* x, int dtype, int64_t b, int h, int w, float* lap, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(dtype == GS_F32 || dtype == GS_BF16, "swd_pyramid: bad dtype %d", dtype);
    GS_CHECK_ARG(sw_batch_ok(b), "swd_pyramid: b must be in [1, %d] (got %lld)", GS_SWD_MAX_BATCH, (long long)b);
    const int levels = sw_levels(h, w);
    GS_CHECK_ARG(levels > 0, "swd_pyramid: %d x %d has no level (both sides at least 16 and at most %d, every halved size even)", h, w, GS_SWD_MAX_SIDE);
    GS_CHECK_ARG(x && lap, "swd_pyramid: null pointer (x and lap are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(lap, 4), "swd_pyramid: misaligned pointer (4 bytes)");
    SW_CHECK_WS("swd_pyramid", sw_ws_bytes(GS_SWD_STAGE_PYRAMID, b, h, w));
    hipStream_t st = as_stream(stream);
    GS_DISPATCH_DTYPE(dtype, {
        const float* g = nullptr;          // G_l for l >= 1 (G_0 is x)
        float* next = static_cast<float*>(ws);
        float* o = lap;
        for (int l = 0; l < levels; ++l) {
            const int hl = h >> l, wl = w >> l;
            const long px = (long)b * hl * wl;
            if (l == levels - 1) {
                if (l == 0) hipLaunchKernelGGL((swd_widen_kernel<T>), dim3(sw_grid(px * 2)), dim3(SW_NT), 0, st, static_cast<const T*>(x), px * 2, o);
                else hipLaunchKernelGGL((swd_widen_kernel<float>), dim3(sw_grid(px * 2)), dim3(SW_NT), 0, st, g, px * 2, o);
                break;
            }
            if (l == 0) {
                hipLaunchKernelGGL((swd_down_kernel<T>), dim3(sw_grid(px / 4)), dim3(SW_NT), 0, st, static_cast<const T*>(x), (long)b, hl, wl, next);
                hipLaunchKernelGGL((swd_lap_kernel<T>), dim3(sw_grid(px)), dim3(SW_NT), 0, st, static_cast<const T*>(x), static_cast<const float*>(next), (long)b, hl, wl, o);
            } else {
                hipLaunchKernelGGL((swd_down_kernel<float>), dim3(sw_grid(px / 4)), dim3(SW_NT), 0, st, g, (long)b, hl, wl, next);
                hipLaunchKernelGGL((swd_lap_kernel<float>), dim3(sw_grid(px)), dim3(SW_NT), 0, st, g, static_cast<const float*>(next), (long)b, hl, wl, o);
            }
            g = next;
            next += px / 4 * 2;
            o += px * 2;
        }
    });
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_swd_patches(const float* level, int64_t b, int h, int w, const int32_t* ys, const int32_t* xs, float* desc, int64_t desc_rows, int64_t row_offset,
                              void* stream) {
    GS_CHECK_ARG(sw_batch_ok(b), "swd_patches: b must be in [1, %d] (got %lld)", GS_SWD_MAX_BATCH, (long long)b);
    GS_CHECK_ARG(h >= 7 && w >= 7 && h <= GS_SWD_MAX_SIDE && w <= GS_SWD_MAX_SIDE, "swd_patches: a level of %d x %d holds no 7 x 7 patch (or exceeds %d)", h, w,
                 GS_SWD_MAX_SIDE);
    GS_CHECK_ARG(desc_rows >= 1 && desc_rows <= GS_SWD_MAX_N, "swd_patches: desc_rows must be in [1, %d] (got %lld)", GS_SWD_MAX_N, (long long)desc_rows);
    GS_CHECK_ARG(row_offset >= 0 && row_offset + b * SW_PP <= desc_rows, "swd_patches: rows [%lld, %lld) do not lie inside desc_rows %lld", (long long)row_offset,
                 (long long)(row_offset + b * SW_PP), (long long)desc_rows);
    GS_CHECK_ARG(level && ys && xs && desc, "swd_patches: null pointer (level, ys, xs and desc are required)");
    GS_CHECK_ARG(aligned(level, 4) && aligned(ys, 4) && aligned(xs, 4) && aligned(desc, 4), "swd_patches: misaligned pointer (4 bytes)");
    hipLaunchKernelGGL(swd_patches_kernel, dim3(sw_grid(b * SW_PP * SW_D)), dim3(SW_NT), 0, as_stream(stream), level, (long)b, h, w, ys, xs, desc, (long)row_offset);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_swd_moments(const float* desc, int64_t rows, double* out, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(rows >= 1 && rows <= GS_SWD_MAX_N, "swd_moments: rows must be in [1, %d] (got %lld)", GS_SWD_MAX_N, (long long)rows);
    GS_CHECK_ARG(desc && out, "swd_moments: null pointer (desc and out are required)");
    GS_CHECK_ARG(aligned(desc, 4) && aligned(out, 8), "swd_moments: misaligned pointer (out: 8 bytes, desc: 4)");
    SW_CHECK_WS("swd_moments", sw_ws_bytes(GS_SWD_STAGE_MOMENTS, rows, 0, 0));
    hipStream_t st = as_stream(stream);
    const long count = (long)rows * SW_D;
    const int blocks = sw_blocks(count);
    const long share = (count + blocks - 1) / blocks;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(swd_moments_kernel, dim3(blocks), dim3(SW_NT), 0, st, desc, count, share, part);
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(SW_NT), 0, st, static_cast<const double*>(part), blocks, 4, (long)rows * 49, out);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_swd_project(const float* desc, int64_t n, const double* moments, const float* dirs, int ndir, float* out, void* stream) {
    GS_CHECK_ARG(n >= 1 && n <= GS_SWD_MAX_N, "swd_project: n must be in [1, %d] (got %lld)", GS_SWD_MAX_N, (long long)n);
    GS_CHECK_ARG(ndir >= 1 && ndir <= GS_SWD_MAX_ROWS, "swd_project: ndir must be in [1, %d] (got %d)", GS_SWD_MAX_ROWS, ndir);
    GS_CHECK_ARG(desc && moments && dirs && out, "swd_project: null pointer (desc, moments, dirs and out are required)");
    GS_CHECK_ARG(aligned(desc, 4) && aligned(moments, 8) && aligned(dirs, 4) && aligned(out, 4), "swd_project: misaligned pointer (moments: 8 bytes, the others: 4)");
    hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)((n + PJ_ROWS - 1) / PJ_ROWS)), dim3(SW_NT), 0, as_stream(stream), desc, (long)n, moments, dirs, ndir, out);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_swd_sort(float* data, int64_t rows, int64_t n, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(rows >= 1 && rows <= GS_SWD_MAX_ROWS, "swd_sort: rows must be in [1, %d] (got %lld)", GS_SWD_MAX_ROWS, (long long)rows);
    GS_CHECK_ARG(n >= 1 && n <= GS_SWD_MAX_N, "swd_sort: n must be in [1, %d] (got %lld)", GS_SWD_MAX_N, (long long)n);
    GS_CHECK_ARG(data, "swd_sort: null pointer (data is required)");
    GS_CHECK_ARG(aligned(data, 4), "swd_sort: misaligned pointer (4 bytes)");
    SW_CHECK_WS("swd_sort", sw_ws_bytes(GS_SWD_STAGE_SORT, rows, n, 0));
    hipStream_t st = as_stream(stream);
    int passes = 0;
    for (long run = SW_TILE; run < n; run *= 2) ++passes;
    float* other = static_cast<float*>(ws);
    float* cur = (passes & 1) ? other : data;   // an odd number of passes starts in the workspace: the last pass writes data
    const dim3 tiles((unsigned)((n + SW_TILE - 1) / SW_TILE), (unsigned)rows), chunks((unsigned)((n + SW_MC - 1) / SW_MC), (unsigned)rows);
    hipLaunchKernelGGL(swd_sort_tile_kernel, tiles, dim3(SW_NT), 0, st, static_cast<const float*>(data), cur, (long)n);
    for (long run = SW_TILE; run < n; run *= 2) {
        float* dst = cur == data ? other : data;
        hipLaunchKernelGGL(swd_merge_kernel, chunks, dim3(SW_NT), 0, st, static_cast<const float*>(cur), dst, (long)n, run);
        cur = dst;
    }
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_swd_l1(const float* a, const float* b, int64_t rows, int64_t n, double* out, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(rows >= 1 && rows <= GS_SWD_MAX_ROWS, "swd_l1: rows must be in [1, %d] (got %lld)", GS_SWD_MAX_ROWS, (long long)rows);
    GS_CHECK_ARG(n >= 1 && n <= GS_SWD_MAX_N, "swd_l1: n must be in [1, %d] (got %lld)", GS_SWD_MAX_N, (long long)n);
    GS_CHECK_ARG(a && b && out, "swd_l1: null pointer (a, b and out are required)");
    GS_CHECK_ARG(aligned(a, 4) && aligned(b, 4) && aligned(out, 8), "swd_l1: misaligned pointer (out: 8 bytes, the others: 4)");
    SW_CHECK_WS("swd_l1", sw_ws_bytes(GS_SWD_STAGE_L1, rows, n, 0));
    hipStream_t st = as_stream(stream);
    const long count = (long)rows * n;
    const int blocks = sw_blocks(count);
    const long share = (count + blocks - 1) / blocks;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(swd_l1_kernel, dim3(blocks), dim3(SW_NT), 0, st, a, b, count, share, part);
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(SW_NT), 0, st, static_cast<const double*>(part), blocks, 1, 0L, out);
    GS_CHECK_LAUNCH();
    return 0;
}
