// k-means for the NDB metric (gansynth_amd/kmeans.py, metrics.num_different_bins_device; the rules are this project's own and are stated in
// include/gansynth_hip.h and DESIGN.md "NDB on the device").  fp32, fixed-order sums, no float atomics: two calls agree bit for bit.
//
// Assign is 3 n k d flops on 4 n d bytes: the fp32 vector pipe binds.  The distance is sum (x - c)^2, a subtraction and an FMA per term -- never
// the expansion |x|^2 - 2 x.c + |c|^2, which cancels on features with a common offset.
//   * The all-pairs tile is pairs_tile.h's (staging, LDS layout, the chain), in its scalar form: a block of four waves owns KM_TILE = 256 rows,
//     a wave KG <= 16 consecutive centres (k = 50: 13 each), a lane KM_P = 4 rows against them: 4 KG accumulators, each ONE chain over the
//     columns ascending.
//   * k > 4 KG: rounds of 4 KG centres, the rows staged again every round (from the cache); the running (best, index) stays in registers.
//   * The four waves' candidates meet in LDS and are folded in centre order with a strict <: ties go to the lowest index.
//   kmeans_assign_kernel<KG>    grid (tiles): labels, dist, and the tile's moved-label count and sum of minima (double, a fixed tree)
//   kmeans_assign_fold_kernel   grid (1): the tiles' partials in tile order
// The inertia of given labels in double (gs_kmeans_inertia: what chooses between runs) is one read of x:
//   kmeans_inertia_kernel       grid (tiles): every row's distance to its label's centre, terms and sums in double; then the same fold
// Update is one read of x: HBM binds.
//   kmeans_update_slab_kernel   grid (slices, ceil(d / 64)), one wave: a lane owns a column and adds the slice's rows, in order, into its own
//                               column of a [k, 64] LDS slab (no conflicts; the label is wave-uniform, in a scalar register); 16 rows in flight
//   kmeans_update_fold_kernel   grid (ceil(d / 256), k): the slabs in slice order, the counts, the division
//   kmeans_mindist_kernel       a wave per row, the lanes' partial sums joined by the fixed butterfly of wave_sum
#include <math.h>

#include "gs_common.h"
#include "pairs_tile.h"

namespace gs {

constexpr int KM_NT = PT_NT, KM_WAVES = PT_WAVES, KM_P = PT_P, KM_TILE = PT_TILE;   // assign's tile; the other kernels here take its block shape
constexpr int KM_MAX_KG = 16;              // centres a wave owns, at most
constexpr int KU_COLS = 64;                // columns a block of update owns
constexpr int KU_ROWS = 16;                // rows in flight per wave of update
static_assert(KM_TILE == GS_KMEANS_TILE && KM_TILE == KM_NT, "one thread per row in the epilogue");
static_assert(KM_TILE * PT_XS >= 2 * KM_WAVES * KM_TILE + 3 * KM_TILE, "the epilogue's arrays live in xs");

// grid (tiles of n).  labels / dist of the tile's rows; block_inertia[b] / block_changed[b] its sum of minima (in double) and count of moved labels
template <int KG>
__global__ __launch_bounds__(KM_NT) void kmeans_assign_kernel(const float* __restrict__ x, size_t ldx, long n, int d, const float* __restrict__ centres, int k,
                                                              int* __restrict__ labels, float* __restrict__ dist, int count_moved,
                                                              double* __restrict__ block_inertia, int* __restrict__ block_changed) {
    __shared__ __attribute__((aligned(16))) float xs[KM_TILE * PT_XS];
    __shared__ __attribute__((aligned(16))) float cs[KM_WAVES * KG * PT_DC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tile_begin = (long)blockIdx.x * KM_TILE;
    float best[KM_P];
    int best_k[KM_P];
#pragma unroll
    for (int p = 0; p < KM_P; ++p) { best[p] = INFINITY; best_k[p] = 0; }

    const int rounds = (k + KM_WAVES * KG - 1) / (KM_WAVES * KG);
    for (int r = 0; r < rounds; ++r) {
        const int round_k = r * KM_WAVES * KG;   // the round's first centre
        const int kb = round_k + wave * KG;      // the wave's first centre
        pairs_acc<KG, false> acc;
#pragma unroll
        for (int p = 0; p < KM_P; ++p)
#pragma unroll
            for (int j = 0; j < KG; ++j) acc[p][j] = 0.f;
        for (int d0 = 0; d0 < d; d0 += PT_DC) {
            pairs_stage<KM_WAVES * KG>(xs, cs, x, ldx, tile_begin, n, centres, (size_t)d, round_k, k, d0, d);
            if (kb < k) pairs_chain<KG, false>(xs, cs + wave * KG * PT_DC, lane, acc);   // (wave-uniform)
        }
#pragma unroll
        for (int j = 0; j < KG; ++j)
            if (kb + j < k) {
#pragma unroll
                for (int p = 0; p < KM_P; ++p)
                    if (acc[p][j] < best[p]) { best[p] = acc[p][j]; best_k[p] = kb + j; }   // ascending centres, strict <: the lowest index on ties
            }
    }

    __syncthreads();   // xs is free: the waves' candidates, then the block's sums
    float* cand = xs;                                                     // [KM_WAVES][KM_TILE]
    int* cand_k = reinterpret_cast<int*>(xs + KM_WAVES * KM_TILE);        // [KM_WAVES][KM_TILE]
    double* sum = reinterpret_cast<double*>(xs + 2 * KM_WAVES * KM_TILE); // [KM_TILE] (8-byte aligned: an even number of floats in front)
    int* moved = reinterpret_cast<int*>(xs + 2 * KM_WAVES * KM_TILE + 2 * KM_TILE);   // [KM_TILE]
#pragma unroll
    for (int p = 0; p < KM_P; ++p) {
        cand[wave * KM_TILE + lane + 64 * p] = best[p];
        cand_k[wave * KM_TILE + lane + 64 * p] = best_k[p];
    }
    __syncthreads();
    const int t = threadIdx.x;   // the thread's row of the tile
    float b = cand[t];
    int bk = cand_k[t];
#pragma unroll
    for (int w = 1; w < KM_WAVES; ++w)   // a wave's centres lie below the next wave's in every round; across rounds the index decides
        if (cand[w * KM_TILE + t] < b || (cand[w * KM_TILE + t] == b && cand_k[w * KM_TILE + t] < bk)) { b = cand[w * KM_TILE + t]; bk = cand_k[w * KM_TILE + t]; }
    const long gi = tile_begin + t;
    int mv = 0;
    if (gi < n) {
        if (count_moved) mv = labels[gi] != bk;
        labels[gi] = bk;
        if (dist != nullptr) dist[gi] = b;
    }
    sum[t] = gi < n ? (double)b : 0.0;
    moved[t] = mv;
    for (int s = KM_TILE / 2; s > 0; s >>= 1) {   // a fixed tree
        __syncthreads();
        if (t < s) { sum[t] += sum[t + s]; moved[t] += moved[t + s]; }
    }
    if (t == 0) { block_inertia[blockIdx.x] = sum[0]; block_changed[blockIdx.x] = moved[0]; }
}

// v[lane] + v[lane ^ ...] over the 64 lanes in double: the moves of wave_sum on both halves of the value (the sum of a pair is the same
// number in both of its lanes, so every lane ends with the same bits)
template <int CTRL> __device__ inline double dpp_add_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return v + __hiloint2double(hi, lo);
}
__device__ inline double wave_sum_f64(double v) {
    v = dpp_add_f64<0xB1>(v);
    v = dpp_add_f64<0x4E>(v);
    v = dpp_add_f64<0x141>(v);
    v = dpp_add_f64<0x140>(v);
    float alo, blo, ahi, bhi;
    swap16_pair(__int_as_float(__double2loint(v)), alo, blo);
    swap16_pair(__int_as_float(__double2hiint(v)), ahi, bhi);
    v = __hiloint2double(__float_as_int(ahi), __float_as_int(alo)) + __hiloint2double(__float_as_int(bhi), __float_as_int(blo));
    swap32_pair(__int_as_float(__double2loint(v)), alo, blo);
    swap32_pair(__int_as_float(__double2hiint(v)), ahi, bhi);
    return __hiloint2double(__float_as_int(ahi), __float_as_int(alo)) + __hiloint2double(__float_as_int(bhi), __float_as_int(blo));
}

// gs_kmeans_inertia.  grid (tiles of n).  block_inertia[b] = the sum over the tile's rows of |x_i - centres[labels[i]]|^2, every term and every
// sum in double: the figure that decides between runs that end within fp32 rounding of each other carries none of its own.  A wave takes 64 rows one after the
// other (a row and its centre are read along the columns: coalesced), a lane its columns ascending, the lanes join in wave_sum_f64's fixed
// butterfly, the rows and then the four waves add up in order.
__global__ __launch_bounds__(KM_NT) void kmeans_inertia_kernel(const float* __restrict__ x, size_t ldx, long n, int d, const float* __restrict__ centres, int k,
                                                               const int* __restrict__ labels, double* __restrict__ block_inertia) {
    __shared__ double part[KM_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long first = (long)blockIdx.x * KM_TILE + wave * 64;
    double total = 0.0;
    for (int r = 0; r < 64 && first + r < n; ++r) {
        const int kk = __builtin_amdgcn_readfirstlane(labels[first + r]);
        if (kk < 0 || kk >= k) continue;   // (a label outside [0, k) is no cluster's row: it adds nothing)
        const float* __restrict__ xr = x + (size_t)(first + r) * ldx;
        const float* __restrict__ cr = centres + (size_t)kk * d;
        double s = 0.0;
        for (int c = lane; c < d; c += 64) {
            const double t = (double)xr[c] - (double)cr[c];
            s = fma(t, t, s);
        }
        total += wave_sum_f64(s);
    }
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < KM_WAVES; ++w) sum += part[w];
        block_inertia[blockIdx.x] = sum;
    }
}

// grid (1).  inertia / changed = the tiles' partials, a thread's share in tile order, then a fixed tree
__global__ __launch_bounds__(KM_NT) void kmeans_assign_fold_kernel(const double* __restrict__ block_inertia, const int* __restrict__ block_changed, int tiles,
                                                                   double* __restrict__ inertia, int* __restrict__ changed) {
    __shared__ double sum[KM_NT];
    __shared__ int moved[KM_NT];
    const int t = threadIdx.x;
    double s = 0.0;
    int m = 0;
    for (int i = t; i < tiles; i += KM_NT) {
        if (inertia != nullptr) s += block_inertia[i];
        if (changed != nullptr) m += block_changed[i];
    }
    sum[t] = s;
    moved[t] = m;
    for (int h = KM_NT / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h) { sum[t] += sum[t + h]; moved[t] += moved[t + h]; }
    }
    if (t == 0) {
        if (inertia != nullptr) *inertia = sum[0];
        if (changed != nullptr) *changed = moved[0];
    }
}

// grid (slices, ceil(d / 64)), 64 threads, k * 64 floats of dynamic LDS.  part[slice][kk][col] = the sum of the slice's rows of label kk, in
// row order; cnt_part[slice][kk] their number (written by the blocks of the first columns)
__global__ __launch_bounds__(64) void kmeans_update_slab_kernel(const float* __restrict__ x, size_t ldx, long n, int d, const int* __restrict__ labels, int k,
                                                                long rows_per_slice, float* __restrict__ part, int* __restrict__ cnt_part) {
    extern __shared__ __attribute__((aligned(16))) float slab[];   // [k][KU_COLS]
    const int lane = threadIdx.x;
    const int col = blockIdx.y * KU_COLS + lane;
    const bool col_ok = col < d, counting = blockIdx.y == 0;
    for (int kk = 0; kk < k; ++kk) slab[kk * KU_COLS + lane] = 0.f;
    int cnt[GS_KMEANS_MAX_K / 64] = {0, 0, 0, 0};   // lane l counts the labels l, l + 64, l + 128, l + 192
    const long r0 = (long)blockIdx.x * rows_per_slice;
    const long r1 = r0 + rows_per_slice < n ? r0 + rows_per_slice : n;
    for (long i = r0; i < r1; i += KU_ROWS) {
        float v[KU_ROWS];
        int lab[KU_ROWS];
#pragma unroll
        for (int u = 0; u < KU_ROWS; ++u) {
            const long row = i + u;
            lab[u] = row < r1 ? __builtin_amdgcn_readfirstlane(labels[row]) : -1;
            v[u] = (row < r1 && col_ok) ? x[(size_t)row * ldx + col] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < KU_ROWS; ++u)
            if (lab[u] >= 0 && lab[u] < k) {   // (wave-uniform; a label outside [0, k) is no cluster's row)
                slab[lab[u] * KU_COLS + lane] += v[u];
                if (counting) {
#pragma unroll
                    for (int g = 0; g < GS_KMEANS_MAX_K / 64; ++g) cnt[g] += lab[u] == lane + 64 * g;
                }
            }
    }
    float* out = part + (size_t)blockIdx.x * k * d;
    if (col_ok)
        for (int kk = 0; kk < k; ++kk) out[(size_t)kk * d + col] = slab[kk * KU_COLS + lane];
    if (counting) {
#pragma unroll
        for (int g = 0; g < GS_KMEANS_MAX_K / 64; ++g)
            if (lane + 64 * g < k) cnt_part[(size_t)blockIdx.x * k + lane + 64 * g] = cnt[g];
    }
}

// grid (ceil(d / 256), k).  counts[kk] = sum of cnt_part[.][kk]; with rows: centres[kk][col] = (sum over the slices, ascending) / count
__global__ __launch_bounds__(KM_NT) void kmeans_update_fold_kernel(const float* __restrict__ part, const int* __restrict__ cnt_part, int slices, int d, int k,
                                                                   float* __restrict__ centres, int* __restrict__ counts) {
    __shared__ int total[KM_NT];
    const int t = threadIdx.x, kk = blockIdx.y;
    int m = 0;
    for (int s = t; s < slices; s += KM_NT) m += cnt_part[(size_t)s * k + kk];
    total[t] = m;
    for (int h = KM_NT / 2; h > 0; h >>= 1) {   // (integers: exact in any order)
        __syncthreads();
        if (t < h) total[t] += total[t + h];
    }
    __syncthreads();
    m = total[0];
    if (blockIdx.x == 0 && t == 0) counts[kk] = m;
    const int col = blockIdx.x * KM_NT + t;
    if (m == 0 || col >= d) return;   // an empty cluster keeps its centre
    float s = 0.f;
    for (int sl = 0; sl < slices; ++sl) s += part[((size_t)sl * k + kk) * d + col];
    centres[(size_t)kk * d + col] = s / (float)m;
}

// grid (blocks), a wave per row (grid-stride).  dist[i] = |x_i - centre|^2, or the smaller of it and dist[i]
__global__ __launch_bounds__(KM_NT) void kmeans_mindist_kernel(const float* __restrict__ x, size_t ldx, long n, int d, const float* __restrict__ centre,
                                                               float* __restrict__ dist, int first) {
    const int lane = threadIdx.x & 63;
    for (long row = (long)blockIdx.x * KM_WAVES + (threadIdx.x >> 6); row < n; row += (long)gridDim.x * KM_WAVES) {
        const float* __restrict__ xr = x + (size_t)row * ldx;
        float s = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float t = xr[c] - centre[c];
            s = fmaf(t, t, s);
        }
        s = wave_sum(s);
        if (lane == 0) dist[row] = first ? s : fminf(dist[row], s);
    }
}

static bool km_shape_ok(int64_t n, int d, int k) { return feature_dims_ok(n, d) && k >= 1 && k <= GS_KMEANS_MAX_K; }
static long km_tiles(int64_t n) { return (long)((n + KM_TILE - 1) / KM_TILE); }
static long km_rows_per_slice(int64_t n, int d) {
    long s0 = 2048 / ((d + KU_COLS - 1) / KU_COLS);
    if (s0 > GS_KMEANS_MAX_SLICES) s0 = GS_KMEANS_MAX_SLICES;
    const long by_rows = (long)((n + 63) / 64);
    if (s0 > by_rows) s0 = by_rows;
    if (s0 < 1) s0 = 1;
    return (long)((n + s0 - 1) / s0);
}
static long km_slices(int64_t n, int d) {
    const long rows = km_rows_per_slice(n, d);
    return (long)((n + rows - 1) / rows);
}
static size_t km_ws_bytes(int64_t n, int d, int k) {
    const size_t assign = (size_t)km_tiles(n) * (sizeof(double) + sizeof(int));
    const size_t update = (size_t)km_slices(n, d) * k * ((size_t)d + 1) * sizeof(float);
    return ((assign > update ? assign : update) + 15) & ~(size_t)15;
}
// the centres a wave owns: the listed size that covers k in the fewest rounds with the fewest idle slots
static int km_group(int k) {
    const int groups = (k + KM_MAX_KG - 1) / KM_MAX_KG;                       // wave-rounds at 16 a wave
    const int waves = (groups + KM_WAVES - 1) / KM_WAVES * KM_WAVES;          // ... filled up to whole rounds
    const int need = (k + waves - 1) / waves;
    return need <= 4 ? 4 : need <= 8 ? 8 : need <= 13 ? 13 : 16;
}

}  // namespace gs

using namespace gs;

#define KM_CHECK_ROWS(what)              \
    GS_CHECK_FEATURE_D(what);            \
    GS_CHECK_FEATURE_ROWS(what, "n", n); \
    GS_CHECK_FEATURE_LD(what, "ldx", ldx)
#define KM_CHECK_SHAPE(what)                                                                                  \
    GS_CHECK_ARG(k >= 1 && k <= GS_KMEANS_MAX_K, what ": k must be in [1, %d] (got %d)", GS_KMEANS_MAX_K, k); \
    KM_CHECK_ROWS(what)

extern "C" size_t gs_kmeans_workspace_bytes(int64_t n, int d, int k) {
    if (!km_shape_ok(n, d, k)) return 0;
    return km_ws_bytes(n, d, k);
}

extern "C" int gs_kmeans_assign(const float* x, int64_t ldx, int64_t n, int d, const float* centres, int k, int32_t* labels, float* dist, int32_t* changed,
                                double* inertia, void* ws, size_t ws_bytes, void* stream) {
    KM_CHECK_SHAPE("kmeans_assign");
    GS_CHECK_ARG(x && centres && labels, "kmeans_assign: null pointer (x, centres and labels are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(centres, 4) && aligned(labels, 4) && aligned(dist, 4) && aligned(changed, 4) && aligned(inertia, 8),
                 "kmeans_assign: misaligned pointer (inertia: 8 bytes, the others: 4)");
    const size_t need = km_ws_bytes(n, d, k);
    GS_CHECK_ARG(ws && ws_bytes >= need && aligned(ws, 16), "kmeans_assign: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int tiles = (int)km_tiles(n);
    double* block_inertia = static_cast<double*>(ws);
    int* block_changed = reinterpret_cast<int*>(block_inertia + tiles);
    with_constant<4, 8, 13, 16>(km_group(k), [&](auto kg) {
        hipLaunchKernelGGL((kmeans_assign_kernel<decltype(kg)::value>), dim3((unsigned)tiles), dim3(KM_NT), 0, st, x, (size_t)ldx, (long)n, d, centres, k, labels,
                           dist, changed != nullptr ? 1 : 0, block_inertia, block_changed);
        return true;
    });
    if (changed != nullptr || inertia != nullptr)
        hipLaunchKernelGGL(kmeans_assign_fold_kernel, dim3(1), dim3(KM_NT), 0, st, static_cast<const double*>(block_inertia),
                           static_cast<const int*>(block_changed), tiles, inertia, changed);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_kmeans_inertia(const float* x, int64_t ldx, int64_t n, int d, const float* centres, int k, const int32_t* labels, double* inertia, void* ws,
                                 size_t ws_bytes, void* stream) {
    KM_CHECK_SHAPE("kmeans_inertia");
    GS_CHECK_ARG(x && centres && labels && inertia, "kmeans_inertia: null pointer (x, centres, labels and inertia are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(centres, 4) && aligned(labels, 4) && aligned(inertia, 8),
                 "kmeans_inertia: misaligned pointer (inertia: 8 bytes, the others: 4)");
    const size_t need = km_ws_bytes(n, d, k);
    GS_CHECK_ARG(ws && ws_bytes >= need && aligned(ws, 16), "kmeans_inertia: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int tiles = (int)km_tiles(n);
    double* block_inertia = static_cast<double*>(ws);
    hipLaunchKernelGGL(kmeans_inertia_kernel, dim3((unsigned)tiles), dim3(KM_NT), 0, st, x, (size_t)ldx, (long)n, d, centres, k, labels, block_inertia);
    hipLaunchKernelGGL(kmeans_assign_fold_kernel, dim3(1), dim3(KM_NT), 0, st, static_cast<const double*>(block_inertia), static_cast<const int*>(nullptr), tiles,
                       inertia, static_cast<int*>(nullptr));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_kmeans_update(const float* x, int64_t ldx, int64_t n, int d, const int32_t* labels, int k, float* centres, int32_t* counts, void* ws,
                                size_t ws_bytes, void* stream) {
    KM_CHECK_SHAPE("kmeans_update");
    GS_CHECK_ARG(x && labels && centres && counts, "kmeans_update: null pointer (x, labels, centres and counts are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(labels, 4) && aligned(centres, 4) && aligned(counts, 4), "kmeans_update: misaligned pointer (4 bytes)");
    const size_t need = km_ws_bytes(n, d, k);
    GS_CHECK_ARG(ws && ws_bytes >= need && aligned(ws, 16), "kmeans_update: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const long rows = km_rows_per_slice(n, d);
    const int slices = (int)km_slices(n, d);
    float* part = static_cast<float*>(ws);
    int* cnt_part = reinterpret_cast<int*>(part + (size_t)slices * k * d);
    hipLaunchKernelGGL(kmeans_update_slab_kernel, dim3((unsigned)slices, (unsigned)((d + KU_COLS - 1) / KU_COLS)), dim3(64), (size_t)k * KU_COLS * sizeof(float),
                       st, x, (size_t)ldx, (long)n, d, labels, k, rows, part, cnt_part);
    hipLaunchKernelGGL(kmeans_update_fold_kernel, dim3((unsigned)((d + KM_NT - 1) / KM_NT), (unsigned)k), dim3(KM_NT), 0, st, static_cast<const float*>(part),
                       static_cast<const int*>(cnt_part), slices, d, k, centres, counts);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_kmeans_mindist(const float* x, int64_t ldx, int64_t n, int d, const float* centre, float* dist, int first, void* stream) {
    KM_CHECK_ROWS("kmeans_mindist");
    GS_CHECK_ARG(x && centre && dist, "kmeans_mindist: null pointer (x, centre and dist are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(centre, 4) && aligned(dist, 4), "kmeans_mindist: misaligned pointer (4 bytes)");
    const long blocks = (long)((n + KM_WAVES - 1) / KM_WAVES);
    hipLaunchKernelGGL(kmeans_mindist_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(KM_NT), 0, as_stream(stream), x, (size_t)ldx, (long)n, d, centre,
                       dist, first);
    GS_CHECK_LAUNCH();
    return 0;
}
