// k-nearest-neighbour radii and cover for precision / recall / density / coverage (gansynth_amd/manifold.py, metrics.precision_recall_device; the
// rules are stated in include/gansynth_hip.h and DESIGN.md "Precision and recall on the device").  fp32, no float atomics, and every result a
// multiset of values or an integer sum: two calls agree bit for bit, whatever the slicing.
//
// Both entries are all-pairs squared distances, 3 n m d flops, of which nothing is written: the fp32 vector pipe binds.  The distance is
// pairs_tile.h's, sum (x - y)^2 as ONE chain over the columns ascending -- (x - y)^2 and (y - x)^2 have the same bits, so d(i, j) is one number
// in gs_knn_kth and gs_knn_within and from either side.
//   * The all-pairs tile is pairs_tile.h's (staging, LDS layout, the chain), as in kmeans_assign_kernel: a block of four waves owns KN_TILE = 256
//     rows of the first side; a wave owns KN_KG = 16 consecutive rows of the other side, a lane KN_P = 4 rows of the tile against them: 64
//     accumulators.
//   * Packed fp32 math, the tile's packed form: two rows of a lane sit in one register pair, t = x - y is a v_pk_add_f32 and the chain a
//     v_pk_fma_f32 -- 7 to 10 % faster than v_sub_f32 / v_fmac_f32 at 50 000 rows (DESIGN.md has both numbers).
//   * The grid is (row tiles) x (slices of the other side): a block walks its slice in rounds of 4 KN_KG = 64 rows.  After a round a lane holds
//     64 finished distances.  kth: each goes through ONE compare against the lane's current K-th value for that row and, under it, a sorted
//     insert into K registers (v_med3_f32 per place: fully unrolled, no indexed private array); within: one compare against the other row's
//     radius (wave-uniform: a scalar register) and an integer add.  Per pair that is a handful of instructions beside 2 d of the chain.
//   * The four waves' lists (counts) of a row meet in LDS; the block's list goes to ws as [slice][n][k] (count: [slice][n]), or, with one
//     slice, straight to the output.
//   knn_kernel<K>              grid (tiles, slices).  K >= 1: the K smallest; K == 0: the count within radius2
//   knn_kth_fold_kernel<K>     grid (tiles): a thread a row, the slices' lists through the same insert
//   knn_within_fold_kernel     grid (tiles): a thread a row, the slices' counts added
#include <math.h>

#include "gs_common.h"
#include "pairs_tile.h"

namespace gs {

constexpr int KN_NT = PT_NT, KN_WAVES = PT_WAVES, KN_P = PT_P, KN_TILE = PT_TILE;   // the tile; the folds take its block shape
constexpr int KN_KG = 16;                  // rows of the other side a wave owns per round
constexpr int KN_ROUND = KN_WAVES * KN_KG; // rows of the other side a block takes per round
constexpr int KN_OCC = 3;                  // blocks a CU is asked to hold, a wave of each per SIMD: 168 registers (at 2, kth is 14 % slower at 50 000 rows)
static_assert(KN_TILE == GS_KMEANS_TILE && KN_TILE == KN_NT, "one thread per row in the epilogue");
static_assert(KN_TILE * PT_XS >= KN_WAVES * KN_TILE * GS_KNN_MAX_K, "the epilogue's lists live in xs");
static_assert(GS_KNN_MIN_SLICE_ROWS % KN_ROUND == 0, "a slice is whole rounds");

// t[0] <= ... <= t[K - 1] keeps the K smallest values it has seen: one compare for a value that does not belong, and under it a place-by-place
// median (t[j - 1] <= t[j], so med3(t[j - 1], v, t[j]) is t[j - 1] when v lies below both, v between them, t[j] above).  A value equal to the
// K-th is not taken: the multiset is the same.  NaN is never taken.
template <int K> __device__ inline void topk_insert(float (&t)[K], float v) {
    if (v < t[K - 1]) {
#pragma unroll
        for (int j = K - 1; j > 0; --j) t[j] = __builtin_amdgcn_fmed3f(t[j - 1], v, t[j]);
        t[0] = v < t[0] ? v : t[0];
    }
}

// grid (tiles of n, slices of m).  K >= 1: part[slice][i][0 .. k) = the k smallest |a_i - b_j|^2 over the slice's j (j != i with exclude),
// ascending, +inf where they run out.  K == 0: cnt_part[slice][i] = the number of the slice's j with |a_i - b_j|^2 <= radius2[j].
template <int K>
__global__ __launch_bounds__(KN_NT, KN_OCC) void knn_kernel(const float* __restrict__ a, size_t lda, long n, const float* __restrict__ b, size_t ldb, long m, int d,
                                                    long rows_per_slice, int k, int exclude, const float* __restrict__ radius2, float* __restrict__ part,
                                                    int* __restrict__ cnt_part) {
    __shared__ __attribute__((aligned(16))) float xs[KN_TILE * PT_XS];
    __shared__ __attribute__((aligned(16))) float cs[KN_ROUND * PT_DC];
    constexpr int KK = K > 0 ? K : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tile_begin = (long)blockIdx.x * KN_TILE;
    const long m0 = (long)blockIdx.y * rows_per_slice;
    const long m1 = m0 + rows_per_slice < m ? m0 + rows_per_slice : m;
    float top[KN_P][KK];
    int cnt[KN_P];
#pragma unroll
    for (int p = 0; p < KN_P; ++p) {
        cnt[p] = 0;
#pragma unroll
        for (int e = 0; e < KK; ++e) top[p][e] = INFINITY;
    }

    for (long round_b = m0; round_b < m1; round_b += KN_ROUND) {
        const long kb = round_b + wave * KN_KG;   // the wave's first row of b
        pairs_acc<KN_KG, true> acc;   // rows (2 pp, 2 pp + 1) of the lane side by side, each half its own chain
#define KN_ACC(p, j) acc[(p) / 2][j][(p) & 1]
#pragma unroll
        for (int p = 0; p < KN_P; ++p)
#pragma unroll
            for (int j = 0; j < KN_KG; ++j) KN_ACC(p, j) = 0.f;
        for (int d0 = 0; d0 < d; d0 += PT_DC) {
            pairs_stage<KN_ROUND>(xs, cs, a, lda, tile_begin, n, b, ldb, round_b, m1, d0, d);
            if (kb < m1) pairs_chain<KN_KG, true>(xs, cs + wave * KN_KG * PT_DC, lane, acc);   // (wave-uniform)
        }
#pragma unroll
        for (int j = 0; j < KN_KG; ++j)
            if (kb + j < m1) {   // (wave-uniform)
                if constexpr (K > 0) {
#pragma unroll
                    for (int p = 0; p < KN_P; ++p) {
                        const bool self = exclude && kb + j == tile_begin + lane + 64 * p;
                        topk_insert<KK>(top[p], self ? INFINITY : KN_ACC(p, j));
                    }
                } else {
                    const float r = radius2[kb + j];
#pragma unroll
                    for (int p = 0; p < KN_P; ++p) cnt[p] += KN_ACC(p, j) <= r ? 1 : 0;
                }
            }
    }

    __syncthreads();   // xs is free: the four waves' lists (counts) of every row
    const int t = threadIdx.x;   // the thread's row of the tile
    const long gi = tile_begin + t;
    if constexpr (K > 0) {
        float* cand = xs;   // [KN_WAVES][KN_TILE][K]
#pragma unroll
        for (int p = 0; p < KN_P; ++p)
#pragma unroll
            for (int e = 0; e < KK; ++e) cand[(wave * KN_TILE + lane + 64 * p) * KK + e] = top[p][e];
        __syncthreads();
        float best[KK];
#pragma unroll
        for (int e = 0; e < KK; ++e) best[e] = cand[t * KK + e];
#pragma unroll
        for (int w = 1; w < KN_WAVES; ++w)
#pragma unroll
            for (int e = 0; e < KK; ++e) topk_insert<KK>(best, cand[(w * KN_TILE + t) * KK + e]);
        if (gi < n) {
            float* out = part + ((size_t)blockIdx.y * n + gi) * k;
#pragma unroll
            for (int e = 0; e < KK; ++e)
                if (e < k) out[e] = best[e];
        }
    } else {
        int* cand = reinterpret_cast<int*>(xs);   // [KN_WAVES][KN_TILE]
#pragma unroll
        for (int p = 0; p < KN_P; ++p) cand[wave * KN_TILE + lane + 64 * p] = cnt[p];
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int w = 0; w < KN_WAVES; ++w) total += cand[w * KN_TILE + t];
        if (gi < n) cnt_part[(size_t)blockIdx.y * n + gi] = total;
    }
}

// grid (tiles of n).  out[i][0 .. k) = the k smallest of part[0 .. slices)[i][0 .. k)
template <int K>
__global__ __launch_bounds__(KN_NT) void knn_kth_fold_kernel(const float* __restrict__ part, int slices, long n, int k, float* __restrict__ out) {
    const long i = (long)blockIdx.x * KN_NT + threadIdx.x;
    if (i >= n) return;
    float best[K];
#pragma unroll
    for (int e = 0; e < K; ++e) best[e] = INFINITY;
    for (int s = 0; s < slices; ++s) {
        const float* __restrict__ row = part + ((size_t)s * n + i) * k;
#pragma unroll
        for (int e = 0; e < K; ++e)
            if (e < k) topk_insert<K>(best, row[e]);
    }
#pragma unroll
    for (int e = 0; e < K; ++e)
        if (e < k) out[(size_t)i * k + e] = best[e];
}

// grid (tiles of n).  count[i] = the sum of cnt_part[0 .. slices)[i]
__global__ __launch_bounds__(KN_NT) void knn_within_fold_kernel(const int* __restrict__ cnt_part, int slices, long n, int* __restrict__ count) {
    const long i = (long)blockIdx.x * KN_NT + threadIdx.x;
    if (i >= n) return;
    int total = 0;
    for (int s = 0; s < slices; ++s) total += cnt_part[(size_t)s * n + i];
    count[i] = total;
}

static bool kn_shape_ok(int64_t n, int64_t m, int d, int k) {
    return feature_dims_ok(n, d) && feature_dims_ok(m, d) && k >= 1 && k <= GS_KNN_MAX_K;
}
static long kn_tiles(int64_t n) { return (long)((n + KN_TILE - 1) / KN_TILE); }
// the rows of the other side a block walks: whole rounds, at least GS_KNN_MIN_SLICE_ROWS, and few enough for GS_KNN_BLOCKS blocks where m allows
static long kn_rows_per_slice(int64_t n, int64_t m) {
    const long tiles = kn_tiles(n);
    const long want = (GS_KNN_BLOCKS + tiles - 1) / tiles;
    long rows = (long)((m + want - 1) / want);
    rows = (rows + KN_ROUND - 1) / KN_ROUND * KN_ROUND;
    return rows < GS_KNN_MIN_SLICE_ROWS ? GS_KNN_MIN_SLICE_ROWS : rows;
}
static int kn_slices(int64_t n, int64_t m) {
    const long rows = kn_rows_per_slice(n, m);
    return (int)((m + rows - 1) / rows);
}
static size_t kn_ws_bytes(int64_t n, int64_t m, int k) {
    const int slices = kn_slices(n, m);
    if (slices == 1) return 16;
    return ((size_t)slices * (size_t)n * k * sizeof(float) + 15) & ~(size_t)15;
}

}  // namespace gs

using namespace gs;

#define KN_CHECK_SHAPE(what, lda, ldb, sa, sb) \
    GS_CHECK_FEATURE_D(what);                  \
    GS_CHECK_FEATURE_ROWS(what, "n", n);       \
    GS_CHECK_FEATURE_ROWS(what, "m", m);       \
    GS_CHECK_FEATURE_LD(what, sa, lda);        \
    GS_CHECK_FEATURE_LD(what, sb, ldb)

extern "C" int gs_knn_slices(int64_t n, int64_t m, int d) {
    if (!kn_shape_ok(n, m, d, 1)) return 0;
    return kn_slices(n, m);
}

extern "C" size_t gs_knn_workspace_bytes(int64_t n, int64_t m, int d, int k) {
    if (!kn_shape_ok(n, m, d, k)) return 0;
    return kn_ws_bytes(n, m, k);
}

extern "C" int gs_knn_kth(const float* a, int64_t lda, int64_t n, const float* b, int64_t ldb, int64_t m, int d, int k, int exclude_diagonal, float* out,
                          void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(k >= 1 && k <= GS_KNN_MAX_K, "knn_kth: k must be in [1, %d] (got %d)", GS_KNN_MAX_K, k);
    KN_CHECK_SHAPE("knn_kth", lda, ldb, "lda", "ldb");
    GS_CHECK_ARG(a && b && out, "knn_kth: null pointer (a, b and out are required)");
    GS_CHECK_ARG(aligned(a, 4) && aligned(b, 4) && aligned(out, 4), "knn_kth: misaligned pointer (a, b and out: 4 bytes)");
    const size_t need = kn_ws_bytes(n, m, k);
    GS_CHECK_ARG(ws && ws_bytes >= need && aligned(ws, 16), "knn_kth: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const unsigned tiles = (unsigned)kn_tiles(n);
    const long rows = kn_rows_per_slice(n, m);
    const int slices = kn_slices(n, m);
    float* part = slices == 1 ? out : static_cast<float*>(ws);
    with_constant<1, 3, 5, 8>(k <= 1 ? 1 : k <= 3 ? 3 : k <= 5 ? 5 : 8, [&](auto kk) {
        constexpr int K = decltype(kk)::value;
        hipLaunchKernelGGL((knn_kernel<K>), dim3(tiles, (unsigned)slices), dim3(KN_NT), 0, st, a, (size_t)lda, (long)n, b, (size_t)ldb, (long)m, d, rows, k,
                           exclude_diagonal != 0 ? 1 : 0, static_cast<const float*>(nullptr), part, static_cast<int*>(nullptr));
        if (slices > 1)
            hipLaunchKernelGGL((knn_kth_fold_kernel<K>), dim3(tiles), dim3(KN_NT), 0, st, static_cast<const float*>(part), slices, (long)n, k, out);
        return true;
    });
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_knn_within(const float* q, int64_t ldq, int64_t n, const float* ref, int64_t ldr, int64_t m, int d, const float* radius2, int32_t* count,
                             void* ws, size_t ws_bytes, void* stream) {
    KN_CHECK_SHAPE("knn_within", ldq, ldr, "ldq", "ldr");
    GS_CHECK_ARG(q && ref && radius2 && count, "knn_within: null pointer (q, ref, radius2 and count are required)");
    GS_CHECK_ARG(aligned(q, 4) && aligned(ref, 4) && aligned(radius2, 4) && aligned(count, 4),
                 "knn_within: misaligned pointer (q, ref, radius2 and count: 4 bytes)");
    const size_t need = kn_ws_bytes(n, m, 1);
    GS_CHECK_ARG(ws && ws_bytes >= need && aligned(ws, 16), "knn_within: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const unsigned tiles = (unsigned)kn_tiles(n);
    const long rows = kn_rows_per_slice(n, m);
    const int slices = kn_slices(n, m);
    int* cnt_part = slices == 1 ? count : static_cast<int*>(ws);
    hipLaunchKernelGGL((knn_kernel<0>), dim3(tiles, (unsigned)slices), dim3(KN_NT), 0, st, q, (size_t)ldq, (long)n, ref, (size_t)ldr, (long)m, d, rows, 1, 0, radius2,
                       static_cast<float*>(nullptr), cnt_part);
    if (slices > 1) hipLaunchKernelGGL(knn_within_fold_kernel, dim3(tiles), dim3(KN_NT), 0, st, static_cast<const int*>(cnt_part), slices, (long)n, count);
    GS_CHECK_LAUNCH();
    return 0;
}
