// The three kernel sums of the kernel inception distance (gansynth_amd/kid.py, metrics.kernel_inception_distance_device; the rules are stated in
// include/gansynth_hip.h and DESIGN.md "KID on the device"): all pairs of rows through k(a, b) = (a.b / d + 1)^3, summed in fp64, nothing but
// one double a block ever written.  The library's only fp64 matrix-core kernel: a sum of up to 2.5e9 terms whose three means agree to three or
// four digits is no place for fp32, and a product of two fp32 features is exact in fp64.
//
//   kid_kernel       grid (tiles of a subset, subsets), four waves.  A block owns KD_TILE x KD_TILE = 128 x 128 pairs of one of the three jobs
//                    (x against x, y against y, x against y) of one subset, a wave 64 x 64 of them as 4 x 4 tiles of v_mfma_f64_16x16x4_f64:
//                    64 doubles of accumulator a lane.  The columns are walked in chunks of KD_DC = 32; a chunk of both sides is staged in LDS
//                    as fp32 (half the bytes; the widening is exact and happens at the fragment read), rows KD_LD = 36 floats apart: the 64
//                    lanes of a fragment read (16 rows x 4 columns) fall on 64 distinct banks.  The next chunk's global loads are issued before
//                    the current chunk's MFMAs and wait in registers.  A row is found through the subset's index list by the loader (the row
//                    numbers of a tile sit in LDS): no gathered copy exists.
//                    Columns past d are zero in LDS (the load itself is clamped to column d - 1: nothing past a row's d floats is read), rows
//                    past the end repeat the last row and are masked in the epilogue.
//                    The symmetric jobs visit the tiles with tile_col >= tile_row only: an off-diagonal tile counts twice (an exact doubling of
//                    the block's double), a diagonal tile holds (i, j) and (j, i) both and drops i == j.
//                    Epilogue: t = p / d + 1, k = t t t in registers, the lane's 64 values added in one fixed chain, the block's 256 lanes in a
//                    fixed tree in LDS, one double to ws[subset][tile].
//   kid_fold_kernel  grid (3, subsets): thread t adds the job's partials t, t + 256, ... in ascending order, the 256 threads in the same tree.
//
// The MFMA's fp64 result map is NOT the fp32 one: a lane's register r holds row (lane >> 4) + 4 r, column lane & 15 of the 16 x 16 tile.
// Every sum has one fixed order whatever the grid: two calls write the same bits, and a subset's sums do not depend on the batch it is in (the
// tiling is a function of `size` alone).
#include "gs_common.h"

namespace gs {

constexpr int KD_NT = 256;                     // threads per block
constexpr int KD_TILE = GS_KID_TILE;           // pairs a block owns: KD_TILE x KD_TILE
constexpr int KD_WT = KD_TILE / 2;             // a wave's share: KD_WT x KD_WT, the waves 2 x 2
constexpr int KD_F = KD_WT / 16;               // MFMA tiles a wave holds each way
constexpr int KD_DC = 32;                      // columns per chunk
constexpr int KD_LD = KD_DC + 4;               // floats between two rows in LDS
constexpr int KD_SR = KD_NT / KD_DC;           // rows a staging pass covers
constexpr int KD_SL = KD_TILE / KD_SR;         // staging loads a thread and side
static_assert(KD_NT == 2 * KD_TILE, "one thread per row of either side fills the row table");
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct KidShape {
    long rows_x, rows_y;    // rows a job's side has: n and m, or `size` with subsets
    long tx, ty;            // tiles a side
    long txx, tyy, txy;     // tiles a job: tx (tx + 1) / 2, ty (ty + 1) / 2, tx ty
    long per_subset;        // txx + tyy + txy
};

__host__ __device__ inline KidShape kid_shape(long n, long m, int subsets, long size) {
    KidShape s;
    s.rows_x = subsets > 0 ? size : n;
    s.rows_y = subsets > 0 ? size : m;
    s.tx = (s.rows_x + KD_TILE - 1) / KD_TILE;
    s.ty = (s.rows_y + KD_TILE - 1) / KD_TILE;
    s.txx = s.tx * (s.tx + 1) / 2;
    s.tyy = s.ty * (s.ty + 1) / 2;
    s.txy = s.tx * s.ty;
    s.per_subset = s.txx + s.tyy + s.txy;
    return s;
}

// idx in [0, T (T + 1) / 2) -> (row, col) with col >= row, the upper triangle row by row: row r begins at r T - r (r - 1) / 2
__device__ inline void kid_triangle(long idx, long T, long& row, long& col) {
    const double b = 2.0 * (double)T + 1.0;
    long r = (long)((b - sqrt(b * b - 8.0 * (double)idx)) * 0.5);
    r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
    while (r + 1 < T && (r + 1) * T - (r + 1) * r / 2 <= idx) ++r;   // (the square root may be one off either way)
    while (r > 0 && r * T - r * (r - 1) / 2 > idx) --r;
    row = r;
    col = r + (idx - (r * T - r * (r - 1) / 2));
}

__global__ __launch_bounds__(KD_NT, 2) void kid_kernel(const float* __restrict__ x, size_t ldx, long n, const float* __restrict__ y, size_t ldy, long m, int d,
                                                       const int* __restrict__ xi, const int* __restrict__ yi, int subsets, long size, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float as[KD_TILE * KD_LD];
    __shared__ __attribute__((aligned(16))) float bs[KD_TILE * KD_LD];
    __shared__ int rows_lds[2 * KD_TILE];   // the rows of the two sides' tiles in their matrices
    __shared__ double red[KD_NT];
    const KidShape sh = kid_shape(n, m, subsets, size);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long sub = blockIdx.y;

    // the block's job and tile (block-uniform)
    long tile = blockIdx.x, tr, tc;
    int job;   // 0: x against x, 1: y against y, 2: x against y
    if (tile < sh.txx) {
        job = 0;
        kid_triangle(tile, sh.tx, tr, tc);
    } else if (tile < sh.txx + sh.tyy) {
        job = 1;
        kid_triangle(tile - sh.txx, sh.ty, tr, tc);
    } else {
        job = 2;
        tile -= sh.txx + sh.tyy;
        tr = tile / sh.ty;
        tc = tile % sh.ty;
    }
    const float* __restrict__ pa = job == 1 ? y : x;
    const float* __restrict__ pb = job == 0 ? x : y;
    const size_t lda = job == 1 ? ldy : ldx, ldb = job == 0 ? ldx : ldy;
    const long rows_a = job == 1 ? sh.rows_y : sh.rows_x, rows_b = job == 0 ? sh.rows_x : sh.rows_y;

    {   // thread t < 128: row t of the a side's tile; the others: of the b side's.  Past the end: the last row (masked in the epilogue).  An index
        // outside its set never leaves it (the host refuses such a list; this keeps the reads inside the matrix whatever arrives).
        const bool side_b = tid >= KD_TILE;
        const long rows = side_b ? rows_b : rows_a;
        long r = (side_b ? tc : tr) * KD_TILE + (tid & (KD_TILE - 1));
        r = r < rows ? r : rows - 1;
        if (subsets > 0) {
            const bool from_y = side_b ? job != 0 : job == 1;
            const long limit = from_y ? m : n;
            long g = (from_y ? yi : xi)[sub * size + r];
            r = g < 0 ? 0 : (g < limit ? g : limit - 1);
        }
        rows_lds[tid] = (int)r;
    }
    __syncthreads();

    const int scol = tid & (KD_DC - 1), srow = tid / KD_DC;   // staging: a thread owns a column of every 8th row
    float va[KD_SL], vb[KD_SL];
    auto load = [&](int d0) {   // every load in bounds (the column clamped) and unconditional: all of a thread's loads are in flight together
        const size_t col = d0 + scol < d ? d0 + scol : d - 1;
#pragma unroll
        for (int i = 0; i < KD_SL; ++i) {
            va[i] = pa[(size_t)rows_lds[srow + i * KD_SR] * lda + col];
            vb[i] = pb[(size_t)rows_lds[KD_TILE + srow + i * KD_SR] * ldb + col];
        }
    };

    f64x4 acc[KD_F][KD_F];
#pragma unroll
    for (int i = 0; i < KD_F; ++i)
#pragma unroll
        for (int j = 0; j < KD_F; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;   // the lane's row (column) of a 16 x 16 tile and its k of a step of 4: A[fr][fk], B[fk][fr]
    const float* __restrict__ fa = as + (wr * KD_WT + fr) * KD_LD + fk;
    const float* __restrict__ fb = bs + (wc * KD_WT + fr) * KD_LD + fk;

    load(0);
    for (int d0 = 0; d0 < d; d0 += KD_DC) {
        __syncthreads();   // the chunk before is consumed
        const bool col_ok = d0 + scol < d;
#pragma unroll
        for (int i = 0; i < KD_SL; ++i) {
            as[(srow + i * KD_SR) * KD_LD + scol] = col_ok ? va[i] : 0.f;
            bs[(srow + i * KD_SR) * KD_LD + scol] = col_ok ? vb[i] : 0.f;
        }
        __syncthreads();
        if (d0 + KD_DC < d) load(d0 + KD_DC);   // under this chunk's MFMAs
        const int left = d - d0;
        const int steps = left >= KD_DC ? KD_DC / 4 : (left + 3) / 4;   // (the steps past d would add exact zeros)
#pragma unroll 1
        for (int q = 0; q < steps; ++q) {
            double a[KD_F], b[KD_F];
#pragma unroll
            for (int i = 0; i < KD_F; ++i) {
                a[i] = (double)fa[i * 16 * KD_LD + 4 * q];
                b[i] = (double)fb[i * 16 * KD_LD + 4 * q];
            }
#pragma unroll
            for (int i = 0; i < KD_F; ++i)
#pragma unroll
                for (int j = 0; j < KD_F; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // the cubic and the lane's chain, in the order (i, j, r).  Register r of tile (i, j): row (lane >> 4) + 4 r, column lane & 15 -- the fp64 map.
    const bool diagonal = job != 2 && tr == tc;
    const long row0 = tr * KD_TILE + wr * KD_WT + fk, col0 = tc * KD_TILE + wc * KD_WT + fr;
    const double dd = (double)d;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < KD_F; ++i)
#pragma unroll
        for (int j = 0; j < KD_F; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long gi = row0 + i * 16 + 4 * r, gj = col0 + j * 16;
                const double t = acc[i][j][r] / dd + 1.0;
                const double k = t * t * t;
                const bool take = gi < rows_a && gj < rows_b && !(diagonal && gi == gj);
                sum += take ? k : 0.0;
            }
    const double total = block_tree_f64<KD_NT>(sum, red);
    if (tid == 0) part[sub * sh.per_subset + blockIdx.x] = (job != 2 && !diagonal) ? 2.0 * total : total;
}

// grid (3, subsets).  out[subset][job] = the job's partials: thread t the partials t, t + 256 ... ascending, then the block's tree
__global__ __launch_bounds__(KD_NT) void kid_fold_kernel(const double* __restrict__ part, long n, long m, int subsets, long size, double* __restrict__ out) {
    __shared__ double red[KD_NT];
    const KidShape sh = kid_shape(n, m, subsets, size);
    const int job = blockIdx.x;
    const long begin = job == 0 ? 0 : job == 1 ? sh.txx : sh.txx + sh.tyy;
    const long count = job == 0 ? sh.txx : job == 1 ? sh.tyy : sh.txy;
    const double* __restrict__ p = part + (long)blockIdx.y * sh.per_subset + begin;
    double sum = 0.0;
    for (long i = threadIdx.x; i < count; i += KD_NT) sum += p[i];
    const double total = block_tree_f64<KD_NT>(sum, red);
    if (threadIdx.x == 0) out[(long)blockIdx.y * 3 + job] = total;
}

static bool kd_shape_ok(int64_t n, int64_t m, int d, int subsets, int64_t size) {
    if (n < 2 || n > GS_KID_MAX_ROWS || m < 2 || m > GS_KID_MAX_ROWS || d < 1 || d > GS_KMEANS_MAX_D || subsets < 0 || subsets > GS_KID_MAX_SUBSETS) return false;
    return subsets == 0 ? size == 0 : (size >= 2 && size <= n && size <= m);
}
static size_t kd_ws_bytes(int64_t n, int64_t m, int subsets, int64_t size) {
    const KidShape sh = kid_shape((long)n, (long)m, subsets, (long)size);
    return ((size_t)(subsets > 0 ? subsets : 1) * (size_t)sh.per_subset * sizeof(double) + 15) & ~(size_t)15;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_kid_workspace_bytes(int64_t n, int64_t m, int d, int subsets, int64_t size) {
    if (!kd_shape_ok(n, m, d, subsets, size)) return 0;
    return kd_ws_bytes(n, m, subsets, size);
}

extern "C" int gs_kid_sums(const float* x, int64_t ldx, int64_t n, const float* y, int64_t ldy, int64_t m, int d, const int32_t* xi, const int32_t* yi, int subsets,
                           int64_t size, double* out, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_FEATURE_D("kid_sums");
    GS_CHECK_ARG(n >= 2 && n <= GS_KID_MAX_ROWS, "kid_sums: n must be in [2, %d] (got %lld)", GS_KID_MAX_ROWS, (long long)n);
    GS_CHECK_ARG(m >= 2 && m <= GS_KID_MAX_ROWS, "kid_sums: m must be in [2, %d] (got %lld)", GS_KID_MAX_ROWS, (long long)m);
    GS_CHECK_FEATURE_LD("kid_sums", "ldx", ldx);
    GS_CHECK_FEATURE_LD("kid_sums", "ldy", ldy);
    GS_CHECK_ARG(subsets >= 0 && subsets <= GS_KID_MAX_SUBSETS, "kid_sums: subsets must be in [0, %d] (got %d)", GS_KID_MAX_SUBSETS, subsets);
    if (subsets == 0) {
        GS_CHECK_ARG(!xi && !yi, "kid_sums: xi and yi must be NULL with subsets 0 (the full sets)");
        GS_CHECK_ARG(size == 0, "kid_sums: size must be 0 with subsets 0 (got %lld)", (long long)size);
    } else {
        GS_CHECK_ARG(xi && yi, "kid_sums: null pointer (xi and yi are required with subsets %d)", subsets);
        GS_CHECK_ARG(aligned(xi, 4) && aligned(yi, 4), "kid_sums: misaligned pointer (xi and yi: 4 bytes)");
        GS_CHECK_ARG(size >= 2 && size <= n && size <= m, "kid_sums: size must be in [2, min(n, m)] (got %lld for n %lld, m %lld)", (long long)size, (long long)n,
                     (long long)m);
    }
    GS_CHECK_ARG(x && y && out, "kid_sums: null pointer (x, y and out are required)");
    GS_CHECK_ARG(aligned(x, 4) && aligned(y, 4) && aligned(out, 8), "kid_sums: misaligned pointer (x and y: 4 bytes, out: 8)");
    const size_t need = kd_ws_bytes(n, m, subsets, size);
    GS_CHECK_ARG(ws && ws_bytes >= need && aligned(ws, 16), "kid_sums: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const KidShape sh = kid_shape((long)n, (long)m, subsets, (long)size);
    const unsigned jobs = (unsigned)(subsets > 0 ? subsets : 1);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(kid_kernel, dim3((unsigned)sh.per_subset, jobs), dim3(KD_NT), 0, st, x, (size_t)ldx, (long)n, y, (size_t)ldy, (long)m, d, xi, yi, subsets,
                       (long)size, part);
    hipLaunchKernelGGL(kid_fold_kernel, dim3(3, jobs), dim3(KD_NT), 0, st, static_cast<const double*>(part), (long)n, (long)m, subsets, (long)size, out);
    GS_CHECK_LAUNCH();
    return 0;
}
