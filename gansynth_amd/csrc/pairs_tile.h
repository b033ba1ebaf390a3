// The all-pairs squared-distance tile of kmeans_assign_kernel (kmeans.hip) and knn_kernel (knn.hip): d(i, j) = sum (x_i - y_j)^2 in fp32 as ONE
// chain over the columns ascending, a subtraction and an FMA per term.  Both kernels stage through pairs_stage and add through pairs_chain, so
// d(i, j) is one number, bit for bit, in gs_kmeans_assign, gs_knn_kth and gs_knn_within (tests/test_knn_gpu.py compares them).
//   * A block of four waves owns PT_TILE = 256 rows of the first side and walks the columns in chunks of PT_DC = 32.  The rows' chunk is staged
//     in LDS as xs[row][36] (global reads: a wave covers two rows' 128-byte pieces per instruction; nothing needs more than 4-byte alignment),
//     a group of SLOTS rows of the other side as cs[slot][32].  Columns past d are 0 on both sides: they add an exact 0.
//   * A wave owns KG <= 16 consecutive slots, a lane PT_P = 4 rows of the tile against them: 4 KG accumulators.  A row's four floats are one
//     ds_read_b128 (the stride of 36 floats puts the 16 lanes of a group on 64 distinct banks), a slot's four floats one broadcast ds_read_b128
//     that feeds 32 VALU instructions: the LDS pipe runs at about a third of the VALU.
// Rounds, slices, what becomes of a finished distance, the epilogues and the launch bounds are the callers'.
// (kid.hip stays apart: it gathers rows through an index list, keeps the next chunk in registers under its MFMAs and stages both sides alike.)
#pragma once
#include <type_traits>

#include "gs_common.h"

namespace gs {

constexpr int PT_NT = 256;                 // threads per block
constexpr int PT_WAVES = PT_NT / 64;
constexpr int PT_P = 4;                    // rows of the tile a lane owns
constexpr int PT_TILE = 64 * PT_P;         // rows a block owns
constexpr int PT_DC = 32;                  // columns per chunk
constexpr int PT_XS = PT_DC + 4;           // floats between two rows of xs: 16 lanes of a ds_read_b128 group on 64 distinct banks
constexpr int PT_SR = PT_NT / PT_DC;       // staging: a thread owns a column of every PT_SR-th row
typedef float f32x2 __attribute__((ext_vector_type(2)));   // two rows of a lane in one register pair

// A lane's accumulators.  Scalar: acc[p][j], row lane + 64 p of the tile against slot j of the wave.  Packed: rows (2 pp, 2 pp + 1) side by side
// in acc[pp][j], so that t = x - y is a v_pk_add_f32 and the chain a v_pk_fma_f32 -- per half the scalar form's operations in its order, bit
// for bit (measured: the same sums over every output).  Which form is faster depends on the kernel around it (build.sh).
template <int KG, bool PACKED> using pairs_acc = std::conditional_t<PACKED, f32x2[PT_P / 2][KG], float[PT_P][KG]>;

// Columns [d0, d0 + PT_DC) of the tile's rows a[tile_begin ..) into xs and of the other side's rows b[begin + (0 .. SLOTS)) into cs; the other
// side ends at `end` (Index: int or long, the caller's).  Every load is in bounds (row and column clamped) and unconditional, so that all of a
// thread's loads are in flight together; what lies past n, `end` or d is dropped for a 0 on the way into LDS.  Called by the whole block.
// (Plain `inline`, not __forceinline__: inlined ahead of the caller's own optimisation, knn_kernel<3, 5, 8> spill 8 to 12 bytes more.)
template <int SLOTS, typename Index>
__device__ inline void pairs_stage(float* __restrict__ xs, float* __restrict__ cs, const float* __restrict__ a, size_t lda, long tile_begin, long n,
                                   const float* __restrict__ b, size_t ldb, Index begin, Index end, int d0, int d) {
    const int scol = threadIdx.x & (PT_DC - 1), srow = threadIdx.x / PT_DC;
    __syncthreads();   // the chunk before is consumed
    const bool col_ok = d0 + scol < d;
    const size_t col = col_ok ? d0 + scol : d - 1;
    constexpr int XL = PT_TILE / PT_SR / 2, CL = (SLOTS + PT_SR - 1) / PT_SR;
    float cv[CL];
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        const Index bj = begin + srow + i * PT_SR;
        cv[i] = b[(size_t)(bj < end ? bj : end - 1) * ldb + col];
    }
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {   // (two batches of 16 loads: all 32 at once cost kmeans_assign_kernel a wave per SIMD in registers)
        float xv[XL];
        const int row0 = srow + half * XL * PT_SR;
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const long gi = tile_begin + row0 + i * PT_SR;
            xv[i] = a[(size_t)(gi < n ? gi : n - 1) * lda + col];
        }
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int row = row0 + i * PT_SR;
            xs[row * PT_XS + scol] = (col_ok && tile_begin + row < n) ? xv[i] : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        const int s = srow + i * PT_SR;
        if (SLOTS % PT_SR == 0 || s < SLOTS) cs[s * PT_DC + scol] = (col_ok && begin + s < end) ? cv[i] : 0.f;
    }
    __syncthreads();
}

// The staged chunk's PT_DC terms onto every accumulator of the lane, columns ascending.  cs_wave: the wave's first slot.
template <int KG, bool PACKED>
__device__ inline void pairs_chain(const float* __restrict__ xs, const float* __restrict__ cs_wave, int lane, pairs_acc<KG, PACKED>& acc) {
#pragma unroll 1
    for (int q = 0; q < PT_DC / 4; ++q) {
        float xr[PT_P][4];
#pragma unroll
        for (int p = 0; p < PT_P; ++p) ld4(xs + (lane + 64 * p) * PT_XS + 4 * q, xr[p]);
#pragma unroll
        for (int j = 0; j < KG; ++j) {
            float c[4];
            ld4(cs_wave + j * PT_DC + 4 * q, c);   // one address a wave: a broadcast
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (PACKED) {
#pragma unroll
                    for (int pp = 0; pp < PT_P / 2; ++pp) {
                        const f32x2 x2 = {xr[2 * pp][e], xr[2 * pp + 1][e]};
                        const f32x2 t = x2 - c[e];
                        acc[pp][j] = __builtin_elementwise_fma(t, t, acc[pp][j]);
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < PT_P; ++p) {
                        const float t = xr[p][e] - c[e];
                        acc[p][j] = fmaf(t, t, acc[p][j]);
                    }
                }
            }
        }
    }
}

}  // namespace gs
