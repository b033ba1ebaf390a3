// What the conv translation units share (conv_igemm.hip, conv_wgrad.hip, conv_thin.hip, conv_api.hip): the kernel-role constants, which layers the
// implicit GEMM takes (igemm_supported), the weight-gradient launch descriptors and plan (WgradPlan), and the weight-prep kernel.
#pragma once
#include "gs_common.h"

namespace gs {

enum { MODE_S1 = 0, MODE_S2 = 1, MODE_T2 = 2 };
// the epilogue of an implicit-GEMM launch (conv_igemm_kernel's NORM): none, pixel norm, its first-order backward, its second-order backward
enum { IGEMM_PLAIN = 0, IGEMM_NORM_FWD = 1, IGEMM_NORM_BWD = 2, IGEMM_NORM_BWD2 = 3 };
#define GS_WGRAD_MAX_SRC 4   // (x, gy) pairs one weight-gradient launch contracts (GS_WGRAD_MAX_SOURCES)

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The channel counts the implicit-GEMM kernels take (3x3 layers; kernel-role ic -> oc): 64-byte channel chunks in, 32-channel tiles out.
// Everything else runs the VALU kernels of conv_thin.hip (conv_thin_route.h) and stores its prepared weight as fp32 (prep_plan).
__host__ __device__ inline bool igemm_supported(int ic, int oc, int dtype) {
    const int bk = dtype == GS_F32 ? 16 : 32;
    return ic % bk == 0 && oc % 32 == 0;
}

// Every weight gradient of a layer is two phases: block-partial sums over pixel slices (in the call's ws), then a reduction over the slices
// into gw (+ gb).  A call given a GsWgradReduce runs phase 1 only and describes phase 2 in it; wgrad_reduce_batch (conv_api.hip) then folds
// many pending reductions in a handful of launches (a backward pass has ~70 of them; each is a 10 us launch on its own).  The call's ws must
// stay untouched until then; nslices == 0 on return means nothing is pending (shapes without the vector reduce ran both phases at once).
struct GsWgradReduce {
    const float* partials;   // [nslices][taps*ic*oc (+ oc when gb)] fp32, inside the call's ws
    float* gw;               // [taps][ic][oc], or [taps][oc][ic] when transpose
    float* gb;               // optional [oc]
    int32_t nslices, taps, ic, oc;
    float alpha;
    int32_t transpose, accumulate;
    int32_t ic_ld;           // 0, or the input-channel rows of the stored variable when gw is a channel slice of a wider one (not with transpose)
};

// Several (x, gy) pairs of ONE layer -- the real and the fake discriminator pass, the second-order contribution -- are contracted
// by one launch: the images of all sources form one list (source s owns images n_end[s-1] .. n_end[s] - 1), so the layer costs one set of block
// partials and one slice reduction instead of one per pair.  bias_mask: which sources contribute to the bias gradient.
struct WgradSrcs {
    const void* x[GS_WGRAD_MAX_SRC];
    const void* gy[GS_WGRAD_MAX_SRC];
    int n_end[GS_WGRAD_MAX_SRC];   // cumulative image counts (unused entries = the total)
    unsigned bias_mask;
};
__device__ __forceinline__ int wgrad_source(const WgradSrcs& s, int nn, int& n_local) {
    const int src = (nn >= s.n_end[0]) + (nn >= s.n_end[1]) + (nn >= s.n_end[2]);
    n_local = nn - (src ? s.n_end[src - 1] : 0);
    return src;
}

// ---- grouped weight gradients (gs_conv_wgrad_jobs): the 64 x 64 channel-tile kernel run ONCE over the layers of a backward pass that
// share its instantiation (the conv mode: conv_wgrad.hip).  The work of the group is one list of units -- (layer, channel tile, pixel tile), in that
// order -- cut into equal contiguous ranges, one per block (a "stream-K" schedule).  A block keeps its accumulators across the pixel
// tiles of one (layer, channel tile) RUN and writes a partial only where its range leaves the run: partials = blocks + runs per
// launch instead of blocks per LAYER, and the summation order of a run (ascending block index) is a function of the shapes alone.
#define GS_SK_MAX_JOBS 16
#define GS_SK_PSTRIDE (9 * 64 * 64 + 64)   // floats of one partial: 9 taps of a 64 x 64 tile + 64 bias sums
struct SkJob {
    WgradSrcs srcs;
    float* gw;                      // [9][IC][OC] (or [9][OC][IC] when transpose), fp32
    float* gb;                      // optional [OC]
    float alpha;
    int transpose, accumulate;
    int Hi, Wi, IC, OC, Hb, Wb;     // kernel-role geometry (input side / gradient side)
    int ICld;                       // input-channel rows of the stored variable (IC, or more when gw is a channel slice of a wider one)
    int tiles_x, tiles_y, ntiles;   // pixel tiles over the images of all sources
    int n_ict, nct;                 // IC / 64, channel tiles (IC / 64) * (OC / 64)
    int unit_base, run_base;        // first unit / first run of the layer inside the group
};
struct SkGroup {
    int njobs, total_units, total_runs, nblocks;
    SkJob job[GS_SK_MAX_JOBS];
};
// block that owns unit u when block b owns [b * total / nb, (b + 1) * total / nb)
__host__ __device__ inline int sk_block_of(long u, long nb, long total) { return (int)(((u + 1) * nb - 1) / total); }

// ------------------------------------------------------------------------------ weight prep
// Re-lays the fp32 HWIO master weight into the kernel operand Wp[tap][OCk][ICk] (ICk contiguous,
// storage type T, no scaling -- alpha is applied to the fp32 accumulators).
//   variant 0 (fwd)        : Wp[t][co][ci]       = w[t][ci][co]      (OCk = co, ICk = ci)
//   variant 1 (bwd-data S1): Wp[taps-1-t][ci][co] = w[t][ci][co]     (OCk = ci, ICk = co; taps flipped)
//   variant 2 (bwd-data T2): Wp[t][ci][co]       = w[t][ci][co]      (OCk = ci, ICk = co)
template <typename T>
__global__ void weight_prep_kernel(const float* __restrict__ w, T* __restrict__ wp, int taps, int ci, int co, int variant) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)taps * ci * co;
    if (idx >= total) return;
    if (variant == 0) {
        int c_i = idx % ci;
        int c_o = (idx / ci) % co;
        int t = idx / ((long)ci * co);
        DT<T>::st(wp + idx, w[((long)t * ci + c_i) * co + c_o]);
    } else {
        int t = idx / ((long)ci * co);
        long rem = idx % ((long)ci * co);
        int tt = variant == 1 ? taps - 1 - t : t;
        DT<T>::st(wp + (long)tt * ci * co + rem, w[idx]);
    }
}

// ---- THE selection of a layer's weight-gradient kernel (conv_wgrad.hip: wgrad_plan): which kernel takes a kernel-role shape, its tiling, its
// slice count and the fold behind it.  The launchers (run_wgrad_mfma, run_wgrad_direct), the workspace sizes, plan_jobs and the host-only
// queries gs_conv_wgrad_plan / gs_conv_wgrad_jobs_plan all read this struct; nobody decides a second time.
enum { WG_DIRECT = 0, WG_THIN = 1, WG_F32 = 2, WG_BF16 = 3, WG_THIN_DMA = 4, WG_TILE64 = 5 };   // GS_WGRAD_* of include/gansynth_hip.h
struct WgradPlan {
    int family;                    // WG_*
    int mode;                      // MODE_S1 / MODE_S2
    int tw;                        // pixel-tile width of the MFMA kernels (16 / 32); 0: direct / thin
    int ot;                        // MFMA: 32-channel output tiles per block (1 / 2; 2 x 2 for WG_TILE64); WG_THIN: 1 when x is the wide side
    int tiles_x, tiles_y, ntiles;  // MFMA: pixel tiles over all images; direct / thin: ntiles = output pixels
    int nslices;                   // block partials the fold sums
    int ws_slices;                 // partials the workspace is sized for (>= nslices)
    long pps;                      // direct / thin: pixels per slice
    int fold;                      // the immediate fold: 0 the scalar kernel, else wgrad_reduce_kernel's slice lanes (4 / 16)
    int batch_lanes;               // slice lanes of wgrad_reduce_batch_kernel for this entry (4 / 16); 0: the fold cannot stay pending
    int fused_bias;                // 1: the kernel produces the bias gradient on the side (a bias row per slice)
};
WgradPlan wgrad_plan(int mode, int ks, int dtype, int N, int Hb, int Wb, int IC, int OC);
// slice lanes of the vector folds for a reduction over `nslices` partials (immediate and batched alike)
static inline int wgrad_fold_lanes(int nslices) { return nslices > 32 ? 16 : 4; }

// ---- slice reductions (kernels and launchers: conv_wgrad.hip)
// phase 2 of one weight gradient: gw = alpha * sum over the slices of `part` (+ gb), or, given `defer` and a shape with the vector reduce, its description
void wgrad_reduce_launch(float* part, float* gw, float* gb, int nslices, int taps, int ic, int oc, float alpha, int transpose, int accumulate, hipStream_t st,
                         GsWgradReduce* defer = nullptr);
// many reductions per launch (wgrad_reduce_batch): blockIdx.y = entry, blockIdx.x = element chunk of that entry
#define GS_REDUCE_BATCH 16
struct ReduceBatch {
    GsWgradReduce e[GS_REDUCE_BATCH];
};
// the first `count` entries of b in one launch of `blocks_x` element chunks each
void wgrad_reduce_batch_launch(const ReduceBatch& b, int count, long blocks_x, hipStream_t st);

}  // namespace gs
