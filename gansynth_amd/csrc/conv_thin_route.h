// Which VALU kernel a conv call outside the implicit GEMM runs -- the 1x1 colour convs, the one-output-channel gradients of the stddev plane,
// the generic direct conv: ONE host function, thin_route, read by the entry points of conv_api.hip, the launcher of conv_thin.hip and the
// host-only query gs_conv_thin_route.  Nobody decides a second time.  Host arithmetic only: no HIP call, so it answers without a device.
// The split between the implicit GEMM and these kernels is NOT made here: it is the caller's (conv_api.hip: on_igemm, on igemm_supported of
// conv_shared.h), so thin_route answers for any shape, those it is never asked about included.
// (The weight gradients of these layers belong to wgrad_plan, conv_wgrad.hip.)
#pragma once
#include <stdlib.h>

#include "conv_shared.h"

namespace gs {

// What is asked: a kernel-role shape (conv_api.hip: conv_role) and the passes that ride with the conv
struct ThinCall {
    int mode, ks, ICk, OCk, dtype;
    long P;          // output pixels: N * Ho * Wo
    int form;        // GS_THIN_PLAIN / GS_THIN_FWD_MASK / GS_THIN_BWD_PNBWD
    int act;         // plain, masked: the activation behind the conv; through the norm: the one in front of it (none / leaky relu)
    int has_bias;
    int mask_act;    // masked forward: the activation whose derivative multiplies the result (0: no mask given, the plain kernel)
    int want_bits;   // the bf16 leaky-relu result is to carry its sign words behind it
};

// the grid caps of the two streaming kernels (measurement knobs)
struct ThinKnobs {
    long expand_blocks, reduce_blocks;
};
inline ThinKnobs thin_knobs_env() {   // read once per process
    static const ThinKnobs k = [] {
        ThinKnobs v;
        // (2048 blocks: 18.5 us for the 67 MB of the top level against 19.4 at 4096 and 23.0 at 8192 -- every block pays the weight prologue)
        v.expand_blocks = getenv("GS_THIN_EXPAND_BLOCKS") ? atol(getenv("GS_THIN_EXPAND_BLOCKS")) : 2048;
        v.reduce_blocks = getenv("GS_THIN_REDUCE_BLOCKS") ? atol(getenv("GS_THIN_REDUCE_BLOCKS")) : 4096;
        return v;
    }();
    return k;
}

// What runs.  The first GS_THIN_ROUTE_INTS - 3 fields name the launch, the last three say which of the requested passes the kernel does itself:
// what it does not do, the caller adds (gs_bias_act_fwd / gs_pixel_norm_bwd_fused, gs_act_bwd, gs_pack_act_bits).  All int, in the order
// gs_conv_thin_route reports them.
struct ThinRoute {
    int kernel;           // GS_THIN_*
    int C;                // the few-channel side as a template constant: IC of EXPAND / EXPAND_PNBWD, OC of REDUCE; else 0
    int ACT, MASKED;      // EXPAND, REDUCE (ACT)
    int LC;               // REDUCE: lanes per pixel as a constant (4 / 8), 0 = run-time
    int OCV, VEC;         // DIRECT
    int grid;             // blocks of 256 threads
    int ppb;              // pixels per block pass (DIRECT: 0, its threads are flat over pixel x channel group)
    int trips, tails;     // passes a block makes: full four-pass trips (EXPAND, REDUCE) and single passes (EXPAND: of a block's first pixel lane)
    int epilogue_fused;   // bias + activation, or the norm's backward, happen in the kernel
    int mask_fused;
    int bits_fused;
};

inline ThinRoute thin_route(const ThinCall& c, const ThinKnobs& k) {
    ThinRoute r;
    memset(&r, 0, sizeof(r));
    const int wn = c.dtype == GS_F32 ? 4 : 8;   // Wide<T>::N
    const bool colour = c.ks == 1 && c.mode == MODE_S1;
    auto stream = [&](int kernel, int lanes, long cap) {   // lanes of a pixel, pixel passes over a capped grid
        long nb = cdiv(c.P * lanes, 256);
        if (nb > cap) nb = cap;
        r.kernel = kernel;
        r.grid = (int)nb;
        r.ppb = 256 / lanes;
        return nb > 0 ? (c.P + nb * r.ppb - 1) / (nb * r.ppb) : 0;
    };
    if (c.form == GS_THIN_BWD_PNBWD) {
        const int groups = c.OCk / wn;
        if (colour && c.ICk >= 1 && c.ICk <= 4 && c.OCk % wn == 0 && groups >= 1 && groups <= 64 && (groups & (groups - 1)) == 0) {   // the colour block as a gradient
            r.tails = (int)stream(GS_THIN_EXPAND_PNBWD, groups, 4096);
            r.C = c.ICk;
            r.epilogue_fused = 1;
            return r;
        }
    }
    // (through the norm without that kernel: the plain data gradient, the norm's backward left to the caller)
    const int act = c.form == GS_THIN_BWD_PNBWD ? GS_ACT_NONE : c.act;
    const bool epilogue = c.form != GS_THIN_BWD_PNBWD && (c.has_bias || act != GS_ACT_NONE);
    if (colour && c.ICk <= 4 && c.OCk % wn == 0 && 256 % (c.OCk / wn) == 0) {   // colour -> features
        const long npass = stream(GS_THIN_EXPAND, c.OCk / wn, k.expand_blocks);
        r.trips = (int)(npass / 4);
        r.tails = (int)(npass % 4);
        r.C = c.ICk;
        r.ACT = act;
        r.MASKED = c.form == GS_THIN_FWD_MASK && c.mask_act != GS_ACT_NONE;
        r.epilogue_fused = epilogue;
        r.mask_fused = r.MASKED;
        r.bits_fused = c.want_bits && !r.MASKED && act == GS_ACT_LRELU && c.dtype == GS_BF16 && c.OCk % 32 == 0;
        return r;
    }
    const int lanes = c.ICk / wn;
    if (colour && c.OCk <= 4 && c.ICk % wn == 0 && lanes <= 64 && (lanes & (lanes - 1)) == 0) {   // features -> colour
        const long npass = stream(GS_THIN_REDUCE, lanes, k.reduce_blocks);
        r.trips = (int)(npass / 4);
        r.tails = (int)(npass % 4);
        r.C = c.OCk;
        r.ACT = act;
        r.LC = lanes == 4 || lanes == 8 ? lanes : 0;
        r.epilogue_fused = epilogue;
        return r;
    }
    if (c.OCk == 1 && c.ICk >= 64) {   // a wave per output pixel; 256 channels at 3x3: every load ahead of the first multiply
        r.kernel = c.ICk == 256 && c.ks == 3 ? GS_THIN_SINGLE3 : GS_THIN_SINGLE;
        r.grid = cdiv(c.P, 4);
        r.ppb = 4;
        r.tails = 1;
        r.epilogue_fused = epilogue;
        return r;
    }
    r.kernel = GS_THIN_DIRECT;
    r.OCV = c.OCk % 4 == 0 ? 4 : (c.OCk % 2 == 0 ? 2 : 1);
    r.VEC = c.ICk % 4 == 0 ? 4 : 1;
    r.grid = cdiv(c.P * (c.OCk / r.OCV), 256);
    r.tails = 1;
    r.epilogue_fused = epilogue;   // (on the fp32 sum: a pass behind the kernel would add the bias to a sum already rounded to bf16)
    return r;
}

// The operands of one launch: pointers, kernel-role geometry, alpha, and the norm's eps / activation of EXPAND_PNBWD
struct ThinArgs {
    const void* x;          // what the kernel reads: x, or gy of a data gradient
    const float* wp;        // the prepared fp32 weight [tap][OCk][ICk]
    void* y;
    const float* bias;      // optional
    const void* mask;       // masked forward
    int mask_act;
    unsigned* bits;         // where the sign words go (behind y)
    const void* z;          // EXPAND_PNBWD: the previous block's activation, and the optional second gradient into it
    const void* addend;
    float eps;
    int act;
    int dtype, mode, ks, N, Hi, Wi, ICk, OCk, Ho, Wo;
    long P;                 // N * Ho * Wo
    float alpha;
};
// launches what the route says (conv_thin.hip); GS_ERR_UNSUPPORTED for a route that names no compiled instantiation
int run_thin(const ThinRoute& r, const ThinArgs& a, hipStream_t st);

}  // namespace gs
