// Pieces the pitch classifier's forward (classifier.hip) and backward (classifier_bwd.hip) share: the weight-standardisation block
// body (one definition, so that the per-weight and the batched launch give the same bits), the group-norm slice geometry and checks.
#pragma once
#include <math.h>

#include "gs_common.h"

namespace gs {

// ------------------------------------------------------------------------------------------ weight standardisation (ops.py:53-66)
// out[:, c] = (w[:, c] - mean) / sqrt(var + eps) over the fan_in rows of an HWIO weight viewed as [fan_in][co]; population variance,
// two passes in double.  A block owns WS_CH consecutive channels (one 64-byte row segment per read) and splits the rows over WS_RL
// row lanes; the row lanes' sums meet in LDS and are added in a fixed tree order.
constexpr int WS_CH = 16, WS_RL = 16;

__device__ inline double ws_block_sum(double v, double* red) {   // sum over the WS_RL row lanes of this thread's channel, fixed order
    const int ch = threadIdx.x % WS_CH, rl = threadIdx.x / WS_CH;
    red[rl * WS_CH + ch] = v;
    __syncthreads();
    for (int h = WS_RL / 2; h > 0; h >>= 1) {
        if (rl < h) red[rl * WS_CH + ch] += red[(rl + h) * WS_CH + ch];
        __syncthreads();
    }
    const double r = red[ch];
    __syncthreads();
    return r;
}

// channels blk * WS_CH ... of one weight; rstd (optional) receives 1 / sqrt(var + eps) per channel for the backward
__device__ inline void weight_std_block(const float* __restrict__ w, float* __restrict__ out, float* __restrict__ rstd, int fan, int co, float eps,
                                        int blk, double* red /* WS_CH * WS_RL */) {
    const int ch = threadIdx.x % WS_CH, rl = threadIdx.x / WS_CH;
    const int c = blk * WS_CH + ch;
    const bool ok = c < co;
    double s = 0.0;
    if (ok)
        for (int i = rl; i < fan; i += WS_RL) s += w[(long)i * co + c];
    const double m = ws_block_sum(s, red) / fan;
    double v = 0.0;
    if (ok)
        for (int i = rl; i < fan; i += WS_RL) { const double d = w[(long)i * co + c] - m; v += d * d; }
    const double r = 1.0 / sqrt(ws_block_sum(v, red) / fan + (double)eps);
    if (ok) {
        for (int i = rl; i < fan; i += WS_RL) out[(long)i * co + c] = (float)((w[(long)i * co + c] - m) * r);
        if (rstd && rl == 0) rstd[c] = (float)r;
    }
}

// ---------------------------------------------------------------------------------------------- group normalisation (ops.py:120-146)
// slices of one image's pixels: S slices of pps pixels (both passes of the statistics and of the backward walk the same slices)
inline int gn_geometry(int n, int hw, int c, int* S, int* pps) {
    const int R = 256 / (c / 4);
    int s = 2048 / (n > 0 ? n : 1);
    const int cap = hw / (4 * R);
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    *pps = (hw + s - 1) / s;
    *S = (hw + *pps - 1) / *pps;
    return 0;
}

inline int check_gn(int n, int hw, int c, int groups, int dtype) {
    GS_CHECK_ARG(n > 0 && hw > 0 && groups > 0, "group_norm: bad sizes (n %d, hw %d, groups %d)", n, hw, groups);
    GS_CHECK_ARG(c >= 4 && c <= 1024 && (c & (c - 1)) == 0, "group_norm: %d channels (a power of two from 4 to 1024)", c);
    GS_CHECK_ARG(c % groups == 0 && groups <= 256, "group_norm: %d channels in %d groups", c, groups);
    GS_CHECK_ARG(dtype == GS_F32 || dtype == GS_BF16, "group_norm: bad dtype %d", dtype);
    return 0;
}

}  // namespace gs
