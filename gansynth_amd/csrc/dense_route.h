// Which kernel a dense call runs -- forward, data gradient, weight gradient, plain rows or the row map of a channels-last input: ONE host
// function, dense_route, read by the three launchers of dense.hip, by gs_dense_fwd_workspace_bytes and by the host-only query gs_dense_route.
// Nobody decides a second time.  Host arithmetic only: no HIP call, so it answers without a device.
#pragma once
#include <stdlib.h>

#include "gs_common.h"

namespace gs {

constexpr int DENSE_BT = 16;  // batch rows held in registers per pass
constexpr int DENSE_WR = 16;  // weight rows per block of dense_bwd_weight_fast_kernel

// What is asked.  rc = rhw = 0: plain rows; else the input side is a channels-last [b][rhw][rc] activation, in == rc * rhw
struct DenseCall {
    int map;   // GS_DENSE_MAP_*
    int b, in, out, rc, rhw, dtype;
};

struct DenseKnobs {
    int no_mfma;   // A/B switch: the MFMA layers on the VALU kernels
};
inline DenseKnobs dense_knobs_env() {   // read once per process
    static const DenseKnobs k = {getenv("GS_NO_DENSE_MFMA") != nullptr};
    return k;
}

// What runs: `passes` launches of `kernel` over `step` batch rows each, then the finalize pass where one follows.  All int, in the order
// gs_dense_route reports them; ws_bytes as its last two (low word first).
struct DenseRoute {
    int kernel;           // GS_DENSE_*
    int FB, WPR;          // template constants; 0 where the kernel has none
    int step, passes;     // batch rows per launch, launches over the batch
    int grid_x, grid_y;   // blocks of 256 threads
    int ksplit, ipb;      // forward: slices of the reduction and input rows per slice (no split: 1, in); gradients: 0
    int finalize;         // a dense_finalize_kernel launch follows (it folds the ksplit partials and applies alpha, bias, activation)
    size_t ws_bytes;      // forward: the partials [ksplit][b][out] (sized by the split whichever kernel runs)
};

// batch rows per pass of the fast kernels: 8, 16 or 24 (FB template parameter) -- the discriminator's 16- and 24-row calls read the
// weight matrix once instead of two or three times
inline int dense_fast_rows(int b) { return b <= 8 ? 8 : (b <= 16 ? 16 : 24); }

// 0 and the route, or the error code the entry points answer with and `why`
inline int dense_route(const DenseCall& c, const DenseKnobs& k, DenseRoute* route, const char** why) {
    DenseRoute r;
    memset(&r, 0, sizeof(r));
    *route = r;
    const int b = c.b, in = c.in, out = c.out;
    auto refuse = [&](int code, const char* text) { *why = text; return code; };
    if (!(b > 0 && in > 0 && out > 0)) return refuse(GS_ERR_ARG, "bad args");
    if (!(c.rc == 0 || (c.rc > 0 && c.rhw > 0 && (long)c.rc * c.rhw == in))) return refuse(GS_ERR_ARG, "the channels-last input is not `in` wide");
    auto launch = [&](int kernel, int step, int gx, int gy) { r.kernel = kernel; r.grid_x = gx; r.grid_y = gy; r.step = step; r.passes = cdiv(b, step); };   // step b: one launch
    if (c.map == GS_DENSE_MAP_FWD) {
        const bool fast = in % 4 == 0 && out % 32 == 0;
        const bool mfma = !k.no_mfma && in >= 2048 && in % 64 == 0 && out % 64 == 0 && out <= 1024;
        if (c.rc && !fast) return refuse(GS_ERR_UNSUPPORTED, "channels-last input needs in % 4 == 0 and out % 32 == 0");
        int ks, ipb;
        if (mfma) {   // tall layer on the fp32 MFMA: 64 input rows per wave
            ipb = 64;
            ks = in / 64;
        } else if (fast) {   // (out/32) x ksplit blocks should cover the chip twice; a split handles >= 128 rows
            const int tiles = out / 32, maxks = in / 128 > 0 ? in / 128 : 1;
            ks = tiles >= 128 ? 1 : (512 + tiles - 1) / tiles;   // >= 128 column tiles: no split, no finalize launch
            if (ks > maxks) ks = maxks;
            ipb = ((in + ks - 1) / ks + 3) & ~3;
            ks = (in + ipb - 1) / ipb;
        } else {
            const int tiles = cdiv(out, 64), maxks = in / 32 > 0 ? in / 32 : 1;
            ks = 1024 / tiles > 0 ? 1024 / tiles : 1;
            if (ks > maxks) ks = maxks;
            ipb = cdiv(in, ks);
            ks = cdiv(in, ipb);
        }
        r.ws_bytes = (size_t)ks * b * out * sizeof(float);
        r.ksplit = ks;
        r.ipb = ipb;
        if (!c.rc && in <= 1024 && out <= 256 && b <= 64) {   // small layer: direct, one launch
            launch(GS_DENSE_FWD_SMALL, b, cdiv(out, 64), b);
            r.ksplit = 1;
            r.ipb = in;
        } else if (mfma) {
            launch(GS_DENSE_FWD_MFMA, b, cdiv((out / 64) * ks, 4), 1);
            r.finalize = 1;
        } else if (fast) {
            r.FB = dense_fast_rows(b);
            launch(GS_DENSE_FWD_FAST, r.FB, out / 32, ks);
            r.finalize = ks > 1;   // ksplit == 1: the kernel writes the result itself
        } else {
            launch(GS_DENSE_FWD, DENSE_BT, cdiv(out, 64), ks);
            r.finalize = 1;
        }
    } else if (c.map == GS_DENSE_MAP_BWD_DATA) {
        if (c.rc && out % 256 != 0) return refuse(GS_ERR_UNSUPPORTED, "channels-last input needs out % 256 == 0");
        if (!k.no_mfma && in >= 1024 && out % 16 == 0 && out <= 4096) {   // many short rows: a wave per 16 weight rows on the fp32 MFMA
            launch(GS_DENSE_BWD_DATA_MFMA, b, cdiv(cdiv(in, 16), 4), 1);
        } else if (out % 256 == 0) {
            r.WPR = in <= 1024 && out >= 1024 ? 4 : 1;   // few long rows: the whole block on one row
            r.FB = dense_fast_rows(b);
            launch(GS_DENSE_BWD_DATA_FAST, r.FB, r.WPR == 4 ? in : cdiv(in, 4), 1);
        } else if (out >= 2048) {
            launch(GS_DENSE_BWD_DATA_WIDE, DENSE_BT, in, 1);
        } else {
            launch(GS_DENSE_BWD_DATA, DENSE_BT, cdiv(in, 4), 1);
        }
    } else if (c.map == GS_DENSE_MAP_BWD_WEIGHT) {
        const bool fast = out % 256 == 0 && b <= DENSE_BT;
        if (c.rc && !fast) return refuse(GS_ERR_UNSUPPORTED, "channels-last input needs out % 256 == 0 and batch <= 16");
        if (fast) launch(GS_DENSE_BWD_WEIGHT_FAST, b, out / 256, cdiv(in, DENSE_WR));
        else launch(GS_DENSE_BWD_WEIGHT, b, cdiv((long)in * out, 256), 1);
    } else {
        return refuse(GS_ERR_ARG, "bad map");
    }
    *route = r;
    return 0;
}

}  // namespace gs
