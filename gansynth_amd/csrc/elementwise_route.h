// Which kernel an elementwise / row-reduction call runs (elementwise.hip, the batch-stddev kernels of small_ops.hip), on which path, with
// which template constants, grid, partial rows and workspace: ONE host function, elementwise_route, read by the entry points, by
// gs_channel_sum_workspace_bytes, gs_pixel_norm_bwd_bias_workspace_bytes and gs_bias_partial_rows, and by the host-only query
// gs_elementwise_route.  Nobody decides a second time.  Host arithmetic only: no HIP call, so it answers without a device.
// (channel_sum_kernel picks colour / quads / generic inside the kernel, from p and c alone: the route states the same conditions.)
#pragma once
#include <stdlib.h>

#include "gs_common.h"

namespace gs {

constexpr int CS_SLAB = 64;      // partial rows per first-level block of the channel-sum finalize
constexpr int SSQ_CHUNKS = 64;   // blocks a row of sumsq_rows is split over

// What is asked.  The shape words by operation:
//   bias_act, channel_sum, act_bwd_bias, pixel_norm_*:   p rows of c channels
//   act_bwd, tanh_bwd_bwd, axpby, axpby_dev:             p = numel
//   upscale, blocksum:                                   p = OUTPUT elements (n * ho * wo * c), fy x fx the factors
//   row_scale, sumsq_rows:                               p = cols, fy = rows
//   batch_stddev_*:                                      p = hw, c, fy = batch
struct EwCall {
    int op, dtype;   // GS_EW_OP_*, GS_F32 / GS_BF16
    long p;
    int c, fy, fx;
};

struct EwKnobs {
    long ew_cap;       // GS_EW_GRID_CAP: blocks of a grid-stride kernel (256 CUs x 8 blocks x 4)
    int pn_bias_cap;   // GS_PN_BIAS_GRID_CAP: blocks of the pixel-norm backward that also sums its result per channel
};
inline EwKnobs ew_knobs_env() {   // read once per process (measurement knobs)
    static const EwKnobs k = {getenv("GS_EW_GRID_CAP") ? atol(getenv("GS_EW_GRID_CAP")) : 8192,
                              getenv("GS_PN_BIAS_GRID_CAP") ? atoi(getenv("GS_PN_BIAS_GRID_CAP")) : 1024};
    return k;
}

// What runs.  All int, in the order gs_elementwise_route reports them; ws_bytes as its last two (low word first).
struct EwRoute {
    int kernel;           // GS_EW_*: the kernel template
    int path;             // GS_EW_PATH_*: the branch inside it
    int E;                // elements per lane and access: 4 (ld4 / st4), Wide<T>::N (pixel norm, stddev VN), 1 scalar
    int P, U, L;          // pixel norm: passes per row, row groups per trip, lanes per row; 0 elsewhere
    int rows;             // pixel norm: rows per wave; channel_sum / act_bwd_sum: row lanes per block; 0 elsewhere
    int grid_x, grid_y;   // blocks (256 threads; stddev 1024)
    int trips;            // trips of the busiest thread's loop (channel_sum quads / generic, act_bwd_sum: rows a row lane visits)
    int tail;             // a sub-vector tail runs (act_bwd, axpby*, sumsq_rows) | the last trip is partial (blocksum wave, stddev, rows kernel)
    int nparts;           // partial rows left for the fold (what gs_bias_partial_rows answers); 0: the kernel writes the sums itself
    int levels;           // channel_sum_final_kernel launches that follow: 0, 1, 2 (nparts > CS_SLAB)
    int per;              // sumsq_rows: 4-element vectors per chunk
    int two_pass;         // act_bwd_bias: the channel sum this route describes (of g * act'(y): its ACT instantiation), then an act_bwd launch over p * c elements
    int reserved;
    size_t ws_bytes;      // what the workspace functions answer (sized for the partial rows whichever kernel runs)
};

inline int ew_grid(long nvec, long cap) {
    long g = (nvec + 255) / 256;
    if (g > cap) g = cap;  // grid-stride the rest
    if (g < 1) g = 1;
    return (int)g;
}

inline int channel_sum_parts(long p, int c) {
    long rows_per_block = 256 / (c >= 4 ? ((c & 3) == 0 ? c / 4 : (c < 256 ? c : 256)) : c);
    if (rows_per_block < 1) rows_per_block = 1;
    long nb = (p + rows_per_block * 8 - 1) / (rows_per_block * 8);
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    return (int)nb;
}

// the partial rows of `nparts` blocks and the finalize that folds them
inline void ew_partials(EwRoute& r, int nparts, int c) {
    r.nparts = nparts;
    r.levels = nparts <= CS_SLAB ? 1 : 2;
    r.ws_bytes = (size_t)(nparts + cdiv(nparts, CS_SLAB)) * c * sizeof(float);
}

inline void channel_sum_route(long p, int c, EwRoute& r) {
    const int nparts = channel_sum_parts(p, c);
    ew_partials(r, nparts, c);
    r.grid_y = 1;
    if (p <= 64 && c >= 256) {   // few rows, many channels: a thread per channel, no partials
        r.kernel = GS_EW_CHANNEL_SUM_ROWS;
        r.grid_x = cdiv(c, 256);
        r.trips = (int)p;
        r.tail = c % 256 != 0;
        r.E = 1;
        r.nparts = r.levels = 0;
        return;
    }
    r.kernel = GS_EW_CHANNEL_SUM;
    r.grid_x = nparts;
    if ((c == 1 || c == 2 || c == 4) && ((p * c) & 7) == 0) {
        r.path = GS_EW_PATH_COLOUR;
        r.E = 8;
        r.trips = cdiv((p * c) >> 3, (long)nparts * 256);
    } else if ((c & 3) == 0 && c <= 1024) {
        r.path = GS_EW_PATH_QUADS;
        r.E = 4;
        r.rows = 256 / (c >> 2) > 0 ? 256 / (c >> 2) : 1;
        r.trips = cdiv(p, (long)nparts * r.rows);
    } else {
        r.path = GS_EW_PATH_GENERIC;
        r.E = 1;
        r.rows = 256 / (c < 256 ? c : 256);
        r.trips = cdiv(p, (long)nparts * r.rows);
    }
}

// 0 and the route, or the error code the entry point answers with and `why`
inline int elementwise_route(const EwCall& q, const EwKnobs& k, EwRoute* route, const char** why) {
    EwRoute r;
    memset(&r, 0, sizeof(r));
    *route = r;
    const long p = q.p;
    const int c = q.c, wn = q.dtype == GS_F32 ? 4 : 8;
    auto refuse = [&](int code, const char* text) { *why = text; return code; };
    if (q.dtype != GS_F32 && q.dtype != GS_BF16) return refuse(GS_ERR_ARG, "bad dtype");
    auto stream = [&](int kernel, int E, long n) {   // a grid-stride kernel over n elements, E per thread and trip (+ a scalar tail for E = 4)
        r.kernel = kernel;
        r.E = E;
        r.grid_x = ew_grid(E == 4 ? (n >> 2) + 4 : n, k.ew_cap);
        r.grid_y = 1;
        r.trips = cdiv(E == 4 ? n >> 2 : n, (long)r.grid_x * 256);
        r.tail = E == 4 && (n & 3) != 0;
    };
    switch (q.op) {
        case GS_EW_OP_BIAS_ACT:
            if (!(p > 0 && c > 0)) return refuse(GS_ERR_ARG, "bad args");
            if ((c & 3) == 0) {
                r.kernel = GS_EW_BIAS_ACT;
                r.E = 4;
                r.grid_x = ew_grid((p * c) >> 2, k.ew_cap);
                r.trips = cdiv((p * c) >> 2, (long)r.grid_x * 256);
            } else {   // c not a multiple of 4: the 2-channel images
                r.kernel = GS_EW_BIAS_ACT_SCALAR;
                r.E = 1;
                r.grid_x = ew_grid(p * c, k.ew_cap);
                r.trips = cdiv(p * c, (long)r.grid_x * 256);
            }
            r.grid_y = 1;
            break;
        case GS_EW_OP_ACT_BWD:
        case GS_EW_OP_AXPBY:
        case GS_EW_OP_AXPBY_DEV:
            if (!(p > 0)) return refuse(GS_ERR_ARG, "bad args");
            stream(q.op == GS_EW_OP_ACT_BWD ? GS_EW_ACT_BWD : (q.op == GS_EW_OP_AXPBY ? GS_EW_AXPBY : GS_EW_AXPBY_DEV), 4, p);
            break;
        case GS_EW_OP_TANH_BWD_BWD:
            if (!(p > 0)) return refuse(GS_ERR_ARG, "bad args");
            stream(GS_EW_TANH_BWD_BWD, 1, p);
            break;
        case GS_EW_OP_UPSCALE:
            if (!(p > 0 && q.fy > 0 && q.fx > 0)) return refuse(GS_ERR_ARG, "bad args");
            stream(GS_EW_UPSCALE, 1, p);
            break;
        case GS_EW_OP_ROW_SCALE:
            if (!(q.fy > 0 && p > 0 && p % 4 == 0)) return refuse(GS_ERR_ARG, "cols must be a multiple of 4");
            r.kernel = GS_EW_ROW_SCALE;
            r.E = 4;
            r.grid_x = ew_grid(((long)q.fy * p) >> 2, k.ew_cap);
            r.grid_y = 1;
            r.trips = cdiv(((long)q.fy * p) >> 2, (long)r.grid_x * 256);
            break;
        case GS_EW_OP_CHANNEL_SUM:
            if (!(p > 0 && c > 0)) return refuse(GS_ERR_ARG, "bad args");
            channel_sum_route(p, c, r);
            break;
        case GS_EW_OP_ACT_BWD_BIAS:
            if (!(p > 0 && c > 0)) return refuse(GS_ERR_ARG, "bad args");
            if ((c & 3) != 0 || c > 1024 || 256 % (c >> 2) != 0) {   // generic shapes: two passes
                channel_sum_route(p, c, r);
                r.two_pass = 1;
            } else {
                r.kernel = GS_EW_ACT_BWD_SUM;
                r.path = GS_EW_PATH_QUADS;
                r.E = 4;
                r.rows = 256 / (c >> 2);
                ew_partials(r, channel_sum_parts(p, c), c);
                r.grid_x = r.nparts;
                r.grid_y = 1;
                r.trips = cdiv(p, (long)r.nparts * r.rows);
            }
            break;
        case GS_EW_OP_PIXEL_NORM_FWD:
        case GS_EW_OP_PIXEL_NORM_BWD:
        case GS_EW_OP_PIXEL_NORM_BWD_BIAS:
        case GS_EW_OP_PIXEL_NORM_BWD_BWD: {
            if (!(p > 0 && c >= 4 && c <= 1024 && (c & (c - 1)) == 0)) return refuse(GS_ERR_ARG, "c must be a power of two in [4,1024]");
            // a row is owned by L = min(64, c/E) lanes, E = 16 bytes of channels per lane and pass (E = 4 for bf16 rows of 4 channels),
            // P passes per row, U independent row groups per trip
            r.kernel = GS_EW_PIXEL_NORM;
            r.E = c % wn == 0 ? wn : 4;
            const int vecs = c / r.E;
            r.L = vecs < 64 ? vecs : 64;
            r.P = vecs / r.L;   // 1, 2, 4 (4: fp32 only)
            r.U = r.P == 1 ? 2 : 1;
            r.rows = 64 / r.L;
            const long rows_per_block = 4L * r.rows * r.U;
            r.grid_x = ew_grid((p + rows_per_block - 1) / rows_per_block * 256, k.ew_cap);
            r.grid_y = 1;
            if (q.op == GS_EW_OP_PIXEL_NORM_BWD_BIAS) {
                // every block ends with a cross-lane + LDS fold of its channel sums and one partial row: as many trips per block as the plain
                // pass has blocks (top level, 32 channels: 61.5 us at 8192 blocks, 50.5 at 1024 -- 42.3 without the sums; scripts/bench_ew.py)
                if (r.grid_x > k.pn_bias_cap) r.grid_x = k.pn_bias_cap;
                ew_partials(r, r.grid_x, c);
            }
            r.trips = cdiv(p, (long)r.grid_x * rows_per_block);
            break;
        }
        case GS_EW_OP_BLOCKSUM:
            if (!(p > 0 && q.fy > 0 && q.fx > 0)) return refuse(GS_ERR_ARG, "bad args");
            r.E = 1;
            r.grid_y = 1;
            if (q.fy * q.fx >= 32) {   // a wave per output element
                r.kernel = GS_EW_BLOCKSUM;
                r.grid_x = ew_grid(p * 64, k.ew_cap);
                r.trips = cdiv(p, (long)r.grid_x * 4);
                r.tail = (q.fy * q.fx) % 64 != 0;
            } else {
                r.kernel = GS_EW_BLOCKSUM_SMALL;
                r.grid_x = ew_grid(p, k.ew_cap);
                r.trips = cdiv(p, (long)r.grid_x * 256);
            }
            break;
        case GS_EW_OP_SUMSQ_ROWS: {
            if (!(q.fy > 0 && p > 0)) return refuse(GS_ERR_ARG, "bad args");
            // rows after the first start at r * cols elements: 4-element loads stay aligned only when cols % 4 == 0 or there is one row;
            // any other call reads its rows with scalar loads (the tail loop of the last chunk takes the whole row)
            const bool vec = (p & 3) == 0 || q.fy == 1;
            r.kernel = GS_EW_SUMSQ_ROWS;
            r.path = vec ? GS_EW_PATH_VECTOR : GS_EW_PATH_SCALAR;
            r.E = vec ? 4 : 1;
            r.grid_x = SSQ_CHUNKS;
            r.grid_y = q.fy;
            const long nvec = vec ? p >> 2 : 0;
            r.per = (int)((nvec + SSQ_CHUNKS - 1) / SSQ_CHUNKS);
            r.trips = vec ? cdiv(r.per, 256) : cdiv(p, 256);
            r.tail = nvec * 4 != p;
            r.ws_bytes = (size_t)q.fy * SSQ_CHUNKS * sizeof(float);
            break;
        }
        case GS_EW_OP_BATCH_STDDEV_FWD:
        case GS_EW_OP_BATCH_STDDEV_BWD:
        case GS_EW_OP_BATCH_STDDEV_BWD_BWD: {
            if (!(q.fy > 0 && q.fy % 4 == 0 && p > 0 && c > 0)) return refuse(GS_ERR_ARG, "batch must be a positive multiple of 4 (ops.py:341)");
            r.kernel = q.op == GS_EW_OP_BATCH_STDDEV_FWD ? GS_EW_BATCH_STDDEV_FWD
                                                         : (q.op == GS_EW_OP_BATCH_STDDEV_BWD ? GS_EW_BATCH_STDDEV_BWD : GS_EW_BATCH_STDDEV_BWD_BWD);
            const long npos = p * c;
            r.E = npos % wn == 0 ? wn : 1;   // VN: 16 bytes of positions per thread and member, or the scalar fallback
            r.grid_x = q.fy / 4;             // one block of 1024 threads per column of four members
            r.grid_y = 1;
            r.trips = cdiv(npos, 1024L * r.E);
            r.tail = npos % (1024L * r.E) != 0;
            break;
        }
        default:
            return refuse(GS_ERR_ARG, "bad op");
    }
    *route = r;
    return 0;
}

// the route under this process's knobs, for the entry points: 0 or the refusal, reported
inline int ew_plan(const char* who, int op, int dtype, long p, int c, int fy, int fx, EwRoute* r) {
    const char* why = "";
    const int e = elementwise_route(EwCall{op, dtype, p, c, fy, fx}, ew_knobs_env(), r, &why);
    return e ? fail(e, "%s: %s", who, why) : 0;
}

}  // namespace gs
