// C-ABI entry points of the conv family: the layer -> kernel-role relabelling (conv_role), the hand-over to the implicit GEMM (conv_igemm.hip), to
// the VALU convs (conv_thin.hip, through thin_route) or to the weight gradients (conv_wgrad.hip), the planning of gs_conv_wgrad_jobs, the host-only
// queries, and the batched weight re-layout (gs_weight_prep_batch) with its kernel -- the only kernel of this file.
#include "conv_thin_route.h"
#include <utility>
#include <vector>

namespace gs {

// from conv_igemm.hip / conv_wgrad.hip
bool igemm_norm_fused(int mode, int N, int Hb, int Wb, int IC, int OC, int dtype, int want);
int igemm_config(int mode, int N, int Hb, int Wb, int IC, int OC, int dtype, int want, int* out);
int igemm_table(int index, int* out);
extern "C" int gs_pixel_norm_bwd_bwd_fused(const void* gg, const void* g, const void* x, void* out, void* out_g, int64_t p, int c, float eps, int pre_act,
                                           int dtype, void* stream);
size_t igemm_prep_bytes(int ic, int oc, int dtype);
int run_igemm(int mode, int variant, const void* x, const float* w_hwio, void* y, int N, int Hi, int Wi, int ICk,
              int OCk, int w_ci, int w_co, int Hb, int Wb, float alpha, const float* bias, int act, int dtype, int w_prepared,
              void* ws, size_t ws_bytes, hipStream_t st, const void* mask = nullptr, int mask_act = 0, void* y2 = nullptr, float pn_eps = 0.f,
              const void* addend = nullptr, int normbwd = 0);
extern "C" int gs_pixel_norm_bwd_fused(const void* g, const void* x, const void* addend, void* gx, int64_t p, int c, float eps, int pre_act, int post_act, int dtype,
                                       void* stream);
size_t wgrad_mfma_bytes(int mode, int dtype, int N, int Hb, int Wb, int IC, int OC);
size_t wgrad_direct_bytes(int mode, int ks, int dtype, int N, int Hb, int Wb, int IC, int OC);
int run_wgrad_direct(int mode, int ks, const void* x, const void* gy, float* gw, int N, int Hi, int Wi, int IC, int OC, int Hb, int Wb, float alpha, int transpose,
                     int accumulate, int dtype, void* ws, size_t ws_bytes, hipStream_t st, GsWgradReduce* defer = nullptr);
int run_wgrad_mfma(int mode, const WgradSrcs& srcs, int nsrc, float* gw, float* gb, int N, int Hi, int Wi, int IC, int OC, int Hb,
                   int Wb, float alpha, int transpose, int accumulate, int dtype, void* ws, size_t ws_bytes, hipStream_t st,
                   GsWgradReduce* defer = nullptr);
void wgrad_sk_job_geometry(int mode, int N, SkJob& q);
void wgrad_sk_plan(int mode, SkGroup& g);
size_t wgrad_sk_bytes(const SkGroup& g);
int run_wgrad_sk(int mode, const SkGroup& g, void* ws, size_t ws_bytes, hipStream_t st);

// ------------------------------------------------------------------ batched weight re-layout
// which operand a map's entry point builds: (variant of weight_prep_kernel, fp32 storage for the direct kernels / T for MFMA)
__device__ __host__ inline void prep_plan(int map, int ci, int co, int ksize, int dtype, int* variant, bool* store_f32) {
    const bool fwd = map == GS_PREP_CONV_FWD || map == GS_PREP_CONVT_FWD;   // (a data gradient contracts the layer's output channels)
    *variant = fwd ? 0 : (map == GS_PREP_CONV_BWD_DATA ? 1 : 2);            // bwd_data, stride 1: flipped taps; stride 2: transposed-conv walk (set by the caller)
    const bool mfma = (ksize == 3 || map == GS_PREP_CONVT_BWD_DATA) && (fwd ? igemm_supported(ci, co, dtype) : igemm_supported(co, ci, dtype));   // (that map's descriptors: ksize unread, as before)
    *store_f32 = !mfma || dtype == GS_F32;
}
// One 64 x 64 (ci x co) tile of one tap per trip, staged through LDS so that both sides move whole 256-byte rows: the forward operand
// is the TRANSPOSE of the stored [ci][co] slab (a thread-per-element gather read it with a stride of co floats: 31 us per launch for the
// ~20 MB of a network, now bandwidth-bound); the data-gradient operands are (tap-flipped) copies.
static __global__ __launch_bounds__(256) void weight_prep_batch_kernel(const GsPrepDesc* __restrict__ descs) {
    __shared__ float tile[64][65];
    const GsPrepDesc d = descs[blockIdx.y];
    int variant;
    bool f32;
    prep_plan(d.map, d.ci, d.co, d.ksize, d.dtype, &variant, &f32);
    if (d.map == GS_PREP_CONV_BWD_DATA && d.stride == 2) variant = 2;
    const int taps = d.ksize * d.ksize, ci = d.ci, co = d.co;
    const int tci = (ci + 63) >> 6, tco = (co + 63) >> 6;
    const int ntiles = taps * tci * tco;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // 16 x 16 threads, 4 consecutive elements each
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int t = tl / (tci * tco), r = tl % (tci * tco);
        const int i0 = (r / tco) * 64, o0 = (r % tco) * 64;
        const float* src = d.w_hwio + (long)t * ci * co;
        if (variant == 0) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // rows i0 + ty + 16 k, columns o0 + 4 tx ..
                const int i = i0 + ty + 16 * k, o = o0 + 4 * tx;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (i < ci) {
                    if (o + 3 < co && (co & 3) == 0) { const float4 q = *reinterpret_cast<const float4*>(src + (long)i * co + o); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
                    else { for (int e = 0; e < 4; ++e) if (o + e < co) v[e] = src[(long)i * co + o + e]; }
                }
                for (int e = 0; e < 4; ++e) tile[ty + 16 * k][4 * tx + e] = v[e];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // output rows o0 + ty + 16 k, 4 consecutive input channels i0 + 4 tx ..
                const int o = o0 + ty + 16 * k, i = i0 + 4 * tx;
                if (o >= co) continue;
                float v[4];
                for (int e = 0; e < 4; ++e) v[e] = tile[4 * tx + e][ty + 16 * k];
                const long dst = ((long)t * co + o) * ci + i;
                if (i + 3 < ci && (ci & 3) == 0) {
                    if (f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.ws) + dst) = make_float4(v[0], v[1], v[2], v[3]);
                    else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(d.ws) + dst) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (i + e < ci) {
                            if (f32) reinterpret_cast<float*>(d.ws)[dst + e] = v[e];
                            else reinterpret_cast<bf16_t*>(d.ws)[dst + e] = f32_to_bf16(v[e]);
                        }
                }
            }
        } else {
            const int tt = variant == 1 ? taps - 1 - t : t;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + ty + 16 * k, o = o0 + 4 * tx;
                if (i >= ci) continue;
                const long so = (long)i * co + o, dst = (long)tt * ci * co + so;
                if (o + 3 < co && (co & 3) == 0) {
                    const float4 q = *reinterpret_cast<const float4*>(src + so);
                    if (f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.ws) + dst) = q;
                    else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(d.ws) + dst) = make_uint2(pack_bf16x2(q.x, q.y), pack_bf16x2(q.z, q.w));
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (o + e < co) {
                            if (f32) reinterpret_cast<float*>(d.ws)[dst + e] = src[so + e];
                            else reinterpret_cast<bf16_t*>(d.ws)[dst + e] = f32_to_bf16(src[so + e]);
                        }
                }
            }
        }
    }
}

extern "C" int gs_weight_prep_batch(const GsPrepDesc* descs, int n, void* stream) {
    GS_CHECK_ARG(descs != nullptr && n > 0 && n <= 65535, "weight_prep_batch: bad args");
    hipLaunchKernelGGL(weight_prep_batch_kernel, dim3(48, n), dim3(256), 0, as_stream(stream), descs);
    GS_CHECK_LAUNCH();
    return 0;
}

static int check_conv(const GsConv* c) {
    GS_CHECK_ARG(c != nullptr, "conv: no layer descriptor");
    GS_CHECK_ARG(c->n > 0 && c->h > 0 && c->w > 0 && c->ci > 0 && c->co > 0, "conv: non-positive dim");
    GS_CHECK_ARG(!c->transposed || (c->ksize == 3 && c->stride == 2), "conv: a transposed layer is 3x3 stride 2 (got %dx%d stride %d)", c->ksize, c->ksize, c->stride);
    GS_CHECK_ARG(c->ksize == 1 || c->ksize == 3, "conv: ksize %d not in {1,3}", c->ksize);
    GS_CHECK_ARG(c->stride == 1 || (c->stride == 2 && c->ksize == 3), "conv: stride %d unsupported with ksize %d", c->stride, c->ksize);
    GS_CHECK_ARG(c->stride == 1 || c->transposed || (c->h % 2 == 0 && c->w % 2 == 0), "conv: stride 2 needs even h,w (got %d,%d)", c->h, c->w);
    GS_CHECK_ARG(c->dtype == GS_F32 || c->dtype == GS_BF16, "conv: bad dtype %d", c->dtype);
    return 0;
}

// ---- THE relabelling: a layer and one of its three maps -> the roles the kernels know.  A transposed conv is the stride-2 conv with its two
// sides swapped, so every map of either kind is one of MODE_S1 / MODE_S2 / MODE_T2 over (ICk -> OCk) channels, reading Hi x Wi and walking
// the base grid Hb x Wb (the smaller side of a strided map).  Every entry point below, plan_jobs and the *_is_fused queries take their
// geometry from here and nowhere else (a valid layer is assumed: check_conv first).
struct ConvRole {
    int mode;         // MODE_*
    int variant;      // weight_prep_kernel's (fwd / bwd_data)
    int ICk, OCk;     // channels the kernel contracts / produces; bwd_weight: its input side / gradient side
    int Hi, Wi;       // what the kernel reads (bwd_weight: its input side)
    int Hb, Wb;       // base grid
    int Ho, Wo;       // what the kernel writes: the base grid, twice it in MODE_T2
    int swapped;      // bwd_weight of a transposed layer: x and gy change places and gw is stored transposed
};
static ConvRole conv_role(const GsConv& c, int map) {
    const int s = c.stride;
    ConvRole r;
    memset(&r, 0, sizeof(r));
    const bool up = c.transposed != 0;
    if (map == GS_CONV_BWD_DATA) {
        r.ICk = c.co; r.OCk = c.ci;
        if (up) { r.mode = MODE_S2; r.variant = 2; r.Hi = 2 * c.h; r.Wi = 2 * c.w; r.Hb = c.h; r.Wb = c.w; }
        else if (s == 2) { r.mode = MODE_T2; r.variant = 2; r.Hi = r.Hb = c.h / 2; r.Wi = r.Wb = c.w / 2; }
        else { r.mode = MODE_S1; r.variant = 1; r.Hi = r.Hb = c.h; r.Wi = r.Wb = c.w; }
    } else if (map == GS_CONV_BWD_WEIGHT && up) {   // the stride-2 conv from the big side to the small one
        r.mode = MODE_S2; r.swapped = 1;
        r.ICk = c.co; r.OCk = c.ci; r.Hi = 2 * c.h; r.Wi = 2 * c.w; r.Hb = c.h; r.Wb = c.w;
    } else {                                         // fwd, and the plain conv's bwd_weight
        r.mode = up ? MODE_T2 : (s == 2 ? MODE_S2 : MODE_S1);
        r.ICk = c.ci; r.OCk = c.co; r.Hi = c.h; r.Wi = c.w;
        r.Hb = up ? c.h : c.h / s; r.Wb = up ? c.w : c.w / s;
    }
    const int f = r.mode == MODE_T2 ? 2 : 1;
    r.Ho = f * r.Hb; r.Wo = f * r.Wb;
    return r;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_channel_sum_workspace_bytes(int64_t p, int c);
extern "C" int gs_channel_sum(const void* g, float* out, int64_t p, int c, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
extern "C" int gs_bias_act_fwd(const void* x, const float* bias, void* y, int64_t p, int c, int act, int dtype, void* stream);   // the epilogue of the shapes without the MFMA kernel
extern "C" int gs_act_bwd(const void* g, const void* y, void* gx, int64_t numel, int act, int dtype, void* stream);

// Does the implicit GEMM take this map of the layer (a tanh behind the conv is not among its epilogues)?  Otherwise: thin_conv below.
static bool on_igemm(const GsConv& c, const ConvRole& r, int act = GS_ACT_NONE) { return c.ksize == 3 && igemm_supported(r.ICk, r.OCk, c.dtype) && act != GS_ACT_TANH; }

static ThinCall thin_call(const GsConv& c, const ConvRole& r, int form, int act, bool has_bias, int mask_act, bool want_bits) {
    ThinCall t;
    t.mode = r.mode; t.ks = c.ksize; t.ICk = r.ICk; t.OCk = r.OCk; t.dtype = c.dtype;
    t.P = (long)c.n * r.Ho * r.Wo;
    t.form = form; t.act = act; t.has_bias = has_bias; t.mask_act = mask_act; t.want_bits = want_bits;
    return t;
}

// The optional operands of a conv outside the implicit GEMM: what rides with it (t.form says how z / addend / eps are meant)
struct ThinExtras {
    const float* bias;
    const void* mask;      // with t.mask_act: y *= mask_act'(.) through it
    const void* z;         // GS_THIN_BWD_PNBWD: the norm the gradient continues through
    const void* addend;
    float eps;
};

// Every conv the implicit GEMM does not take, for all four entry points: the fp32 weight [tap][OCk][ICk] at the start of the layer's workspace
// (prepared here unless w_prepared), the one launch thin_route chooses, then whatever of the request that kernel left open, as passes in place.
static int thin_conv(const GsConv& c, const ConvRole& r, const ThinCall& t, const void* x, const float* w_hwio, void* y, const ThinExtras& e, void* stream) {
    hipStream_t st = as_stream(stream);
    const long total = (long)c.ksize * c.ksize * c.ci * c.co;
    if (c.ws_bytes < (size_t)total * 4) return fail(GS_ERR_WORKSPACE, "conv direct: workspace %zu < %zu", c.ws_bytes, (size_t)total * 4);
    float* wp = reinterpret_cast<float*>(c.ws);
    if (!c.w_prepared) {
        hipLaunchKernelGGL((weight_prep_kernel<float>), dim3(cdiv(total, 256)), dim3(256), 0, st, w_hwio, wp, c.ksize * c.ksize, c.ci, c.co, r.variant);
        GS_CHECK_LAUNCH();
    }
    const ThinRoute route = thin_route(t, thin_knobs_env());
    ThinArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.wp = wp; a.y = y; a.bias = e.bias; a.mask = e.mask; a.mask_act = t.mask_act; a.z = e.z; a.addend = e.addend; a.eps = e.eps; a.act = t.act;
    a.bits = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(y) + (size_t)t.P * r.OCk);   // (behind the values: include/gansynth_hip.h, GS_ACT_WRITE_BITS)
    a.dtype = c.dtype; a.mode = r.mode; a.ks = c.ksize; a.N = c.n; a.Hi = r.Hi; a.Wi = r.Wi; a.ICk = r.ICk; a.OCk = r.OCk; a.Ho = r.Ho; a.Wo = r.Wo;
    a.P = t.P; a.alpha = c.alpha;
    if (int rc = run_thin(route, a, st)) return rc;
    if (t.form == GS_THIN_BWD_PNBWD)
        return route.epilogue_fused ? 0 : gs_pixel_norm_bwd_fused(y, e.z, e.addend, y, t.P, r.OCk, e.eps, GS_ACT_NONE, t.act, c.dtype, stream);
    if (!route.epilogue_fused && (e.bias || t.act != GS_ACT_NONE))
        if (int rc = gs_bias_act_fwd(y, e.bias, y, t.P, r.OCk, t.act, c.dtype, stream)) return rc;
    if (e.mask && !route.mask_fused)
        if (int rc = gs_act_bwd(y, e.mask, y, t.P * r.OCk, t.mask_act, c.dtype, stream)) return rc;
    if (t.want_bits && !route.bits_fused) return gs_pack_act_bits(y, t.P, r.OCk, c.dtype, stream);
    return 0;
}

extern "C" size_t gs_conv_workspace_bytes(const GsConv* c, int which) {
    if (check_conv(c)) return 0;
    if (which != GS_CONV_BWD_WEIGHT) return align256((size_t)c->ksize * c->ksize * c->ci * c->co * 4);   // the re-laid weight
    const ConvRole r = conv_role(*c, GS_CONV_BWD_WEIGHT);
    const size_t wg = wgrad_plan(r.mode, c->ksize, c->dtype, c->n, r.Hb, r.Wb, r.ICk, r.OCk).family >= WG_F32
                          ? wgrad_mfma_bytes(r.mode, c->dtype, c->n, r.Hb, r.Wb, r.ICk, r.OCk)
                          : wgrad_direct_bytes(r.mode, c->ksize, c->dtype, c->n, r.Hb, r.Wb, r.ICk, r.OCk);
    if (c->transposed) return wg;   // (no bias)
    const size_t cs = align256(gs_channel_sum_workspace_bytes((int64_t)c->n * r.Hb * r.Wb, c->co));   // bias-gradient fallback of gs_conv_bwd_weight
    return wg > cs ? wg : cs;
}

static int mask_fuse_min_channels() {
    static const int v = [] { const char* e = getenv("GS_MASK_FUSE_MIN_CI"); return e ? atoi(e) : 32; }();   // (env: measurement knob)
    return v;
}
static bool mask_act_ok(int a) { return a == GS_ACT_LRELU || a == GS_ACT_TANH || a == GS_ACT_LRELU_BITS; }

// y_norm (optional): y_norm = pixel_norm(act(conv + bias)) as well -- fused into the conv epilogue where the tile owns all channels of a
// pixel, a separate pass otherwise; y (the activation itself) may then be NULL
extern "C" int gs_conv_fwd(const GsConv* c, const void* x, const float* w_hwio, const float* bias, int act, void* y, void* y_norm, float eps, void* stream) {
    if (int e = check_conv(c)) return e;
    const bool want_bits = (act & GS_ACT_WRITE_BITS) != 0;   // (the caller's y has room for the sign bits behind it: include/gansynth_hip.h)
    act &= ~GS_ACT_WRITE_BITS;
    GS_CHECK_ARG(act == GS_ACT_NONE || act == GS_ACT_LRELU || act == GS_ACT_TANH, "conv_fwd: bad activation %d", act);
    GS_CHECK_ARG(!want_bits || (act == GS_ACT_LRELU && c->dtype == GS_BF16 && c->co % 32 == 0 && y && !c->transposed),
                 "conv_fwd: sign bits go with a plain conv's bf16 leaky-relu result of 32 k channels");
    GS_CHECK_ARG(y || y_norm, "conv_fwd: no output");
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    if (on_igemm(*c, r, act))
        return run_igemm(r.mode, r.variant, x, w_hwio, y, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, bias, act | (want_bits ? GS_ACT_WRITE_BITS : 0),
                         c->dtype, c->w_prepared, c->ws, c->ws_bytes, st, nullptr, 0, y_norm, eps);
    void* z = y ? y : y_norm;
    const bool bits_now = want_bits && !y_norm;   // (with a norm pass behind it the words are packed last)
    if (int e = thin_conv(*c, r, thin_call(*c, r, GS_THIN_PLAIN, act, bias != nullptr, GS_ACT_NONE, bits_now), x, w_hwio, z, ThinExtras{bias, nullptr, nullptr, nullptr, 0.f}, stream))
        return e;
    if (!y_norm) return 0;
    if (int e = gs_pixel_norm_fwd(z, y_norm, (int64_t)c->n * r.Ho * r.Wo, c->co, eps, c->dtype, stream)) return e;
    return want_bits ? gs_pack_act_bits(y, (int64_t)c->n * r.Ho * r.Wo, c->co, c->dtype, stream) : 0;
}

// y = conv(x, w) * mask_act'(.) through `mask` (an activation OUTPUT of y's shape): the second-order pass of the R1 penalty runs
// the discriminator's convs forward on cotangents and multiplies each result by the derivative of the activation that follows
// the conv; in the epilogue on the MFMA path (see gs_conv_bwd_data), in place after the conv otherwise
extern "C" int gs_conv_fwd_mask(const GsConv* c, const void* x, const float* w_hwio, const void* mask, int mask_act, void* y, void* stream) {
    if (int e = check_conv(c)) return e;
    if (c->transposed) return fail(GS_ERR_UNSUPPORTED, "conv_fwd_mask: no masked forward of a transposed layer");
    GS_CHECK_ARG(mask == nullptr || mask_act_ok(mask_act), "conv_fwd_mask: bad activation %d", mask_act);
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    const int bits_act = mask_act;   // (only the MFMA epilogue reads the sign bits; every other path reads the values they stand behind)
    if (mask_act == GS_ACT_LRELU_BITS) mask_act = GS_ACT_LRELU;
    if (!on_igemm(*c, r))   // (the colour block's streaming kernel applies the mask itself; the other VALU kernels leave it to a pass in place)
        return thin_conv(*c, r, thin_call(*c, r, mask ? GS_THIN_FWD_MASK : GS_THIN_PLAIN, GS_ACT_NONE, false, mask ? mask_act : GS_ACT_NONE, false), x, w_hwio, y,
                         ThinExtras{nullptr, mask, nullptr, nullptr, 0.f}, stream);
    const bool fused = mask != nullptr && c->co >= mask_fuse_min_channels();
    const int rc = run_igemm(r.mode, r.variant, x, w_hwio, y, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared,
                             c->ws, c->ws_bytes, st, fused ? mask : nullptr, bits_act);
    if (rc || !mask || fused) return rc;
    return gs_act_bwd(y, mask, y, (int64_t)c->n * r.Ho * r.Wo * c->co, mask_act, c->dtype, stream);
}

// gx = bwd_data(gy, w) * mask_act'(.) through `mask` (the activation OUTPUT that was the layer's input; NULL: plain)
extern "C" int gs_conv_bwd_data(const GsConv* c, const void* gy, const float* w_hwio, const void* mask, int mask_act, void* gx, void* stream) {
    if (int e = check_conv(c)) return e;
    if (c->transposed && mask) return fail(GS_ERR_UNSUPPORTED, "conv_bwd_data: no masked data gradient of a transposed layer");
    GS_CHECK_ARG(mask == nullptr || mask_act_ok(mask_act), "conv_bwd_data: bad activation %d", mask_act);
    const int bits_act = mask_act;   // (see gs_conv_fwd_mask)
    if (mask_act == GS_ACT_LRELU_BITS) mask_act = GS_ACT_LRELU;
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_BWD_DATA);
    if (!on_igemm(*c, r))   // (the mask: a pass in place behind the kernel)
        return thin_conv(*c, r, thin_call(*c, r, GS_THIN_PLAIN, GS_ACT_NONE, false, mask ? mask_act : GS_ACT_NONE, false), gy, w_hwio, gx, ThinExtras{nullptr, mask, nullptr, nullptr, 0.f},
                         stream);
    // In the epilogue the mask costs one more read of gx's size; with the mask vectors fetched ahead of the epilogue arithmetic
    // (conv_igemm.hip) that beats the separate in-place pass on every MFMA-path layer, the HBM-bound 32-channel top included
    // (+1.6 % on the step against fusing from 64 channels up).
    const bool fused = mask != nullptr && c->ci >= mask_fuse_min_channels();
    const int rc = run_igemm(r.mode, r.variant, gy, w_hwio, gx, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared,
                             c->ws, c->ws_bytes, st, fused ? mask : nullptr, bits_act);
    if (rc || !mask || fused) return rc;
    return gs_act_bwd(gx, mask, gx, (int64_t)c->n * r.Ho * r.Wo * c->ci, mask_act, c->dtype, stream);
}

// the (x, gy) pairs of one launch, as the kernels want them; for the transposed conv the roles of the two sides swap
static WgradSrcs make_srcs(const void* const* xs, const void* const* gys, int nsrc, int n_per, const int* ns, unsigned bias_mask, bool swap, int* total) {
    WgradSrcs s;
    memset(&s, 0, sizeof(s));
    int end = 0;
    for (int i = 0; i < GS_WGRAD_MAX_SRC; ++i) {
        if (i < nsrc) {
            s.x[i] = swap ? gys[i] : xs[i];
            s.gy[i] = swap ? xs[i] : gys[i];
            end += ns ? ns[i] : n_per;
        }
        s.n_end[i] = end;
    }
    s.bias_mask = bias_mask;
    *total = end;
    return s;
}

// One layer's weight gradient from several (x, gy) pairs in one launch: gw (+)= sum_s bwd_weight(xs[s], gys[s]); pair s has ns[s] images
// (ns NULL: c.n each) and bit s of bias_mask says whether it contributes to gb (ignored when gb is NULL).  The layer then costs one set of
// block partials and one slice reduction instead of one per pair.  `pending` (NULL = reduce at once): see GsWgradReduce.  c.ws is sized by
// gs_conv_workspace_bytes(GS_CONV_BWD_WEIGHT) for the total image count.
static int wgrad_layer(const GsConv& c, const void* const* xs, const void* const* gys, const int* ns, int nsrc, unsigned bias_mask, float* gw_hwio, float* gb,
                       int accumulate, GsWgradReduce* pending, void* stream) {
    if (int e = check_conv(&c)) return e;
    GS_CHECK_ARG(!(c.transposed && gb), "conv_bwd_weight: a transposed layer has no bias gradient");
    GS_CHECK_ARG(xs && gys && nsrc >= 1 && nsrc <= GS_WGRAD_MAX_SRC, "conv_bwd_weight: %d sources (1..%d)", nsrc, GS_WGRAD_MAX_SRC);
    for (int i = 0; i < nsrc; ++i) GS_CHECK_ARG(xs[i] && gys[i], "conv_bwd_weight: null source %d", i);
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(c, GS_CONV_BWD_WEIGHT);
    const WgradPlan lp = wgrad_plan(r.mode, c.ksize, c.dtype, c.n, r.Hb, r.Wb, r.ICk, r.OCk);   // (family and bias form: functions of the layer, not of n)
    const bool mfma = lp.family >= WG_F32;
    if (pending) memset(pending, 0, sizeof(*pending));
    if (!gb) bias_mask = 0;
    if (nsrc > 1 && !(mfma && (!gb || lp.fused_bias))) {
        // shapes without the multi-source kernels: one call per source (the first applies `accumulate`, the rest add)
        for (int i = 0; i < nsrc; ++i) {
            GsConv one = c;
            if (ns) one.n = ns[i];
            const int rc = wgrad_layer(one, xs + i, gys + i, nullptr, 1, 1u, gw_hwio, ((bias_mask >> i) & 1u) ? gb : nullptr, i == 0 ? accumulate : 1, nullptr, stream);
            if (rc) return rc;
        }
        return 0;
    }
    const bool fused_bias = bias_mask && lp.fused_bias;
    // the channel-sum fallback of the bias gradient reuses ws: such calls cannot leave their partials pending
    GsWgradReduce* defer = (bias_mask && !fused_bias) ? nullptr : pending;
    int rc;
    const int n0 = ns ? ns[0] : c.n;   // (the single-source paths below)
    if (mfma) {
        int total = 0;
        const WgradSrcs srcs = make_srcs(xs, gys, nsrc, c.n, ns, bias_mask, r.swapped != 0, &total);
        rc = run_wgrad_mfma(r.mode, srcs, nsrc, gw_hwio, fused_bias ? gb : nullptr, total, r.Hi, r.Wi, r.ICk, r.OCk, r.Hb, r.Wb, c.alpha, r.swapped, accumulate, c.dtype, c.ws,
                            c.ws_bytes, st, defer);
    } else {
        rc = run_wgrad_direct(r.mode, c.ksize, r.swapped ? gys[0] : xs[0], r.swapped ? xs[0] : gys[0], gw_hwio, n0, r.Hi, r.Wi, r.ICk, r.OCk, r.Hb, r.Wb, c.alpha, r.swapped,
                              accumulate, c.dtype, c.ws, c.ws_bytes, st, defer);
    }
    if (rc || !bias_mask || fused_bias) return rc;
    // shapes without the fused path: the plain channel sum (stream-ordered after the kernels above, same workspace)
    return gs_channel_sum(gys[0], gb, (int64_t)n0 * r.Hb * r.Wb, c.co, accumulate, c.dtype, c.ws, c.ws_bytes, stream);
}

extern "C" int gs_conv_bwd_weight(const GsConv* c, const void* x, const void* gy, float* gw_hwio, float* gb, int accumulate, void* stream) {
    if (int e = check_conv(c)) return e;
    return wgrad_layer(*c, &x, &gy, nullptr, 1, 1u, gw_hwio, gb, accumulate, nullptr, stream);
}

// many pending slice reductions in a handful of launches: up to GS_REDUCE_BATCH entries per launch, a new launch whenever an
// entry adds into a gradient that the current launch already touches (list order = summation order).  `pending`: host array
static int wgrad_reduce_batch(const GsWgradReduce* pending, int n, void* stream) {
    GS_CHECK_ARG(n >= 0 && (n == 0 || pending), "wgrad_reduce_batch: bad args");
    hipStream_t st = as_stream(stream);
    ReduceBatch b;
    int cnt = 0;
    long gx = 0;   // blocks of the entry that needs most (64 element quads per block with 4 slice lanes, 16 with 16: see the kernel)
    auto flush = [&]() {
        if (cnt == 0) return;
        wgrad_reduce_batch_launch(b, cnt, gx, st);
        cnt = 0;
        gx = 0;
    };
    for (int i = 0; i < n; ++i) {
        const GsWgradReduce& d = pending[i];
        if (d.nslices <= 0) continue;   // nothing pending for this call
        GS_CHECK_ARG(d.partials && d.gw && d.taps > 0 && d.ic > 0 && d.oc > 0 && (((long)d.taps * d.ic * d.oc) & 3) == 0 && (!d.gb || (d.oc & 3) == 0),
                     "wgrad_reduce_batch: entry %d is not a pending reduction", i);
        bool clash = cnt == GS_REDUCE_BATCH;
        for (int j = 0; j < cnt && !clash; ++j) clash = b.e[j].gw == d.gw || (d.gb && b.e[j].gb == d.gb);
        if (clash) flush();
        b.e[cnt++] = d;
        const long pstride = (long)d.taps * d.ic * d.oc + (d.gb ? d.oc : 0);
        const long epb = 256 / wgrad_fold_lanes(d.nslices);
        const long blocks = (pstride / 4 + epb - 1) / epb;
        if (blocks > gx) gx = blocks;
    }
    flush();
    GS_CHECK_LAUNCH();
    return 0;
}

// ---- all weight gradients of a backward pass in one call (gs_conv_wgrad_jobs): the layers the 64 x 64-tile bf16 kernel takes are
// grouped by its instantiation (the conv mode) and each group runs as ONE stream-K launch + one fold (conv_shared.h); every
// other layer goes through wgrad_layer above, its slice reduction left pending, and one wgrad_reduce_batch folds
// those at the end.  Workspace: the largest group (groups run one after the other on the stream) + the sum of the per-layer needs.
namespace gs {
struct JobPlan {
    std::vector<std::pair<int, SkGroup>> groups;   // (conv mode, group), in launch order
    std::vector<GsWgradJob> single;               // jobs on the per-layer path (one source each where the layer has no multi-source kernel)
    std::vector<size_t> single_off;               // their workspace offsets
    std::vector<std::vector<int>> group_jobs;      // per group: the index in the caller's list of each of its jobs (gs_conv_wgrad_jobs_plan)
    std::vector<std::pair<int, int>> single_src;   // per single job: (index in the caller's list, source it was split off for or -1)
    size_t group_bytes = 0, total_bytes = 0;
};
static GsConv job_conv(const GsWgradJob& jb, int n) {   // the job's layer, with n images
    GsConv c;
    memset(&c, 0, sizeof(c));
    c.n = n; c.h = jb.h; c.w = jb.w; c.ci = jb.ci; c.co = jb.co; c.ksize = jb.ksize; c.stride = jb.stride; c.transposed = jb.transposed;
    c.dtype = jb.dtype; c.alpha = jb.alpha;
    return c;
}
static int job_check(const GsWgradJob& jb, int idx) {
    GS_CHECK_ARG(jb.nsrc >= 1 && jb.nsrc <= GS_WGRAD_MAX_SRC && jb.gw, "conv_wgrad_jobs: job %d has %d sources (1..%d) / no output", idx, jb.nsrc, GS_WGRAD_MAX_SRC);
    for (int i = 0; i < jb.nsrc; ++i) GS_CHECK_ARG(jb.x[i] && jb.gy[i] && jb.n[i] > 0, "conv_wgrad_jobs: job %d, null or empty source %d", idx, i);
    GS_CHECK_ARG(!jb.transposed || (jb.ksize == 3 && jb.stride == 2 && !jb.gb), "conv_wgrad_jobs: job %d: the transposed conv is 3x3 stride 2 without bias", idx);
    GS_CHECK_ARG(jb.gw_ci_stride == 0 || (jb.gw_ci_stride >= jb.ci && !jb.transposed), "conv_wgrad_jobs: job %d: bad gw_ci_stride %d", idx, jb.gw_ci_stride);
    const GsConv c = job_conv(jb, jb.n[0]);
    return check_conv(&c);
}
static int job_total_images(const GsWgradJob& jb) {
    int t = 0;
    for (int i = 0; i < jb.nsrc; ++i) t += jb.n[i];
    return t;
}
static int plan_jobs(const GsWgradJob* jobs, int njobs, JobPlan& plan) {
    static const bool no_sk = getenv("GS_NO_WGRAD_GROUPS") != nullptr;   // measurement knob: everything on the per-layer path
    int open_idx[3] = {-1, -1, -1};   // conv mode -> index of the group still accepting jobs
    for (int i = 0; i < njobs; ++i) {
        const GsWgradJob& jb = jobs[i];
        if (int e = job_check(jb, i)) return e;
        const int total = job_total_images(jb);
        const ConvRole r = conv_role(job_conv(jb, total), GS_CONV_BWD_WEIGHT);
        const WgradPlan lp = wgrad_plan(r.mode, jb.ksize, jb.dtype, total, r.Hb, r.Wb, r.ICk, r.OCk);
        if (!no_sk && lp.family == WG_TILE64) {
            int gi = open_idx[r.mode];
            if (gi >= 0) {   // a full group, or one that already adds into this gradient, is closed (launch order = summation order)
                const SkGroup& og = plan.groups[gi].second;
                bool close = og.njobs == GS_SK_MAX_JOBS;
                for (int j = 0; j < og.njobs && !close; ++j) close = og.job[j].gw == jb.gw || (jb.gb && og.job[j].gb == jb.gb);
                if (close) gi = -1;
            }
            if (gi < 0) {
                SkGroup ng;
                memset(&ng, 0, sizeof(ng));
                plan.groups.push_back(std::make_pair(r.mode, ng));
                plan.group_jobs.push_back(std::vector<int>());
                gi = (int)plan.groups.size() - 1;
                open_idx[r.mode] = gi;
            }
            SkGroup& g = plan.groups[gi].second;
            SkJob& q = g.job[g.njobs++];
            plan.group_jobs[gi].push_back(i);
            int tot = 0;
            q.srcs = make_srcs(jb.x, jb.gy, jb.nsrc, 0, jb.n, jb.gb ? jb.bias_mask : 0u, r.swapped != 0, &tot);
            q.gw = jb.gw; q.gb = jb.gb; q.alpha = jb.alpha; q.transpose = r.swapped; q.accumulate = jb.accumulate;
            q.Hi = r.Hi; q.Wi = r.Wi; q.IC = r.ICk; q.OC = r.OCk; q.Hb = r.Hb; q.Wb = r.Wb;
            q.ICld = jb.gw_ci_stride > 0 ? jb.gw_ci_stride : r.ICk;
            wgrad_sk_job_geometry(r.mode, total, q);
        } else {
            // layers without a multi-source kernel (direct / thin kernels, fp32 bias sums): one single-source job per pair, each with its own
            // partials so that every slice reduction can stay pending
            const bool multi = lp.family >= WG_F32 && (!jb.gb || lp.fused_bias);
            if (jb.nsrc == 1 || multi) {
                plan.single.push_back(jb);
                plan.single_src.push_back(std::make_pair(i, -1));
            } else {
                for (int sidx = 0; sidx < jb.nsrc; ++sidx) {
                    GsWgradJob one = jb;
                    one.nsrc = 1;
                    one.x[0] = jb.x[sidx]; one.gy[0] = jb.gy[sidx]; one.n[0] = jb.n[sidx];
                    one.bias_mask = (jb.bias_mask >> sidx) & 1u;
                    if (!one.bias_mask) one.gb = nullptr;
                    if (sidx > 0) one.accumulate = 1;
                    plan.single.push_back(one);
                    plan.single_src.push_back(std::make_pair(i, sidx));
                }
            }
        }
    }
    for (auto& kg : plan.groups) {
        wgrad_sk_plan(kg.first, kg.second);
        const size_t b = wgrad_sk_bytes(kg.second);
        if (b > plan.group_bytes) plan.group_bytes = b;
    }
    size_t off = plan.group_bytes;
    for (const GsWgradJob& jb : plan.single) {
        const GsConv c = job_conv(jb, job_total_images(jb));
        plan.single_off.push_back(off);
        off += gs_conv_workspace_bytes(&c, GS_CONV_BWD_WEIGHT);
    }
    plan.total_bytes = off;
    return 0;
}
}  // namespace gs

extern "C" size_t gs_conv_wgrad_jobs_workspace_bytes(const GsWgradJob* jobs, int njobs) {
    if (!jobs || njobs <= 0) return 0;
    JobPlan plan;
    if (plan_jobs(jobs, njobs, plan)) return 0;
    return plan.total_bytes;
}

extern "C" int gs_conv_wgrad_jobs(const GsWgradJob* jobs, int njobs, void* ws, size_t ws_bytes, void* stream) {
    GS_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs), "conv_wgrad_jobs: bad args");
    if (njobs == 0) return 0;
    JobPlan plan;
    if (int e = plan_jobs(jobs, njobs, plan)) return e;
    if (ws_bytes < plan.total_bytes) return fail(GS_ERR_WORKSPACE, "conv_wgrad_jobs: workspace %zu < %zu", ws_bytes, plan.total_bytes);
    hipStream_t st = as_stream(stream);
    for (auto& kg : plan.groups)
        if (int e = run_wgrad_sk(kg.first, kg.second, ws, plan.group_bytes, st)) return e;
    std::vector<GsWgradReduce> pend;
    for (size_t k = 0; k < plan.single.size(); ++k) {
        const GsWgradJob& jb = plan.single[k];
        GsConv c = job_conv(jb, jb.n[0]);
        c.ws = reinterpret_cast<unsigned char*>(ws) + plan.single_off[k];
        c.ws_bytes = (k + 1 < plan.single.size() ? plan.single_off[k + 1] : plan.total_bytes) - plan.single_off[k];
        GsWgradReduce d;
        memset(&d, 0, sizeof(d));
        if (int rc = wgrad_layer(c, jb.x, jb.gy, jb.n, jb.nsrc, jb.bias_mask, jb.gw, jb.gb, jb.accumulate, &d, stream)) return rc;
        if (jb.gw_ci_stride > jb.ci) {   // a channel-slice target: only the pending (batched) fold knows the row stride
            if (d.nslices <= 0 || d.transpose) return fail(GS_ERR_UNSUPPORTED, "conv_wgrad_jobs: a %d -> %d layer cannot add into a channel slice", jb.ci, jb.co);
            d.ic_ld = jb.gw_ci_stride;
        }
        if (d.nslices > 0) pend.push_back(d);
    }
    if (!pend.empty()) return wgrad_reduce_batch(pend.data(), (int)pend.size(), stream);
    return 0;
}

// Second-order pass (the mode-seeking term differentiates the generator's backward, models.py:60): the forward conv applied to a cotangent gives
// t = the gradient w.r.t. u = act'(z) pixel_norm_bwd(g, z), the first-order backward of the block whose activation z and incoming gradient g
// are given.  Both gradients of that node in the conv's epilogue (h = t act'(z)):
//   out_g = pixel_norm_bwd(h, z)                 (w.r.t. g)          out_z = d<h, pixel_norm_bwd(g, z)>/dz      (w.r.t. z)
// where a tile owns all channels of a pixel; otherwise the conv into out_g and gs_pixel_norm_bwd_bwd_fused (out_g in place).
extern "C" int gs_conv_fwd_pnbwdbwd(const GsConv* c, const void* x, const float* w_hwio, const void* g, const void* z, int act, float eps, void* out_g, void* out_z,
                                    void* stream) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(g && z && out_g && out_z && (act == GS_ACT_NONE || act == GS_ACT_LRELU), "conv_fwd_pnbwdbwd: g, z and both outputs are required, activation none or leaky relu (got %d)", act);
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    if (on_igemm(*c, r))
        return run_igemm(r.mode, r.variant, x, w_hwio, out_g, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared, c->ws,
                         c->ws_bytes, as_stream(stream), z, act, out_z, eps, g, 2);
    if (int e = gs_conv_fwd(c, x, w_hwio, nullptr, GS_ACT_NONE, out_g, nullptr, 0.f, stream)) return e;
    return gs_pixel_norm_bwd_bwd_fused(out_g, g, z, out_z, out_g, (int64_t)c->n * r.Ho * r.Wo, c->co, eps, act, c->dtype, stream);
}
// 1 when that call runs as one launch for the layer
extern "C" int gs_conv_fwd_pnbwdbwd_is_fused(const GsConv* c) {
    if (check_conv(c) || c->ksize != 3 || !(c->transposed || c->stride == 1)) return 0;
    const ConvRole r = conv_role(*c, GS_CONV_FWD);
    return igemm_norm_fused(r.mode, c->n, r.Hb, r.Wb, r.ICk, r.OCk, c->dtype, IGEMM_NORM_BWD2) ? 1 : 0;
}

// Data gradient of a conv whose INPUT was y = pixel_norm(z), z = act(...) the previous block's activation (networks.py:41-93: every
// generator block ends conv -> leaky_relu -> pixel_norm), continued through that norm and activation in the conv's epilogue:
//   gx = (pixel_norm_bwd(B^T(gy, w), z) + addend) * act'(z)       (addend: optional second gradient into z, same shape)
// i.e. the gradient w.r.t. the previous block's pre-activation in ONE pass.  The epilogue form exists where a tile owns every channel of a
// pixel (the 32- / 64-channel layers -- where the bytes are); other shapes run the plain data gradient and gs_pixel_norm_bwd_fused in place.
extern "C" int gs_conv_bwd_data_pnbwd(const GsConv* c, const void* gy, const float* w_hwio, const void* z, const void* addend, int act, float eps, void* gx, void* stream) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(z && gx && (act == GS_ACT_NONE || act == GS_ACT_LRELU), "conv_bwd_data_pnbwd: z is required, activation none or leaky relu (got %d)", act);
    hipStream_t st = as_stream(stream);
    const ConvRole r = conv_role(*c, GS_CONV_BWD_DATA);
    const bool epilogue_map = c->transposed || c->stride == 1;   // (the stride-2 conv's data gradient, MODE_T2, has no norm epilogue)
    if (epilogue_map && on_igemm(*c, r))
        return run_igemm(r.mode, r.variant, gy, w_hwio, gx, c->n, r.Hi, r.Wi, r.ICk, r.OCk, c->ci, c->co, r.Hb, r.Wb, c->alpha, nullptr, GS_ACT_NONE, c->dtype, c->w_prepared, c->ws,
                         c->ws_bytes, st, z, act, nullptr, eps, addend, 1);
    if (!on_igemm(*c, r))   // the colour block (few -> many channels as a gradient) streams it in one pass; other shapes: the plain kernel + the norm's backward in place
        return thin_conv(*c, r, thin_call(*c, r, GS_THIN_BWD_PNBWD, act, false, GS_ACT_NONE, false), gy, w_hwio, gx, ThinExtras{nullptr, nullptr, z, addend, eps}, stream);
    if (int e = gs_conv_bwd_data(c, gy, w_hwio, nullptr, 0, gx, stream)) return e;
    return gs_pixel_norm_bwd_fused(gx, z, addend, gx, (int64_t)c->n * r.Ho * r.Wo, c->ci, eps, GS_ACT_NONE, act, c->dtype, stream);
}
// 1 when the call above runs as ONE launch for the layer (the epilogue form), 0 when it is the conv + the norm's backward in place
extern "C" int gs_conv_bwd_data_pnbwd_is_fused(const GsConv* c) {
    if (check_conv(c) || !(c->transposed || c->stride == 1)) return 0;
    const ConvRole r = conv_role(*c, GS_CONV_BWD_DATA);
    if (!on_igemm(*c, r)) return thin_route(thin_call(*c, r, GS_THIN_BWD_PNBWD, GS_ACT_NONE, false, GS_ACT_NONE, false), thin_knobs_env()).epilogue_fused;
    return igemm_norm_fused(r.mode, c->n, r.Hb, r.Wb, r.ICk, r.OCk, c->dtype, IGEMM_NORM_BWD) ? 1 : 0;
}
// Which implicit-GEMM configuration a 3x3 layer runs with (kernel-role shape: hb x wb the base grid, ic -> oc the kernel's channels; mode 0 stride
// 1, 1 stride 2, 2 transposed; want: the epilogue asked for, 0 none, 1 pixel norm, 2 / 3 its first- / second-order backward).  Host arithmetic
// only -- no launch, no device needed.  out_cfg[10]: A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC, then 1 if that configuration is compiled.
extern "C" int gs_conv_igemm_config(int mode, int n, int hb, int wb, int ic, int oc, int dtype, int want, int* out_cfg) {
    return igemm_config(mode, n, hb, wb, ic, oc, dtype, want, out_cfg);
}
// Row `index` of the table of compiled implicit-GEMM kernels (conv_igemm.hip: GS_IGEMM_CONFIGS), for tests that want one case per kernel.  Host
// only.  out11: mode, bf16_only, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC; GS_ERR_ARG past the last row.
extern "C" int gs_conv_igemm_table(int index, int* out11) { return igemm_table(index, out11); }

// Which VALU kernel a call runs (include/gansynth_hip.h), from the route the entry points above read.  Host only.
extern "C" int gs_conv_thin_route(const GsConv* c, int map, int form, int act, int has_bias, int mask_act, int want_bits, const int* caps_or_null, int* out) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(out && (map == GS_CONV_FWD || map == GS_CONV_BWD_DATA) && form >= GS_THIN_PLAIN && form <= GS_THIN_BWD_PNBWD, "conv_thin_route: bad map %d / form %d / no output", map, form);
    GS_CHECK_ARG(act >= GS_ACT_NONE && act <= GS_ACT_TANH && mask_act >= GS_ACT_NONE && mask_act <= GS_ACT_TANH, "conv_thin_route: bad activation %d / %d", act, mask_act);
    GS_CHECK_ARG(!caps_or_null || (caps_or_null[0] > 0 && caps_or_null[1] > 0), "conv_thin_route: grid caps are positive");
    // the forms as the entry points have them: a masked forward is a forward of a plain conv, the norm's backward rides on a data gradient (none / leaky relu)
    GS_CHECK_ARG(form != GS_THIN_FWD_MASK || (map == GS_CONV_FWD && !c->transposed), "conv_thin_route: a masked forward is the forward map of a plain conv");
    GS_CHECK_ARG(form != GS_THIN_BWD_PNBWD || (map == GS_CONV_BWD_DATA && act != GS_ACT_TANH), "conv_thin_route: the norm's backward goes with a data gradient, activation none or leaky relu");
    const ConvRole r = conv_role(*c, map);
    // (only gs_conv_fwd leaves the implicit GEMM for a tanh; every other entry point decides by the layer alone)
    if (on_igemm(*c, r, map == GS_CONV_FWD && form == GS_THIN_PLAIN ? act : GS_ACT_NONE)) {
        memset(out, 0, GS_THIN_ROUTE_INTS * sizeof(int));
        out[0] = -1;
        return 0;
    }
    const ThinKnobs knobs = caps_or_null ? ThinKnobs{caps_or_null[0], caps_or_null[1]} : thin_knobs_env();
    const ThinRoute t = thin_route(thin_call(*c, r, form, act, has_bias != 0, mask_act, want_bits != 0), knobs);
    static_assert(sizeof(ThinRoute) == GS_THIN_ROUTE_INTS * sizeof(int), "ThinRoute is the ints the query reports");
    memcpy(out, &t, sizeof(t));
    return 0;
}

// ---- what the weight-gradient entry points WOULD launch, asked without launching (host arithmetic on wgrad_plan / plan_jobs, the structs the
// launchers themselves read; no device needed: the CU count then defaults to 256).  tests/test_wgrad_cover_*.py key their cases by these answers.
static void layer_plan_ints(const GsConv& c, int* out) {   // c.n: images of all sources
    const ConvRole r = conv_role(c, GS_CONV_BWD_WEIGHT);
    const WgradPlan p = wgrad_plan(r.mode, c.ksize, c.dtype, c.n, r.Hb, r.Wb, r.ICk, r.OCk);
    const int v[GS_WGRAD_PLAN_INTS] = {p.family, p.mode, p.tw, p.ot, r.swapped, r.ICk, r.OCk, r.Hb, r.Wb, p.ntiles, p.nslices, p.fold, p.batch_lanes,
                                       p.fused_bias, p.tiles_x, p.tiles_y};
    memcpy(out, v, sizeof(v));
}
extern "C" int gs_conv_wgrad_plan(const GsConv* c, int* out) {
    if (int e = check_conv(c)) return e;
    GS_CHECK_ARG(out != nullptr, "conv_wgrad_plan: no output");
    layer_plan_ints(*c, out);
    return 0;
}
extern "C" int gs_conv_wgrad_jobs_plan(const GsWgradJob* jobs, int njobs, int* out, int out_len) {
    GS_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs) && out && out_len >= 2, "conv_wgrad_jobs_plan: bad args");
    JobPlan plan;
    if (njobs > 0)
        if (int e = plan_jobs(jobs, njobs, plan)) return e;
    std::vector<int> v;
    v.push_back((int)plan.groups.size());
    v.push_back((int)plan.single.size());
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const SkGroup& g = plan.groups[gi].second;
        const int head[5] = {plan.groups[gi].first, g.njobs, g.total_units, g.total_runs, g.nblocks};
        v.insert(v.end(), head, head + 5);
        for (int j = 0; j < g.njobs; ++j) {
            const int row[5] = {plan.group_jobs[gi][j], g.job[j].unit_base, g.job[j].run_base, g.job[j].ntiles, g.job[j].nct};
            v.insert(v.end(), row, row + 5);
        }
    }
    for (size_t k = 0; k < plan.single.size(); ++k) {
        int row[2 + GS_WGRAD_PLAN_INTS] = {plan.single_src[k].first, plan.single_src[k].second};
        layer_plan_ints(job_conv(plan.single[k], job_total_images(plan.single[k])), row + 2);
        v.insert(v.end(), row, row + 2 + GS_WGRAD_PLAN_INTS);
    }
    if ((int)v.size() > out_len) return fail(GS_ERR_ARG, "conv_wgrad_jobs_plan: %d ints needed, room for %d", (int)v.size(), out_len);
    memcpy(out, v.data(), v.size() * sizeof(int));
    return (int)v.size();
}
