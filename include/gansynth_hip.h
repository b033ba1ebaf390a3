/* libgansynth_hip.so -- C ABI of the MI355X (gfx950) GANSynth hot path.
 *
 * The reference (skmhrk1209/GANSynth) has no FFI layer: its boundary is the Python call
 * surface of ops.py / networks.py / spectral_ops.py / models.py, whose arithmetic runs inside
 * TensorFlow kernels.  Each entry point below replaces the TF kernel(s) behind one of those
 * reference call sites (cited as file:line relative to the reference tree); the Python host in
 * gansynth_amd/ re-exposes the reference's own function names on top of them.
 *
 * Conventions
 *  - every function returns 0 on success, a negative GS_ERR_* code otherwise;
 *    gs_last_error() returns a thread-local message for the last failure;
 *  - all pointers are DEVICE pointers owned by the caller (torch); the library never allocates,
 *    frees or synchronises on the hot path and is hipGraph-capture safe; scratch space is passed
 *    in as `ws` and sized by the matching *_workspace_bytes query;
 *  - activations are channels-last: a logical NCHW tensor [n,c,h,w] is stored [n][h][w][c]
 *    ("NHWC"); 2-D tensors are [rows][cols] row-major.  `dtype` is the storage type of
 *    activations (GS_F32 or GS_BF16); accumulation is always fp32;
 *  - parameters (weights, biases), their gradients and optimizer state are always fp32 in the
 *    reference's own layouts: conv HWIO [kh][kw][Cin][Cout], dense [in][out];
 *  - `alpha` is the equalized-learning-rate runtime scale sqrt(variance_scale / fan_in) of
 *    ops.py:154-160, applied inside the kernel;
 *  - `stream` is a hipStream_t passed as void*.
 */
#ifndef GANSYNTH_HIP_H
#define GANSYNTH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GS_F32 = 0, GS_BF16 = 1 };
enum { GS_OK = 0, GS_ERR_ARG = -1, GS_ERR_HIP = -2, GS_ERR_UNSUPPORTED = -3, GS_ERR_WORKSPACE = -4 };
enum { GS_ACT_NONE = 0, GS_ACT_LRELU = 1, GS_ACT_TANH = 2 };
/* 1-bit leaky-relu masks (bf16 activations whose channel count is a multiple of 32).  A forward conv called with `act = GS_ACT_LRELU |
 * GS_ACT_WRITE_BITS` also leaves the SIGN BITS of its result behind it: the caller's buffer holds the activation (numel values) followed by
 * numel / 8 bytes, one 32-bit word per (pixel, 32-channel tile), bit 8 (2 h + q) + k = "channel 16 q + 8 h + k of the tile is > 0".  A masked
 * conv (gs_conv_fwd_mask / gs_conv_bwd_data) called with `mask_act = GS_ACT_LRELU_BITS` is promised such a buffer as `mask` and reads
 * the words instead of the values where its epilogue can (1 / 16 of the mask bytes); everywhere else it reads the values as with GS_ACT_LRELU.
 * gs_pack_act_bits writes the words for an activation that some other kernel produced. */
enum { GS_ACT_LRELU_BITS = 5, GS_ACT_WRITE_BITS = 16 };
/* which of the three bilinear conv maps a workspace query is for */
enum { GS_CONV_FWD = 0, GS_CONV_BWD_DATA = 1, GS_CONV_BWD_WEIGHT = 2 };

const char* gs_last_error(void);
int gs_version(void);
/* number of CUs etc. are queried lazily; this forces it (and checks the device is gfx950) */
int gs_init(void);
/* n plain (normal priority, non-blocking) streams, made and destroyed around the instantiation of a hipGraph WITH PARALLEL BRANCHES.
 * The runtime hands every new stream the least-used of its GPU_MAX_HW_QUEUES hardware queues; ROCm 7.0.2's hip::GraphExec makes one
 * stream more than the branches need and hip::Graph::UpdateStreams, at every launch, skips those that share the LAUNCH stream's hardware
 * queue -- without a bounds check: two of them on that queue and hipGraphLaunch reads past the end of the list (segmentation fault,
 * profiles/r05_e_graph_replay_crash.txt).  Two consecutive new streams only land on one queue when it is at least two users short of
 * every other one; a hundred-odd throw-away streams level the pool first (each goes to the least-used queue), so the exec's streams
 * land on different queues and at most one is skipped.  The reference has no such object (one TF session, models.py:189-194). */
int gs_streams_create(int n, void** streams);
int gs_streams_destroy(int n, void** streams);

/* ---------------------------------------------------------------- profiling hooks (bench.py)
 * When enabled, every launch of conv_igemm_kernel (the MFMA implicit-GEMM conv) is bracketed by a pair of
 * HIP events on its own stream.  gs_prof_collect synchronises those events and returns the number
 * of launches, their summed duration (ms) and summed algorithmic FLOPs.
 * gs_prof_enable(n) with n > 1 = burst mode: a conv launch (a pure function of its inputs) is issued n times back to back inside
 * its event pair and the elapsed time divided by n -- the steady-state launch-to-launch time (one launch boundary included), free
 * of the host's eager-launch latency that an event pair around a single few-microsecond launch also measures. */
int gs_prof_enable(int on);
int gs_prof_collect(int* launches, double* total_ms, double* total_flops);
/* roofline accounting of the launches recorded since gs_prof_enable(1): algorithmic bytes (every operand read once, the result
 * written once) and the time the binding roof allows, summed per launch (max of flops / peak_tflops and bytes / peak_gbps);
 * roof_ms_hbm_bound = the part of it that comes from HBM-bound launches.  Call before gs_prof_collect (which resets). */
int gs_prof_roofline(double peak_tflops, double peak_gbps, double* total_bytes, double* roof_ms, double* roof_ms_hbm_bound);
/* per-launch records (implicit-GEMM convs and their weight gradients) for a per-stage roofline: duration, algorithmic FLOPs and
 * bytes, and desc[8 * i .. +8] = {kind, N, Hb, Wb, IC, OC, masked | sources, fused norm | deferred}; kind = 0 / 1 / 2 for the
 * stride-1 / stride-2 / transposed conv map (ops.py:237-243, 269-276), 10 + that for its weight gradient.  Before gs_prof_collect. */
int gs_prof_records(int max_records, int* n, double* ms, double* flops, double* bytes, int* desc);

/* ------------------------------------------------------------------------ data parallelism (new: the reference is single GPU,
 * gan_synth_main.py:91-98).  One process per GPU.  A communicator wraps ncclCommInitRank of RCCL (resolved at run
 * time from the librccl.so.1 the process already has, none needed on one GPU); the collectives run ON THE CALLER'S STREAM, i.e.
 * ordered behind the backward that produced the gradients and ahead of gs_adam_tf_step, with no cross-stream event.
 *   gs_comm_available   0 when librccl can be resolved in this process (no communicator is created): lets every rank agree that the
 *                       blocking gs_comm_init will be entered by ALL of them before any of them enters it
 *   gs_comm_unique_id   rank 0 fills 128 bytes (ncclGetUniqueId) and ships them to the other ranks by any means
 *   gs_comm_init        every rank, same id; binds to the current HIP device
 *   gs_allreduce_sum_f32 / gs_broadcast_f32   in place, fp32 (the flat gradient / parameter buffers of models.py:67-89's two
 *                       optimizers; the 1 / world averaging is gs_adam_tf_step's grad_scale) */
#define GS_COMM_ID_BYTES 128
typedef struct gs_comm gs_comm;
int gs_comm_available(void);
int gs_comm_unique_id(void* id128);
int gs_comm_init(gs_comm** out, int rank, int world, const void* id128);
int gs_comm_destroy(gs_comm* comm);
int gs_comm_count(gs_comm* comm, int* ranks);   /* ncclCommCount: the ranks the communicator was built over (bench.py reports it as rccl_ranks) */
int gs_allreduce_sum_f32(gs_comm* comm, float* data, int64_t count, void* stream);
/* test hook, ONE-rank communicators only (RCCL short-cuts their all-reduce to nothing): from now on gs_allreduce_sum_f32 launches a one-block
 * kernel that holds the stream for `us` microseconds instead (us < 0: off again) -- where a collective sits in a captured graph then shows as time */
int gs_comm_set_marker_us(gs_comm* comm, double us);
int gs_broadcast_f32(gs_comm* comm, float* data, int64_t count, int root, void* stream);

/* ------------------------------------------------------------------------------- conv2d / conv2d_transpose
 * tf.nn.conv2d NCHW/HWIO padding=SAME (ops.py:237-243) with ksize in {1,3}, stride in {1,2} (stride 2 only with ksize 3; TF SAME on
 * an even input pads 0 before / 1 after), and tf.nn.conv2d_transpose NCHW, 3x3, stride 2, SAME, output = 2h x 2w (ops.py:266-276: the
 * gradient-of-conv definition out[2i+k] += x[i] * w[k][ci][co], cropped at the end).
 *   conv:        x [n][h][w][ci]  w [k][k][ci][co] fp32  y [n][h/stride][w/stride][co]
 *   transposed:  x [n][h][w][ci]  w [3][3][ci][co] fp32 (the STORED variable of ops.py:259-265)  y [n][2h][2w][co]
 * A GsConv names the LAYER, in its own forward labelling, whichever of its three maps is asked for:
 *   fwd       : y = alpha * conv(x, w)
 *   bwd_data  : gx[n][h][w][ci] = alpha * d<gy, conv(x,w)>/dx
 *   bwd_weight: gw[k][k][ci][co] = alpha * d<gy, conv(x,w)>/dw   (fp32 out)
 * The maps are closed under differentiation (each one's gradient is another one), which is how the Python host gets the second-order
 * terms of models.py:47,60 -- and the transposed layer's maps are the stride-2 conv's with the two sides swapped, run by the same
 * kernels: its fwd is that conv's bwd_data, its bwd_data that conv's fwd, its bwd_weight that conv's with x and gy exchanged, stored
 * transposed.  The library does that relabelling in one place (conv_api.hip: conv_role).
 * fwd / bwd_data first re-lay the weight into the kernel operand at the start of `ws`; `w_prepared` != 0 says that `ws` still holds
 * that operand from an earlier call with the same weight values (same map, dtype), so the re-layout is skipped -- the caller keeps one
 * persistent ws per (weight, map) between optimizer steps.  `ws` is sized by gs_conv_workspace_bytes for the map.
 * Every gradient-of-a-parameter entry point (bwd_weight, dense_bwd_weight, channel_sum, act_bwd_bias) takes `accumulate`: 0 overwrites
 * the output, 1 adds into it (tf.gradients sums the contributions of a variable used several times; accumulating in the producing
 * kernel replaces one read-modify-write pass per contribution). */
typedef struct GsConv {
    int32_t n, h, w;             /* the layer's forward INPUT (a transposed layer's small side) */
    int32_t ci, co, ksize, stride;
    int32_t transposed;          /* != 0: the transposed conv (ksize 3, stride 2 only) */
    int32_t dtype, w_prepared;
    float alpha;
    void* ws;
    size_t ws_bytes;
} GsConv;
size_t gs_conv_workspace_bytes(const GsConv* c, int which);   /* which: GS_CONV_*; 0 for a layer the entry points refuse */
/* y = act(alpha * conv(x, w) + bias): the bias add + activation the reference applies right after (ops.py:244-246 + tf.nn.leaky_relu /
 * tf.nn.tanh in networks.py) ride in the GEMM epilogue; bias may be NULL, act GS_ACT_NONE.  With y_norm a generator block in one call
 * (networks.py:44-61: conv -> leaky_relu -> pixel_norm): y_norm = pixel_norm(y, eps) over the channels (ops.py:330), fused into the
 * conv epilogue where a tile owns every channel of a pixel (co = 32 / 64 on the MFMA path), a separate pass otherwise; y may then be
 * NULL when the caller keeps no copy of the activation (inference, the no-grad generator pass of the D run). */
int gs_conv_fwd(const GsConv* c, const void* x, const float* w_hwio, const float* bias, int act, void* y, void* y_norm, float eps, void* stream);
int gs_pack_act_bits(void* z, int64_t p, int c, int dtype, void* stream);   /* z: [p][c] values followed by p * c / 8 bytes (written here); c % 32 == 0 */
/* The forward map on a cotangent: y = conv(x, w) * act'(.)|mask with mask (an activation OUTPUT) of y's shape -- the second-order pass
 * of a gradient penalty runs the convs forward on cotangents; each result meets the derivative of the activation that follows that
 * conv.  mask NULL: the plain forward.  Plain convs only (GS_ERR_UNSUPPORTED for a transposed layer). */
int gs_conv_fwd_mask(const GsConv* c, const void* x, const float* w_hwio, const void* mask, int mask_act, void* y, void* stream);
/* The data gradient, optionally multiplied by the derivative of the activation that PRODUCED the layer's input, expressed through that
 * input itself: gx = bwd_data(gy, w) * act'(.)|mask  (mask = x of the forward, gx's shape; mask_act = LRELU, TANH or LRELU_BITS) -- the
 * gradient w.r.t. the previous layer's pre-activation in one pass.  mask NULL: plain; a mask is refused for a transposed layer. */
int gs_conv_bwd_data(const GsConv* c, const void* gy, const float* w_hwio, const void* mask, int mask_act, void* gx, void* stream);
/* Data gradient continued through the PREVIOUS block's pixel norm and activation (networks.py:41-93: conv -> leaky_relu -> pixel_norm;
 * the backward tf.gradients builds for ops.py:330-333 behind ops.py:237-243 / 269-276), one pass where a tile owns all channels of a pixel:
 *   gx = (pixel_norm_bwd(B^T(gy, w), z) + addend) * act'(z);  z: the previous block's activation output (gx's shape), addend: optional
 * gs_conv_bwd_data_pnbwd_is_fused: 1 when that is one launch for the layer, 0 when it runs as the plain data gradient followed by
 * gs_pixel_norm_bwd_fused in place. */
int gs_conv_bwd_data_pnbwd(const GsConv* c, const void* gy, const float* w_hwio, const void* z, const void* addend, int act, float eps, void* gx, void* stream);
int gs_conv_bwd_data_pnbwd_is_fused(const GsConv* c);
/* Second-order pass of the mode-seeking term (models.py:57-64: tf.gradients of tf.gradients(fake_images, [latents])): the conv applied to a cotangent
 * yields t = the gradient w.r.t. u = act'(z) pixel_norm_bwd(g, z) (a block's first-order backward); with h = t act'(z) the epilogue writes
 *   out_g = pixel_norm_bwd(h, z)   and   out_z = d<h, pixel_norm_bwd(g, z)>/dz      (g, z, out_g, out_z: the conv's output shape)
 * in one pass where a tile owns all channels of a pixel (gs_conv_fwd_pnbwdbwd_is_fused), else as the conv + gs_pixel_norm_bwd_bwd_fused. */
int gs_conv_fwd_pnbwdbwd(const GsConv* c, const void* x, const float* w_hwio, const void* g, const void* z, int act, float eps, void* out_g, void* out_z, void* stream);
int gs_conv_fwd_pnbwdbwd_is_fused(const GsConv* c);
/* One layer's weight gradient from one (x, gy) pair, at once (a backward pass that wants all of them goes through gs_conv_wgrad_jobs).
 * gb (optional, plain convs only): the bias gradient of the block, gb[co] (+)= sum_{n,h,w} gy (fp32; no alpha) -- for bf16 3x3 convs the
 * sum rides along in the same two launches (one extra MFMA per 16 pixels against an all-ones operand), other shapes fall back to
 * gs_channel_sum inside.  `accumulate` applies to gw and gb alike. */
int gs_conv_bwd_weight(const GsConv* c, const void* x, const void* gy, float* gw_hwio, float* gb, int accumulate, void* stream);
/* Which implicit-GEMM tile configuration a 3x3 layer runs with, asked without running it: host arithmetic only, works without a device (the CU
 * count then defaults to the MI355X's 256).  Kernel-role arguments: mode 0 stride 1 / 1 stride 2 / 2 transposed, hb x wb the base grid (the smaller
 * side of a strided map), ic -> oc the channels the kernel contracts / produces; want: the epilogue asked for, 0 none, 1 pixel norm, 2 / 3 its
 * first- / second-order backward.  out_cfg[10] = A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC (conv_igemm.hip: IgemmCfg) and 1 if that
 * configuration is compiled for the dtype; NORM == want says the epilogue is fused, 0 that the norm runs as its own pass. */
int gs_conv_igemm_config(int mode, int n, int hb, int wb, int ic, int oc, int dtype, int want, int* out_cfg);
/* The table of compiled implicit-GEMM kernels, row by row (conv_igemm.hip: GS_IGEMM_CONFIGS): out11 = mode, bf16_only (1: compiled for bf16 alone,
 * 0: for fp32 and bf16), then A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC as above.  0 for 0 <= index < number of rows, GS_ERR_ARG past the end.  Host
 * only: no launch, no device.  tests/test_igemm_cover_*.py run one case per row and dtype. */
int gs_conv_igemm_table(int index, int* out11);
/* Which VALU kernel a conv call outside the implicit GEMM would run -- the 1x1 colour convs, the one-output-channel gradients of the stddev plane, the
 * generic direct conv -- asked without running it: host arithmetic on the very route the entry points and the launcher read (csrc/conv_thin_route.h),
 * no launch, no device.  map: GS_CONV_FWD or GS_CONV_BWD_DATA of layer c; form: what is asked of that map -- GS_THIN_PLAIN (gs_conv_fwd,
 * gs_conv_bwd_data), GS_THIN_FWD_MASK (gs_conv_fwd_mask with mask_act), GS_THIN_BWD_PNBWD (gs_conv_bwd_data_pnbwd; act: none or leaky relu); act,
 * has_bias, want_bits: the epilogue asked for.  caps_or_null: {grid cap of EXPAND, of REDUCE}, NULL for the environment's (GS_THIN_EXPAND_BLOCKS,
 * GS_THIN_REDUCE_BLOCKS: 2048, 4096).  out[GS_THIN_ROUTE_INTS] =
 *    0 kernel   GS_THIN_* below; -1 (and nothing else) when the call belongs to the implicit GEMM -- decided as the form's entry point decides: a tanh
 *               behind the conv takes only gs_conv_fwd off it.  GS_ERR_ARG for a map / form / activation no entry point has
 *    1 C        the few-channel side as a template constant: input channels of EXPAND / EXPAND_PNBWD, output channels of REDUCE
 *    2 ACT, 3 MASKED (EXPAND, REDUCE),   4 LC (REDUCE: lanes per pixel as a constant, 0 = run time),   5 OCV, 6 VEC (DIRECT)
 *    7 grid (blocks of 256 threads),   8 pixels per block pass (DIRECT: 0)
 *    9 full four-pass trips (EXPAND, REDUCE), 10 single passes a block makes
 *   11 epilogue fused (bias + activation, or the norm's backward), 12 mask fused, 13 sign bits fused: what the kernel does of the request itself;
 *      the entry point adds the rest as passes of their own. */
enum { GS_THIN_EXPAND = 0, GS_THIN_REDUCE = 1, GS_THIN_EXPAND_PNBWD = 2, GS_THIN_SINGLE3 = 3, GS_THIN_SINGLE = 4, GS_THIN_DIRECT = 5 };
enum { GS_THIN_PLAIN = 0, GS_THIN_FWD_MASK = 1, GS_THIN_BWD_PNBWD = 2 };
#define GS_THIN_ROUTE_INTS 14
int gs_conv_thin_route(const GsConv* c, int map, int form, int act, int has_bias, int mask_act, int want_bits, const int* caps_or_null, int* out);

/* Every conv weight gradient of a backward pass in ONE call -- where `minimize` asks for the gradients of all variables of a
 * network at once (models.py:81-89).  A job is one layer (h, w, ci, co, ksize, stride, transposed as in GsConv; a transposed layer has no
 * bias) with up to GS_WGRAD_MAX_SOURCES (x, gy) pairs of n[s] images each -- the real and the fake pass of the discriminator, the second-order
 * contribution of a gradient penalty: gw (+)= sum_s bwd_weight(x[s], gy[s]), bit s of bias_mask says whether pair s contributes to gb.
 * bf16 layers with >= 64 channels on both sides are grouped by kernel instantiation and each
 * group runs as one stream-K launch over the pixel tiles of all its layers + one fold: partials = blocks + (layer, channel tile)
 * runs per GROUP instead of blocks per layer, summed in a fixed order (deterministic).  Other layers take the per-layer path with
 * their reductions batched at the end.  Jobs that add into the same gw are applied in list order.  `jobs` is a host array. */
#define GS_WGRAD_MAX_SOURCES 4
typedef struct GsWgradJob {
    const void* x[GS_WGRAD_MAX_SOURCES];
    const void* gy[GS_WGRAD_MAX_SOURCES];
    int32_t n[GS_WGRAD_MAX_SOURCES];
    int32_t nsrc;
    uint32_t bias_mask;     /* which pairs contribute to gb */
    float* gw;              /* [k][k][ci][co] fp32 */
    float* gb;              /* optional [co] */
    int32_t h, w, ci, co, ksize, stride, transposed;
    float alpha;
    int32_t accumulate, dtype;
    int32_t gw_ci_stride;   /* 0, or the input-channel count of the stored variable when gw is the slice [:, :, lo:lo+ci, :] of a
                             * wider one (the 257-channel conv of the last discriminator block, networks.py:174-176): element
                             * (t, i, o) lives at gw[(t * gw_ci_stride + i) * co + o].  Grouped (stream-K) layers and layers whose slice reduction stays
                             * pending (the 1-channel direct kernel). */
} GsWgradJob;
size_t gs_conv_wgrad_jobs_workspace_bytes(const GsWgradJob* jobs, int njobs);
int gs_conv_wgrad_jobs(const GsWgradJob* jobs, int njobs, void* ws, size_t ws_bytes, void* stream);
/* Size the weight-gradient launches of the calls that follow for `cap` CUs instead of the whole chip (0: the whole chip); returns the
 * previous setting.  For a call whose launches run on a forked branch of a hipGraph beside a latency-bound chain of few-block kernels,
 * which then finds CUs to land on.  Host-side state, read when a launch is planned (workspace query and launch alike). */
int gs_wgrad_cu_cap(int cap);
/* What gs_conv_bwd_weight would launch for a layer, asked without launching: host arithmetic on the very plan the launcher reads, no device
 * needed (the CU count then defaults to the MI355X's 256; gs_wgrad_cu_cap is honoured).  out[GS_WGRAD_PLAN_INTS] =
 *    0 family   GS_WGRAD_DIRECT / THIN (the VALU kernels of the 1- / 2-channel layers), F32, BF16, THIN_DMA, TILE64 (the MFMA kernels)
 *    1 mode     0 stride 1, 1 stride 2 (a transposed layer runs as the stride-2 kernel with its sides swapped)
 *    2 TW       pixel-tile width of an MFMA kernel (16 / 32), 0 otherwise
 *    3 OT       32-channel output tiles per block (TILE64: 2 on both sides); THIN: 1 when x is the wide side, 0 when gy is
 *    4 swapped  1: x and gy change places and gw is stored transposed (the transposed layer)
 *    5-8        kernel-role ICk, OCk, Hb, Wb (what the kernel contracts / the gradient side / the base grid)
 *    9 ntiles   pixel tiles over all images (DIRECT / THIN: output pixels),   10 nslices: block partials the fold sums
 *   11 fold     the fold run at once: 0 the scalar kernel, else its slice lanes (4 / 16)
 *   12 batch    slice lanes of the batched fold when the reduction is left pending (gs_conv_wgrad_jobs); 0: it cannot be deferred
 *   13 bias     1: the kernel produces the bias gradient on the side,   14-15 tiles_x, tiles_y (MFMA)
 * c->n counts the images of all sources. */
enum { GS_WGRAD_DIRECT = 0, GS_WGRAD_THIN = 1, GS_WGRAD_F32 = 2, GS_WGRAD_BF16 = 3, GS_WGRAD_THIN_DMA = 4, GS_WGRAD_TILE64 = 5 };
#define GS_WGRAD_PLAN_INTS 16
int gs_conv_wgrad_plan(const GsConv* c, int* out);
/* What gs_conv_wgrad_jobs would do with a job list (same planning code, nothing dereferenced, nothing launched).  out, a stream of ints:
 *   ngroups, nsingle,
 *   per stream-K group: mode, njobs, total_units, total_runs, nblocks, then per job: index in `jobs`, unit_base, run_base, ntiles, nct
 *   per per-layer job:  index in `jobs`, the source it was split off for (-1: the whole job), then the GS_WGRAD_PLAN_INTS of gs_conv_wgrad_plan.
 * Returns the number of ints written (>= 2), or a negative GS_ERR_* (GS_ERR_ARG when out_len is too small). */
int gs_conv_wgrad_jobs_plan(const GsWgradJob* jobs, int njobs, int* out, int out_len);

/* Refreshing many prepared weight operands in one launch (after an optimizer step: ~60 conv maps, one kernel instead of
 * one re-layout launch in front of each conv).  A descriptor names the fp32 HWIO master weight, the persistent workspace
 * of one (weight, map) pair and the map: GS_PREP_* below, (ci, co, ksize, stride) of the variable, activation dtype.
 * gs_weight_prep_batch writes exactly what the map's entry point would write with w_prepared = 0, so the next call of that
 * entry point may pass w_prepared = 1.  `descs` lives in DEVICE memory (n descriptors). */
enum { GS_PREP_CONV_FWD = 0, GS_PREP_CONV_BWD_DATA = 1, GS_PREP_CONVT_FWD = 2, GS_PREP_CONVT_BWD_DATA = 3 };
typedef struct GsPrepDesc {
    const float* w_hwio; /* master weight [k][k][ci][co] */
    void* ws;            /* the map's workspace (operand at its start) */
    int32_t map, ci, co, ksize, stride, dtype;
} GsPrepDesc;
int gs_weight_prep_batch(const GsPrepDesc* descs, int n, void* stream);

/* -------------------------------------------------------------------------------- dense
 * tf.matmul (ops.py:197).  A GsDense names the LAYER, whichever of its three maps is asked for:
 *   fwd       : y[b][out] = act(alpha * x[b][in] @ w[in][out] + bias)   (split-K partials live in ws)
 *   bwd_data  : gx[b][in] = alpha * gy @ w^T
 *   bwd_weight: gw[in][out] (+)= alpha * x^T @ gy   (fp32 out)
 * fwd is ops.py:183-201 as the reference calls it -- dense, bias_add, activation (networks.py:185-187: the discriminator's 8192 -> 256 dense
 * + leaky_relu and its 256 -> 61 logits layer): bias (may be NULL) and activation (GS_ACT_NONE: none) are applied where the forward writes
 * its result (the split-K finalize pass or the direct store): one or two launches instead of three.  fp32: the same operations in the
 * same order as the plain product + gs_bias_act_fwd (bit-identical); bf16: one rounding instead of two.
 * c, hw != 0: the INPUT side is in channels-last memory -- x / gx are the [b][hw][c] memory of an activation whose tf.layers.flatten
 * (NCHW: column c * hw + p, networks.py:185) feeds the layer, in == c * hw, w stays [c * hw][out] as stored.  The flatten is a row-index
 * map inside the kernels -- no NCHW copy of the activation, no copy of its gradient back.  Vector-path shapes only (fwd: in % 4 == 0 and
 * out % 32 == 0; bwd_data: out % 256 == 0; bwd_weight: out % 256 == 0 and b <= 16; GS_ERR_UNSUPPORTED otherwise). */
typedef struct GsDense {
    int32_t b, in, out;
    int32_t c, hw;               /* != 0: the input side is a channels-last [b][hw][c] activation, in == c * hw, weight rows in NCHW-flatten order */
    int32_t dtype;
    float alpha;
    void* ws;                    /* fwd only, sized by gs_dense_fwd_workspace_bytes */
    size_t ws_bytes;
} GsDense;
size_t gs_dense_fwd_workspace_bytes(const GsDense* d);   /* 0 for a layer gs_dense_fwd refuses */
int gs_dense_fwd(const GsDense* d, const void* x, const float* w, const float* bias, int act, void* y, void* stream);
int gs_dense_bwd_data(const GsDense* d, const void* gy, const float* w, void* gx, void* stream);
int gs_dense_bwd_weight(const GsDense* d, const void* x, const void* gy, float* gw, int accumulate, void* stream);
/* Which kernel a map of layer d would run, asked without running it: host arithmetic on the very route the three entry points read
 * (csrc/dense_route.h), no launch, no device.  map: GS_DENSE_MAP_*; no_mfma_or_minus1: the GS_NO_DENSE_MFMA switch as 0 / 1, -1 for the
 * process's environment.  A layer the map's entry point refuses is refused here with the same code.  out[GS_DENSE_ROUTE_INTS] =
 *    0 kernel   GS_DENSE_* below, one per kernel template (GS_DENSE_FINALIZE never leads a route: see 9)
 *    1 FB, 2 WPR          template constants: batch rows per pass of the FAST kernels (8 / 16 / 24), waves per weight row of BWD_DATA_FAST
 *                         (1 / 4); 0 where the kernel has none
 *    3 step, 4 passes     batch rows per launch, launches over the batch
 *    5 grid x, 6 grid y   blocks of 256 threads
 *    7 ksplit, 8 ipb      fwd: slices of the reduction, input rows per slice (no split: 1, in); the gradients: 0
 *    9 finalize           a GS_DENSE_FINALIZE launch follows: it folds the ksplit partials and applies alpha, bias and activation
 *   10, 11 ws_bytes       fwd: what gs_dense_fwd_workspace_bytes answers, low word first */
enum { GS_DENSE_MAP_FWD = 0, GS_DENSE_MAP_BWD_DATA = 1, GS_DENSE_MAP_BWD_WEIGHT = 2 };
enum { GS_DENSE_FWD = 0, GS_DENSE_FWD_SMALL = 1, GS_DENSE_FWD_FAST = 2, GS_DENSE_FWD_MFMA = 3, GS_DENSE_FINALIZE = 4, GS_DENSE_BWD_DATA = 5,
       GS_DENSE_BWD_DATA_WIDE = 6, GS_DENSE_BWD_DATA_FAST = 7, GS_DENSE_BWD_DATA_MFMA = 8, GS_DENSE_BWD_WEIGHT = 9, GS_DENSE_BWD_WEIGHT_FAST = 10 };
#define GS_DENSE_ROUTE_INTS 12
int gs_dense_route(const GsDense* d, int map, int no_mfma_or_minus1, int* out);

/* tf.nn.embedding_lookup(w*alpha, argmax(labels,1)) (ops.py:217): idx[b] are the argmax indices.
 * fwd: y[b][units] = alpha * w[idx[b]][:]  ; bwd: gw[rows][units] = alpha * scatter_add(gy) (gw zero-filled here).
 * gs_embedding_fwd clamps an index outside [0, rows) to the nearest valid row (idx < 0 reads row 0, idx >= rows reads row rows - 1);
 * gs_embedding_bwd adds nothing for such an index. */
int gs_embedding_fwd(const int64_t* idx, const float* w, void* y, int b, int rows, int units, float alpha, int dtype, void* stream);
/* ... with the row index taken from the one-hot input itself (ops.py:207: tf.argmax of the inputs; first maximum), written to idx_out[b]
 * for gs_embedding_bwd: labels [b][rows] of `dtype`, y [b][units] of `dtype` */
int gs_embedding_onehot_fwd(const void* labels, const float* w, void* y, int64_t* idx_out, int b, int rows, int units, float alpha, int dtype, void* stream);
int gs_embedding_bwd(const int64_t* idx, const void* gy, float* gw, int b, int rows, int units, float alpha, int dtype, void* stream);

/* ----------------------------------------------------- bias / activations (channels-last)
 * tf.nn.bias_add + tf.nn.leaky_relu(alpha=0.2) / tf.nn.tanh (ops.py:244-246, networks.py:55,66,106 ...).
 *   y[p][c] = act(x[p][c] + bias[c])        (bias may be NULL)
 *   act_bwd : gx = g * act'(.) expressed through the activation OUTPUT y
 *   tanh_bwd_bwd: second-order term d/dy [g*(1-y^2)] . gg = -2*y*g*gg  (lrelu has none)
 *   channel_sum: out[c] = sum_p g[p][c] (bias gradient, fp32 out) */
int gs_bias_act_fwd(const void* x, const float* bias, void* y, int64_t p, int c, int act, int dtype, void* stream);
int gs_act_bwd(const void* g, const void* y, void* gx, int64_t numel, int act, int dtype, void* stream);
/* The generator's first block, networks.py:41-56 (dense -> tf.reshape to [n, c, h, w] -> leaky_relu): the dense layer's units are channel-major
 * (unit u = ch * hw + p), activations here are channels-last -- the reorder rides in the bias / activation pass.
 *   gs_units_bias_act_to_nhwc: z[n][p][ch] = act(y[n][u] + bias[u]) (mask NULL), or y[n][u] * act'(mask[n][p][ch]) (second-order pass)
 *   gs_nhwc_act_bwd_to_units:  gu[n][u] = g[n][p][ch] * act'(z[n][p][ch])  (the backward, in the units' order for gs_dense_bwd_*) */
int gs_units_bias_act_to_nhwc(const void* y, const float* bias, const void* mask, void* z, int n, int c, int hw, int act, int dtype, void* stream);
int gs_nhwc_act_bwd_to_units(const void* g, const void* z, void* gu, int n, int c, int hw, int act, int dtype, void* stream);

/* act_bwd and the bias gradient in one pass: gx = g*act'(y), gb[c] = sum_p gx[p][c] (ws: gs_channel_sum_workspace_bytes).  The sums are taken
 * over the fp32 values as computed, before a bf16 gx is rounded -- also for the shapes that take two passes (c % 4 != 0, c > 1024, 256 % (c/4) != 0). */
int gs_act_bwd_bias(const void* g, const void* y, void* gx, float* gb, int64_t p, int c, int act, int accumulate, int dtype,
                    void* ws, size_t ws_bytes, void* stream);
int gs_tanh_bwd_bwd(const void* gg, const void* g, const void* y, void* out, int64_t numel, int dtype, void* stream);
size_t gs_channel_sum_workspace_bytes(int64_t p, int c);
int gs_channel_sum(const void* g, float* out, int64_t p, int c, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
/* Deferred folds of the bias gradients (the variable gradients of models.py:81-89 are only read after the whole backward).  With
 * GS_SUM_PARTIALS or-ed into `accumulate`, gs_channel_sum / gs_act_bwd_bias / gs_pixel_norm_bwd_fused_bias leave their per-block
 * partial rows in `ws` (the caller's own buffer of gs_bias_partial_rows(...) x c floats, alive until the fold) and do not touch
 * gb; gs_channel_fold_batch then folds every pending gradient in ONE launch (two when a producer left more than 64 rows), in
 * the order the immediate fold uses (bit-identical).  gs_bias_partial_rows == 0: that shape is summed directly whatever the flag. */
#define GS_SUM_PARTIALS 2
enum { GS_BIAS_FROM_CHANNEL_SUM = 0, GS_BIAS_FROM_ACT_BWD = 1, GS_BIAS_FROM_PIXEL_NORM_BWD = 2 };
typedef struct GsFoldJob {
    const float* part; /* [nparts][c] partial rows */
    float* out;        /* [c] */
    int32_t nparts, c;
    int32_t accumulate; /* 1: out += sum */
    int32_t reserved;
} GsFoldJob;
int gs_bias_partial_rows(int producer, int64_t p, int c, int dtype);
size_t gs_channel_fold_batch_workspace_bytes(const GsFoldJob* jobs, int njobs);
int gs_channel_fold_batch(const GsFoldJob* jobs, int njobs, void* ws, size_t ws_bytes, void* stream);

/* pixel_normalization (ops.py:330-333): y = x / sqrt(mean_c(x^2) + eps), per row p over c.
 *   bwd      : gx = r*(g - y*mean_c(y*g)),  r = rsqrt(mean_c(x^2)+eps)
 *   bwd_bwd_x: d<gg, bwd(g,x)>/dx = (r^2/C) * (-(gg.g) y - (y.g) gg - (y.gg) g + 3 (y.gg)(y.g) y / C)
 *   (d<gg, bwd(g,x)>/dg = bwd(gg, x): the Jacobian is symmetric) */
int gs_pixel_norm_fwd(const void* x, void* y, int64_t p, int c, float eps, int dtype, void* stream);
/* The generator blocks are conv -> activation -> pixel norm, i.e. the norm's input x is an activation OUTPUT.  The passes
 * that surround the norm's gradients fold into them (act'(.) is expressed through x; act = NONE / LRELU / TANH):
 *   bwd_fused    : gx = (pixel_norm_bwd(g * pre_act'(x), x) + addend) * post_act'(x)      (addend may be NULL)
 *     post_act  -> gradient w.r.t. the pre-activation (replaces the act_bwd pass that follows);
 *     addend    -> a second gradient arriving at x (from the second-order graph), summed in the same pass;
 *     pre_act   -> the transposed form, used when this chain is itself differentiated (mode-seeking term)
 *   bwd_bwd_fused: out = pixel_norm_bwd_bwd(gg', g, x) with gg' = gg * pre_act'(x); out_g (may be NULL) = pixel_norm_bwd(gg', x)
 *                  -- both gradients of a differentiated norm-backward node from one pass over gg, g, x */
int gs_pixel_norm_bwd_fused(const void* g, const void* x, const void* addend, void* gx, int64_t p, int c, float eps, int pre_act, int post_act,
                            int dtype, void* stream);
/* ... the same pass also sums its result over the pixels: gb[c] (+)= sum_p gx[p][c] -- the bias gradient of the block
 * z = act(conv + bias) whose output x is (networks.py:80-87: conv_transpose -> bias -> leaky_relu -> pixel_norm); one partial row per block
 * in ws, folded in a fixed order */
size_t gs_pixel_norm_bwd_bias_workspace_bytes(int64_t p, int c, int dtype);
int gs_pixel_norm_bwd_fused_bias(const void* g, const void* x, const void* addend, void* gx, float* gb, int64_t p, int c, float eps, int pre_act,
                                 int post_act, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
int gs_pixel_norm_bwd_bwd_fused(const void* gg, const void* g, const void* x, void* out, void* out_g, int64_t p, int c, float eps, int pre_act,
                                int dtype, void* stream);

/* upscale2d / downscale2d (ops.py:283-305).
 *   upscale : y[n][h*fy][w*fx][c] = x[n][h][w][c]                       (bit-exact copy)
 *   blocksum: y[n][h/fy][w/fx][c] = scale * sum_{fy x fx block} x        (scale = 1/(fy*fx) is avg_pool;
 *             scale = 1 is the adjoint of upscale) */
int gs_upscale2d(const void* x, void* y, int n, int h, int w, int c, int fy, int fx, float scale, int dtype, void* stream);
int gs_blocksum2d(const void* x, void* y, int n, int h, int w, int c, int fy, int fx, float scale, int dtype, void* stream);

/* batch_stddev (ops.py:336-348), groups = 4: x [b][h][w][c] -> y [b][h][w][1], b % 4 == 0.
 *   bwd: gx from gy ; bwd_bwd: (ggy, gx2) = gradients of <ggx, bwd(gy, x)> w.r.t. gy and x. */
int gs_batch_stddev_fwd(const void* x, void* y, int b, int hw, int c, float eps, int dtype, void* stream);
/* (addend, optional: the other gradient into x -- that of the conv beside the statistic, networks.py:174-176 -- added in the same pass) */
int gs_batch_stddev_bwd(const void* gy, const void* x, const void* addend, void* gx, int b, int hw, int c, float eps, int dtype, void* stream);
int gs_batch_stddev_bwd_bwd(const void* ggx, const void* gy, const void* x, void* ggy, void* gx2,
                            int b, int hw, int c, float eps, int dtype, void* stream);

/* lerp (networks.py:10-11) and generic fused axpby: out = ca*a + cb*b. */
int gs_axpby(const void* a, const void* b, void* out, int64_t numel, float ca, float cb, int dtype, void* stream);
/* The same with the two coefficients read from a device table (coef[ia], coef[ib]): a fade-in weight that changes every step
 * must not be frozen into a captured hipGraph as a by-value scalar. */
int gs_axpby_dev(const void* a, const void* b, void* out, int64_t numel, const float* coef, int ia, int ib, int dtype, void* stream);

/* per-sample sum of squares (the R1 penalty reduction, models.py:48): out[r] = sum_j x[r][j]^2 (fp32 out);
 * row_scale: out[r][j] = s[r] * x[r][j]  (its gradient, s fp32). */
size_t gs_sumsq_rows_workspace_bytes(int rows);
int gs_sumsq_rows(const void* x, float* out, int rows, int64_t cols, int dtype, void* ws, size_t ws_bytes, void* stream);
int gs_row_scale(const void* x, const float* s, float alpha, void* out, int rows, int64_t cols, int dtype, void* stream);   /* out[r][:] = alpha s[r] x[r][:] */

/* Which kernel an elementwise / row-reduction call above would run, asked without running it: host arithmetic on the very route the entry
 * points, the two workspace functions and gs_bias_partial_rows read (csrc/elementwise_route.h), no launch, no device.  The shape words by op:
 *    BIAS_ACT, CHANNEL_SUM, ACT_BWD_BIAS, PIXEL_NORM_*    p rows of c channels
 *    ACT_BWD, TANH_BWD_BWD, AXPBY, AXPBY_DEV              p = numel
 *    UPSCALE, BLOCKSUM                                    p = OUTPUT elements, fy x fx the factors
 *    ROW_SCALE, SUMSQ_ROWS                                p = cols, fy = rows
 *    BATCH_STDDEV_*                                       p = hw, c, fy = batch
 * The two grid caps (GS_EW_GRID_CAP, GS_PN_BIAS_GRID_CAP) as positive values, -1 for the process's environment.  A call its entry point refuses
 * is refused here with the same code.  out[GS_EW_ROUTE_INTS] =
 *    0 kernel             GS_EW_* below, one per kernel template
 *    1 path               GS_EW_PATH_*: the branch inside channel_sum_kernel (colour / quads / generic) and sumsq_rows_kernel (vector / scalar
 *                         rows: rows > 1 with cols % 4 != 0 would break the alignment of the 4-element loads and are read element by element)
 *    2 E                  elements per lane and access: 4, 8 (16 bytes of bf16: pixel norm, stddev VN), 1 scalar
 *    3 P, 4 U, 5 L        pixel norm: passes per row, row groups per trip, lanes per row
 *    6 rows               pixel norm: rows per wave; channel_sum / act_bwd_sum: row lanes per block
 *    7 grid x, 8 grid y   blocks
 *    9 trips              loop trips of the busiest thread (channel sums: rows a row lane visits)
 *   10 tail               a sub-vector tail runs (act_bwd, axpby, sumsq_rows) / the last trip is partial (blocksum wave, stddev, channel_sum rows)
 *   11 nparts             partial rows left for the fold = gs_bias_partial_rows; 12 levels: finalize launches that follow (0, 1, 2)
 *   13 per                sumsq_rows: 4-element vectors per chunk
 *   14 two_pass           ACT_BWD_BIAS: the channel sum this route describes, over g * act'(y) as computed, then a gs_act_bwd launch over p * c elements
 *   15 reserved; 16, 17 ws_bytes: what the op's workspace function answers, low word first */
enum { GS_EW_OP_BIAS_ACT = 0, GS_EW_OP_ACT_BWD = 1, GS_EW_OP_TANH_BWD_BWD = 2, GS_EW_OP_AXPBY = 3, GS_EW_OP_AXPBY_DEV = 4, GS_EW_OP_UPSCALE = 5,
       GS_EW_OP_ROW_SCALE = 6, GS_EW_OP_CHANNEL_SUM = 7, GS_EW_OP_ACT_BWD_BIAS = 8, GS_EW_OP_PIXEL_NORM_FWD = 9, GS_EW_OP_PIXEL_NORM_BWD = 10,
       GS_EW_OP_PIXEL_NORM_BWD_BIAS = 11, GS_EW_OP_PIXEL_NORM_BWD_BWD = 12, GS_EW_OP_BLOCKSUM = 13, GS_EW_OP_SUMSQ_ROWS = 14,
       GS_EW_OP_BATCH_STDDEV_FWD = 15, GS_EW_OP_BATCH_STDDEV_BWD = 16, GS_EW_OP_BATCH_STDDEV_BWD_BWD = 17 };
enum { GS_EW_BIAS_ACT = 0, GS_EW_BIAS_ACT_SCALAR = 1, GS_EW_ACT_BWD = 2, GS_EW_TANH_BWD_BWD = 3, GS_EW_AXPBY = 4, GS_EW_AXPBY_DEV = 5, GS_EW_UPSCALE = 6,
       GS_EW_ROW_SCALE = 7, GS_EW_CHANNEL_SUM = 8, GS_EW_CHANNEL_SUM_ROWS = 9, GS_EW_ACT_BWD_SUM = 10, GS_EW_PIXEL_NORM = 11, GS_EW_BLOCKSUM = 12,
       GS_EW_BLOCKSUM_SMALL = 13, GS_EW_SUMSQ_ROWS = 14, GS_EW_BATCH_STDDEV_FWD = 15, GS_EW_BATCH_STDDEV_BWD = 16, GS_EW_BATCH_STDDEV_BWD_BWD = 17 };
enum { GS_EW_PATH_NONE = 0, GS_EW_PATH_COLOUR = 1, GS_EW_PATH_QUADS = 2, GS_EW_PATH_GENERIC = 3, GS_EW_PATH_VECTOR = 4, GS_EW_PATH_SCALAR = 5 };
#define GS_EW_ROUTE_INTS 18
int gs_elementwise_route(int op, int dtype, int64_t p, int c, int fy, int fx, int ew_grid_cap_or_minus1, int pn_bias_grid_cap_or_minus1, int* out);

/* The two GAN losses (models.py:39-65) with their gradients, one launch each.  logits / labels [n][c] in the activation dtype,
 * labels one-hot (real_logit_i = sum_c logits[i][c] * labels[i][c] = tf.gather_nd(logits, tf.where(labels))):
 *   L_D = mean_i [ softplus(-r_i) + softplus(f_i) + penalty_weight penalty_i ]     penalty: optional (R1 term: sum of squared gradients per example), fp32 [n]
 *   L_G = mean_i [ softplus(-f_i) + weight / (sumsq_i + eps) ]       sumsq: optional, sum((d sum(G(z)) / d z_i)^2), fp32 [n]
 * loss: fp32 scalar; g_*: d loss / d logits ([n][c], activation dtype), g_sumsq: d L_G / d sumsq (fp32 [n]); g_penalty: d L_D / d penalty = penalty_weight / n (fp32 [n], written when penalty is given).
 * Either half of a sum may be ABSENT (real_logits or fake_logits NULL with its g_*; for L_G fake_logits NULL with sumsq given, c = 1): a run that
 * keeps two independent passes on two streams takes the loss as two launches, each the partial mean over its own terms -- the gradients are the same
 * numbers, and no pass waits for the other's forward before its backward starts. */
int gs_gan_d_loss(const void* real_logits, const void* fake_logits, const void* labels, const float* penalty, float penalty_weight, int n, int c,
                  float* loss, void* g_real, void* g_fake, float* g_penalty, int dtype, void* stream);
int gs_gan_g_loss(const void* fake_logits, const void* labels, const float* sumsq, float weight, float eps, int n, int c, float* loss,
                  void* g_fake, float* g_sumsq, int dtype, void* stream);

/* tf.train.AdamOptimizer step (models.py:67-89), TF form, fused over one flat fp32 buffer:
 *   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ; p -= lr_t * m / (sqrt(v) + eps),
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller; grad_scale multiplies g first (1/world).
 * All-zero elements (p = g = m = v = +0.0: the padding between the tensors of a flat buffer) stay +0.0.
 * Refused by the three entry points (GS_ERR_ARG, nothing launched): numel <= 0, a null p, g, m or v, one of them off a 16-byte
 * boundary (the kernel reads and writes them as float4), and for gs_adam_tf_step_dev a null lr_t_dev. */
int gs_adam_tf_step(float* p, const float* g, float* m, float* v, int64_t numel, float lr_t, float beta1,
                    float beta2, float eps, float grad_scale, void* stream);
/* the same step, and g is cleared behind it: tf.gradients starts every run from zero (models.py:81-89 builds the sums anew), the
 * flat gradient buffers are accumulated into across a run, so the update hands the next run a zeroed buffer without a fill pass */
int gs_adam_tf_step_zero_grad(float* p, float* g, float* m, float* v, int64_t numel, float lr_t, float beta1,
                              float beta2, float eps, float grad_scale, void* stream);
/* the same step with lr_t READ FROM DEVICE MEMORY at execution time (`lr_t_dev[0]`, written by the caller stream-ordered ahead of the
 * launch): a by-value scalar would be frozen into a captured hipGraph, and with the optimizer step inside the iteration's graph no eager
 * launch is left between the two runs of models.py:191-192.  A NEGATIVE value means "no step pending": every buffer is left untouched
 * (the first replay of a graph that starts with the PREVIOUS iteration's update).  zero_grad != 0: g is cleared behind the update. */
int gs_adam_tf_step_dev(float* p, float* g, float* m, float* v, int64_t numel, const float* lr_t_dev, float beta1,
                        float beta2, float eps, float grad_scale, int zero_grad, void* stream);

/* The averaged generator: one step of tf.train.ExponentialMovingAverage over a flat fp32 buffer, TF's assign_sub form
 *   shadow -= (shadow - p) * one_minus_decay          (one_minus_decay = 1 - decay_t, computed and rounded to fp32 by the caller)
 * per element in fp32 with TWO roundings: the difference d = shadow - p, then one fused multiply-add fma(-one_minus_decay, d, shadow).
 * |shadow - p| beyond FLT_MAX overflows as it does in TF; a NaN or an infinity in p reaches the shadow at that element only.
 * one_minus_decay must lie in [0, 1]; with exactly 0 nothing is launched and the shadow keeps every bit.
 * Refused (GS_ERR_ARG, nothing launched): numel <= 0, a null pointer, a pointer that is not 16-byte aligned, shadow == p or any overlap
 * of the two ranges, one_minus_decay outside [0, 1] (NaN included).  12 bytes of traffic per element. */
int gs_ema_step(float* shadow, const float* p, int64_t numel, float one_minus_decay, void* stream);
/* the same step with the scalar READ FROM DEVICE MEMORY at execution time, under the contract of gs_adam_tf_step_dev: written by the
 * caller stream-ordered ahead of the launch, so that the step can be a node of a captured hipGraph; a NEGATIVE value means "no step
 * pending" and the launch leaves the shadow untouched (so does 0, and anything else that is not > 0).  Values above 1 are the caller's
 * error and are not detected.  Same refusals, and a null one_minus_decay_dev. */
int gs_ema_step_dev(float* shadow, const float* p, int64_t numel, const float* one_minus_decay_dev, void* stream);
/* a and b exchange their contents in place, word by word: no arithmetic, NaN payloads and the sign of zero survive.  Swapping the live
 * weights with their average keeps every pointer a captured graph holds valid and needs no third buffer.  Same refusals (a == b). */
int gs_swap_f32(float* a, float* b, int64_t numel, void* stream);

/* ------------------------------------------------------------------------------ spectral
 * spectral_ops.py:45-94.  Plan = immutable per-device tables (Hann window, twiddles, CSR mel matrix
 * supplied by the caller as built by linear_to_mel_weight_matrix, dense pinv for the inverse). */
typedef struct gs_spectral_plan gs_spectral_plan;
int gs_spectral_plan_create(gs_spectral_plan** plan, int frame_length, int frame_step, int time_steps,
                            const float* mel_dense /* host [nbins][nbins] */, const float* mel_pinv /* host, may be NULL */);
int gs_spectral_plan_destroy(gs_spectral_plan* plan);
/* stage-wise entry points (parity tests) */
int gs_stft_fwd(const gs_spectral_plan* plan, const float* wave, int batch, int wave_len, int front_pad,
                float* magnitude, float* phase, void* stream);           /* [b][T][nbins] each, DC dropped */
int gs_mel_project(const gs_spectral_plan* plan, const float* in, float* out, int64_t rows, void* stream);
int gs_if_unwrap(const gs_spectral_plan* plan, const float* mel_phase, float* mel_if, int batch, void* stream);
/* fused: waveform -> (log-mel, IF) written as one channels-last image [b][T][nbins][2] */
int gs_stft_mel_if_fwd(const gs_spectral_plan* plan, const float* wave, int batch, int wave_len, int front_pad,
                       void* images, int dtype, void* ws, size_t ws_bytes, void* stream);
size_t gs_stft_mel_if_workspace_bytes(const gs_spectral_plan* plan, int batch);
/* inverse (spectral_ops.py:97-149): images [b][T][nbins][2] -> wave [b][wave_len] */
int gs_mel_if_to_waveform(const gs_spectral_plan* plan, const void* images, int batch, int wave_len, int front_pad,
                          float* wave, int dtype, void* ws, size_t ws_bytes, void* stream);
size_t gs_mel_if_to_waveform_workspace_bytes(const gs_spectral_plan* plan, int batch);
/* The measurement switches of the spectral kernels, as the library reads them from the environment (once per process; GS_SPECTRAL_GENERIC
 * when a plan is created): generic GS_SPECTRAL_GENERIC, fp32_gemm GS_INVERSE_FP32_GEMM, mag_6terms GS_INVERSE_MAG_6TERMS, gemm_256
 * GS_INVERSE_GEMM_256, gemm_kb GS_INVERSE_GEMM_KB (default 4), gemm_kb3 GS_INVERSE_GEMM_KB3 (default 2), block_fft GS_INVERSE_BLOCK_FFT,
 * separate_ola GS_INVERSE_SEPARATE_OLA. */
typedef struct GsSpectralKnobs {
    int32_t generic, fp32_gemm, mag_6terms, gemm_256, gemm_kb, gemm_kb3, block_fft, separate_ola;
} GsSpectralKnobs;
enum { GS_SPEC_FWD_GENERIC = 0, GS_SPEC_FWD_WAVE = 1 };
enum { GS_SPEC_GEMM_NONE = 0, GS_SPEC_GEMM_F32_64 = 1, GS_SPEC_GEMM_F32_128 = 2, GS_SPEC_GEMM_SPLIT_ALL = 3, GS_SPEC_GEMM_SPLIT_TWO = 4,
       GS_SPEC_GEMM_WIDE_256 = 5 };
enum { GS_SPEC_ISTFT_NONE = 0, GS_SPEC_ISTFT_WAVE_OLA = 1, GS_SPEC_ISTFT_WAVE_FRAMES = 2, GS_SPEC_ISTFT_BLOCK_FFT = 3 };
/* Which kernels a spectral call runs: the one decision the plan, the launchers and the workspace queries read. */
typedef struct GsSpectralRoute {
    int64_t fwd_workspace_bytes;   /* what gs_stft_mel_if_workspace_bytes answers: wave path 4 KB per run, generic path the mel phases */
    int32_t fwd_kind;              /* GS_SPEC_FWD_*: stft_wave_kernel, or stft_kernel + if_unwrap_kernel */
    int32_t maxnz, mz;             /* ELL width of the mel tables, and the stft_kernel<.., 1, MZ> instantiation (0: run-time width) */
    int32_t mel_cnt[8];            /* 1024 bins: longest run of non-zeros per 128-column block of the mel matrix (0 otherwise) */
    int32_t runs, q, rem;          /* wave path: runs per example, frames per run, runs with one frame more */
    int32_t exchange;              /* wave path, fused: neighbouring runs exchange their edge phases (else every run recomputes its lead frame) */
    int32_t span_examples;         /* wave path: runs < waves per block, a block holds runs of several examples */
    int32_t gemm_kind;             /* GS_SPEC_GEMM_* of the pinv(mel) contraction (NONE: the plan has no pinv) */
    int32_t gemm_launches;         /* 1 or 2 (magnitude rows, then phase rows) */
    int32_t gemm_nj[2], gemm_np[2], gemm_kb[2];   /* gemm_bf16x6_kernel<NJ, NP, KB> per launch (0 for the fp32 kernels) */
    int32_t istft_kind;            /* GS_SPEC_ISTFT_* */
    int32_t reserved;
} GsSpectralRoute;
/* What the spectral entry points would run for a geometry, asked without a plan and without a device: host arithmetic on the very
 * function the launchers read.  mel_dense as for gs_spectral_plan_create; fwd_ws_bytes: the workspace gs_stft_mel_if_fwd would be
 * given; knobs NULL: the process's environment.  out[count]: the routes of the batch sizes batch, batch + 1 ... batch + count - 1 (the
 * matrix is read once per call). */
int gs_spectral_route(int frame_length, int frame_step, int time_steps, const float* mel_dense, int has_pinv, int batch, int count,
                      int wave_len, int front_pad, int dtype, size_t fwd_ws_bytes, const GsSpectralKnobs* knobs, GsSpectralRoute* out);

/* ------------------------------------------------------------------- pitch classifier, forward (GANSynth.evaluate)
 * The ResNet of networks.py:293-413 (pitch_classifier_main.py:39-50: 7x7 stem, 3x3 max pool, four stages of pre-activation residual
 * blocks with group normalisation and weight-standardised convs, global mean, dense logits).  Its 3x3 convs are gs_conv_fwd
 * with alpha = 1 on standardised weights, its logits gs_dense_fwd; the entry points below are the rest.  Deterministic:
 * fixed-order reductions, no float atomics.
 *   weight_standardize  ops.py:53-66 on an HWIO weight viewed as [fan_in][co]: per output channel (w - mean) / sqrt(var + eps),
 *                       population variance; fp32 in, fp32 out (run once per loaded weight set, not per batch)
 *   resnet_stem_pool    conv 7x7 stride 2, 2 -> co = 64 channels, + bias, TF SAME on h, w multiples of 4 (2 before / 3 after), then
 *                       max pool 3x3 stride 2 SAME (0 before / 1 after): x [n][h][w][2] -> y_pool [n][h/4][w/4][64] in one kernel,
 *                       the stem output never leaves the CU; y_stem [n][h/2][w/2][64] (optional) receives it anyway (tests)
 *   max_pool2d          ops.py:308-316 with kernel 3x3, stride 2, SAME on even h, w: x [n][h][w][c] -> y [n][h/2][w/2][c]
 *   conv1x1_fwd         the projection shortcut (networks.py:320-330): y = x[:, ::stride, ::stride, :] @ w [ci][co], no bias;
 *                       stride 1 or 2, ci % 32 == 0, co % 64 == 0
 *   group_norm_stats    ops.py:120-146, statistics only: stats [n][groups][2] = (mean, 1 / sqrt(var + eps)) per (image, group) over
 *                       hw * c / groups values (Welford within a thread, Chan merges in a fixed order).  addend (optional): the
 *                       statistics are of x + addend, which is written to `sum` in the same pass (the residual add of a block)
 *   group_norm_apply    y = (x - mean) * rstd * gamma[c] + beta[c], then relu when `relu` != 0 (networks.py:316-320,338-342)
 *   group_norm_relu_mean  the head (networks.py:396-402): features [n][c] fp32 = mean over hw of relu(group_norm(x)); c % 64 == 0
 * x / y / sum: [n][hw][c] channels-last in `dtype`; gamma, beta: [c] fp32. */
int gs_weight_standardize(const float* w, float* out, int fan_in, int co, float eps, void* stream);
int gs_resnet_stem_pool(const void* x, const float* w_hwio, const float* bias, void* y_stem, void* y_pool, int n, int h, int w, int co,
                        int dtype, void* stream);
int gs_max_pool2d(const void* x, void* y, int n, int h, int w, int c, int dtype, void* stream);
int gs_conv1x1_fwd(const void* x, const float* w_io, void* y, int n, int h, int w, int ci, int co, int stride, int dtype, void* stream);
size_t gs_group_norm_workspace_bytes(int n, int hw, int c, int groups);
int gs_group_norm_stats(const void* x, const void* addend, void* sum, float* stats, int n, int hw, int c, int groups, float eps, int dtype,
                        void* ws, size_t ws_bytes, void* stream);
int gs_group_norm_apply(const void* x, const float* stats, const float* gamma, const float* beta, void* y, int n, int hw, int c, int groups,
                        int relu, int dtype, void* stream);
int gs_group_norm_relu_mean(const void* x, const float* stats, const float* gamma, const float* beta, float* features, int n, int hw, int c,
                            int groups, int dtype, void* stream);

/* ------------------------------------------------------------------- pitch classifier, training (models.py:253-299)
 * The backward of the entry points above, softmax cross-entropy and tf.train.MomentumOptimizer.  The 3x3 convs and the logits layer
 * reuse gs_conv_bwd_data, gs_conv_bwd_weight and gs_dense_bwd_* on the standardised weights with alpha = 1.  Deterministic:
 * fixed-order reductions, no float atomics.  `accumulate` != 0: the result is added into its target.
 *   group_norm_relu_bwd       y = relu(group_norm(x)): from x, its stats, gamma, beta and gy -> dx (+ addend, the identity-shortcut
 *                             gradient of a pre-activation block), dgamma [c], dbeta [c] (folded over the images in order).  The ReLU
 *                             mask is recomputed with gs_group_norm_apply's expression.  c / groups <= 64
 *   group_norm_relu_mean_bwd  the head: the same from d features [n][c] fp32 (every pixel receives d features / hw)
 *   weight_standardize_batch  every row of a descriptor table (DEVICE memory) in one launch: out = standardised w (bit-identical to
 *                             gs_weight_standardize), rstd [co] = 1 / sqrt(var + eps).  max_co: the widest weight of the table
 *   weight_standardize_bwd_batch  gw = (gout - mean(gout) - out mean(gout out)) rstd per output channel; gout is cleared behind it
 *   max_pool2d_bwd            3x3 stride 2 SAME on any h, w (odd sizes pad 1 / 1): a window's gradient goes to its first maximum in
 *                             row-major order; x [n][h][w][c], gy [n][ceil(h/2)][ceil(w/2)][c] -> gx
 *   resnet_stem_bwd_weight    the 7x7 / 2 stem: x [n][h][w][2], d stem [n][h/2][w/2][64] -> gw [7][7][2][64], gb [64] (fp32 FMA, K split
 *                             over blocks, folded in order)
 *   conv1x1_bwd_data / _weight  the projection shortcut, stride 1 or 2, ci and co multiples of 64: gx [n][h][w][ci] (pixels the stride
 *                             skips are zero, or untouched when accumulating); gw [ci][co]
 *   softmax_xent              loss[0] = mean_n xent(logits_n, labels_n), dlogits (optional) its gradient, correct[0] = rows whose
 *                             argmax equals the labels' argmax; logits, labels [n][c] fp32
 *   momentum_tf_step          over a flat fp32 buffer of n (multiple of 4) elements: g += weight_decay p on [decay_lo, decay_hi),
 *                             accum = momentum accum + g, p -= lr g + lr momentum accum (nesterov) or lr accum; g cleared when
 *                             zero_grad; l2 (optional) receives sum p^2 / 2 over the decayed range at the pre-update values */
typedef struct GsWsDesc {
    const float* w;   /* [fan_in][co] */
    float* out;       /* standardised copy */
    float* rstd;      /* [co] */
    float* gout;      /* gradient w.r.t. out (backward: read, then cleared) */
    float* gw;        /* gradient w.r.t. w (backward: written) */
    int32_t fan_in, co;
} GsWsDesc;
size_t gs_group_norm_bwd_workspace_bytes(int n, int hw, int c, int groups);
int gs_group_norm_relu_bwd(const void* x, const float* stats, const float* gamma, const float* beta, const void* gy, const void* addend, void* dx,
                           float* dgamma, float* dbeta, int n, int hw, int c, int groups, int accumulate, int dtype, void* ws, size_t ws_bytes,
                           void* stream);
int gs_group_norm_relu_mean_bwd(const void* x, const float* stats, const float* gamma, const float* beta, const float* gfeatures, void* dx,
                                float* dgamma, float* dbeta, int n, int hw, int c, int groups, int accumulate, int dtype, void* ws, size_t ws_bytes,
                                void* stream);
int gs_weight_standardize_batch(const GsWsDesc* descs, int n, int max_co, float eps, void* stream);
int gs_weight_standardize_bwd_batch(const GsWsDesc* descs, int n, int max_co, void* stream);
int gs_max_pool2d_bwd(const void* x, const void* gy, void* gx, int n, int h, int w, int c, int dtype, void* stream);
size_t gs_resnet_stem_bwd_weight_workspace_bytes(int n, int h, int w);
int gs_resnet_stem_bwd_weight(const void* x, const void* gstem, float* gw, float* gb, int n, int h, int w, int co, int accumulate, int dtype,
                              void* ws, size_t ws_bytes, void* stream);
int gs_conv1x1_bwd_data(const void* gy, const float* w_io, void* gx, int n, int h, int w, int ci, int co, int stride, int accumulate, int dtype,
                        void* stream);
size_t gs_conv1x1_bwd_weight_workspace_bytes(int n, int h, int w, int ci, int co, int stride);
int gs_conv1x1_bwd_weight(const void* x, const void* gy, float* gw, int n, int h, int w, int ci, int co, int stride, int accumulate, int dtype,
                          void* ws, size_t ws_bytes, void* stream);
int gs_softmax_xent(const float* logits, const float* labels, float* loss, float* dlogits, int* correct, int n, int c, void* stream);
size_t gs_momentum_workspace_bytes(int64_t n);
int gs_momentum_tf_step(float* p, float* g, float* accum, int64_t n, int64_t decay_lo, int64_t decay_hi, float weight_decay, float lr,
                        float momentum, int nesterov, int zero_grad, float* l2, void* ws, size_t ws_bytes, void* stream);

/* ---- TensorBoard summaries (models.py:131-161, :327-354: tf.summary.image / tf.summary.audio with max_outputs = 4) -------------------
 * What a summary step sends to the host is quantised on the device: 8-bit image planes and 16-bit PCM, not activations.
 *
 * summary_image_u8: tf.summary.image's rule for float input, per image and per channel plane.  x: [n][p][c] (p = h*w pixels, c = 1 or 2
 * interleaved channels -- the channels-last [B,2,T,F] images give both planes in one pass), out: [n][c][p] uint8.  Of a plane, lo / hi
 * are the min / max over its FINITE values; lo < 0: m = max(|lo|, |hi|), scale = m < 1e-6 ? 0 : 127 / m, offset = 128; else
 * scale = hi < 1e-6 ? 0 : 255 / hi, offset = 0.  A finite v becomes (uint8) trunc(fl(fl(v * scale) + offset)), a non-finite v 255.
 * fp32 throughout, the divide correctly rounded, the multiply and the add rounded separately (no FMA); bf16 widens exactly.
 * Two launches, no atomics (ws: per-slab (min, max) pairs, sized by the query; 0 for a shape the entry point refuses).
 *
 * summary_audio_s16: TF's FloatToInt16Sample.  x: [n] rows of l samples, `row_stride` elements apart; out: [n][l] int16,
 * s = clamp(roundf(x * 32768), -32768, 32767), roundf rounding halves away from zero; NaN -> 0 (TF leaves it undefined).
 * GS_ERR_ARG without a launch: c outside {1, 2}, n <= 0, a workspace that is too small. */
size_t gs_summary_image_u8_workspace_bytes(int n, int64_t p, int c);
int gs_summary_image_u8(const void* x, uint8_t* out, int n, int64_t p, int c, int dtype, void* ws, size_t ws_bytes, void* stream);
int gs_summary_audio_s16(const void* x, int16_t* out, int n, int64_t l, int64_t row_stride, int dtype, void* stream);

/* ---- Note sequences: the mixdown of generated notes into one clip (GANSynth.synthesize; this project's own rules, DESIGN.md "Note
 * sequences") ---------------------------------------------------------------------------------------------------------------------
 * waves: [rows] generated notes of `length` fp32 samples, `row_stride` elements apart.  notes: a DEVICE table sorted by onset.  Note n
 * sounds on the clip's samples onset <= t < onset + hold + release as waves[row][k], k = t - onset, under the envelope
 *     env(k) = 1 for k < hold,   (release - (k - hold)) / (release + 1) for hold <= k < hold + release
 * (a linear ramp that would reach 1 at k = hold - 1 and 0 at k = hold + release), and
 *     mix[t] = sum over the covering notes, in ascending table order, of (gain * env(k)) * waves[row][k]
 * in fp32, every product and sum rounded on its own (no FMA), env's quotient as a multiplication by fl(1 / (release + 1)).  A sample
 * no note covers is 0 (out arrives uninitialised).  peak = max |mix[t]| (exact).  out = mix / peak (correctly rounded) when
 * `normalize` and peak > 1, else mix.  pcm (or NULL): summary_audio_s16's rule applied to out.  peak (or NULL): [1].
 * Gather form, no atomics: a block owns GS_MIX_TILE consecutive samples and finds the notes that reach into them by two binary
 * searches on the onsets.  Two launches: the mix with one |max| per block into ws (sized by the query), then every block folds the
 * block maxima, scales and quantises its own tile; the second is skipped when normalize == 0 and pcm == peak == NULL.
 * A bad table cannot make the kernel read outside waves or write outside [0, total): a note with row outside [0, rows), hold < 1,
 * release < 0, hold + release > length or onset < 0 is skipped IN the kernel, and every note is clipped at total.
 * GS_ERR_ARG without a launch: n_notes, total, rows or length <= 0, row_stride < length, waves / notes / out NULL, a workspace that
 * is too small. */
#define GS_MIX_TILE 4096   /* samples per block: 256 lanes x 4 samples x 4 steps */
typedef struct GsMixNote {
    int64_t onset;          /* first sample of the note in the clip */
    int32_t hold, release;  /* samples at full level, then samples of the linear release */
    int32_t row;            /* which row of waves */
    float gain;
} GsMixNote;                /* 24 bytes */
size_t gs_note_mix_workspace_bytes(int64_t total);
int gs_note_mix(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNote* notes, int n_notes, int64_t total,
                int normalize, float* out, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream);

/* ---- Parts and stereo: the same mixdown into two channels with ONE peak (GANSynth.synthesize with stereo; this project's own rules,
 * DESIGN.md "Parts and stereo") ----------------------------------------------------------------------------------------------------
 * waves, the table's order, onset / hold / release / row and env(k) are gs_note_mix's.  A note carries two gains, and for each channel c
 *     mix_c[t] = sum over the covering notes, in ascending table order, of (gain_c * env(k)) * waves[row][k]
 * with gs_note_mix's operation order and separate roundings (no FMA, env's quotient as a multiplication by fl(1 / (release + 1))); every
 * waves[row][k] is loaded ONCE and enters both sums.  mix_l of a table with gain_l = g is therefore bit-identical to gs_note_mix's mix
 * of the same table with gain = g, and likewise on the right.  out: [2] rows of `total` samples, `out_stride` elements apart (channel 0
 * is the left one); a sample no note covers is 0, the elements between total and out_stride are not touched.
 * peak = max over both channels and all t of |mix_c[t]| (exact): ONE peak, so that normalising cannot move the stereo image.  Both
 * channels are divided by it (correctly rounded) when `normalize` and peak > 1.  pcm (or NULL): [total][2] interleaved,
 * pcm[t][c] = summary_audio_s16's rule applied to out[c][t].  peak (or NULL): [1].
 * Gather form, no atomics: a 256-thread block owns GS_MIX_TILE consecutive samples of BOTH channels (32 accumulators a lane) and finds
 * the notes that reach into them by two binary searches on the onsets; the table's rows come through uniform loads.  The output leaves
 * in 16-byte packs when both row bases are 16-byte aligned (and, in the second launch, pcm as well), sample by sample otherwise and at
 * the tail.  Two launches: the mix with one |max| per block into ws (sized by the query), then every block folds the block maxima,
 * scales and quantises its own tile of both channels; the second is skipped when normalize == 0 and pcm == peak == NULL.
 * A bad table cannot make the kernel read outside waves or write outside the two rows' [0, total): a note with row outside [0, rows),
 * hold < 1, release < 0, hold + release > length or onset < 0 is skipped IN the kernel before an address is formed from it, and every
 * note is clipped at total.  `reserved` is not read.
 * GS_ERR_ARG with a message and without a launch: n_notes, total, rows or length <= 0, row_stride < length, out_stride < total,
 * waves / notes / out NULL, notes off 8 bytes, waves / out / peak off 4 bytes, pcm off 2 bytes, a workspace that is too small.
 *
 * gs_stereo_finish is that second stage on its own, for a [2]-row clip the mix did not leave (the resampled one): x: [2] rows of n
 * samples, `row_stride` >= n elements apart (any such stride: a row 1 off 16 bytes takes the sample-by-sample path), IN PLACE.  A first
 * launch leaves one |max| per GS_MIX_TILE samples of both rows in ws, then the SAME finish kernel runs: peak, the quotient and pcm are
 * defined as above with x for the mix.  With normalize == 0 and pcm == NULL x is only read; with peak == NULL too nothing is launched.
 * GS_ERR_ARG with a message and without a launch: n <= 0, row_stride < n, x NULL, x / peak off 4 bytes, pcm off 2 bytes, a workspace
 * that is too small. */
typedef struct GsMixNoteStereo {
    int64_t onset;          /* as GsMixNote */
    int32_t hold, release;
    int32_t row;
    float gain_l, gain_r;   /* the note's gain on channel 0 (left) and on channel 1 (right) */
    int32_t reserved;       /* pads the row to 32 bytes; not read */
} GsMixNoteStereo;          /* 32 bytes */
size_t gs_note_mix_stereo_workspace_bytes(int64_t total);
int gs_note_mix_stereo(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNoteStereo* notes, int n_notes,
                       int64_t total, int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes,
                       void* stream);
size_t gs_stereo_finish_workspace_bytes(int64_t n);
int gs_stereo_finish(float* x, int64_t n, int64_t row_stride, int normalize, int16_t* pcm, float* peak, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- Controllers: the same mixdown under gains that are functions of clip time (GANSynth.synthesize with controllers; this project's own
 * rules, DESIGN.md "Controllers") ----------------------------------------------------------------------------------------------------------
 * waves, the table's order, onset / hold / release / row and env(k) are gs_note_mix's.  A note carries ONE gain and names a curve; a
 * curve is the piecewise-linear function through its points: curve p owns points[first[p] .. first[p + 1]) (first: a DEVICE array of
 * n_curves + 1 int32, non-decreasing from 0 to n_points, every range non-empty), their pos strictly increasing.  With i the last point
 * of the range whose pos is <= t, for each channel c (v = v_l for channel 0, v_r for channel 1; one channel reads v_l only)
 *     curve_c(t) = v_first                       for t before the first point,
 *                  v_last                        from the last point on (and for a one-point curve everywhere),
 *                  fl(v_i + fl(fl((float)(t - pos_i) * fl(1 / (float)(pos_{i+1} - pos_i))) * fl(v_{i+1} - v_i)))   otherwise
 * (so curve_c(pos_i) = v_i exactly), and
 *     mix_c[t] = sum over the covering notes, in ascending table order, of fl(fl(fl(gain * env(k)) * curve_c(t)) * waves[row][k])
 * in fp32, every operation rounded on its own (no FMA; both quotients correctly rounded reciprocals that are multiplied by; the two
 * int64 differences converted to fp32 with one rounding).  A table whose curves are all the one point (0, 1, 1) therefore gives
 * gs_note_mix's bits with one channel and gs_note_mix_stereo's with gain_l = gain_r = gain with two.
 * out, peak, the quotient and pcm: gs_note_mix's for channels == 1 (out_stride is not read), gs_note_mix_stereo's for channels == 2.
 * Gather form, no atomics: gs_note_mix_stereo's block and searches.  A curve's value does not depend on the note, so a lane keeps the
 * values of its 16 samples (per channel) in registers and evaluates them again only when the next candidate names another curve: every
 * wave finds the last point at or before the tile's first sample by a 64-way search of the curve's range, every thread brings one
 * point from there on into LDS (256 points, 4 KB), and each of the lane's four packs searches that window and walks through its four
 * samples; a tile that needs more than 256 points of one curve searches global memory instead, with the same result.  Two launches as for the other mixes, the second one clip_finish's, skipped when normalize == 0 and
 * pcm == peak == NULL.
 * A bad table cannot make the kernel read outside waves, points or first, or write outside the rows' [0, total): the judgements of
 * gs_note_mix_stereo hold, a note whose curve is outside [0, n_curves) is skipped IN the kernel, first's entries are clamped so that
 * every index into points lies in [0, n_points) before an address is formed, positions out of order give some value (finite or not)
 * of the points in range, and a segment of length <= 0 is not divided by (the curve takes v_i there).  `reserved` is not read.
 * GS_ERR_ARG with a message and without a launch: gs_note_mix_stereo's conditions (out_stride only with two channels), n_points or
 * n_curves <= 0, channels outside {1, 2}, points / first NULL, points off 8 bytes, first off 4 bytes. */
typedef struct GsMixNoteCurve {
    int64_t onset;          /* as GsMixNote */
    int32_t hold, release;
    int32_t row;
    float gain;             /* the note's own gain (velocity / 127); everything else comes through the curve */
    int32_t curve;          /* which curve: 0 <= curve < n_curves */
    int32_t reserved;       /* pads the row to 32 bytes; not read */
} GsMixNoteCurve;           /* 32 bytes */
typedef struct GsCurvePoint {
    int64_t pos;            /* a clip sample */
    float v_l, v_r;         /* the curve's value there on channel 0 and on channel 1 */
} GsCurvePoint;             /* 16 bytes */
size_t gs_note_mix_curves_workspace_bytes(int64_t total);
int gs_note_mix_curves(const float* waves, int rows, int64_t length, int64_t row_stride, const GsMixNoteCurve* notes, int n_notes,
                       const GsCurvePoint* points, int n_points, const int32_t* first, int n_curves, int channels, int64_t total,
                       int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream);

/* ---- Pitch bend: bent copies of the affected notes' waveforms, written ahead of the mix (GANSynth.synthesize with bend; this project's
 * own rule, DESIGN.md "Pitch bend") ---------------------------------------------------------------------------------------------------
 * waves: gs_note_mix's buffer, [rows] rows of `length` fp32 samples, `row_stride` elements apart; it is read AND written.  A curve is a
 * playback-rate ratio over clip samples: curve p owns points[first[p] .. first[p + 1]) (first: a DEVICE array of n_curves + 1 int32,
 * non-decreasing from 0 to n_points, every range non-empty); a point is (pos, ratio, cum), all float64, pos an integer-valued clip
 * sample, strictly increasing inside a curve, ratio in [0.25, 4].  Between two points the ratio is linear in t, before the first and
 * from the last on it is constant, and cum = Phi(pos) with Phi(t) = integral from 0 to t of the ratio.  With i the last point of the
 * curve whose pos is <= t (the first point for a t before it), d = t - pos_i, and -- inside a segment -- dp = pos_{i+1} - pos_i,
 * dr = ratio_{i+1} - ratio_i, in float64, every operation rounded on its own (no FMA) and in this order:
 *     Phi(t) = cum_i + ratio_i * d + dr * d * d / (2 * dp),   ratio(t) = ratio_i + dr * d / dp     inside a segment,
 *     Phi(t) = cum_i + ratio_i * d,                           ratio(t) = ratio_i                   outside the points.
 * A note (src_row, dst_row, onset, count, curve) gives, for k in [0, count):
 *     q = Phi(onset + k) - Phi(onset),   n = floor(q),   f = (float)(q - n),   c = (float)min(1, 1 / ratio(onset + k))
 *     waves[dst_row][k] = sum over integers i of h_i * x[i],   h_i = c * lerp(T, c * |(float)(i - n) - f| * Q),
 * x = waves[src_row], and x[i] = 0 for an i outside [0, length) -- whatever lies in the stride padding or in the next row.  lerp(T, a),
 * in fp32: a is first limited to Z Q, m = (int)a, T[m] + (a - m) * (T[m + 1] - T[m]); the table is
 *     T[m] = sinc(m / Q) * I0(BETA * sqrt(1 - (m / (Q Z))^2)) / I0(BETA),   m = 0 .. Z Q,   sinc(x) = sin(pi x) / (pi x),
 * computed in double and rounded once to fp32, with the exact values T[0] = 1 and T[j Q] = 0 for j >= 1 forced, and T[Z Q + 1] = 0.
 * So h_i is an exact 0 wherever |c (n + f - i)| >= Z: 2 Z taps count at a ratio <= 1 and 8 Z at ratio 4, where the cutoff has followed
 * the ratio down to a quarter of the band.  fp32 accumulation in a fixed order, FMA allowed; no atomics; two calls are bit-identical.
 * With the ratio identically 1, q = k, f = 0 and c = 1: every coefficient but one is an exact 0 and the row comes back unchanged.
 * gs_note_warp writes exactly `count` samples of each dst_row and nothing else.  The caller sees to it that no dst_row is the src_row or
 * the dst_row of another note of the call.  One launch: a block owns GS_WARP_TILE consecutive outputs of one note (grid: tiles x
 * notes) and stages the table (GS_WARP_TABLE_FLOATS floats) and the source span it can reach, at most 4 * GS_WARP_TILE + 8 Z + 4
 * samples, in LDS.  Capture-safe: no allocation, no synchronisation.
 * The table is filled in HOST memory by gs_note_warp_table (gs_note_warp_table_bytes bytes: T, the zero that follows, padding to 16
 * bytes) and uploaded by the caller once; both are host arithmetic and need no device.
 * A bad table cannot make the kernel read outside waves, points or first, or write outside the dst rows' [0, count): IN the kernel, and
 * before an address is formed, a note whose src_row or dst_row is outside [0, rows), whose src_row == dst_row, whose count is outside
 * [1, length], whose onset < 0 or whose curve is outside [0, n_curves) is skipped; first's entries are clamped so that every index
 * into points lies in [0, n_points); a segment of length <= 0 is not divided by (the curve is constant there); a ratio that is NaN or
 * outside [0.25, 4] is clamped into it; q is clamped into [0, length + 4 Z] (from there on every tap reads zeros, at every cutoff), and
 * a lane's offset into the staged span into that span.
 * GS_ERR_ARG with a message and without a launch: n_notes outside [1, 65535], rows / n_curves / n_points <= 0, length outside
 * [1, GS_WARP_MAX_LENGTH], row_stride < length, waves / notes / points / first / table NULL, table off 16 bytes, notes / points off 8,
 * waves / first off 4; gs_note_warp_table: a NULL table. */
#define GS_WARP_ZEROS 32
#define GS_WARP_Q 256
#define GS_WARP_BETA 12.0
#define GS_WARP_TILE 1024                           /* outputs per block: 256 lanes x 4 */
#define GS_WARP_TABLE_FLOATS 8196                   /* Z Q + 1 entries, the zero that follows, padding to whole 16 bytes */
#define GS_WARP_MAX_LENGTH ((int64_t)1 << 30)
typedef struct GsWarpNote {
    int32_t src_row, dst_row;   /* rows of waves: read [0, length) of the one, write [0, count) of the other */
    int64_t onset;              /* the note's first clip sample: where its curve is read */
    int32_t count;              /* samples to write: hold + release, 1 <= count <= length */
    int32_t curve;              /* which curve: 0 <= curve < n_curves */
} GsWarpNote;                   /* 24 bytes */
typedef struct GsWarpPoint {
    double pos;                 /* a clip sample (integer-valued) */
    double ratio;               /* the playback-rate ratio there, in [0.25, 4] */
    double cum;                 /* Phi(pos) */
} GsWarpPoint;                  /* 24 bytes */
size_t gs_note_warp_table_bytes(void);
int gs_note_warp_table(float* table_host);
int gs_note_warp(float* waves, int rows, int64_t length, int64_t row_stride, const GsWarpNote* notes, int n_notes,
                 const GsWarpPoint* points, const int32_t* first, int n_curves, int n_points, const float* table_dev, void* stream);

/* ---- Sustain: notes held past the generated length, as looped copies written ahead of the mix (GANSynth.synthesize with sustain; this
 * project's own rule, DESIGN.md "Sustain") -------------------------------------------------------------------------------------------
 * waves: gs_note_mix's buffer, [rows] rows of `length` fp32 samples, `row_stride` elements apart.
 *
 * gs_loop_search scores every candidate loop length of every note.  A note (row, a, m_min, m_max, window), x = waves[row], W = window:
 *     S_aa = sum_{i<W} x[a+i]^2,   S_ab(m) = sum_{i<W} x[a+i] x[a+m+i],   S_bb(m) = sum_{i<W} x[a+m+i]^2,
 *     scores[n * scores_stride + (m - m_min)] = S_ab / sqrt(S_aa * S_bb),  or 0 where S_aa * S_bb == 0,     m in [m_min, m_max].
 * fp32 accumulation in a fixed order (S_ab and S_bb: four chains by tap index mod 4, folded (0 + 1) + (2 + 3); S_aa: one chain per lane,
 * folded over the block in a fixed tree), FMA allowed, no atomics: two calls are bit-identical.  One launch: a 256-lane block owns
 * GS_SUSTAIN_LAG_TILE consecutive lags of one note (grid: lag tiles x notes), stages x[a .. a+W) and the span of its lags in LDS
 * (zero-filled past the row's end; with W <= GS_SUSTAIN_MAX_WINDOW under 34 KB) and computes S_aa itself -- no second launch and no
 * workspace.  Which lag to take is host work on the returned scores.  waves is only read.
 * A bad table cannot fault: IN the kernel, and before an address is formed, a note whose row is outside [0, rows), whose a < 0,
 * m_min < 1, m_max < m_min, window < 1 or window > GS_SUSTAIN_MAX_WINDOW, whose a + m_max + window > length (in 64 bits) or whose
 * m_max - m_min + 1 > scores_stride is skipped, and its scores are left untouched.
 *
 * gs_note_sustain writes pieces of the endless waveform of a looped note.  For a source row x, a loop (a, m), b = a + m and a crossfade
 * of X = xfade samples (b + X <= length):
 *     y[k] = x[k]                                          k < b
 *     y[k] = (1 - w) * x[b + p] + w * x[a + p]             k >= b,  p = (k - b) mod m < X,   w = (float)(p + 1) * fl(1 / (X + 1))
 *     y[k] = x[a + p]                                      k >= b,  p >= X
 * in fp32, every operation rounded on its own and in the order written (no FMA): at every wrap the outgoing signal is the waveform's
 * own continuation past b, fading out under the loop's start.  A job (src_row, dst_row, offset, count, a, m, xfade) makes
 * waves[dst_row][j] = y[offset + j] for j in [0, count), x = waves[src_row], and writes nothing else; (k - b) mod m is taken in 64 bits.
 * The caller sees to it that no dst_row is the src_row or the dst_row of another job.  One launch: a 256-lane block owns
 * GS_SUSTAIN_TILE consecutive outputs of one job (grid: tiles x jobs), 16 bytes per lane on the store side where the row allows it.
 * A bad table cannot fault: IN the kernel, and before an address is formed, a job whose src_row or dst_row is outside [0, rows), whose
 * src_row == dst_row, whose count is outside [1, length], whose offset < 0, a < 0, m < 1 or xfade < 0, or whose a + m + xfade > length
 * (in 64 bits) is skipped.
 * Both are capture-safe: no allocation, no synchronisation.  GS_ERR_ARG with a message and without a launch: n_notes / n_jobs outside
 * [1, 65535], rows <= 0, length outside [1, GS_SUSTAIN_MAX_LENGTH], row_stride < length, scores_stride outside [1, 2^24], a NULL
 * pointer, waves / scores off 4 bytes, notes off 4, jobs off 8. */
#define GS_SUSTAIN_MAX_WINDOW 4096
#define GS_SUSTAIN_LAG_TILE 256                     /* lags per block of gs_loop_search: one per lane */
#define GS_SUSTAIN_TILE 1024                        /* outputs per block of gs_note_sustain: 256 lanes x 4 */
#define GS_SUSTAIN_MAX_LENGTH ((int64_t)1 << 30)
typedef struct GsLoopNote {
    int32_t row;                /* the row of waves that is searched */
    int32_t a;                  /* the loop's start */
    int32_t m_min, m_max;       /* the lags that are scored: 1 <= m_min <= m_max */
    int32_t window;             /* W: taps per correlation, 1 <= W <= GS_SUSTAIN_MAX_WINDOW */
    int32_t reserved;           /* not read */
} GsLoopNote;                   /* 24 bytes */
typedef struct GsSustainJob {
    int32_t src_row, dst_row;   /* rows of waves: read [0, a + m + xfade) of the one, write [0, count) of the other */
    int64_t offset;             /* the index into y of the first sample written */
    int32_t count;              /* samples to write, 1 <= count <= length */
    int32_t a, m, xfade;        /* the loop's start, its length and the crossfade: a + m + xfade <= length */
} GsSustainJob;                 /* 32 bytes */
int gs_loop_search(const float* waves, int rows, int64_t length, int64_t row_stride, const GsLoopNote* notes, int n_notes, float* scores,
                   int64_t scores_stride, void* stream);
int gs_note_sustain(float* waves, int rows, int64_t length, int64_t row_stride, const GsSustainJob* jobs, int n_jobs, void* stream);

/* ---- Resident notes: one batch drawn from the int16 bank on the device (gansynth_amd/bank.py, DESIGN.md "Resident notes") ----------
 * pcm: [rows] notes of `length` int16 samples, `row_stride` elements apart.  class_of_row: [rows] int32, the label index of a row or -1.
 * order: [n_order] int32 row numbers; the batch is order[first .. first + batch).  For b in [0, batch), r = order[first + b]:
 *     waves[b][i]  = (float)pcm[r * row_stride + i] * 2^-15       (exact in fp32: dataset.decode_wav's value bit for bit)
 *     labels[b][c] = (c == class_of_row[r]) ? 1 : 0
 * waves == NULL writes the labels only.  An r outside [0, rows) reads nothing: zeros and an all-zero label.  A class outside
 * [0, n_classes) gives an all-zero label.  Every row offset is 64-bit.  One launch, no workspace, no atomics.  16-byte loads of eight
 * samples per lane when length % 8 == 0, row_stride % 8 == 0 and pcm and waves are 16-byte aligned (chosen here, on the host), one
 * sample per lane otherwise.
 * GS_ERR_ARG without a launch: pcm / class_of_row / order / labels NULL, rows / length / batch / n_classes <= 0, row_stride < length,
 * first < 0 or first + batch > n_order, pcm not 2-byte or waves / labels not 4-byte aligned, a batch too large for one grid. */
int gs_bank_gather(const int16_t* pcm, int64_t rows, int64_t length, int64_t row_stride, const int32_t* class_of_row, const int32_t* order,
                   int64_t n_order, int64_t first, int batch, int n_classes, float* waves, float* labels, void* stream);

/* ---- Output rates: a rational-ratio polyphase resampler (GANSynth.synthesize / generate with sample_rate, spectral_ops.resample; this
 * project's own rule, DESIGN.md "Output rates") -------------------------------------------------------------------------------------
 * For rate_in != rate_out, both positive: g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g,
 *     c = ROLLOFF * min(1, up / down),   taps = 2 * ceil(ZEROS / c),   n_out = ceil(n_in * up / down)
 * with the fixed design constants below.  The continuous kernel is a Kaiser-windowed sinc,
 *     h(u) = c * sinc(c u) * I0(BETA * sqrt(1 - a^2)) / I0(BETA),   a = c u / ZEROS,   for |a| < 1, else 0;   sinc(x) = sin(pi x) / (pi x)
 * and the table is T[p][k] = h(p / up + taps/2 - 1 - k), p in [0, up), k in [0, taps), computed in double and rounded once to fp32.
 * Output j of a row (all index arithmetic in 64 bits):
 *     i0 = floor(j * down / up),   p = (j * down) mod up,   y[j] = sum over k of T[p][k] * x[i0 - taps/2 + 1 + k]
 * where an x index outside [0, n_in) contributes 0 -- so a tap that falls into a row's stride padding or into the neighbouring row
 * contributes 0 whatever lies there.  No per-phase renormalisation.  fp32 accumulation in a fixed order, FMA allowed; no atomics; two
 * calls are bit-identical.
 * Tail, per row, with gs_note_mix's semantics: peak[r] = max over j of |y[r][j]| (exact); out = y / peak[r] (correctly rounded) when
 * `normalize` and peak[r] > 1, else y; pcm (or NULL): summary_audio_s16's rule applied to out.  x: [rows] rows of n_in fp32 samples,
 * `row_stride` elements apart; out: [rows][n_out] fp32; pcm: [rows][n_out] int16 or NULL; peak: [rows] fp32 or NULL.
 * Two launches: the filter -- a block owns GS_RESAMPLE_TILE consecutive outputs of one row, stages the input span they need in LDS
 * (zero-filled beyond the row's ends) and leaves one |max| per block in ws (sized by the query) -- then every block folds its row's
 * maxima, scales and quantises; the second is skipped when normalize == 0 and pcm == peak == NULL.  Capture-safe: no allocation, no
 * synchronisation.
 * The table is filled in HOST memory and uploaded by the caller once per (rate_in, rate_out).  device_layout == 0: the logical
 * [up][taps] order above.  device_layout != 0: what gs_resample reads -- the same rows, each padded with zeros to
 * GS_RESAMPLE_ROW(taps) floats so that every row starts on 16 bytes ([up][GS_RESAMPLE_ROW(taps)]; the base must be 16-byte aligned).
 * gs_resample_design, _out_len, _table_bytes, _table and _workspace_bytes are host arithmetic and need no device.
 * GS_ERR_ARG with a message and without a launch: non-positive rates, equal rates, up > GS_RESAMPLE_MAX_UP, taps > GS_RESAMPLE_MAX_TAPS
 * (e.g. 16000 -> 44101, or a ratio beyond about 1/15), rows <= 0 (or > 65535), n_in <= 0 (or > GS_RESAMPLE_MAX_N), row_stride < n_in,
 * x / out / table NULL, a misaligned pointer, a workspace that is too small, a descriptor whose up / down / taps / zeros do not follow
 * from its rates.  (The queries answer a refusal with 0 bytes, gs_resample_out_len with the negative code.) */
#define GS_RESAMPLE_ZEROS 32
#define GS_RESAMPLE_ROLLOFF 0.95
#define GS_RESAMPLE_BETA 12.0
#define GS_RESAMPLE_MAX_UP 1024
#define GS_RESAMPLE_MAX_TAPS 1024
#define GS_RESAMPLE_MAX_N ((int64_t)1 << 40)
#define GS_RESAMPLE_TILE 512                        /* outputs per block of the filter: 256 lanes x 2 */
#define GS_RESAMPLE_ROW(taps) (((taps) + 3) & ~3)   /* floats per row of the device table */
typedef struct GsResample {
    int32_t rate_in, rate_out;
    int32_t up, down, taps;   /* as defined above */
    int32_t zeros;            /* GS_RESAMPLE_ZEROS */
} GsResample;                 /* 24 bytes */
int gs_resample_design(int rate_in, int rate_out, GsResample* out);
int64_t gs_resample_out_len(const GsResample* r, int64_t n_in);
size_t gs_resample_table_bytes(const GsResample* r, int device_layout);
int gs_resample_table(const GsResample* r, int device_layout, float* table_host);
size_t gs_resample_workspace_bytes(const GsResample* r, int rows, int64_t n_in);
int gs_resample(const GsResample* r, const float* table_dev, const float* x, int rows, int64_t n_in, int64_t row_stride, int normalize,
                float* out, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream);

/* ---- Reverb: convolution of a clip with an impulse response, partitioned FFT (gansynth_amd/reverb.py, kernels.fft_convolve; this
 * project's own rule, DESIGN.md "Reverb") ---------------------------------------------------------------------------------------------
 * x: [rows] rows of n fp32 samples, `row_stride` elements apart (rows is 1 or 2: a clip is mono or stereo).  h: [ir_rows] rows of m fp32
 * taps, `ir_stride` apart, ir_rows == 1 (shared) or == rows.  n_out = n + m - 1, and for t in [0, n_out), rh = r when ir_rows == rows else 0:
 *     y[r][t] = dry * x[r][t] + wet * sum over k in [0, m) of h[rh][k] * x[r][t - k]
 * where an x index outside [0, n) contributes 0, whatever lies in the stride padding or in the next row.  With lead[rh] the index of the
 * first non-zero tap of h[rh] (m when there is none), the sum is EXACTLY 0 for t < lead[rh]: a predelay is silent, not nearly silent.
 * Tail with gs_note_mix_stereo's semantics: ONE peak = max over all rows and t of |y| (exact); out = y / peak (correctly rounded) when
 * `normalize` and peak > 1, else y; pcm (or NULL): [n_out][rows] interleaved (plain [n_out] for rows == 1), summary_audio_s16's rule applied
 * to out; peak (or NULL): [1].  out: [rows] rows of n_out samples, `out_stride` apart; the elements between n_out and out_stride are not
 * touched.
 * Form: uniform partitioned overlap-save, B = GS_FFTCONV_BLOCK new samples per block, P = ceil(m / B) partitions, J = ceil(n_out / B)
 * blocks; a 2B-point real transform runs as a B-point complex one (even samples real, odd imaginary) in LDS, fp32, radix-2 Stockham
 * (natural order in and out), twiddles computed in double and rounded once.  A spectrum is stored as B complex values: slot 0 holds the
 * two real bins (0 and B) as (re, im), slot k the bin k.  The sum over partitions runs over p ascending, in registers, FMA allowed; the
 * result is not bit-defined against another FFT, but no atomics: two calls are bit-identical.
 * gs_fftconv_prepare, once per impulse response (3 launches): the twiddle tables, the transform of every partition of every IR row
 * (zero-padded to 2B) and lead[] go into the caller's `spectrum` buffer (gs_fftconv_spectrum_bytes:
 * GS_FFTCONV_HEADER_BYTES + ir_rows * P * B * 8; 16-byte aligned).
 * gs_fftconv (3 launches; capture-safe: no allocation, no synchronisation): block j of row r covers the samples [(j - 1) B, (j + 1) B),
 * zero outside [0, n) -- only the XB = min(J, floor((n - 1) / B) + 2) blocks that can hold a sample are transformed --; then one workgroup
 * per (r, j) accumulates sum over p of X[r][j - p] * H[rh][p] (the p with j - p in [0, XB)), inverts, keeps the last B samples, applies dry
 * and wet, writes 16 bytes per lane where the row bases are 16-byte aligned and leaves one |max| per block in ws; then the finish kernel
 * of gs_note_mix (rows == 1) or gs_note_mix_stereo (rows == 2).  ws (gs_fftconv_workspace_bytes: rows * XB * B * 8 + rows * J * 4;
 * 16-byte aligned).  Every bound the kernels use is recomputed from n and m.
 * gs_fftconv_design, _out_len, _spectrum_bytes and _workspace_bytes are host arithmetic and need no device.
 * GS_ERR_ARG with a message and without a launch: n, m or rows <= 0, rows > 2, n > GS_FFTCONV_MAX_N, m > GS_FFTCONV_MAX_TAPS, ir_rows
 * outside {1, rows}, row_stride < n, ir_stride < m, out_stride < n_out, x / out / spectrum / ir NULL, x / out / ir / peak off 4 bytes, pcm
 * off 2, spectrum / ws off 16, a workspace or spectrum buffer that is too small, a descriptor whose block / partitions / blocks /
 * x_blocks do not follow from its n and m.  (The byte queries answer a refusal with 0, gs_fftconv_out_len with the negative code.) */
#define GS_FFTCONV_BLOCK 2048
#define GS_FFTCONV_MAX_TAPS (1 << 20)
#define GS_FFTCONV_MAX_N ((int64_t)1 << 40)
#define GS_FFTCONV_HEADER_BYTES ((GS_FFTCONV_BLOCK + GS_FFTCONV_BLOCK / 2 + 8) * 8 + 16)   /* stage twiddles, pack twiddles, lead[2] */
typedef struct GsFftConv {
    int64_t n, m;              /* samples per row, taps per IR row */
    int32_t rows, ir_rows;
    int32_t block;             /* GS_FFTCONV_BLOCK */
    int32_t partitions;        /* P */
    int32_t blocks, x_blocks;  /* J, XB */
} GsFftConv;                   /* 40 bytes */
int gs_fftconv_design(int64_t n, int64_t m, int rows, int ir_rows, GsFftConv* out);
int64_t gs_fftconv_out_len(const GsFftConv* c);
size_t gs_fftconv_spectrum_bytes(const GsFftConv* c);
size_t gs_fftconv_workspace_bytes(const GsFftConv* c);
int gs_fftconv_prepare(const GsFftConv* c, const float* ir, int64_t ir_stride, void* spectrum, size_t spectrum_bytes, void* stream);
int gs_fftconv(const GsFftConv* c, const void* spectrum, size_t spectrum_bytes, const float* x, int64_t row_stride, float dry, float wet,
               int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream);

/* ---- Limiter: a look-ahead peak limiter as the last stage of a rendered clip (gansynth_amd/limiter.py, kernels.limit; this project's
 * own rule, DESIGN.md "Limiter") -----------------------------------------------------------------------------------------------------
 * x: [rows] rows of n fp32 samples, `row_stride` elements apart (rows is 1 or 2).  d = pre_gain (finite, > 0), c = ceiling (0 < c <= 1),
 * W = lookahead in samples (1 <= W <= GS_LIMIT_MAX_LOOKAHEAD).  For t in [0, n):
 *   1. y[r][t] = fl(d * x[r][t])                           one fp32 rounding, no FMA into a later step
 *   2. a[t]    = max over the rows of |y[r][t]|            an fmaxf chain from 0: ONE gain for both channels, the stereo image cannot move; a
 *                                                          NaN sample contributes nothing, passes to out as NaN, is PCM 0, disturbs no neighbour
 *   3. r[t]    = c / a[t] if a[t] > c, else 1              a correctly rounded fp32 quotient
 *   4. m[s]    = min of r over [max(s, 0), min(s + W, n - 1)]   for s in [-W, n); exact
 *   5. g[t]    = (m[t - W] + ... + m[t]) / (W + 1)         W + 1 terms, a true division; every fp32 sum a tree over the window's own
 *                                                          W + 1 terms (never a running sum along the clip)
 *   6. out[r][t] = clamp(fl(g[t] * y[r][t]), -c, c)        (a NaN stays a NaN)
 *   7. pcm     = summary_audio_s16's rule applied to out: [n] for one row, interleaved [n][2] for two
 *   8. peak    = max |out| (exact)         9. min_gain = min g (exact): the deepest gain reduction
 * Every window [s, s + W] with s in [t - W, t] contains t, so every term of the mean is <= r[t], g[t] <= r[t] and |g[t] y[t]| <= c in exact
 * arithmetic: the clamp removes only a last ulp of rounding, and |out| <= c holds bit for bit.  Where no sample within W on either side
 * exceeds c every term is exactly 1, W + 1 ones sum exactly in any order and (W + 1) / (W + 1) == 1: out == fl(d * x) bit for bit there.  The
 * release is as long as the attack.  No atomics: two calls are bit-identical.
 * pcm, peak ([1]) and min_gain ([1]) may be NULL.  out: [rows] rows of n samples, `out_stride` apart; the elements between n and out_stride
 * are not touched.  out must not overlap x (a block reads its neighbours' input).
 * One launch over tiles of GS_LIMIT_TILE samples of both rows (r with a halo of W on either side in LDS, the sliding minimum and the sliding
 * sum by doubling, 16 bytes per lane where every row of x and out is 16-byte aligned -- and pcm 8 * rows --, sample by sample otherwise),
 * which leaves one |max| and one min per block in ws (gs_limit_workspace_bytes: 2 * 4 * ceil(n / GS_LIMIT_TILE), rounded up to 16; 16-byte
 * aligned), and one small fold launch when peak or min_gain is asked for.  Every bound is recomputed from n and W.  Capture-safe: no
 * allocation, no synchronisation.  gs_limit_workspace_bytes is host arithmetic and answers 0 for a refused shape.
 * GS_ERR_ARG with a message and without a launch: rows outside {1, 2}, n <= 0 (or > GS_LIMIT_MAX_N), a stride below n, x or out NULL,
 * x / out / peak / min_gain off 4 bytes, pcm off 2, ws off 16 or too small, pre_gain not finite or <= 0, ceiling outside (0, 1], lookahead
 * outside [1, GS_LIMIT_MAX_LOOKAHEAD], overlapping x and out. */
#define GS_LIMIT_MAX_LOOKAHEAD 2048
#define GS_LIMIT_TILE 4096
#define GS_LIMIT_MAX_N ((int64_t)1 << 40)
size_t gs_limit_workspace_bytes(int rows, int64_t n);
int gs_limit(const float* x, int rows, int64_t n, int64_t row_stride, float pre_gain, float ceiling, int lookahead, float* out,
             int64_t out_stride, int16_t* pcm, float* peak, float* min_gain, void* ws, size_t ws_bytes, void* stream);

/* ---- True peak: a 4x oversampled peak detector and the limiter that listens to it (gansynth_amd/true_peak.py, kernels.true_peak,
 * kernels.limit(envelope=...); this project's own rule, DESIGN.md "True peak") ----------------------------------------------------------
 * Detector.  T is the [4][68] fp32 table that gs_resample_table gives for the design 1 -> 4 (up 4, down 1, taps 68): the same Kaiser design
 * and the same single rounding to fp32 as the resampler's; it does not depend on the clip's rate.  For x of [rows] rows (1 or 2) of n
 * samples, `row_stride` elements apart, with x outside [0, n) taken as 0:
 *     z[r][4t + p] = sum over k in [0, 68) of T[p][k] * x[r][t - 33 + k]      p = 0..3   (what gs_resample 1:4 would write)
 *     e[t]         = max over rows r of max(|x[r][t]|, |z[r][4t + 0]|, ..., |z[r][4t + 3]|)        an fmaxf chain from 0
 *     true_peak    = max over t in [0, n) of e[t]                              the exact fold of the computed e
 * e[t] covers the reconstructed waveform on [t, t + 1).  |x| is in the maximum because phase 0 of a 0.95-rolloff design is not the identity
 * and a true peak below the sample peak would be absurd.  fp32 accumulation in any order, with or without FMA: the contract is the
 * resampler's, |z - z64| <= (taps + 3) * 2^-24 * B with B = sum |T||x|, and e inherits the largest bound among its five terms.  No atomics:
 * two calls are bit-identical.  The 4x signal is never written to memory.
 * gs_true_peak: table_dev is the device-layout table of the 1 -> 4 design, as gs_resample takes it (16-byte aligned).  env ([n]) and peak
 * ([1]) may each be NULL, not both.  One launch over tiles of GS_TRUE_PEAK_TILE samples of all rows (the tile with a halo of 33 before and 34
 * after in LDS, a lane register-blocks 8 samples x 4 phases, the coefficients come through scalar registers), which leaves one |max| per block
 * in ws (gs_true_peak_workspace_bytes: 4 * ceil(n / GS_TRUE_PEAK_TILE), rounded up to 16; 16-byte aligned), and one small fold launch when
 * peak is asked for.  Capture-safe: no allocation, no synchronisation.  gs_true_peak_workspace_bytes is host arithmetic and answers 0 for a
 * refused shape.
 * GS_ERR_ARG with a message and without a launch: rows outside {1, 2}, n <= 0 (or > GS_TRUE_PEAK_MAX_N), row_stride < n, table or x NULL, env
 * and peak both NULL, table off 16 bytes, x / env / peak off 4, ws NULL, off 16 or too small.
 * True-peak limiter.  gs_limit_env is gs_limit's rule, steps 1-9, with one change in step 2:
 *   2'. a[t] = max( max over the rows of |y[r][t]| ,  fl(d * env[t]) )         env: the detector's e of the unscaled x ([n], required)
 * Everything else is character for character gs_limit's: the correctly rounded quotient, the exact minimum, the tree sums over exactly W + 1
 * terms, the clamp, |out| <= c bit for bit per sample, out == fl(d * x) bit for bit where no a within W exceeds c.  What it adds: every
 * reconstructed point between t and t + 1 sees gains <= c / (d e[t]); the remaining overshoot comes only from the gain moving under the
 * 68-tap kernel and is second order.  A NaN in env contributes nothing.  With env[t] = max over the rows of |x[r][t]| it is gs_limit bit for
 * bit.  Same launches, workspace and refusals as gs_limit, and env NULL or off 4 bytes. */
#define GS_TRUE_PEAK_TILE 2048
#define GS_TRUE_PEAK_TAPS 68
#define GS_TRUE_PEAK_OVERSAMPLE 4
#define GS_TRUE_PEAK_MAX_N ((int64_t)1 << 40)
size_t gs_true_peak_workspace_bytes(int rows, int64_t n);
int gs_true_peak(const float* table_dev, const float* x, int rows, int64_t n, int64_t row_stride, float* env, float* peak, void* ws,
                 size_t ws_bytes, void* stream);
int gs_limit_env(const float* x, const float* env, int rows, int64_t n, int64_t row_stride, float pre_gain, float ceiling, int lookahead, float* out,
                 int64_t out_stride, int16_t* pcm, float* peak, float* min_gain, void* ws, size_t ws_bytes, void* stream);

/* ---- Loudness: the K-weighted hop energies of ITU-R BS.1770, from which the host gates the integrated loudness of a rendered clip
 * (gansynth_amd/loudness.py, kernels.loudness_energy; DESIGN.md "Loudness") ------------------------------------------------------------
 * gs_loudness_design(rate): host arithmetic in float64, no device.  hop = floor(0.1 * rate + 0.5) samples (a gating block is 4 hops: 400 ms
 * with 75 % overlap; at a rate that is no multiple of 10 a hop departs from 100 ms by under half a sample).  The two K-weighting sections
 * for any rate, by the bilinear forms whose 48 kHz values are the table of BS.1770 (a[0] = 1):
 *   stage 1 (shelf):     f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196;
 *                        K = tan(pi f0 / rate), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *                        b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0,   a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *   stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773;   b = [1, -2, 1],   a as above
 * and what the kernels' chunking needs: chunk = ceil(hop / 256) | 1 samples a lane (odd), lanes = ceil(hop / chunk), rem = hop - (lanes - 1) *
 * chunk samples of the last lane, and with A the 4 x 4 matrix that one silent sample applies to the cascade's state (s1[0], s1[1], s2[0],
 * s2[1]; transposed direct form II), row-major: chunk_pow[k] = A^(chunk * 2^k), hop_pow[k] = A^(hop * 2^k), k in [0, GS_LOUDNESS_STEPS),
 * rem_pow = A^rem.
 * gs_loudness: x is [rows] rows (1 or 2) of n fp32 samples, `row_stride` elements apart.  hops = floor(n / hop): an incomplete last hop is
 * not measured.  Per row, starting at rest at sample 0 and running through the whole row,
 *     y1[t] = b1[0] x[t] + b1[1] x[t-1] + b1[2] x[t-2] - a1[1] y1[t-1] - a1[2] y1[t-2],    y2 likewise from y1 with b2, a2
 *     energy[r * energy_stride + j] = sum over t in [j hop, (j + 1) hop) of y2[t]^2,  j in [0, hops),  as fp32
 * -- the EXACT recurrence: no block restarts at rest from a halo.  The recurrence is linear, so k samples from a state s end in A^k s plus
 * their end from rest; everything after the fp32 load (filter, states, squares, sums) is float64, FMA allowed, rounded once at the store.
 * Rows are independent: row 0 of a two-row call is bit-identical to the one-row call on it.  A non-finite sample propagates as IEEE
 * arithmetic has it, to that row's energies from its hop on, and to nothing else.  Samples and hops before the first non-zero sample give
 * exactly 0.  No atomics: two calls are bit-identical.  energy is written in [0, hops) of each row only; with hops == 0 nothing is launched.
 * Three launches: (hops, rows) blocks, one hop in LDS each, leave the hop's end state from rest; one block per row carries the states
 * across the hops (a scan with the powers of A^hop); (hops, rows) blocks run every chunk from its true state and reduce the squares in a
 * fixed tree.  16-byte loads from the hop's first 16-byte boundary on whatever the row base, sample by sample before it and at the tail.
 * Every bound is recomputed from n and the descriptor.  Capture-safe: no allocation, no synchronisation.  ws (gs_loudness_workspace_bytes:
 * rows * max(hops, 1) * 64 -- two states of four doubles a hop; 16-byte aligned).
 * gs_loudness_design, _hops and _workspace_bytes are host arithmetic and need no device.
 * GS_ERR_ARG with a message and without a launch: a rate outside [GS_LOUDNESS_MIN_RATE, GS_LOUDNESS_MAX_RATE], rows outside {1, 2}, n <= 0
 * (or > GS_LOUDNESS_MAX_N), row_stride < n, energy_stride < hops, x or energy NULL or off 4 bytes, ws NULL, off 16 or too small, a
 * descriptor that differs in any byte from gs_loudness_design of its rate.  (The byte query answers a refusal with 0, gs_loudness_hops
 * with the negative code.) */
#define GS_LOUDNESS_MIN_RATE 8000
#define GS_LOUDNESS_MAX_RATE 192000
#define GS_LOUDNESS_MAX_N ((int64_t)1 << 40)
#define GS_LOUDNESS_STEPS 8
typedef struct GsLoudness {
    int32_t rate, hop;
    int32_t chunk, lanes, rem, reserved;
    double b1[3], a1[3], b2[3], a2[3];
    double chunk_pow[GS_LOUDNESS_STEPS][16];
    double hop_pow[GS_LOUDNESS_STEPS][16];
    double rem_pow[16];
} GsLoudness;                  /* 2296 bytes */
int gs_loudness_design(int rate, GsLoudness* out);
int64_t gs_loudness_hops(const GsLoudness* d, int64_t n);
size_t gs_loudness_workspace_bytes(const GsLoudness* d, int rows, int64_t n);
int gs_loudness(const GsLoudness* d, const float* x, int rows, int64_t n, int64_t row_stride, float* energy, int64_t energy_stride, void* ws,
                size_t ws_bytes, void* stream);

/* ---- k-means for the NDB metric (gansynth_amd/kmeans.py, metrics.num_different_bins_device; DESIGN.md "NDB on the device") ----
 * fp32, deterministic (fixed-order sums, no float atomics): two calls with the same arguments write the same bits.  x is [n, d] with its rows
 * ldx >= d floats apart, 4-byte aligned; centres is [k, d] dense.  Inputs are finite.
 *
 * gs_kmeans_assign: labels[i] = the centre nearest to row i in the squared Euclidean distance, sum over the columns in ascending order of
 * (x - c)^2 on the vector ALU (never |x|^2 - 2 x.c + |c|^2: that form cancels on features with a common offset); ties to the lowest centre
 * index.  dist ([n], the minimum), changed ([1] int32: labels is read before it is written, and the rows whose label moved are counted) and
 * inertia ([1] double: the sum of those fp32 minima, accumulated in double in a fixed order) may each be NULL.  One launch over tiles of GS_KMEANS_TILE rows, and
 * a one-block fold of the tiles' partial sums when changed or inertia is asked for.
 *
 * gs_kmeans_inertia: inertia ([1] double) = the sum over the rows of |x_i - centres[labels[i]]|^2 with every term and every sum in double, in
 * a fixed order: the figure kmeans.py chooses between runs by (two runs that end within fp32 rounding of each other are not told apart by the
 * sum of fp32 minima).  One read of x: a launch over the same tiles and the same one-block fold.  A row whose label is outside [0, k) adds
 * nothing.
 *
 * gs_kmeans_update: counts[k] (int32) = the rows of every label, and for every label with rows the mean of them into its row of centres; the
 * centre of an empty label is not written.  A row whose label is outside [0, k) is ignored.  A block of one wave owns a slice of rows and 64
 * columns and adds row after row, in order, into its own [k, 64] slab; the slabs go to ws and a second launch folds them in slice order.
 *
 * gs_kmeans_mindist (the k-means++ step): dist[i] = |x_i - centre|^2 when first != 0, else min(dist[i], |x_i - centre|^2); centre is d floats
 * on the device (it may be a row of x).
 *
 * gs_kmeans_workspace_bytes (host arithmetic; 0 for a shape the entries refuse) covers both launches:
 *   max(12 * ceil(n / GS_KMEANS_TILE),  4 * slices * k * (d + 1)),  rounded up to 16, with
 *   slices = ceil(n / ceil(n / s0)),  s0 = max(1, min(GS_KMEANS_MAX_SLICES, 2048 / ceil(d / 64), ceil(n / 64))).
 * ws is 16-byte aligned.  Capture-safe: no allocation, no synchronisation.
 * GS_ERR_ARG with a message that names the argument and without a launch: k outside [1, GS_KMEANS_MAX_K], d outside [1, GS_KMEANS_MAX_D] (update
 * puts ceil(d / 64) into a grid dimension), n < 1 (or > GS_KMEANS_MAX_N),
 * ldx < d, a NULL or misaligned pointer, a workspace that is too small. */
#define GS_KMEANS_MAX_K 256
#define GS_KMEANS_MAX_D (1 << 20)
#define GS_KMEANS_TILE 256
#define GS_KMEANS_MAX_SLICES 512
#define GS_KMEANS_MAX_N ((int64_t)0x7fffffff)
size_t gs_kmeans_workspace_bytes(int64_t n, int d, int k);
int gs_kmeans_assign(const float* x, int64_t ldx, int64_t n, int d, const float* centres, int k, int32_t* labels, float* dist, int32_t* changed,
                     double* inertia, void* ws, size_t ws_bytes, void* stream);
int gs_kmeans_inertia(const float* x, int64_t ldx, int64_t n, int d, const float* centres, int k, const int32_t* labels, double* inertia, void* ws,
                      size_t ws_bytes, void* stream);
int gs_kmeans_update(const float* x, int64_t ldx, int64_t n, int d, const int32_t* labels, int k, float* centres, int32_t* counts, void* ws,
                     size_t ws_bytes, void* stream);
int gs_kmeans_mindist(const float* x, int64_t ldx, int64_t n, int d, const float* centre, float* dist, int first, void* stream);

/* ---- sliced Wasserstein distance of Laplacian-pyramid patches (gansynth_amd/swd.py, metrics.sliced_wasserstein_distance_device; DESIGN.md
 * "SWD on the device") ----
 * fp32 values, sums in double, fixed orders, no float atomics: two calls with the same arguments write the same bits.  No sort library.
 * Images are channels-last [b][h][w][2], fp32 or bf16 (widened exactly at the first read).  Inputs are finite.
 *
 * gs_swd_levels (host arithmetic): the number L of l >= 0 with min(h, w) >> l >= 16; 0 (refused) when there is none, when a size that is halved
 * on the way down is odd, or when a side exceeds GS_SWD_MAX_SIDE.
 *
 * gs_swd_pyramid: lap receives the L Laplacian levels of x one after the other, level l as [b][h >> l][w >> l][2] fp32.  G_0 = x; G_{l+1} =
 * G_l filtered by outer(k, k) / 256, k = [1, 4, 6, 4, 1], at the even rows and columns, the border mirrored without the edge sample;
 * Lap_l = G_l - up(G_{l+1}) with up = zero stuffing to twice the size and 4 x the same filter under the same border rule; Lap_{L-1} = G_{L-1}.
 * Every product is exact (dyadic weights); a row of taps is summed left to right, then the row sums top to bottom.  ws holds G_1 .. G_{L-1}.
 *
 * gs_swd_patches: desc[row_offset + i * 128 + p][(c * 7 + dy) * 7 + dx] = level[i][ys[i * 128 + p] + dy][xs[i * 128 + p] + dx][c] for the b
 * images of one level ([b][h][w][2] fp32); ys, xs are int32 on the device, desc is [desc_rows][GS_SWD_DESC].  A corner outside
 * [0, h - 7] x [0, w - 7] is moved to the nearest one inside.
 *
 * gs_swd_moments: out[8] (double) = for channel 0 then channel 1 of desc [rows][GS_SWD_DESC]: the sum, the sum of squares, the mean and the
 * population standard deviation sqrt(max(0, sumsq / m - mean^2)) of its m = rows * 49 values.  Two launches: the blocks' shares, then their fold
 * in block order.
 *
 * gs_swd_project: out[j][i] = sum over k ascending (fp32 FMA) of a_ik * dirs[k][j], a_ik = (desc[i][k] - mean_c) / std_c with mean and std the
 * fp32 roundings of moments[2], [3] (k < 49) and moments[6], [7] (k >= 49); dirs is [GS_SWD_DESC][ndir], out [ndir][n]: a direction's n values
 * are contiguous.
 *
 * gs_swd_sort: every one of the `rows` rows of n floats of data (dense) ascending, in place (-0 before +0).  Tiles of GS_SWD_SORT_TILE values
 * are sorted in LDS, then ceil(log2(ceil(n / GS_SWD_SORT_TILE))) merge passes alternate between data and ws (rows * n floats when
 * n > GS_SWD_SORT_TILE).  n <= GS_SWD_MAX_N.  NaN is not ordered.
 *
 * gs_swd_l1: out[1] (double) = the sum of |a - b| over two dense [rows][n] buffers, differences and sums in double; a == b gives 0.
 *
 * gs_swd_workspace_bytes(stage, a, b, c) (host arithmetic; 0 for arguments the entry refuses): GS_SWD_STAGE_PYRAMID (b, h, w),
 * GS_SWD_STAGE_MOMENTS (rows), GS_SWD_STAGE_SORT (rows, n), GS_SWD_STAGE_L1 (rows, n).  ws is 16-byte aligned.  Capture-safe.
 * GS_ERR_ARG with a message and without a launch: a shape outside the stated limits, a NULL or misaligned pointer, a workspace that is too small. */
#define GS_SWD_DESC 98
#define GS_SWD_PATCHES 128
#define GS_SWD_SORT_TILE 4096
#define GS_SWD_MAX_N (1 << 21)
#define GS_SWD_MAX_ROWS 65535
#define GS_SWD_MAX_SIDE 16384
#define GS_SWD_MAX_BATCH 65536
#define GS_SWD_STAGE_PYRAMID 0
#define GS_SWD_STAGE_MOMENTS 1
#define GS_SWD_STAGE_SORT 2
#define GS_SWD_STAGE_L1 3
int gs_swd_levels(int h, int w);
size_t gs_swd_workspace_bytes(int stage, int64_t a, int64_t b, int64_t c);
int gs_swd_pyramid(const void* x, int dtype, int64_t b, int h, int w, float* lap, void* ws, size_t ws_bytes, void* stream);
int gs_swd_patches(const float* level, int64_t b, int h, int w, const int32_t* ys, const int32_t* xs, float* desc, int64_t desc_rows, int64_t row_offset,
                   void* stream);
int gs_swd_moments(const float* desc, int64_t rows, double* out, void* ws, size_t ws_bytes, void* stream);
int gs_swd_project(const float* desc, int64_t n, const double* moments, const float* dirs, int ndir, float* out, void* stream);
int gs_swd_sort(float* data, int64_t rows, int64_t n, void* ws, size_t ws_bytes, void* stream);
int gs_swd_l1(const float* a, const float* b, int64_t rows, int64_t n, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- k-nearest-neighbour radii and cover, for precision / recall / density / coverage (gansynth_amd/manifold.py,
 * metrics.precision_recall_device; DESIGN.md "Precision and recall on the device") ----
 * fp32, deterministic (no float atomics; a result is a multiset of values or an integer sum, so it depends neither on the slicing nor on any
 * merge order): two calls with the same arguments write the same bits.  Both sides are matrices of d columns with their rows lda / ldb (ldq /
 * ldr) >= d floats apart, 4-byte aligned.  Inputs are finite.  No distance is ever written to memory.
 *
 * The distance, in both entries: |x - y|^2 in fp32 as ONE chain over the columns in ascending order, t = x - y; acc = fmaf(t, t, acc), from
 * acc = 0 (never |x|^2 - 2 x.y + |y|^2: that form cancels on features with a common offset).  (x - y)^2 and (y - x)^2 have the same bits, so
 * d(i, j) has the same bits in either entry and from either side: a radius that gs_knn_kth returned admits, in gs_knn_within, exactly the
 * pairs that defined it.
 *
 * gs_knn_kth: out[i][0 .. k) = the k smallest values of |a_i - b_j|^2 over j in [0, m), ascending; with exclude_diagonal != 0 over j != i (the
 * index alone excludes: a duplicate of row i elsewhere is a candidate like any other and gives an exact 0).  Where fewer than k candidates
 * exist the rest is +inf.  out is [n][k] dense.
 *
 * gs_knn_within: count[i] (int32) = the number of j in [0, m) with |q_i - ref_j|^2 <= radius2[j].  A NaN radius admits nothing, a +inf radius
 * every row.
 *
 * One launch over a grid of (tiles of GS_KMEANS_TILE rows of the first side) x (slices of the second side), every block leaving its rows'
 * partial list or count in ws as [slices][n][k] floats or [slices][n] int32, and a fold over the slices; with one slice the block writes the
 * result itself and ws is not touched.  gs_knn_slices (host arithmetic; 0 for a shape the entries refuse; d does not enter today):
 *   slices = ceil(m / rows),  rows = max(GS_KNN_MIN_SLICE_ROWS, 64 * ceil(ceil(m / want) / 64)),  want = ceil(GS_KNN_BLOCKS / ceil(n / GS_KMEANS_TILE)).
 * gs_knn_workspace_bytes (host arithmetic; 0 for a shape the entries refuse): 16 with one slice, else 4 * slices * n * k rounded up to 16;
 * gs_knn_within needs that of k = 1.  ws is 16-byte aligned.  Capture-safe: no allocation, no synchronisation.
 * GS_ERR_ARG with a message that names the argument and without a launch: k outside [1, GS_KNN_MAX_K], d, n or m below 1, n or m above
 * GS_KMEANS_MAX_N, d above GS_KMEANS_MAX_D, a row stride below d, a NULL or misaligned pointer, a workspace that is too small. */
#define GS_KNN_MAX_K 8
#define GS_KNN_BLOCKS 3072
#define GS_KNN_MIN_SLICE_ROWS 256
size_t gs_knn_workspace_bytes(int64_t n, int64_t m, int d, int k);
int gs_knn_slices(int64_t n, int64_t m, int d);
int gs_knn_kth(const float* a, int64_t lda, int64_t n, const float* b, int64_t ldb, int64_t m, int d, int k, int exclude_diagonal, float* out, void* ws,
               size_t ws_bytes, void* stream);
int gs_knn_within(const float* q, int64_t ldq, int64_t n, const float* ref, int64_t ldr, int64_t m, int d, const float* radius2, int32_t* count, void* ws,
                  size_t ws_bytes, void* stream);

/* ---- YIN fundamental-frequency tracker (de Cheveigne & Kawahara 2002, steps 1-5), for gansynth_amd/pitch.py, metrics.f0_pitch_accuracy_device
 * and GANSynth.evaluate(f0=True); DESIGN.md "Pitch tracking on the device" ----
 * x holds `rows` rows of n fp32 samples, ldx >= n floats apart, 4-byte aligned (any 4-byte alignment); inputs are finite.  A row has
 * F = (n - W - L) / hop + 1 frames (integer division), frame f starts at t = f hop and reads x[t .. t + W + L - 2].  Deterministic: no float
 * atomics, two calls with the same arguments write the same bits.  Capture-safe: no allocation, no synchronisation, no workspace.
 *
 *   1. d(tau) = sum_{j < W} (x[t + j] - x[t + j + tau])^2 for tau in [0, L), the direct form in fp32 on the vector ALU, every term a rounded
 *      difference squared into an FMA, the terms added in a fixed order: within (W + 8) 2^-24, relative, of the exact sum, and d(0) = 0 exactly.
 *      (Never energy plus cross-correlation: that form cancels and has no relative bound.)  power = (1 / W) sum_{j < W} x[t + j]^2, in fp32,
 *      within the same bound.
 *   2. In float64: S(tau) = d(1) + ... + d(tau), added sequentially in ascending order; c(0) = 1, c(tau) = d(tau) tau / S(tau), and c(tau) = 1
 *      where S(tau) = 0.
 *   3. Over tau in [tau_min, L - 2]: the first tau with c(tau) < threshold, then, while tau + 1 <= L - 2 and c(tau + 1) < c(tau), tau + 1.  If
 *      no tau is under the threshold: the argmin of c over the range, the lowest index on a tie.
 *   4. den = c(tau - 1) - 2 c(tau) + c(tau + 1); offset = 0.5 (c(tau - 1) - c(tau + 1)) / den clamped to [-1, 1] if den > 0, else 0;
 *      period = tau + offset (float64), aperiodicity = c(tau).
 *
 * gs_yin_difference: rule 1.  d is [rows][F][L] fp32, power [rows][F] fp32, both dense.
 * gs_yin_pick: rules 2-4 on a dense d [rows][F][L].  lag is [rows][F] int32, period and aperiodicity [rows][F] float64 (8-byte aligned).
 * gs_yin_track: the production route, one launch, d never leaves the chip: the four outputs, bit for bit those of gs_yin_pick after
 *   gs_yin_difference (the same device code).
 * gs_yin_frames: host arithmetic; F, or 0 (and a message) for a shape the entries refuse.
 * GS_ERR_ARG with a message that names the argument, before anything is dereferenced or launched: rows < 1, hop < 1, tau_min < 2,
 * L outside [tau_min + 2, GS_YIN_MAX_LAGS] (gs_yin_difference: [4, GS_YIN_MAX_LAGS]), W outside [L, GS_YIN_MAX_WINDOW], n < W + L, ldx < n,
 * more than 2^31 - 1 frames in all, a NULL or misaligned pointer. */
#define GS_YIN_MAX_LAGS 1024
#define GS_YIN_MAX_WINDOW 4096
int64_t gs_yin_frames(int64_t n, int W, int L, int hop);
int gs_yin_difference(const float* x, int64_t ldx, int64_t rows, int64_t n, int W, int L, int hop, float* d, float* power, void* stream);
int gs_yin_pick(const float* d, int64_t rows, int64_t frames, int L, int tau_min, double threshold, int32_t* lag, double* period, double* aperiodicity,
                void* stream);
int gs_yin_track(const float* x, int64_t ldx, int64_t rows, int64_t n, int W, int L, int hop, int tau_min, double threshold, int32_t* lag, double* period,
                 double* aperiodicity, float* power, void* stream);

/* ---- the three kernel sums of the kernel inception distance (Binkowski et al. 2018), for gansynth_amd/kid.py,
 * metrics.kernel_inception_distance_device and GANSynth.evaluate(kid=True); DESIGN.md "KID on the device" ----
 * x is [n][d] and y [m][d] fp32, rows ldx / ldy >= d floats apart, 4-byte aligned (any 4-byte alignment); inputs are finite.  Nothing past a
 * row's d floats is read.  With k(a, b) = (a.b / d + 1)^3 the entry writes, as doubles,
 *   Sxx = sum over i != j of k(x_i, x_j),   Syy = sum over i != j of k(y_i, y_j),   Sxy = sum over all i, j of k(x_i, y_j).
 * The index alone excludes: a duplicate row elsewhere is a pair like any other.
 *
 * subsets == 0 (then xi == yi == NULL and size == 0): the full sets; out is [1][3] = Sxx, Syy, Sxy.
 * subsets >= 1: xi and yi are [subsets][size] int32 on the device, row r of subset s is x[xi[s size + r]] (y[yi[s size + r]]), found by the row
 * loader -- no gathered copy is made; out is [subsets][3].  The entry cannot see the lists: an index outside its set is the caller's to refuse
 * (kernels.kid_sums does); the loader clamps it into the set, so that no read ever leaves the matrices.
 *
 * Arithmetic: the features are widened fp32 -> fp64 (exact); a.b is accumulated in fp64 by v_mfma_f64_16x16x4_f64 over the columns in ascending
 * steps of 4 -- every product is exact, only the additions round; t = p / d + 1.0 and k = t t t in fp64; every sum in fp64 in one fixed order
 * (no float atomics): two calls with the same arguments write the same bits, and a subset's three sums have the same bits alone and as entry s of
 * a batch.  The longest chain of additions behind a sum: 63 (a lane's 64 values) + 8 (the block's tree over 256 lanes) +
 * ceil(tiles / 256) - 1 (a fold thread's partials, ascending) + 8 (the fold's tree), `tiles` the job's tile count below.
 *
 * One launch over (tiles, subsets) and a fold of (3, subsets) blocks.  A tile is GS_KID_TILE x GS_KID_TILE pairs; with T(r) = ceil(r /
 * GS_KID_TILE) and the rows a side r_x, r_y (n, m, or size) the symmetric jobs visit the upper triangle, T (T + 1) / 2 tiles, and Sxy
 * T(r_x) T(r_y).  No n x m array exists at any time; ws holds one double a tile:
 * gs_kid_workspace_bytes (host arithmetic; 0 for a shape the entry refuses) = 8 max(subsets, 1) (T_x (T_x + 1) / 2 + T_y (T_y + 1) / 2 + T_x T_y)
 * rounded up to 16.  ws is 16-byte aligned, out 8.  Capture-safe: no allocation, no synchronisation.
 * GS_ERR_ARG with a message that names the argument and without a launch: n or m outside [2, GS_KID_MAX_ROWS], d outside [1, GS_KMEANS_MAX_D],
 * a row stride below d, subsets outside [0, GS_KID_MAX_SUBSETS], lists or a size with subsets == 0, a NULL or misaligned list or a size outside
 * [2, min(n, m)] with subsets >= 1, a NULL or misaligned pointer, a workspace that is too small. */
#define GS_KID_TILE 128
#define GS_KID_MAX_ROWS 2097152
#define GS_KID_MAX_SUBSETS 65535
size_t gs_kid_workspace_bytes(int64_t n, int64_t m, int d, int subsets, int64_t size);
int gs_kid_sums(const float* x, int64_t ldx, int64_t n, const float* y, int64_t ldy, int64_t m, int d, const int32_t* xi, const int32_t* yi, int subsets,
                int64_t size, double* out /* [max(subsets, 1)][3]: Sxx, Syy, Sxy */, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GANSYNTH_HIP_H */
