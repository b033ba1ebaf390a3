// MFMA implicit-GEMM 3x3 convolution family for gfx950 (channels-last activations).
//
// One LDS-tiled kernel template covers the three "gather-form" maps
//   MODE_S1 : 3x3 stride-1 SAME conv            (also its bwd-data, with flipped/transposed taps)
//   MODE_S2 : 3x3 stride-2 TF-SAME conv         (pad 0 before / 1 after on even inputs)
//   MODE_T2 : 3x3 stride-2 transposed conv      (= bwd-data of MODE_S2; 4 sub-pixel phases, no
//                                                zero insertion: 1+2+2+4 = 9 taps per 2x2 outputs)
// (their weight gradients: conv_wgrad.hip).
//
// GEMM orientation is "swapped": the MFMA A operand is the weight tile (rows = output channels),
// the B operand is the pixel tile (cols = pixels).  D[oc][pixel] then leaves each lane holding 4
// consecutive output channels of ONE pixel per accumulator quad, which is exactly a 16-byte
// channels-last store, and keeps the per-pixel channel reduction (pixel-norm) lane-local.
//
// Reference call sites replaced: tf.nn.conv2d ops.py:237-243 and tf.nn.conv2d_transpose
// ops.py:269-276 (plus the tf.gradients of both, models.py:47,60,81-89).
#include "conv_device.h"
#include "gs_prof.h"

extern "C" int gs_pixel_norm_fwd(const void* x, void* y, int64_t p, int c, float eps, int dtype, void* stream);
extern "C" int gs_pack_act_bits(void* z, int64_t p, int c, int dtype, void* stream);
extern "C" int gs_pixel_norm_bwd_fused(const void* g, const void* x, const void* addend, void* gx, int64_t p, int c, float eps, int pre_act, int post_act, int dtype,
                                       void* stream);
extern "C" int gs_pixel_norm_bwd_bwd_fused(const void* gg, const void* g, const void* x, void* out, void* out_g, int64_t p, int c, float eps, int pre_act,
                                           int dtype, void* stream);

namespace gs {

// ------------------------------------------------------------------------- implicit GEMM
// Persistent kernel fed by LDS-DMA.  Block = 256 threads = 4 waves; every wave owns all 32*A output
// channels of the block and 32*B of its 128*B base pixels.  A block walks a list of work items (spatial
// tile x output-channel tile; the list of an XCD is contiguous so that neighbouring tiles share halo rows
// in that XCD's L2).  The K loop runs over stages = input-channel chunks of 64 bytes (16 f32 / 32 bf16)
// x tap groups.
//
// Staging: nothing passes through registers.  Every operand row is 64 bytes = four 16-byte slots, and a
// `buffer_load_dwordx4 ... lds` wave-instruction deposits 64 slots (1 KiB, 16 rows) at M0 + 16*lane while
// each lane supplies its own source offset -- so the XOR slot swizzle that makes the 16-lane ds_read_b128
// groups conflict-free is applied on the SOURCE side (lane at slot position p fetches part p ^ key(row)).
// Out-of-image patch rows are free: the descriptor covers exactly one image, rows above / below it fall
// outside [0, num_records) and the hardware writes zeros (measured, scripts/probe/dma_probe.hip); columns
// left / right of the image are forced out of range per lane.
// The stages of the next D iterations are always in flight (ring of D+1 weight buffers, 1+ceil(D/NTG) patch
// buffers); a wave waits with a COUNTED s_waitcnt vmcnt(n) -- n = its DMA pieces of the stages that may
// still be in flight -- and one raw s_barrier per stage publishes the landed stage to the other waves.
// hipcc knows nothing about these loads (inline asm), so it adds no vmcnt(0) of its own; the main loop has
// no ordinary global loads (the bias lives in LDS), only the epilogue stores.
// TG == 9 with RESIDENT keeps all taps of all chunks in LDS for the life of the block (thin layers: 32 or
// 64 output channels) and only the input patches stream.
struct ConvP {
    const void* x;
    const void* wp;
    void* y;
    const float* bias;  // optional fused epilogue: y = act(alpha * conv + bias)
    int act;
    const void* mask;   // optional (data gradients): y *= mask_act'(.) expressed through the activation OUTPUT mask[..] (y's shape)
    int mask_act;
    // 1-bit leaky-relu masks (bf16, plain epilogues): the sign bits of an activation output, one dword per (pixel, 32-channel tile) -- bit
    // 8 (2 hi + qp) + k is channel 16 qp + 8 hi + k of the tile, the order the lanes store their 16-byte pieces in -- written by the forward
    // epilogue BEHIND the activation itself (same allocation: z [numel] then numel / 8 bytes) and read by the masked epilogues instead of z:
    // 1/16 of the mask bytes of a launch that is HBM-bound at the top of the pyramid.  (gs_common.h: GS_ACT_LRELU_BITS / GS_ACT_WRITE_BITS)
    const unsigned char* mask_bits;
    unsigned char* bits_out;
    void* y2;           // optional (NORM == 1 kernels): y2 = pixel_norm(y) over the channels, y itself optional then
    float pn_eps;
    // NORM == 2 kernels (data gradients): the conv result g is the gradient w.r.t. y = pixel_norm(z) of the PREVIOUS block; the epilogue turns it
    // into the gradient w.r.t. that block's pre-activation, y = (pixel_norm_bwd(g, z) + addend) * mask_act'(z), with z = `mask` (the
    // activation output, y's shape) and `addend` an optional second gradient into z (same shape): one pass instead of a conv + a 4-tensor
    // elementwise pass
    const void* addend;
    // NORM == 3 kernels (second-order pass): the conv result t is the gradient w.r.t. u = act'(z) pixel_norm_bwd(g, z) (the first-order backward
    // of a generator block, differentiated by the mode-seeking term).  With h = t act'(z): y = pixel_norm_bwd(h, z) (the gradient w.r.t. g) and
    // y2 = d<h, pixel_norm_bwd(g, z)>/dz (the gradient w.r.t. z); z = `mask`, g = `addend`'s slot.  Same normbwd flag, value 2.
    int normbwd;        // host side: the caller asks for the NORM == 2 epilogue; cleared (and *norm_pending = 2) when the chosen kernel has none
    int* norm_pending;  // host side: set to 1 when the chosen kernel did not fuse the norm
    int N, Hi, Wi, IC, OC, Hb, Wb, tiles_x, tiles_y, nsp, noct, nch;
    // ceil(2^32 / d) for d = noct, tiles_x, tiles_y (0 for d = 1): item -> (image, tile row, tile column, channel tile) with one s_mul_hi_u32 per
    // division instead of the ~20 scalar instructions of a signed division each -- on the 32-channel layers (36 MFMAs per tile) the tile's time
    // IS its instruction count (a wave issues one instruction per ~5 cycles), and an item is decoded twice (issue cursor, compute side)
    unsigned m_noct, m_tx, m_ty;
    float alpha;
#ifdef GS_IGEMM_TRACE
    unsigned long long* trace;  // [block][64] shader-clock stamps of wave 0 (scripts/probe/igemm_trace.hip)
#endif
};
#ifdef GS_IGEMM_TRACE
#define GS_TR(slot)                                                                                              \
    do {                                                                                                         \
        if (p.trace && threadIdx.x == 0 && (slot) < 64) {                                                        \
            p.trace[blockIdx.x * 64 + (slot)] = __builtin_amdgcn_s_memtime();                                    \
            if ((slot) == 0 || (slot) == 63) p.trace[4096 * 64 + blockIdx.x * 2 + ((slot) == 63)] = __builtin_amdgcn_s_memrealtime(); \
        }                                                                                                        \
    } while (0)
#else
#define GS_TR(slot) do { } while (0)
#endif

// lds_dma16 (conv_device.h) with a scalar offset: address = base + voff + soff, and soff takes part in the descriptor's range check (measured,
// scripts/probe/dma_probe.hip mode 2) -- so the per-piece part of a WEIGHT address that is uniform over the wave stays in an SGPR and the
// piece costs no VALU instruction at all (a wave issues one instruction per ~4-5 cycles: profiles/r05_c_igemm_mid_timeline.txt prices a
// DMA piece at ~31 cycles of a stage, i.e. at its instruction count).  Only for offsets that never go negative (weights: yes; the
// patch origin of a border tile: no -- a 33-bit sum of a negative soff would not wrap back into range).
__device__ __forceinline__ void lds_dma16_s(unsigned lds_addr, unsigned voff, i32x4 rs, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(lds_addr), "v"(voff), "s"(rs), "s"(__builtin_amdgcn_readfirstlane(soff))   // (uniform by construction; the compiler cannot always prove it)
                 : "memory", "m0");
}

// RB: bytes of an operand row in LDS = of a channel chunk (64: four 16-byte slots, the original layout; 128: eight slots, whole
// 128-byte cache lines per DMA row -- 53-60 instead of 30 B/cycle/CU through the L2 -> LDS path, scripts/probe/dma_rate.hip -- and
// half the stages, barriers and DMA round trips per item; bf16 only)
// SPEC: wave-specialised block of 8 waves -- waves 0-3 run the fragment reads, MFMAs and the epilogue exactly as before, waves 4-7
// (one on each SIMD beside its compute wave) issue every DMA piece and hold the counted waits.  A wave issues one instruction per
// ~5 cycles whatever it is (scripts/probe/valu_rate.hip), so in a 4-wave block the ~60 cycles of each DMA piece (offset arithmetic,
// M0, the load) come ON TOP of the MFMAs of the stage -- measured 2260 ticks per stage for 1152 ticks of MFMA on the few-block layers
// (scripts/probe/igemm_trace.hip); on their own wave they run under them.
#ifndef GS_NORM_EPI_PIPELINE
#define GS_NORM_EPI_PIPELINE 1   // (0: the fused norm-backward epilogues fetch z / addend where they use them -- the build to compare against)
#endif
// BITS (bf16, plain epilogues): the build of the kernel for launches with 1-bit leaky-relu masks -- its mask, if any, is the sign words behind
// an activation (p.mask_bits), and with p.bits_out it writes the sign words of its own result.  Its own instantiation, not a run-time branch: with
// both mask forms in one epilogue the compiler keeps 15-25 more VGPRs live and the larger tiles lose a wave of occupancy.
template <typename T, int MODE, int A, int B, int TW, int TG, bool RESIDENT, int D, int NORM, int RB = 64, bool SPEC = false, bool BITS = false>
__global__ __launch_bounds__(SPEC ? 512 : 256) void conv_igemm_kernel(const ConvP p) {
    static_assert(NORM >= 0 && NORM <= 3, "NORM: 0 plain, 1 pixel norm of the result (forward blocks), 2 pixel-norm backward of the result (data gradients), "
                                          "3 both gradients of a differentiated norm backward (second-order pass)");
    constexpr int NP = 128 * B;
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int S = MODE == MODE_S2 ? 2 : 1;
    constexpr int NPH = MODE == MODE_T2 ? 4 : 1;
    constexpr int SZ = (int)sizeof(T);
    static_assert(RB == 64 || (RB == 128 && SZ == 2), "128-byte rows: bf16 only");
    constexpr int BK = RB / SZ;
    constexpr int SL = RB / 16;               // 16-byte slots per row
    constexpr int KS = RB / 32;               // MFMA k-steps per row (a k-step = two slots: one per lane half)
    constexpr int OCT = 32 * A;
    constexpr int NTG = 9 / TG;
    constexpr int PCH = PH * PW * SL;         // 16-byte slots of a patch chunk
    constexpr int NPP = (PCH + 63) / 64;      // its 1 KiB DMA pieces ...
    constexpr int PP = (NPP + 3) / 4;         // ... per wave
    constexpr int PBUF = PP * 4096;           // bytes of one patch buffer (whole pieces for every wave; the excess is zero-filled)
    constexpr int WBYTES = TG * OCT * RB;     // bytes of one weight stage
    constexpr int NWP = WBYTES / 1024;
    constexpr int WP = (NWP + 3) / 4;
    constexpr int WBUF = WP * 4096;           // bytes of one weight buffer
    constexpr int NPB = 1 + (D + NTG - 1) / NTG;  // patch ring
    constexpr int NWB = D + 1;                    // weight ring
    constexpr int NSTEP = KS * TG;                // (tap, k-step) MFMA steps of a stage
    typedef typename Mma<T>::frag_t frag_t;

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* const lpatch = lds;                // NPB x PBUF
    unsigned char* const lwgt = lds + NPB * PBUF;     // streamed: NWB x WBUF ; resident: nch x WBUF
    float* const lbias = reinterpret_cast<float*>(lwgt + (RESIDENT ? p.nch : NWB) * WBUF);  // OC floats (zeros without a bias)
    const unsigned a_patch = (unsigned)(uintptr_t)lds;  // low 32 bits of a flat LDS address = the LDS byte address
    const unsigned a_wgt = a_patch + NPB * PBUF;

    const T* __restrict__ wp = reinterpret_cast<const T*>(p.wp);
    T* __restrict__ y = reinterpret_cast<T*>(p.y);
    const int Hi = p.Hi, Wi = p.Wi, IC = p.IC, OC = p.OC, Hb = p.Hb, Wb = p.Wb, NCH = p.nch;

    const int tid = threadIdx.x;
    const int lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wv8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = SPEC && wv8 >= 4;     // issues the DMA; !loader computes
    const bool issuer = !SPEC || loader;
    const bool computer = !SPEC || !loader;
    const int wv = wv8 & 3;                   // index within the role: the wave's DMA pieces / its 32*B pixels

    // ---- this block's item list (XCD-contiguous when the grid is a multiple of 8)
    const int total = p.nsp * p.noct;
    int first, stride, count;
    if ((gridDim.x & 7) == 0) {
        const int per_xcd = (total + 7) >> 3, gx = gridDim.x >> 3;
        const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
        first = xcd * per_xcd + loc;
        stride = gx;
        int end = (xcd + 1) * per_xcd;
        if (end > total) end = total;
        count = first < end ? (end - first + gx - 1) / gx : 0;
    } else {
        first = blockIdx.x;
        stride = gridDim.x;
        count = first < total ? (total - first + stride - 1) / stride : 0;
    }
    if (count == 0) return;
    GS_TR(0);

    // ---- per-lane DMA source descriptors, constant for the life of the block
    int p_voff[PP], p_lx[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) {
        const int slot = (wv + 4 * k) * 64 + lane;
        const int row = slot / SL, pos = slot % SL;
        const int ly = row / PW, lx = row - ly * PW;
        // slot swizzle: rows one bank row (256 bytes) apart must land on different slots -- every 4th row of 64 bytes, every 2nd of 128
        p_voff[k] = ((ly * Wi + lx) * IC) * SZ + ((pos ^ (RB == 64 ? (lx >> 2) & 3 : (lx >> 1) & 7)) << 4);
        p_lx[k] = slot < PCH ? lx : 0x40000000;  // never inside the image
    }
    // a 1 KiB weight piece = RPP rows of the stage; row r of a 32-row channel tile takes slot key (r >> 2) & 3 (64-byte rows) or
    // (r >> 1) & 7 (128-byte rows: pieces of 8 rows, so the key also depends on the parity of the piece: two lane offsets)
    constexpr int RPP = 1024 / RB;            // rows per piece
    constexpr int SUBS = OCT / RPP;           // pieces per tap
    const int w_lane0 = RB == 64 ? ((lane >> 2) * IC) * SZ + (((lane & 3) ^ ((lane >> 4) & 3)) << 4)
                                 : ((lane >> 3) * IC) * SZ + (((lane & 7) ^ (lane >> 4)) << 4);
    const int w_lane1 = RB == 64 ? w_lane0 : ((lane >> 3) * IC) * SZ + (((lane & 7) ^ (4 + (lane >> 4))) << 4);
    // block-constant scalar part of every weight piece: rows [tap tt][RPP*sub ..] of the stage (T2 walks the taps phase by phase)
    int w_soff[NTG][WP];
    bool w_odd[WP];
#pragma unroll
    for (int k = 0; k < WP; ++k) w_odd[k] = RB == 128 && (((wv + 4 * k) % SUBS) & 1);
#pragma unroll
    for (int tg = 0; tg < NTG; ++tg)
#pragma unroll
        for (int k = 0; k < WP; ++k) {
            const int j = wv + 4 * k;
            const int tt = j / SUBS, sub = j % SUBS;
            const int i = tg * TG + tt;
            const int wt = MODE == MODE_T2 ? (int)((0x453718620ULL >> (4 * (i < 9 ? i : 0))) & 15) : i;
            w_soff[tg][k] = (NWP % 4 == 0 || j < NWP) ? ((wt * OC + sub * RPP) * IC) * SZ : (int)0x80000000;
        }
    const unsigned img_bytes = (unsigned)Hi * Wi * IC * SZ;
    const unsigned w_bytes = 9u * IC * OC * SZ;
    i32x4 rs_w = make_rsrc(wp, w_bytes);
    const unsigned a_wave = wv * 1024;

    auto item_coords = [&](int item, int& n, int& by, int& bx, int& oc0) __attribute__((always_inline)) {
        // (exact: item < 2^21 and every divisor < 2^11, so item * (m d - 2^32) < 2^32)
        const unsigned it = (unsigned)item;
        const unsigned sp = p.m_noct ? __umulhi(it, p.m_noct) : it;
        oc0 = (int)(it - sp * (unsigned)p.noct) * OCT;
        const unsigned r = p.m_tx ? __umulhi(sp, p.m_tx) : sp;
        const int tile_x = (int)(sp - r * (unsigned)p.tiles_x);
        const unsigned nn = p.m_ty ? __umulhi(r, p.m_ty) : r;
        by = (int)(r - nn * (unsigned)p.tiles_y) * TH;
        bx = tile_x * TW;
        n = (int)nn;
    };

    // ---- issue side: cursor over (item, chunk); the tap group is a compile-time value at every call site
    int i_item = first, i_left = count, i_ch = 0, i_pb = 0, i_wb = 0;
    int i_n, i_by, i_bx, i_oc0;
    item_coords(i_item, i_n, i_by, i_bx, i_oc0);
    int i_oy0 = 0, i_ox0 = 0, i_org = 0;
    i32x4 rs_x = make_rsrc(p.x, img_bytes);

    // Past the end of the item list the stages are still "issued" (the counted waits stay static) but against empty
    // descriptors: every lane is out of range, nothing is fetched, zeros land in ring slots nobody reads again.
    int i_wbase = 0;
    auto issue_setup = [&](int tg) __attribute__((always_inline)) {  // scalars of the stage about to be issued
        const bool more = i_left > 0;
        if (tg == 0) {
            i_oy0 = MODE == MODE_S2 ? 2 * i_by : i_by - 1;
            i_ox0 = MODE == MODE_S2 ? 2 * i_bx : i_bx - 1;
            i_org = ((i_oy0 * Wi + i_ox0) * IC + i_ch * BK) * SZ;
            rs_x = make_rsrc(reinterpret_cast<const unsigned char*>(p.x) + (size_t)(more ? i_n : 0) * img_bytes, more ? img_bytes : 0u);
        }
        if (!RESIDENT) {
            rs_w[2] = more ? (int)w_bytes : 0;
            i_wbase = (i_oc0 * IC + i_ch * BK) * SZ;
        }
    };
    auto issue_patch_piece = [&](int k) __attribute__((always_inline)) {
        const unsigned voff = (unsigned)(i_ox0 + p_lx[k]) < (unsigned)Wi ? (unsigned)(i_org + p_voff[k]) : 0x80000000u;
        lds_dma16(a_patch + a_wave + i_pb * PBUF + k * 4096, voff, rs_x);
    };
    auto issue_weight_piece = [&](int k, int tg, int wbase, unsigned dst_base) __attribute__((always_inline)) {
        // (pieces past the end of the stage carry 0x80000000: out of range for any descriptor)
        // (the lane part is loop-invariant, the rest is wave-uniform and >= 0: scalar offset.  Pieces past the end of the stage carry
        //  0x80000000 in w_soff: base + 2^31 is out of range for any descriptor, with or without wbase on top)
        lds_dma16_s(dst_base + a_wave + k * 4096, (unsigned)(w_odd[k] ? w_lane1 : w_lane0), rs_w, (unsigned)(w_soff[tg][k] + wbase));
    };
    constexpr int NPW = RESIDENT ? 0 : WP;
    auto stage_pieces = [](int tg) { return (tg == 0 ? PP : 0) + NPW; };  // DMA pieces a wave issues for a stage
    // piece q of the stage being issued (patch pieces first)
    auto issue_piece = [&](int q, int tg) __attribute__((always_inline)) {
        const int np = tg == 0 ? PP : 0;
        if (q < np) issue_patch_piece(q);
        else issue_weight_piece(q - np, tg, i_wbase, a_wgt + i_wb * WBUF);
    };
    auto issue_advance = [&](int tg) __attribute__((always_inline)) {
        if (tg == 0) i_pb = i_pb + 1 == NPB ? 0 : i_pb + 1;
        if (!RESIDENT) i_wb = i_wb + 1 == NWB ? 0 : i_wb + 1;
        if (tg == NTG - 1) {
            if (++i_ch == NCH) {
                i_ch = 0;
                --i_left;
                i_item += stride;
                if (i_left > 0) item_coords(i_item, i_n, i_by, i_bx, i_oc0);
                else i_left = 0;
            }
        }
    };

    f32x16 acc[NPH][A][B];
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int b = 0; b < B; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ph][a][b][r] = 0.f;
    };

    // fragment byte offsets with the slot swizzle folded in: B side per (pixel group, horizontal tap offset, k step),
    // A side per k step; the vertical tap offset and the tap / channel-tile row are compile-time immediates
    int b_off[B][3][KS], a_off[KS];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int q = (wv * B + b) * 32 + l31;
        const int pb0 = ((q / TW) * S) * PW + (q % TW) * S;
#pragma unroll
        for (int ox = 0; ox < 3; ++ox) {
            const int lx = (q % TW) * S + ox;
            const int key = RB == 64 ? (lx >> 2) & 3 : (lx >> 1) & 7;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b_off[b][ox][ks] = (pb0 + ox) * RB + (((ks * 2 + hi) ^ key) << 4);
        }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a_off[ks] = l31 * RB + (((ks * 2 + hi) ^ (RB == 64 ? (l31 >> 2) & 3 : (l31 >> 1) & 7)) << 4);

    // ---- prologue: resident weights and the first D stages go out first, the bias is staged while they fly (hipcc waits
    //      vmcnt(0) for the bias loads, which drains the DMAs too -- at this point that is exactly the wait that is needed)
    GS_TR(1);
    if (issuer) {
        if (RESIDENT) {
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int k = 0; k < WP; ++k) issue_weight_piece(k, 0, (i_oc0 * IC + ch * BK) * SZ, a_wgt + ch * WBUF);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            issue_setup(d % NTG);
#pragma unroll
            for (int q = 0; q < stage_pieces(d % NTG); ++q) issue_piece(q, d % NTG);
            issue_advance(d % NTG);
        }
    }
    GS_TR(2);
    for (int c = tid; c < OC; c += (SPEC ? 512 : 256)) lbias[c] = p.bias ? p.bias[c] : 0.f;
    // Everything the first MFMA needs besides the landed stage is computed HERE, in the shadow of the DMA round trip: left to itself hipcc
    // sinks the fragment-offset tables and the accumulator clears behind the barrier (their first use) -- ~340 instructions between "stage 0
    // landed" and the first MFMA of every block of every launch (profiles/r05_c_igemm_rb128_isa_slots.txt, slot 0); pinned here, ~180 of
    // them run before the barrier.  (Ordering the table arithmetic behind the first DMA statements as well -- opaque lane ids -- costs the
    // common subexpressions of the tables: +118 instructions, the last piece goes out later; measured in the ISA, not adopted.)
    zero_acc();
    if (computer) {
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int ox = 0; ox < 3; ++ox)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(b_off[b][ox][ks]));
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(a_off[ks]));
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int b = 0; b < B; ++b) asm volatile("" : "+v"(acc[ph][a][b]));
    }
    wait_vmcnt(0);
    block_barrier();
    GS_TR(3);
#ifdef GS_IGEMM_TRACE
    int tr_stage = 0;
#endif

    int item = first, done = 0, c_pb = 0, c_wb = 0;
    while (true) {
        int n, by, bx, oc0;
        item_coords(item, n, by, bx, oc0);
        // BITS: the sign words of the lane's pixels, fetched at the START of the item's last stage -- one register per (pixel, 32-channel tile), so
        // they can wait through the MFMAs of the stage, where the 16-byte mask vectors (8-32 registers) cannot: a mask fetched in the epilogue
        // costs every item one exposed memory round trip (~0.9 us per 256-pixel item on the 32-channel layers: scripts/mask_bits_micro.py).
        unsigned mbw[BITS ? B * (MODE == MODE_T2 ? 4 : 1) : 1][A];
        // NORM 2 / 3 (the fused pixel-norm backward epilogues): the z vectors and the addend / g vectors of the lane's (pixel group, phase) steps, double
        // buffered -- step 0 is fetched at the start of the item's last stage like the sign words above, step i + 1 while step i is computed: fetched
        // where they are used, every step pays a memory round trip (1-4 per item).  Free registers: two blocks per CU leave a wave 256 VGPRs.
        // (not the 2 x 2 tiling: 64 more registers would take it past 256 and to one block per CU)
        constexpr bool NPIPE = (NORM == 2 || NORM == 3) && A * B <= 2 && GS_NORM_EPI_PIPELINE;
        typedef typename std::conditional<SZ == 4, float4, uint4>::type nvec_t;
        constexpr int NNV = SZ == 4 ? 4 : 2;
        nvec_t nz[NPIPE ? 2 : 1][A][NNV], nx[NPIPE ? 2 : 1][A][NNV];
        auto norm_fetch = [&](int i, nvec_t (&zq)[A][NNV], nvec_t (&xq)[A][NNV]) __attribute__((always_inline)) {
            constexpr int NPHB = MODE == MODE_T2 ? 4 : 1;
            const int b = i / NPHB, ph = i % NPHB;
            const int Ho = MODE == MODE_T2 ? 2 * Hb : Hb, Wo = MODE == MODE_T2 ? 2 * Wb : Wb;
            const int q = (wv * B + b) * 32 + l31;
            const int gy = by + q / TW, gx = bx + q % TW;
            const int oy = MODE == MODE_T2 ? 2 * gy + (ph >> 1) : gy;
            const int ox = MODE == MODE_T2 ? 2 * gx + (ph & 1) : gx;
            const long base = (gy < Hb && gx < Wb) ? (((long)n * Ho + oy) * Wo + ox) * OC + oc0 : 0;   // clamped: the loads stay unconditional
#ifdef GS_ABL_NOMASKLOAD
            const long zbase = base & 1023;
#else
            const long zbase = base;
#endif
#pragma unroll
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int v = 0; v < NNV; ++v) {
                    zq[a][v] = *reinterpret_cast<const nvec_t*>(reinterpret_cast<const T*>(p.mask) + zbase + a * 32 + v * (32 / NNV) + hi * (16 / NNV));
                    if (NORM == 3 || p.addend)
                        xq[a][v] = *reinterpret_cast<const nvec_t*>(reinterpret_cast<const T*>(p.addend) + base + a * 32 + v * (32 / NNV) + hi * (16 / NNV));
                }
        };
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int tg = 0; tg < NTG; ++tg) {
                const int itg = (tg + D) % NTG;            // tap group of the stage issued during this one
                const int npiece = stage_pieces(itg);
                if (issuer) issue_setup(itg);
                if constexpr (NPIPE) {
                    if (tg == NTG - 1 && ch == NCH - 1 && computer) norm_fetch(0, nz[0], nx[0]);
                }
                if constexpr (BITS) {
                    if (tg == NTG - 1 && ch == NCH - 1 && computer && p.mask_bits) {
                        constexpr int NPHB = MODE == MODE_T2 ? 4 : 1;
                        const int Ho = MODE == MODE_T2 ? 2 * Hb : Hb, Wo = MODE == MODE_T2 ? 2 * Wb : Wb;
#pragma unroll
                        for (int b = 0; b < B; ++b) {
                            const int q = (wv * B + b) * 32 + l31;
                            const int gy = by + q / TW, gx = bx + q % TW;
#pragma unroll
                            for (int ph = 0; ph < NPHB; ++ph) {
                                const int oy = MODE == MODE_T2 ? 2 * gy + (ph >> 1) : gy;
                                const int ox = MODE == MODE_T2 ? 2 * gx + (ph & 1) : gx;
                                const long off = (gy < Hb && gx < Wb) ? (((long)n * Ho + oy) * Wo + ox) * OC + oc0 : 0;   // clamped: unconditional loads
#pragma unroll
                                for (int a = 0; a < A; ++a) mbw[b * NPHB + ph][a] = *reinterpret_cast<const unsigned*>(p.mask_bits + ((off + a * 32) >> 3));
                            }
                        }
                    }
                }
                if (SPEC && loader) {   // the whole stage +D in one go, under the compute waves' MFMAs
#pragma unroll
                    for (int q = 0; q < npiece; ++q) issue_piece(q, itg);
                }
                // ---- MFMAs of this stage; fragment reads run one (tap, k-step) ahead, the DMA pieces of stage +D are
                //      spread over the steps
                const unsigned char* lp = lpatch + c_pb * PBUF;
                const unsigned char* lw = RESIDENT ? lwgt + ch * WBUF : lwgt + c_wb * WBUF;
                if (computer) {
                    constexpr int PF = NSTEP >= 6 ? 2 : 1;   // fragment reads run PF steps ahead of their MFMAs (LDS latency with 4
                                                             // waves on the pipe exceeds one step of 2-4 MFMAs)
                    frag_t af[PF + 1][A], bf[PF + 1][B];
                    // one fragment read of (step, r): r < A -> weight rows of channel tile r, else pixel group r - A
                    auto load_frag = [&](int step, int r) __attribute__((always_inline)) {
                        const int tt = step / KS, ks = step % KS, buf = step % (PF + 1);
                        const int i = tg * TG + tt;
                        const int oyv = tap_off<MODE>(tap_ky<MODE>(i)), oxv = tap_off<MODE>(tap_kx<MODE>(i));
                        if (r < A) af[buf][r] = *reinterpret_cast<const frag_t*>(lw + (tt * OCT + r * 32) * RB + a_off[ks]);
                        else bf[buf][r - A] = *reinterpret_cast<const frag_t*>(lp + oyv * PW * RB + b_off[r - A][oxv][ks]);
                    };
#if !defined(GS_ABL_NOMMA)
#pragma unroll
                    for (int st0 = 0; st0 < PF; ++st0)
#pragma unroll
                        for (int r = 0; r < A + B; ++r) load_frag(st0, r);
#endif
                    // Every MFMA is followed by its share of the other work of the step -- the fragment reads of step+1 and
                    // the DMA pieces of stage +D -- and the order is pinned: with one wave per SIMD only what is issued
                    // inside an MFMA's 32-cycle shadow is free, and left alone hipcc sinks the reads next to their consumers.
                    constexpr int NMMA = A * B;
                    constexpr int RPM = (A + B + NMMA - 1) / NMMA;            // reads per MFMA slot
                    const int ppm = (npiece + NSTEP * NMMA - 1) / (NSTEP * NMMA);  // DMA pieces per MFMA slot
#pragma unroll
                    for (int step = 0; step < NSTEP; ++step) {
                        const int ph = tap_phase<MODE>(tg * TG + step / KS);
#pragma unroll
                        for (int m = 0; m < NMMA; ++m) {
#ifndef GS_ABL_NOMMA
                            Mma<T>::mma(af[step % (PF + 1)][m / B], bf[step % (PF + 1)][m % B], acc[ph][m / B][m % B]);
#if !defined(GS_ABL_NOFRAG)
                            if (step + PF < NSTEP) {
#pragma unroll
                                for (int r = m * RPM; r < (m + 1) * RPM && r < A + B; ++r) load_frag(step + PF, r);
                            }
#endif
#endif
#ifndef GS_ABL_NODMA
                            if constexpr (!SPEC) {
                                const int slot = step * NMMA + m;
#pragma unroll
                                for (int q = slot * ppm; q < (slot + 1) * ppm && q < npiece; ++q) issue_piece(q, itg);
                            }
#endif
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                if (issuer) issue_advance(itg);
                // ---- the next stage must have landed before the barrier below: leave only the younger stages in flight
                if (issuer) {
                    int younger = 0;
#pragma unroll
                    for (int d = 2; d <= D; ++d) younger += stage_pieces((tg + d) % NTG);
#ifndef GS_ABL_NODMA
                    wait_vmcnt(younger);
#endif
                }
                // ---- epilogue of the item.  D[oc][pixel]: a lane holds oc = 8q + 4hi + (0..3) of pixel l31 per accumulator quad.
                //      The store path sustains ~7 B/cycle/CU with 8-byte stores and twice that with 16-byte ones (measured with
                //      the ablations of scripts/probe/igemm_trace.hip: the top-of-pyramid layers are bound by it), so a lane must
                //      leave with 16 bytes.  fp32: a quad is 16 bytes.  bf16: v_permlane32_swap exchanges the quads q / q+1
                //      between the two lane halves, after which lane (pixel, hi) owns 8 consecutive channels 16*(q/2) + 8*hi + ...
#ifndef GS_ABL_NOEPI
                if (tg == NTG - 1 && ch == NCH - 1 && computer) {
                    const int Ho = MODE == MODE_T2 ? 2 * Hb : Hb, Wo = MODE == MODE_T2 ? 2 * Wb : Wb;
                    const float slope = p.act == GS_ACT_LRELU ? 0.2f : 1.f;
                    auto mask_factor = [&](float z) __attribute__((always_inline)) {
                        return p.mask_act == GS_ACT_LRELU ? (z > 0.f ? 1.f : 0.2f) : (p.mask_act == GS_ACT_TANH ? 1.f - z * z : 1.f);
                    };
                    // the 32 channels of tile a of one pixel: act(alpha * acc + bias); o[qd][e] = channel 8 qd + 4 hi + e
                    auto finish = [&](int ph, int a, int b, float (&o)[4][4]) __attribute__((always_inline)) {
#pragma unroll
                        for (int qd = 0; qd < 4; ++qd) {
                            const float4 bv = *reinterpret_cast<const float4*>(lbias + oc0 + a * 32 + qd * 8 + hi * 4);
                            const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float v = acc[ph][a][b][qd * 4 + e] * p.alpha + bb[e];
                                o[qd][e] = fmaxf(v, slope * v);  // leaky relu (slope 1: identity)
                            }
                        }
                    };
                    // ... to dst[off + a * 32 + ...] (16 bytes per lane), optionally times mask_act'(.) through mask[off + ...]
                    // The mask vectors of a lane (its 16-byte pieces of the activation output, laid out like its stores) are fetched
                    // AHEAD of the arithmetic, several at a time: loaded where they are used, each costs the lane a full memory
                    // round trip (4-8 dependent trips per tile).
                    typedef typename std::conditional<SZ == 4, float4, uint4>::type mvec_t;
                    constexpr int NV = SZ == 4 ? 4 : 2;              // mask vectors per 32-channel tile of a pixel
                    constexpr bool use_mb = BITS;   // (1-bit masks: bf16, plain epilogues)
                    const bool emit_bits = BITS && p.bits_out != nullptr;
                    auto mask_fetch = [&](long off, bool inside, mvec_t (&mz)[A][NV]) __attribute__((always_inline)) {
#ifdef GS_ABL_NOMASKLOAD   // (ablation build only: every mask load hits the same few cache lines -- what would a mask of no bytes be worth?)
                        const long base = (inside ? off : 0) & 1023;
#else
                        const long base = inside ? off : 0;          // clamped: the loads stay unconditional
#endif
#pragma unroll
                        for (int a = 0; a < A; ++a)
#pragma unroll
                            for (int v = 0; v < NV; ++v)
                                mz[a][v] = *reinterpret_cast<const mvec_t*>(reinterpret_cast<const T*>(p.mask) + base + a * 32 + v * (32 / NV) + hi * (16 / NV));
                    };
                    auto store = [&](T* dst, long off, int a, float (&o)[4][4], bool inside, const mvec_t* mz, int mkind = 0,
                                     bool emit = false) __attribute__((always_inline)) {   // mkind: 0 no mask, 1 mask values in mz, 2 mask bits in mz[0].x
                        if constexpr (SZ == 4) {
#pragma unroll
                            for (int qd = 0; qd < 4; ++qd) {
                                if (mkind == 1) {
                                    const float4 zv = mz[qd];
                                    if (p.mask_act == GS_ACT_LRELU) {   // (the common case by itself: compare, scale, select per value)
                                        o[qd][0] = zv.x > 0.f ? o[qd][0] : 0.2f * o[qd][0]; o[qd][1] = zv.y > 0.f ? o[qd][1] : 0.2f * o[qd][1];
                                        o[qd][2] = zv.z > 0.f ? o[qd][2] : 0.2f * o[qd][2]; o[qd][3] = zv.w > 0.f ? o[qd][3] : 0.2f * o[qd][3];
                                    } else {
                                        o[qd][0] *= mask_factor(zv.x); o[qd][1] *= mask_factor(zv.y); o[qd][2] *= mask_factor(zv.z); o[qd][3] *= mask_factor(zv.w);
                                    }
                                }
                                if (inside) st4(reinterpret_cast<float*>(dst) + off + a * 32 + qd * 8 + hi * 4, o[qd]);
                            }
                        } else {
                            unsigned sign_bytes = 0u;
#pragma unroll
                            for (int qp = 0; qp < 2; ++qp) {
                                float lo[4], hi4[4];
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[2 * qp][e]), __float_as_uint(o[2 * qp + 1][e]), false, false);
                                    lo[e] = __uint_as_float(r[0]);
                                    hi4[e] = __uint_as_float(r[1]);
                                }
                                if (BITS && mkind) {   // 1-bit mask: this lane's byte of the pixel's dword
                                    const unsigned byte = mz[0].x >> (8 * (2 * hi + qp));
#define GS_BR(V, K) V = (byte >> (K)) & 1u ? V : 0.2f * V
                                    GS_BR(lo[0], 0); GS_BR(lo[1], 1); GS_BR(lo[2], 2); GS_BR(lo[3], 3);
                                    GS_BR(hi4[0], 4); GS_BR(hi4[1], 5); GS_BR(hi4[2], 6); GS_BR(hi4[3], 7);
#undef GS_BR
                                } else if (!BITS && mkind) {   // the lane's 8 channels of the mask sit where its 16 bytes go
                                    const uint4 zv = mz[qp];
                                    if (p.mask_act == GS_ACT_LRELU) {
                                        // z > 0 on the packed pair: low half shifted up and compared as an integer, high half in place (>= 0x10000: sign
                                        // clear, magnitude bits not all zero); compare, scale, select per value
#define GS_LR(V, Z) V = (int)((Z) << 16) > 0 ? V : 0.2f * V
#define GS_HR(V, Z) V = (int)(Z) >= 0x10000 ? V : 0.2f * V
                                        GS_LR(lo[0], zv.x); GS_HR(lo[1], zv.x); GS_LR(lo[2], zv.y); GS_HR(lo[3], zv.y);
                                        GS_LR(hi4[0], zv.z); GS_HR(hi4[1], zv.z); GS_LR(hi4[2], zv.w); GS_HR(hi4[3], zv.w);
#undef GS_LR
#undef GS_HR
                                    } else {
                                        lo[0] *= mask_factor(__uint_as_float(zv.x << 16)); lo[1] *= mask_factor(__uint_as_float(zv.x & 0xffff0000u));
                                        lo[2] *= mask_factor(__uint_as_float(zv.y << 16)); lo[3] *= mask_factor(__uint_as_float(zv.y & 0xffff0000u));
                                        hi4[0] *= mask_factor(__uint_as_float(zv.z << 16)); hi4[1] *= mask_factor(__uint_as_float(zv.z & 0xffff0000u));
                                        hi4[2] *= mask_factor(__uint_as_float(zv.w << 16)); hi4[3] *= mask_factor(__uint_as_float(zv.w & 0xffff0000u));
                                    }
                                }
                                uint4 v;
                                v.x = pack_bf16x2(lo[0], lo[1]); v.y = pack_bf16x2(lo[2], lo[3]);
                                v.z = pack_bf16x2(hi4[0], hi4[1]); v.w = pack_bf16x2(hi4[2], hi4[3]);
                                if (inside) *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(dst) + off + a * 32 + qp * 16 + hi * 8) = v;
                                if (BITS && emit) {   // sign bits of the STORED values (z > 0 exactly as the masked epilogues test it on the bf16 pair)
                                    const unsigned b8 = ((int)(v.x << 16) > 0 ? 1u : 0u) | ((int)v.x >= 0x10000 ? 2u : 0u) | ((int)(v.y << 16) > 0 ? 4u : 0u) |
                                                        ((int)v.y >= 0x10000 ? 8u : 0u) | ((int)(v.z << 16) > 0 ? 16u : 0u) | ((int)v.z >= 0x10000 ? 32u : 0u) |
                                                        ((int)(v.w << 16) > 0 ? 64u : 0u) | ((int)v.w >= 0x10000 ? 128u : 0u);
                                    sign_bytes |= b8 << (8 * qp);
                                }
                            }
                            if (BITS && emit && inside)   // the lane's two bytes of the pixel's dword: bytes 2 hi, 2 hi + 1
                                *reinterpret_cast<unsigned short*>(p.bits_out + ((off + a * 32) >> 3) + 2 * hi) = (unsigned short)sign_bytes;
                        }
                    };
                    // all mask vectors of the tile in one go when they fit in 32 registers, else one (pixel group, phase) at a time
                    constexpr bool MASK_ALL = !NORM && (BITS || B * NPH * A * NV <= 8);   // (sign words: one register per (pixel, tile), always ahead)
                    mvec_t mz_all[MASK_ALL ? B * NPH : 1][A][NV];
                    if constexpr (BITS) {
#pragma unroll
                        for (int i = 0; i < B * NPH; ++i)
#pragma unroll
                            for (int a = 0; a < A; ++a) mz_all[i][a][0].x = mbw[i][a];
                    } else if constexpr (MASK_ALL) {
                        if (p.mask) {
#pragma unroll
                            for (int b = 0; b < B; ++b) {
                                const int q = (wv * B + b) * 32 + l31;
                                const int gy = by + q / TW, gx = bx + q % TW;
#pragma unroll
                                for (int ph = 0; ph < NPH; ++ph) {
                                    const int oy = MODE == MODE_T2 ? 2 * gy + (ph >> 1) : gy;
                                    const int ox = MODE == MODE_T2 ? 2 * gx + (ph & 1) : gx;
                                    mask_fetch((((long)n * Ho + oy) * Wo + ox) * OC + oc0, gy < Hb && gx < Wb, mz_all[b * NPH + ph]);
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int b = 0; b < B; ++b) {
                        const int q = (wv * B + b) * 32 + l31;
                        const int gy = by + q / TW, gx = bx + q % TW;
#ifdef GS_ABL_NOSTORE
                        const bool inside = gy < -1000;
#else
                        const bool inside = gy < Hb && gx < Wb;
#endif
#pragma unroll
                        for (int ph = 0; ph < NPH; ++ph) {
                            const int oy = MODE == MODE_T2 ? 2 * gy + (ph >> 1) : gy;
                            const int ox = MODE == MODE_T2 ? 2 * gx + (ph & 1) : gx;
                            const long off = (((long)n * Ho + oy) * Wo + ox) * OC + oc0;
                            if constexpr (NORM == 2) {
                                // the block owns every channel of the pixel (OC == 32 A) and the accumulators are g = d L / d pixel_norm(z): finish
                                // the previous block's backward here.  With r = rsqrt(mean z^2 + eps): gx = r (g - z r^2 mean(z g)), then + addend
                                // and times act'(z).  Values are brought to the STORE layout first (bf16: the lane-half swap), where the lane's
                                // 16 channels per 32-channel tile sit exactly like the 16-byte vectors of z / addend it fetches.
                                constexpr int EV = 16 / NV;                    // values per 16-byte vector: 4 (fp32) or 8 (bf16)
                                const int cur = NPIPE ? ((b * NPH + ph) & 1) : 0;
                                if constexpr (NPIPE) {   // (this step's vectors are on their way since the last stage / the previous step: fetch the next one's)
                                    if (b * NPH + ph + 1 < B * NPH) norm_fetch(b * NPH + ph + 1, nz[(b * NPH + ph + 1) & 1], nx[(b * NPH + ph + 1) & 1]);
                                } else {
                                    mask_fetch(off, inside, nz[0]);
                                    if (p.addend) {
                                        const long base = inside ? off : 0;
#pragma unroll
                                        for (int a = 0; a < A; ++a)
#pragma unroll
                                            for (int v = 0; v < NV; ++v)
                                                nx[0][a][v] = *reinterpret_cast<const mvec_t*>(reinterpret_cast<const T*>(p.addend) + base + a * 32 + v * (32 / NV) + hi * (16 / NV));
                                    }
                                }
                                mvec_t (&zq)[A][NV] = nz[cur];
                                mvec_t (&aq)[A][NV] = nx[cur];
                                float gv[A][NV][EV], zv[A][NV][EV];
                                float ssq = 0.f, szg = 0.f;
#pragma unroll
                                for (int a = 0; a < A; ++a) {
                                    float o[4][4];
                                    finish(ph, a, b, o);   // (no bias, no activation on a data gradient: alpha * acc)
                                    if constexpr (SZ == 4) {
#pragma unroll
                                        for (int qd = 0; qd < 4; ++qd) {
                                            const float4 z4 = zq[a][qd];
                                            const float zz[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
                                            for (int e = 0; e < 4; ++e) { gv[a][qd][e] = o[qd][e]; zv[a][qd][e] = zz[e]; }
                                        }
                                    } else {
#pragma unroll
                                        for (int qp = 0; qp < 2; ++qp) {
#pragma unroll
                                            for (int e = 0; e < 4; ++e) {
                                                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[2 * qp][e]), __float_as_uint(o[2 * qp + 1][e]), false, false);
                                                gv[a][qp][e] = __uint_as_float(r[0]);
                                                gv[a][qp][4 + e] = __uint_as_float(r[1]);
                                            }
                                            const uint4 z4 = zq[a][qp];
                                            const unsigned zw[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
                                            for (int e = 0; e < 4; ++e) { zv[a][qp][2 * e] = __uint_as_float(zw[e] << 16); zv[a][qp][2 * e + 1] = __uint_as_float(zw[e] & 0xffff0000u); }
                                        }
                                    }
#pragma unroll
                                    for (int v = 0; v < NV; ++v)
#pragma unroll
                                        for (int e = 0; e < EV; ++e) { ssq += zv[a][v][e] * zv[a][v][e]; szg += zv[a][v][e] * gv[a][v][e]; }
                                }
                                ssq = swap32_sum(ssq);   // the partner lane of the other half holds the pixel's other channels
                                szg = swap32_sum(szg);
                                const float inv_c = 1.f / (float)(32 * A);
                                const float r = rsqrtf(ssq * inv_c + p.pn_eps);
                                const float m = szg * inv_c * r * r;
#pragma unroll
                                for (int a = 0; a < A; ++a)
#pragma unroll
                                    for (int v = 0; v < NV; ++v) {
                                        float out[EV], ad[EV];
#pragma unroll
                                        for (int e = 0; e < EV; ++e) ad[e] = 0.f;
                                        if (p.addend) {
                                            if constexpr (SZ == 4) {
                                                const float4 a4 = aq[a][v];
                                                ad[0] = a4.x; ad[1] = a4.y; ad[2] = a4.z; ad[3] = a4.w;
                                            } else {
                                                const uint4 a4 = aq[a][v];
                                                const unsigned aw[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                                                for (int e = 0; e < 4; ++e) { ad[2 * e] = __uint_as_float(aw[e] << 16); ad[2 * e + 1] = __uint_as_float(aw[e] & 0xffff0000u); }
                                            }
                                        }
#pragma unroll
                                        for (int e = 0; e < EV; ++e) out[e] = (r * (gv[a][v][e] - zv[a][v][e] * m) + ad[e]) * mask_factor(zv[a][v][e]);
                                        if (inside) {
                                            if constexpr (SZ == 4) {
                                                st4(reinterpret_cast<float*>(y) + off + a * 32 + v * 8 + hi * 4, out);
                                            } else {
                                                uint4 w4;
                                                w4.x = pack_bf16x2(out[0], out[1]); w4.y = pack_bf16x2(out[2], out[3]);
                                                w4.z = pack_bf16x2(out[4], out[5]); w4.w = pack_bf16x2(out[6], out[7]);
                                                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(y) + off + a * 32 + v * 16 + hi * 8) = w4;
                                            }
                                        }
                                    }
                            } else if constexpr (NORM == 3) {
                                // accumulators t = gradient w.r.t. u = M J(z) g (M = act'(z), J the norm's Jacobian).  h = M t;
                                //   y  = J h                                   = r (h - z r^2 mean(h z))
                                //   y2 = d<h, J g>/dz = -r^3 (mean(h g) z + mean(z g) h + mean(h z) g) + 3 r^5 mean(h z) mean(z g) z
                                constexpr int EV = 16 / NV;
                                const int cur = NPIPE ? ((b * NPH + ph) & 1) : 0;
                                if constexpr (NPIPE) {
                                    if (b * NPH + ph + 1 < B * NPH) norm_fetch(b * NPH + ph + 1, nz[(b * NPH + ph + 1) & 1], nx[(b * NPH + ph + 1) & 1]);
                                } else {
                                    mask_fetch(off, inside, nz[0]);
                                    const long base = inside ? off : 0;
#pragma unroll
                                    for (int a = 0; a < A; ++a)
#pragma unroll
                                        for (int v = 0; v < NV; ++v)
                                            nx[0][a][v] = *reinterpret_cast<const mvec_t*>(reinterpret_cast<const T*>(p.addend) + base + a * 32 + v * (32 / NV) + hi * (16 / NV));
                                }
                                mvec_t (&zq)[A][NV] = nz[cur];
                                mvec_t (&gq)[A][NV] = nx[cur];
                                float hv[A][NV][EV], zv[A][NV][EV], gv[A][NV][EV];
                                float ssq = 0.f, shg = 0.f, shz = 0.f, szg = 0.f;
#pragma unroll
                                for (int a = 0; a < A; ++a) {
                                    float o[4][4];
                                    finish(ph, a, b, o);   // (alpha * acc: no bias, no activation)
                                    if constexpr (SZ == 4) {
#pragma unroll
                                        for (int qd = 0; qd < 4; ++qd) {
                                            const float4 z4 = zq[a][qd], g4 = gq[a][qd];
                                            const float zz[4] = {z4.x, z4.y, z4.z, z4.w}, g_[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                                            for (int e = 0; e < 4; ++e) { hv[a][qd][e] = o[qd][e]; zv[a][qd][e] = zz[e]; gv[a][qd][e] = g_[e]; }
                                        }
                                    } else {
#pragma unroll
                                        for (int qp = 0; qp < 2; ++qp) {
#pragma unroll
                                            for (int e = 0; e < 4; ++e) {
                                                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[2 * qp][e]), __float_as_uint(o[2 * qp + 1][e]), false, false);
                                                hv[a][qp][e] = __uint_as_float(r[0]);
                                                hv[a][qp][4 + e] = __uint_as_float(r[1]);
                                            }
                                            const uint4 z4 = zq[a][qp], g4 = gq[a][qp];
                                            const unsigned zw[4] = {z4.x, z4.y, z4.z, z4.w}, gw_[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                                            for (int e = 0; e < 4; ++e) {
                                                zv[a][qp][2 * e] = __uint_as_float(zw[e] << 16); zv[a][qp][2 * e + 1] = __uint_as_float(zw[e] & 0xffff0000u);
                                                gv[a][qp][2 * e] = __uint_as_float(gw_[e] << 16); gv[a][qp][2 * e + 1] = __uint_as_float(gw_[e] & 0xffff0000u);
                                            }
                                        }
                                    }
#pragma unroll
                                    for (int v = 0; v < NV; ++v)
#pragma unroll
                                        for (int e = 0; e < EV; ++e) {
                                            const float zc = zv[a][v][e], gc = gv[a][v][e];
                                            const float hc = hv[a][v][e] * mask_factor(zc);
                                            hv[a][v][e] = hc;
                                            ssq += zc * zc; shg += hc * gc; shz += hc * zc; szg += zc * gc;
                                        }
                                }
                                ssq = swap32_sum(ssq); shg = swap32_sum(shg);
                                shz = swap32_sum(shz); szg = swap32_sum(szg);
                                const float inv_c = 1.f / (float)(32 * A);
                                const float r = rsqrtf(ssq * inv_c + p.pn_eps);
                                const float r2 = r * r, r3 = r2 * r;
                                const float ma = shg * inv_c, mb = shz * inv_c, mm = szg * inv_c;
                                const float kz = 3.f * r3 * r2 * mb * mm - r3 * ma;   // coefficient of z in y2
#pragma unroll
                                for (int a = 0; a < A; ++a)
#pragma unroll
                                    for (int v = 0; v < NV; ++v) {
                                        float o1[EV], o2[EV];
#pragma unroll
                                        for (int e = 0; e < EV; ++e) {
                                            const float zc = zv[a][v][e], gc = gv[a][v][e], hc = hv[a][v][e];
                                            o1[e] = r * (hc - zc * r2 * mb);
                                            o2[e] = kz * zc - r3 * (mm * hc + mb * gc);
                                        }
                                        if (inside) {
                                            if constexpr (SZ == 4) {
                                                st4(reinterpret_cast<float*>(y) + off + a * 32 + v * 8 + hi * 4, o1);
                                                st4(reinterpret_cast<float*>(p.y2) + off + a * 32 + v * 8 + hi * 4, o2);
                                            } else {
                                                uint4 w4;
                                                w4.x = pack_bf16x2(o1[0], o1[1]); w4.y = pack_bf16x2(o1[2], o1[3]); w4.z = pack_bf16x2(o1[4], o1[5]); w4.w = pack_bf16x2(o1[6], o1[7]);
                                                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(y) + off + a * 32 + v * 16 + hi * 8) = w4;
                                                w4.x = pack_bf16x2(o2[0], o2[1]); w4.y = pack_bf16x2(o2[2], o2[3]); w4.z = pack_bf16x2(o2[4], o2[5]); w4.w = pack_bf16x2(o2[6], o2[7]);
                                                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p.y2) + off + a * 32 + v * 16 + hi * 8) = w4;
                                            }
                                        }
                                    }
                            } else if constexpr (NORM == 1) {
                                // the block owns every channel of the pixel (OC == 32 A): pixel norm in the same pass.  The lane and its
                                // partner in the other half hold the pixel's channels between them.
                                float o[A][4][4], ssq = 0.f;
#pragma unroll
                                for (int a = 0; a < A; ++a) {
                                    finish(ph, a, b, o[a]);
#pragma unroll
                                    for (int k = 0; k < 16; ++k) ssq += o[a][k >> 2][k & 3] * o[a][k >> 2][k & 3];
                                }
                                ssq = swap32_sum(ssq);
                                const float r = rsqrtf(ssq * (1.f / (float)(32 * A)) + p.pn_eps);
#pragma unroll
                                for (int a = 0; a < A; ++a) {
                                    if (y) {   // the pre-norm activation, kept for the backward
                                        float oz[4][4];
#pragma unroll
                                        for (int k = 0; k < 16; ++k) oz[k >> 2][k & 3] = o[a][k >> 2][k & 3];
                                        store(y, off, a, oz, inside, static_cast<const mvec_t*>(nullptr));
                                    }
#pragma unroll
                                    for (int k = 0; k < 16; ++k) o[a][k >> 2][k & 3] *= r;
                                    store(reinterpret_cast<T*>(p.y2), off, a, o[a], inside, static_cast<const mvec_t*>(nullptr));
                                }
                            } else {
                                mvec_t mz_one[A][NV];
                                if constexpr (!MASK_ALL) {
                                    if (p.mask) mask_fetch(off, inside, mz_one);
                                }
#pragma unroll
                                for (int a = 0; a < A; ++a) {
                                    float o[4][4];
                                    finish(ph, a, b, o);
                                    const mvec_t* mz = MASK_ALL ? mz_all[MASK_ALL ? b * NPH + ph : 0][a] : mz_one[a];
                                    store(y, off, a, o, inside, mz, p.mask ? (use_mb ? 2 : 1) : 0, emit_bits);
                                }
                            }
                        }
                    }
                    zero_acc();
                }
#endif
                block_barrier();
#ifdef GS_IGEMM_TRACE
                GS_TR(4 + tr_stage);
                ++tr_stage;
#endif
                if (tg == NTG - 1) c_pb = c_pb + 1 == NPB ? 0 : c_pb + 1;
                if (!RESIDENT) c_wb = c_wb + 1 == NWB ? 0 : c_wb + 1;
            }
        }
        if (++done >= count) break;
        item += stride;
    }
    GS_TR(63);
    wait_vmcnt(0);  // the (empty) stages issued past the end must have retired before this block's LDS is handed on
}

// ------------------------------------------------------------------------------ dispatch

#ifndef GS_MAX_BLOCKS_PER_CU
#define GS_MAX_BLOCKS_PER_CU 2
#endif
#ifndef GS_SMALL_D
#define GS_SMALL_D 2   // stages in flight for the few-block ("small") configurations
#endif
template <typename T, int MODE, int A, int B, int TW, int TG, bool RESIDENT = false, int D = 2, int NORM = 0, int RB = 64, bool SPEC = false, bool BITS = false>
static int launch_igemm(ConvP p, hipStream_t st) {
    if constexpr (!BITS && sizeof(T) == 2 && NORM == 0) {
        if (p.mask_bits || p.bits_out) return launch_igemm<T, MODE, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC, true>(p, st);
    }
    constexpr int NP = 128 * B;
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int OCT = 32 * A;
    constexpr int BK = RB / (int)sizeof(T);
    constexpr int NTG = 9 / TG;
    constexpr int PBUF = ((PH * PW * (RB / 16) + 255) / 256) * 4096;
    constexpr int WBUF = ((TG * OCT * RB + 4095) / 4096) * 4096;
    constexpr int NPB = 1 + (D + NTG - 1) / NTG, NWB = D + 1;
    p.tiles_x = cdiv(p.Wb, TW);
    p.tiles_y = cdiv(p.Hb, TH);
    p.nsp = p.N * p.tiles_x * p.tiles_y;
    p.noct = cdiv(p.OC, OCT);
    p.nch = p.IC / BK;
    {   // reciprocals for the kernel's item decoding (see ConvP): exact while items < 2^21 and divisors < 2^11
        auto magic = [](int d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); };
        if (p.noct >= 2048 || p.tiles_x >= 2048 || p.tiles_y >= 2048)
            return fail(GS_ERR_UNSUPPORTED, "conv igemm: %d channel tiles / %d x %d spatial tiles exceed the item decoder's range", p.noct, p.tiles_x, p.tiles_y);
        static const long max_items = getenv("GS_IGEMM_MAX_ITEMS") ? atol(getenv("GS_IGEMM_MAX_ITEMS")) : (1L << 21);   // (tests lower it)
        if ((long)p.nsp * p.noct >= max_items) {
            // More work items than the reciprocal decoder is exact for (large-batch evaluation at full resolution): images are independent,
            // so the batch runs as several launches of as many images as fit the range -- same kernel, same results.
            const long per_image = (long)p.tiles_x * p.tiles_y * p.noct;
            const int chunk = (int)((max_items - 1) / per_image);
            if (chunk < 1) return fail(GS_ERR_UNSUPPORTED, "conv igemm: %ld work items per image exceed the item decoder's range", per_image);
            const size_t in_img = (size_t)p.Hi * p.Wi * p.IC * sizeof(T);
            const size_t out_img = (size_t)p.Hb * p.Wb * (MODE == MODE_T2 ? 4 : 1) * p.OC * sizeof(T);
            auto adv = [](const void* q, size_t b) -> const void* { return q ? (const char*)q + b : nullptr; };
            for (int n0 = 0; n0 < p.N; n0 += chunk) {
                ConvP q = p;
                q.N = p.N - n0 < chunk ? p.N - n0 : chunk;
                q.x = adv(p.x, n0 * in_img);
                q.y = const_cast<void*>(adv(p.y, n0 * out_img));
                q.y2 = const_cast<void*>(adv(p.y2, n0 * out_img));
                q.mask = adv(p.mask, n0 * out_img);
                q.mask_bits = reinterpret_cast<const unsigned char*>(adv(p.mask_bits, n0 * out_img / (8 * sizeof(T))));
                q.bits_out = reinterpret_cast<unsigned char*>(const_cast<void*>(adv(p.bits_out, n0 * out_img / (8 * sizeof(T)))));
                q.addend = adv(p.addend, n0 * out_img);
                int pending = 0;
                if (p.norm_pending) q.norm_pending = &pending;
                if (int e = launch_igemm<T, MODE, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC, BITS>(q, st)) return e;
                if (p.norm_pending && pending) *p.norm_pending = pending;
            }
            return 0;
        }
        p.m_noct = magic(p.noct); p.m_tx = magic(p.tiles_x); p.m_ty = magic(p.tiles_y);
    }
    const int wbufs = RESIDENT ? p.nch : NWB;
    const size_t lds = (size_t)NPB * PBUF + (size_t)wbufs * WBUF + (size_t)((p.OC + 3) / 4) * 16 + 0;
    if (p.OC % OCT != 0) return fail(GS_ERR_UNSUPPORTED, "conv igemm: %d output channels with %d-wide tiles", p.OC, OCT);
    if ((size_t)p.Hi * p.Wi * p.IC * sizeof(T) >= (1ull << 31)) return fail(GS_ERR_UNSUPPORTED, "conv igemm: one image exceeds 2 GiB");
    if (lds > 160 * 1024) return fail(GS_ERR_UNSUPPORTED, "conv igemm: %zu bytes of LDS needed", lds);
    if (NORM && p.OC != OCT) return fail(GS_ERR_UNSUPPORTED, "conv igemm: fused pixel norm needs the whole channel range in one tile");
    if ((NORM == 2 || NORM == 3) && p.OC != OCT) return fail(GS_ERR_UNSUPPORTED, "conv igemm: fused pixel-norm backward needs the whole channel range in one tile");
    if (!((NORM == 2 && p.normbwd == 1) || (NORM == 3 && p.normbwd == 2)) && p.normbwd) {
        // no fused form here: plain conv, the caller runs the norm's backward kernel(s) as their own pass
        if (p.norm_pending) *p.norm_pending = 1 + p.normbwd;   // 2: first-order form, 3: second-order form
        p.normbwd = 0;
        p.mask = nullptr;
        p.addend = nullptr;
        p.y2 = nullptr;
    }
    if (NORM != 1 && NORM != 3 && p.y2) {   // the norm stays a separate pass: this launch leaves the activation where that pass will read it
        if (!p.y) p.y = p.y2;
        p.y2 = nullptr;
        if (p.norm_pending) *p.norm_pending = 1;
    }
    if (p.IC % BK != 0) return fail(GS_ERR_UNSUPPORTED, "conv igemm: %d input channels with %d-channel chunks", p.IC, BK);
    auto kern = conv_igemm_kernel<T, MODE, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC, BITS>;
    static size_t max_set = 0;  // per template instantiation
    if (lds > max_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(GS_ERR_HIP, "conv igemm: cannot reserve %zu bytes of dynamic LDS", lds);
        max_set = lds;
    }
    // resident blocks per CU: LDS-limited, and at most 2 (accumulator-heavy kernels hold 1-2 waves per SIMD)
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > GS_MAX_BLOCKS_PER_CU) per_cu = GS_MAX_BLOCKS_PER_CU;
    if (per_cu < 1 || SPEC) per_cu = 1;   // (8 waves of up to 256 VGPRs: one block per CU)
    const long total = (long)p.nsp * p.noct;
    long grid = (long)per_cu * num_cus();
    if (grid > total) grid = total;
    if (grid >= 8) grid &= ~7L;
    const double flops = 2.0 * 9.0 * (double)p.N * p.Hb * p.Wb * p.IC * p.OC;
    const double out_px = (double)p.N * p.Hb * p.Wb * (MODE == MODE_T2 ? 4 : 1);
    // algorithmic bytes: input + output + weights, + the activation mask a masked launch reads (1/16 of it as sign words), + the sign words a
    // forward launch writes, + the second output of a fused norm
    const double bytes = ((double)p.N * p.Hi * p.Wi * p.IC + out_px * p.OC * (1.0 + (p.mask ? (p.mask_bits ? 1.0 / 16.0 : 1.0) : 0.0) + (p.bits_out ? 1.0 / 16.0 : 0.0) + ((NORM == 1 && p.y) ? 1.0 : 0.0) + ((NORM == 2 && p.addend) ? 1.0 : 0.0) + (NORM == 3 ? 2.0 : 0.0)) + 9.0 * p.IC * p.OC) * sizeof(T);
    const int reps = prof_reps();   // (1 unless profiling in burst mode: the kernel is a pure function of its inputs)
    ProfScope ps(st, flops, bytes, MODE, p.N, p.Hb, p.Wb, p.IC, p.OC, p.mask ? 1 : 0, NORM ? 1 : 0, reps);
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(SPEC ? 512 : 256), lds, st, p);
    return 0;
}

// ---- which configuration: one value, one chooser, one table of instantiations
// The template arguments of conv_igemm_kernel a launch runs with, bar T and MODE (the caller's) and BITS (launch_igemm reads it off ConvP).
struct IgemmCfg {
    int A, B, TW, TG;                         // 32 A channels x 128 B pixels per tile, TW pixels wide; TG taps per stage
    bool RESIDENT = false;                    // the layer's whole weight slab stays in LDS
    int D = 2, NORM = IGEMM_PLAIN, RB = 64;   // stages in flight; the epilogue (IGEMM_*); bytes per operand row
    bool SPEC = false;                        // wave-specialised 8-wave block
    bool operator==(const IgemmCfg& o) const {
        return A == o.A && B == o.B && TW == o.TW && TG == o.TG && RESIDENT == o.RESIDENT && D == o.D && NORM == o.NORM && RB == o.RB && SPEC == o.SPEC;
    }
};
// Measurement knobs of the chooser, read from the environment once.  GS_SPEC: 1 (default) runs the few-block bf16 layers wave-specialised,
// 0 does not -- per iteration of configs[1] (scripts/run_spec.sh) those layers go 1086 -> 1068 us.  (Its former bits 1 and 2, the same for the
// larger S1 / S2 / T2 tiles, lost 60-190 us -- stages bound by the fragment reads and the barrier, not by the DMA issue -- and are retired:
// DESIGN.md, "Measured and rejected in round 3".)
struct IgemmKnobs { bool no_small_tiles, no_rb128, spec; };
static IgemmKnobs igemm_knobs() {
    static const IgemmKnobs k = {getenv("GS_NO_SMALL_TILES") != nullptr, getenv("GS_NO_RB128") != nullptr,
                                 getenv("GS_SPEC") ? (atoi(getenv("GS_SPEC")) & 1) != 0 : true};
    return k;
}

// The configuration a layer runs with: (mode, dtype, kernel-role shape, wanted epilogue) -> IgemmCfg.  Pure host arithmetic -- `cus` and the
// knobs arrive as arguments.  Where the wanted fused norm form has no epilogue for the shape the answer is the plain configuration (NORM ==
// IGEMM_PLAIN) and the caller runs the norm as its own pass: the forms exist only where a tile owns every channel of a pixel (OC = 32 A) and
// that the generator's 32- / 64-channel blocks actually use.
static IgemmCfg choose_igemm(int mode, int dtype, int N, int Hb, int Wb, int IC, int OC, int want, long cus, IgemmKnobs knobs) {
    constexpr int FWD = 1 << IGEMM_NORM_FWD, BWD = 1 << IGEMM_NORM_BWD, BWD2 = 1 << IGEMM_NORM_BWD2;
    auto epi = [&](int forms) { return (forms >> want) & 1 ? want : IGEMM_PLAIN; };   // `want` if the configuration has that epilogue
    const int nch = IC / (dtype == GS_F32 ? 16 : 32);   // 64-byte channel chunks
    const bool a2 = OC % 64 == 0;
    const int tw = Wb >= 32 ? 32 : 16;
    // blocks the layer gives with 128*B-pixel x 64-channel tiles (TW = 32)
    auto items64 = [&](int B_) { return (long)N * cdiv(Hb, 4 * B_) * cdiv(Wb, 32) * (OC / 64); };
    // Measured on the layers of the fully grown networks (scripts/probe/run_variants.sh): two resident blocks per CU (<= 80 KiB
    // of LDS each, i.e. a one-stage-deep ring) beat one block with a deeper ring or a larger tile wherever the layer has at
    // least two blocks per CU to give -- the epilogue and DMA waits of one block run under the MFMAs of the other.
    const bool small = !knobs.no_small_tiles && items64(1) <= cus;   // no more blocks than CUs: a serial chain of stages per block
    // 128-byte operand rows (whole cache lines per DMA row, half the stages), bf16 only
    const bool rb128 = dtype == GS_BF16 && !knobs.no_rb128 && IC % 64 == 0;
    if (mode == MODE_S2) {
        if (small) return {1, 1, tw, 9, false, 1};
        if (!a2) return {1, 1, 32, 3};
        // stride 2: the patch is 4.6x the output tile, so a 128-channel tile (the patch staged once for all of them) is worth
        // more than a second pixel tile as long as every CU still gets a block
        if (OC == 64 && nch == 1 && Wb >= 32 && items64(1) >= cus) return {2, 1, 32, 9, true, 1, epi(BWD)};   // 36 KiB of weights: resident
        if (OC % 128 == 0 && Wb >= 32 && (long)N * cdiv(Hb, 4) * cdiv(Wb, 32) * (OC / 128) >= cus) return {4, 1, 32, 3};
        return {2, 1, tw, 3};
    }
    const bool s1 = mode == MODE_S1;   // (else MODE_T2: four output pixels per base pixel, so half the base pixels per tile)
    if (OC == 32 && nch <= 2 && Wb >= 64) return {1, s1 ? 2 : 1, 64, 9, true, 1, epi(s1 ? FWD | BWD | BWD2 : FWD | BWD2)};
    // few blocks, each a serial chain of stages: 32-channel tiles double the number of busy CUs, 9-tap stages cut the
    // barriers and DMA round trips of the chain to a third
    if (small) {
        // 128-byte rows: the few-block layers are bound by the L2 -> LDS rate of a CU, not by its MFMAs
        if (rb128) return {1, 1, tw, 9, false, 1, IGEMM_PLAIN, 128, knobs.spec};
        return {1, 1, tw, 9, false, GS_SMALL_D};
    }
    if (!a2) return {1, 1, s1 ? 32 : tw, 3};
    if (!s1) return {2, 1, tw, 3, false, 2, Wb >= 32 && OC == 64 ? epi(FWD | BWD2) : IGEMM_PLAIN};
    if (Wb >= 32 && items64(2) >= 2 * cus) return {2, 2, 32, 3, false, 1, OC == 64 ? epi(FWD | BWD | BWD2) : IGEMM_PLAIN};
    if (OC == 64 && nch <= 2 && Wb >= 32 && items64(2) >= cus / 2) return {2, 2, 32, 9, true};   // 9 taps x 64 x (<= 64 channels) <= 72 KiB stay in LDS
    // every block re-streams its 64 x IC x 9 weight slab from L2: the more pixels a block owns the smaller that
    // stream is per MFMA -- take the largest pixel tile that still gives every CU a block
    if (Wb >= 32 && items64(2) >= cus) {
        // one block per CU: 128-byte rows halve the stages of the chain (22.0 -> 20.1 us on 256 -> 256 @ 16x128 x8, scripts/run_abl.sh)
        if (rb128) return {2, 2, 32, 3, false, 1, IGEMM_PLAIN, 128};
        return {2, 2, 32, 3};
    }
    return {2, 1, tw, 3};
}

// Every (MODE, configuration) that is compiled, once: X(MODE, BF16_ONLY, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC).  A configuration the
// chooser can return has a row here (tests/test_igemm_config_cpu.py sweeps it); BF16_ONLY rows are the ones only bf16 reaches.
#define GS_APPLY(X, ...) X(__VA_ARGS__)
#ifdef GS_FORCE_CFG   // probes only: -DGS_FORCE_MODE=0 -DGS_FORCE_CFG=2,2,32,3,false,1,0,64,false -- all nine fields of one IgemmCfg, which every
                      // bf16 launch of that mode then runs with (scripts/probe/build_variants.sh)
#define GS_IGEMM_FORCED(X) GS_APPLY(X, GS_FORCE_MODE, true, GS_FORCE_CFG)
#else
#define GS_IGEMM_FORCED(X)
#endif
#define GS_IGEMM_CONFIGS(X)                                                     \
    X(MODE_S1, false, 1, 2, 64, 9, true, 1, IGEMM_PLAIN, 64, false)             \
    X(MODE_S1, false, 1, 2, 64, 9, true, 1, IGEMM_NORM_FWD, 64, false)          \
    X(MODE_S1, false, 1, 2, 64, 9, true, 1, IGEMM_NORM_BWD, 64, false)          \
    X(MODE_S1, false, 1, 2, 64, 9, true, 1, IGEMM_NORM_BWD2, 64, false)         \
    X(MODE_S1, true, 1, 1, 32, 9, false, 1, IGEMM_PLAIN, 128, true)             \
    X(MODE_S1, true, 1, 1, 16, 9, false, 1, IGEMM_PLAIN, 128, true)             \
    X(MODE_S1, true, 1, 1, 32, 9, false, 1, IGEMM_PLAIN, 128, false)            \
    X(MODE_S1, true, 1, 1, 16, 9, false, 1, IGEMM_PLAIN, 128, false)            \
    X(MODE_S1, false, 1, 1, 32, 9, false, GS_SMALL_D, IGEMM_PLAIN, 64, false)   \
    X(MODE_S1, false, 1, 1, 16, 9, false, GS_SMALL_D, IGEMM_PLAIN, 64, false)   \
    X(MODE_S1, false, 1, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S1, false, 2, 2, 32, 3, false, 1, IGEMM_PLAIN, 64, false)            \
    X(MODE_S1, false, 2, 2, 32, 3, false, 1, IGEMM_NORM_FWD, 64, false)         \
    X(MODE_S1, false, 2, 2, 32, 3, false, 1, IGEMM_NORM_BWD, 64, false)         \
    X(MODE_S1, false, 2, 2, 32, 3, false, 1, IGEMM_NORM_BWD2, 64, false)        \
    X(MODE_S1, false, 2, 2, 32, 9, true, 2, IGEMM_PLAIN, 64, false)             \
    X(MODE_S1, true, 2, 2, 32, 3, false, 1, IGEMM_PLAIN, 128, false)            \
    X(MODE_S1, false, 2, 2, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S1, false, 2, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S1, false, 2, 1, 16, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S2, false, 1, 1, 32, 9, false, 1, IGEMM_PLAIN, 64, false)            \
    X(MODE_S2, false, 1, 1, 16, 9, false, 1, IGEMM_PLAIN, 64, false)            \
    X(MODE_S2, false, 1, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S2, false, 2, 1, 32, 9, true, 1, IGEMM_PLAIN, 64, false)             \
    X(MODE_S2, false, 2, 1, 32, 9, true, 1, IGEMM_NORM_BWD, 64, false)          \
    X(MODE_S2, false, 4, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S2, false, 2, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_S2, false, 2, 1, 16, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_T2, false, 1, 1, 64, 9, true, 1, IGEMM_PLAIN, 64, false)             \
    X(MODE_T2, false, 1, 1, 64, 9, true, 1, IGEMM_NORM_FWD, 64, false)          \
    X(MODE_T2, false, 1, 1, 64, 9, true, 1, IGEMM_NORM_BWD2, 64, false)         \
    X(MODE_T2, true, 1, 1, 32, 9, false, 1, IGEMM_PLAIN, 128, true)             \
    X(MODE_T2, true, 1, 1, 16, 9, false, 1, IGEMM_PLAIN, 128, true)             \
    X(MODE_T2, true, 1, 1, 32, 9, false, 1, IGEMM_PLAIN, 128, false)            \
    X(MODE_T2, true, 1, 1, 16, 9, false, 1, IGEMM_PLAIN, 128, false)            \
    X(MODE_T2, false, 1, 1, 32, 9, false, GS_SMALL_D, IGEMM_PLAIN, 64, false)   \
    X(MODE_T2, false, 1, 1, 16, 9, false, GS_SMALL_D, IGEMM_PLAIN, 64, false)   \
    X(MODE_T2, false, 1, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_T2, false, 1, 1, 16, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_T2, false, 2, 1, 32, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    X(MODE_T2, false, 2, 1, 32, 3, false, 2, IGEMM_NORM_FWD, 64, false)         \
    X(MODE_T2, false, 2, 1, 32, 3, false, 2, IGEMM_NORM_BWD2, 64, false)        \
    X(MODE_T2, false, 2, 1, 16, 3, false, 2, IGEMM_PLAIN, 64, false)            \
    GS_IGEMM_FORCED(X)

static bool igemm_instantiated(int mode, int dtype, const IgemmCfg& c) {
#define GS_ROW(M, BF16_ONLY, ...) if (mode == M && (dtype == GS_BF16 || !BF16_ONLY) && c == IgemmCfg{__VA_ARGS__}) return true;
    GS_IGEMM_CONFIGS(GS_ROW)
#undef GS_ROW
    return false;
}

template <typename T, int MODE>
static int dispatch_igemm(ConvP p, hipStream_t st) {
    constexpr int dtype = sizeof(T) == 4 ? GS_F32 : GS_BF16;
    const int want = p.normbwd ? 1 + p.normbwd : (p.y2 ? IGEMM_NORM_FWD : IGEMM_PLAIN);   // the epilogue asked for, as ConvP carries it
    IgemmCfg c = choose_igemm(MODE, dtype, p.N, p.Hb, p.Wb, p.IC, p.OC, want, num_cus(), igemm_knobs());
#ifdef GS_FORCE_CFG
    if (MODE == GS_FORCE_MODE && dtype == GS_BF16) c = IgemmCfg{GS_FORCE_CFG};
#endif
#define GS_ROW(M, BF16_ONLY, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC)                                \
    if constexpr (MODE == M && (dtype == GS_BF16 || !BF16_ONLY))                                       \
        if (c == IgemmCfg{A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC}) return launch_igemm<T, MODE, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC>(p, st);
    GS_IGEMM_CONFIGS(GS_ROW)
#undef GS_ROW
    return fail(GS_ERR_UNSUPPORTED, "conv igemm: no instantiation of mode %d dtype %d A=%d B=%d TW=%d TG=%d RESIDENT=%d D=%d NORM=%d RB=%d SPEC=%d", MODE, dtype,
                c.A, c.B, c.TW, c.TG, (int)c.RESIDENT, c.D, c.NORM, c.RB, (int)c.SPEC);
}

// does the layer get the epilogue `want` (IGEMM_NORM_*), i.e. run as one launch?
bool igemm_norm_fused(int mode, int N, int Hb, int Wb, int IC, int OC, int dtype, int want) {
    return igemm_supported(IC, OC, dtype) && choose_igemm(mode, dtype, N, Hb, Wb, IC, OC, want, num_cus(), igemm_knobs()).NORM == want;
}
// gs_conv_igemm_config: the chosen fields in IgemmCfg's order, then whether that (mode, dtype, configuration) is compiled
int igemm_config(int mode, int N, int Hb, int Wb, int IC, int OC, int dtype, int want, int* out) {
    if (mode < MODE_S1 || mode > MODE_T2 || (dtype != GS_F32 && dtype != GS_BF16) || want < IGEMM_PLAIN || want > IGEMM_NORM_BWD2 || N < 1 || Hb < 1 || Wb < 1 || !out)
        return fail(GS_ERR_ARG, "conv igemm config: bad mode %d / dtype %d / epilogue %d / shape %d x %d x %d", mode, dtype, want, N, Hb, Wb);
    if (!igemm_supported(IC, OC, dtype)) return fail(GS_ERR_UNSUPPORTED, "conv igemm config: %d -> %d channels do not run on the implicit GEMM", IC, OC);
    const IgemmCfg c = choose_igemm(mode, dtype, N, Hb, Wb, IC, OC, want, num_cus(), igemm_knobs());
    const int v[10] = {c.A, c.B, c.TW, c.TG, c.RESIDENT, c.D, c.NORM, c.RB, c.SPEC, igemm_instantiated(mode, dtype, c)};
    memcpy(out, v, sizeof(v));
    return 0;
}
// gs_conv_igemm_table: row `index` of GS_IGEMM_CONFIGS as the table spells it -- mode, BF16_ONLY, then IgemmCfg's fields -- expanded from the
// table itself.  The probes' forced row (last, GS_FORCE_CFG builds only) is not a row of the table.
int igemm_table(int index, int* out) {
    static const int rows[][11] = {
#define GS_ROW(M, BF16_ONLY, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC) {M, BF16_ONLY, A, B, TW, TG, RESIDENT, D, NORM, RB, SPEC},
        GS_IGEMM_CONFIGS(GS_ROW)
#undef GS_ROW
    };
#ifdef GS_FORCE_CFG
    constexpr int n = (int)(sizeof(rows) / sizeof(rows[0])) - 1;
#else
    constexpr int n = (int)(sizeof(rows) / sizeof(rows[0]));
#endif
    if (index < 0 || index >= n || !out) return fail(GS_ERR_ARG, "conv igemm table: row %d of %d", index, n);
    memcpy(out, rows[index], sizeof(rows[0]));
    return 0;
}

size_t igemm_prep_bytes(int ic, int oc, int dtype) {
    return align256((size_t)9 * ic * oc * (dtype == GS_F32 ? 4 : 2));
}

// mode: MODE_*; variant: weight_prep variant; (ICk, OCk) are the kernel-role channel counts
template <typename T>
static int run_igemm_t(int mode, int variant, const void* x, const float* w_hwio, void* y, int N, int Hi, int Wi,
                       int ICk, int OCk, int w_ci, int w_co, int Hb, int Wb, float alpha, const float* bias, int act,
                       int w_prepared, void* ws, size_t ws_bytes, hipStream_t st, const void* mask, int mask_act, void* y2, float pn_eps,
                       const void* addend, int normbwd) {
    const size_t need = (size_t)9 * w_ci * w_co * sizeof(T);
    if (ws_bytes < need) return fail(GS_ERR_WORKSPACE, "conv igemm: workspace %zu < %zu", ws_bytes, need);
    T* wp = reinterpret_cast<T*>(ws);
    const long total = 9L * w_ci * w_co;
    if (!w_prepared)
        hipLaunchKernelGGL((weight_prep_kernel<T>), dim3(cdiv(total, 256)), dim3(256), 0, st, w_hwio, wp, 9, w_ci, w_co, variant);
    ConvP p;
    memset(&p, 0, sizeof(p));
    const size_t out_numel = (size_t)N * Hb * Wb * (mode == MODE_T2 ? 4 : 1) * OCk;
    const bool plain = y2 == nullptr && !normbwd;   // (the fused-norm epilogues need z itself and write no bits)
    const bool write_bits = (act & GS_ACT_WRITE_BITS) != 0;
    act &= ~GS_ACT_WRITE_BITS;
    if (mask_act == GS_ACT_LRELU_BITS) {   // mask = an activation output with its sign bits behind it
        mask_act = GS_ACT_LRELU;
        if (sizeof(T) == 2 && plain && mask && OCk % 32 == 0) p.mask_bits = reinterpret_cast<const unsigned char*>(mask) + out_numel * sizeof(T);
    }
    bool bits_pending = write_bits;
    if (write_bits && sizeof(T) == 2 && plain && y && act == GS_ACT_LRELU && OCk % 32 == 0 && (!mask || p.mask_bits)) {   // (the BITS kernel reads no mask VALUES)
        p.bits_out = reinterpret_cast<unsigned char*>(y) + out_numel * sizeof(T);
        bits_pending = false;
    }
    p.x = x; p.wp = wp; p.y = y; p.bias = bias; p.act = act; p.mask = mask; p.mask_act = mask_act;
    p.N = N; p.Hi = Hi; p.Wi = Wi; p.IC = ICk; p.OC = OCk; p.Hb = Hb; p.Wb = Wb; p.alpha = alpha;
    int pending = 0;
    p.y2 = y2; p.pn_eps = pn_eps; p.norm_pending = &pending;
    p.addend = normbwd ? addend : nullptr; p.normbwd = normbwd;
    int rc;
    if (mode == MODE_S1) rc = dispatch_igemm<T, MODE_S1>(p, st);
    else if (mode == MODE_S2) rc = dispatch_igemm<T, MODE_S2>(p, st);
    else rc = dispatch_igemm<T, MODE_T2>(p, st);
    if (rc) return rc;
    GS_CHECK_LAUNCH();
    if (pending == 3) {   // second-order form without an epilogue: y holds t; both gradients from the norm's own kernel (y in place, y2)
        const long px = (long)N * Hb * Wb * (mode == MODE_T2 ? 4 : 1);
        return gs_pixel_norm_bwd_bwd_fused(y, addend, mask, y2, y, px, OCk, pn_eps, mask_act, sizeof(T) == 4 ? GS_F32 : GS_BF16, st);
    }
    if (pending == 2) {   // no fused pixel-norm backward for this shape: y holds the plain data gradient g; the norm's backward runs in place
        const long px = (long)N * Hb * Wb * (mode == MODE_T2 ? 4 : 1);
        return gs_pixel_norm_bwd_fused(y, mask, addend, y, px, OCk, pn_eps, GS_ACT_NONE, mask_act, sizeof(T) == 4 ? GS_F32 : GS_BF16, st);
    }
    if (pending) {   // y2 = pixel_norm(activation), the activation sitting in y (or in y2 itself when the caller keeps no copy)
        const long px = (long)N * Hb * Wb * (mode == MODE_T2 ? 4 : 1);
        if (int e = gs_pixel_norm_fwd(y ? y : y2, y2, px, OCk, pn_eps, sizeof(T) == 4 ? GS_F32 : GS_BF16, st)) return e;
    }
    if (bits_pending && y)   // (asked for the sign bits where this epilogue does not write them: the packing pass)
        return gs_pack_act_bits(y, (int64_t)(out_numel / OCk), OCk, sizeof(T) == 4 ? GS_F32 : GS_BF16, st);
    return 0;
}

int run_igemm(int mode, int variant, const void* x, const float* w_hwio, void* y, int N, int Hi, int Wi, int ICk,
              int OCk, int w_ci, int w_co, int Hb, int Wb, float alpha, const float* bias, int act, int dtype, int w_prepared,
              void* ws, size_t ws_bytes, hipStream_t st, const void* mask, int mask_act, void* y2, float pn_eps, const void* addend, int normbwd) {
    GS_DISPATCH_DTYPE(dtype, return (run_igemm_t<T>(mode, variant, x, w_hwio, y, N, Hi, Wi, ICk, OCk, w_ci, w_co, Hb,
                                                    Wb, alpha, bias, act, w_prepared, ws, ws_bytes, st, mask, mask_act, y2, pn_eps, addend, normbwd)));
}

}  // namespace gs

extern "C" int gs_prof_enable(int on) {
    gs::g_prof.on = on != 0;
    gs::g_prof.burst = on > 1 ? on : 1;
    gs::g_prof.used = 0;
    gs::g_prof.flops = 0.0;
    return 0;
}

// Roofline accounting of the same launches: total algorithmic bytes, and the sum over launches of the time the binding roof
// (MFMA peak or HBM bandwidth, whichever is larger for that launch) allows.  Call BEFORE gs_prof_collect (which resets).
extern "C" int gs_prof_roofline(double peak_tflops, double peak_gbps, double* total_bytes, double* roof_ms, double* roof_ms_hbm_bound) {
    double bytes = 0.0, roof = 0.0, roof_hbm = 0.0;
    for (int i = 0; i < gs::g_prof.used; ++i) {
        if (gs::g_prof.ldesc[i][0] >= 10) continue;
        const double tf = gs::g_prof.lflops[i] / (peak_tflops * 1e12) * 1e3, tb = gs::g_prof.lbytes[i] / (peak_gbps * 1e9) * 1e3;
        bytes += gs::g_prof.lbytes[i];
        roof += tf > tb ? tf : tb;
        if (tb >= tf) roof_hbm += tb;
    }
    if (total_bytes) *total_bytes = bytes;
    if (roof_ms) *roof_ms = roof;
    if (roof_ms_hbm_bound) *roof_ms_hbm_bound = roof_hbm;
    return 0;
}

// Per-launch records of everything recorded since gs_prof_enable(1) (implicit-GEMM convs AND weight gradients): duration (ms),
// algorithmic FLOPs and bytes, and 8 ints {kind, N, Hb, Wb, IC, OC, masked | sources, fused norm | deferred}; kind = conv mode
// (0 stride 1, 1 stride 2, 2 transposed) or 10 + mode for the weight gradient of that conv.  Call BEFORE gs_prof_collect.
extern "C" int gs_prof_records(int max_records, int* n, double* ms, double* flops, double* bytes, int* desc) {
    int k = 0;
    for (int i = 0; i < gs::g_prof.used && k < max_records; ++i, ++k) {
        (void)hipEventSynchronize(gs::g_prof.ev[i][1]);
        float t = 0.f;
        if (hipEventElapsedTime(&t, gs::g_prof.ev[i][0], gs::g_prof.ev[i][1]) != hipSuccess) t = 0.f;
        t /= (float)gs::g_prof.lreps[i];
        ms[k] = t; flops[k] = gs::g_prof.lflops[i]; bytes[k] = gs::g_prof.lbytes[i];
        for (int j = 0; j < 8; ++j) desc[8 * k + j] = gs::g_prof.ldesc[i][j];
    }
    if (n) *n = k;
    return 0;
}

extern "C" int gs_prof_collect(int* launches, double* total_ms, double* total_flops) {
    double ms = 0.0;
    int count = 0;
    for (int i = 0; i < gs::g_prof.used; ++i) {
        if (gs::g_prof.ldesc[i][0] >= 10) continue;
        ++count;
        (void)hipEventSynchronize(gs::g_prof.ev[i][1]);
        float t = 0.f;
        if (hipEventElapsedTime(&t, gs::g_prof.ev[i][0], gs::g_prof.ev[i][1]) == hipSuccess) ms += t / (float)gs::g_prof.lreps[i];
    }
    if (launches) *launches = count;
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = gs::g_prof.flops;
    gs::g_prof.used = 0;
    gs::g_prof.flops = 0.0;
    return 0;
}
