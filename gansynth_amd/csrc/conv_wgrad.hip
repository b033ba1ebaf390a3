// Every conv weight gradient: the 3x3 convs on the MFMA units (channels-last activations, K = pixels), the direct VALU kernels of the 1- / 2-channel
// layers (conv_wgrad_direct_kernel, thin_wgrad_kernel), the host planning that chooses among them (wgrad_plan) and the slice reductions that fold
// every kernel's block partials.
#include "conv_device.h"
#include "gs_prof.h"

namespace gs {

// --------------------------------------------------------------------- weight gradient
// gw[tap][ic][oc] = sum_pixels x[in(pixel,tap)][ic] * gy[pixel][oc].  MFMA with K = pixels:
// A[i=ic][k=pixel], B[k=pixel][j=oc].  A block owns a 32x32 (ic,oc) tile for all 9 taps and
// strides over spatial tiles (`slice`); its 4 waves split each tile's pixels, then reduce through
// LDS and write one fp32 partial per slice (summed by wgrad_reduce_kernel -> deterministic).
template <typename T, int MODE, int TW>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(
    const WgradSrcs srcs, float* __restrict__ part,
    int N, int Hi, int Wi, int IC, int OC, int Hb, int Wb, int tiles_x, int tiles_y, int ntiles, int nslices) {
    // T = bf16: operands are widened to fp32 while staging (exact), the contraction runs on the fp32 MFMA.
    constexpr int NP = MODE == MODE_S2 ? 64 : 128;
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int S = MODE == MODE_S2 ? 2 : 1;
    constexpr int ROWF = 32;  // floats per LDS row (32 channels)
    constexpr int LDS_MAIN = (PH * PW + NP) * ROWF;
    constexpr int LDS_RED = 4 * 1024;
    __shared__ __attribute__((aligned(16))) float lds[LDS_MAIN > LDS_RED ? LDS_MAIN : LDS_RED];
    float* lp = lds;
    float* lg = lds + PH * PW * ROWF;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int n_ict = IC / 32;
    const int ic0 = (blockIdx.x % n_ict) * 32, oc0 = (blockIdx.x / n_ict) * 32;
    const int slice = blockIdx.y;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int tile = slice; tile < ntiles; tile += nslices) {
        int b = tile;
        const int tile_x = b % tiles_x;
        b /= tiles_x;
        const int tile_y = b % tiles_y;
        int n;
        const int src = wgrad_source(srcs, b / tiles_y, n);
        const T* __restrict__ x = reinterpret_cast<const T*>(srcs.x[src]);
        const T* __restrict__ gy = reinterpret_cast<const T*>(srcs.gy[src]);
        const int by = tile_y * TH, bx = tile_x * TW;
        const int oy0 = MODE == MODE_S2 ? 2 * by : by - 1;
        const int ox0 = MODE == MODE_S2 ? 2 * bx : bx - 1;
        __syncthreads();
        for (int c = tid; c < PH * PW * 8; c += 256) {
            const int pix = c >> 3, part = c & 7;
            const int ly = pix / PW, lx = pix % PW;
            const int iy = oy0 + ly, ix = ox0 + lx;
            float v[4];
            const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
            ld4(ok ? x + (((long)n * Hi + iy) * Wi + ix) * IC + ic0 + part * 4 : x, v);  // unconditional load, zero-select after
            *reinterpret_cast<float4*>(lp + pix * ROWF + part * 4) = ok ? make_float4(v[0], v[1], v[2], v[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int c = tid; c < NP * 8; c += 256) {
            const int pix = c >> 3, part = c & 7;
            const int gy_ = by + pix / TW, gx_ = bx + pix % TW;
            float v[4];
            const bool ok = gy_ < Hb && gx_ < Wb;
            ld4(ok ? gy + (((long)n * Hb + gy_) * Wb + gx_) * OC + oc0 + part * 4 : gy, v);
            *reinterpret_cast<float4*>(lg + pix * ROWF + part * 4) = ok ? make_float4(v[0], v[1], v[2], v[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
#pragma unroll 2
        for (int pp = 0; pp < NP / 8; ++pp) {
            const int p = wv * (NP / 4) + 2 * pp + hi;
            const int ty = p / TW, tx = p % TW;
            const float bfrag = lg[p * ROWF + l31];
            const float* pbase = lp + ((ty * S) * PW + tx * S) * ROWF + l31;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float afrag = pbase[((t / 3) * PW + (t % 3)) * ROWF];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(afrag, bfrag, acc[t], 0, 0, 0);
            }
        }
    }
    // ---- cross-wave reduction, one tap at a time: lds[wave][ic i][oc j]
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
            lds[wv * 1024 + i * 32 + l31] = acc[t][r];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = tid + 256 * k;
            const float s = lds[e] + lds[1024 + e] + lds[2048 + e] + lds[3072 + e];
            const int i = e >> 5, j = e & 31;
            part[(((long)slice * 9 + t) * IC + ic0 + i) * OC + oc0 + j] = s;
        }
    }
}

// bf16 weight gradient on the bf16 MFMA (32x32x16, K = 16 pixels per instruction).
// The contraction index is the PIXEL while channels-last tiles keep channels contiguous, i.e. the operands
// sit K-major in LDS ([pixel][32 channels], 64-byte rows, staged with plain 16-byte copies).  gfx950's
// transposing LDS read ds_read_b64_tr_b16 turns that into K-contiguous fragments for free.  Measured
// semantics (scripts/probe/tr_probe.hip): inside each 16-lane group, lane s supplies the address of 4
// consecutive b16 (8 bytes); lane i = 4m + pos receives, for j = 0..3, element `pos` of the data supplied
// by lane 4j + m.  With lane s pointing at (pixel row k0 + (s >> 2), channels 4(s & 3)..+3) every lane gets
// 4 consecutive pixels of its own channel; two reads = one MFMA operand.  The three horizontal taps of a
// kernel row use overlapping pixel windows, so 3 reads (12 pixels) + 4 v_alignbit feed 3 MFMAs.
// Block = 192 threads = 3 waves; wave w owns kernel row ky = w (3 taps, 48 fp32 accumulators) over all pixels
// of the tile: no cross-wave reduction, small register footprint, 3 blocks per CU.
__device__ inline unsigned int shr16(unsigned int hi, unsigned int lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }
__device__ inline bf16x8 mk_frag(unsigned int a, unsigned int b, unsigned int c, unsigned int d) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 v = {a, b, c, d};
    return __builtin_bit_cast(bf16x8, v);
}
__device__ inline uint2 lds_tr16(const unsigned char* p) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (s16x4 __attribute__((address_space(3)))*)(reinterpret_cast<const s16x4*>(p)));
    return __builtin_bit_cast(uint2, v);
}

// acc += a.lo + a.hi for a packed bf16 pair (v_dot2c_f32_bf16 against (1, 1); hipcc has no builtin for it on gfx950)
__device__ inline void add_bf16_pair(float& acc, unsigned int a) {
    asm volatile("v_dot2c_f32_bf16 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(0x3F803F80u));
}

// OT = 2: the block owns TWO 32-channel output tiles (a 32 x 64 pair): the patch is staged and its fragments are read once for both --
// the 32 -> 64 stride-2 layer of the top of the pyramid re-staged its (4-5x larger) patch for each of its two output tiles.
template <int MODE, int TW, int OT = 1>
__global__ __launch_bounds__(192) void conv_wgrad_bf16_kernel(
    const WgradSrcs srcs, float* __restrict__ part,
    int N, int Hi, int Wi, int IC, int OC, int Hb, int Wb, int tiles_x, int tiles_y, int ntiles, int nslices, int with_bias) {
    constexpr bool S2 = MODE == MODE_S2;
    constexpr int NP = S2 ? 128 : 256;
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int S = S2 ? 2 : 1;
    constexpr int XCH = PH * PW * 4, GCH = NP * 4 * OT;     // 16-byte chunks to stage (gradient tile: OT planes of 32 channels)
    constexpr int XIT = (XCH + 191) / 192, GIT = (GCH + 191) / 192;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[(PH * PW + NP * OT) * 64];
    unsigned char* const lx_ = lds_raw;
    unsigned char* const lg_ = lds_raw + PH * PW * 64;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int n_ict = IC / 32;
    const int ic0 = (blockIdx.x % n_ict) * 32, oc0 = (blockIdx.x / n_ict) * 32 * OT;
    const int slice = blockIdx.y;
    // transposing-read supplier role of this lane: pixel row (lane & 15) >> 2 of the 4-row block, channel quad
    const int t_row = (lane & 15) >> 2;
    const int t_col = (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;  // byte offset inside the 64-byte row

    f32x16 acc[OT][3];
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[o][t][r] = 0.f;
    // bias gradient = sum over pixels of gy: the gradient fragment of a lane is 8 pixels of its output channel, four packed
    // dot-2 adds per pixel group fold them into one register; done by the first wave of the blocks of input-channel tile 0
    const bool bias_wave = with_bias && wv == 0 && ic0 == 0;
    float accb[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) accb[o] = 0.f;

    // Software pipeline over the block's tiles: the global loads of tile t + 1 are issued -- into
    // registers -- BEFORE the MFMAs of tile t and stored to LDS after them, so that a block's memory latency runs under its own MFMAs instead
    // of only under those of the two other blocks of the CU.  These layers are HBM-bound (32 channels: 144 flop/byte): what counts is bytes in
    // flight per CU.
    uint4 xv[XIT], gv[GIT];
    unsigned int xok = 0, gok = 0;
    bool bias_fetched = false;
    auto fetch = [&](int tile) __attribute__((always_inline)) {
        int b = tile;
        const int tile_x = b % tiles_x;
        b /= tiles_x;
        const int tile_y = b % tiles_y;
        int n;
        const int src = wgrad_source(srcs, b / tiles_y, n);
        const bf16_t* __restrict__ x = reinterpret_cast<const bf16_t*>(srcs.x[src]);
        const bf16_t* __restrict__ gy = reinterpret_cast<const bf16_t*>(srcs.gy[src]);
        bias_fetched = bias_wave && ((srcs.bias_mask >> src) & 1u);
        const int by = tile_y * TH, bx = tile_x * TW;
        const int oy0 = S2 ? 2 * by : by - 1;
        const int ox0 = S2 ? 2 * bx : bx - 1;
        xok = 0; gok = 0;
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int c = tid + 192 * it;
            const int pix = c >> 2, part4 = c & 3;
            const int ly = pix / PW, lx = pix - ly * PW;
            const int iy = oy0 + ly, ix = ox0 + lx;
            const bool ok = c < XCH && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
            xok |= ok ? (1u << it) : 0u;   // loads are unconditional; out-of-image slots are zeroed at the LDS store
            xv[it] = *reinterpret_cast<const uint4*>(ok ? x + (((long)n * Hi + iy) * Wi + ix) * IC + ic0 + part4 * 8 : x);
        }
#pragma unroll
        for (int it = 0; it < GIT; ++it) {
            const int c = tid + 192 * it;   // chunk c of LDS plane c / (NP * 4): pixel (c >> 2) % NP, channels 32 plane + 8 (c & 3)
            const int pix = (c >> 2) % NP, part4 = (c & 3) + 4 * (c / (NP * 4));
            const int gy_ = by + pix / TW, gx_ = bx + pix % TW;
            const bool ok = c < GCH && gy_ < Hb && gx_ < Wb;
            gok |= ok ? (1u << it) : 0u;
            gv[it] = *reinterpret_cast<const uint4*>(ok ? gy + (((long)n * Hb + gy_) * Wb + gx_) * OC + oc0 + part4 * 8 : gy);
        }
    };
    if (slice < ntiles) fetch(slice);
    for (int tile = slice; tile < ntiles; tile += nslices) {
        const bool do_bias = bias_fetched;
        __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int c = tid + 192 * it;
            if (c < XCH) *reinterpret_cast<uint4*>(lx_ + c * 16) = (xok >> it) & 1u ? xv[it] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int it = 0; it < GIT; ++it) {
            const int c = tid + 192 * it;
            if (c < GCH) *reinterpret_cast<uint4*>(lg_ + c * 16) = (gok >> it) & 1u ? gv[it] : make_uint4(0, 0, 0, 0);
        }
        if (tile + nslices < ntiles) fetch(tile + nslices);   // in flight under the MFMAs below
        __syncthreads();
        // ---- MFMAs: this wave's kernel row (ky = wv) over every 16-pixel group of the tile
#pragma unroll 2
        for (int g = 0; g < NP / 16; ++g) {
            const int ty = (g * 16) / TW, tx0 = (g * 16) % TW + 8 * hi;
            bf16x8 bfrag[OT];
#pragma unroll
            for (int o = 0; o < OT; ++o) {
                const unsigned char* gp = lg_ + o * NP * 64 + (ty * TW + tx0 + t_row) * 64 + t_col;
                const uint2 b0 = lds_tr16(gp), b1 = lds_tr16(gp + 4 * 64);
                bfrag[o] = mk_frag(b0.x, b0.y, b1.x, b1.y);
                if (do_bias) { add_bf16_pair(accb[o], b0.x); add_bf16_pair(accb[o], b0.y); add_bf16_pair(accb[o], b1.x); add_bf16_pair(accb[o], b1.y); }
            }
            const unsigned char* xp = lx_ + (((ty * S + wv) * PW + tx0 * S) + t_row * S) * 64 + t_col;
            if (!S2) {
                const uint2 d0 = lds_tr16(xp), d1 = lds_tr16(xp + 4 * 64), d2 = lds_tr16(xp + 8 * 64);
                const bf16x8 a0 = mk_frag(d0.x, d0.y, d1.x, d1.y), a1 = mk_frag(shr16(d0.y, d0.x), shr16(d1.x, d0.y), shr16(d1.y, d1.x), shr16(d2.x, d1.y)),
                             a2 = mk_frag(d0.y, d1.x, d1.y, d2.x);
#pragma unroll
                for (int o = 0; o < OT; ++o) {
                    acc[o][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bfrag[o], acc[o][0], 0, 0, 0);
                    acc[o][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bfrag[o], acc[o][1], 0, 0, 0);
                    acc[o][2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, bfrag[o], acc[o][2], 0, 0, 0);
                }
            } else {
                // even columns 2(p)+0 / +2 share a 9-pixel window; odd columns 2(p)+1 are their own 8-pixel window
                const uint2 e0 = lds_tr16(xp), e1 = lds_tr16(xp + 8 * 64), e2 = lds_tr16(xp + 16 * 64);
                const uint2 o0 = lds_tr16(xp + 64), o1 = lds_tr16(xp + 9 * 64);
                const bf16x8 a0 = mk_frag(e0.x, e0.y, e1.x, e1.y), a1 = mk_frag(o0.x, o0.y, o1.x, o1.y),
                             a2 = mk_frag(shr16(e0.y, e0.x), shr16(e1.x, e0.y), shr16(e1.y, e1.x), shr16(e2.x, e1.y));
#pragma unroll
                for (int o = 0; o < OT; ++o) {
                    acc[o][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bfrag[o], acc[o][0], 0, 0, 0);
                    acc[o][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bfrag[o], acc[o][1], 0, 0, 0);
                    acc[o][2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, bfrag[o], acc[o][2], 0, 0, 0);
                }
            }
        }
    }
    // ---- each wave owns its 3 taps: D[ic i][oc j], lane = (j = l31, i = (r&3) + 8(r>>2) + 4hi)
    const long pstride = 9L * IC * OC + (with_bias ? OC : 0);   // fp32 elements per slice: 9 taps (+ the bias row)
#pragma unroll
    for (int o = 0; o < OT; ++o) {
        if (bias_wave) {   // the two lane halves hold different pixels of the same channel
            const float tot = swap32_sum(accb[o]);
            if (hi == 0) part[(long)slice * pstride + 9L * IC * OC + oc0 + o * 32 + l31] = tot;
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            float* dst = part + (long)slice * pstride + (((long)wv * 3 + kx) * IC + ic0) * OC + oc0 + o * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(long)((r & 3) + 8 * (r >> 2) + 4 * hi) * OC] = acc[o][kx][r];
        }
    }
}

// The same contraction for the HBM-bound top of the pyramid (32 input channels: 144 flop / byte), staged by LDS-DMA and wave-specialised.
// SQ counters of conv_wgrad_bf16_kernel on these layers (profiles/r04_n_step_sq_pmc.txt): ~810 VALU instructions per tile and wave for 48 MFMAs --
// the per-thread address arithmetic of 14 16-byte loads, their border selects and LDS stores -- waves issuing 47 % of the time, MFMA pipe busy
// 17 %, 2.9 TB/s over x + gy where a streaming kernel reaches 4.5-6: the kernel is bound by its own instruction stream, not by HBM.  Here
//   * wave 3 is the LOADER: it owns the tile descriptors and issues every DMA piece of tile t + 1 (1 KiB = 16 pixel rows of 64 bytes each,
//     plain row-major: exactly the [pixel][32 channels] layout the transposing reads want; rows above / below the image fall outside the
//     per-image descriptor and arrive as zeros, columns outside are forced out of range) while
//   * waves 0-2 (wave = kernel row, 3 taps, no cross-wave reduction: as conv_wgrad_bf16_kernel) run the MFMAs of tile t from the other buffer;
//   * ONE barrier per tile: behind the loader's vmcnt(0).  It publishes tile t and, since the loader issues tile t + 1 only after it, also
//     says that every compute wave is done with the buffer tile t + 1 goes to.
// Two blocks per CU (2 x ~77 KiB of LDS): 77 KiB in flight per CU at any time.  TW = 32 only; stride 2 takes 64-pixel tiles (its patch is
// 4.6x the tile).  Same partial layout as conv_wgrad_bf16_kernel: the fold does not know which kernel ran.
template <int MODE, int OT>
__global__ __launch_bounds__(256, 2) void conv_wgrad_bf16_thin_dma_kernel(   // (two waves per SIMD: two blocks per CU must fit the register file)
    const WgradSrcs srcs, float* __restrict__ part,
    int N, int Hi, int Wi, int IC, int OC, int Hb, int Wb, int tiles_x, int tiles_y, int ntiles, int nslices, int with_bias) {
    constexpr bool S2 = MODE == MODE_S2;
    constexpr int TW = 32;
    constexpr int NP = S2 ? 64 : 256;
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int S = S2 ? 2 : 1;
    constexpr int XP = (PH * PW + 15) / 16;     // 1 KiB pieces (16 rows of 64 bytes) of the patch ...
    constexpr int GP = NP / 16;                 // ... and of one 32-channel plane of the gradient tile
    constexpr int XB = XP * 1024, GB = NP * 64;
    constexpr int BUF = XB + OT * GB;           // one staged tile; two of them
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const unsigned a_base = (unsigned)(uintptr_t)lds_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wv == 3;
    const int oc0 = blockIdx.x * 32 * OT;       // (IC == 32: one input-channel tile)
    const int slice = blockIdx.y;
    const int t_row = (lane & 15) >> 2;
    const int t_col = (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;

    // ---- loader: piece j of the patch = rows 16 j + (lane >> 2) of its PH x PW pixel rows.  The (patch row, column) of a lane's row is
    //      walked incrementally from piece to piece (+16 columns, wrapping at PW) instead of being kept in 2 x XP registers: the register
    //      file is shared with the compute waves' accumulators, and the loader has instruction slots to spare
    const int x_lx0 = lane >> 2;                                 // row of piece 0: patch row 0, column lane >> 2 (PW > 16)
    const int x_voff0 = (x_lx0 * IC) * 2 + (lane & 3) * 16;
    // a gradient piece = 16 consecutive pixels of one tile row: pixel (j >> 1, 16 (j & 1) + (lane >> 2))
    const int g_lane = ((lane >> 2) * OC) * 2 + (lane & 3) * 16;
    const unsigned ximg = (unsigned)Hi * Wi * IC * 2, gimg = (unsigned)Hb * Wb * OC * 2;

    f32x16 acc[OT][3];
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[o][t][r] = 0.f;
    const bool bias_wave = with_bias && wv == 0;
    float accb[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) accb[o] = 0.f;

    auto tile_coords = [&](int tile, int& n, int& by, int& bx) __attribute__((always_inline)) {   // -> source index
        int b = tile;
        const int tile_x = b % tiles_x;
        b /= tiles_x;
        const int tile_y = b % tiles_y;
        const int src = wgrad_source(srcs, b / tiles_y, n);
        by = tile_y * TH;
        bx = tile_x * TW;
        return src;
    };
    auto issue_tile = [&](int tile, int bufi) __attribute__((always_inline)) {
        int n, by, bx;
        const int src = tile_coords(tile, n, by, bx);
        const int oy0 = S2 ? 2 * by : by - 1, ox0 = S2 ? 2 * bx : bx - 1;
        const i32x4 rs_x = make_rsrc(reinterpret_cast<const unsigned char*>(srcs.x[src]) + (size_t)n * ximg, ximg);
        const i32x4 rs_g = make_rsrc(reinterpret_cast<const unsigned char*>(srcs.gy[src]) + (size_t)n * gimg, gimg);
        const int xorg = ((oy0 * Wi + ox0) * IC) * 2;
        const unsigned a_x = a_base + bufi * BUF, a_g = a_x + XB;
        int lx = x_lx0, voff = xorg + x_voff0;
        asm volatile("" : "+v"(lx));   // (opaque per tile: or the compiler hoists the whole column walk out of the tile loop -- 2 x XP registers again)
        const int wrap = ((Wi - PW) * IC) * 2;                  // byte step from (ly, lx + PW) to (ly + 1, lx)
#pragma unroll
        for (int j = 0; j < XP; ++j) {
            // (the last piece's rows past the patch: any column outside the image will do -- they are never read)
            const bool in = (unsigned)(ox0 + lx) < (unsigned)Wi && (j * 16 + 15 < PH * PW || j * 16 + (lane >> 2) < PH * PW);
            lds_dma16(a_x + j * 1024, in ? (unsigned)voff : 0x80000000u, rs_x);
            lx += 16;
            voff += 16 * IC * 2;
            const bool w = lx >= PW;
            lx = w ? lx - PW : lx;
            voff = w ? voff + wrap : voff;
        }
        const bool in0 = bx + (lane >> 2) < Wb, in1 = bx + 16 + (lane >> 2) < Wb;
#pragma unroll
        for (int o = 0; o < OT; ++o)
#pragma unroll
            for (int j = 0; j < GP; ++j) {
                const int gy_ = by + (j >> 1);                        // (wave-uniform)
                const int gorg = ((gy_ * Wb + bx + 16 * (j & 1)) * OC + oc0 + 32 * o) * 2;
                const unsigned v = (gy_ < Hb && ((j & 1) ? in1 : in0)) ? (unsigned)(gorg + g_lane) : 0x80000000u;
                lds_dma16(a_g + o * GB + j * 1024, v, rs_g);
            }
    };

    int buf = 0;
    if (loader && slice < ntiles) issue_tile(slice, 0);
    for (int tile = slice; tile < ntiles; tile += nslices) {
        if (loader) wait_vmcnt(0);   // this tile has landed ...
        block_barrier();             // ... for everybody; and everybody is done with the other buffer
        if (loader) {
            if (tile + nslices < ntiles) issue_tile(tile + nslices, buf ^ 1);
        } else {
            bool do_bias = false;
            if (bias_wave) {
                int n, by, bx;
                do_bias = (srcs.bias_mask >> tile_coords(tile, n, by, bx)) & 1u;
            }
            const unsigned char* const lx_ = lds_raw + buf * BUF;
            const unsigned char* const lg_ = lx_ + XB;
            auto group = [&](int g) __attribute__((always_inline)) {
                const int ty = (g * 16) / TW, tx0 = (g * 16) % TW + 8 * hi;
                bf16x8 bfrag[OT];
#pragma unroll
                for (int o = 0; o < OT; ++o) {
                    const unsigned char* gp = lg_ + o * GB + (ty * TW + tx0 + t_row) * 64 + t_col;
                    const uint2 b0 = lds_tr16(gp), b1 = lds_tr16(gp + 4 * 64);
                    bfrag[o] = mk_frag(b0.x, b0.y, b1.x, b1.y);
                    if (do_bias) { add_bf16_pair(accb[o], b0.x); add_bf16_pair(accb[o], b0.y); add_bf16_pair(accb[o], b1.x); add_bf16_pair(accb[o], b1.y); }
                }
                const unsigned char* xp = lx_ + (((ty * S + wv) * PW + tx0 * S) + t_row * S) * 64 + t_col;
                if (!S2) {
                    const uint2 d0 = lds_tr16(xp), d1 = lds_tr16(xp + 4 * 64), d2 = lds_tr16(xp + 8 * 64);
                    const bf16x8 a0 = mk_frag(d0.x, d0.y, d1.x, d1.y), a1 = mk_frag(shr16(d0.y, d0.x), shr16(d1.x, d0.y), shr16(d1.y, d1.x), shr16(d2.x, d1.y)),
                                 a2 = mk_frag(d0.y, d1.x, d1.y, d2.x);
#pragma unroll
                    for (int o = 0; o < OT; ++o) {
                        acc[o][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bfrag[o], acc[o][0], 0, 0, 0);
                        acc[o][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bfrag[o], acc[o][1], 0, 0, 0);
                        acc[o][2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, bfrag[o], acc[o][2], 0, 0, 0);
                    }
                } else {
                    // even columns 2(p)+0 / +2 share a 9-pixel window; odd columns 2(p)+1 are their own 8-pixel window
                    const uint2 e0 = lds_tr16(xp), e1 = lds_tr16(xp + 8 * 64), e2 = lds_tr16(xp + 16 * 64);
                    const uint2 o0 = lds_tr16(xp + 64), o1 = lds_tr16(xp + 9 * 64);
                    const bf16x8 a0 = mk_frag(e0.x, e0.y, e1.x, e1.y), a1 = mk_frag(o0.x, o0.y, o1.x, o1.y),
                                 a2 = mk_frag(shr16(e0.y, e0.x), shr16(e1.x, e0.y), shr16(e1.y, e1.x), shr16(e2.x, e1.y));
#pragma unroll
                    for (int o = 0; o < OT; ++o) {
                        acc[o][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bfrag[o], acc[o][0], 0, 0, 0);
                        acc[o][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bfrag[o], acc[o][1], 0, 0, 0);
                        acc[o][2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, bfrag[o], acc[o][2], 0, 0, 0);
                    }
                }
            };
            if constexpr (OT == 1) {
#pragma unroll 2
                for (int g = 0; g < NP / 16; ++g) group(g);
            } else {   // (two output tiles: 96 accumulators -- one group in flight keeps the wave within 256 registers, i.e. two blocks per CU)
#pragma unroll 1
                for (int g = 0; g < NP / 16; ++g) group(g);
            }
        }
        buf ^= 1;
    }
    if (loader) return;
    // ---- each compute wave owns its 3 taps: D[ic i][oc j], lane = (j = l31, i = (r&3) + 8(r>>2) + 4hi)
    const long pstride = 9L * IC * OC + (with_bias ? OC : 0);   // fp32 elements per slice: 9 taps (+ the bias row)
#pragma unroll
    for (int o = 0; o < OT; ++o) {
        if (bias_wave) {   // the two lane halves hold different pixels of the same channel
            const float tot = swap32_sum(accb[o]);
            if (hi == 0) part[(long)slice * pstride + 9L * IC * OC + oc0 + o * 32 + l31] = tot;
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            float* dst = part + (long)slice * pstride + (((long)wv * 3 + kx) * IC) * OC + oc0 + o * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(long)((r & 3) + 8 * (r >> 2) + 4 * hi) * OC] = acc[o][kx][r];
        }
    }
}

// One 16-pixel group of the 64 x 64-tile weight-gradient kernels: 9 MFMAs (3 kernel rows x 3 taps) against the gradient fragment, with the
// OTHER work of the wave interleaved between them -- the fragment reads of the next group (2 gradient + 9 / 15 input reads), the
// v_alignbit windows of the shifted taps, the DMA pieces of the next tile.  A wave issues in order and a 32x32x16 MFMA occupies the
// pipe for 32 cycles, so only what is issued right behind an MFMA runs in its shadow; with the reads and the DMA issue in front of the
// nine MFMAs of a group (round 1) the pipe idled half of the time (measured: 9.7 K cycles per 4.6 K-cycle unit).
//   needs in scope: fb[2][2], fx[2][3][XR], acc[9], accb, do_bias, S2, S, PW, TW, NG, XR, hi, t_row, t_col, issue_piece
#define GS_WG_GROUP_STEP(GI, MORE, XPL, GPL, NBUF)                                                                                  \
    do {                                                                                                                            \
        constexpr int cur_ = (GI) & 1, nxt_ = cur_ ^ 1;                                                                             \
        constexpr bool pre_ = (GI) + 1 < NG;                                                                                        \
        constexpr int NR_ = 2 + 3 * XR;                 /* fragment reads of the next group */                                      \
        constexpr int RPS_ = (NR_ + 8) / 9;             /* ... per MFMA slot */                                                     \
        constexpr int nty_ = (((GI) + 1) * 16) / TW, ntxc_ = (((GI) + 1) * 16) % TW;                                                \
        const unsigned char* const ngp_ = g_ptr_((GPL), nty_, ntxc_);                                                               \
        auto next_read_ = [&](int r) __attribute__((always_inline)) {                                                               \
            if (r < 2) { fb[nxt_][r] = lds_tr16(ngp_ + r * 4 * GROWB); return; }                                                    \
            const int ky = (r - 2) / XR, k = (r - 2) % XR;                                                                          \
            if (!S2) { fx[nxt_][ky][k] = lds_tr16(x_ptr_((XPL), nty_, ky, ntxc_, 0) + k * 4 * XROWB); return; }                     \
            /* stride 2: reads 0-2 = the even columns (rows +0, +8, +16), 3-4 = the odd ones (rows +1, +9) */                       \
            fx[nxt_][ky][k] = k < 3 ? lds_tr16(x_ptr_((XPL), nty_, ky, ntxc_, 0) + k * 8 * XROWB)                                   \
                                    : lds_tr16(x_ptr_((XPL), nty_, ky, ntxc_, 1) + (k - 3) * 8 * XROWB);                            \
        };                                                                                                                          \
        auto slot_ = [&](int m) __attribute__((always_inline)) {                                                                    \
            if (pre_) {                                                                                                             \
                _Pragma("unroll") for (int r = m * RPS_; r < (m + 1) * RPS_ && r < NR_; ++r) next_read_(r);                         \
            }                                                                                                                       \
            if (MORE) {                                                                                                             \
                _Pragma("unroll") for (int q = (GI) * PPG; q < ((GI) + 1) * PPG && q < NPIECE; ++q)                                 \
                    if ((q - (GI) * PPG) * 9 / PPG == m) issue_piece(q, NBUF);                                                      \
            }                                                                                                                       \
            __builtin_amdgcn_sched_barrier(0);                                                                                      \
        };                                                                                                                          \
        const uint2 b0_ = fb[cur_][0], b1_ = fb[cur_][1];                                                                           \
        const bf16x8 bfrag_ = mk_frag(b0_.x, b0_.y, b1_.x, b1_.y);                                                                  \
        if (do_bias) { add_bf16_pair(accb, b0_.x); add_bf16_pair(accb, b0_.y); add_bf16_pair(accb, b1_.x); add_bf16_pair(accb, b1_.y); } \
        _Pragma("unroll") for (int ky = 0; ky < 3; ++ky) {                                                                          \
            if (!S2) {                                                                                                              \
                const uint2 d0 = fx[cur_][ky][0], d1 = fx[cur_][ky][1], d2 = fx[cur_][ky][2];                                       \
                acc[ky * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk_frag(d0.x, d0.y, d1.x, d1.y), bfrag_, acc[ky * 3 + 0], 0, 0, 0); \
                slot_(ky * 3 + 0);                                                                                                  \
                acc[ky * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk_frag(shr16(d0.y, d0.x), shr16(d1.x, d0.y), shr16(d1.y, d1.x), shr16(d2.x, d1.y)), bfrag_, acc[ky * 3 + 1], 0, 0, 0); \
                slot_(ky * 3 + 1);                                                                                                  \
                acc[ky * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk_frag(d0.y, d1.x, d1.y, d2.x), bfrag_, acc[ky * 3 + 2], 0, 0, 0); \
                slot_(ky * 3 + 2);                                                                                                  \
            } else {                                                                                                                \
                /* even columns 2(p)+0 / +2 share a 9-pixel window; odd columns 2(p)+1 are their own 8-pixel window */              \
                const uint2 e0 = fx[cur_][ky][0], e1 = fx[cur_][ky][1], e2 = fx[cur_][ky][2], o0 = fx[cur_][ky][3], o1 = fx[cur_][ky][4]; \
                acc[ky * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk_frag(e0.x, e0.y, e1.x, e1.y), bfrag_, acc[ky * 3 + 0], 0, 0, 0); \
                slot_(ky * 3 + 0);                                                                                                  \
                acc[ky * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk_frag(o0.x, o0.y, o1.x, o1.y), bfrag_, acc[ky * 3 + 1], 0, 0, 0); \
                slot_(ky * 3 + 1);                                                                                                  \
                acc[ky * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk_frag(shr16(e0.y, e0.x), shr16(e1.x, e0.y), shr16(e1.y, e1.x), shr16(e2.x, e1.y)), bfrag_, acc[ky * 3 + 2], 0, 0, 0); \
                slot_(ky * 3 + 2);                                                                                                  \
            }                                                                                                                       \
        }                                                                                                                           \
    } while (0)

// 64 x 64 (input x output channel) tiles per block for layers with >= 64 channels on both sides: the four 32 x 32 pairs of
// the tile share ONE staged copy of the input patch and of the gradient tile (a 32 x 32 block re-stages the patch for every
// output tile and the gradients for every input tile: twice the L2 -> LDS stream per MFMA, and that stream is what bounds the
// kernel).  Block = 256 threads = 4 waves, wave w owns the pair (input tile w >> 1, output tile w & 1) for all 9 taps
// (144 fp32 accumulators); operands sit in LDS as two 32-channel planes per side so that the transposing reads keep their
// conflict-free 64-byte rows.
template <int MODE, int TW>
__global__ __launch_bounds__(256) void conv_wgrad_bf16_2x2_kernel(
    const WgradSrcs srcs, float* __restrict__ part,
    int N, int Hi, int Wi, int IC, int OC, int Hb, int Wb, int tiles_x, int tiles_y, int ntiles, int nslices, int with_bias) {
    constexpr bool S2 = MODE == MODE_S2;
    constexpr int NP = S2 ? 64 : 256;   // stride 2: the patch is 4-5x the tile, 64 output pixels keep two staged tiles in LDS
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int S = S2 ? 2 : 1;
    constexpr int XRG = (PH * PW + 15) / 16;          // 16-row groups (= 1 KiB LDS-DMA pieces) of a patch plane
    constexpr int GRG = NP / 16;
    constexpr int XK = (XRG + 3) / 4, GK = GRG / 4;   // row groups per wave (every wave issues the same number of pieces)
    constexpr int XPL = XK * 4096, GPL = NP * 64;     // bytes of one 32-channel plane
    constexpr int BUF = 2 * XPL + 2 * GPL;            // one staged tile; two of them: the DMA of tile t+1 runs under the MFMAs of tile t
    constexpr int NPIECE = 2 * XK + 2 * GK;           // DMA pieces a wave issues per tile
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const unsigned a_base = (unsigned)(uintptr_t)lds_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_ict = IC / 64;
    const int ic0 = (blockIdx.x % n_ict) * 64, oc0 = (blockIdx.x / n_ict) * 64;
    const int it = wv >> 1, ot = wv & 1;
    const int slice = blockIdx.y;
    const int t_row = (lane & 15) >> 2;
    const int t_col = (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;

    // staging = LDS-DMA (no registers, see the implicit-GEMM kernel): a piece is 16 rows x 64 bytes of one channel plane; rows
    // above / below the image fall outside the per-image descriptor (zero fill), columns outside are forced out of range.
    int x_voff[XK], x_lx[XK];
#pragma unroll
    for (int k = 0; k < XK; ++k) {
        const int row = (wv + 4 * k) * 16 + (lane >> 2);
        const int ly = row / PW, lx = row - ly * PW;
        x_voff[k] = ((ly * Wi + lx) * IC) * 2 + (lane & 3) * 16;
        x_lx[k] = row < PH * PW ? lx : 0x40000000;
    }
    const unsigned ximg = (unsigned)Hi * Wi * IC * 2, gimg = (unsigned)Hb * Wb * OC * 2;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // bias gradient (see conv_wgrad_bf16_kernel): the two waves of input tile 0 in the blocks of input-channel tile 0
    const bool bias_wave = with_bias && it == 0 && ic0 == 0;
    bool do_bias = false, bias_next = false;   // per tile: does the tile's source contribute to the bias gradient
    float accb = 0.f;

    // one DMA piece of a tile (q in [0, NPIECE)): patch plane 0 / 1 pieces first, then the gradient planes
    int n_t = 0, by_t = 0, bx_t = 0, ox0_t = 0, xorg_t = 0;
    i32x4 rs_xt = make_rsrc(srcs.x[0], ximg), rs_gt = make_rsrc(srcs.gy[0], gimg);
    auto tile_setup = [&](int tile) __attribute__((always_inline)) {
        int b = tile;
        const int tile_x = b % tiles_x;
        b /= tiles_x;
        const int tile_y = b % tiles_y;
        const int src = wgrad_source(srcs, b / tiles_y, n_t);
        bias_next = bias_wave && ((srcs.bias_mask >> src) & 1u);
        by_t = tile_y * TH;
        bx_t = tile_x * TW;
        const int oy0 = S2 ? 2 * by_t : by_t - 1;
        ox0_t = S2 ? 2 * bx_t : bx_t - 1;
        rs_xt = make_rsrc(reinterpret_cast<const unsigned char*>(srcs.x[src]) + (size_t)n_t * ximg, ximg);
        rs_gt = make_rsrc(reinterpret_cast<const unsigned char*>(srcs.gy[src]) + (size_t)n_t * gimg, gimg);
        xorg_t = ((oy0 * Wi + ox0_t) * IC + ic0) * 2;
    };
    auto issue_piece = [&](int q, int bufi) __attribute__((always_inline)) {
        const unsigned a_x = a_base + bufi * BUF, a_g = a_x + 2 * XPL;
        if (q < 2 * XK) {
            const int k = q >> 1, pl = q & 1;
            unsigned v = (unsigned)(ox0_t + x_lx[k]) < (unsigned)Wi ? (unsigned)(xorg_t + x_voff[k]) : 0x80000000u;
            if (pl && v != 0x80000000u) v += 64;
            lds_dma16(a_x + pl * XPL + (wv + 4 * k) * 1024, v, rs_xt);
        } else {
            const int k = (q - 2 * XK) >> 1, pl = (q - 2 * XK) & 1;
            const int pix = (wv + 4 * k) * 16 + (lane >> 2);
            const int gy_ = by_t + pix / TW, gx_ = bx_t + pix % TW;
            unsigned v = gy_ < Hb && gx_ < Wb ? (unsigned)(((gy_ * Wb + gx_) * OC + oc0) * 2 + (lane & 3) * 16) : 0x80000000u;
            if (pl && v != 0x80000000u) v += 64;
            lds_dma16(a_g + pl * GPL + (wv + 4 * k) * 1024, v, rs_gt);
        }
    };

    // fragments of one 16-pixel group: the gradient columns (2 transposing reads) and, per kernel row, the 3 (stride 1) or
    // 5 (stride 2) reads of the input window.  Two sets: the reads of group g+1 are issued before the MFMAs of group g.
    constexpr int XR = S2 ? 5 : 3;
    constexpr int NG = NP / 16;
    uint2 fb[2][2], fx[2][3][XR];
    // fragment addresses (GS_WG_GROUP_STEP): two 32-channel planes of 64-byte rows per side
    constexpr int XROWB = 64, GROWB = 64;
    auto x_ptr_ = [&](const unsigned char* xpl, int ty, int ky, int txc, int c) __attribute__((always_inline)) {
        return xpl + (((ty * S + ky) * PW + (txc + 8 * hi) * S) + t_row * S + c) * 64 + t_col;
    };
    auto g_ptr_ = [&](const unsigned char* gpl, int ty, int txc) __attribute__((always_inline)) {
        return gpl + (ty * TW + txc + 8 * hi + t_row) * 64 + t_col;
    };
    auto load_group = [&](int g, int fbuf, const unsigned char* xpl, const unsigned char* gpl) __attribute__((always_inline)) {
        const int ty = (g * 16) / TW, txc = (g * 16) % TW;
        const unsigned char* gp = g_ptr_(gpl, ty, txc);
        fb[fbuf][0] = lds_tr16(gp);
        fb[fbuf][1] = lds_tr16(gp + 4 * GROWB);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const unsigned char* xp = x_ptr_(xpl, ty, ky, txc, 0);
            if (!S2) {
                fx[fbuf][ky][0] = lds_tr16(xp); fx[fbuf][ky][1] = lds_tr16(xp + 4 * XROWB); fx[fbuf][ky][2] = lds_tr16(xp + 8 * XROWB);
            } else {
                const unsigned char* xo = x_ptr_(xpl, ty, ky, txc, 1);
                fx[fbuf][ky][0] = lds_tr16(xp); fx[fbuf][ky][1] = lds_tr16(xp + 8 * XROWB); fx[fbuf][ky][2] = lds_tr16(xp + 16 * XROWB);
                fx[fbuf][ky][3] = lds_tr16(xo); fx[fbuf][ky][4] = lds_tr16(xo + 8 * XROWB);
            }
        }
    };

    int buf = 0;
    if (slice < ntiles) {
        tile_setup(slice);
#pragma unroll
        for (int q = 0; q < NPIECE; ++q) issue_piece(q, 0);
    }
    constexpr int PPG = (NPIECE + NG - 1) / NG;   // DMA pieces of the next tile issued per pixel group of this one
    for (int tile = slice; tile < ntiles; tile += nslices) {
        const bool more = tile + nslices < ntiles;
        wait_vmcnt(0);    // this tile has landed (the next one is issued below, under the MFMAs)
        block_barrier();
        do_bias = bias_next;
        if (more) tile_setup(tile + nslices);
        const unsigned char* const xpl = lds_raw + buf * BUF + it * XPL;
        const unsigned char* const gpl = lds_raw + buf * BUF + 2 * XPL + ot * GPL;
        load_group(0, 0, xpl, gpl);
        __builtin_amdgcn_sched_barrier(0);
        static_for<NG>([&](auto gc) __attribute__((always_inline)) { GS_WG_GROUP_STEP(decltype(gc)::value, more, xpl, gpl, buf ^ 1); });
        block_barrier();  // every wave is done with this buffer: the next iteration may overwrite it
        buf ^= 1;
    }
    // ---- D[ic i][oc j], lane = (j = l31, i = (r&3) + 8(r>>2) + 4hi)
    const long pstride = 9L * IC * OC + (with_bias ? OC : 0);
    if (bias_wave) {
        const float tot = swap32_sum(accb);
        if (hi == 0) part[(long)slice * pstride + 9L * IC * OC + oc0 + ot * 32 + l31] = tot;
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* dst = part + (long)slice * pstride + ((long)t * IC + ic0 + it * 32) * OC + oc0 + ot * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(long)((r & 3) + 8 * (r >> 2) + 4 * hi) * OC] = acc[t][r];
    }
}

// The same kernel over a GROUP of layers (conv_shared.h, SkGroup): block b walks the units [b T / nb, (b + 1) T / nb) of the group's
// unit list; the pipeline (DMA of unit u+1 under the MFMAs of unit u) runs straight across run and layer boundaries -- the MFMA
// side only sees staged LDS tiles, whatever layer they came from -- and the accumulators are flushed to partial `b + run` where the
// block's range leaves a run.  Always 32-wide tiles: a 16-wide image leaves half of a tile's columns empty either way (a 2 x 16 image fills
// 1/8 of a 16 x 16 tile and 1/8 of an 8 x 32 one), and with one width all layers of a conv mode share ONE group.
template <int MODE>
__global__ __launch_bounds__(256) void conv_wgrad_bf16_2x2_sk_kernel(const SkGroup g, float* __restrict__ part) {
    constexpr bool S2 = MODE == MODE_S2;
    constexpr int TW = 32;
    constexpr int NP = S2 ? 64 : 256;
    constexpr int TH = NP / TW;
    constexpr int PH = patch_dim<MODE>(TH), PW = patch_dim<MODE>(TW);
    constexpr int S = S2 ? 2 : 1;
    // Staged layout: ONE plane per side with 128-byte rows = all 64 channels of a pixel, a DMA piece = 8 whole rows, i.e. whole 128-byte
    // cache lines (scripts/probe/dma_rate.hip); a unit's time IS the issuing wave's serial sum -- MFMAs + ~13 cycles per transposing read
    // + the DMA issue (model and counters: DESIGN.md 6.4).  The 32-channel half h of row r sits at (h ^ (r >> 1 & 1)) * 64, applied on
    // the DMA's source side, so that the four rows of a transposing read (r .. r + 3) cover all 64 banks as 64-byte rows would.
    constexpr int XRG = (PH * PW + 7) / 8;      // DMA pieces (1 KiB) of the patch
    constexpr int GRG = NP / 8;
    constexpr int XK = (XRG + 3) / 4, GK = GRG / 4;
    constexpr int XT = XK * 4096, GT = NP * 128;   // bytes of the staged patch / gradient tile
    constexpr int BUF = XT + GT;
    constexpr int NPIECE = XK + GK;
    constexpr int XROWB = 128, GROWB = XROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const unsigned a_base = (unsigned)(uintptr_t)lds_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;   // (& 3: a block has 4 waves -- the compiler folds the bounds tests of whole pieces with it)
    const int it = wv >> 1, ot = wv & 1;
    const int t_row = (lane & 15) >> 2;
    const int t_col = (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;
    const long nb = gridDim.x, total = g.total_units;
    const int U0 = (int)((blockIdx.x * total) / nb), U1 = (int)(((blockIdx.x + 1) * total) / nb);
    if (U0 >= U1) return;

    // ---- DMA side: the unit being staged (one ahead of the one being multiplied)
    constexpr int RPP = 8;              // rows per piece
    const int p_row = lane >> 3;        // row of the piece this lane fetches 16 bytes of
    int x_ly[XK], x_lx[XK], x_voff[XK], x_sw[XK];
#pragma unroll
    for (int k = 0; k < XK; ++k) {
        const int row = (wv + 4 * k) * RPP + p_row;
        x_ly[k] = row / PW;
        x_lx[k] = row - x_ly[k] * PW;
        x_voff[k] = 0;
        x_sw[k] = ((lane & 7) ^ (((row >> 1) & 1) << 2)) * 16;   // source bytes of the lane's 16-byte slot within the channel row
    }
    int j_n = 0, ct_n = 0, tile_n = 0;                               // layer, channel tile, pixel tile
    int Hi = 0, Wi = 0, IC = 0, OC = 0, Hb = 0, Wb = 0, tiles_x = 1, tiles_y = 1, ntiles = 1, n_ict = 1, nct = 1;
    unsigned ximg = 0, gimg = 0;
    int ic0_n = 0, oc0_n = 0, run_n = 0;
    bool bias_wave_n = false;
    auto load_job = [&](int j) __attribute__((always_inline)) {
        const SkJob& q = g.job[j];
        Hi = q.Hi; Wi = q.Wi; IC = q.IC; OC = q.OC; Hb = q.Hb; Wb = q.Wb;
        tiles_x = q.tiles_x; tiles_y = q.tiles_y; ntiles = q.ntiles; n_ict = q.n_ict; nct = q.nct;
        ximg = (unsigned)Hi * Wi * IC * 2;
        gimg = (unsigned)Hb * Wb * OC * 2;
#pragma unroll
        for (int k = 0; k < XK; ++k) x_voff[k] = ((x_ly[k] * Wi + x_lx[k]) * IC) * 2 + x_sw[k];
    };
    auto set_ct = [&](int j, int ct) __attribute__((always_inline)) {
        ic0_n = (ct % n_ict) * 64;
        oc0_n = (ct / n_ict) * 64;
        run_n = g.job[j].run_base + ct;
        bias_wave_n = g.job[j].gb != nullptr && it == 0 && ic0_n == 0;
    };
    int n_t = 0, by_t = 0, bx_t = 0, ox0_t = 0, xorg_t = 0;
    bool bias_next = false;
    i32x4 rs_xt = make_rsrc(g.job[0].srcs.x[0], 0), rs_gt = rs_xt;
    // pixel-tile coordinates of the unit being staged, advanced incrementally (three runtime divisions per unit cost more issue
    // slots than a group of MFMAs leaves)
    int tx_n = 0, ty_n = 0, img_n = 0;
    auto tile_setup = [&](int j) __attribute__((always_inline)) {
        const SkJob& q = g.job[j];
        const int src = wgrad_source(q.srcs, img_n, n_t);
        bias_next = bias_wave_n && ((q.srcs.bias_mask >> src) & 1u);
        by_t = ty_n * TH;
        bx_t = tx_n * TW;
        const int oy0 = S2 ? 2 * by_t : by_t - 1;
        ox0_t = S2 ? 2 * bx_t : bx_t - 1;
        rs_xt = make_rsrc(reinterpret_cast<const unsigned char*>(q.srcs.x[src]) + (size_t)n_t * ximg, ximg);
        rs_gt = make_rsrc(reinterpret_cast<const unsigned char*>(q.srcs.gy[src]) + (size_t)n_t * gimg, gimg);
        xorg_t = ((oy0 * Wi + ox0_t) * IC + ic0_n) * 2;
    };
    auto issue_piece = [&](int q, int bufi) __attribute__((always_inline)) {
        const unsigned a_x = a_base + bufi * BUF, a_g = a_x + XT;
        if (q < XK) {
            const int k = q;
            const bool in = (wv + 4 * k) * 8 + p_row < PH * PW && (unsigned)(ox0_t + x_lx[k]) < (unsigned)Wi;
            const unsigned v = in ? (unsigned)(xorg_t + x_voff[k]) : 0x80000000u;
            lds_dma16(__builtin_amdgcn_readfirstlane(a_x + (wv + 4 * k) * 1024), v, rs_xt);
        } else {
            const int k = q - XK;
            const int pix = (wv + 4 * k) * 8 + p_row;
            const int gy_ = by_t + pix / TW, gx_ = bx_t + pix % TW;
            const bool in = gy_ < Hb && gx_ < Wb;
            const unsigned v = in ? (unsigned)(((gy_ * Wb + gx_) * OC + oc0_n) * 2 + (((lane & 7) ^ (((pix >> 1) & 1) << 2)) * 16)) : 0x80000000u;
            lds_dma16(__builtin_amdgcn_readfirstlane(a_g + (wv + 4 * k) * 1024), v, rs_gt);
        }
    };

    // ---- MFMA side (as conv_wgrad_bf16_2x2_kernel)
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float accb = 0.f;
    bool do_bias = false;
    constexpr int XR = S2 ? 5 : 3;
    constexpr int NG = NP / 16;
    uint2 fb[2][2], fx[2][3][XR];
    // fragment addresses (GS_WG_GROUP_STEP): row r of the tile at r * 128, this wave's 32-channel half at ((half ^ bit 1 of r) << 6).
    // Bit 1 of the row a lane reads is (a compile-time bit of the group / kernel row / column parity) ^ (a bit of t_row): everything that
    // depends on the lane is folded into two offsets per side, the rest into the instruction's immediate offset.
    //   stride 1: r = (ty + ky) PW + txc + 8 hi + t_row (+ 4 k),  PW = 34:  bit 1 = ((ty + ky) & 1) ^ (t_row >> 1)
    //   stride 2: r = (2 ty + ky) PW + 2 txc + 16 hi + 2 t_row + c (+ 8 k),  PW = 65:  bit 1 = (((2 ty + ky + c) >> 1) & 1) ^ (t_row & 1)
    //   gradient: r = ty TW + txc + 8 hi + t_row (+ 4 i):  bit 1 = t_row >> 1
    static_assert(S2 ? PW % 4 == 1 : PW % 4 == 2, "the swizzle algebra below assumes PW = 34 (stride 1) / 65 (stride 2)");
    const int xl_base = (t_row * S + 8 * S * hi) * 128 + t_col;
    const int xl_sw = S2 ? (t_row & 1) : (t_row >> 1);
    const int xlane[2] = {xl_base + (((it ^ xl_sw) & 1) << 6), xl_base + (((it ^ xl_sw ^ 1) & 1) << 6)};
    const int glane = (t_row + 8 * hi) * 128 + t_col + (((ot ^ (t_row >> 1)) & 1) << 6);
    auto x_ptr_ = [&](const unsigned char* xt, int ty, int ky, int txc, int c) __attribute__((always_inline)) {
        const int a = S2 ? ((2 * ty + ky + c) >> 1) & 1 : (ty + ky) & 1;
        return xt + ((ty * S + ky) * PW + txc * S + c) * 128 + xlane[a];
    };
    auto g_ptr_ = [&](const unsigned char* gt, int ty, int txc) __attribute__((always_inline)) {
        return gt + (ty * TW + txc) * 128 + glane;
    };
    auto load_group = [&](int gi, int fbuf, const unsigned char* xt, const unsigned char* gt) __attribute__((always_inline)) {
        const int ty = (gi * 16) / TW, txc = (gi * 16) % TW;
        const unsigned char* gp = g_ptr_(gt, ty, txc);
        fb[fbuf][0] = lds_tr16(gp);
        fb[fbuf][1] = lds_tr16(gp + 4 * GROWB);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const unsigned char* xp = x_ptr_(xt, ty, ky, txc, 0);
            if (!S2) {
                fx[fbuf][ky][0] = lds_tr16(xp); fx[fbuf][ky][1] = lds_tr16(xp + 4 * XROWB); fx[fbuf][ky][2] = lds_tr16(xp + 8 * XROWB);
            } else {
                const unsigned char* xo = x_ptr_(xt, ty, ky, txc, 1);
                fx[fbuf][ky][0] = lds_tr16(xp); fx[fbuf][ky][1] = lds_tr16(xp + 8 * XROWB); fx[fbuf][ky][2] = lds_tr16(xp + 16 * XROWB);
                fx[fbuf][ky][3] = lds_tr16(xo); fx[fbuf][ky][4] = lds_tr16(xo + 8 * XROWB);
            }
        }
    };

    // ---- first unit of the block
    while (j_n + 1 < g.njobs && U0 >= g.job[j_n + 1].unit_base) ++j_n;
    load_job(j_n);
    ct_n = (U0 - g.job[j_n].unit_base) / ntiles;
    tile_n = (U0 - g.job[j_n].unit_base) - ct_n * ntiles;
    tx_n = tile_n % tiles_x;
    ty_n = (tile_n / tiles_x) % tiles_y;
    img_n = tile_n / (tiles_x * tiles_y);
    set_ct(j_n, ct_n);
    tile_setup(j_n);
#pragma unroll
    for (int q = 0; q < NPIECE; ++q) issue_piece(q, 0);

    // DMA pieces of the next unit per pixel group of this one.  FRONT = k > 0: all of them within the first k groups, so that
    // the last piece issued has the remaining groups' MFMAs between it and the wait at the top of the next unit (a piece issued in the
    // last group meets that wait ~300 cycles later and the unit pays its whole L2 / HBM latency: SQ_WAIT_ANY 45 % of the stride-2 kernel's
    // wave cycles, profiles/r04_a_wgrad_group_sq_pmc.txt).  Stride 2 fronts them into the first group (flush 131 -> 121 / 183 -> 167 us at
    // 16 / 24 images, profiles/r04_c_ab_wgrad_front.txt); stride 1 spreads them over all groups (no change at 4 or 8).
    constexpr int FRONT_S1 = 0, FRONT_S2 = 1;
    constexpr int FRONT = S2 ? FRONT_S2 : FRONT_S1;
    constexpr int PPG = FRONT > 0 ? (NPIECE + FRONT - 1) / FRONT : (NPIECE + NG - 1) / NG;
    int buf = 0;
    for (int u = U0; u < U1; ++u) {
        const bool more = u + 1 < U1;
        wait_vmcnt(0);
        block_barrier();
        // the unit being multiplied: what the DMA side was set to when it was issued
        do_bias = bias_next;
        const int run_c = run_n;
        const bool bias_wave_c = bias_wave_n;
        bool leave = !more;   // does the block's range leave the run after this unit?
        if (more) {
            if (++tx_n == tiles_x) {
                tx_n = 0;
                if (++ty_n == tiles_y) { ty_n = 0; ++img_n; }
            }
            if (++tile_n == ntiles) {
                tile_n = 0;
                tx_n = ty_n = img_n = 0;
                leave = true;
                if (++ct_n == nct) { ct_n = 0; ++j_n; load_job(j_n); }
                set_ct(j_n, ct_n);
            }
            tile_setup(j_n);
        }
        const unsigned char* const xpl = lds_raw + buf * BUF;          // the staged patch / gradient tile (x_ptr_ / g_ptr_ pick this wave's half)
        const unsigned char* const gpl = lds_raw + buf * BUF + XT;
        load_group(0, 0, xpl, gpl);
        __builtin_amdgcn_sched_barrier(0);
        static_for<NG>([&](auto gc) __attribute__((always_inline)) { GS_WG_GROUP_STEP(decltype(gc)::value, more, xpl, gpl, buf ^ 1); });
        block_barrier();
        buf ^= 1;
        if (leave) {   // partial (block + run): [tap][ic 64][oc 64] + 64 bias sums; lane = (oc j = l31, ic i = (r&3) + 8(r>>2) + 4hi)
            float* const dst0 = part + (long)(blockIdx.x + run_c) * GS_SK_PSTRIDE;
            if (bias_wave_c) {
                const float tot = swap32_sum(accb);
                if (hi == 0) dst0[9 * 4096 + ot * 32 + l31] = tot;
            }
            accb = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                float* dst = dst0 + (t * 64 + it * 32) * 64 + ot * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dst[((r & 3) + 8 * (r >> 2) + 4 * hi) * 64] = acc[t][r];
                    acc[t][r] = 0.f;
                }
            }
        }
    }
}

// folds the partials of every run of a group into the gradients: grid (145, runs); block = 64 consecutive quads of the partial
// (1 KiB per partial: whole DRAM bursts) x 4 partial lanes, a thread keeps four partials in flight; fixed order -> deterministic
__global__ __launch_bounds__(256) void wgrad_sk_reduce_kernel(const SkGroup g, const float* __restrict__ part) {
    constexpr int L = 4, EPB = 64;
    __shared__ float4 red[256];
    const int r = blockIdx.y;
    int j = 0;
    while (j + 1 < g.njobs && r >= g.job[j + 1].run_base) ++j;
    const SkJob& q = g.job[j];
    const int ct = r - q.run_base;
    const int ic0 = (ct % q.n_ict) * 64, oc0 = (ct / q.n_ict) * 64;
    const long s0 = (long)q.unit_base + (long)ct * q.ntiles;
    const int b0 = sk_block_of(s0, g.nblocks, g.total_units), b1 = sk_block_of(s0 + q.ntiles - 1, g.nblocks, g.total_units);
    const int e = blockIdx.x * EPB + (threadIdx.x % EPB);   // quad index inside the partial
    const int sl = threadIdx.x / EPB;
    const bool live = e < GS_SK_PSTRIDE / 4;
    const bool is_bias = e >= 9 * 1024;
    if (blockIdx.x * EPB >= 9 * 1024 && !(q.gb && ic0 == 0)) return;   // (the bias quads are the last, whole block)
    const float* const base = part + (long)r * GS_SK_PSTRIDE + (long)e * 4;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    if (live) {
        int b = b0 + sl;
        for (; b + 3 * L <= b1; b += 4 * L) {
            const float4 v0 = *reinterpret_cast<const float4*>(base + (long)b * GS_SK_PSTRIDE);
            const float4 v1 = *reinterpret_cast<const float4*>(base + (long)(b + L) * GS_SK_PSTRIDE);
            const float4 v2 = *reinterpret_cast<const float4*>(base + (long)(b + 2 * L) * GS_SK_PSTRIDE);
            const float4 v3 = *reinterpret_cast<const float4*>(base + (long)(b + 3 * L) * GS_SK_PSTRIDE);
            a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
            a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
            a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
            a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
        }
        for (; b <= b1; b += L) {
            const float4 v0 = *reinterpret_cast<const float4*>(base + (long)b * GS_SK_PSTRIDE);
            a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        }
    }
    a0.x += a2.x; a0.y += a2.y; a0.z += a2.z; a0.w += a2.w;
    a1.x += a3.x; a1.y += a3.y; a1.z += a3.z; a1.w += a3.w;
    red[threadIdx.x] = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
    __syncthreads();
    if (sl != 0 || !live) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const float4 v = red[threadIdx.x + k * EPB];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (is_bias) {
        if (!(q.gb && ic0 == 0)) return;
        float4* o = reinterpret_cast<float4*>(q.gb + oc0 + (e - 9 * 1024) * 4);
        const float4 old = q.accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
        *o = make_float4(old.x + s.x, old.y + s.y, old.z + s.z, old.w + s.w);
        return;
    }
    const int t = e >> 10, i = (e >> 4) & 63, j4 = (e & 15) * 4;
    const float al = q.alpha;
    if (!q.transpose) {
        float4* o = reinterpret_cast<float4*>(q.gw + ((long)t * q.ICld + ic0 + i) * q.OC + oc0 + j4);
        const float4 old = q.accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
        *o = make_float4(old.x + s.x * al, old.y + s.y * al, old.z + s.z * al, old.w + s.w * al);
    } else {
        const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float* o = q.gw + ((long)t * q.OC + oc0 + j4 + c) * q.IC + ic0 + i;
            *o = q.accumulate ? *o + v[c] * al : v[c] * al;
        }
    }
}

// ---------------------------------------------------------------------- slice reductions
// gw[e] = alpha * sum_s part[s][e]; `transpose` swaps the last two dims on output
// (used by conv2d_transpose's weight gradient, whose stored variable is [k][k][Cin_T][Cout_T]).
// Block = (256 / L) consecutive elements x L slice lanes; one launch whatever the slice count (L = 4 for a few slices,
// 16 for the hundreds of slices of the thin top-of-pyramid layers); fixed summation order -> deterministic.
template <int L>
static __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, float* __restrict__ gb, int nslices,
                                                                  int taps, int ic, int oc, float alpha, int transpose, int accumulate) {
    // a thread sums 4 consecutive elements (one 16-byte load per slice) over its share of the slices; EPB element quads per block
    constexpr int EPB = 256 / L;
    __shared__ float4 red[256];
    const long total = (long)taps * ic * oc;
    const long pstride = total + (gb ? oc : 0);   // a slice = the taps (+ one row of bias sums when gb is given); multiple of 4
    const long e = ((long)blockIdx.x * EPB + (threadIdx.x % EPB)) * 4;
    const int sl = threadIdx.x / EPB;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    if (e < pstride) {
        int k = sl;
        // eight slices per trip, all eight loads in flight together (the thin colour-block gradients fold 1024 slices of 64 floats in ONE
        // block: with two loads per trip that was 32 dependent round trips, 12 us)
        for (; k + 7 * L < nslices; k += 8 * L) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float4*>(part + (long)(k + j * L) * pstride + e);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                s0.x += v[j].x; s0.y += v[j].y; s0.z += v[j].z; s0.w += v[j].w;
                s1.x += v[j + 1].x; s1.y += v[j + 1].y; s1.z += v[j + 1].z; s1.w += v[j + 1].w;
            }
        }
        for (; k + L < nslices; k += 2 * L) {
            const float4 a = *reinterpret_cast<const float4*>(part + (long)k * pstride + e);
            const float4 b = *reinterpret_cast<const float4*>(part + (long)(k + L) * pstride + e);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
            s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
        }
        if (k < nslices) {
            const float4 a = *reinterpret_cast<const float4*>(part + (long)k * pstride + e);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
        }
    }
    red[threadIdx.x] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
    __syncthreads();
    if (sl == 0 && e < pstride) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const float4 v = red[threadIdx.x + j * EPB];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        const float s[4] = {t.x, t.y, t.z, t.w};
        if (e >= total) {   // bias gradient: no equalized-LR scale
            float4* o = reinterpret_cast<float4*>(gb + (e - total));
            const float4 old = accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
            *o = make_float4(old.x + s[0], old.y + s[1], old.z + s[2], old.w + s[3]);
            return;
        }
        if (!transpose) {
            float4* o = reinterpret_cast<float4*>(gw + e);
            const float4 old = accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
            *o = make_float4(old.x + s[0] * alpha, old.y + s[1] * alpha, old.z + s[2] * alpha, old.w + s[3] * alpha);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long ee = e + c;
                const int o = ee % oc;
                const int i = (ee / oc) % ic;
                const int tp = ee / ((long)ic * oc);
                const long dst = ((long)tp * oc + o) * ic + i;
                gw[dst] = accumulate ? gw[dst] + s[c] * alpha : s[c] * alpha;
            }
        }
    }
}

// element counts that are not a multiple of 4 (odd channel counts of the direct kernels): one element per thread
static __global__ __launch_bounds__(256) void wgrad_reduce_scalar_kernel(const float* __restrict__ part, float* __restrict__ gw, int nslices, int taps, int ic,
                                                                         int oc, float alpha, int transpose, int accumulate) {
    const long total = (long)taps * ic * oc;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = 0.f;
    for (int k = 0; k < nslices; ++k) s += part[(long)k * total + e];
    s *= alpha;
    long dst = e;
    if (transpose) {
        const int o = e % oc;
        const int i = (e / oc) % ic;
        const int t = e / ((long)ic * oc);
        dst = ((long)t * oc + o) * ic + i;
    }
    gw[dst] = accumulate ? gw[dst] + s : s;
}

// Many reductions per launch (ReduceBatch, conv_shared.h).
// L = 4: block = 64 consecutive element quads (1 KiB per slice row: whole DRAM bursts) x 4 slice lanes; L = 16: 16 quads x 16 slice lanes
// (the thin top-level layers leave 256 slices of 18 K floats each: with 4 slice lanes that is 72 blocks per entry walking 64 slices per
// thread, four loads in flight -- 32-37 us for 19 MB; 16 lanes put four times the loads in flight on four times the blocks).  A thread keeps
// four slice rows in flight.
// The lane count is a function of the ENTRY (its slice count), never of what else shares the launch: the association of an entry's sum must
// not depend on how the caller batches the folds (a bucketed flush batches them differently, and two schedules of one iteration must agree).
static __global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const ReduceBatch b) {
    const GsWgradReduce& d = b.e[blockIdx.y];
    const int nslices = d.nslices, oc = d.oc, ic = d.ic;
    const int L = nslices > 32 ? 16 : 4, EPB = 256 / L;
    __shared__ float4 red[256];
    const long total = (long)d.taps * ic * oc;
    const long pstride = total + (d.gb ? oc : 0);
    const long e = ((long)blockIdx.x * EPB + (threadIdx.x % EPB)) * 4;
    if ((long)blockIdx.x * EPB * 4 >= pstride) return;   // (whole block past the end of this entry)
    const int sl = threadIdx.x / EPB;
    const float* __restrict__ part = d.partials;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
    if (e < pstride) {
        int k = sl;
        for (; k + 3 * L < nslices; k += 4 * L) {
            const float4 a0 = *reinterpret_cast<const float4*>(part + (long)k * pstride + e);
            const float4 a1 = *reinterpret_cast<const float4*>(part + (long)(k + L) * pstride + e);
            const float4 a2 = *reinterpret_cast<const float4*>(part + (long)(k + 2 * L) * pstride + e);
            const float4 a3 = *reinterpret_cast<const float4*>(part + (long)(k + 3 * L) * pstride + e);
            s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
            s1.x += a1.x; s1.y += a1.y; s1.z += a1.z; s1.w += a1.w;
            s2.x += a2.x; s2.y += a2.y; s2.z += a2.z; s2.w += a2.w;
            s3.x += a3.x; s3.y += a3.y; s3.z += a3.z; s3.w += a3.w;
        }
        for (; k < nslices; k += L) {
            const float4 a = *reinterpret_cast<const float4*>(part + (long)k * pstride + e);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
        }
    }
    s0.x += s2.x; s0.y += s2.y; s0.z += s2.z; s0.w += s2.w;
    s1.x += s3.x; s1.y += s3.y; s1.z += s3.z; s1.w += s3.w;
    red[threadIdx.x] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
    __syncthreads();
    if (sl != 0 || e >= pstride) return;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < L; ++j) {
        const float4 v = red[threadIdx.x + j * EPB];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    const float s[4] = {t.x, t.y, t.z, t.w};
    const int accumulate = d.accumulate;
    if (e >= total) {   // bias gradient: no equalized-LR scale
        float4* o = reinterpret_cast<float4*>(d.gb + (e - total));
        const float4 old = accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
        *o = make_float4(old.x + s[0], old.y + s[1], old.z + s[2], old.w + s[3]);
        return;
    }
    const float alpha = d.alpha;
    float* __restrict__ gw = d.gw;
    if (!d.transpose) {
        long dst = e;
        if (d.ic_ld > ic) {   // channel slice of a wider variable: tap t starts at t * ic_ld * oc (a quad never straddles taps: ic * oc % 4 == 0)
            const long per_tap = (long)ic * oc;
            const long tp = e / per_tap;
            dst = tp * d.ic_ld * oc + (e - tp * per_tap);
        }
        float4* o = reinterpret_cast<float4*>(gw + dst);
        const float4 old = accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
        *o = make_float4(old.x + s[0] * alpha, old.y + s[1] * alpha, old.z + s[2] * alpha, old.w + s[3] * alpha);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long ee = e + c;
            const int o = ee % oc;
            const int i = (ee / oc) % ic;
            const int tp = ee / ((long)ic * oc);
            const long dst = ((long)tp * oc + o) * ic + i;
            gw[dst] = accumulate ? gw[dst] + s[c] * alpha : s[c] * alpha;
        }
    }
}

void wgrad_reduce_launch(float* part, float* gw, float* gb, int nslices, int taps, int ic, int oc, float alpha, int transpose, int accumulate, hipStream_t st,
                         GsWgradReduce* defer) {
    const bool vec = !((((long)taps * ic * oc) & 3) != 0 || (gb && (oc & 3) != 0));
    if (defer && vec) {   // phase 2 is left to wgrad_reduce_batch
        defer->partials = part; defer->gw = gw; defer->gb = gb;
        defer->nslices = nslices; defer->taps = taps; defer->ic = ic; defer->oc = oc;
        defer->alpha = alpha; defer->transpose = transpose; defer->accumulate = accumulate; defer->ic_ld = 0;
        return;
    }
    if (!vec) {
        const long total = (long)taps * ic * oc;   // (gb never comes with such shapes: the fused bias path needs oc % 32 == 0)
        hipLaunchKernelGGL(wgrad_reduce_scalar_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, gw, nslices, taps, ic, oc, alpha, transpose, accumulate);
        return;
    }
    const long n4 = ((long)taps * ic * oc + (gb ? oc : 0)) / 4;   // element quads
    if (wgrad_fold_lanes(nslices) == 4) {
        hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3((unsigned)((n4 + 63) / 64)), dim3(256), 0, st, part, gw, gb, nslices, taps, ic, oc, alpha, transpose, accumulate);
    } else {
        hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3((unsigned)((n4 + 15) / 16)), dim3(256), 0, st, part, gw, gb, nslices, taps, ic, oc, alpha, transpose, accumulate);
    }
}
void wgrad_reduce_batch_launch(const ReduceBatch& b, int count, long blocks_x, hipStream_t st) {
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)blocks_x, (unsigned)count), dim3(256), 0, st, b);
}

// ------------------------------------------------------------------------------ dispatch

// weight-gradient launches sized for fewer CUs than the chip has (0: all): what runs beside a latency-bound chain on a forked branch of
// the run's hipGraph leaves that chain's few blocks somewhere to land (gs_wgrad_cu_cap; models.GANSynth._early_flush)
static int g_wgrad_cu_cap = 0;
static int wgrad_cus() {
    const int n = num_cus();
    return g_wgrad_cu_cap > 0 && g_wgrad_cu_cap < n ? g_wgrad_cu_cap : n;
}

static bool wgrad_mfma_supported(int ic, int oc, int dtype) { return (dtype == GS_F32 || dtype == GS_BF16) && ic % 32 == 0 && oc % 32 == 0; }

static int patch_dim_rt(int mode, int t) { return mode == MODE_S1 ? t + 2 : (mode == MODE_S2 ? 2 * t + 1 : t + 1); }
// ---- weight gradient (fp32 MFMA path)
static bool wgrad_2x2(int mode, int dtype, int IC, int OC) { (void)mode; return dtype == GS_BF16 && IC % 64 == 0 && OC % 64 == 0; }
// thin bf16 layers whose output side has a multiple of 64 channels: 32 x 64 pairs per block (conv_wgrad_bf16_kernel<.., 2>)
static bool wgrad_thin_pairs(int mode, int dtype, int IC, int OC) {
    static const bool off = getenv("GS_NO_THIN_PAIRS") != nullptr;   // measurement knob
    return !off && dtype == GS_BF16 && !wgrad_2x2(mode, dtype, IC, OC) && OC % 64 == 0;
}
// the 32-input-channel bf16 layers (HBM-bound top of the pyramid): LDS-DMA staged, wave-specialised kernel (conv_wgrad_bf16_thin_dma_kernel)
static bool wgrad_thin_dma(int mode, int dtype, int IC, int OC, int Wb) {
    static const bool off = getenv("GS_NO_THIN_DMA") != nullptr;   // measurement knob: back to conv_wgrad_bf16_kernel
    (void)mode;
    return !off && dtype == GS_BF16 && IC == 32 && (OC == 32 || OC == 64) && Wb >= 32;
}
// the 1 x 1 colour layers (2 channels on one side): thin_wgrad_kernel below
static bool thin_wgrad_ok(int ks, int ci, int co) {
    if (ks != 1) return false;
    const int c = ci == 2 ? co : (co == 2 ? ci : 0);
    return c >= 4 && c <= 1024 && (c & 3) == 0 && 256 % (c >> 2) == 0 && !(ci == 2 && co == 2);
}
static void thin_wgrad_geometry(long npix, int c, int* nslices, long* pps) {
    const long rpi = 256 / (c >> 2);
    long ns = (npix + rpi * 32 - 1) / (rpi * 32);
    if (ns > 1024) ns = 1024;
    if (ns < 1) ns = 1;
    *pps = (npix + ns - 1) / ns;
    *nslices = (int)((npix + *pps - 1) / *pps);
}
static void wgrad_direct_geometry(long npix, int* nslices, long* pps) {
    long ns = (npix + 63) / 64;   // a thread walks its slice serially (index arithmetic + two dependent loads per pixel): keep it short
    if (ns > 1024) ns = 1024;
    if (ns < 1) ns = 1;
    *pps = (npix + ns - 1) / ns;
    *nslices = (int)((npix + *pps - 1) / *pps);
}

// THE selection (conv_shared.h: WgradPlan) for a kernel-role shape; N = images of all sources
WgradPlan wgrad_plan(int mode, int ks, int dtype, int N, int Hb, int Wb, int IC, int OC) {
    WgradPlan p;
    memset(&p, 0, sizeof(p));
    p.mode = mode;
    const long elems = (long)ks * ks * IC * OC;
    if (!(ks == 3 && wgrad_mfma_supported(IC, OC, dtype))) {
        const long npix = (long)N * Hb * Wb;
        p.ntiles = (int)npix;
        if (thin_wgrad_ok(ks, IC, OC) && mode == MODE_S1) {
            p.family = WG_THIN;
            p.ot = IC == 2 ? 0 : 1;
            thin_wgrad_geometry(npix, IC == 2 ? OC : IC, &p.nslices, &p.pps);
            long dpps;   // (the workspace of a colour layer holds the direct kernel's partials as well, should they be more)
            wgrad_direct_geometry(npix, &p.ws_slices, &dpps);
        } else {
            p.family = WG_DIRECT;
            wgrad_direct_geometry(npix, &p.nslices, &p.pps);
        }
    } else {
        p.fused_bias = dtype == GS_BF16;   // the bf16 kernels produce the bias gradient on the side
        int np = (mode == MODE_S2 ? 64 : 128) * (dtype == GS_BF16 ? 2 : 1);
        if (wgrad_thin_dma(mode, dtype, IC, OC, Wb)) {   // 256-pixel tiles, 64 at stride 2; two double-buffered blocks per CU
            p.family = WG_THIN_DMA;
            p.ot = OC / 32;
            np = mode == MODE_S2 ? 64 : 256;
            p.tw = 32;
            const int th = np / 32;
            p.tiles_x = cdiv(Wb, 32);
            p.tiles_y = cdiv(Hb, th);
            p.ntiles = N * p.tiles_x * p.tiles_y;
            const int lds = 2 * (((patch_dim_rt(mode, th) * patch_dim_rt(mode, 32) + 15) / 16) * 1024 + (OC / 32) * np * 64);
            int per_cu = (160 * 1024) / lds;
            if (per_cu > 2) per_cu = 2;
            if (per_cu < 1) per_cu = 1;
            int ns = per_cu * wgrad_cus();
            if (ns > p.ntiles) ns = p.ntiles;
            p.nslices = ns;
        } else {
            int pairs = (IC / 32) * (OC / 32);
            int target = dtype == GS_BF16 ? 768 : 512;
            if (dtype == GS_F32) {
                p.family = WG_F32;
                p.ot = 1;
            } else if (wgrad_2x2(mode, dtype, IC, OC)) {   // 64 x 64 tiles, double-buffered: one block of 4 waves per CU
                p.family = WG_TILE64;
                p.ot = 2;
                if (mode == MODE_S2) np = 64;
                pairs /= 4;
                target = 256;
            } else {
                p.family = WG_BF16;
                p.ot = wgrad_thin_pairs(mode, dtype, IC, OC) ? 2 : 1;
                pairs /= p.ot;
            }
            p.tw = Wb >= 32 ? 32 : 16;
            const int th = np / p.tw;
            p.tiles_x = cdiv(Wb, p.tw);
            p.tiles_y = cdiv(Hb, th);
            p.ntiles = N * p.tiles_x * p.tiles_y;
            int ns = target / pairs;
            if (ns < 1) ns = 1;
            if (ns > p.ntiles) ns = p.ntiles;
            p.nslices = ns;
        }
    }
    if (p.ws_slices < p.nslices) p.ws_slices = p.nslices;
    const bool vec = (elems & 3) == 0;   // (a bias row comes with oc % 32 == 0 only)
    p.fold = vec ? wgrad_fold_lanes(p.nslices) : 0;
    p.batch_lanes = p.fold;
    return p;
}

// ------------------------------------------------------------------ direct weight gradient (the layers outside the MFMA kernels: WG_DIRECT / WG_THIN)
// part[slice][t][ic][oc] = sum over the slice's output pixels of x[in(p,t)][ic] * gy[p][oc]
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_direct_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                                                                float* __restrict__ part, int mode, int ks, int N, int Hi,
                                                                int Wi, int IC, int OC, int Hb, int Wb, long E, long npix,
                                                                long pps) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const long e = (long)blockIdx.x * 64 + (tid & 63);
    const int sub = tid >> 6;
    const int slice = blockIdx.y;
    float acc = 0.f;
    if (e < E) {
        const int oc = e % OC;
        const int ic = (e / OC) % IC;
        const int t = e / ((long)IC * OC);
        const int ky = t / ks, kx = t % ks;
        const long p0 = (long)slice * pps;
        long p1 = p0 + pps;
        if (p1 > npix) p1 = npix;
        // (branch-free body, clamped addresses: unrolled, the loads of four pixels are in flight together -- with a `continue` per pixel the
        //  loop was a chain of dependent load pairs: 10 us for the 256 pixels of the stddev-plane conv at 2 x 16)
#pragma unroll 4
        for (long p = p0 + sub; p < p1; p += 4) {
            const int px = (int)(p % Wb);
            const long q = p / Wb;
            const int py = (int)(q % Hb);
            const int n = (int)(q / Hb);
            int iy, ix;
            if (mode == MODE_S1) { iy = py + ky - (ks >> 1); ix = px + kx - (ks >> 1); }
            else { iy = 2 * py + ky; ix = 2 * px + kx; }
            const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
            const float xv = DT<T>::ld(x + (((long)n * Hi + (ok ? iy : 0)) * Wi + (ok ? ix : 0)) * IC + ic);
            const float gv = DT<T>::ld(gy + p * OC + oc);
            acc += ok ? xv * gv : 0.f;
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (sub == 0 && e < E) part[(long)slice * E + e] = red[tid] + red[tid + 64] + red[tid + 128] + red[tid + 192];
}

// ------------------------------------------------------------- thin 1x1 weight gradient
// The colour convs have 2 channels on one side: gw = sum_p wide[p][C] (x) thin[p][2].  One streaming pass:
// C/4 lanes per pixel hold 4 wide channels x 2 thin values = 8 accumulators, pixel lanes reduce through LDS.
// WIDE_IS_X: x is the wide tensor (gw[c][j], Cout = 2), else gy is (gw[j][c], Cin = 2).
template <typename T, bool WIDE_IS_X>
__global__ __launch_bounds__(256) void thin_wgrad_kernel(const T* __restrict__ wide, const T* __restrict__ thin, float* __restrict__ part,
                                                         int C, long npix, long pps) {
    __shared__ float red[256 * 8];
    const int quads = C >> 2;
    const int rpi = 256 / quads;  // pixel lanes per iteration
    const int q = threadIdx.x % quads, r = threadIdx.x / quads;
    const long p0 = (long)blockIdx.x * pps;
    long p1 = p0 + pps;
    if (p1 > npix) p1 = npix;
    float acc[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    if (r < rpi) {
        long p = p0 + r;
        for (; p + 3 * rpi < p1; p += 4 * rpi) {   // four pixels per trip: their loads are in flight together
            float w4[4][4], t[4][2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ld4(wide + (p + k * rpi) * C + q * 4, w4[k]);
                t[k][0] = DT<T>::ld(thin + (p + k * rpi) * 2);
                t[k][1] = DT<T>::ld(thin + (p + k * rpi) * 2 + 1);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[e][0] += w4[k][e] * t[k][0]; acc[e][1] += w4[k][e] * t[k][1]; }
        }
        for (; p < p1; p += rpi) {
            float w4[4];
            ld4(wide + p * C + q * 4, w4);
            const float t0 = DT<T>::ld(thin + p * 2), t1 = DT<T>::ld(thin + p * 2 + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e][0] += w4[e] * t0; acc[e][1] += w4[e] * t1; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[threadIdx.x * 8 + e * 2] = acc[e][0]; red[threadIdx.x * 8 + e * 2 + 1] = acc[e][1]; }
    __syncthreads();
    if (threadIdx.x < quads) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < rpi; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += red[(k * quads + threadIdx.x) * 8 + e];
        float* out = part + (long)blockIdx.x * C * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = threadIdx.x * 4 + e;
            if (WIDE_IS_X) { out[c * 2] = s[e * 2]; out[c * 2 + 1] = s[e * 2 + 1]; }
            else { out[c] = s[e * 2]; out[C + c] = s[e * 2 + 1]; }
        }
    }
}

size_t wgrad_direct_bytes(int mode, int ks, int dtype, int N, int Hb, int Wb, int IC, int OC) {
    const WgradPlan p = wgrad_plan(mode, ks, dtype, N, Hb, Wb, IC, OC);
    return align256((size_t)p.ws_slices * ks * ks * IC * OC * 4);
}

int run_wgrad_direct(int mode, int ks, const void* x, const void* gy, float* gw, int N, int Hi, int Wi, int IC,
                            int OC, int Hb, int Wb, float alpha, int transpose, int accumulate, int dtype, void* ws, size_t ws_bytes,
                            hipStream_t st, GsWgradReduce* defer) {
    const WgradPlan p = wgrad_plan(mode, ks, dtype, N, Hb, Wb, IC, OC);
    if (p.family > WG_THIN) return fail(GS_ERR_UNSUPPORTED, "conv wgrad direct: %d -> %d channels belong to the MFMA kernels", IC, OC);
    const long ns = p.nslices, pps = p.pps;
    const long npix = (long)N * Hb * Wb;
    const long E = (long)ks * ks * IC * OC;
    if (p.family == WG_THIN) {
        const int C = IC == 2 ? OC : IC;
        if (ws_bytes < (size_t)ns * E * 4) return fail(GS_ERR_WORKSPACE, "conv wgrad thin: workspace too small (%zu)", ws_bytes);
        float* tpart = reinterpret_cast<float*>(ws);
        if (!p.ot) {
            GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((thin_wgrad_kernel<T, false>), dim3((unsigned)ns), dim3(256), 0, st,
                                                        reinterpret_cast<const T*>(gy), reinterpret_cast<const T*>(x), tpart, C, npix, pps));
        } else {
            GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((thin_wgrad_kernel<T, true>), dim3((unsigned)ns), dim3(256), 0, st,
                                                        reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(gy), tpart, C, npix, pps));
        }
        GS_CHECK_LAUNCH();
        wgrad_reduce_launch(tpart, gw, nullptr, (int)ns, 1, IC, OC, alpha, transpose, accumulate, st, defer);
        GS_CHECK_LAUNCH();
        return 0;
    }
    if (ws_bytes < (size_t)ns * E * 4) return fail(GS_ERR_WORKSPACE, "conv wgrad direct: workspace too small (%zu)", ws_bytes);
    float* part = reinterpret_cast<float*>(ws);
    dim3 grid(cdiv(E, 64), (unsigned)ns);
    GS_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv_wgrad_direct_kernel<T>), grid, dim3(256), 0, st,
                                                reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(gy), part, mode,
                                                ks, N, Hi, Wi, IC, OC, Hb, Wb, E, npix, pps));
    GS_CHECK_LAUNCH();
    wgrad_reduce_launch(part, gw, nullptr, (int)ns, ks * ks, IC, OC, alpha, transpose, accumulate, st, defer);
    GS_CHECK_LAUNCH();
    return 0;
}

size_t wgrad_mfma_bytes(int mode, int dtype, int N, int Hb, int Wb, int IC, int OC) {
    const WgradPlan p = wgrad_plan(mode, 3, dtype, N, Hb, Wb, IC, OC);
    return align256((size_t)p.ws_slices * (9 * (size_t)IC * OC + OC) * sizeof(float));
}

// x: conv input side [N][Hi][Wi][IC]; gy: [N][Hb][Wb][OC]; gw[9][IC][OC] (or transposed)
// gb (optional, bf16 only): bias gradient sum_pixels gy[.][oc], produced by the same two launches
int run_wgrad_mfma(int mode, const WgradSrcs& srcs, int nsrc, float* gw, float* gb, int N, int Hi, int Wi, int IC, int OC, int Hb,
                   int Wb, float alpha, int transpose, int accumulate, int dtype, void* ws, size_t ws_bytes, hipStream_t st,
                   GsWgradReduce* defer) {
    // N = images of ALL sources
    if (nsrc < 1 || nsrc > GS_WGRAD_MAX_SRC || srcs.n_end[nsrc - 1] != N) return fail(GS_ERR_ARG, "conv wgrad: %d sources ending at image %d for N=%d", nsrc, srcs.n_end[nsrc > 0 ? nsrc - 1 : 0], N);
    const WgradPlan p = wgrad_plan(mode, 3, dtype, N, Hb, Wb, IC, OC);
    if (p.family < WG_F32) return fail(GS_ERR_UNSUPPORTED, "conv wgrad: no MFMA kernel for %d -> %d channels", IC, OC);
    const int tw = p.tw, tiles_x = p.tiles_x, tiles_y = p.tiles_y, ntiles = p.ntiles, nslices = p.nslices;
    if (gb && !p.fused_bias) return fail(GS_ERR_UNSUPPORTED, "conv wgrad: fused bias gradient needs the bf16 kernels");
    const int with_bias = gb != nullptr;
    const size_t need = (size_t)nslices * (9 * (size_t)IC * OC + (with_bias ? OC : 0)) * sizeof(float);
    if (ws_bytes < need) return fail(GS_ERR_WORKSPACE, "conv wgrad: workspace %zu < %zu", ws_bytes, need);
    float* part = reinterpret_cast<float*>(ws);
    dim3 grid((IC / 32) * (OC / 32), nslices);
    // algorithmic work of a weight gradient: the forward conv's FLOPs over all sources; bytes = x + gy read once, gw written once
    const double wg_flops = 2.0 * 9.0 * (double)N * Hb * Wb * IC * OC;
    const double wg_bytes = ((double)N * Hi * Wi * IC + (double)N * Hb * Wb * OC) * (dtype == GS_F32 ? 4.0 : 2.0) + 9.0 * IC * OC * 4.0;
    ProfScope ps(st, wg_flops, wg_bytes, 10 + mode, N, Hb, Wb, IC, OC, nsrc, defer ? 1 : 0);
    {
#define GS_WG(TT, M, TWV)                                                                                              \
    hipLaunchKernelGGL((conv_wgrad_kernel<TT, M, TWV>), grid, dim3(256), 0, st, srcs,                                  \
                       part, N, Hi, Wi, IC, OC, Hb, Wb, tiles_x, tiles_y, ntiles, nslices)
#define GS_WG_ALL(TT)                                                                       \
    do {                                                                                    \
        if (mode == MODE_S1) { if (tw == 32) GS_WG(TT, MODE_S1, 32); else GS_WG(TT, MODE_S1, 16); } \
        else { if (tw == 32) GS_WG(TT, MODE_S2, 32); else GS_WG(TT, MODE_S2, 16); }          \
    } while (0)
        if (p.family == WG_F32) {
            GS_WG_ALL(float);
        } else {
#define GS_WGB(M, TWV)                                                                                                  \
    do {                                                                                                                \
        if (p.ot == 2)                                                                                                  \
            hipLaunchKernelGGL((conv_wgrad_bf16_kernel<M, TWV, 2>), dim3((IC / 32) * (OC / 64), nslices), dim3(192), 0, st, srcs, \
                               part, N, Hi, Wi, IC, OC, Hb, Wb, tiles_x, tiles_y, ntiles, nslices, with_bias);         \
        else                                                                                                            \
            hipLaunchKernelGGL((conv_wgrad_bf16_kernel<M, TWV>), grid, dim3(192), 0, st, srcs,                          \
                               part, N, Hi, Wi, IC, OC, Hb, Wb, tiles_x, tiles_y, ntiles, nslices, with_bias);         \
    } while (0)
#define GS_WGB2(M, TWV)                                                                                                 \
    do {                                                                                                                \
        constexpr int np_ = (M == MODE_S2 ? 64 : 256), th_ = np_ / TWV;                                                 \
        constexpr int rows_ = patch_dim<M>(th_) * patch_dim<M>(TWV);                                                    \
        constexpr int lds_ = 2 * (2 * ((((rows_ + 15) / 16 + 3) / 4) * 4096) + 2 * np_ * 64);   /* two staged tiles of two planes per side */ \
        auto kern_ = conv_wgrad_bf16_2x2_kernel<M, TWV>;                                                                \
        static bool set_ = false;                                                                                       \
        if (!set_) {                                                                                                    \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern_), hipFuncAttributeMaxDynamicSharedMemorySize, lds_) != hipSuccess) \
                return fail(GS_ERR_HIP, "conv wgrad: cannot reserve %d bytes of dynamic LDS", lds_);                    \
            set_ = true;                                                                                                \
        }                                                                                                               \
        hipLaunchKernelGGL(kern_, dim3((IC / 64) * (OC / 64), nslices), dim3(256), lds_, st, srcs,                          \
                           part, N, Hi, Wi, IC, OC, Hb, Wb, tiles_x, tiles_y, ntiles, nslices, with_bias);              \
    } while (0)
#define GS_WGT(M, OTV)                                                                                                  \
    do {                                                                                                                \
        constexpr int np_ = (M == MODE_S2 ? 64 : 256), th_ = np_ / 32;                                                  \
        constexpr int lds_ = 2 * (((patch_dim<M>(th_) * patch_dim<M>(32) + 15) / 16) * 1024 + OTV * np_ * 64);           \
        auto kern_ = conv_wgrad_bf16_thin_dma_kernel<M, OTV>;                                                           \
        static bool set_ = false;                                                                                       \
        if (!set_) {                                                                                                    \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern_), hipFuncAttributeMaxDynamicSharedMemorySize, lds_) != hipSuccess) \
                return fail(GS_ERR_HIP, "conv wgrad: cannot reserve %d bytes of dynamic LDS", lds_);                    \
            set_ = true;                                                                                                \
        }                                                                                                               \
        hipLaunchKernelGGL(kern_, dim3(1, nslices), dim3(256), lds_, st, srcs,                                          \
                           part, N, Hi, Wi, IC, OC, Hb, Wb, tiles_x, tiles_y, ntiles, nslices, with_bias);              \
    } while (0)
            if (p.family == WG_THIN_DMA) {
                if (mode == MODE_S1) { if (p.ot == 1) GS_WGT(MODE_S1, 1); else GS_WGT(MODE_S1, 2); }
                else { if (p.ot == 1) GS_WGT(MODE_S2, 1); else GS_WGT(MODE_S2, 2); }
            } else if (p.family == WG_TILE64) {
                if (mode == MODE_S1) { if (tw == 32) GS_WGB2(MODE_S1, 32); else GS_WGB2(MODE_S1, 16); }
                else { if (tw == 32) GS_WGB2(MODE_S2, 32); else GS_WGB2(MODE_S2, 16); }
            } else {
                if (mode == MODE_S1) { if (tw == 32) GS_WGB(MODE_S1, 32); else GS_WGB(MODE_S1, 16); }
                else { if (tw == 32) GS_WGB(MODE_S2, 32); else GS_WGB(MODE_S2, 16); }
            }
#undef GS_WGT
#undef GS_WGB2
#undef GS_WGB
        }
#undef GS_WG_ALL
#undef GS_WG
    }
    GS_CHECK_LAUNCH();
    wgrad_reduce_launch(part, gw, gb, nslices, 9, IC, OC, alpha, transpose, accumulate, st, defer);
    GS_CHECK_LAUNCH();
    return 0;
}

// ---- grouped weight gradients: planning and launch of one group (the layers of one conv mode; tiles are 32 pixels wide)
// fills the tiling of job q (its srcs / channel counts / image sizes already set; N = images of all sources)
void wgrad_sk_job_geometry(int mode, int N, SkJob& q) {
    const int np = mode == MODE_S2 ? 64 : 256;
    const int th = np / 32;
    q.tiles_x = cdiv(q.Wb, 32);
    q.tiles_y = cdiv(q.Hb, th);
    q.ntiles = N * q.tiles_x * q.tiles_y;
    q.n_ict = q.IC / 64;
    q.nct = q.n_ict * (q.OC / 64);
}
// unit / run numbering and the block count of a group whose jobs carry their geometry
void wgrad_sk_plan(int mode, SkGroup& g) {
    long units = 0;
    int runs = 0;
    for (int j = 0; j < g.njobs; ++j) {
        g.job[j].unit_base = (int)units;
        g.job[j].run_base = runs;
        units += (long)g.job[j].nct * g.job[j].ntiles;
        runs += g.job[j].nct;
    }
    g.total_units = (int)units;
    g.total_runs = runs;
    // a unit is 2.4 us of MFMAs (stride 1: 144 per wave) or ~2.5 us of patch staging (stride 2: 36 MFMAs under a 4-5x larger patch); a block
    // needs a few of them to amortise its prologue and its flush
    const int upb = mode == MODE_S2 ? 4 : 2;
    long nb = units / upb;
    if (nb > wgrad_cus()) nb = wgrad_cus();
    if (nb < 1) nb = 1;
    g.nblocks = (int)nb;
}
size_t wgrad_sk_bytes(const SkGroup& g) { return align256((size_t)(g.nblocks + g.total_runs) * GS_SK_PSTRIDE * sizeof(float)); }

int run_wgrad_sk(int mode, const SkGroup& g, void* ws, size_t ws_bytes, hipStream_t st) {
    if (g.njobs < 1 || g.njobs > GS_SK_MAX_JOBS) return fail(GS_ERR_ARG, "conv wgrad group: %d jobs", g.njobs);
    if (ws_bytes < wgrad_sk_bytes(g)) return fail(GS_ERR_WORKSPACE, "conv wgrad group: workspace %zu < %zu", ws_bytes, wgrad_sk_bytes(g));
    if ((long)g.total_units <= 0) return 0;
    float* part = reinterpret_cast<float*>(ws);
    double flops = 0.0, bytes = 0.0;
    int images = 0;
    for (int j = 0; j < g.njobs; ++j) {
        const SkJob& q = g.job[j];
        const int N = q.srcs.n_end[GS_WGRAD_MAX_SRC - 1];
        images += N;
        flops += 2.0 * 9.0 * (double)N * q.Hb * q.Wb * q.IC * q.OC;
        bytes += ((double)N * q.Hi * q.Wi * q.IC + (double)N * q.Hb * q.Wb * q.OC) * 2.0 + 9.0 * q.IC * q.OC * 4.0;
    }
    {
        // kind 20 + mode: a GROUP of weight gradients (N = layers, Hb = tile width, Wb = blocks, IC = units, OC = runs)
        ProfScope ps(st, flops, bytes, 20 + mode, g.njobs, 32, g.nblocks, g.total_units, g.total_runs, images, 1);
#define GS_WGSK(M)                                                                                                      \
    do {                                                                                                                \
        constexpr int np_ = (M == MODE_S2 ? 64 : 256), th_ = np_ / 32;                                                  \
        constexpr int lds_ = 2 * ((((patch_dim<M>(th_) * patch_dim<M>(32) + 7) / 8 + 3) / 4) * 4096 + np_ * 128);       /* two staged tiles */ \
        auto kern_ = conv_wgrad_bf16_2x2_sk_kernel<M>;                                                                  \
        static bool set_ = false;                                                                                       \
        if (!set_) {                                                                                                    \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern_), hipFuncAttributeMaxDynamicSharedMemorySize, lds_) != hipSuccess) \
                return fail(GS_ERR_HIP, "conv wgrad group: cannot reserve %d bytes of dynamic LDS", lds_);              \
            set_ = true;                                                                                                \
        }                                                                                                               \
        hipLaunchKernelGGL(kern_, dim3((unsigned)g.nblocks), dim3(256), lds_, st, g, part);                             \
    } while (0)
        if (mode == MODE_S1) GS_WGSK(MODE_S1);
        else GS_WGSK(MODE_S2);
#undef GS_WGSK
    }
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(wgrad_sk_reduce_kernel, dim3((GS_SK_PSTRIDE / 4 + 63) / 64, (unsigned)g.total_runs), dim3(256), 0, st, g, part);
    GS_CHECK_LAUNCH();
    return 0;
}

}  // namespace gs

extern "C" int gs_wgrad_cu_cap(int cap) {
    const int was = gs::g_wgrad_cu_cap;
    gs::g_wgrad_cu_cap = cap < 0 ? 0 : cap;
    return was;
}
