// The dense layers of the PGGAN hot path (ops.py:183-201): forward, data gradient and weight gradient, on plain rows or on the row map of a
// channels-last input.  Weight-bandwidth-bound (16.8 MB of fp32 weights for 8 rows) except the tall discriminator layer, which runs on the
// exact-fp32 MFMA.  Which kernel a call runs is decided in dense_route.h; the launchers at the end of this file launch what it says.
#include "dense_route.h"

namespace gs {

// epilogue of the forward (gs_dense_fwd): y = act(alpha * sum + bias[col]); bias may be NULL, act = GS_ACT_*
__device__ __forceinline__ float dense_epilogue(float sum, float alpha, const float* __restrict__ bias, int col, int act) {
    float v = sum * alpha;
    if (bias) v += bias[col];
    if (act == GS_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
    else if (act == GS_ACT_TANH) v = tanhf(v);
    return v;
}

// ---------------------------------------------------------------------------- dense fwd
// y[b][o] = alpha * sum_i x[b][i] * w[i][o].  Block = 64 output columns x 4 i-lanes; grid.y
// splits the reduction so that (out/64)*ksplit blocks cover the chip; partial sums go through
// `part[ks][b][o]` and a finalize pass (deterministic).
template <typename T>
__global__ __launch_bounds__(256) void dense_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ part,
                                                        int b0, int nb, int in, int out, int b_total, int ipb) {
    __shared__ float red[4][DENSE_BT][64];
    const int tid = threadIdx.x;
    const int col = blockIdx.x * 64 + (tid & 63);
    const int sub = tid >> 6;
    const int ks = blockIdx.y;
    const int i0 = ks * ipb;
    int i1 = i0 + ipb;
    if (i1 > in) i1 = in;
    float acc[DENSE_BT];
#pragma unroll
    for (int b = 0; b < DENSE_BT; ++b) acc[b] = 0.f;
    if (col < out) {
#pragma unroll 4
        for (int i = i0 + sub; i < i1; i += 4) {
            const float wv = w[(long)i * out + col];
            // (unconditional loads -- rows past nb re-read the last valid row, their sums are never written: a per-row `if (b < nb) load`
            //  makes hipcc branch around every load and drain vmcnt(0) each time, 13 us for the 256 -> 61 logits layer)
#pragma unroll
            for (int b = 0; b < DENSE_BT; ++b) acc[b] += DT<T>::ld(x + (long)(b0 + (b < nb ? b : nb - 1)) * in + i) * wv;
        }
    }
#pragma unroll
    for (int b = 0; b < DENSE_BT; ++b) red[sub][b][tid & 63] = acc[b];
    __syncthreads();
    if (sub == 0 && col < out) {
        for (int b = 0; b < nb; ++b)
            part[((long)ks * b_total + b0 + b) * out + col] = red[0][b][tid] + red[1][b][tid] + red[2][b][tid] + red[3][b][tid];
    }
}
// Small layers (the 256 -> 61 logits, ops.py:183-201 on networks.py:186): one block per (64 columns, batch row), 4 row lanes folded through
// LDS, the result written directly -- instead of 8 row-split blocks + a finalize launch (10 + 5 us for a 16 x 256 x 61 product).
template <typename T>
__global__ __launch_bounds__(256) void dense_fwd_small_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y, int in, int out, float alpha,
                                                              const float* __restrict__ bias, int act) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c;
    const int colc = col < out ? col : out - 1;   // (unconditional loads)
    const T* xr = x + (long)blockIdx.y * in;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = sub;
    // 16 weight rows per trip, all 32 loads of the trip in flight together (a chain of 4-row trips was 16 dependent round trips: 10 us)
    for (; i + 60 < in; i += 64) {
        float wv[16], xv[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { wv[k] = w[(long)(i + 4 * k) * out + colc]; xv[k] = DT<T>::ld(xr + i + 4 * k); }
#pragma unroll
        for (int k = 0; k < 16; k += 4) { a0 += xv[k] * wv[k]; a1 += xv[k + 1] * wv[k + 1]; a2 += xv[k + 2] * wv[k + 2]; a3 += xv[k + 3] * wv[k + 3]; }
    }
    for (; i < in; i += 4) a0 += DT<T>::ld(xr + i) * w[(long)i * out + colc];
    red[sub][c] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sub == 0 && col < out) DT<T>::st(y + (long)blockIdx.y * out + col, dense_epilogue(red[0][c] + red[1][c] + red[2][c] + red[3][c], alpha, bias, col, act));
}

// block = 64 elements x 4 split lanes (a narrow layer has few elements and up to 64 splits: a thread per element would walk them
// as one chain in a handful of blocks)
template <typename T>
__global__ __launch_bounds__(256) void dense_finalize_kernel(const float* __restrict__ part, T* __restrict__ y, long n, int ksplit, float alpha,
                                                             const float* __restrict__ bias = nullptr, int act = 0, int out = 1) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, kl = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + e;
    float s0 = 0.f, s1 = 0.f;
    if (i < n) {
        int k = kl;
        for (; k + 4 < ksplit; k += 8) { s0 += part[(long)k * n + i]; s1 += part[(long)(k + 4) * n + i]; }
        if (k < ksplit) s0 += part[(long)k * n + i];
    }
    red[kl][e] = s0 + s1;
    __syncthreads();
    if (kl == 0 && i < n) DT<T>::st(y + i, dense_epilogue(red[0][e] + red[1][e] + red[2][e] + red[3][e], alpha, bias, (int)(i % out), act));
}

// ------------------------------------------------------------------------ dense bwd data
// gx[b][i] = alpha * sum_o gy[b][o] * w[i][o] : one wave per weight row i (coalesced along o).
template <typename T>
__global__ __launch_bounds__(256) void dense_bwd_data_kernel(const T* __restrict__ gy, const float* __restrict__ w, T* __restrict__ gx,
                                                             int b0, int nb, int in, int out, float alpha) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= in) return;
    float acc[DENSE_BT];
#pragma unroll
    for (int b = 0; b < DENSE_BT; ++b) acc[b] = 0.f;
    const float* wr = w + (long)i * out;
#pragma unroll 2
    for (int o = lane; o < out; o += 64) {
        const float wv = wr[o];
#pragma unroll
        for (int b = 0; b < DENSE_BT; ++b) acc[b] += DT<T>::ld(gy + (long)(b0 + (b < nb ? b : nb - 1)) * out + o) * wv;   // (unconditional, see dense_fwd_kernel)
    }
#pragma unroll
    for (int b = 0; b < DENSE_BT; ++b) {
        if (b < nb) {
            const float s = wave_sum(acc[b]);
            if (lane == 0) DT<T>::st(gx + (long)(b0 + b) * in + i, s * alpha);
        }
    }
}

// ---------------------------------------------------------------------- dense bwd weight
// gw[i][o] = alpha * sum_b x[b][i] * gy[b][o]
template <typename T>
__global__ void dense_bwd_weight_kernel(const T* __restrict__ x, const T* __restrict__ gy, float* __restrict__ gw, int b, int in, int out, float alpha, int accumulate) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)in * out) return;
    const int o = e % out;
    const int i = e / out;
    float s = 0.f;
    int k = 0;
    for (; k + 8 <= b; k += 8) {   // eight batch rows per trip, their 16 loads in flight together
        float xv[8], gv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { xv[j] = DT<T>::ld(x + (long)(k + j) * in + i); gv[j] = DT<T>::ld(gy + (long)(k + j) * out + o); }
#pragma unroll
        for (int j = 0; j < 8; ++j) s += xv[j] * gv[j];
    }
    for (; k < b; ++k) s += DT<T>::ld(x + (long)k * in + i) * DT<T>::ld(gy + (long)k * out + o);
    gw[e] = accumulate ? gw[e] + s * alpha : s * alpha;
}

// wide rows (out >= 2048, e.g. the generator's 512 -> 8192 dense): one block per weight row
template <typename T>
__global__ __launch_bounds__(256) void dense_bwd_data_wide_kernel(const T* __restrict__ gy, const float* __restrict__ w, T* __restrict__ gx,
                                                                  int b0, int nb, int in, int out, float alpha) {
    __shared__ float red[4];
    const int i = blockIdx.x;
    float acc[DENSE_BT];
#pragma unroll
    for (int b = 0; b < DENSE_BT; ++b) acc[b] = 0.f;
    const float* wr = w + (long)i * out;
    for (int o = threadIdx.x; o < out; o += 256) {
        const float wv = wr[o];
#pragma unroll
        for (int b = 0; b < DENSE_BT; ++b)
            if (b < nb) acc[b] += DT<T>::ld(gy + (long)(b0 + b) * out + o) * wv;
    }
#pragma unroll
    for (int b = 0; b < DENSE_BT; ++b) {
        if (b < nb) {
            const float s = block_sum<256>(acc[b], red);
            if (threadIdx.x == 0) DT<T>::st(gx + (long)(b0 + b) * in + i, s * alpha);
        }
    }
}


// ---- fast paths (vector loads; the generic kernels above remain for odd shapes) ------------------------------------
// Input side in channels-last order (rc, rhw != 0): x / gx are the memory of a channels-last [b][hw][c] activation while the weight
// rows follow tf.layers.flatten of NCHW (row = c * hw + p, networks.py:185-186).  Weight rows are read and written whole, so the
// flatten is a ROW INDEX MAP inside the kernels: no NCHW copy of the activation, no copy of its gradient back.
__device__ __forceinline__ long dense_row(int r, int rc, int rhw) { return rc ? (long)(r % rc) * rhw + r / rc : (long)r; }

// y[b][o] = alpha * sum_i x[b][i] w[i][o], in % 4 == 0, out % 32 == 0.  Block = 8 column threads (float4: 32 columns) x 32 row
// lanes; a row lane takes 4 consecutive rows per pass (one 8/16-byte load of x per batch row).  Row lanes are folded with
// xor-shuffles inside a wave and through LDS across the 4 waves; with ksplit == 1 the result is written directly.
template <typename T, int FB>
__global__ __launch_bounds__(256) void dense_fwd_fast_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ part,
                                                             T* __restrict__ y, int b0, int nb, int in, int out, int b_total, int ipb, float alpha, int rc, int rhw,
                                                             const float* __restrict__ bias, int act) {
    __shared__ float red[4][FB][32];
    const int tid = threadIdx.x;
    const int c = tid & 7, r = tid >> 3;           // column thread, row lane (0..31)
    const int col = blockIdx.x * 32 + c * 4;
    const int i0 = blockIdx.y * ipb;
    int i1 = i0 + ipb;
    if (i1 > in) i1 = in;
    float acc[FB][4];
#pragma unroll
    for (int b = 0; b < FB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[b][e] = 0.f;
#pragma unroll 2
    for (int i = i0 + 4 * r; i < i1; i += 128) {
        float4 wv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = *reinterpret_cast<const float4*>(w + dense_row(i + k, rc, rhw) * out + col);
        // (loads are unconditional -- rows past nb re-read the last valid row and their sums are never written: a per-row
        //  `if (b < nb) load` makes hipcc branch around every load and drain vmcnt(0) each time)
#pragma unroll
        for (int b = 0; b < FB; ++b) {
            float xv[4];
            ld4(x + (long)(b0 + (b < nb ? b : nb - 1)) * in + i, xv);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[b][0] += xv[k] * wv[k].x; acc[b][1] += xv[k] * wv[k].y; acc[b][2] += xv[k] * wv[k].z; acc[b][3] += xv[k] * wv[k].w;
            }
        }
    }
    // fold the 8 row lanes of the wave (lane = r_local * 8 + c)
#pragma unroll
    for (int b = 0; b < FB; ++b) {
        if (b < nb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[b][e];
                v = residue_sum(v, 8);   // lanes l, l + 8 ... l + 56
                acc[b][e] = v;
            }
        }
    }
    const int wv_ = tid >> 6;
    if ((tid & 63) < 8) {
#pragma unroll
        for (int b = 0; b < FB; ++b)
            if (b < nb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) red[wv_][b][c * 4 + e] = acc[b][e];
            }
    }
    __syncthreads();
    for (int k = tid; k < nb * 32; k += 256) {
        const int b = k >> 5, cc = k & 31;
        const float s = red[0][b][cc] + red[1][b][cc] + red[2][b][cc] + red[3][b][cc];
        const int o = blockIdx.x * 32 + cc;
        if (part) part[((long)blockIdx.y * b_total + b0 + b) * out + o] = s;
        else DT<T>::st(y + (long)(b0 + b) * out + o, dense_epilogue(s, alpha, bias, o, act));
    }
}

// gx[b][i] = alpha * sum_o gy[b][o] w[i][o], out % 256 == 0: WPR waves per weight row (1: a wave per row; 4: the block's four
// waves split a long row -- the generator's 512 x 8192 dense has only 512 rows, a wave per row is 128 blocks of 32 serial
// trips), 16 bytes of w per lane per pass.
template <typename T, int WPR, int FB>
__global__ __launch_bounds__(256) void dense_bwd_data_fast_kernel(const T* __restrict__ gy, const float* __restrict__ w, T* __restrict__ gx,
                                                                  int b0, int nb, int in, int out, float alpha, int rc, int rhw) {
    __shared__ float red[4][FB];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * (4 / WPR) + wv / WPR;
    const int sub = wv % WPR;
    float acc[FB];
#pragma unroll
    for (int b = 0; b < FB; ++b) acc[b] = 0.f;
    const float* wr = w + dense_row(i < in ? i : in - 1, rc, rhw) * out;
#pragma unroll 4
    for (int o = (sub * 64 + lane) * 4; o < out; o += 256 * WPR) {
        const float4 wv = *reinterpret_cast<const float4*>(wr + o);
#pragma unroll
        for (int b = 0; b < FB; ++b) {   // unconditional loads, see dense_fwd_fast_kernel
            float gv[4];
            ld4(gy + (long)(b0 + (b < nb ? b : nb - 1)) * out + o, gv);
            acc[b] += gv[0] * wv.x + gv[1] * wv.y + gv[2] * wv.z + gv[3] * wv.w;
        }
    }
    if constexpr (WPR == 1) {
        if (i >= in) return;
#pragma unroll
        for (int b = 0; b < FB; ++b) {
            if (b < nb) {
                const float sum = wave_sum(acc[b]);
                if (lane == 0) DT<T>::st(gx + (long)(b0 + b) * in + i, sum * alpha);
            }
        }
    } else {
#pragma unroll
        for (int b = 0; b < FB; ++b) {
            const float sum = wave_sum(acc[b]);
            if (lane == 0) red[wv][b] = sum;
        }
        __syncthreads();
        if (threadIdx.x < nb && i < in)
            DT<T>::st(gx + (long)(b0 + threadIdx.x) * in + i, (red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]) * alpha);
    }
}

// The same map for MANY SHORT ROWS (the discriminator's 8192 x 256 dense: 8192 one-KiB weight rows) on the exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32: an fmaf chain, bitwise): a wave per tile of 16 weight rows x 16 batch rows, K = out.  The wave-per-row
// form above spends its time in cross-lane sums -- 16 wave reductions of 6 shuffle steps per KiB of weights, 21 us for 8.4 MB --
// where the matrix core reduces in hardware.  Lane (n = lane & 15, kq = lane >> 4) feeds B[k][n] = w[row n][k] and A[m][k] = gy[m][k] with
// m = lane & 15; step (j, e) of the K loop uses k = 16 j + 4 kq + e, so that a lane reads 16 contiguous bytes of its weight row per j
// (the four lanes of a row 64 contiguous bytes) and 4 consecutive gradients.  D[m = 4 (lane >> 4) + r][n = lane & 15] = acc[r].
typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <typename T>
__global__ __launch_bounds__(256) void dense_bwd_data_mfma_kernel(const T* __restrict__ gy, const float* __restrict__ w, T* __restrict__ gx,
                                                                  int b, int in, int out, float alpha, int rc, int rhw) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 16 >= in) return;
    const int n = lane & 15, kq = lane >> 4;
    const int row = tile * 16 + n;
    const float* wr = w + dense_row(row < in ? row : in - 1, rc, rhw) * out + 4 * kq;
    for (int m0 = 0; m0 < b; m0 += 16) {
        const int m = m0 + n;   // (this lane's A row; rows past b re-read the last one, their results are never written)
        const T* ar = gy + (long)(m < b ? m : b - 1) * out + 4 * kq;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = 0; k < out; k += 16) {
            const float4 bv = *reinterpret_cast<const float4*>(wr + k);
            float av[4];
            ld4(ar + k, av);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv.w, acc, 0, 0, 0);
        }
        if (row < in) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mm = m0 + 4 * kq + r;
                if (mm < b) DT<T>::st(gx + (long)mm * in + row, acc[r] * alpha);
            }
        }
    }
}

// Forward of the same tall layer (in = 8192, out = 256, 8 or 16 batch rows): y[m][c] = sum_k x[m][k] w[k][c] on the exact-fp32 MFMA, K split
// over waves (64 input rows each: 512 waves for the discriminator's dense), partial sums through `part[ks][b][out]` and the existing
// finalize pass (fixed order: deterministic).  A wave owns 64 columns as four interleaved 16-column tiles -- tile e = columns 4 n + e --
// so that a lane's B operands of the four tiles are ONE 16-byte load of weight row k (the 16 lanes of a kq group read 256 contiguous
// bytes); lane (n, kq) takes k = k0 + 16 kq + 4 t + u.
template <typename T>
__global__ __launch_bounds__(256) void dense_fwd_mfma_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ part,
                                                             int b, int in, int out, int rc, int rhw) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ncg = out / 64;
    const int cg = wave % ncg, ks = wave / ncg;
    if (ks * 64 >= in) return;
    const int n = lane & 15, kq = lane >> 4;
    const int kb = ks * 64 + 16 * kq;   // this lane's 16 input rows
    const float* wc = w + cg * 64 + 4 * n;
    // all 16 weight loads of the lane go out before the first MFMA (a `rc ? mapped : plain` branch per row made hipcc wait for every load
    // by itself: 16 serial memory latencies, 12-15 us); the row map is walked incrementally -- rc_ = "rows per column block", 1 << 30 when
    // there is no map, so that row % rc_ = row and row / rc_ = 0
    const int rc_ = rc ? rc : (1 << 30), rhw_ = rc ? rhw : 1;
    int rem = kb % rc_, quo = kb / rc_;
    float4 bv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        bv[i] = *reinterpret_cast<const float4*>(wc + ((long)rem * rhw_ + quo) * out);
        ++rem;
        const bool wrap = rem == rc_;
        rem = wrap ? 0 : rem;
        quo += wrap ? 1 : 0;
    }
    for (int m0 = 0; m0 < b; m0 += 16) {
        const int m = m0 + n;
        const T* ar = x + (long)(m < b ? m : b - 1) * in + kb;
        float av[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ld4(ar + 4 * t, av[t]);
        f32x4_t acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float a = av[i >> 2][i & 3];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[i].x, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[i].y, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[i].z, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[i].w, acc[3], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mm = m0 + 4 * kq + r;
            if (mm < b) *reinterpret_cast<float4*>(part + ((long)ks * b + mm) * out + cg * 64 + 4 * n) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        }
    }
}

// gw[i][o] (+)= alpha * sum_b x[b][i] gy[b][o], out % 256 == 0, b <= DENSE_BT: a thread keeps its 4 columns of gy for every
// batch row in registers and walks DENSE_WR rows of the weight matrix (16-byte stores).
template <typename T>
__global__ __launch_bounds__(256) void dense_bwd_weight_fast_kernel(const T* __restrict__ x, const T* __restrict__ gy, float* __restrict__ gw,
                                                                    int b, int in, int out, float alpha, int accumulate, int rc, int rhw) {
    __shared__ float xs[DENSE_BT][DENSE_WR];
    const int tid = threadIdx.x;
    const int ct = tid & 63, rl = tid >> 6;
    const int col = blockIdx.x * 256 + ct * 4;
    const int r0 = blockIdx.y * DENSE_WR;
    for (int k = tid; k < DENSE_BT * DENSE_WR; k += 256) {
        const int bb = k / DENSE_WR, rr = k % DENSE_WR;
        xs[bb][rr] = (bb < b && r0 + rr < in) ? DT<T>::ld(x + (long)bb * in + r0 + rr) * alpha : 0.f;
    }
    float g[DENSE_BT][4];
#pragma unroll
    for (int bb = 0; bb < DENSE_BT; ++bb) {   // unconditional loads; rows past b are multiplied by the zeros staged in xs
        ld4(gy + (long)(bb < b ? bb : b - 1) * out + col, g[bb]);
    }
    __syncthreads();
    for (int rr = rl; rr < DENSE_WR && r0 + rr < in; rr += 4) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int bb = 0; bb < DENSE_BT; ++bb) {
            const float xv = xs[bb][rr];
            o[0] += xv * g[bb][0]; o[1] += xv * g[bb][1]; o[2] += xv * g[bb][2]; o[3] += xv * g[bb][3];
        }
        float4* dst = reinterpret_cast<float4*>(gw + dense_row(r0 + rr, rc, rhw) * out + col);
        if (accumulate) {
            const float4 old = *dst;
            o[0] += old.x; o[1] += old.y; o[2] += old.z; o[3] += old.w;
        }
        *dst = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ------------------------------------------------------------------------------ launchers: what the route says, one per map
template <typename T>
static int dense_fwd_run(const DenseRoute& r, const GsDense& d, const T* x, const float* w, const float* bias, int act, T* y, hipStream_t st) {
    const dim3 grid(r.grid_x, r.grid_y), block(256);
    float* part = (float*)d.ws;
    for (int b0 = 0; b0 < d.b; b0 += r.step) {
        const int nb = d.b - b0 < r.step ? d.b - b0 : r.step;
        if (r.kernel == GS_DENSE_FWD_SMALL) hipLaunchKernelGGL((dense_fwd_small_kernel<T>), grid, block, 0, st, x, w, y, d.in, d.out, d.alpha, bias, act);
        else if (r.kernel == GS_DENSE_FWD_MFMA) hipLaunchKernelGGL((dense_fwd_mfma_kernel<T>), grid, block, 0, st, x, w, part, d.b, d.in, d.out, d.c, d.hw);
        else if (r.kernel == GS_DENSE_FWD) hipLaunchKernelGGL((dense_fwd_kernel<T>), grid, block, 0, st, x, w, part, b0, nb, d.in, d.out, d.b, r.ipb);
        else if (r.kernel != GS_DENSE_FWD_FAST || !with_constant<8, 16, 24>(r.FB, [&](auto fb) {
                     hipLaunchKernelGGL((dense_fwd_fast_kernel<T, decltype(fb)::value>), grid, block, 0, st, x, w, r.ksplit > 1 ? part : nullptr, y, b0, nb, d.in, d.out, d.b, r.ipb,
                                        d.alpha, d.c, d.hw, bias, act);
                     return true;
                 }))
            return fail(GS_ERR_UNSUPPORTED, "dense_fwd: kernel %d with FB %d is not compiled", r.kernel, r.FB);
        GS_CHECK_LAUNCH();
    }
    if (!r.finalize) return 0;
    const long n = (long)d.b * d.out;
    hipLaunchKernelGGL((dense_finalize_kernel<T>), dim3(cdiv(n, 64)), block, 0, st, part, y, n, r.ksplit, d.alpha, bias, act, d.out);
    GS_CHECK_LAUNCH();
    return 0;
}
template <typename T>
static int dense_bwd_data_run(const DenseRoute& r, const GsDense& d, const T* gy, const float* w, T* gx, hipStream_t st) {
    const dim3 grid(r.grid_x, r.grid_y), block(256);
    for (int b0 = 0; b0 < d.b; b0 += r.step) {
        const int nb = d.b - b0 < r.step ? d.b - b0 : r.step;
        if (r.kernel == GS_DENSE_BWD_DATA_MFMA) hipLaunchKernelGGL((dense_bwd_data_mfma_kernel<T>), grid, block, 0, st, gy, w, gx, d.b, d.in, d.out, d.alpha, d.c, d.hw);
        else if (r.kernel == GS_DENSE_BWD_DATA_WIDE) hipLaunchKernelGGL((dense_bwd_data_wide_kernel<T>), grid, block, 0, st, gy, w, gx, b0, nb, d.in, d.out, d.alpha);
        else if (r.kernel == GS_DENSE_BWD_DATA) hipLaunchKernelGGL((dense_bwd_data_kernel<T>), grid, block, 0, st, gy, w, gx, b0, nb, d.in, d.out, d.alpha);
        else if (r.kernel != GS_DENSE_BWD_DATA_FAST || !with_constant<4, 1>(r.WPR, [&](auto wpr) {
                     return with_constant<8, 16, 24>(r.FB, [&](auto fb) {
                         hipLaunchKernelGGL((dense_bwd_data_fast_kernel<T, decltype(wpr)::value, decltype(fb)::value>), grid, block, 0, st, gy, w, gx, b0, nb, d.in, d.out, d.alpha, d.c, d.hw);
                         return true;
                     });
                 }))
            return fail(GS_ERR_UNSUPPORTED, "dense_bwd_data: kernel %d with WPR %d, FB %d is not compiled", r.kernel, r.WPR, r.FB);
        GS_CHECK_LAUNCH();
    }
    return 0;
}
template <typename T>
static int dense_bwd_weight_run(const DenseRoute& r, const GsDense& d, const T* x, const T* gy, float* gw, int accumulate, hipStream_t st) {
    const dim3 grid(r.grid_x, r.grid_y), block(256);
    if (r.kernel == GS_DENSE_BWD_WEIGHT_FAST) hipLaunchKernelGGL((dense_bwd_weight_fast_kernel<T>), grid, block, 0, st, x, gy, gw, d.b, d.in, d.out, d.alpha, accumulate, d.c, d.hw);
    else if (r.kernel == GS_DENSE_BWD_WEIGHT) hipLaunchKernelGGL((dense_bwd_weight_kernel<T>), grid, block, 0, st, x, gy, gw, d.b, d.in, d.out, d.alpha, accumulate);
    else return fail(GS_ERR_UNSUPPORTED, "dense_bwd_weight: no kernel %d", r.kernel);
    GS_CHECK_LAUNCH();
    return 0;
}

// the route of a map of layer d, or the refusal the entry point answers with.  no_mfma < 0: the process's knob
static int dense_plan(const char* who, const GsDense* d, int map, int no_mfma, DenseRoute* r) {
    GS_CHECK_ARG(d && (d->dtype == GS_F32 || d->dtype == GS_BF16), "%s: no layer descriptor, or a bad dtype", who);
    const char* why = "";
    const int e = dense_route(DenseCall{map, d->b, d->in, d->out, d->c, d->hw, d->dtype}, no_mfma < 0 ? dense_knobs_env() : DenseKnobs{no_mfma != 0}, r, &why);
    return e ? fail(e, "%s: %s (b %d, in %d, out %d, c %d, hw %d)", who, why, d->b, d->in, d->out, d->c, d->hw) : 0;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_dense_fwd_workspace_bytes(const GsDense* d) {
    DenseRoute r;
    return dense_plan("dense_fwd", d, GS_DENSE_MAP_FWD, -1, &r) ? 0 : r.ws_bytes;
}

extern "C" int gs_dense_fwd(const GsDense* d, const void* x, const float* w, const float* bias, int act, void* y, void* stream) {
    GS_CHECK_ARG(act >= 0 && act <= 2, "dense_fwd: bad activation %d", act);
    DenseRoute r;
    if (int e = dense_plan("dense_fwd", d, GS_DENSE_MAP_FWD, -1, &r)) return e;
    if (d->ws_bytes < r.ws_bytes) return fail(GS_ERR_WORKSPACE, "dense_fwd: workspace too small");
    GS_DISPATCH_DTYPE(d->dtype, return dense_fwd_run<T>(r, *d, (const T*)x, w, bias, act, (T*)y, as_stream(stream)));
    return 0;
}

extern "C" int gs_dense_bwd_data(const GsDense* d, const void* gy, const float* w, void* gx, void* stream) {
    DenseRoute r;
    if (int e = dense_plan("dense_bwd_data", d, GS_DENSE_MAP_BWD_DATA, -1, &r)) return e;
    GS_DISPATCH_DTYPE(d->dtype, return dense_bwd_data_run<T>(r, *d, (const T*)gy, w, (T*)gx, as_stream(stream)));
    return 0;
}

extern "C" int gs_dense_bwd_weight(const GsDense* d, const void* x, const void* gy, float* gw, int accumulate, void* stream) {
    DenseRoute r;
    if (int e = dense_plan("dense_bwd_weight", d, GS_DENSE_MAP_BWD_WEIGHT, -1, &r)) return e;
    GS_DISPATCH_DTYPE(d->dtype, return dense_bwd_weight_run<T>(r, *d, (const T*)x, (const T*)gy, gw, accumulate, as_stream(stream)));
    return 0;
}

extern "C" int gs_dense_route(const GsDense* d, int map, int no_mfma_or_minus1, int* out) {
    GS_CHECK_ARG(out, "dense_route: no output");
    DenseRoute r;
    if (int e = dense_plan("dense_route", d, map, no_mfma_or_minus1, &r)) return e;
    static_assert(sizeof(DenseRoute) == GS_DENSE_ROUTE_INTS * sizeof(int), "DenseRoute is the ints the query reports");
    memcpy(out, &r, sizeof(r));
    return 0;
}
