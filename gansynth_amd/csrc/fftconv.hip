// Reverb: the convolution of a clip with an impulse response as a uniform partitioned overlap-save FFT convolution (gansynth_amd/reverb.py,
// kernels.fft_convolve; the rule is this project's own and is stated in include/gansynth_hip.h and DESIGN.md "Reverb").
//
// B = GS_FFTCONV_BLOCK new samples per block.  A 2B-point real transform runs as a B-point complex one (even samples real, odd imaginary)
// held in LDS, and a spectrum is stored as B complex values: slot 0 the two real bins (0 and B), slot k the bin k.
// The FFT is a radix-2 Stockham autosort: natural order in and out, ping-pong between two 16 KB LDS buffers, one barrier per stage.  Stage
// `ls` (stride s = 2^ls) reads src[t] and src[t + B/2] -- contiguous over the lanes, conflict-free -- and writes dst[q + 2 p s] and
// dst[q + 2 p s + s] (t = p s + q): runs of s contiguous float2, so the stores of the stages with s < 32 meet two-way bank conflicts and
// the rest none.  (The DIT form of spectral.hip's fft_lds wants its input bit-reversed: at 2048 points the 32 lanes of a half-wave would
// store to one bank.)  The stage twiddles lie stage by stage, T[m + p] = exp(-i pi p / m) for m = 1, 2 .. B/2, so that a stage reads them
// contiguously too; they are staged in LDS once per block (16 KB).  48 KB of LDS a block: three blocks a CU.
//
//   fc_tables_kernel     the two twiddle tables, in double, rounded once (gs_fftconv_prepare).
//   fc_lead_kernel       the index of the first non-zero tap of every IR row (the wet part is exactly 0 before it).
//   fc_transform_kernel  one block per (segment, row): 2B samples from global (16 bytes per lane where the row base allows, zero outside the
//                        row), forward FFT, the unpacking to the real signal's spectrum.  The partitions of h (prepare) and the blocks of x.
//   fc_mac_kernel        one block per (row, j): sum over p of X[j - p] * H[p] in registers (a lane owns 4 bin pairs (k, B - k): 16
//                        accumulators), the packing, inverse FFT, the last B samples times wet plus dry * x, 16-byte stores, one |max| a block.
// The finish (ONE peak, quotient, PCM) is clip_finish.hip's, through launch_clip_finish: one clip of `rows` channels.
#include <math.h>

#include "clip_finish.h"
#include "gs_common.h"

namespace gs {

constexpr int FC_NT = 256;                  // threads per block
constexpr int FC_B = GS_FFTCONV_BLOCK;      // new samples per block = complex points of the packed transform
constexpr int FC_LOG2B = 11;
constexpr int FC_HALF = FC_B / 2;
constexpr int FC_BF = FC_HALF / FC_NT;      // butterflies (and bin pairs) per lane
constexpr int FC_TWP = FC_HALF + 8;         // float2 of the pack table: exp(-i pi k / B), k in [0, B/2], padded to 16 bytes
constexpr size_t FC_LEAD_OFF = (size_t)(FC_B + FC_TWP) * sizeof(float2);
constexpr size_t FC_HEAD = FC_LEAD_OFF + 16;
static_assert(FC_B == (1 << FC_LOG2B) && FC_BF * FC_NT == FC_HALF && FC_B % (4 * FC_NT) == 0, "the kernels are written for this block");
static_assert(FC_HEAD == GS_FFTCONV_HEADER_BYTES, "include/gansynth_hip.h states the header");
static_assert(sizeof(GsFftConv) == 40, "GsFftConv is 40 bytes (gansynth_amd/_lib.py mirrors it)");

__device__ inline float2 fc_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// the stage twiddles from the spectrum buffer into LDS, 16 bytes per lane (no barrier: the caller's comes before the first use)
__device__ inline void fc_stage_twiddles(float2* tw, const float2* __restrict__ tables) {
    const float4* __restrict__ g = reinterpret_cast<const float4*>(tables);
    float4* l = reinterpret_cast<float4*>(tw);
#pragma unroll
    for (int u = 0; u < FC_B / 2 / FC_NT; ++u) l[u * FC_NT + threadIdx.x] = g[u * FC_NT + threadIdx.x];
}

// FFT of the FC_B points in `a` (filled, barrier passed), natural order in and out; INV conjugates the twiddles (no scaling).
// -> the buffer that holds the result (barrier passed)
template <bool INV>
__device__ inline float2* fc_fft(float2* a, float2* b, const float2* tw) {
    float2* src = a;
    float2* dst = b;
#pragma unroll
    for (int ls = 0; ls < FC_LOG2B; ++ls) {
        const int m = FC_HALF >> ls;            // half the length of this stage's sub-transforms; their stride is s = 1 << ls
#pragma unroll
        for (int u = 0; u < FC_BF; ++u) {
            const int t = u * FC_NT + threadIdx.x;
            const int p = t >> ls, q = t & ((1 << ls) - 1);
            float2 w = tw[m + p];
            if (INV) w.y = -w.y;
            const float2 x0 = src[t], x1 = src[t + FC_HALF];
            dst[q + ((2 * p) << ls)] = make_float2(x0.x + x1.x, x0.y + x1.y);
            dst[q + ((2 * p + 1) << ls)] = fc_cmul(make_float2(x0.x - x1.x, x0.y - x1.y), w);
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
    }
    return src;
}

// grid (1).  tables[m + p] = exp(-i pi p / m) for m = 1, 2 .. B/2 and p < m (tables[0] = 1 is not read); tables[B + k] = exp(-i pi k / B), k <= B/2
__global__ __launch_bounds__(FC_NT) void fc_tables_kernel(float2* __restrict__ tables) {
    for (int i = threadIdx.x; i < FC_B + FC_TWP; i += FC_NT) {
        double a = 0.0;
        if (i >= FC_B) a = i - FC_B <= FC_HALF ? (double)(i - FC_B) / (double)FC_B : 0.0;
        else if (i > 0) {
            const int m = 1 << (31 - __clz(i));
            a = (double)(i - m) / (double)m;
        }
        double sn, cs;
        sincospi(-a, &sn, &cs);
        tables[i] = make_float2((float)cs, (float)sn);
    }
}

// grid (ir_rows).  lead[row] = the index of the first tap of h[row] that is not 0, m when there is none (m <= 2^20: exact as a float)
__global__ __launch_bounds__(FC_NT) void fc_lead_kernel(const float* __restrict__ h, long m, long stride, int* __restrict__ lead) {
    const float* __restrict__ row = h + (size_t)blockIdx.x * stride;
    float first = (float)m;
    for (long k = threadIdx.x; k < m; k += FC_NT)
        if (row[k] != 0.f) { first = (float)k; break; }
    first = wave_extreme<false>(first);
    __shared__ float part[FC_NT / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = part[0];
#pragma unroll
        for (int w = 1; w < FC_NT / 64; ++w) r = fminf(r, part[w]);
        lead[blockIdx.x] = (int)r;
    }
}

// grid (segments, rows).  Segment g of row r is the 2B samples from (g + shift) * B on; the first `live` of them (a multiple of 4) are read
// from src -- an index outside [0, len) gives 0 -- and the rest are 0.  dst[(r * segments + g) * B + slot] = the spectrum.
__global__ __launch_bounds__(FC_NT) void fc_transform_kernel(const float* __restrict__ src, long len, long stride, int shift, int live,
                                                             const float2* __restrict__ tables, float2* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float2 za[FC_B];
    __shared__ __attribute__((aligned(16))) float2 zb[FC_B];
    __shared__ __attribute__((aligned(16))) float2 tw[FC_B];
    fc_stage_twiddles(tw, tables);
    const long seg0 = ((long)blockIdx.x + shift) * FC_B;
    const float* __restrict__ row = src + (size_t)blockIdx.y * stride;
    const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;   // block-uniform
#pragma unroll
    for (int u = 0; u < 2 * FC_B / 4 / FC_NT; ++u) {
        const int c = u * FC_NT + threadIdx.x;     // the pack of samples 4c .. 4c + 3 of the segment
        const long t0 = seg0 + 4 * c;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (4 * c < live) {
            if (wide && t0 >= 0 && t0 + 4 <= len) ld4(row + t0, v);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t0 + j >= 0 && t0 + j < len) v[j] = row[t0 + j];
            }
        }
        *reinterpret_cast<float4*>(&za[2 * c]) = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    const float2* z = fc_fft<false>(za, zb, tw);
    const float2* __restrict__ twp = tables + FC_B;
    float2* __restrict__ o = dst + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * FC_B;
    for (int k = threadIdx.x; k <= FC_HALF; k += FC_NT) {
        if (k == 0) {   // the two real bins
            const float2 z0 = z[0];
            o[0] = make_float2(z0.x + z0.y, z0.x - z0.y);
            continue;
        }
        const float2 zk = z[k], zc = z[FC_B - k];
        const float2 e = make_float2(zk.x + zc.x, zk.y - zc.y);      // 2 E = Zk + conj(Zc): the even samples' bin
        const float2 d = make_float2(zk.y + zc.y, zc.x - zk.x);      // 2 O = -i (Zk - conj(Zc)): the odd samples' bin
        const float2 wo = fc_cmul(twp[k], d);
        o[k] = make_float2(0.5f * (e.x + wo.x), 0.5f * (e.y + wo.y));                                  // X[k] = E + w^k O
        if (k != FC_HALF) o[FC_B - k] = make_float2(0.5f * (e.x - wo.x), -0.5f * (e.y - wo.y));       // X[B - k] = conj(E - w^k O)
    }
}

// grid (J, rows).  Block j of row r: out[r][jB + i] = dry * x[r][jB + i] + wet * conv for i < B below n_out, block_max[r * J + j] = its max |.|
__global__ __launch_bounds__(FC_NT) void fc_mac_kernel(const float2* __restrict__ xs, int x_blocks, const float2* __restrict__ spectrum, int partitions,
                                                       int shared_ir, const float* __restrict__ x, long n, long row_stride, float dry, float wet,
                                                       long n_out, float* __restrict__ out, long out_stride, float* __restrict__ block_max) {
    __shared__ __attribute__((aligned(16))) float2 za[FC_B];
    __shared__ __attribute__((aligned(16))) float2 zb[FC_B];
    __shared__ __attribute__((aligned(16))) float2 tw[FC_B];
    fc_stage_twiddles(tw, spectrum);
    const int j = blockIdx.x, r = blockIdx.y, rh = shared_ir ? 0 : r;
    const float2* __restrict__ twp = spectrum + FC_B;
    const int lead = reinterpret_cast<const int*>(reinterpret_cast<const char*>(spectrum) + FC_LEAD_OFF)[rh];
    const float2* __restrict__ hs = reinterpret_cast<const float2*>(reinterpret_cast<const char*>(spectrum) + FC_HEAD) + (size_t)rh * partitions * FC_B;
    const float2* __restrict__ xr = xs + (size_t)r * x_blocks * FC_B;

    // bin pair u of this lane: k = u * FC_NT + threadIdx.x in [0, B/2) and its mirror B - k; the pair of k == 0 is slot 0 (two real bins) and B/2
    float2 acc_a[FC_BF], acc_b[FC_BF];
#pragma unroll
    for (int u = 0; u < FC_BF; ++u) acc_a[u] = acc_b[u] = make_float2(0.f, 0.f);
    const int p_lo = j - x_blocks + 1 > 0 ? j - x_blocks + 1 : 0;
    const int p_hi = j < partitions - 1 ? j : partitions - 1;
    for (int p = p_lo; p <= p_hi; ++p) {
        const float2* __restrict__ xp = xr + (size_t)(j - p) * FC_B;
        const float2* __restrict__ hp = hs + (size_t)p * FC_B;
#pragma unroll
        for (int u = 0; u < FC_BF; ++u) {
            const int k = u * FC_NT + threadIdx.x;
            const int kb = k == 0 ? FC_HALF : FC_B - k;
            const float2 xa = xp[k], ha = hp[k], xb = xp[kb], hb = hp[kb];
            const float2 pa = k == 0 ? make_float2(xa.x * ha.x, xa.y * ha.y) : fc_cmul(xa, ha);
            const float2 pb = fc_cmul(xb, hb);
            acc_a[u].x += pa.x; acc_a[u].y += pa.y;
            acc_b[u].x += pb.x; acc_b[u].y += pb.y;
        }
    }
    // the packing Z[k] = (Y[k] + conj(Y[B - k])) + i conj(w^k) (Y[k] - conj(Y[B - k])): twice the spectrum of y[2n] + i y[2n + 1]
#pragma unroll
    for (int u = 0; u < FC_BF; ++u) {
        const int k = u * FC_NT + threadIdx.x;
        if (k == 0) {
            za[0] = make_float2(acc_a[u].x + acc_a[u].y, acc_a[u].x - acc_a[u].y);
            za[FC_HALF] = make_float2(2.f * acc_b[u].x, -2.f * acc_b[u].y);
            continue;
        }
        const float2 a = acc_a[u], b = acc_b[u];
        const float2 e = make_float2(a.x + b.x, a.y - b.y);
        const float2 d = make_float2(a.x - b.x, a.y + b.y);
        float2 w = twp[k];
        w.y = -w.y;
        const float2 o = fc_cmul(w, d);
        za[k] = make_float2(e.x - o.y, e.y + o.x);
        za[FC_B - k] = make_float2(e.x + o.y, o.x - e.y);
    }
    __syncthreads();
    const float2* z = fc_fft<true>(za, zb, tw);

    const float sc = 1.f / (float)(2 * FC_B);    // a power of two: the halves of the packing and the 1 / B of the inverse, exact
    const float* __restrict__ x_row = x + (size_t)r * row_stride;
    float* __restrict__ o_row = out + (size_t)r * out_stride;
    const bool x_wide = (reinterpret_cast<uintptr_t>(x_row) & 15) == 0, o_wide = (reinterpret_cast<uintptr_t>(o_row) & 15) == 0;   // block-uniform
    float mx = 0.f;
#pragma unroll
    for (int u = 0; u < FC_B / 4 / FC_NT; ++u) {
        const int c = u * FC_NT + threadIdx.x;     // the pack of the block's outputs 4c .. 4c + 3: the samples B + 4c .. of the 2B-point result
        const long t0 = (long)j * FC_B + 4 * c;
        if (t0 >= n_out) continue;
        const float4 c4 = *reinterpret_cast<const float4*>(&z[FC_HALF + 2 * c]);
        const float conv[4] = {c4.x * sc, c4.y * sc, c4.z * sc, c4.w * sc};
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, y[4];
        if (x_wide && t0 + 4 <= n) ld4(x_row + t0, xv);
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (t0 + i < n) xv[i] = x_row[t0 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = fmaf(wet, t0 + i < lead ? 0.f : conv[i], dry * xv[i]);
        if (o_wide && t0 + 4 <= n_out) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, fabsf(y[i]));
            st4(o_row + t0, y);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (t0 + i < n_out) { mx = fmaxf(mx, fabsf(y[i])); o_row[t0 + i] = y[i]; }
        }
    }
    publish_block_max<FC_NT>(mx, block_max + (size_t)r * gridDim.x + j);
}

// ------------------------------------------------------------------------------------------------------------- host: the design
static int fc_design(int64_t n, int64_t m, int rows, int ir_rows, GsFftConv* d) {
    GS_CHECK_ARG(n > 0 && n <= GS_FFTCONV_MAX_N, "fftconv: n must be in [1, 2^40] (got %lld)", (long long)n);
    GS_CHECK_ARG(m > 0, "fftconv: m must be positive (got %lld)", (long long)m);
    GS_CHECK_ARG(m <= GS_FFTCONV_MAX_TAPS, "fftconv: m = %lld taps, more than %d", (long long)m, GS_FFTCONV_MAX_TAPS);
    GS_CHECK_ARG(rows > 0 && rows <= 2, "fftconv: rows must be 1 or 2 (got %d)", rows);
    GS_CHECK_ARG(ir_rows == 1 || ir_rows == rows, "fftconv: ir_rows must be 1 or rows = %d (got %d)", rows, ir_rows);
    const int64_t n_out = n + m - 1;
    const int64_t blocks = (n_out + FC_B - 1) / FC_B, reach = (n - 1) / FC_B + 2;
    d->n = n; d->m = m; d->rows = rows; d->ir_rows = ir_rows; d->block = FC_B;
    d->partitions = (int32_t)((m + FC_B - 1) / FC_B);
    d->blocks = (int32_t)blocks;
    d->x_blocks = (int32_t)(reach < blocks ? reach : blocks);
    return 0;
}

// a caller's descriptor is what fc_design gives for its n, m, rows and ir_rows
static int fc_check(const GsFftConv* c) {
    GS_CHECK_ARG(c != nullptr, "fftconv: null descriptor");
    GsFftConv d;
    const int code = fc_design(c->n, c->m, c->rows, c->ir_rows, &d);
    if (code != 0) return code;
    GS_CHECK_ARG(c->block == d.block && c->partitions == d.partitions && c->blocks == d.blocks && c->x_blocks == d.x_blocks,
                 "fftconv: descriptor (block %d, partitions %d, blocks %d, x_blocks %d) does not follow from its n %lld and m %lld (block %d, "
                 "partitions %d, blocks %d, x_blocks %d)", c->block, c->partitions, c->blocks, c->x_blocks, (long long)c->n, (long long)c->m, d.block,
                 d.partitions, d.blocks, d.x_blocks);
    return 0;
}

static size_t fc_spectrum_bytes(const GsFftConv* c) { return FC_HEAD + (size_t)c->ir_rows * (size_t)c->partitions * FC_B * sizeof(float2); }
static size_t fc_xs_bytes(const GsFftConv* c) { return (size_t)c->rows * (size_t)c->x_blocks * FC_B * sizeof(float2); }

}  // namespace gs

using namespace gs;

extern "C" int gs_fftconv_design(int64_t n, int64_t m, int rows, int ir_rows, GsFftConv* out) {
    GS_CHECK_ARG(out != nullptr, "fftconv_design: null descriptor");
    return fc_design(n, m, rows, ir_rows, out);
}

extern "C" int64_t gs_fftconv_out_len(const GsFftConv* c) {
    const int code = fc_check(c);
    if (code != 0) return code;
    return c->n + c->m - 1;
}

extern "C" size_t gs_fftconv_spectrum_bytes(const GsFftConv* c) {
    if (fc_check(c) != 0) return 0;
    return fc_spectrum_bytes(c);
}

extern "C" size_t gs_fftconv_workspace_bytes(const GsFftConv* c) {
    if (fc_check(c) != 0) return 0;
    return fc_xs_bytes(c) + (size_t)c->rows * (size_t)c->blocks * sizeof(float);
}

extern "C" int gs_fftconv_prepare(const GsFftConv* c, const float* ir, int64_t ir_stride, void* spectrum, size_t spectrum_bytes, void* stream) {
    const int code = fc_check(c);
    if (code != 0) return code;
    GS_CHECK_ARG(ir_stride >= c->m, "fftconv_prepare: ir_stride %lld is below m %lld", (long long)ir_stride, (long long)c->m);
    GS_CHECK_ARG(ir && spectrum, "fftconv_prepare: null pointer (ir and spectrum are required)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(ir) & 3) == 0 && (reinterpret_cast<uintptr_t>(spectrum) & 15) == 0,
                 "fftconv_prepare: misaligned pointer (ir: 4 bytes, spectrum: 16)");
    GS_CHECK_ARG(spectrum_bytes >= fc_spectrum_bytes(c), "fftconv_prepare: spectrum buffer too small (%zu bytes, need %zu)", spectrum_bytes,
                 fc_spectrum_bytes(c));
    hipStream_t st = as_stream(stream);
    float2* tables = static_cast<float2*>(spectrum);
    hipLaunchKernelGGL(fc_tables_kernel, dim3(1), dim3(FC_NT), 0, st, tables);
    hipLaunchKernelGGL(fc_lead_kernel, dim3((unsigned)c->ir_rows), dim3(FC_NT), 0, st, ir, (long)c->m, (long)ir_stride,
                       reinterpret_cast<int*>(static_cast<char*>(spectrum) + FC_LEAD_OFF));
    // partition p of an IR row: its taps [p B, (p + 1) B), then B zeros
    hipLaunchKernelGGL(fc_transform_kernel, dim3((unsigned)c->partitions, (unsigned)c->ir_rows), dim3(FC_NT), 0, st, ir, (long)c->m, (long)ir_stride, 0,
                       FC_B, static_cast<const float2*>(tables), reinterpret_cast<float2*>(static_cast<char*>(spectrum) + FC_HEAD));
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_fftconv(const GsFftConv* c, const void* spectrum, size_t spectrum_bytes, const float* x, int64_t row_stride, float dry, float wet,
                          int normalize, float* out, int64_t out_stride, int16_t* pcm, float* peak, void* ws, size_t ws_bytes, void* stream) {
    const int code = fc_check(c);
    if (code != 0) return code;
    const long n_out = (long)(c->n + c->m - 1);
    GS_CHECK_ARG(row_stride >= c->n, "fftconv: row_stride %lld is below n %lld", (long long)row_stride, (long long)c->n);
    GS_CHECK_ARG(out_stride >= n_out, "fftconv: out_stride %lld is below n_out %ld", (long long)out_stride, n_out);
    GS_CHECK_ARG(x && out && spectrum, "fftconv: null pointer (x, out and spectrum are required)");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(peak) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(pcm) & 1) == 0 && (reinterpret_cast<uintptr_t>(spectrum) & 15) == 0,
                 "fftconv: misaligned pointer (x / out / peak: 4 bytes, pcm: 2, spectrum: 16)");
    GS_CHECK_ARG(spectrum_bytes >= fc_spectrum_bytes(c), "fftconv: spectrum buffer too small (%zu bytes, need %zu)", spectrum_bytes, fc_spectrum_bytes(c));
    const size_t need = gs_fftconv_workspace_bytes(c);
    GS_CHECK_ARG(ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "fftconv: workspace too small or misaligned (%zu bytes, need %zu)",
                 ws_bytes, need);
    hipStream_t st = as_stream(stream);
    float2* xs = static_cast<float2*>(ws);
    float* block_max = reinterpret_cast<float*>(static_cast<char*>(ws) + fc_xs_bytes(c));
    const float2* tables = static_cast<const float2*>(spectrum);
    // block j of a row: its samples [(j - 1) B, (j + 1) B)
    hipLaunchKernelGGL(fc_transform_kernel, dim3((unsigned)c->x_blocks, (unsigned)c->rows), dim3(FC_NT), 0, st, x, (long)c->n, (long)row_stride, -1,
                       2 * FC_B, tables, xs);
    hipLaunchKernelGGL(fc_mac_kernel, dim3((unsigned)c->blocks, (unsigned)c->rows), dim3(FC_NT), 0, st, static_cast<const float2*>(xs), (int)c->x_blocks,
                       tables, (int)c->partitions, c->ir_rows == 1 ? 1 : 0, x, (long)c->n, (long)row_stride, dry, wet, n_out, out, (long)out_stride,
                       block_max);
    if (normalize != 0 || pcm != nullptr || peak != nullptr)
        launch_clip_finish(out, c->rows, 1, n_out, (long)out_stride, reinterpret_cast<short*>(pcm), peak, block_max, c->rows * c->blocks, normalize, st);
    GS_CHECK_LAUNCH();
    return 0;
}
