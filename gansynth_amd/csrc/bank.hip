// Resident notes: one batch of waveforms and one-hot labels drawn from the int16 bank on the device (gansynth_amd/bank.py; the rules
// are stated in include/gansynth_hip.h and DESIGN.md "Resident notes").
//
// A plain streaming kernel: 2 bytes read and 4 written per sample, nothing shared between lanes.  The grid is one-dimensional,
// `chunks` blocks per batch row; a block owns BANK_NT * PER consecutive samples of its row (PER = 8: one 16-byte load and two 16-byte
// stores per lane; PER = 1: the scalar path for geometry that is not 16-byte aligned).  The first block of a row also writes the row's
// label.  With waves == NULL the grid is one block per row and only labels are written.  The int16 -> float conversion and the
// multiplication by 2^-15 are exact, so the result does not depend on the path.
#include "gs_common.h"

namespace gs {

constexpr int BANK_NT = 256;   // threads per block

// grid (batch * chunks).  PER samples per lane
template <int PER>
__global__ __launch_bounds__(BANK_NT) void bank_gather_kernel(const short* __restrict__ pcm, long rows, long length, long row_stride,
                                                              const int* __restrict__ class_of_row, const int* __restrict__ order,
                                                              int chunks, int n_classes, float* __restrict__ waves,
                                                              float* __restrict__ labels) {
    const long b = (long)(blockIdx.x / (unsigned)chunks);
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const long r = (long)order[b];                       // (order already points at the batch's first entry)
    const bool have = r >= 0 && r < rows;                // block-uniform
    if (chunk == 0) {
        const int cls = have ? class_of_row[r] : -1;
        float* __restrict__ lab = labels + b * (long)n_classes;
        for (int c = threadIdx.x; c < n_classes; c += BANK_NT) lab[c] = c == cls ? 1.f : 0.f;
    }
    if (waves == nullptr) return;
    const long i = ((long)chunk * BANK_NT + threadIdx.x) * PER;
    if (i >= length) return;                             // PER == 8: length % 8 == 0, so i + 8 <= length
    float* __restrict__ dst = waves + b * length + i;
    if (PER == 8) {
        float v[8];
        if (have) {
            const uint4 q = *reinterpret_cast<const uint4*>(pcm + r * row_stride + i);
            const unsigned int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[2 * k] = (float)(short)(w[k] & 0xffffu) * 0x1p-15f;
                v[2 * k + 1] = (float)(short)(w[k] >> 16) * 0x1p-15f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = 0.f;
        }
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        *dst = have ? (float)pcm[r * row_stride + i] * 0x1p-15f : 0.f;
    }
}

}  // namespace gs

using namespace gs;

extern "C" int gs_bank_gather(const int16_t* pcm, int64_t rows, int64_t length, int64_t row_stride, const int32_t* class_of_row,
                              const int32_t* order, int64_t n_order, int64_t first, int batch, int n_classes, float* waves, float* labels,
                              void* stream) {
    GS_CHECK_ARG(pcm != nullptr, "bank_gather: pcm is null");
    GS_CHECK_ARG(class_of_row != nullptr, "bank_gather: class_of_row is null");
    GS_CHECK_ARG(order != nullptr, "bank_gather: order is null");
    GS_CHECK_ARG(labels != nullptr, "bank_gather: labels is null");
    GS_CHECK_ARG(rows > 0, "bank_gather: rows must be positive (got %lld)", (long long)rows);
    GS_CHECK_ARG(length > 0, "bank_gather: length must be positive (got %lld)", (long long)length);
    GS_CHECK_ARG(batch > 0, "bank_gather: batch must be positive (got %d)", batch);
    GS_CHECK_ARG(n_classes > 0, "bank_gather: n_classes must be positive (got %d)", n_classes);
    GS_CHECK_ARG(row_stride >= length, "bank_gather: row_stride %lld is below length %lld", (long long)row_stride, (long long)length);
    GS_CHECK_ARG(first >= 0 && first <= n_order && (int64_t)batch <= n_order - first,
                 "bank_gather: first %lld + batch %d is outside the n_order %lld entries", (long long)first, batch, (long long)n_order);
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(pcm) & 1) == 0, "bank_gather: pcm is not 2-byte aligned");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(waves) & 3) == 0, "bank_gather: waves is not 4-byte aligned");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(labels) & 3) == 0, "bank_gather: labels is not 4-byte aligned");
    GS_CHECK_ARG((reinterpret_cast<uintptr_t>(class_of_row) & 3) == 0 && (reinterpret_cast<uintptr_t>(order) & 3) == 0,
                 "bank_gather: class_of_row / order is not 4-byte aligned");
    const bool wide = waves != nullptr && length % 8 == 0 && row_stride % 8 == 0 && (reinterpret_cast<uintptr_t>(pcm) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(waves) & 15) == 0;
    const int64_t per_block = (int64_t)BANK_NT * (wide ? 8 : 1);
    const int64_t chunks = waves == nullptr ? 1 : (length + per_block - 1) / per_block;
    GS_CHECK_ARG(chunks * (int64_t)batch <= 0x7fffffffLL, "bank_gather: batch %d x length %lld is too large for one launch", batch,
                 (long long)length);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(chunks * batch));
    const short* p = reinterpret_cast<const short*>(pcm);
    if (wide)
        hipLaunchKernelGGL(bank_gather_kernel<8>, grid, dim3(BANK_NT), 0, st, p, (long)rows, (long)length, (long)row_stride, class_of_row,
                           order + first, (int)chunks, n_classes, waves, labels);
    else
        hipLaunchKernelGGL(bank_gather_kernel<1>, grid, dim3(BANK_NT), 0, st, p, (long)rows, (long)length, (long)row_stride, class_of_row,
                           order + first, (int)chunks, n_classes, waves, labels);
    GS_CHECK_LAUNCH();
    return 0;
}
