// Device primitives and geometry shared by the MFMA conv kernels (conv_igemm.hip), the weight-gradient kernels (conv_wgrad.hip) and the VALU
// convs (conv_thin.hip).
#pragma once
#include <type_traits>
#include "conv_shared.h"

namespace gs {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------- MFMA traits
template <typename T> struct Mma;
template <> struct Mma<float> {
    typedef f32x4 frag_t;  // 4 consecutive k for one row; substep e: lanes 0-31 carry k=e, 32-63 carry k=4+e
    __device__ static inline void mma(const frag_t& a, const frag_t& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], c, 0, 0, 0);
    }
};
template <> struct Mma<bf16_t> {
    typedef bf16x8 frag_t;  // 8 consecutive k for one row
    __device__ static inline void mma(const frag_t& a, const frag_t& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

// -------------------------------------------------------------------------- mode geometry
template <int MODE> __host__ __device__ constexpr int patch_dim(int t) {
    return MODE == MODE_S1 ? t + 2 : (MODE == MODE_S2 ? 2 * t + 1 : t + 1);
}
// flat tap i in [0,9) -> kernel row/col, phase, LDS offset inside the patch
template <int MODE> __host__ __device__ constexpr int tap_ky(int i) {
    return MODE == MODE_T2 ? (i < 4 ? (i >> 1) * 2 : (i < 6 ? (i - 4) * 2 : 1)) : i / 3;
}
template <int MODE> __host__ __device__ constexpr int tap_kx(int i) {
    return MODE == MODE_T2 ? (i < 4 ? (i & 1) * 2 : (i < 6 ? 1 : (i < 8 ? (i - 6) * 2 : 1))) : i % 3;
}
template <int MODE> __host__ __device__ constexpr int tap_phase(int i) {
    return MODE == MODE_T2 ? (i < 4 ? 0 : (i < 6 ? 1 : (i < 8 ? 2 : 3))) : 0;
}
template <int MODE> __host__ __device__ constexpr int tap_off(int k) {  // patch offset for kernel index k
    return MODE == MODE_T2 ? (k == 2 ? 0 : 1) : k;
}

// One axis of a tap with the mode at run time (conv_thin.hip): output index o, kernel index k of ks -> the input index i the tap reads; false
// where it reads nothing on this axis (outside the n_in inputs, or, transposed, an output of the other parity -- i is then still d >> 1).
__device__ inline bool tap_input(int mode, int ks, int o, int k, int n_in, int& i) {
    bool ok = true;
    if (mode == MODE_S1) i = o + k - (ks >> 1);
    else if (mode == MODE_S2) i = 2 * o + k;
    else { const int d = o - k; ok = d >= 0 && !(d & 1); i = d >> 1; }
    return ok && i >= 0 && i < n_in;
}

// compile-time loop: f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>)
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

typedef int i32x4 __attribute__((ext_vector_type(4)));

// one LDS-DMA piece: 64 lanes x 16 bytes -> LDS[lds_addr + 16*lane].  M0 is written and consumed inside the statement and
// not restored; it is DECLARED as clobbered, so a compiler use of M0 (v_movrel / s_movrel indexing, LDS-direct) can never straddle a piece.
__device__ __forceinline__ void lds_dma16(unsigned lds_addr, unsigned voff, i32x4 rs) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                 :
                 : "s"(lds_addr), "v"(voff), "s"(rs)
                 : "memory", "m0");
}
// raw buffer descriptor over [base, base + bytes): stride 0, 32-bit data format (gfx950)
__device__ __forceinline__ i32x4 make_rsrc(const void* base, unsigned bytes) {
    const unsigned long long b = reinterpret_cast<unsigned long long>(base);
    i32x4 rs;
    rs[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
    rs[1] = __builtin_amdgcn_readfirstlane((int)((b >> 32) & 0xffffu));
    rs[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    rs[3] = 0x00020000;
    return rs;
}
// s_waitcnt vmcnt(n) with n known only after unrolling (the asm immediate must be a literal)
__device__ __forceinline__ void wait_vmcnt(int n) {
#define GS_VM(K) case K: asm volatile("s_waitcnt vmcnt(" #K ")" ::: "memory"); break;
    switch (n) {
        GS_VM(0) GS_VM(1) GS_VM(2) GS_VM(3) GS_VM(4) GS_VM(5) GS_VM(6) GS_VM(7) GS_VM(8) GS_VM(9) GS_VM(10) GS_VM(11)
        GS_VM(12) GS_VM(13) GS_VM(14) GS_VM(15) GS_VM(16) GS_VM(17) GS_VM(18) GS_VM(19) GS_VM(20) GS_VM(21) GS_VM(22)
        GS_VM(23) GS_VM(24) GS_VM(25) GS_VM(26) GS_VM(27) GS_VM(28) GS_VM(29) GS_VM(30) GS_VM(31) GS_VM(32)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef GS_VM
}
__device__ __forceinline__ void block_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// compute units of the current device (host side; each file that includes this asks once)
static int g_num_cus = 0;
static int num_cus() {
    if (g_num_cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            g_num_cus = n;
        else
            g_num_cus = 256;
    }
    return g_num_cus;
}

}  // namespace gs
