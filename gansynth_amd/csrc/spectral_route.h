// Which kernels a spectral call runs: ONE host function, spectral_route, read by gs_spectral_plan_create, the launchers of spectral.hip
// and spectral_wave.hip, the workspace queries and the host-only query gs_spectral_route.  Nobody decides a second time.
// Host arithmetic only: no HIP call, so it answers on a machine without a device.
#pragma once
#include <stdlib.h>
#include <string.h>

#include "../../include/gansynth_hip.h"

namespace gs {

#ifndef SW_WAVES
#define SW_WAVES 12         // waves per block = per CU of the wave-per-frame kernels (spectral_wave.hip, where the measurements are)
#endif                      // (another value: -DSW_WAVES=n through GS_EXTRA_FLAGS, so that both translation units that include this see it)

// run lengths of the mel columns per 128-column block that stft_wave_kernel's gather is unrolled for (SW_SHAPE there)
static const int SW_SHAPE_HOST[8] = {1, 1, 2, 2, 3, 3, 4, 6};

// What the route needs to know of a dense mel matrix [H][H] (linear bin major)
struct SpectralMel {
    int maxnz;     // non-zeros of the fullest column (>= 1)
    int one_run;   // 1024 bins: every column's non-zeros lie within 8 consecutive linear bins
    int cnt[8];    // 1024 bins and one_run: longest such span per 128-column block (>= 1), else 0
};

inline SpectralMel spectral_mel_digest(const float* mel_dense, int H) {
    SpectralMel d;
    d.maxnz = 1; d.one_run = 0;
    for (int j = 0; j < 8; ++j) d.cnt[j] = 0;
    for (int m = 0; m < H; ++m) { int c = 0; for (int f = 0; f < H; ++f) if (mel_dense[(long)f * H + m] != 0.f) ++c; if (c > d.maxnz) d.maxnz = c; }
    if (H != 1024) return d;
    int len[1024];
    bool ok = true;
    for (int m = 0; m < H && ok; ++m) {
        int first = -1, last = -1;
        for (int f = 0; f < H; ++f) if (mel_dense[(long)f * H + m] != 0.f) { if (first < 0) first = f; last = f; }
        len[m] = first < 0 ? 0 : last - first + 1;
        ok = len[m] <= 8;
    }
    if (!ok) return d;
    d.one_run = 1;
    for (int j = 0; j < 8; ++j) {
        int c = 1;
        for (int m = 128 * j; m < 128 * (j + 1); ++m) c = len[m] > c ? len[m] : c;
        d.cnt[j] = c;
    }
    return d;
}

// the measurement knobs, from the environment; the seven of the inverse path are read once per process
inline GsSpectralKnobs spectral_knobs_env() {
    static const GsSpectralKnobs inverse = [] {
        GsSpectralKnobs k;
        k.generic = 0;
        k.fp32_gemm = getenv("GS_INVERSE_FP32_GEMM") != nullptr;        // the exact-fp32 MFMA kernel
        k.mag_6terms = getenv("GS_INVERSE_MAG_6TERMS") != nullptr;      // six terms for the magnitude rows too
        k.gemm_256 = getenv("GS_INVERSE_GEMM_256") != nullptr;          // 128 x 256 tiles, one block per CU
        k.gemm_kb = getenv("GS_INVERSE_GEMM_KB") ? atoi(getenv("GS_INVERSE_GEMM_KB")) : 4;
        k.gemm_kb3 = getenv("GS_INVERSE_GEMM_KB3") ? atoi(getenv("GS_INVERSE_GEMM_KB3")) : 2;
        k.block_fft = getenv("GS_INVERSE_BLOCK_FFT") != nullptr;        // the block-per-frame radix-2 kernel
        k.separate_ola = getenv("GS_INVERSE_SEPARATE_OLA") != nullptr;  // frames through memory + the gather kernel
        return k;
    }();
    GsSpectralKnobs k = inverse;
    k.generic = getenv("GS_SPECTRAL_GENERIC") != nullptr;               // read when a plan is created: the plan keeps it
    return k;
}

// runs per example: enough wave-runs to fill SW_WAVES waves on every CU (a run of R frames costs R + 1 transforms), at most one per frame
inline int runs_per_example(int batch, int time_steps) {
    int runs = (256 * SW_WAVES + batch - 1) / batch;
    if (runs > time_steps) runs = time_steps;
    if (runs < 1) runs = 1;
    if (runs >= SW_WAVES) runs -= runs % SW_WAVES;   // whole blocks per example: neighbouring runs exchange their edge phases in the block
    return runs;
}

// batch <= 0: only the fields a plan fixes (forward kind, ELL width, mel_cnt) are filled
inline GsSpectralRoute spectral_route(int frame_length, int frame_step, int time_steps, const SpectralMel& mel, bool has_pinv, int batch,
                                      int wave_len, int front_pad, int dtype, size_t fwd_ws_bytes, const GsSpectralKnobs& k) {
    (void)dtype;   // (fp32 and bf16 images take the same route: the instantiation's T)
    GsSpectralRoute r;
    memset(&r, 0, sizeof(r));
    const int H = frame_length / 2;
    // ---- forward
    r.maxnz = mel.maxnz;
    if (r.maxnz <= 8) r.maxnz = (r.maxnz + 1) & ~1;   // even widths have an unrolled kernel instantiation (padding = weight 0 on bin 0)
    r.mz = r.maxnz <= 8 ? r.maxnz : 0;
    for (int j = 0; j < 8; ++j) r.mel_cnt[j] = mel.cnt[j];
    // wave-per-frame path (spectral_wave.hip): every mel column's non-zeros must be ONE run of linear bins, the longest run of each
    // 128-column block as in the reference configuration (the kernel's gather is unrolled for that shape)
    bool wave = H == 1024 && !k.generic && mel.one_run;
    for (int j = 0; j < 8 && wave; ++j) wave = mel.cnt[j] == SW_SHAPE_HOST[j];
    r.fwd_kind = wave ? GS_SPEC_FWD_WAVE : GS_SPEC_FWD_GENERIC;
    if (batch <= 0) return r;
    if (wave) {
        r.runs = runs_per_example(batch, time_steps);
        r.q = time_steps / r.runs;
        r.rem = time_steps % r.runs;
        r.span_examples = r.runs < SW_WAVES;
        r.fwd_workspace_bytes = (int64_t)batch * r.runs * 1024 * sizeof(float);   // the mel phases stay in registers; 4 KB per run for the run-edge exchange
        r.exchange = r.runs % SW_WAVES == 0 && fwd_ws_bytes >= (size_t)r.fwd_workspace_bytes;   // (no scratch: every run recomputes its lead frame)
    } else {
        r.fwd_workspace_bytes = (int64_t)batch * time_steps * H * sizeof(float);
    }
    if (!has_pinv) return r;
    // ---- inverse: [mel_mag; mel_phase] @ pinv(mel), 2 x rows stacked
    const long rows = (long)batch * time_steps;
    const bool split = (2 * rows) % 128 == 0 && H % 128 == 0 && !k.fp32_gemm;
    const bool two = split && rows % 128 == 0 && !k.mag_6terms;   // magnitude rows [0, rows): two planes, three terms
    auto launch = [&](int i, int nj, int np, int kb) { r.gemm_nj[i] = nj; r.gemm_np[i] = np; r.gemm_kb[i] = kb; r.gemm_launches = i + 1; };
    if (split && k.gemm_256 && H % 256 == 0) {
        r.gemm_kind = GS_SPEC_GEMM_WIDE_256;
        if (two) { launch(0, 4, 2, 2); launch(1, 4, 3, 2); }
        else launch(0, 4, 3, 2);
    } else if (two) {
        r.gemm_kind = GS_SPEC_GEMM_SPLIT_TWO;
        launch(0, 2, 2, k.gemm_kb == 4 ? 4 : 2);
        launch(1, 2, 3, k.gemm_kb3 == 4 ? 4 : 2);
    } else if (split) {
        r.gemm_kind = GS_SPEC_GEMM_SPLIT_ALL;
        launch(0, 2, 3, 2);
    } else {
        r.gemm_kind = (2 * rows) % 128 == 0 && H % 128 == 0 ? GS_SPEC_GEMM_F32_128 : GS_SPEC_GEMM_F32_64;
        r.gemm_launches = 1;
    }
    // frames of a whole example per block, overlap-add and crop included: needs >= 3 frames per run and even crop offsets
    const bool ola_ok = frame_length == 2048 && frame_step == 512 && time_steps >= 3 * SW_WAVES && (wave_len & 1) == 0 && (front_pad & 1) == 0;
    if (wave && !k.block_fft && !k.separate_ola && ola_ok) r.istft_kind = GS_SPEC_ISTFT_WAVE_OLA;
    else if (wave && !k.block_fft) r.istft_kind = GS_SPEC_ISTFT_WAVE_FRAMES;
    else r.istft_kind = GS_SPEC_ISTFT_BLOCK_FFT;
    return r;
}

}  // namespace gs
