"""ctypes binding of libgansynth_hip.so (C ABI declared in include/gansynth_hip.h).

Fails loudly: if the shared library has not been built (`python -c 'import __graft_entry__ as g;
g.build()'` or gansynth_amd/csrc/build.sh) loading raises -- there is no fallback path.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgansynth_hip.so")

GS_F32, GS_BF16 = 0, 1
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
ACT_LRELU_BITS, ACT_WRITE_BITS = 5, 16   # include/gansynth_hip.h: 1-bit leaky-relu masks
PREP_CONV_FWD, PREP_CONV_BWD_DATA, PREP_CONVT_FWD, PREP_CONVT_BWD_DATA = 0, 1, 2, 3
CONV_FWD, CONV_BWD_DATA, CONV_BWD_WEIGHT = 0, 1, 2

P, I, F, L, Z = c_void_p, c_int, c_float, c_int64, c_size_t


class GsConv(ctypes.Structure):
    """include/gansynth_hip.h: one conv / transposed-conv LAYER in its own forward labelling, whichever of its maps is asked for."""
    _fields_ = [("n", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("ci", ctypes.c_int32), ("co", ctypes.c_int32),
                ("ksize", ctypes.c_int32), ("stride", ctypes.c_int32), ("transposed", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("w_prepared", ctypes.c_int32), ("alpha", c_float), ("ws", c_void_p), ("ws_bytes", c_size_t)]


C = POINTER(GsConv)


class GsDense(ctypes.Structure):
    """include/gansynth_hip.h: one dense LAYER, whichever of its maps is asked for; c, hw != 0: a channels-last input side."""
    _fields_ = [("b", ctypes.c_int32), ("inp", ctypes.c_int32), ("out", ctypes.c_int32), ("c", ctypes.c_int32), ("hw", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("alpha", c_float), ("ws", c_void_p), ("ws_bytes", c_size_t)]


D = POINTER(GsDense)


class GsSpectralKnobs(ctypes.Structure):
    """include/gansynth_hip.h: the measurement switches of the spectral kernels (GS_SPECTRAL_GENERIC, GS_INVERSE_*)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("generic", "fp32_gemm", "mag_6terms", "gemm_256", "gemm_kb", "gemm_kb3", "block_fft", "separate_ola")]


class GsSpectralRoute(ctypes.Structure):
    """include/gansynth_hip.h: which kernels a spectral call runs (gs_spectral_route)."""
    _fields_ = [("fwd_workspace_bytes", ctypes.c_int64), ("fwd_kind", ctypes.c_int32), ("maxnz", ctypes.c_int32), ("mz", ctypes.c_int32),
                ("mel_cnt", ctypes.c_int32 * 8), ("runs", ctypes.c_int32), ("q", ctypes.c_int32), ("rem", ctypes.c_int32),
                ("exchange", ctypes.c_int32), ("span_examples", ctypes.c_int32), ("gemm_kind", ctypes.c_int32), ("gemm_launches", ctypes.c_int32),
                ("gemm_nj", ctypes.c_int32 * 2), ("gemm_np", ctypes.c_int32 * 2), ("gemm_kb", ctypes.c_int32 * 2), ("istft_kind", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class GsResample(ctypes.Structure):
    """include/gansynth_hip.h: the design of one rate conversion (gs_resample_design fills it)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("rate_in", "rate_out", "up", "down", "taps", "zeros")]


R = POINTER(GsResample)
RESAMPLE_TILE = 512   # GS_RESAMPLE_TILE: output samples per block of gs_resample's filter


class GsFftConv(ctypes.Structure):
    """include/gansynth_hip.h: the design of one partitioned FFT convolution (gs_fftconv_design fills it)."""
    _fields_ = [("n", ctypes.c_int64), ("m", ctypes.c_int64)] + [(n, ctypes.c_int32) for n in ("rows", "ir_rows", "block", "partitions", "blocks", "x_blocks")]


V = POINTER(GsFftConv)
FFTCONV_BLOCK = 2048                                              # GS_FFTCONV_BLOCK: new samples per block of gs_fftconv
FFTCONV_MAX_TAPS = 1 << 20                                        # GS_FFTCONV_MAX_TAPS
FFTCONV_HEADER_BYTES = (FFTCONV_BLOCK + FFTCONV_BLOCK // 2 + 8) * 8 + 16   # GS_FFTCONV_HEADER_BYTES
LIMIT_MAX_LOOKAHEAD = 2048                                        # GS_LIMIT_MAX_LOOKAHEAD: samples
LIMIT_TILE = 4096                                                 # GS_LIMIT_TILE: samples per block of gs_limit
TRUE_PEAK_TILE, TRUE_PEAK_TAPS, TRUE_PEAK_OVERSAMPLE = 2048, 68, 4   # GS_TRUE_PEAK_TILE, GS_TRUE_PEAK_TAPS, GS_TRUE_PEAK_OVERSAMPLE
KMEANS_MAX_K, KMEANS_TILE, KMEANS_MAX_SLICES, KMEANS_MAX_N, KMEANS_MAX_D = 256, 256, 512, 2 ** 31 - 1, 1 << 20   # GS_KMEANS_MAX_K, _TILE, _MAX_SLICES, _MAX_N, _MAX_D
SWD_DESC, SWD_PATCHES, SWD_SORT_TILE, SWD_MAX_N, SWD_MAX_ROWS, SWD_MAX_SIDE, SWD_MAX_BATCH = 98, 128, 4096, 1 << 21, 65535, 16384, 65536   # GS_SWD_*
SWD_STAGE_PYRAMID, SWD_STAGE_MOMENTS, SWD_STAGE_SORT, SWD_STAGE_L1 = range(4)   # GS_SWD_STAGE_*
KNN_MAX_K, KNN_BLOCKS, KNN_MIN_SLICE_ROWS = 8, 3072, 256   # GS_KNN_MAX_K, _BLOCKS, _MIN_SLICE_ROWS
KID_TILE, KID_MAX_ROWS, KID_MAX_SUBSETS = 128, 1 << 21, 65535   # GS_KID_TILE, _MAX_ROWS, _MAX_SUBSETS
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE = 8000, 192000              # GS_LOUDNESS_MIN_RATE, GS_LOUDNESS_MAX_RATE
LOUDNESS_STEPS = 8                                                # GS_LOUDNESS_STEPS: matrix powers per scan of gs_loudness


class GsLoudness(ctypes.Structure):
    """include/gansynth_hip.h: the K-weighting meter of one sample rate (gs_loudness_design fills it)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("rate", "hop", "chunk", "lanes", "rem", "reserved")] + \
               [(n, c_double * 3) for n in ("b1", "a1", "b2", "a2")] + \
               [("chunk_pow", c_double * 16 * LOUDNESS_STEPS), ("hop_pow", c_double * 16 * LOUDNESS_STEPS), ("rem_pow", c_double * 16)]


W = POINTER(GsLoudness)


SPEC_FWD_GENERIC, SPEC_FWD_WAVE = 0, 1                                                                        # GS_SPEC_FWD_*
SPEC_GEMM_NONE, SPEC_GEMM_F32_64, SPEC_GEMM_F32_128, SPEC_GEMM_SPLIT_ALL, SPEC_GEMM_SPLIT_TWO, SPEC_GEMM_WIDE_256 = range(6)   # GS_SPEC_GEMM_*
SPEC_ISTFT_NONE, SPEC_ISTFT_WAVE_OLA, SPEC_ISTFT_WAVE_FRAMES, SPEC_ISTFT_BLOCK_FFT = range(4)                # GS_SPEC_ISTFT_*

# name -> (restype, argtypes); every symbol include/gansynth_hip.h declares
SIGNATURES = {
    "gs_last_error": (c_char_p, []),
    "gs_version": (I, []),
    "gs_init": (I, []),
    "gs_streams_create": (I, [I, POINTER(P)]),
    "gs_streams_destroy": (I, [I, POINTER(P)]),
    "gs_prof_enable": (I, [I]),
    "gs_prof_collect": (I, [POINTER(c_int), POINTER(c_double), POINTER(c_double)]),
    "gs_prof_roofline": (I, [ctypes.c_double, ctypes.c_double, P, P, P]),
    "gs_prof_records": (I, [I, P, P, P, P, P]),
    "gs_comm_available": (I, []),
    "gs_comm_unique_id": (I, [P]),
    "gs_comm_init": (I, [POINTER(P), I, I, P]),
    "gs_comm_destroy": (I, [P]),
    "gs_comm_count": (I, [P, POINTER(I)]),
    "gs_allreduce_sum_f32": (I, [P, P, ctypes.c_int64, P]),
    "gs_comm_set_marker_us": (I, [P, ctypes.c_double]),
    "gs_broadcast_f32": (I, [P, P, ctypes.c_int64, I, P]),
    # conv entry points: C = POINTER(GsConv), the layer (include/gansynth_hip.h)
    "gs_conv_workspace_bytes": (Z, [C, I]),
    "gs_conv_fwd": (I, [C, P, P, P, I, P, P, F, P]),
    "gs_conv_fwd_mask": (I, [C, P, P, P, I, P, P]),
    "gs_conv_bwd_data": (I, [C, P, P, P, I, P, P]),
    "gs_conv_bwd_data_pnbwd": (I, [C, P, P, P, P, I, F, P, P]),
    "gs_conv_bwd_data_pnbwd_is_fused": (I, [C]),
    "gs_conv_fwd_pnbwdbwd": (I, [C, P, P, P, P, I, F, P, P, P]),
    "gs_conv_fwd_pnbwdbwd_is_fused": (I, [C]),
    "gs_conv_bwd_weight": (I, [C, P, P, P, P, I, P]),
    "gs_conv_wgrad_jobs_workspace_bytes": (Z, [P, I]),
    "gs_conv_wgrad_jobs": (I, [P, I, P, Z, P]),
    "gs_wgrad_cu_cap": (I, [I]),
    "gs_conv_wgrad_plan": (I, [C, POINTER(c_int)]),
    "gs_conv_wgrad_jobs_plan": (I, [P, I, POINTER(c_int), I]),
    "gs_conv_igemm_config": (I, [I, I, I, I, I, I, I, I, POINTER(c_int)]),
    "gs_conv_igemm_table": (I, [I, POINTER(c_int)]),
    "gs_conv_thin_route": (I, [C, I, I, I, I, I, I, POINTER(c_int), POINTER(c_int)]),
    "gs_units_bias_act_to_nhwc": (I, [P, P, P, P, I, I, I, I, I, P]),
    "gs_nhwc_act_bwd_to_units": (I, [P, P, P, I, I, I, I, I, P]),
    # dense entry points: D = POINTER(GsDense), the layer
    "gs_dense_fwd_workspace_bytes": (Z, [D]),
    "gs_dense_fwd": (I, [D, P, P, P, I, P, P]),
    "gs_dense_bwd_data": (I, [D, P, P, P, P]),
    "gs_dense_bwd_weight": (I, [D, P, P, P, I, P]),
    "gs_dense_route": (I, [D, I, I, POINTER(c_int)]),
    "gs_embedding_fwd": (I, [P, P, P, I, I, I, F, I, P]),
    "gs_embedding_onehot_fwd": (I, [P, P, P, P, I, I, I, F, I, P]),
    "gs_embedding_bwd": (I, [P, P, P, I, I, I, F, I, P]),
    "gs_bias_act_fwd": (I, [P, P, P, L, I, I, I, P]),
    "gs_act_bwd": (I, [P, P, P, L, I, I, P]),
    "gs_act_bwd_bias": (I, [P, P, P, P, L, I, I, I, I, P, Z, P]),
    "gs_tanh_bwd_bwd": (I, [P, P, P, P, L, I, P]),
    "gs_channel_sum_workspace_bytes": (Z, [L, I]),
    "gs_channel_sum": (I, [P, P, L, I, I, I, P, Z, P]),
    "gs_bias_partial_rows": (I, [I, L, I, I]),
    "gs_channel_fold_batch_workspace_bytes": (Z, [P, I]),
    "gs_channel_fold_batch": (I, [P, I, P, Z, P]),
    "gs_pixel_norm_fwd": (I, [P, P, L, I, F, I, P]),
    "gs_pixel_norm_bwd_fused": (I, [P, P, P, P, L, I, F, I, I, I, P]),
    "gs_pixel_norm_bwd_bias_workspace_bytes": (Z, [L, I, I]),
    "gs_pixel_norm_bwd_fused_bias": (I, [P, P, P, P, P, L, I, F, I, I, I, I, P, Z, P]),
    "gs_pixel_norm_bwd_bwd_fused": (I, [P, P, P, P, P, L, I, F, I, I, P]),
    "gs_upscale2d": (I, [P, P, I, I, I, I, I, I, F, I, P]),
    "gs_blocksum2d": (I, [P, P, I, I, I, I, I, I, F, I, P]),
    "gs_batch_stddev_fwd": (I, [P, P, I, I, I, F, I, P]),
    "gs_batch_stddev_bwd": (I, [P, P, P, P, I, I, I, F, I, P]),
    "gs_batch_stddev_bwd_bwd": (I, [P, P, P, P, P, I, I, I, F, I, P]),
    "gs_axpby": (I, [P, P, P, L, F, F, I, P]),
    "gs_axpby_dev": (I, [P, P, P, L, P, I, I, I, P]),
    "gs_sumsq_rows_workspace_bytes": (Z, [I]),
    "gs_sumsq_rows": (I, [P, P, I, L, I, P, Z, P]),
    "gs_row_scale": (I, [P, P, F, P, I, L, I, P]),
    "gs_elementwise_route": (I, [I, I, L, I, I, I, I, I, POINTER(c_int)]),
    "gs_weight_prep_batch": (I, [P, I, P]),
    "gs_gan_d_loss": (I, [P, P, P, P, F, I, I, P, P, P, P, I, P]),
    "gs_gan_g_loss": (I, [P, P, P, F, F, I, I, P, P, P, I, P]),
    "gs_adam_tf_step": (I, [P, P, P, P, L, F, F, F, F, F, P]),
    "gs_adam_tf_step_zero_grad": (I, [P, P, P, P, L, F, F, F, F, F, P]),
    "gs_adam_tf_step_dev": (I, [P, P, P, P, L, P, F, F, F, F, I, P]),
    "gs_ema_step": (I, [P, P, L, F, P]),
    "gs_ema_step_dev": (I, [P, P, L, P, P]),
    "gs_swap_f32": (I, [P, P, L, P]),
    "gs_pack_act_bits": (I, [P, L, I, I, P]),
    "gs_spectral_plan_create": (I, [POINTER(c_void_p), I, I, I, P, P]),
    "gs_spectral_plan_destroy": (I, [P]),
    "gs_stft_fwd": (I, [P, P, I, I, I, P, P, P]),
    "gs_mel_project": (I, [P, P, P, L, P]),
    "gs_if_unwrap": (I, [P, P, P, I, P]),
    "gs_stft_mel_if_fwd": (I, [P, P, I, I, I, P, I, P, Z, P]),
    "gs_stft_mel_if_workspace_bytes": (Z, [P, I]),
    "gs_mel_if_to_waveform": (I, [P, P, I, I, I, P, I, P, Z, P]),
    "gs_mel_if_to_waveform_workspace_bytes": (Z, [P, I]),
    "gs_spectral_route": (I, [I, I, I, P, I, I, I, I, I, I, Z, POINTER(GsSpectralKnobs), POINTER(GsSpectralRoute)]),
    "gs_weight_standardize": (I, [P, P, I, I, F, P]),
    "gs_resnet_stem_pool": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "gs_max_pool2d": (I, [P, P, I, I, I, I, I, P]),
    "gs_conv1x1_fwd": (I, [P, P, P, I, I, I, I, I, I, I, P]),
    "gs_group_norm_workspace_bytes": (Z, [I, I, I, I]),
    "gs_group_norm_stats": (I, [P, P, P, P, I, I, I, I, F, I, P, Z, P]),
    "gs_group_norm_apply": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
    "gs_group_norm_relu_mean": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "gs_group_norm_bwd_workspace_bytes": (Z, [I, I, I, I]),
    "gs_group_norm_relu_bwd": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, Z, P]),
    "gs_group_norm_relu_mean_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, Z, P]),
    "gs_weight_standardize_batch": (I, [P, I, I, F, P]),
    "gs_weight_standardize_bwd_batch": (I, [P, I, I, P]),
    "gs_max_pool2d_bwd": (I, [P, P, P, I, I, I, I, I, P]),
    "gs_resnet_stem_bwd_weight_workspace_bytes": (Z, [I, I, I]),
    "gs_resnet_stem_bwd_weight": (I, [P, P, P, P, I, I, I, I, I, I, P, Z, P]),
    "gs_conv1x1_bwd_data": (I, [P, P, P, I, I, I, I, I, I, I, I, P]),
    "gs_conv1x1_bwd_weight_workspace_bytes": (Z, [I, I, I, I, I, I]),
    "gs_conv1x1_bwd_weight": (I, [P, P, P, I, I, I, I, I, I, I, I, P, Z, P]),
    "gs_softmax_xent": (I, [P, P, P, P, P, I, I, P]),
    "gs_momentum_workspace_bytes": (Z, [L]),
    "gs_momentum_tf_step": (I, [P, P, P, L, L, L, F, F, F, I, I, P, P, Z, P]),
    "gs_summary_image_u8_workspace_bytes": (Z, [I, L, I]),
    "gs_summary_image_u8": (I, [P, P, I, L, I, I, P, Z, P]),
    "gs_summary_audio_s16": (I, [P, P, I, L, L, I, P]),
    "gs_note_mix_workspace_bytes": (Z, [L]),
    "gs_note_mix": (I, [P, I, L, L, P, I, L, I, P, P, P, P, Z, P]),
    "gs_note_mix_stereo_workspace_bytes": (Z, [L]),
    "gs_note_mix_stereo": (I, [P, I, L, L, P, I, L, I, P, L, P, P, P, Z, P]),
    "gs_note_mix_curves_workspace_bytes": (Z, [L]),
    "gs_note_mix_curves": (I, [P, I, L, L, P, I, P, I, P, I, I, L, I, P, L, P, P, P, Z, P]),
    "gs_note_warp_table_bytes": (Z, []),
    "gs_note_warp_table": (I, [P]),
    "gs_note_warp": (I, [P, I, L, L, P, I, P, P, I, I, P, P]),
    "gs_loop_search": (I, [P, I, L, L, P, I, P, L, P]),
    "gs_note_sustain": (I, [P, I, L, L, P, I, P]),
    "gs_stereo_finish_workspace_bytes": (Z, [L]),
    "gs_stereo_finish": (I, [P, L, L, I, P, P, P, Z, P]),
    "gs_bank_gather": (I, [P, L, L, L, P, P, L, L, I, I, P, P, P]),
    # R = POINTER(GsResample), the design of one (rate_in, rate_out)
    "gs_resample_design": (I, [I, I, R]),
    "gs_resample_out_len": (L, [R, L]),
    "gs_resample_table_bytes": (Z, [R, I]),
    "gs_resample_table": (I, [R, I, P]),
    "gs_resample_workspace_bytes": (Z, [R, I, L]),
    "gs_resample": (I, [R, P, P, I, L, L, I, P, P, P, P, Z, P]),
    # V = POINTER(GsFftConv), the design of one (n, m, rows, ir_rows)
    "gs_fftconv_design": (I, [L, L, I, I, V]),
    "gs_fftconv_out_len": (L, [V]),
    "gs_fftconv_spectrum_bytes": (Z, [V]),
    "gs_fftconv_workspace_bytes": (Z, [V]),
    "gs_fftconv_prepare": (I, [V, P, L, P, Z, P]),
    "gs_fftconv": (I, [V, P, Z, P, L, F, F, I, P, L, P, P, P, Z, P]),
    "gs_limit_workspace_bytes": (Z, [I, L]),
    "gs_limit": (I, [P, I, L, L, F, F, I, P, L, P, P, P, P, Z, P]),
    "gs_limit_env": (I, [P, P, I, L, L, F, F, I, P, L, P, P, P, P, Z, P]),
    "gs_true_peak_workspace_bytes": (Z, [I, L]),
    "gs_true_peak": (I, [P, P, I, L, L, P, P, P, Z, P]),
    "gs_kmeans_workspace_bytes": (Z, [L, I, I]),
    "gs_kmeans_assign": (I, [P, L, L, I, P, I, P, P, P, P, P, Z, P]),
    "gs_kmeans_inertia": (I, [P, L, L, I, P, I, P, P, P, Z, P]),
    "gs_kmeans_update": (I, [P, L, L, I, P, I, P, P, P, Z, P]),
    "gs_kmeans_mindist": (I, [P, L, L, I, P, P, I, P]),
    "gs_swd_levels": (I, [I, I]),
    "gs_swd_workspace_bytes": (Z, [I, L, L, L]),
    "gs_swd_pyramid": (I, [P, I, L, I, I, P, P, Z, P]),
    "gs_swd_patches": (I, [P, L, I, I, P, P, P, L, L, P]),
    "gs_swd_moments": (I, [P, L, P, P, Z, P]),
    "gs_swd_project": (I, [P, L, P, P, I, P, P]),
    "gs_swd_sort": (I, [P, L, L, P, Z, P]),
    "gs_swd_l1": (I, [P, P, L, L, P, P, Z, P]),
    "gs_knn_workspace_bytes": (Z, [L, L, I, I]),
    "gs_knn_slices": (I, [L, L, I]),
    "gs_knn_kth": (I, [P, L, L, P, L, L, I, I, I, P, P, Z, P]),
    "gs_knn_within": (I, [P, L, L, P, L, L, I, P, P, P, Z, P]),
    "gs_yin_frames": (L, [L, I, I, I]),
    "gs_yin_difference": (I, [P, L, L, L, I, I, I, P, P, P]),
    "gs_yin_pick": (I, [P, L, L, I, I, c_double, P, P, P, P]),
    "gs_yin_track": (I, [P, L, L, L, I, I, I, I, c_double, P, P, P, P, P]),
    "gs_kid_workspace_bytes": (Z, [L, L, I, I, L]),
    "gs_kid_sums": (I, [P, L, L, P, L, L, I, P, P, I, L, P, P, Z, P]),
    # W = POINTER(GsLoudness), the meter of one rate
    "gs_loudness_design": (I, [I, W]),
    "gs_loudness_hops": (L, [W, L]),
    "gs_loudness_workspace_bytes": (Z, [W, I, L]),
    "gs_loudness": (I, [W, P, I, L, L, P, L, P, Z, P]),
}

WGRAD_MAX_SOURCES = 4   # GS_WGRAD_MAX_SOURCES
WGRAD_DIRECT, WGRAD_THIN, WGRAD_F32, WGRAD_BF16, WGRAD_THIN_DMA, WGRAD_TILE64 = range(6)   # GS_WGRAD_* families of gs_conv_wgrad_plan
WGRAD_PLAN_INTS = 16   # GS_WGRAD_PLAN_INTS
THIN_EXPAND, THIN_REDUCE, THIN_EXPAND_PNBWD, THIN_SINGLE3, THIN_SINGLE, THIN_DIRECT = range(6)   # GS_THIN_* kernels of gs_conv_thin_route
THIN_PLAIN, THIN_FWD_MASK, THIN_BWD_PNBWD = range(3)   # GS_THIN_* forms
THIN_ROUTE_INTS = 14   # GS_THIN_ROUTE_INTS
DENSE_MAP_FWD, DENSE_MAP_BWD_DATA, DENSE_MAP_BWD_WEIGHT = range(3)   # GS_DENSE_MAP_*
(DENSE_FWD, DENSE_FWD_SMALL, DENSE_FWD_FAST, DENSE_FWD_MFMA, DENSE_FINALIZE, DENSE_BWD_DATA, DENSE_BWD_DATA_WIDE, DENSE_BWD_DATA_FAST, DENSE_BWD_DATA_MFMA,
 DENSE_BWD_WEIGHT, DENSE_BWD_WEIGHT_FAST) = range(11)   # GS_DENSE_* kernels of gs_dense_route
DENSE_ROUTE_INTS = 12   # GS_DENSE_ROUTE_INTS
(EW_OP_BIAS_ACT, EW_OP_ACT_BWD, EW_OP_TANH_BWD_BWD, EW_OP_AXPBY, EW_OP_AXPBY_DEV, EW_OP_UPSCALE, EW_OP_ROW_SCALE, EW_OP_CHANNEL_SUM, EW_OP_ACT_BWD_BIAS,
 EW_OP_PIXEL_NORM_FWD, EW_OP_PIXEL_NORM_BWD, EW_OP_PIXEL_NORM_BWD_BIAS, EW_OP_PIXEL_NORM_BWD_BWD, EW_OP_BLOCKSUM, EW_OP_SUMSQ_ROWS, EW_OP_BATCH_STDDEV_FWD,
 EW_OP_BATCH_STDDEV_BWD, EW_OP_BATCH_STDDEV_BWD_BWD) = range(18)   # GS_EW_OP_* operations of gs_elementwise_route
(EW_BIAS_ACT, EW_BIAS_ACT_SCALAR, EW_ACT_BWD, EW_TANH_BWD_BWD, EW_AXPBY, EW_AXPBY_DEV, EW_UPSCALE, EW_ROW_SCALE, EW_CHANNEL_SUM, EW_CHANNEL_SUM_ROWS,
 EW_ACT_BWD_SUM, EW_PIXEL_NORM, EW_BLOCKSUM, EW_BLOCKSUM_SMALL, EW_SUMSQ_ROWS, EW_BATCH_STDDEV_FWD, EW_BATCH_STDDEV_BWD,
 EW_BATCH_STDDEV_BWD_BWD) = range(18)   # GS_EW_* kernel templates
EW_PATH_NONE, EW_PATH_COLOUR, EW_PATH_QUADS, EW_PATH_GENERIC, EW_PATH_VECTOR, EW_PATH_SCALAR = range(6)   # GS_EW_PATH_*
EW_ROUTE_INTS = 18   # GS_EW_ROUTE_INTS


SUM_PARTIALS = 2   # GS_SUM_PARTIALS
BIAS_FROM_CHANNEL_SUM, BIAS_FROM_ACT_BWD, BIAS_FROM_PIXEL_NORM_BWD = 0, 1, 2


class GsFoldJob(ctypes.Structure):
    """include/gansynth_hip.h: one pending fold of bias-gradient partial rows for gs_channel_fold_batch."""
    _fields_ = [("part", c_void_p), ("out", c_void_p), ("nparts", ctypes.c_int32), ("c", ctypes.c_int32), ("accumulate", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class GsWgradJob(ctypes.Structure):
    """include/gansynth_hip.h: one layer's weight gradient (up to WGRAD_MAX_SOURCES (x, gy) pairs) for gs_conv_wgrad_jobs."""
    _fields_ = [("x", c_void_p * WGRAD_MAX_SOURCES), ("gy", c_void_p * WGRAD_MAX_SOURCES), ("n", ctypes.c_int32 * WGRAD_MAX_SOURCES),
                ("nsrc", ctypes.c_int32), ("bias_mask", ctypes.c_uint32), ("gw", c_void_p), ("gb", c_void_p),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("ci", ctypes.c_int32), ("co", ctypes.c_int32), ("ksize", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("transposed", ctypes.c_int32), ("alpha", c_float), ("accumulate", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("gw_ci_stride", ctypes.c_int32)]


class GsWsDesc(ctypes.Structure):
    """include/gansynth_hip.h: one weight of gs_weight_standardize_batch / _bwd_batch (the table lives in device memory)."""
    _fields_ = [("w", c_void_p), ("out", c_void_p), ("rstd", c_void_p), ("gout", c_void_p), ("gw", c_void_p),
                ("fan_in", ctypes.c_int32), ("co", ctypes.c_int32)]


MIX_TILE = 4096   # GS_MIX_TILE: output samples per block of gs_note_mix


class GsMixNote(ctypes.Structure):
    """include/gansynth_hip.h: one note of gs_note_mix's table (24 bytes; the table lives in device memory, sorted by onset)."""
    _fields_ = [("onset", ctypes.c_int64), ("hold", ctypes.c_int32), ("release", ctypes.c_int32), ("row", ctypes.c_int32), ("gain", c_float)]


class GsMixNoteStereo(ctypes.Structure):
    """include/gansynth_hip.h: one note of gs_note_mix_stereo's table (32 bytes; device memory, sorted by onset; `reserved` is not read)."""
    _fields_ = [("onset", ctypes.c_int64), ("hold", ctypes.c_int32), ("release", ctypes.c_int32), ("row", ctypes.c_int32),
                ("gain_l", c_float), ("gain_r", c_float), ("reserved", ctypes.c_int32)]


class GsMixNoteCurve(ctypes.Structure):
    """include/gansynth_hip.h: one note of gs_note_mix_curves' table (32 bytes; device memory, sorted by onset; `reserved` is not read)."""
    _fields_ = [("onset", ctypes.c_int64), ("hold", ctypes.c_int32), ("release", ctypes.c_int32), ("row", ctypes.c_int32),
                ("gain", c_float), ("curve", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class GsCurvePoint(ctypes.Structure):
    """include/gansynth_hip.h: one point of a gain curve of gs_note_mix_curves (16 bytes; device memory, a curve's points by position)."""
    _fields_ = [("pos", ctypes.c_int64), ("v_l", c_float), ("v_r", c_float)]


WARP_TILE, WARP_ZEROS, WARP_Q = 1024, 32, 256   # GS_WARP_TILE, GS_WARP_ZEROS, GS_WARP_Q


class GsWarpNote(ctypes.Structure):
    """include/gansynth_hip.h: one bent note of gs_note_warp (24 bytes; device memory)."""
    _fields_ = [("src_row", ctypes.c_int32), ("dst_row", ctypes.c_int32), ("onset", ctypes.c_int64), ("count", ctypes.c_int32),
                ("curve", ctypes.c_int32)]


class GsWarpPoint(ctypes.Structure):
    """include/gansynth_hip.h: one point of a ratio curve of gs_note_warp (24 bytes; device memory, a curve's points by position)."""
    _fields_ = [("pos", c_double), ("ratio", c_double), ("cum", c_double)]


SUSTAIN_MAX_WINDOW, SUSTAIN_LAG_TILE, SUSTAIN_TILE = 4096, 256, 1024   # GS_SUSTAIN_MAX_WINDOW, GS_SUSTAIN_LAG_TILE, GS_SUSTAIN_TILE


class GsLoopNote(ctypes.Structure):
    """include/gansynth_hip.h: one note of gs_loop_search (24 bytes; device memory; `reserved` is not read)."""
    _fields_ = [("row", ctypes.c_int32), ("a", ctypes.c_int32), ("m_min", ctypes.c_int32), ("m_max", ctypes.c_int32),
                ("window", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class GsSustainJob(ctypes.Structure):
    """include/gansynth_hip.h: one piece of a looped note of gs_note_sustain (32 bytes; device memory)."""
    _fields_ = [("src_row", ctypes.c_int32), ("dst_row", ctypes.c_int32), ("offset", ctypes.c_int64), ("count", ctypes.c_int32),
                ("a", ctypes.c_int32), ("m", ctypes.c_int32), ("xfade", ctypes.c_int32)]


_lib = None


class GansynthHipError(RuntimeError):
    pass


def load():
    """Load the library once and attach prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GansynthHipError(
            f"{LIB_PATH} not found: build it with gansynth_amd/csrc/build.sh (or __graft_entry__.build()). "
            "gansynth_amd has no CPU/torch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().gs_last_error()
        raise GansynthHipError(f"{what} failed ({code}): {msg.decode() if msg else ''}")
