// The finishing stage of synth.hip for another translation unit (fftconv.hip): a clip of 1 or 2 rows that its producer left together with
// one |max| per block.
#pragma once
#include "gs_common.h"

namespace gs {

// Launches note_mix_finish_kernel (rows == 1) or stereo_finish_kernel (rows == 2) on x: [rows] rows of n samples, row_stride apart, IN PLACE.
// block_max: n_max maxima over all rows (folded into ONE peak).  pcm / peak may be null; the caller skips the call when nothing is asked for.
void launch_clip_finish(float* x, int rows, long n, long row_stride, short* pcm, float* peak, const float* block_max, int n_max, int normalize,
                        hipStream_t st);

}  // namespace gs
