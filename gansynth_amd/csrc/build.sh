#!/bin/bash
# Builds libgansynth_hip.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [--clean] [outdir]
#   --clean   drop every object first (obj/ is git-ignored but travels with the tree: without the flag the build is incremental by mtime)
set -e
cd "$(dirname "$0")"
if [ "$1" = "--clean" ]; then
  rm -rf obj
  shift
fi
OUT=${1:-..}
mkdir -p obj
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $GS_EXTRA_FLAGS"
pids=()
for f in conv_igemm conv_wgrad conv_thin conv_api elementwise small_ops dense spectral spectral_wave classifier classifier_bwd summary synth mix_curves warp sustain clip_finish bank resample fftconv limiter loudness true_peak kmeans swd knn yin kid; do
  [ -f $f.hip ] || continue
  stale=0   # (-nt also holds when the object is missing)
  for s in $f.hip *.h ../../include/gansynth_hip.h; do [ $s -nt obj/$f.o ] && stale=1; done
  if [ $stale = 1 ]; then
    EXTRA=""
    # MFMA accumulators in VGPRs (hipcc otherwise parks them in AGPRs and every epilogue value costs a v_accvgpr_read)
    { [ $f = conv_igemm ] || [ $f = conv_wgrad ]; } && EXTRA="-mllvm -amdgpu-mfma-vgpr-form $GS_IGEMM_FLAGS"
    # (complex arithmetic as float2: SLP-packing it into v_pk_* costs more register shuffling than it saves -- measured -8 %)
    [ $f = spectral_wave ] && EXTRA="-fno-slp-vectorize $GS_SW_FLAGS"
    # (the tap loop's four chains stay scalar: packed into v_pk_* they cost 14 register moves per four taps -- measured, DESIGN.md "Pitch bend")
    [ $f = warp ] && EXTRA="-fno-slp-vectorize"
    # (assign's 4 x KG chains stay scalar: packed by row pairs, every centre value is first copied into a register pair and the kernel needs
    #  220 registers instead of 136 -- two waves a SIMD instead of three; DESIGN.md "NDB on the device")
    [ $f = kmeans ] && EXTRA="-fno-slp-vectorize"
    # (knn packs its chains by row pairs by hand, as float2: nothing is left to the SLP vectoriser; DESIGN.md "Precision and recall on the device")
    [ $f = knn ] && EXTRA="-fno-slp-vectorize"
    # (yin's eight chains a thread stay scalar: a packed pair would hold two lags whose windows lie a sample apart; DESIGN.md "Pitch tracking on the device")
    [ $f = yin ] && EXTRA="-fno-slp-vectorize"
    ( hipcc $FLAGS $EXTRA -c $f.hip -o obj/$f.o ) &
    pids+=($!)
  fi
done
if [ ! -f obj/core.o ] || [ core.cpp -nt obj/core.o ] || [ gs_common.h -nt obj/core.o ] || [ gs_prof.h -nt obj/core.o ]; then
  ( hipcc $FLAGS -x hip -c core.cpp -o obj/core.o ) &
  pids+=($!)
fi
if [ ! -f obj/comm.o ] || [ comm.cpp -nt obj/comm.o ] || [ gs_common.h -nt obj/comm.o ] || [ ../../include/gansynth_hip.h -nt obj/comm.o ]; then
  ( hipcc $FLAGS -x hip -c comm.cpp -o obj/comm.o ) &
  pids+=($!)
fi
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC obj/*.o -ldl -o $OUT/libgansynth_hip.so
echo "built $OUT/libgansynth_hip.so"
