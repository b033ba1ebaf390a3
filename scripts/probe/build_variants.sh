#!/bin/bash
# builds igemm_trace_<tag> probes with forced tile configurations / ablations (see conv_igemm.hip GS_FORCE_CFG, GS_ABL_*)
# usage: build_variants.sh  "tag|mode|cfg|extra flags" ...
#   cfg: the nine fields of one IgemmCfg, A,B,TW,TG,RESIDENT,D,NORM,RB,SPEC -- e.g. "m0_d2|0|2,2,32,3,false,2,0,64,false" (empty: the chooser's own pick)
#        build_variants.sh role_check     conv_role_check (host-only: the conv geometry under ASan + UBSan; run it on a CPU, never on a GPU box)
#        build_variants.sh route_check    thin_route_check, dense_route_check (host-only: thin_route / dense_route over their covers' grids under ASan + UBSan;
#                                         run them on a CPU)
cd "$(dirname "$0")"
C=../../gansynth_amd/csrc
[ "$1" = role_check ] && exec hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I../../include -I$C -o conv_role_check conv_role_check.hip $C/conv_igemm.hip $C/conv_wgrad.hip $C/conv_thin.hip $C/elementwise.hip -x hip $C/core.cpp
if [ "$1" = route_check ]; then
  for p in thin_route_check dense_route_check; do
    hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I../../include -I$C -o $p $p.hip || exit 1
  done
  exit 0
fi
pids=()
for v in "$@"; do
  IFS='|' read -r tag mode cfg extra <<< "$v"
  F=""
  [ -n "$cfg" ] && F="-DGS_FORCE_MODE=$mode -DGS_FORCE_CFG=$cfg"
  ( hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form -I../../include -I../../gansynth_amd/csrc $F $extra -o igemm_trace_$tag igemm_trace.hip 2>&1 | grep -E "error" ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
ls igemm_trace_*
