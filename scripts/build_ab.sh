#!/bin/bash
# builds ab/lib_<tag>.so variants of the library that differ in the compile flags of ONE kernel file (A/B measurements inside one GPU job).
# usage: scripts/build_ab.sh [-f conv_wgrad | conv_thin | dense] "tag|flags" ...      (-f: the file to rebuild, default conv_igemm; ab/ is git-ignored; delete
#        it when done: it travels with the tree)
F=conv_igemm
if [ "$1" = "-f" ]; then F=$2; shift 2; fi
cd "$(dirname "$0")/../gansynth_amd/csrc"
[ -f $F.hip ] || { echo "no $F.hip"; exit 1; }
mkdir -p ../../ab
./build.sh > /dev/null
pids=()
for v in "$@"; do
  IFS='|' read -r tag flags <<< "$v"
  ( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form $flags -c $F.hip -o ../../ab/${F}_$tag.o 2>/dev/null \
    && hipcc --offload-arch=gfx950 -shared -fPIC ../../ab/${F}_$tag.o $(ls obj/*.o | grep -v "obj/$F.o") -ldl -o ../../ab/lib_$tag.so && rm ../../ab/${F}_$tag.o && echo built $tag ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
ls -la ../../ab
