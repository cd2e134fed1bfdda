#!/bin/bash
# build a variant of the library into ab/<name>.so: tools/build_variant.sh name "-DFLAG ..." [file-that-gets-the-flags|all]
set -e
name=$1; flags=$2; only=${3:-all}
rm -rf /tmp/stb_$name && mkdir -p /tmp/stb_$name ab && cp hoigen_amd/csrc/*.hip hoigen_amd/csrc/*.h hoigen_amd/csrc/*.inc /tmp/stb_$name/
repo=$(pwd)
cd /tmp/stb_$name && sed -i "s#\"../../include/hoigen_amd.h\"#\"$repo/include/hoigen_amd.h\"#" hg_host.h
for f in $(ls *.hip | sed 's/\.hip$//'); do      # every source of the library, as build.sh
  fl=""; if [ "$only" = all ] || [ "$only" = $f ]; then fl="$flags"; fi
  if [ $f = hg_preproc ]; then fl="$fl -ffp-contract=off"; fi      # as build.sh: bit-exact arithmetic, never fused
  ( /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -Wno-unused-function -ffp-contract=fast $fl -c $f.hip -o $f.o 2>&1 | grep -E "error" || true ) &
done; wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC *.o -o $repo/ab/$name.so && echo "built ab/$name.so"
