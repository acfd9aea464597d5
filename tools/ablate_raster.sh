#!/bin/bash
# Compile-time variants of rasterize.hip as copies of libia_hip.so under tools/_variants/, timed with tools/bench_raster.py.
# IA_RAST_ABLATE: 1 no static-crop loads, 2 no texture walk, 4 no stores of the blended channels (3, 7: what is left is the chain).
#   tools/ablate_raster.sh build <tag> [flags]   (CPU container; needs the library's objects: python -m invertavatar_amd.build first.
#                                                 Also writes the compiler's resource report to tools/_variants/raster_<tag>_resources.txt)
#   tools/ablate_raster.sh run <tag>             (GPU box)
set -e
cd "$(dirname "$0")/.."
CS=invertavatar_amd/csrc
mkdir -p tools/_variants
mode=$1; tag=${2:-tree}; shift; shift || true
if [ "$mode" = build ]; then
  objs=$(ls $CS/build/*.o | grep -v "/rasterize\.")
  for n in 0 1 2 3 4 7; do
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DIA_RAST_ABLATE=$n "$@" -c $CS/rasterize.hip -o tools/_variants/raster_${tag}_a$n.o
    hipcc -shared -fPIC --offload-arch=gfx950 $objs tools/_variants/raster_${tag}_a$n.o -o tools/_variants/libia_raster_${tag}_a$n.so
    rm tools/_variants/raster_${tag}_a$n.o
  done
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off "$@" -Rpass-analysis=kernel-resource-usage -c $CS/rasterize.hip -o /dev/null 2>&1 \
    | grep -A11 "Function Name: .*rasterize_" | grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size" > tools/_variants/raster_${tag}_resources.txt
  cat tools/_variants/raster_${tag}_resources.txt
else
  for n in 0 1 2 3 4 7; do
    echo "== $tag IA_RAST_ABLATE=$n"
    IA_HIP_LIB=$PWD/tools/_variants/libia_raster_${tag}_a$n.so timeout -k 10 120 python tools/bench_raster.py
  done
fi
