#!/bin/bash
# Development: build a variant of libalproj_hip.so with extra -D flags for alp_raster.hip (always with -DALP_DEV:
# the library then reports its switches through alp_build_flags() and tests / bench.py refuse it).
#   tools/build_variant.sh NAME -DFOO=1 ...   ->  build/abl/libalproj_NAME.so   (use with ALPROJ_HIP_LIB)
# The other units' objects are the regular build's (python -m alproj_amd._build first); which they are comes from
# alproj_amd/_build.py: SOURCES.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build/abl
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -Iinclude -Ialproj_amd/csrc \
    -ffp-contract=off -DALP_DEV "$@" -c alproj_amd/csrc/alp_raster.hip -o build/abl/raster_$name.o
objs=$(python3 -c "
import os, sys
sys.path.insert(0, '.')
from alproj_amd import _build as b
print(' '.join('build/abl/raster_$name.o' if s == 'alp_raster.hip' else os.path.join('build', os.path.splitext(os.path.basename(s))[0] + '.o') for s in b.SOURCES))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/abl/libalproj_$name.so $objs -L/opt/rocm/lib -lrccl -lpthread -Wl,-rpath,/opt/rocm/lib
echo build/abl/libalproj_$name.so
