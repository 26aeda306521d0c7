#!/bin/bash
# tools/build_variant.sh NAME "-DFLAG ..." -> ringpop_amd/variants/libringpop_hip_NAME.so (experiments only)
# SRC=<dir>: take the .hip sources from <dir> (e.g. a git-exported older tree) instead of ringpop_amd/csrc
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
mkdir -p ringpop_amd/variants/$NAME
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function $*"
SRC=${SRC:-ringpop_amd/csrc}
pids=()
# the product's source list (ringpop_amd/build.py), read without importing the package (no GPU needed)
SOURCES=$(python3 -c "import runpy; print(' '.join(s[:-4] for s in runpy.run_path('ringpop_amd/build.py')['SOURCES']))")
rm -f ringpop_amd/variants/$NAME/*.o
for s in $SOURCES; do /opt/rocm/bin/hipcc $F -I$SRC -c $SRC/$s.hip -o ringpop_amd/variants/$NAME/$s.o & pids+=($!); done
for p in "${pids[@]}"; do wait $p || { echo "variant $NAME: compile failed" >&2; exit 1; }; done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ringpop_amd/variants/libringpop_hip_$NAME.so ringpop_amd/variants/$NAME/*.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
