#!/bin/bash
# Diagnostic library variant: one HIP source (default lzf_lane.hip, or
# SRC=lzf_decompress.hip ...) rebuilt with extra defines, linked with the
# other objects of the normal build (make first).  SRC may name several files
# (SRC="lzf_lane.hip lzf_lane_diag.hip" for the wave-form parse's -DLZF_DIAG
# -DKW_PHASES): each is rebuilt with the defines.
# usage: [SRC="file.hip ..."] tools/build_variant.sh NAME -DFLAG [...]   -> gibson_amd/liblzf_hip_NAME.so
set -e
name=$1; shift
srcs=${SRC:-lzf_lane.hip}
cd "$(dirname "$0")/../gibson_amd/csrc"
H="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -munsafe-fp-atomics -I. -I../../include"
objs=""
excl="-e var_ -e stats_ -e diag_ -e lzf_serial.o"
for src in $srcs; do
    $H "$@" -c "$src" -o "build/var_${name}_${src%.hip}.o"
    objs="$objs build/var_${name}_${src%.hip}.o"
    excl="$excl -e build/${src%.hip}.o"
done
[ -n "$EXCL" ] && excl="$excl -e build/$EXCL"
$H -shared -o ../liblzf_hip_$name.so $objs $(ls build/*.o | grep -v $excl)
echo built gibson_amd/liblzf_hip_$name.so
