#!/bin/bash
# tools/build_variant.sh NAME [-DFOO=1 ...]: an experimental build of libgss_hip.so with extra
# compiler flags, written to pb_chime5_amd/lib/variants/libgss_NAME.so (select it with
# GSS_HIP_LIBRARY=<path>).  For A/B timing of kernel variants on the GPU box.  The translation
# units and the flags are the package build's own (pb_chime5_amd/build.py: SOURCES, FLAGS).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
OUT=$R/pb_chime5_amd/lib/variants; mkdir -p $OUT/$NAME
cd $R
SOURCES=$(python3 -c "from pb_chime5_amd.build import SOURCES; print(' '.join(SOURCES))")
FLAGS="-DGSS_EXPERIMENT_BUILD=1 $(python3 -c "from pb_chime5_amd.build import FLAGS; print(' '.join(FLAGS))")"
pids=()
for f in $SOURCES; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c $R/pb_chime5_amd/csrc/$f -o $OUT/$NAME/${f%.hip}.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OUT/$NAME/*.o -o $OUT/libgss_$NAME.so
rm -rf $OUT/$NAME
echo $OUT/libgss_$NAME.so
