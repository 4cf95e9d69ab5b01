#!/bin/bash
# Builds libsimclr_hip.so for gfx950 (cross-compiles without a GPU).
set -e
cd "$(dirname "$0")"
# SIMCLR_SO_OUT / SIMCLR_BUILD_DIR: build somewhere else (compile checks while a GPU call is using the in-tree library)
OUT=${SIMCLR_SO_OUT:-../libsimclr_hip.so}
B=${SIMCLR_BUILD_DIR:-build}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result"
# the translation units, one <name>.hip each: the compile loop and both link lines come from this list
UNITS="runtime ntxent gcl supcon hcl nnclr barlow vicreg repr logreg kmeans spectrum byol moco dino swav swav_multicrop dino_multicrop knn dropblock lars conv bn pool augment comm"
# an object is stale when its source or ANY header of this directory is newer
stale() {
  [ -f $B/$1.o ] || return 0
  for d in $1.hip *.h; do [ $d -nt $B/$1.o ] && return 0; done
  return 1
}
# objects of the link line; objs <unit> <other> puts $B/<other>.o in <unit>'s place
objs() {
  for f in $UNITS; do if [ "$f" = "$1" ]; then echo $B/$2.o; else echo $B/$f.o; fi; done
}
mkdir -p $B
pids=()
for f in $UNITS; do
  if stale $f; then
    hipcc $FLAGS -c $f.hip -o $B/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC $(objs) -o $OUT
echo "built $(realpath $OUT)"
if [ "$1" = "diag" ]; then
  # diagnostic library (tools/diag_conv.py): conv kernels with run-time switches that skip pipeline parts
  hipcc $FLAGS -DSIMCLR_DIAG -c conv.hip -o $B/conv_diag.o
  hipcc --offload-arch=gfx950 -shared -fPIC $(objs conv conv_diag) -o ../libsimclr_hip_diag.so
  echo "built $(realpath ../libsimclr_hip_diag.so)"
fi
