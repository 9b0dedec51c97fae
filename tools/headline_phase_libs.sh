#!/bin/bash
# Early-exit builds of roi_features.hip for the per-phase instruction budget of the metric kernel (results are wrong by design):
#   gpurun_scratch/libexit_<k>.so ends roi_features_kernel at STAMP(k).  Measure with tools/headline_phase_insts.sh on the GPU box.
# Boundaries of the headline build (roi_features_kernel_occ8<1, 0>, INTENSITY + GLCM at 8 levels) since round 29 -- the order
# differs from the one profiles/r06_headline_phases.txt was taken in (there 3 -> 4 was the engine alone, 6 -> 7 chain | entropy and
# their barrier, 7 -> 8 the central-sum sweep, 9 -> 10 the zeroing pair, 10 -> 11 the co-occurrence sweep):
#   0 LDS cleared | 1 load pass | 2 sums, mean published | 3 central-sum sweep, matrices zeroed, counting engine (two barriers) |
#   4, 5, 6 nothing for a non-blank ROI | 7 wave 0: order-statistics chain, wave 1: n-bin bounds and entropy, waves 2 and 3: nothing
#   (no barrier: a wave that leaves at 7 has not waited for the others) | 8, 9, 10 nothing | 11 the wave's rows of the co-occurrence
#   sweep (glcm_row_bounds: 3, 9, 24 and 25 of the benchmark's 61 rows) and the barrier that ends the interval | 12 counts exported.
# So 6 -> 7 and 10 -> 11 are per-wave figures of waves that do different work: read them per wave role, not as workgroup phases.
# Since round 32 the cloud launches of these builds issue the first trip's loads IN FRONT of phase 0 and rotate the trips (section 4.1 of
# DESIGN.md).  The build that ends at boundary 0 issues no loads (the hoist is compiled out for NYX_EXIT_AT <= 0), so libexit_0 is still
# "prologue, clears, barrier" and leaves with nothing in flight; 0 -> 1 is then the load pass WITH its first round trip, which the full
# kernel has partly behind it when it reaches boundary 0.  Read 0 -> 1 as an upper bound of the load pass, not as its share.
# Launches whose carve-out does not allow the overlap (LdsLayout::overlap = 0), and a library built with -DNYX_NO_OVERLAP, keep a
# barrier at 7 and the zeroing pair in front of 10; every other build of the body keeps the round-6 order.
cd $(dirname $0)/../nyxus_amd/csrc
mkdir -p ../../gpurun_scratch/objexit
build() {
  k=$1
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -w -DNYX_EXIT_AT=$k -c -o ../../gpurun_scratch/objexit/rf_$k.o roi_features.hip &&
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../../gpurun_scratch/libexit_$k.so ../../gpurun_scratch/objexit/rf_$k.o $(ls obj/*.o | grep -v roi_features.o)
}
for grp in "0 1 2 3" "4 5 6 7" "8 10 11 12"; do
  for k in $grp; do build $k & done
  wait
done
ls ../../gpurun_scratch/libexit_*.so
