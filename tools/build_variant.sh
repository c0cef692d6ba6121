# build a variant of libilcc_hip.so with extra compile-time knobs into build/ab/ (selected through ILCC_HIP_LIB):
#   tools/build_variant.sh NAME -DILCC_K6_TIMING [...]
# The sources are copied to build/variant_NAME/ (as deep in the tree as csrc/, so the Makefile's relative paths hold) and built there
# by csrc/Makefile itself: the same objects and flags as the shipped library, plus the knobs.
set -e
NAME=$1; shift
R=$(cd $(dirname $0)/.. && pwd)
D=$R/build/variant_$NAME
mkdir -p $D $R/build/ab
cp $R/lidar_camera_calibration_amd/csrc/Makefile $R/lidar_camera_calibration_amd/csrc/*.hip $R/lidar_camera_calibration_amd/csrc/*.cpp \
   $R/lidar_camera_calibration_amd/csrc/*.h $D/
make -C $D -j8 -s EXTRA="$*" OUT=$R/build/ab/libilcc_hip_$NAME.so
echo built $R/build/ab/libilcc_hip_$NAME.so
