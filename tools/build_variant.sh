# DIAGNOSTIC: build an experimental libptmi.so from the working tree with extra
# defines.  usage: bash tools/build_variant.sh <name> [-DNAME=VAL ...]
#   -> pathtracer-ocl_amd/build/exp/libptmi_<name>.so   (tools/exp_variants.sh times it)
# <name> = head: the HEAD commit's sources instead of the working tree.
# FROMREV=<commit>: that commit's sources (an A/B build of an alternative the tree no longer holds:
# DESIGN.md "settled switches" names the last commit that has each).
set -e
NAME=$1; shift
cd "$(dirname "$0")/../pathtracer-ocl_amd"
mkdir -p build/exp
SRC=csrc
REV=${REV:-${FROMREV:-HEAD}}
if [ "$NAME" = head ] || [ -n "$FROMREV" ]; then
  SRC=$(mktemp -d)/csrc; mkdir -p $SRC
  for f in ptmi_kernels.hip ptmi_api.cpp ptmi_bvh.cpp ptmi_bvh.h ptmi_device.h ptmi_sinf.h ptmi_fp64core.h ptmi_f16.h; do
    git show $REV:pathtracer-ocl_amd/csrc/$f > $SRC/$f
  done
  # (the study kernels' file: revisions before the split keep that code in ptmi_kernels.hip)
  git show $REV:pathtracer-ocl_amd/csrc/ptmi_study_kernels.h > $SRC/ptmi_study_kernels.h 2>/dev/null || rm -f $SRC/ptmi_study_kernels.h
  # (the tile classifier, the motion records, the flags / launch / plan headers, the image passes' file: older
  # revisions have none, and keep the image passes in ptmi_kernels.hip)
  for f in ptmi_camcull.h ptmi_motion.h ptmi_flags.h ptmi_launch.h ptmi_plan.h ptmi_image_kernels.hip \
           ptmi_image_api.cpp ptmi_image_args.h ptmi_api_internal.h; do
    git show $REV:pathtracer-ocl_amd/csrc/$f > $SRC/$f 2>/dev/null || rm -f $SRC/$f
  done
  mkdir -p $(dirname $SRC)/../include
  for f in ptmi.h ptmi_diag.h ptmi_host.h; do
    git show $REV:include/$f > $(dirname $SRC)/../include/$f 2>/dev/null || true
  done
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-result \
  "$@" -shared -o build/exp/libptmi_$NAME.so $SRC/ptmi_kernels.hip $(ls $SRC/ptmi_image_kernels.hip 2>/dev/null) \
  $SRC/ptmi_api.cpp $(ls $SRC/ptmi_image_api.cpp 2>/dev/null) $SRC/ptmi_bvh.cpp
