#!/usr/bin/env bash
# Device assembly of one kernel translation unit: tools/kernel_isa.sh fast|exact|plain OUT.s [-DMGCFD_EXP_...]
#   fast, exact: csrc/kernels.hip for that namespace;  plain: csrc/kernels_plain.hip, sa: csrc/kernels_sa.hip, wall_heat: csrc/kernels_wall_heat.hip, face_gradient: csrc/kernels_face_gradient.hip, statistics: csrc/kernels_statistics.hip (compiled once, never contracted).
# MGCFD_EXP_SRC=FILE compiles FILE instead, with the flags of the translation unit named.
set -e
ns=$1; out=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd); CS=$ROOT/mg-cfd-app-plain_amd/csrc
src=$CS/kernels.hip
case "$ns" in
  fast)  nsf="-ffp-contract=fast -DMGCFD_KERNEL_NS=fast -DMGCFD_ORDER_FREE=1" ;;
  exact) nsf="-ffp-contract=off -DMGCFD_KERNEL_NS=exact" ;;
  plain) nsf="-ffp-contract=off"; src=$CS/kernels_plain.hip ;;
  sa) nsf="-ffp-contract=off"; src=$CS/kernels_sa.hip ;;
  wall_heat) nsf="-ffp-contract=off"; src=$CS/kernels_wall_heat.hip ;;
  face_gradient) nsf="-ffp-contract=off"; src=$CS/kernels_face_gradient.hip ;;
  statistics) nsf="-ffp-contract=off"; src=$CS/kernels_statistics.hip ;;
  *) echo "usage: $0 fast|exact|plain OUT.s [flags]" >&2; exit 2 ;;
esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 --offload-device-only -O3 -std=c++17 -fno-fast-math -Wno-unused-result -mllvm -amdgpu-kernarg-preload-count=16 \
  $nsf "$@" -I$ROOT/include -I$CS -S ${MGCFD_EXP_SRC:-$src} -o $out
