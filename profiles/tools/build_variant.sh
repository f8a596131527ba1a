#!/bin/bash
# Builds a variant of libtvae_hip.so with ONE unit recompiled under extra flags (ablation / experiment macros), next to the
# shipped library:  bash profiles/tools/build_variant.sh dense_wgrad_x6_p2 "-DTVAE_WW_ABL=1" ab_var/ww1.so
# UNIT is an object of csrc/Makefile: abi_<family>, an instance of dense_x6_instances.def (dense_x6_v<XV>e<EPI>p<NP>, e.g.
# dense_x6_v0e0p2 "-DTVAE_ABL=8") or dense_wgrad_x6_p<NP>.
# Compare on one box:  gpurun -- 'bash profiles/tools/ab_kernels.sh TVAE_LIB "$PWD/ab_var/ww1.so ..." wgrad'
set -eu
UNIT=$1; XF=$2; OUT=$3
cd "$(dirname "$0")/../../target-vae_amd/csrc"
test -f "build/$UNIT.o" || { echo "no object build/$UNIT.o: run make first, and name one of its units" >&2; exit 1; }
mkdir -p "$(dirname "../../$OUT")"
TAG=$(echo "$UNIT$XF" | md5sum | cut -c1-8)
make -s var UNIT="$UNIT" XF="$XF" VAROBJ="build/var/$UNIT.$TAG.o"
OBJS=$(ls build/*.o | grep -v "build/$UNIT.o" | grep -v -e build/abi_cluster.o -e build/abi_ward.o -e build/abi_tsne.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fno-gpu-rdc -shared -fPIC $OBJS build/var/$UNIT.$TAG.o -ldl -o "../../$OUT"
echo "built $OUT"
