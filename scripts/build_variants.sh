#!/bin/bash
# Variant libraries for same-box A/B (scripts/ab_kernels.py): each NAME=DEFS
# pair builds dstd-gcn_amd/libdstd_gcn_NAME.so from the current sources.
#   scripts/build_variants.sh stamps=-DDSTD_STAMPS
# (DSTD_STAMPS is the only build switch; an experiment edits a constant in
# csrc/ and builds it under a name: scripts/build_variants.sh try1=)
cd "$(dirname "$0")/../dstd-gcn_amd" || exit 2
for spec in "$@"; do
  name=${spec%%=*}; defs=${spec#*=}
  make -j8 VARIANT="$name" DEFS="$defs" > /dev/null 2>"/tmp/build_$name.err" || { cat "/tmp/build_$name.err"; exit 1; }
  echo "built libdstd_gcn_$name.so ($defs)"
done
