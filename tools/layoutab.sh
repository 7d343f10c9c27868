#!/bin/bash
# tools/layoutab.sh [CFG ...] -- dev-only, ON THE GPU BOX: A/B of the Euclidean G1 kernels' global-memory layout
# (pair: row-aligned | block: workgroup-dense | wave: wave-dense), via tools/bin/membench
# (tools/membench.hip linked against the library).  CFG = fwdlayout,bwdlayout[,fusedlayout]
[ $# -eq 0 ] && set -- pair,pair pair,block block,block
for cfg in "$@"; do
  IFS=, read -r lf lb lfu <<< "$cfg"
  lfu=${lfu:-pair}
  echo "=== forward $lf, backward $lb, fused $lfu"
  MMS_EUCLID_LAYOUT_FWD=$lf MMS_EUCLID_LAYOUT_BWD=$lb MMS_EUCLID_LAYOUT_FUSED=$lfu timeout -k 10 120 tools/bin/membench | grep -E "mms fwd|mms bwd|SEQ mms" || exit 1
done
