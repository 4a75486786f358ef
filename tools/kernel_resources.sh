#!/bin/bash
# Compact per-kernel resource table (VGPRs, AGPRs, scratch, occupancy, LDS) for a source of the product library, compiled with
# the flags its object carries in redsec_amd/build.py (HIP_OBJECTS).
# usage: tools/kernel_resources.sh redsec_amd/csrc/rs_bootstrap.hip [filter]      (likewise rs_bootstrap_split.hip, rs_bootstrap_listed.hip ...)
cd "$(dirname "$0")/.."
OBJ="$(basename "${1%.*}")"
FLAGS="$(python -m redsec_amd.build --print-flags "$OBJ" 2>/dev/null)" || { echo "no object $OBJ in HIP_OBJECTS (redsec_amd/build.py)"; exit 2; }
hipcc $FLAGS --cuda-device-only -c "$1" -o /tmp/kr.o \
  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|Name:|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size" \
  | sed -E 's/^[^ ]+ remark: [^ ]+ +//; s/ \[-Rpass.*//' | paste - - - - - - | grep -E "${2:-.}" | c++filt | sed -E 's/rs::BlindRotateArgs//; s/rs:://g'
