#!/bin/bash
# Build libredsec_hip.so from a source tree into variants/lib_<name>.so (git-ignored, travels to the GPU
# box) for same-box A/B timing with REDSEC_HIP_LIB. usage: tools/build_variant.sh NAME [SRC_ROOT] [extra hipcc flags...]
# A wrapper over `python -m redsec_amd.build --variant`: the objects and their flags are the HIP_OBJECTS of SRC_ROOT's own
# redsec_amd/build.py, the extra flags go to every object (flags for one object: that command's --object-flags).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
NAME="$1"; SRC="${2:-$ROOT}"; shift; shift || true
cd "$ROOT"
python -m redsec_amd.build --variant "$NAME" --src "$SRC" -- "$@"
ls -la "$ROOT/variants/lib_$NAME.so"
