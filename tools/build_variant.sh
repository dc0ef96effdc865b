#!/bin/bash
# tools/build_variant.sh <name> [-DFLAG=..]...  -> cvpr23-e3dge_amd/lib/variants/lib_<name>.so  (instrumented and A/B builds)
set -e
NAME=$1; shift
exec python "$(dirname "$0")/../cvpr23-e3dge_amd/build.py" --variant "$NAME" "$@"
