#!/bin/bash
# tools/build_variant_one.sh <name> <source stem> [-DFLAG=..]...  -> cvpr23-e3dge_amd/lib/variants/lib_<name>.so
# Like build_variant.sh, but recompiles ONE source with the flags and links it against the default build's objects of the others
set -e
NAME=$1; STEM=$2; shift; shift
exec python "$(dirname "$0")/../cvpr23-e3dge_amd/build.py" --variant "$NAME" --only "$STEM" "$@"
