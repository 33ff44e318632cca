#!/bin/bash
# Builds an experiment variant of the library into tools/alt/<name>.so (in-tree so that it travels with the tree; the
# directory is git-ignored), through csrc/Makefile with the flags appended:   tools/build_variant.sh <name> [-DFLAG ...]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
mkdir -p "$ROOT/tools/alt"
make -C "$ROOT/eaqhm-analysis-and-synthesis-in-python_amd/csrc" -B OUT="$ROOT/tools/alt/$NAME.so" EXTRA="$*"
echo "built tools/alt/$NAME.so"
