#!/bin/bash
# Build a variant of libm3d.so with extra compile flags into tools/ab/<name>.so (A/B timing of two
# builds in one GPU call; tools that take AB_LIB load it).  The file list and the per-file flag
# groups are the Makefile's own (BUILD / OUT / EXTRA / ICP_FLAGS), so no source file can be missed.
# Usage: [ABX=flags] tools/ab_build.sh NAME [-DFLAG=V ...]   (ABX replaces the ransac/icp/nn_brute flags)
set -eu
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
build=${TMPDIR:-/tmp}/ab_$name; rm -rf "$build"; mkdir -p "$root/tools/ab"  # flags may differ: no stale objects
make -C "$root/3d-matching_amd/csrc" -j"${MAX_JOBS:-8}" BUILD="$build" OUT="$root/tools/ab/$name.so" \
  EXTRA="-w $*" ${ABX+ICP_FLAGS="$ABX"} >&2
echo "tools/ab/$name.so"
