#!/bin/bash
# Build an experimental librnstok variant: tools/build_variant.sh <name> <extra hipcc flags...>
# Output: $EXP_DIR/<name>/librnstok.so, EXP_DIR default build_exp (gpurun-ignored: use
# EXP_DIR=exp_ship for a variant that must travel to the GPU box)  (load with tools/exp_bench.py)
# The sources are the product's: csrc/Makefile builds them, with objects keyed on the flags.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${EXP_DIR:-build_exp}
mkdir -p $ROOT/$OUT/$NAME
make -s -j6 -C $ROOT/reticulum_amd/csrc OUT=$ROOT/$OUT/$NAME/librnstok.so \
  FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -w $*"
echo built $OUT/$NAME
