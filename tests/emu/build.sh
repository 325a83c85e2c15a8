#!/bin/sh
# TEST INFRASTRUCTURE: build the CPU execution harness of the HIP translation unit.
set -e
cd "$(dirname "$0")"
# sh build.sh [output [extra compiler flags]]: a variant of the library (a lowered compile-time threshold) beside the default one
OUT=${1:-libcc_emu.so}
[ $# -gt 0 ] && shift
g++ -O2 -std=c++17 -fPIC -ffp-contract=off -pthread -I. -Wno-unused-value "$@" -shared -o "$OUT" emu_main.cpp -ldl
