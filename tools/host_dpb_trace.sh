#!/bin/bash
# Builds the host side of libh264mi with its test hooks (-DH264MI_TEST_HOOKS) against the null device (tools/hoststub) and
# tools/host_dpb_trace.cpp into ${TMPDIR:-/tmp}/h264mi_host_dpb_trace/ and prints the path of the program.  No GPU, no HIP toolchain needed (g++).
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
out=${TMPDIR:-/tmp}/h264mi_host_dpb_trace
mkdir -p "$out"
srcs=$(make -s -C "$root/h264decode_amd/csrc" host-srcs) # the host sources: one list, csrc/Makefile
g++ -std=c++17 -O1 -g -fPIC -shared -DH264MI_TEST_HOOKS -I"$root/tools/hoststub" -I"$root/include" $srcs -o "$out/libh264mi_host_hooks.so" -lpthread
g++ -std=c++17 -O1 -g -I"$root/include" "$root/tools/host_dpb_trace.cpp" -L"$out" -lh264mi_host_hooks -Wl,-rpath,"$out" -o "$out/host_dpb_trace"
echo "$out/host_dpb_trace"
