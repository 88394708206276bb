#!/bin/bash
# Builds the host side of libh264mi against the null device (tools/hoststub) and tools/host_random_access.cpp into
# ${TMPDIR:-/tmp}/h264mi_host_random_access/ and prints the path of the program.  No GPU, no HIP toolchain needed (g++).
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
out=${TMPDIR:-/tmp}/h264mi_host_random_access
mkdir -p "$out"
srcs=$(make -s -C "$root/h264decode_amd/csrc" host-srcs) # the host sources: one list, csrc/Makefile
g++ -std=c++17 -O1 -g -fPIC -shared -I"$root/tools/hoststub" -I"$root/include" $srcs -o "$out/libh264mi_host.so" -lpthread
g++ -std=c++17 -O1 -g -I"$root/include" "$root/tools/host_random_access.cpp" -L"$out" -lh264mi_host -Wl,-rpath,"$out" -o "$out/host_random_access"
echo "$out/host_random_access"
