// h264decode_amd/csrc/k_deint_rule.h -- what the two K10 kernels share (k_deint.hip: the spatial modes; k_deint_motion.hip: the motion-adaptive ones): a
// thread item's 16-byte load, FIELD's average and EDGE's direction search, by the rule of include/h264mi.h, "Deinterlaced output".
// Device code only; everything is static and inlined, so each kernel keeps its own register allocation.
#pragma once
#include "mi_kernels.h"
#include "k_output_rule.h" // pack4, byte_of, store16

// 16 bytes from p: one load on the aligned path; bytes 0 .. n - 1 (the rest repeat the last one) otherwise
template <bool VEC> __device__ static __forceinline__ void load16(const uint8_t *p, int n, uint32_t o[4]) {
    if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = pack4(p[min(4 * q, n - 1)], p[min(4 * q + 1, n - 1)], p[min(4 * q + 2, n - 1)], p[min(4 * q + 3, n - 1)]);
    }
}

// FIELD: (a + b + 1) >> 1 of the four bytes of a word: a | b is the sum's carry-free half rounded up, minus half of the bits that differ (no byte borrows:
// (a ^ b) >> 1 <= a | b in every byte, and the mask keeps a byte's low bit out of the byte below)
__device__ static __forceinline__ uint32_t avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) & 0xfefefefeu) >> 1); }

// EDGE, a thread's 16 columns of a missing luma row: u / d are the rows above / below, ul, ur, dl, dr the samples left and right of the 16 columns (clamped
// to the plane by the caller).  Directions 0, -1, +1 in that order, the first one of the strictly smallest cost
__device__ static __forceinline__ void edge16(const uint32_t u[4], const uint32_t d[4], uint32_t ul, uint32_t ur, uint32_t dl, uint32_t dr, uint32_t o[4]) {
    int ub[18], db[18];
    ub[0] = static_cast<int>(ul), ub[17] = static_cast<int>(ur), db[0] = static_cast<int>(dl), db[17] = static_cast<int>(dr);
#pragma unroll
    for (int i = 0; i < 16; i++) ub[i + 1] = static_cast<int>(byte_of(u[i >> 2], i & 3)), db[i + 1] = static_cast<int>(byte_of(d[i >> 2], i & 3));
    uint32_t r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        int best = abs(ub[i + 1] - db[i + 1]), sum = ub[i + 1] + db[i + 1];
        const int cm = abs(ub[i] - db[i + 2]), cp = abs(ub[i + 2] - db[i]); // d = -1: up[x - 1], dn[x + 1]; d = +1: up[x + 1], dn[x - 1]
        if (cm < best) best = cm, sum = ub[i] + db[i + 2];
        if (cp < best) best = cp, sum = ub[i + 2] + db[i];
        r[i] = static_cast<uint32_t>((sum + 1) >> 1);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = pack4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
}
