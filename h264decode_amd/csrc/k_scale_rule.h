// h264decode_amd/csrc/k_scale_rule.h -- the sampling rule of include/h264mi.h, "Scaled output" (bilinear and area taps, one scaled sample of a display
// plane) and the pieces of K7's conversion that K8 (k_scale.hip) and K9 (k_tensor.hip) share: the coefficient table, the byte packing, the clip.
// Device code only; everything is static and inlined, so each kernel keeps its own register allocation.
#pragma once
#include "mi_kernels.h"

// {cy, crv, cgu, cgv, cbu} in 1/8192: the rows of H264MI_CSC_COEFFS (include/h264mi.h), as in k_convert.hip
__device__ static const int32_t k_scale_csc[4][5] = {
    {9539, 13075, 3209, 6660, 16525},
    {8192, 11485, 2819, 5850, 14516},
    {9539, 14686, 1747, 4366, 17305},
    {8192, 12901, 1535, 3835, 15201},
};

__device__ static __forceinline__ uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 255u; }
// four values of 0 .. 255 -> one word, by byte permutes (v_perm_b32), never by shifts and ORs: see k_convert.hip, pack4
__device__ static __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return __builtin_amdgcn_perm(b, a, 0x0c0c0400u) | __builtin_amdgcn_perm(d, c, 0x04000c0cu);
}
__device__ static __forceinline__ uint32_t clip255(int v) { return static_cast<uint32_t>(min(max(v, 0), 255)); }

// one axis of one plane
struct Axis {
    int n_in, n_out;
    int step, half; // bilinear only
};
// the taps of output index i (0 <= i < n_out) on an axis.  Bilinear: source samples a and b, fraction f.  Area: a = the first overlapping source
// sample, floor(i n_in / n_out); lo = i n_in (the output sample covers [lo, lo + n_in) in units of 1 / n_out of a source sample)
struct Tap {
    int a, b, f;
    uint32_t lo;
};
template <int FILTER> __device__ static __forceinline__ Tap tap_of(const Axis &A, int i) {
    Tap t;
    if (FILTER == 0) {
        const int P = min(max(i * A.step + A.half, 0), (A.n_in - 1) << 16); // i step < n_in << 16 <= 2^30
        t.a = P >> 16, t.f = (P >> 8) & 255, t.b = min(t.a + 1, A.n_in - 1), t.lo = 0;
    } else {
        t.lo = static_cast<uint32_t>(i) * static_cast<uint32_t>(A.n_in); // < 2^28
        t.a = static_cast<int>(t.lo / static_cast<uint32_t>(A.n_out)), t.b = 0, t.f = 0;
    }
    return t;
}
// area: overlap of the output sample [lo, lo + n_in) with source sample k = [k n_out, (k + 1) n_out); positive for k = a .. while k n_out < lo + n_in
__device__ static __forceinline__ uint32_t overlap(const Axis &A, uint32_t lo, uint32_t k) {
    const uint32_t n_out = static_cast<uint32_t>(A.n_out);
    return min(lo + static_cast<uint32_t>(A.n_in), (k + 1) * n_out) - max(lo, k * n_out);
}
// the horizontal weighted sum of one source row (at pl + row, a 32-bit offset from the uniform plane pointer: one address register per gather, not two):
// weights sum to 256 (bilinear) or n_in (area; at most ceil(n_in / n_out) + 1 taps, each k < n_in)
template <int FILTER> __device__ static __forceinline__ uint32_t hsum(const uint8_t *pl, uint32_t row, const Axis &AX, const Tap &tx) {
    if (FILTER == 0) return static_cast<uint32_t>((256 - tx.f) * pl[row + static_cast<uint32_t>(tx.a)] + tx.f * pl[row + static_cast<uint32_t>(tx.b)]);
    uint32_t s = 0;
    const uint32_t hi = tx.lo + static_cast<uint32_t>(AX.n_in), n_out = static_cast<uint32_t>(AX.n_out);
    for (uint32_t k = static_cast<uint32_t>(tx.a); k * n_out < hi; k++) s += overlap(AX, tx.lo, k) * pl[row + k];
    return s;
}
// one scaled sample of a display plane (row r at pl + r * pitch; a plane of a frame is far below 2^32 bytes)
template <int FILTER> __device__ static __forceinline__ uint32_t sample(const uint8_t *pl, int pitch, const Axis &AX, const Axis &AY, const Tap &tx, const Tap &ty) {
    const uint32_t up = static_cast<uint32_t>(pitch);
    if (FILTER == 0) {
        const uint32_t top = hsum<0>(pl, static_cast<uint32_t>(ty.a) * up, AX, tx), bot = hsum<0>(pl, static_cast<uint32_t>(ty.b) * up, AX, tx);
        return ((256 - ty.f) * top + ty.f * bot + 32768u) >> 16; // < 2^24 before the shift
    }
    // sums of up to 255 w h + (w h >> 1) < 2^32: plain 32-bit multiplies, not 24-bit ones
    uint32_t s = 0;
    const uint32_t hi = ty.lo + static_cast<uint32_t>(AY.n_in), n_out = static_cast<uint32_t>(AY.n_out);
    for (uint32_t k = static_cast<uint32_t>(ty.a); k * n_out < hi; k++) s += overlap(AY, ty.lo, k) * hsum<1>(pl, k * up, AX, tx);
    const uint32_t den = static_cast<uint32_t>(AX.n_in) * static_cast<uint32_t>(AY.n_in);
    return (s + (den >> 1)) / den;
}
