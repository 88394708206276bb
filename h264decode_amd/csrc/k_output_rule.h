// h264decode_amd/csrc/k_output_rule.h -- the output rule of include/h264mi.h, one copy for K7 (k_convert.hip), K8 (k_scale.hip) and K9 (k_tensor.hip):
// the conversion of "Output formats" (coefficients, chroma upsampling, YCbCr -> RGB, the RGB24 / planar RGB stores) and the sampling of "Scaled
// output" (bilinear and area taps, one scaled sample of a display plane).  The conversion is K7's, the sampling is K8's.
// Device code only; everything is static and inlined, so each kernel keeps its own register allocation.
#pragma once
#include "mi_kernels.h"

// ---------------------------------------------------------------- the conversion
// {cy, crv, cgu, cgv, cbu} in 1/8192: BT.601 limited, BT.601 full, BT.709 limited, BT.709 full (H264MI_CSC_COEFFS of include/h264mi.h, the same rows)
__device__ static const int32_t k_csc_coeffs[4][5] = {
    {9539, 13075, 3209, 6660, 16525},
    {8192, 11485, 2819, 5850, 14516},
    {9539, 14686, 1747, 4366, 17305},
    {8192, 12901, 1535, 3835, 15201},
};

__device__ static __forceinline__ uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 255u; }
// four values of 0 .. 255 -> one word, by byte permutes (v_perm_b32).  Shifts and ORs are compiled to v_ashr_pk_u8_i32 for the two low bytes with the other two
// ORed onto its result unmasked, and that form gave wrong third bytes on the GPU (profiles/k7_convert.txt) -- presumably the instruction leaves the upper half
// of its destination as it was; the permute form does not depend on it
__device__ static __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return __builtin_amdgcn_perm(b, a, 0x0c0c0400u) | __builtin_amdgcn_perm(d, c, 0x04000c0cu);
}
__device__ static __forceinline__ uint32_t clip255(int v) { return static_cast<uint32_t>(min(max(v, 0), 255)); }

// 16 bytes at p: one store on the aligned path; bytes 0 .. n - 1 otherwise
template <bool VEC> __device__ static __forceinline__ void store16(uint8_t *p, int n, const uint32_t v[4]) {
    if (VEC) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i < n) p[i] = static_cast<uint8_t>(byte_of(v[i >> 2], i & 3));
    }
}

// bilinear chroma upsampling: N / 2 + 1 samples (columns clamped to the plane) of the chroma rows j - 1, j, j + 1 (clamped too) -> the chroma, minus 128,
// of the N pixels of luma rows 2j and 2j + 1.  Hrow = 2 c[k] (even x) or c[k] + c[k + 1] (odd x); (3 Hrow(j) + Hrow(j') + 4) >> 3
template <int N>
__device__ static __forceinline__ void upsample_chroma(const uint32_t (&a)[N / 2 + 1], const uint32_t (&b)[N / 2 + 1], const uint32_t (&c)[N / 2 + 1], int (&top)[N], int (&bot)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int q = i >> 1, q1 = q + (i & 1);
        const int ha = static_cast<int>(a[q] + a[q1]), hb = static_cast<int>(b[q] + b[q1]), hc = static_cast<int>(c[q] + c[q1]);
        top[i] = ((3 * hb + ha + 4) >> 3) - 128, bot[i] = ((3 * hb + hc + 4) >> 3) - 128;
    }
}

// a row of the table, and the luma offset of its range
struct Csc {
    int cy, crv, cgu, cgv, cbu, yoff;
};
__device__ static __forceinline__ Csc csc_of(uint32_t cset) {
    const int32_t *cf = k_csc_coeffs[cset & 3];
    return {cf[0], cf[1], cf[2], cf[3], cf[4], (cset & 1) ? 0 : 16}; // odd sets are full range
}
// one pixel: Y and its chroma minus 128 -> R, G, B of 0 .. 255
__device__ static __forceinline__ void ycc_to_rgb(uint32_t y, int u, int v, const Csc &k, uint32_t &r, uint32_t &g, uint32_t &b) {
    // every factor fits 24 bits (coefficients < 2^15, samples within +-256): v_mad_i32_i24, not the quarter-rate 32-bit multiply
    const int t = __mul24(k.cy, static_cast<int>(y) - k.yoff) + 4096;
    r = clip255((t + __mul24(k.crv, v)) >> 13);
    g = clip255((t - __mul24(k.cgu, u) - __mul24(k.cgv, v)) >> 13);
    b = clip255((t + __mul24(k.cbu, u)) >> 13);
}

// a thread's two luma rows x 16 columns (row 2j + r at out + (2j + r) * pitch + x, columns i < n, the second row only if `two`), converted and stored as
// FMT 2 RGB24 or 3 planar RGB (planes of npix bytes).  Y: four samples a word; U, V: chroma minus 128 per pixel
template <int FMT, bool VEC>
__device__ static __forceinline__ void store_rgb_rows(uint8_t *out, int pitch, size_t npix, int j, int x, int n, bool two, uint32_t cset, const uint32_t (&Y)[2][4],
                                                      const int (&U)[2][16], const int (&V)[2][16]) {
    const Csc k = csc_of(cset);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r && !two) break;
        uint32_t R[16], G[16], B[16];
#pragma unroll
        for (int i = 0; i < 16; i++) ycc_to_rgb(byte_of(Y[r][i >> 2], i & 3), U[r][i], V[r][i], k, R[i], G[i], B[i]);
        const size_t row = static_cast<size_t>(2 * j + r) * pitch + x;
        if (FMT == 2) {
            if (VEC) {
                uint32_t o[12]; // pixels 4q .. 4q + 3 are 12 bytes, three words; the thread's 48 bytes are three 16-byte stores
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = 4 * q;
                    o[3 * q] = pack4(R[i], G[i], B[i], R[i + 1]);
                    o[3 * q + 1] = pack4(G[i + 1], B[i + 1], R[i + 2], G[i + 2]);
                    o[3 * q + 2] = pack4(B[i + 2], R[i + 3], G[i + 3], B[i + 3]);
                }
                uint4 *d = reinterpret_cast<uint4 *>(out + row * 3);
                d[0] = make_uint4(o[0], o[1], o[2], o[3]), d[1] = make_uint4(o[4], o[5], o[6], o[7]), d[2] = make_uint4(o[8], o[9], o[10], o[11]);
            } else {
                uint8_t *d = out + row * 3;
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (i < n) d[3 * i] = static_cast<uint8_t>(R[i]), d[3 * i + 1] = static_cast<uint8_t>(G[i]), d[3 * i + 2] = static_cast<uint8_t>(B[i]);
            }
        } else {
            uint32_t o[4];
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const uint32_t *c = p == 0 ? R : p == 1 ? G : B;
#pragma unroll
                for (int q = 0; q < 4; q++) o[q] = pack4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
                store16<VEC>(out + p * npix + row, n, o);
            }
        }
    }
}

// ---------------------------------------------------------------- the sampling
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
