// h264decode_amd/csrc/k_convert.hip -- K7: crop + convert a list of frames to NV12 / RGB24 / planar RGB (the rule of include/h264mi.h, "Output formats").
// One launch converts any number of frames (a whole batch): blockIdx.x = frame, blockIdx.y = a chunk of `pairs_per_block` luma row pairs.  A thread
// owns two luma rows x 16 columns and the 8 (Cb, Cr) pairs under them; chroma is read from the frame pool through the crop origin, clamped at the
// edges of the DISPLAY chroma plane, so the result is a function of the tight I420 frame alone.  When source rows, destination rows and the width
// are 16-byte aligned (1080p: always) a thread loads 16 luma bytes / 8 chroma bytes and stores 16 bytes at a time; single bytes otherwise.
#include "mi_kernels.h"

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
// chroma samples k .. k + 8 of a display chroma row (columns clamped to last): 8 bytes + 1 on the aligned path
template <bool VEC, bool NINE> __device__ static __forceinline__ void load_chroma(const uint8_t *row, int k, int last, uint32_t o[9]) {
    if (VEC) {
        const uint2 v = *reinterpret_cast<const uint2 *>(row + k);
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = byte_of(i < 4 ? v.x : v.y, i & 3);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = row[min(k + i, last)];
    }
    o[8] = NINE ? row[min(k + 8, last)] : 0;
}
template <bool VEC> __device__ static __forceinline__ void store16(uint8_t *p, int n, const uint32_t v[4]) {
    if (VEC) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i < n) p[i] = static_cast<uint8_t>(byte_of(v[i >> 2], i & 3));
    }
}

// FMT: 1 NV12, 2 RGB24, 3 planar RGB (H264MI_FMT_*)
template <int FMT, bool BILIN, bool VEC> __device__ static __forceinline__ void convert_item(const ConvDesc &cd, const uint8_t *src, uint8_t *out, int j, int g) {
    const int w = static_cast<int>(cd.w), h = static_cast<int>(cd.h), W = static_cast<int>(cd.W), H = static_cast<int>(cd.H);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2, Wc = W / 2;
    const int x = 16 * g, k = 8 * g, n = min(16, w - x), nc = min(8, wc - k);
    const bool two = 2 * j + 1 < h; // odd h (monochrome streams only): the last row pair is one row
    const uint8_t *sy = src + static_cast<size_t>(cd.y0 + 2 * j) * W + cd.x0 + x;
    const uint8_t *cbp = src + static_cast<size_t>(W) * H + static_cast<size_t>(cd.y0 / 2) * Wc + cd.x0 / 2; // display chroma plane: row r at + r * Wc
    const uint8_t *crp = cbp + static_cast<size_t>(Wc) * (H / 2);
    uint32_t Y[2][4];
    load16<VEC>(sy, n, Y[0]);
    load16<VEC>(sy + (two ? W : 0), n, Y[1]);
    const size_t npix = static_cast<size_t>(w) * h;
    if (FMT == 1) { // no conversion: the luma rows, then one row of (Cb, Cr) pairs
        uint32_t cb[9], cr[9], o[4];
        load_chroma<VEC, false>(cbp + static_cast<size_t>(j) * Wc, k, wc - 1, cb);
        load_chroma<VEC, false>(crp + static_cast<size_t>(j) * Wc, k, wc - 1, cr);
        store16<VEC>(out + static_cast<size_t>(2 * j) * w + x, n, Y[0]);
        if (two) store16<VEC>(out + static_cast<size_t>(2 * j + 1) * w + x, n, Y[1]);
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = pack4(cb[2 * q], cr[2 * q], cb[2 * q + 1], cr[2 * q + 1]);
        store16<VEC>(out + npix + static_cast<size_t>(j) * (2 * wc) + 2 * k, 2 * nc, o);
        return;
    }
    // chroma of each of the 2 x 16 pixels, minus 128
    int U[2][16], V[2][16];
    if (!BILIN) {
        uint32_t cb[9], cr[9];
        load_chroma<VEC, false>(cbp + static_cast<size_t>(j) * Wc, k, wc - 1, cb);
        load_chroma<VEC, false>(crp + static_cast<size_t>(j) * Wc, k, wc - 1, cr);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            U[0][i] = U[1][i] = static_cast<int>(cb[i >> 1]) - 128;
            V[0][i] = V[1][i] = static_cast<int>(cr[i >> 1]) - 128;
        }
    } else {
        // rows j - 1, j, j + 1 clamped to the display plane; Hrow = 2 c[k] (even x) or c[k] + c[k + 1] (odd x); (3 Hrow(j) + Hrow(j') + 4) >> 3
        const int jm = max(j - 1, 0), jp = min(j + 1, hc - 1);
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const uint8_t *pl = p ? crp : cbp;
            uint32_t a[9], b[9], c[9];
            load_chroma<VEC, true>(pl + static_cast<size_t>(jm) * Wc, k, wc - 1, a);
            load_chroma<VEC, true>(pl + static_cast<size_t>(j) * Wc, k, wc - 1, b);
            load_chroma<VEC, true>(pl + static_cast<size_t>(jp) * Wc, k, wc - 1, c);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int q = i >> 1, q1 = q + (i & 1);
                const int ha = static_cast<int>(a[q] + a[q1]), hb = static_cast<int>(b[q] + b[q1]), hcc = static_cast<int>(c[q] + c[q1]);
                const int top = ((3 * hb + ha + 4) >> 3) - 128, bot = ((3 * hb + hcc + 4) >> 3) - 128;
                if (p) V[0][i] = top, V[1][i] = bot;
                else U[0][i] = top, U[1][i] = bot;
            }
        }
    }
    const int32_t *cf = k_csc_coeffs[cd.cset & 3];
    const int cy = cf[0], crv = cf[1], cgu = cf[2], cgv = cf[3], cbu = cf[4];
    const int yoff = (cd.cset & 1) ? 0 : 16; // odd sets are full range
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r && !two) break;
        uint32_t R[16], G[16], B[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            // every factor fits 24 bits (coefficients < 2^15, samples within +-256): v_mad_i32_i24, not the quarter-rate 32-bit multiply
            const int t = __mul24(cy, static_cast<int>(byte_of(Y[r][i >> 2], i & 3)) - yoff) + 4096;
            R[i] = clip255((t + __mul24(crv, V[r][i])) >> 13);
            G[i] = clip255((t - __mul24(cgu, U[r][i]) - __mul24(cgv, V[r][i])) >> 13);
            B[i] = clip255((t + __mul24(cbu, U[r][i])) >> 13);
        }
        const size_t row = static_cast<size_t>(2 * j + r) * w + x;
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

template <int FMT, bool BILIN, bool VEC> __device__ static __forceinline__ void convert_chunk(const ConvDesc &cd, const uint8_t *src, uint8_t *out, int pairs_per_block) {
    const int ngroups = (static_cast<int>(cd.w) + 15) / 16, npairs = (static_cast<int>(cd.h) + 1) / 2;
    const int j0 = static_cast<int>(blockIdx.y) * pairs_per_block, items = min(pairs_per_block, npairs - j0) * ngroups; // (<= 0 beyond the frame's last pair)
    for (int i = static_cast<int>(threadIdx.x); i < items; i += 256) convert_item<FMT, BILIN, VEC>(cd, src, out, j0 + i / ngroups, i % ngroups);
}

extern "C" __global__ void __launch_bounds__(256) k_convert(const ConvDesc *descs, uint8_t *dst, int pairs_per_block) {
    const ConvDesc cd = descs[blockIdx.x];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(cd.src);
    uint8_t *out = dst + cd.dst_off;
    // W is a multiple of 16, so rows stay aligned when the origin is; w % 16 == 0 makes every thread's 16 columns whole and every destination row
    // (w, 2 * ceil(w / 2) = w or 3 w bytes) and plane (w * h bytes) a multiple of 16
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out) | cd.x0 | cd.w) & 15) == 0;
    const bool bilin = cd.bilinear != 0;
    if (cd.format == 1) {
        if (vec) convert_chunk<1, false, true>(cd, src, out, pairs_per_block);
        else convert_chunk<1, false, false>(cd, src, out, pairs_per_block);
    } else if (cd.format == 2) {
        if (vec) { if (bilin) convert_chunk<2, true, true>(cd, src, out, pairs_per_block); else convert_chunk<2, false, true>(cd, src, out, pairs_per_block); }
        else { if (bilin) convert_chunk<2, true, false>(cd, src, out, pairs_per_block); else convert_chunk<2, false, false>(cd, src, out, pairs_per_block); }
    } else if (cd.format == 3) {
        if (vec) { if (bilin) convert_chunk<3, true, true>(cd, src, out, pairs_per_block); else convert_chunk<3, false, true>(cd, src, out, pairs_per_block); }
        else { if (bilin) convert_chunk<3, true, false>(cd, src, out, pairs_per_block); else convert_chunk<3, false, false>(cd, src, out, pairs_per_block); }
    }
}
