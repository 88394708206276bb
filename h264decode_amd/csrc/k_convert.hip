// h264decode_amd/csrc/k_convert.hip -- K7: crop + convert a list of frames to NV12 / RGB24 / planar RGB (the rule of include/h264mi.h, "Output formats").
// One launch converts any number of frames (a whole batch): blockIdx.x = frame, blockIdx.y = a chunk of `pairs_per_block` luma row pairs.  A thread
// owns two luma rows x 16 columns and the 8 (Cb, Cr) pairs under them; chroma is read from the frame pool through the crop origin, clamped at the
// edges of the DISPLAY chroma plane, so the result is a function of the tight I420 frame alone.  When source rows, destination rows and the width
// are 16-byte aligned (1080p: always) a thread loads 16 luma bytes / 8 chroma bytes and stores 16 bytes at a time; single bytes otherwise.
#include "mi_kernels.h"
#include "k_output_rule.h" // the conversion itself: K8 and K9 apply the same text to a scaled frame

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
        // rows j - 1, j, j + 1 and columns k .. k + 8, clamped to the display plane
        const int jm = max(j - 1, 0), jp = min(j + 1, hc - 1);
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const uint8_t *pl = p ? crp : cbp;
            uint32_t a[9], b[9], c[9];
            load_chroma<VEC, true>(pl + static_cast<size_t>(jm) * Wc, k, wc - 1, a);
            load_chroma<VEC, true>(pl + static_cast<size_t>(j) * Wc, k, wc - 1, b);
            load_chroma<VEC, true>(pl + static_cast<size_t>(jp) * Wc, k, wc - 1, c);
            if (p) upsample_chroma<16>(a, b, c, V[0], V[1]);
            else upsample_chroma<16>(a, b, c, U[0], U[1]);
        }
    }
    store_rgb_rows<FMT, VEC>(out, w, npix, j, x, n, two, cd.cset, Y, U, V);
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
