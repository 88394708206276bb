// h264decode_amd/csrc/k_scale.hip -- K8: crop + scale a list of frames to one output size + convert to I420 / NV12 / RGB24 / planar RGB (the rule of
// include/h264mi.h, "Scaled output").  One launch scales any number of frames (a whole batch, of unlike display sizes): blockIdx.x = frame,
// blockIdx.y = a chunk of `pairs_per_block` OUTPUT luma row pairs.  A thread owns two output luma rows x 16 columns and the 8 scaled (Cb, Cr) pairs
// under them, and converts them by K7's rule (k_convert.hip) applied to the scaled frame; the scaled I420 frame exists in registers only.
// Every source sample is gathered from the frame pool through the crop origin, with every clamp at the edges of the DISPLAY planes, so the result is
// a function of the tight I420 frame, the output size and the filter.  The rule, per plane (luma w x h -> ow x oh, each chroma plane
// ceil(w / 2) x ceil(h / 2) -> ceil(ow / 2) x ceil(oh / 2), centre-aligned as planes) and per axis of n_in samples scaled to n_out, output index i:
//   bilinear: step = (n_in << 16) / n_out, P = clamp(i step + (step >> 1) - 32768, 0, (n_in - 1) << 16), a = P >> 16, f = (P >> 8) & 255, b = min(a + 1, n_in - 1);
//             ((256 - fy) ((256 - fx) S[ay][ax] + fx S[ay][bx]) + fy ((256 - fx) S[by][ax] + fx S[by][bx]) + 32768) >> 16      (one rounding)
//   area:     weight of source sample k = overlap of [i n_in, (i + 1) n_in) with [k n_out, (k + 1) n_out) (they sum to n_in);
//             (sum_y wy sum_x wx S + ((w_p h_p) >> 1)) / (w_p h_p), w_p x h_p the source plane; unsigned 32 bits (the host refuses 255 w h + (w h >> 1) >= 2^32)
// In bilinear mode step and the half-step offset come from the descriptor: nothing is divided.  Stores are 16 bytes (8 for an I420 chroma row) when
// the destination and ow are 16-byte aligned, single bytes otherwise; the gathers are byte loads (neighbouring lanes read neighbouring cache lines).
#include "mi_kernels.h"
#include "k_output_rule.h" // the sampling rule and K7's conversion

template <bool VEC> __device__ static __forceinline__ void store8(uint8_t *p, int n, const uint32_t v[8]) {
    if (VEC) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7]));
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (i < n) p[i] = static_cast<uint8_t>(v[i]);
    }
}

// FILTER: H264MI_SCALE_*; FMT: H264MI_FMT_* (0 I420, 1 NV12, 2 RGB24, 3 planar RGB)
template <int FILTER, int FMT, bool BILIN, bool VEC>
__device__ static __forceinline__ void scale_item(const ScaleDesc &sd, const uint8_t *src, uint8_t *out, int ow, int oh, int j, int g) {
    const int w = static_cast<int>(sd.w), h = static_cast<int>(sd.h), W = static_cast<int>(sd.W), H = static_cast<int>(sd.H);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2, Wc = W / 2, owc = (ow + 1) / 2, ohc = (oh + 1) / 2;
    const int x = 16 * g, k = 8 * g, n = min(16, ow - x), nc = min(8, owc - k);
    const bool two = 2 * j + 1 < oh; // odd oh: the last row pair is one row
    const uint8_t *yp = src + static_cast<size_t>(sd.y0) * W + sd.x0;                                        // display luma plane: row r at + r * W
    const uint8_t *cbp = src + static_cast<size_t>(W) * H + static_cast<size_t>(sd.y0 / 2) * Wc + sd.x0 / 2; // display chroma plane: row r at + r * Wc
    const uint8_t *crp = cbp + static_cast<size_t>(Wc) * (H / 2);
    const Axis LX = {w, ow, static_cast<int>(sd.step[0]), sd.half[0]}, LY = {h, oh, static_cast<int>(sd.step[1]), sd.half[1]};
    const Axis CX = {wc, owc, static_cast<int>(sd.step[2]), sd.half[2]}, CY = {hc, ohc, static_cast<int>(sd.step[3]), sd.half[3]};

    // the two scaled luma rows (columns beyond the frame repeat the last one; they are never stored)
    uint32_t Y[2][4];
    {
        const Tap ty0 = tap_of<FILTER>(LY, 2 * j), ty1 = tap_of<FILTER>(LY, min(2 * j + 1, oh - 1));
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t v0[4], v1[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const Tap tx = tap_of<FILTER>(LX, min(x + 4 * q + i, ow - 1));
                v0[i] = sample<FILTER>(yp, W, LX, LY, tx, ty0);
                v1[i] = sample<FILTER>(yp, W, LX, LY, tx, ty1);
            }
            Y[0][q] = pack4(v0[0], v0[1], v0[2], v0[3]);
            Y[1][q] = pack4(v1[0], v1[1], v1[2], v1[3]);
        }
    }
    const size_t npix = static_cast<size_t>(ow) * oh;
    if (FMT == 0 || FMT == 1) { // no conversion: the scaled luma rows and the scaled chroma row j (ohc = the number of row pairs: j < ohc)
        uint32_t cb[8], cr[8];
        const Tap ty = tap_of<FILTER>(CY, j);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const Tap tx = tap_of<FILTER>(CX, min(k + i, owc - 1));
            cb[i] = sample<FILTER>(cbp, Wc, CX, CY, tx, ty);
            cr[i] = sample<FILTER>(crp, Wc, CX, CY, tx, ty);
        }
        store16<VEC>(out + static_cast<size_t>(2 * j) * ow + x, n, Y[0]);
        if (two) store16<VEC>(out + static_cast<size_t>(2 * j + 1) * ow + x, n, Y[1]);
        if (FMT == 0) {
            uint8_t *oc = out + npix + static_cast<size_t>(j) * owc + k;
            store8<VEC>(oc, nc, cb);
            store8<VEC>(oc + static_cast<size_t>(owc) * ohc, nc, cr);
        } else {
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = pack4(cb[2 * q], cr[2 * q], cb[2 * q + 1], cr[2 * q + 1]);
            store16<VEC>(out + npix + static_cast<size_t>(j) * (2 * owc) + 2 * k, 2 * nc, o);
        }
        return;
    }
    // chroma of each of the 2 x 16 pixels, minus 128: K7's upsampling of the SCALED chroma planes (owc x ohc)
    int U[2][16], V[2][16];
    if (!BILIN) {
        const Tap ty = tap_of<FILTER>(CY, j);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const Tap tx = tap_of<FILTER>(CX, min(k + i, owc - 1));
            const int cb = static_cast<int>(sample<FILTER>(cbp, Wc, CX, CY, tx, ty)) - 128, cr = static_cast<int>(sample<FILTER>(crp, Wc, CX, CY, tx, ty)) - 128;
            U[0][2 * i] = U[0][2 * i + 1] = U[1][2 * i] = U[1][2 * i + 1] = cb;
            V[0][2 * i] = V[0][2 * i + 1] = V[1][2 * i] = V[1][2 * i + 1] = cr;
        }
    } else {
        // scaled chroma rows j - 1, j, j + 1 and columns k .. k + 8, clamped to the scaled plane, recomputed here (no intermediate buffer)
        const Tap tya = tap_of<FILTER>(CY, max(j - 1, 0)), tyb = tap_of<FILTER>(CY, j), tyc = tap_of<FILTER>(CY, min(j + 1, ohc - 1));
        uint32_t a[2][9], b[2][9], c[2][9]; // [Cb, Cr]: both planes of a column together -- they share its taps, which then die with the column
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const Tap tx = tap_of<FILTER>(CX, min(k + i, owc - 1));
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const uint8_t *pl = p ? crp : cbp;
                a[p][i] = sample<FILTER>(pl, Wc, CX, CY, tx, tya);
                b[p][i] = sample<FILTER>(pl, Wc, CX, CY, tx, tyb);
                c[p][i] = sample<FILTER>(pl, Wc, CX, CY, tx, tyc);
            }
        }
#pragma unroll
        for (int p = 0; p < 2; p++) upsample_chroma<16>(a[p], b[p], c[p], p ? V[0] : U[0], p ? V[1] : U[1]);
    }
    store_rgb_rows<FMT, VEC>(out, ow, npix, j, x, n, two, sd.cset, Y, U, V);
}

template <int FILTER, int FMT, bool BILIN, bool VEC>
__device__ static __forceinline__ void scale_chunk(const ScaleDesc &sd, const uint8_t *src, uint8_t *out, int ow, int oh, int pairs_per_block) {
    const int ngroups = (ow + 15) / 16, npairs = (oh + 1) / 2;
    const int j0 = static_cast<int>(blockIdx.y) * pairs_per_block, items = min(pairs_per_block, npairs - j0) * ngroups; // (<= 0 beyond the last pair)
    for (int i = static_cast<int>(threadIdx.x); i < items; i += 256) scale_item<FILTER, FMT, BILIN, VEC>(sd, src, out, ow, oh, j0 + i / ngroups, i % ngroups);
}

// format, chroma mode and store path of a frame, for one filter
template <int FILTER> __device__ static __forceinline__ void scale_frame(const ScaleDesc &sd, const uint8_t *src, uint8_t *out, int ow, int oh, int ppb, bool vec) {
    const bool bilin = sd.bilinear != 0;
    switch (sd.format) {
    case 0:
        if (vec) scale_chunk<FILTER, 0, false, true>(sd, src, out, ow, oh, ppb);
        else scale_chunk<FILTER, 0, false, false>(sd, src, out, ow, oh, ppb);
        break;
    case 1:
        if (vec) scale_chunk<FILTER, 1, false, true>(sd, src, out, ow, oh, ppb);
        else scale_chunk<FILTER, 1, false, false>(sd, src, out, ow, oh, ppb);
        break;
    case 2:
        if (vec) { if (bilin) scale_chunk<FILTER, 2, true, true>(sd, src, out, ow, oh, ppb); else scale_chunk<FILTER, 2, false, true>(sd, src, out, ow, oh, ppb); }
        else { if (bilin) scale_chunk<FILTER, 2, true, false>(sd, src, out, ow, oh, ppb); else scale_chunk<FILTER, 2, false, false>(sd, src, out, ow, oh, ppb); }
        break;
    case 3:
        if (vec) { if (bilin) scale_chunk<FILTER, 3, true, true>(sd, src, out, ow, oh, ppb); else scale_chunk<FILTER, 3, false, true>(sd, src, out, ow, oh, ppb); }
        else { if (bilin) scale_chunk<FILTER, 3, true, false>(sd, src, out, ow, oh, ppb); else scale_chunk<FILTER, 3, false, false>(sd, src, out, ow, oh, ppb); }
        break;
    }
}

template <int FILTER> __device__ static __forceinline__ void scale_block(const ScaleDesc *descs, uint8_t *dst, int ow, int oh, int pairs_per_block) {
    const ScaleDesc sd = descs[blockIdx.x];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(sd.src);
    uint8_t *out = dst + sd.dst_off;
    // ow % 16 == 0 makes every thread's 16 columns whole and every destination row (ow, 2 * (ow / 2) or 3 ow bytes) and luma / RGB plane (ow * oh bytes) a
    // multiple of 16; an I420 chroma row (ow / 2) and plane are then multiples of 8, which is what its 8-byte stores need
    const bool vec = ((reinterpret_cast<uintptr_t>(out) | static_cast<uintptr_t>(ow)) & 15) == 0;
    scale_frame<FILTER>(sd, src, out, ow, oh, pairs_per_block, vec);
}

// one entry point per filter (the filter is uniform per call): the register budget of the bilinear kernel is not the area kernel's
extern "C" __global__ void __launch_bounds__(256) k_scale(const ScaleDesc *descs, uint8_t *dst, int ow, int oh, int pairs_per_block) {
    scale_block<0>(descs, dst, ow, oh, pairs_per_block);
}
extern "C" __global__ void __launch_bounds__(256, 2) k_scale_area(const ScaleDesc *descs, uint8_t *dst, int ow, int oh, int pairs_per_block) {
    scale_block<1>(descs, dst, ow, oh, pairs_per_block);
}
