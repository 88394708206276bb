// h264decode_amd/csrc/k_deint.hip -- K10: deinterlace a list of frames into frame slots of their own (the rule of include/h264mi.h, "Deinterlaced output").
// One launch takes any number of (frame, mode, parity) items: blockIdx.x = item, blockIdx.y = a chunk of `pairs_per_block` row pairs of ONE row space --
// the luma row pairs, then the chroma row pairs, where a chroma row pair holds the Cb rows in its first ceil(wc / 16) column groups and the Cr rows in
// the next ones, so that a chroma row pair is about as many thread items as a luma one.  A thread owns 16 columns of rows 2q and 2q + 1 of one plane:
// the kept row of that pair and the missing row beside it.  Source and destination have the same layout (a frame slot of the coded size; only the display
// rectangle is read and written), so where rows, origin and width are 16-byte aligned a thread moves 16 bytes at a time (1080p: always), single
// bytes otherwise; every clamp is at the edge of the display plane.
#include "mi_kernels.h"
#include "k_deint_rule.h" // load16, avg4, edge16 (shared with k_deint_motion.hip); pack4, byte_of, store16

// BLEND: (a + 2 b + c + 2) >> 2 of the four bytes of a word, in two words of two 16-bit lanes (the sum is at most 1022): ONE rounding, which a chain of
// two rounded averages is not
__device__ static __forceinline__ uint32_t blend4(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t m = 0x00ff00ffu;
    const uint32_t lo = (a & m) + 2 * (b & m) + (c & m) + 0x00020002u, hi = ((a >> 8) & m) + 2 * ((b >> 8) & m) + ((c >> 8) & m) + 0x00020002u;
    return ((lo >> 2) & m) | (((hi >> 2) & m) << 8);
}

// rows 2q and 2q + 1, columns 16 g .. of one display plane of wp x hp samples (row r at sp + r * pitch; the destination plane at dp alike)
// MODE: H264MI_DEINT_FIELD 0, _BLEND 1, _EDGE 2 (edge: this plane takes the EDGE rule -- luma; chroma follows FIELD); P: the parity kept
template <int MODE, int P, bool VEC>
__device__ static __forceinline__ void deint_item(const uint8_t *sp, uint8_t *dp, int pitch, int wp, int hp, int q, int g, bool edge) {
    const int x = 16 * g, n = min(16, wp - x);
    const int B = 2 * q, C = B + 1; // B < hp
    const bool has_c = C < hp;      // odd hp: the last pair is one row
    const uint8_t *s = sp + x;
    uint8_t *o = dp + x;
    const size_t up = static_cast<size_t>(pitch);
    uint32_t v[4];
    if (MODE == 1) {
        uint32_t a[4], b[4], c[4], e[4];
        load16<VEC>(s + up * max(B - 1, 0), n, a);
        load16<VEC>(s + up * B, n, b);
        load16<VEC>(s + up * min(C, hp - 1), n, c);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = blend4(a[k], b[k], c[k]);
        store16<VEC>(o + up * B, n, v);
        if (!has_c) return;
        load16<VEC>(s + up * min(C + 1, hp - 1), n, e);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = blend4(b[k], c[k], e[k]);
        store16<VEC>(o + up * C, n, v);
        return;
    }
    // the kept row is copied; the missing row comes from the rows above and below it, which are kept rows: the one of this pair and one of a neighbouring pair
    uint32_t u[4], d[4];
    int miss, ru, rd; // the missing row, the rows above and below it after the clamp
    if (P == 0) {
        load16<VEC>(s + up * B, n, u);
        store16<VEC>(o + up * B, n, u);
        if (!has_c) return;
        miss = C, ru = B, rd = C + 1 < hp ? C + 1 : B;
        load16<VEC>(s + up * rd, n, d);
    } else {
        miss = B, ru = B - 1, rd = has_c ? C : -1;
        if (ru < 0) ru = rd;
        if (rd < 0) rd = ru;
        if (ru < 0) ru = rd = B; // a plane of one row: neither exists, the row is copied
        load16<VEC>(s + up * ru, n, u);
        if (has_c) {
            load16<VEC>(s + up * C, n, d);
            store16<VEC>(o + up * C, n, d);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = u[k];
        }
    }
    if (MODE == 2 && edge) {
        const uint8_t *pu = sp + up * ru, *pd = sp + up * rd;
        const int xl = max(x - 1, 0), xr = min(x + 16, wp - 1);
        edge16(u, d, pu[xl], pu[xr], pd[xl], pd[xr], v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = avg4(u[k], d[k]);
    }
    store16<VEC>(o + up * miss, n, v);
}

template <int MODE, int P> __device__ static __forceinline__ void deint_chunk(const DeintDesc &dd, const uint8_t *src, uint8_t *out, int pairs_per_block) {
    const int w = static_cast<int>(dd.w), h = static_cast<int>(dd.h), W = static_cast<int>(dd.W), H = static_cast<int>(dd.H);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2, Wc = W / 2;
    const int np_y = (h + 1) / 2, np_c = (hc + 1) / 2, ng_y = (w + 15) / 16, ng_c = (wc + 15) / 16;
    const int slots = 2 * ng_c; // thread items per row pair: >= ng_y
    // W is a multiple of 16, so luma rows stay aligned when the origin is; chroma rows, planes and origin need the same of W / 2, x0 / 2 and ceil(w / 2)
    const bool vec_y = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out) | dd.x0 | dd.w) & 15) == 0;
    const bool vec_c = vec_y && ((dd.W | dd.x0 | dd.w) & 31) == 0;
    const int j0 = static_cast<int>(blockIdx.y) * pairs_per_block, items = min(pairs_per_block, np_y + np_c - j0) * slots; // (<= 0 beyond the last pair)
    for (int i = static_cast<int>(threadIdx.x); i < items; i += 256) {
        const int j = j0 + i / slots, sl = i % slots;
        if (j < np_y) {
            if (sl >= ng_y) continue;
            const size_t org = static_cast<size_t>(dd.y0) * W + dd.x0;
            if (vec_y) deint_item<MODE, P, true>(src + org, out + org, W, w, h, j, sl, true);
            else deint_item<MODE, P, false>(src + org, out + org, W, w, h, j, sl, true);
        } else {
            const int c = sl >= ng_c;
            const size_t org = static_cast<size_t>(W) * H + static_cast<size_t>(c) * Wc * (H / 2) + static_cast<size_t>(dd.y0 / 2) * Wc + dd.x0 / 2;
            if (vec_c) deint_item<MODE, P, true>(src + org, out + org, Wc, wc, hc, j - np_y, sl - c * ng_c, false);
            else deint_item<MODE, P, false>(src + org, out + org, Wc, wc, hc, j - np_y, sl - c * ng_c, false);
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) k_deint(const DeintDesc *descs, uint8_t *dst, int pairs_per_block) {
    const DeintDesc dd = descs[blockIdx.x];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(dd.src);
    uint8_t *out = dst + dd.dst_off;
    if (dd.mode == 1) deint_chunk<1, 0>(dd, src, out, pairs_per_block);
    else if (dd.mode == 0) {
        if (dd.parity) deint_chunk<0, 1>(dd, src, out, pairs_per_block);
        else deint_chunk<0, 0>(dd, src, out, pairs_per_block);
    } else if (dd.mode == 2) {
        if (dd.parity) deint_chunk<2, 1>(dd, src, out, pairs_per_block);
        else deint_chunk<2, 0>(dd, src, out, pairs_per_block);
    }
}
