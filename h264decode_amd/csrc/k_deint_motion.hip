// h264decode_amd/csrc/k_deint_motion.hip -- K10, motion-adaptive: deinterlace a list of frames, each against a predecessor frame of the same size, into
// frame slots of their own (the rule of include/h264mi.h, "Motion-adaptive deinterlacing").  The structure is k_deint.hip's: blockIdx.x = item,
// blockIdx.y = a chunk of `pairs_per_block` row pairs of the luma-then-chroma row space, a thread owns 16 columns of rows 2q and 2q + 1 of one plane -- the
// kept row of that pair, which is copied, and the missing row beside it.  The missing row is the spatial value (FIELD's average or EDGE's direction
// search: k_deint_rule.h, the code k_deint runs) pulled to within m of the woven sample, m the largest move of the three rows since the predecessor.
// Source, predecessor and destination have the same layout (a frame slot of the coded size), so where all three, the origin and the width are 16-byte
// aligned a thread moves 16 bytes at a time (1080p: always), single bytes otherwise; every clamp is at the edge of the display plane.
// A streaming kernel: with a predecessor a row pair costs six 16-byte loads and two stores per thread item, and the differences, the maximum and the
// clamp run in packed 16-bit lanes (two samples an instruction), so that the arithmetic stays below the direction search's.
#include "mi_kernels.h"
#include "k_deint_rule.h" // load16, avg4, edge16 (shared with k_deint.hip); pack4, byte_of, store16

typedef short pk16 __attribute__((ext_vector_type(2)));

// bytes 0 and 2 (ODD: 1 and 3) of a word as two 16-bit lanes: one byte permute
template <bool ODD> __device__ static __forceinline__ pk16 lanes_of(uint32_t w) { return __builtin_bit_cast(pk16, __builtin_amdgcn_perm(0u, w, ODD ? 0x0c030c01u : 0x0c020c00u)); }
__device__ static __forceinline__ pk16 absdiff(pk16 a, pk16 b) { return __builtin_elementwise_max(a, b) - __builtin_elementwise_min(a, b); }

// two samples of a missing row: min(max(sp, t - m), t + m), m = max(|su - pu|, |sd - pd|, |t - pt|); every value is 0 .. 255, so t - m >= -255 and
// t + m <= 510 fit a signed lane, and the result is 0 .. 255 again (it lies between sp and t)
__device__ static __forceinline__ pk16 pull2(pk16 sp, pk16 t, pk16 su, pk16 sd, pk16 pu, pk16 pd, pk16 pt) {
    const pk16 m = __builtin_elementwise_max(__builtin_elementwise_max(absdiff(su, pu), absdiff(sd, pd)), absdiff(t, pt));
    return __builtin_elementwise_min(__builtin_elementwise_max(sp, t - m), t + m);
}
// the four samples of a word
__device__ static __forceinline__ uint32_t pull4(uint32_t sp, uint32_t t, uint32_t su, uint32_t sd, uint32_t pu, uint32_t pd, uint32_t pt) {
    const pk16 e = pull2(lanes_of<false>(sp), lanes_of<false>(t), lanes_of<false>(su), lanes_of<false>(sd), lanes_of<false>(pu), lanes_of<false>(pd), lanes_of<false>(pt));
    const pk16 o = pull2(lanes_of<true>(sp), lanes_of<true>(t), lanes_of<true>(su), lanes_of<true>(sd), lanes_of<true>(pu), lanes_of<true>(pd), lanes_of<true>(pt));
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, o), __builtin_bit_cast(uint32_t, e), 0x06020400u); // e0, o0, e1, o1
}

// rows 2q and 2q + 1, columns 16 g .. of one display plane of wp x hp samples (row r at sp + r * pitch; the predecessor's plane at pp and the destination
// plane at dp alike).  MODE: H264MI_DEINT_FIELD 0 or _EDGE 2 (edge: this plane takes the EDGE rule -- luma; chroma follows FIELD); P: the parity kept;
// PREV: there is a predecessor (without one the missing row is the spatial value, k_deint's frame bit for bit)
template <int MODE, int P, bool VEC, bool PREV>
__device__ static __forceinline__ void motion_item(const uint8_t *sp, const uint8_t *pp, uint8_t *dp, int pitch, int wp, int hp, int q, int g, bool edge) {
    const int x = 16 * g, n = min(16, wp - x);
    const int B = 2 * q, C = B + 1; // B < hp
    const bool has_c = C < hp;      // odd hp: the last pair is one row
    const uint8_t *s = sp + x;
    uint8_t *o = dp + x;
    const size_t up = static_cast<size_t>(pitch);
    // the kept row is copied; the missing row's neighbours are kept rows: the one of this pair and one of a neighbouring pair
    uint32_t u[4], d[4], v[4];
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
        if (ru < 0) ru = rd = B; // a plane of one row: neither exists, the row is copied (with a predecessor: m = 0 pulls it to itself)
        load16<VEC>(s + up * ru, n, u);
        if (has_c) {
            load16<VEC>(s + up * C, n, d);
            store16<VEC>(o + up * C, n, d);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = u[k];
        }
    }
    uint32_t t[4], pu[4], pd[4], pt[4];
    if (PREV) { // issued before the spatial arithmetic, which needs none of them
        const uint8_t *p = pp + x;
        load16<VEC>(s + up * miss, n, t);
        load16<VEC>(p + up * ru, n, pu);
        load16<VEC>(p + up * rd, n, pd);
        load16<VEC>(p + up * miss, n, pt);
    }
    if (MODE == 2 && edge) {
        const uint8_t *qu = sp + up * ru, *qd = sp + up * rd;
        const int xl = max(x - 1, 0), xr = min(x + 16, wp - 1);
        edge16(u, d, qu[xl], qu[xr], qd[xl], qd[xr], v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = avg4(u[k], d[k]);
    }
    if (PREV) {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = pull4(v[k], t[k], u[k], d[k], pu[k], pd[k], pt[k]);
    }
    store16<VEC>(o + up * miss, n, v);
}

template <int MODE, int P, bool PREV>
__device__ static __forceinline__ void motion_chunk(const DeintMotionDesc &dd, const uint8_t *src, const uint8_t *prev, uint8_t *out, int pairs_per_block) {
    const int w = static_cast<int>(dd.w), h = static_cast<int>(dd.h), W = static_cast<int>(dd.W), H = static_cast<int>(dd.H);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2, Wc = W / 2;
    const int np_y = (h + 1) / 2, np_c = (hc + 1) / 2, ng_y = (w + 15) / 16, ng_c = (wc + 15) / 16;
    const int slots = 2 * ng_c; // thread items per row pair: >= ng_y
    // W is a multiple of 16, so luma rows stay aligned when the origin is; chroma rows, planes and origin need the same of W / 2, x0 / 2 and ceil(w / 2)
    const bool vec_y = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(out) | dd.x0 | dd.w) & 15) == 0;
    const bool vec_c = vec_y && ((dd.W | dd.x0 | dd.w) & 31) == 0;
    const int j0 = static_cast<int>(blockIdx.y) * pairs_per_block, items = min(pairs_per_block, np_y + np_c - j0) * slots; // (<= 0 beyond the last pair)
    for (int i = static_cast<int>(threadIdx.x); i < items; i += 256) {
        const int j = j0 + i / slots, sl = i % slots;
        if (j < np_y) {
            if (sl >= ng_y) continue;
            const size_t org = static_cast<size_t>(dd.y0) * W + dd.x0;
            if (vec_y) motion_item<MODE, P, true, PREV>(src + org, prev + org, out + org, W, w, h, j, sl, true);
            else motion_item<MODE, P, false, PREV>(src + org, prev + org, out + org, W, w, h, j, sl, true);
        } else {
            const int c = sl >= ng_c;
            const size_t org = static_cast<size_t>(W) * H + static_cast<size_t>(c) * Wc * (H / 2) + static_cast<size_t>(dd.y0 / 2) * Wc + dd.x0 / 2;
            if (vec_c) motion_item<MODE, P, true, PREV>(src + org, prev + org, out + org, Wc, wc, hc, j - np_y, sl - c * ng_c, false);
            else motion_item<MODE, P, false, PREV>(src + org, prev + org, out + org, Wc, wc, hc, j - np_y, sl - c * ng_c, false);
        }
    }
}

template <int MODE, int P> __device__ static __forceinline__ void motion_prev(const DeintMotionDesc &dd, uint8_t *out, int pairs_per_block) {
    const uint8_t *src = reinterpret_cast<const uint8_t *>(dd.src), *prev = reinterpret_cast<const uint8_t *>(dd.prev);
    if (prev) motion_chunk<MODE, P, true>(dd, src, prev, out, pairs_per_block);
    else motion_chunk<MODE, P, false>(dd, src, src, out, pairs_per_block); // (never read)
}

extern "C" __global__ void __launch_bounds__(256) k_deint_motion(const DeintMotionDesc *descs, uint8_t *dst, int pairs_per_block) {
    const DeintMotionDesc dd = descs[blockIdx.x];
    uint8_t *out = dst + dd.dst_off;
    if (dd.mode == 0) {
        if (dd.parity) motion_prev<0, 1>(dd, out, pairs_per_block);
        else motion_prev<0, 0>(dd, out, pairs_per_block);
    } else if (dd.mode == 2) {
        if (dd.parity) motion_prev<2, 1>(dd, out, pairs_per_block);
        else motion_prev<2, 0>(dd, out, pairs_per_block);
    }
}
