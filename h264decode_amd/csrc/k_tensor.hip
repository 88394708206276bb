// h264decode_amd/csrc/k_tensor.hip -- K9: a list of (frame, region) items -> model-input tensors (the rule of include/h264mi.h, "Model input").
// One launch takes any number of items: blockIdx.x = item, blockIdx.y = a chunk of `pairs_per_block` row pairs of the canvas.  An item is the region
// of a frame scaled to sw x sh (K8's rule, k_output_rule.h), converted to 8-bit R, G, B (K7's rule on the scaled frame), placed at (px, py) of the
// out_w x out_h canvas with `pad` everywhere else, every 8-bit value v mapped to u8 (v), or to fl32(fl32(float(v) * scale) + bias) as f32, f16 or bf16,
// in three planes or interleaved.  The scaled frame and the 8-bit RGB picture exist in registers only.
// Work: a thread owns two rows x 8 columns, counted from the PICTURE's origin -- rows py + 2j, py + 2j + 1 and columns px + 8g .. px + 8g + 7 of the
// canvas for j, g of either sign -- so that the 2 x 2 alignment of the scaled frame that K7's chroma needs holds whatever px and py are.  Threads
// with j < 0, g < 0 or beyond the picture own padding only and gather nothing; at the right and bottom edges of the picture a thread mixes picture
// and padding per element.  Every store is inside the canvas: columns outside 0 .. out_w - 1 and rows outside 0 .. out_h - 1 are never written.
// Stores: when the item's address, its row length and px are aligned (8 bytes for u8, 16 for the wider types) a thread whose 8 columns all lie in
// the canvas writes whole words -- f16 / bf16 pairs and u8 quads packed by v_perm_b32 -- else it stores element by element.
// The two float operations are compiled with contraction off (elem_bits): hipcc would contract a * b + c into one fused operation by default, and
// its __fmul_rn / __fadd_rn are a plain * and + that it contracts too; the rule excludes the fused result.
#include "mi_kernels.h"
#include "k_output_rule.h"
#include <hip/hip_fp16.h>

enum { DT_U8 = 0, DT_F16 = 1, DT_BF16 = 2, DT_F32 = 3 }; // H264MI_DT_*

template <int DT> struct ElemSize { static constexpr int value = DT == DT_U8 ? 1 : DT == DT_F32 ? 4 : 2; };

// the element of an 8-bit value, as its bit pattern
template <int DT> __device__ static __forceinline__ uint32_t elem_bits(uint32_t v, float scale, float bias) {
#pragma clang fp contract(off) // two roundings, never an fma: __fmul_rn / __fadd_rn are a plain * and + here, which hipcc would contract
    if (DT == DT_U8) return v;
    const float prod = static_cast<float>(v) * scale;
    const float r = prod + bias;
    if (DT == DT_F32) return __float_as_uint(r);
    if (DT == DT_F16) return static_cast<uint32_t>(__half_as_ushort(__float2half_rn(r)));
    const uint32_t u = __float_as_uint(r);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ static __forceinline__ uint32_t pack2(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x05040100u); }

// N elements (bit patterns) in store order at p.  whole: all of them, as words (p aligned to 8 bytes for u8, 16 otherwise; N a multiple of 8);
// else element by element, those with index lo <= e < hi
template <int DT, int N> __device__ static __forceinline__ void store_run(uint8_t *p, const uint32_t (&e)[N], bool whole, int lo, int hi) {
    if (whole) {
        if (DT == DT_U8) {
#pragma unroll
            for (int q = 0; q < N / 8; q++)
                reinterpret_cast<uint2 *>(p)[q] = make_uint2(pack4(e[8 * q], e[8 * q + 1], e[8 * q + 2], e[8 * q + 3]), pack4(e[8 * q + 4], e[8 * q + 5], e[8 * q + 6], e[8 * q + 7]));
        } else if (DT == DT_F32) {
#pragma unroll
            for (int q = 0; q < N / 4; q++) reinterpret_cast<uint4 *>(p)[q] = make_uint4(e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < N / 8; q++)
                reinterpret_cast<uint4 *>(p)[q] = make_uint4(pack2(e[8 * q], e[8 * q + 1]), pack2(e[8 * q + 2], e[8 * q + 3]), pack2(e[8 * q + 4], e[8 * q + 5]), pack2(e[8 * q + 6], e[8 * q + 7]));
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i < lo || i >= hi) continue;
        if (DT == DT_U8) p[i] = static_cast<uint8_t>(e[i]);
        else if (DT == DT_F32) reinterpret_cast<uint32_t *>(p)[i] = e[i];
        else reinterpret_cast<uint16_t *>(p)[i] = static_cast<uint16_t>(e[i]);
    }
}

// rows py + 2j, py + 2j + 1 and columns px + 8g .. + 7 of the canvas of one item
template <int FILTER, bool BILIN, int DT, bool HWC>
__device__ static __forceinline__ void tensor_item(const TensorDesc &td, const TensorParams &P, const uint8_t *src, uint8_t *out, const uint32_t (&padbits)[3], bool aligned, int j, int g) {
    constexpr int ES = ElemSize<DT>::value;
    const int ow = P.ow, oh = P.oh, sw = static_cast<int>(td.sw), sh = static_cast<int>(td.sh);
    const int x = 8 * g, k = 4 * g;
    const int col0 = static_cast<int>(td.px) + x, row0 = static_cast<int>(td.py) + 2 * j; // of the canvas; either may be negative (by less than 8 and 2)
    const int i0 = max(0, -col0), i1 = min(8, ow - col0);                                   // the thread's columns inside the canvas: i0 <= i < i1
    if (i0 >= i1) return;
    const bool whole = aligned && i0 == 0 && i1 == 8;
    const bool inpic = j >= 0 && 2 * j < sh && g >= 0 && x < sw;

    uint32_t Y[2][2]; // the two scaled luma rows, four samples a word
    int U[2][8], V[2][8];
    if (inpic) {
        const int w = static_cast<int>(td.w), h = static_cast<int>(td.h), W = static_cast<int>(td.W), H = static_cast<int>(td.H);
        const int wc = (w + 1) / 2, hc = (h + 1) / 2, Wc = W / 2, swc = (sw + 1) / 2, shc = (sh + 1) / 2;
        // the region frame: luma from (x0, y0), chroma from (x0 / 2, y0 / 2) of the coded planes; every clamp of the taps is at ITS edges
        const uint8_t *yp = src + static_cast<size_t>(td.y0) * W + td.x0;
        const uint8_t *cbp = src + static_cast<size_t>(W) * H + static_cast<size_t>(td.y0 / 2) * Wc + td.x0 / 2;
        const uint8_t *crp = cbp + static_cast<size_t>(Wc) * (H / 2);
        const Axis LX = {w, sw, static_cast<int>(td.step[0]), td.half[0]}, LY = {h, sh, static_cast<int>(td.step[1]), td.half[1]};
        const Axis CX = {wc, swc, static_cast<int>(td.step[2]), td.half[2]}, CY = {hc, shc, static_cast<int>(td.step[3]), td.half[3]};
        {
            const Tap ty0 = tap_of<FILTER>(LY, 2 * j), ty1 = tap_of<FILTER>(LY, min(2 * j + 1, sh - 1));
#pragma unroll
            for (int q = 0; q < 2; q++) {
                uint32_t v0[4], v1[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const Tap tx = tap_of<FILTER>(LX, min(x + 4 * q + i, sw - 1)); // columns beyond the picture repeat the last one; they become padding
                    v0[i] = sample<FILTER>(yp, W, LX, LY, tx, ty0);
                    v1[i] = sample<FILTER>(yp, W, LX, LY, tx, ty1);
                }
                Y[0][q] = pack4(v0[0], v0[1], v0[2], v0[3]);
                Y[1][q] = pack4(v1[0], v1[1], v1[2], v1[3]);
            }
        }
        // chroma of each of the 2 x 8 pixels, minus 128: K7's upsampling of the SCALED chroma planes (swc x shc), as in k_scale.hip
        if (!BILIN) {
            const Tap ty = tap_of<FILTER>(CY, j);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const Tap tx = tap_of<FILTER>(CX, min(k + i, swc - 1));
                const int cb = static_cast<int>(sample<FILTER>(cbp, Wc, CX, CY, tx, ty)) - 128, cr = static_cast<int>(sample<FILTER>(crp, Wc, CX, CY, tx, ty)) - 128;
                U[0][2 * i] = U[0][2 * i + 1] = U[1][2 * i] = U[1][2 * i + 1] = cb;
                V[0][2 * i] = V[0][2 * i + 1] = V[1][2 * i] = V[1][2 * i + 1] = cr;
            }
        } else {
            const Tap tya = tap_of<FILTER>(CY, max(j - 1, 0)), tyb = tap_of<FILTER>(CY, j), tyc = tap_of<FILTER>(CY, min(j + 1, shc - 1));
            uint32_t a[2][5], b[2][5], c[2][5];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const Tap tx = tap_of<FILTER>(CX, min(k + i, swc - 1));
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    const uint8_t *pl = p ? crp : cbp;
                    a[p][i] = sample<FILTER>(pl, Wc, CX, CY, tx, tya);
                    b[p][i] = sample<FILTER>(pl, Wc, CX, CY, tx, tyb);
                    c[p][i] = sample<FILTER>(pl, Wc, CX, CY, tx, tyc);
                }
            }
            upsample_chroma<8>(a[0], b[0], c[0], U[0], U[1]);
            upsample_chroma<8>(a[1], b[1], c[1], V[0], V[1]);
        }
    }
    const Csc csc = csc_of(td.cset);
    const int npic = sw - x;                 // columns i < npic are picture (where the row is)
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int row = row0 + r;
        if (row < 0 || row >= oh) continue;
        uint32_t e[3][8]; // by channel position
        if (inpic && 2 * j + r < sh) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t c0, c1, c2;
                ycc_to_rgb(byte_of(Y[r][i >> 2], i & 3), U[r][i], V[r][i], csc, c0, c1, c2);
                if (P.bgr) {
                    const uint32_t s = c0;
                    c0 = c2, c2 = s;
                }
                const bool pic = i < npic;
                e[0][i] = pic ? elem_bits<DT>(c0, P.scale[0], P.bias[0]) : padbits[0];
                e[1][i] = pic ? elem_bits<DT>(c1, P.scale[1], P.bias[1]) : padbits[1];
                e[2][i] = pic ? elem_bits<DT>(c2, P.scale[2], P.bias[2]) : padbits[2];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) e[0][i] = padbits[0], e[1][i] = padbits[1], e[2][i] = padbits[2];
        }
        // (col0 may be negative: the address of column i0 is the first one formed into the canvas)
        const ptrdiff_t at = static_cast<ptrdiff_t>(row) * ow + col0;
        if (HWC) {
            uint32_t o[24];
#pragma unroll
            for (int i = 0; i < 8; i++) o[3 * i] = e[0][i], o[3 * i + 1] = e[1][i], o[3 * i + 2] = e[2][i];
            store_run<DT, 24>(out + at * (3 * ES), o, whole, 3 * i0, 3 * i1);
        } else {
            const ptrdiff_t plane = static_cast<ptrdiff_t>(ow) * oh;
#pragma unroll
            for (int p = 0; p < 3; p++) store_run<DT, 8>(out + (p * plane + at) * ES, e[p], whole, i0, i1);
        }
    }
}

template <int FILTER, bool BILIN, int DT, bool HWC> __device__ static __forceinline__ void tensor_chunk(const TensorDesc &td, const TensorParams &P, const uint8_t *src, uint8_t *out) {
    constexpr int ES = ElemSize<DT>::value;
    const int px = static_cast<int>(td.px), py = static_cast<int>(td.py);
    // groups g = -gneg .. and row pairs j = -jneg .. cover the canvas
    const int gneg = (px + 7) / 8, ngroups = gneg + (P.ow - px + 7) / 8, jneg = (py + 1) / 2, npairs = jneg + (P.oh - py + 1) / 2;
    const int jj0 = static_cast<int>(blockIdx.y) * P.pairs_per_block, items = min(P.pairs_per_block, npairs - jj0) * ngroups; // (<= 0 beyond the last pair)
    // word stores need the item, its rows and the picture's first column on the boundary of the widest store
    const uintptr_t unit = static_cast<uintptr_t>(ES) * (HWC ? 3 : 1), need = DT == DT_U8 ? 7 : 15;
    const bool aligned = ((reinterpret_cast<uintptr_t>(out) | (static_cast<uintptr_t>(P.ow) * unit) | (static_cast<uintptr_t>(px) * unit)) & need) == 0;
    uint32_t padbits[3];
#pragma unroll
    for (int p = 0; p < 3; p++) padbits[p] = elem_bits<DT>(P.pad[p], P.scale[p], P.bias[p]);
    for (int i = static_cast<int>(threadIdx.x); i < items; i += 256)
        tensor_item<FILTER, BILIN, DT, HWC>(td, P, src, out, padbits, aligned, jj0 + i / ngroups - jneg, i % ngroups - gneg);
}

template <int FILTER, int DT> __device__ static __forceinline__ void tensor_layout(const TensorDesc &td, const TensorParams &P, const uint8_t *src, uint8_t *out) {
    const bool bilin = td.bilinear != 0;
    if (P.hwc) {
        if (bilin) tensor_chunk<FILTER, true, DT, true>(td, P, src, out);
        else tensor_chunk<FILTER, false, DT, true>(td, P, src, out);
    } else {
        if (bilin) tensor_chunk<FILTER, true, DT, false>(td, P, src, out);
        else tensor_chunk<FILTER, false, DT, false>(td, P, src, out);
    }
}

// element type, layout and chroma mode of an item, for one filter
template <int FILTER> __device__ static __forceinline__ void tensor_block(const TensorDesc *descs, uint8_t *dst, const TensorParams &P) {
    const TensorDesc td = descs[blockIdx.x];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(td.src);
    uint8_t *out = dst + td.dst_off;
    switch (P.dtype) {
    case DT_U8: tensor_layout<FILTER, DT_U8>(td, P, src, out); break;
    case DT_F16: tensor_layout<FILTER, DT_F16>(td, P, src, out); break;
    case DT_BF16: tensor_layout<FILTER, DT_BF16>(td, P, src, out); break;
    case DT_F32: tensor_layout<FILTER, DT_F32>(td, P, src, out); break;
    }
}

// one entry point per filter, as for K8
extern "C" __global__ void __launch_bounds__(256, 2) k_tensor(const TensorDesc *descs, uint8_t *dst, TensorParams P) { tensor_block<0>(descs, dst, P); }
extern "C" __global__ void __launch_bounds__(256, 2) k_tensor_area(const TensorDesc *descs, uint8_t *dst, TensorParams P) { tensor_block<1>(descs, dst, P); }
