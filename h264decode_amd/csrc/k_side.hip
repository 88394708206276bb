// h264decode_amd/csrc/k_side.hip -- K11: macroblock side information of a list of frames as int16 planes per 4x4 luma block (the rule of
// include/h264mi.h, "Macroblock side information").  A streaming re-layout of the MbRec / MbMv1 records the entropy kernels left in HBM: no sample is read.
// One launch takes any number of frames: blockIdx.x = item, blockIdx.y = a chunk of `rows_per_block` macroblock rows of the macroblocks the grid touches.
// One lane per macroblock; the record arrives in 16-byte loads, and only the chunks the selected planes need (the plane mask is uniform per launch).  Per
// plane and block row a macroblock's four cells are one 8-byte store where the item allows it (SideDesc::vec, uniform per item): adjacent lanes write
// adjacent 8 bytes, a wavefront 512 contiguous bytes.  Otherwise -- a crop origin inside a macroblock, a grid width that is no multiple of four -- single
// elements, and cells outside gw x gh are never written.
#include "../../include/h264mi.h"
#include "mi_kernels.h"

// 16-byte chunks of an MbRec (mi_types.h): 0 type .. slice_in_pic | 1 ipm (inter: [0..3] ref_idx_l1) | 2 ref_idx_l0, refslot, slice_idx | 3 .. 6 mv | 7 coef_off,
// coef_mask, refslot1
#define SIDE_L0 (H264MI_SIDE_MVX0 | H264MI_SIDE_MVY0 | H264MI_SIDE_REF0 | H264MI_SIDE_DPOC0)
#define SIDE_L1 (H264MI_SIDE_MVX1 | H264MI_SIDE_MVY1 | H264MI_SIDE_REF1 | H264MI_SIDE_DPOC1)

__device__ static __forceinline__ int s16lo(uint32_t v) { return static_cast<int16_t>(v & 0xFFFFu); }
__device__ static __forceinline__ int s16hi(uint32_t v) { return static_cast<int16_t>(v >> 16); }
__device__ static __forceinline__ int s8at(uint32_t v, int k) { return static_cast<int8_t>((v >> (8 * k)) & 0xFFu); }
__device__ static __forceinline__ uint32_t pack2(int a, int b) { return (static_cast<uint32_t>(a) & 0xFFFFu) | (static_cast<uint32_t>(b) << 16); }

// the four cells v[0..3] of block row r of the macroblock whose first cell is at grid column i0 (may be negative) of grid row j
template <bool VEC> __device__ static __forceinline__ void put_row(uint8_t *plane, int gw, int j, int i0, const int v[4]) {
    int16_t *row = reinterpret_cast<int16_t *>(plane) + static_cast<size_t>(j) * gw;
    if (VEC) { // 0 <= i0, i0 + 3 < gw, the address is 8-byte aligned
        *reinterpret_cast<uint2 *>(row + i0) = uint2{pack2(v[0], v[1]), pack2(v[2], v[3])};
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (i0 + c >= 0 && i0 + c < gw) row[i0 + c] = static_cast<int16_t>(v[c]);
    }
}

// the motion planes of one list: vectors mv[4] (chunks of four blocks = one block row each), whether each quadrant uses the list, its reference index and
// the difference of picture order counts
template <bool VEC>
__device__ static __forceinline__ uint8_t *put_list(uint8_t *out, size_t pb, uint32_t sel, int gw, int gh, int j0, int i0, const uint4 mv[4], bool have_mv,
                                                    const bool use[4], const int ref[4], const int dp[4]) {
    // sel: the list's four plane bits shifted down to bits 0 .. 3 (MVX, MVY, REF, DPOC)
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (!((sel >> p) & 1)) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = j0 + r;
            if (j < 0 || j >= gh) continue;
            const int qa = (r >> 1) * 2, qb = qa + 1; // quadrants of columns 0, 1 and 2, 3
            int v[4];
            if (p < 2) {
                const uint32_t w[4] = {mv[r].x, mv[r].y, mv[r].z, mv[r].w};
#pragma unroll
                for (int c = 0; c < 4; c++) v[c] = (have_mv && use[c < 2 ? qa : qb]) ? (p == 0 ? s16lo(w[c]) : s16hi(w[c])) : 0;
            } else if (p == 2) {
                v[0] = v[1] = use[qa] ? ref[qa] : -1, v[2] = v[3] = use[qb] ? ref[qb] : -1;
            } else {
                v[0] = v[1] = use[qa] ? dp[qa] : 0, v[2] = v[3] = use[qb] ? dp[qb] : 0;
            }
            put_row<VEC>(out, gw, j, i0, v);
        }
        out += pb;
    }
    return out;
}

template <bool VEC> __device__ static __forceinline__ void side_chunk(const SideDesc &sd, uint8_t *dst, uint32_t planes, int rows_per_block) {
    const int gw = static_cast<int>(sd.gw), gh = static_cast<int>(sd.gh), bx0 = static_cast<int>(sd.bx0), by0 = static_cast<int>(sd.by0);
    const int mx0 = bx0 >> 2, my0 = by0 >> 2;
    const int nmx = min(((bx0 + gw - 1) >> 2) + 1, static_cast<int>(sd.wmb)) - mx0, nmy = min(((by0 + gh - 1) >> 2) + 1, static_cast<int>(sd.hmb)) - my0;
    const int r0 = static_cast<int>(blockIdx.y) * rows_per_block, items = min(rows_per_block, nmy - r0) * nmx; // (<= 0 beyond the last row)
    const size_t pb = static_cast<size_t>(gw) * gh * 2;
    const uint4 *recs = reinterpret_cast<const uint4 *>(sd.rec);
    const uint4 *recs1 = reinterpret_cast<const uint4 *>(sd.mv1);
    const int16_t *dpoc = reinterpret_cast<const int16_t *>(sd.dpoc);
    const bool want0 = (planes & SIDE_L0) != 0, want1 = (planes & SIDE_L1) != 0;
    for (int i = static_cast<int>(threadIdx.x); i < items; i += 256) {
        const int mby = my0 + r0 + i / nmx, mbx = mx0 + i % nmx;
        const size_t mb = static_cast<size_t>(mby) * sd.wmb + mbx;
        const uint4 *rec = recs + mb * 8;
        const int j0 = 4 * mby - by0, i0 = 4 * mbx - bx0; // the macroblock's first cell in the grid (negative: cropped away)
        uint8_t *out = dst;
        const uint4 c0 = rec[0];
        const int type = static_cast<int>(c0.x & 0xFFu);
        const bool inter = MB_IS_INTER(type);
        if (planes & (H264MI_SIDE_TYPE | H264MI_SIDE_QP | H264MI_SIDE_NZ | H264MI_SIDE_SLICE)) {
            const int qp = static_cast<int>((c0.x >> 16) & 0xFFu), nz = static_cast<int>(c0.z & 0xFFFFu);
            const int slice = type == MBT_NONE ? -1 : s16hi(c0.w); // (a concealed record carries 0xFFFF)
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (!((planes >> p) & 1)) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = j0 + r;
                    if (j < 0 || j >= gh) continue;
                    int v[4];
#pragma unroll
                    for (int c = 0; c < 4; c++) v[c] = p == 0 ? type : p == 1 ? qp : p == 2 ? ((nz >> (4 * r + c)) & 1) : slice;
                    put_row<VEC>(out, gw, j, i0, v);
                }
                out += pb;
            }
        }
        if (!want0 && !want1) continue;
        uint4 c2 = uint4{0u, 0u, 0u, 0u};
        if (want0 || (planes & H264MI_SIDE_DPOC1)) c2 = rec[2];
        // the slice's row of the table: [list][entry]; a record that names no slice of the batch (never written by the entropy kernels) reads zeros
        const bool row_ok = c2.w < sd.n_slices;
        const int16_t *drow = dpoc + static_cast<size_t>(row_ok ? c2.w : 0u) * 32;
        if (want0) {
            bool use[4];
            int ref[4], dp[4];
            const int slot[4] = {s16lo(c2.y), s16hi(c2.y), s16lo(c2.z), s16hi(c2.z)};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                use[q] = inter && slot[q] >= 0, ref[q] = s8at(c2.x, q);
                dp[q] = ((planes & H264MI_SIDE_DPOC0) && use[q] && row_ok) ? drow[ref[q] & 15] : 0;
            }
            uint4 mv[4] = {};
            const bool have_mv = (planes & (H264MI_SIDE_MVX0 | H264MI_SIDE_MVY0)) != 0;
            if (have_mv) {
#pragma unroll
                for (int r = 0; r < 4; r++) mv[r] = rec[3 + r];
            }
            out = put_list<VEC>(out, pb, (planes >> 4) & 15u, gw, gh, j0, i0, mv, have_mv, use, ref, dp);
        }
        if (want1) {
            const uint4 c1 = rec[1], c7 = rec[7];
            bool use[4];
            int ref[4], dp[4];
            const int slot[4] = {s16lo(c7.z), s16hi(c7.z), s16lo(c7.w), s16hi(c7.w)};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                use[q] = inter && slot[q] >= 0, ref[q] = s8at(c1.x, q);
                dp[q] = ((planes & H264MI_SIDE_DPOC1) && use[q] && row_ok) ? drow[16 + (ref[q] & 15)] : 0;
            }
            uint4 mv[4] = {};
            const bool have_mv = (planes & (H264MI_SIDE_MVX1 | H264MI_SIDE_MVY1)) != 0 && recs1 != nullptr;
            if (have_mv) {
#pragma unroll
                for (int r = 0; r < 4; r++) mv[r] = recs1[mb * 4 + r];
            }
            out = put_list<VEC>(out, pb, (planes >> 8) & 15u, gw, gh, j0, i0, mv, have_mv, use, ref, dp);
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) k_side(const SideDesc *descs, uint8_t *dst, uint32_t planes, int rows_per_block) {
    const SideDesc sd = descs[blockIdx.x];
    if (sd.vec) side_chunk<true>(sd, dst + sd.dst_off, planes, rows_per_block);
    else side_chunk<false>(sd, dst + sd.dst_off, planes, rows_per_block);
}
