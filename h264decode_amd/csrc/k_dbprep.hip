// h264decode_amd/csrc/k_dbprep.hip -- k_dbprep, k_dbprep_ip: boundary strengths (8.7.2.1) and alpha / beta / tC0 (8.7.2.2) of every macroblock of a batch, gfx950.
//
// Neither depends on samples, so they are worked out here for all macroblocks at once, fully parallel, and left as an 80-byte DbPrm per
// macroblock; the deblocking kernels (k_deblock.hip, k_deblock_x.hip) -- a serial dependency chain per picture -- only pick their bytes out of
// it.  (Pictures with B slices differ in the strengths only, so they need no deblocking kernel of their own.)  The same pass leaves K3's work
// list (one bit per intra macroblock) and the ColRec arrays later B pictures take their direct prediction from.
// k_dbprep handles every picture, 16 lanes per macroblock; k_dbprep_ip (below) the launches of I / P pictures that leave no ColRec array, one lane per
// macroblock.  Both write the same bytes; mi_dbprep_kernel_choice (mi_kernels.h) picks one per launch.
// Absent from the reference (only the slice-header fields are parsed: h264/slice.go:1021-1027).
#include <hip/hip_runtime.h>
#include "mi_kernels.h"
#include "k_common.h" // WAVE_SYNC, v4u, xcd_pic_block

// 8.7.2.1 with one list (I / P pictures)
// (strong: the bS of an intra macroblock edge -- 4, but 3 on the horizontal macroblock edges of a field picture; vlim: the vertical vector
// difference that counts as "far" -- 4 quarter frame samples = 2 quarter field samples in a field picture)
__device__ __forceinline__ int prep_bs(const MbRec *mp, int pb, const MbRec *mq, int qb, int strong, int vlim) {
    // branch-free: every operand is fetched up front (independent LDS reads), the decision is a chain of selects
    const int q8p = ((pb >> 3) << 1) | ((pb & 3) >> 1), q8q = ((qb >> 3) << 1) | ((qb & 3) >> 1);
    const int tp = mp->type, tq = mq->type, nzp = mp->nzmask, nzq = mq->nzmask, rp = mp->refslot[q8p], rq = mq->refslot[q8q];
    const int vpx = mp->mv[pb][0], vpy = mp->mv[pb][1], vqx = mq->mv[qb][0], vqy = mq->mv[qb][1];
    const bool far = rp != rq || abs(vpx - vqx) >= 4 || abs(vpy - vqy) >= vlim;
    return (MB_IS_INTRA(tp) || MB_IS_INTRA(tq)) ? strong : ((((nzp >> pb) | (nzq >> qb)) & 1) ? 2 : (far ? 1 : 0));
}
// 8.7.2.1 with two lists (pictures with B slices): the blocks differ if they use different reference PICTURES (frame slots; the
// list a picture comes from does not matter) or a different number of vectors, or if the vectors that belong together differ by >= 4
__device__ __forceinline__ bool mv_far(const int16_t *a, const int16_t *b, int vlim) { return abs(a[0] - b[0]) >= 4 || abs(a[1] - b[1]) >= vlim; }
__device__ __forceinline__ int prep_bs_b(const MbRec *mp, const MbMv1 *vp, int pb, const MbRec *mq, const MbMv1 *vq, int qb, int strong, int vlim) {
    if (MB_IS_INTRA(mp->type) || MB_IS_INTRA(mq->type)) return strong;
    if (((mp->nzmask >> pb) & 1) || ((mq->nzmask >> qb) & 1)) return 2;
    const int p8 = ((pb >> 3) << 1) | ((pb & 3) >> 1), q8 = ((qb >> 3) << 1) | ((qb & 3) >> 1);
    const int p0 = mp->refslot[p8], p1 = mp->refslot1[p8], q0 = mq->refslot[q8], q1 = mq->refslot1[q8];
    const int np = (p0 >= 0) + (p1 >= 0), nq = (q0 >= 0) + (q1 >= 0);
    if (np != nq) return 1;
    const int16_t *pv0 = mp->mv[pb], *pv1 = vp->mv[pb], *qv0 = mq->mv[qb], *qv1 = vq->mv[qb];
    if (np < 2) { // one vector each (or none: corrupt records)
        const int rp = p0 >= 0 ? p0 : p1, rq = q0 >= 0 ? q0 : q1;
        if (rp != rq) return 1;
        return mv_far(p0 >= 0 ? pv0 : pv1, q0 >= 0 ? qv0 : qv1, vlim) ? 1 : 0;
    }
    if (!((p0 == q0 && p1 == q1) || (p0 == q1 && p1 == q0))) return 1;
    if (p0 != p1) // two different pictures: each vector against the one that points to the same picture
        return (p0 == q0 ? (mv_far(pv0, qv0, vlim) || mv_far(pv1, qv1, vlim)) : (mv_far(pv0, qv1, vlim) || mv_far(pv1, qv0, vlim))) ? 1 : 0;
    return ((mv_far(pv0, qv0, vlim) || mv_far(pv1, qv1, vlim)) && (mv_far(pv0, qv1, vlim) || mv_far(pv1, qv0, vlim))) ? 1 : 0; // both vectors into one picture
}

struct PrepSub {
    MbRec rec[3]; // current, left, upper macroblock
    MbMv1 mv1[3]; // their list-1 vectors (pictures with B slices)
    DbPrm out;
    ColRec col;   // what later B pictures need of this macroblock's motion (pictures flagged save_col)
};
// grid = (ceil(macroblocks of the largest picture / MI_DBPREP_MBS), pictures), block = 256: a wavefront works on 4 macroblocks at a
// time, 16 lanes each -- lane li computes the strength of segment li & 3 of vertical edge li >> 2 and of horizontal edge li >> 2
// (the same division of labour K5 had when it did this itself), lanes 0..8 the parameters of (plane, edge kind) li / 3, li % 3.
// The same pass leaves the ColRec array of the pictures a later B picture (or batch) may take as co-located picture
// (8.4.1.2.1: per 4x4 block the vector of the list the block uses -- list 0 if it uses it, otherwise list 1 --, per 8x8 the
// reference index and the frame slot of the picture it points to; -1: intra): the records are staged here anyway.
// (Measured in round 4: issuing the loads of the wavefront's next step before working on the current one -- 7.8 -> 9.3 ms per 7680 pictures; twice the
// macroblocks per workgroup on top of that -- 8.9 ms.  A million short workgroups hide the dependent loads better than a loop carrying 12 registers.)
// col_only: the one-off back-fill of ColRec arrays for a batch whose DbPrm records are already in use (mi_api.cpp: ensure_b_buffers).
extern "C" __global__ void __launch_bounds__(256) k_dbprep(const uint32_t *pic_list, const PicDesc *pics, const DevTables *tab, const MbRec *mbrec, const MbMv1 *mbmv1,
                                                           DbPrm *out, int col_only, unsigned long long *intramask, int n_pics) {
    __shared__ PrepSub subs[4][4];
    __shared__ uint8_t s_alpha[52], s_beta[52], s_tc0[52][4];
    const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, sub = lane >> 4, li = lane & 15;
    uint32_t pic, blk; // XCD-aware order: the row above comes out of the L2 that fetched it a moment ago
    xcd_pic_block(pic, blk);
    if (pic >= static_cast<uint32_t>(n_pics)) return;
    const PicDesc *pd = &pics[pic_list[pic]];
    const int wmb = static_cast<int>(pd->wmb), nmb = wmb * static_cast<int>(pd->hmb);
    const int mb_first = static_cast<int>(blk) * MI_DBPREP_MBS;
    if (mb_first >= nmb) return;
    for (int i = tid; i < 52; i += 256) {
        s_alpha[i] = tab->alpha[i], s_beta[i] = tab->beta[i];
        s_tc0[i][0] = 0, s_tc0[i][1] = tab->tc0[i][1], s_tc0[i][2] = tab->tc0[i][2], s_tc0[i][3] = tab->tc0[i][3];
    }
    __syncthreads();
    const bool two = pd->has_b != 0;
    const MbRec *recs = mbrec + pd->mb_base;
    const MbMv1 *recs1 = two ? mbmv1 + pd->mb_base : nullptr;
    DbPrm *outs = out + pd->mb_base;
    PrepSub *ss = &subs[wave][sub];
    for (int it = wave; it < MI_DBPREP_MBS / 4; it += 4) {
        const int mb = mb_first + it * 4 + sub;
        const bool valid = mb < nmb;
        const int mby = static_cast<int>(MI_MB_ROW(static_cast<uint32_t>(valid ? mb : 0), pd->inv_wmb)), mbx = (valid ? mb : 0) - mby * wmb;
        const bool has_left = valid && mbx > 0, has_top = valid && mby > 0;
        if (valid) { // lanes 0-7: the record, lanes 8-15: the record above; then lanes 0-7: the record to the left
            const v4u z = v4u{0u, 0u, 0u, 0u};
            const bool up = li >= 8;
            v4u a = z, b = z;
            if (!up || has_top) a = reinterpret_cast<const v4u *>(recs + (up ? mb - wmb : mb))[li & 7];
            if (!up && has_left) b = reinterpret_cast<const v4u *>(recs + mb - 1)[li];
            reinterpret_cast<v4u *>(&ss->rec[up ? 2 : 0])[li & 7] = a;
            if (!up) reinterpret_cast<v4u *>(&ss->rec[1])[li] = b;
            if (two) { // list-1 vectors: lanes 0-3 current, 4-7 left, 8-11 above
                const int which = li >> 2;
                if (which < 3) {
                    const bool ok = which == 0 || (which == 1 ? has_left : has_top);
                    reinterpret_cast<v4u *>(&ss->mv1[which == 0 ? 0 : (which == 1 ? 1 : 2)])[li & 3] =
                        ok ? reinterpret_cast<const v4u *>(recs1 + (which == 0 ? mb : (which == 1 ? mb - 1 : mb - wmb)))[li & 3] : z;
                }
            }
        }
        WAVE_SYNC();
        // K3's work list: one bit per macroblock of the batch (index = position in the record array), set for intra macroblocks and for
        // macroblocks no slice delivered -- K3 reads 1 KB per 1080p picture instead of one type byte out of every 128-byte record
        if (valid && !col_only && li == 0 && (MB_IS_INTRA(ss->rec[0].type) || ss->rec[0].type == MBT_NONE)) {
            const unsigned long long gmb = pd->mb_base + static_cast<unsigned long long>(mb);
            atomicOr(&intramask[gmb >> 6], 1ull << (gmb & 63));
        }
        if (valid) {
            const MbRec *mq = &ss->rec[0], *ml = has_left ? &ss->rec[1] : nullptr, *mt = has_top ? &ss->rec[2] : nullptr;
            const int dbf = mq->dbf_idc;
            if (dbf == 2) { // no filtering across slice boundaries
                if (ml && ml->slice_in_pic != mq->slice_in_pic) ml = nullptr;
                if (mt && mt->slice_in_pic != mq->slice_in_pic) mt = nullptr;
            }
            const int e = li >> 2, k = li & 3;
            const bool mb_edge = e == 0;
            const int qb0 = k * 4 + e, qb1 = li; // q block of the vertical / horizontal edge segment
            const int pb0 = mb_edge ? k * 4 + 3 : qb0 - 1, pb1 = mb_edge ? 12 + k : qb1 - 4;
            const bool ok = dbf != 1 && !((e & 1) && mq->t8x8);
            const bool ok0 = ok && !(mb_edge && !ml), ok1 = ok && !(mb_edge && !mt);
            const MbRec *mp0 = mb_edge && ml ? ml : mq, *mp1 = mb_edge && mt ? mt : mq; // (no neighbour: any record, the result is masked)
            int bs0, bs1;
            // 8.7.2.1 in a field picture: bS 4 needs a VERTICAL macroblock edge (horizontal ones get 3), and vectors differ from a
            // vertical distance of 4 quarter FRAME samples on = 2 quarter field samples
            const bool fieldpic = pd->field != 0;
            const int vlim = fieldpic ? 2 : 4, strong0 = mb_edge ? 4 : 3, strong1 = mb_edge && !fieldpic ? 4 : 3;
            if (two) {
                bs0 = prep_bs_b(mp0, mb_edge && ml ? &ss->mv1[1] : &ss->mv1[0], pb0, mq, &ss->mv1[0], qb0, strong0, vlim);
                bs1 = prep_bs_b(mp1, mb_edge && mt ? &ss->mv1[2] : &ss->mv1[0], pb1, mq, &ss->mv1[0], qb1, strong1, vlim);
            } else
                bs0 = prep_bs(mp0, pb0, mq, qb0, strong0, vlim), bs1 = prep_bs(mp1, pb1, mq, qb1, strong1, vlim);
            ss->out.bs[k][0][e] = static_cast<uint8_t>(ok0 ? bs0 : 0);
            ss->out.bs[k][1][e] = static_cast<uint8_t>(ok1 ? bs1 : 0);
            if (li < 9) { // 8.7.2.2: (plane, edge kind): qPav of the left / no / the upper neighbour, indexA / indexB, the table rows
                const int plane = li / 3, kind = li - plane * 3;
                const MbRec *mn = kind == 0 ? ml : (kind == 2 ? mt : nullptr);
                const int qpq = plane == 0 ? mq->qp : mq->qpc[plane - 1];
                const int qpn = mn ? (plane == 0 ? mn->qp : mn->qpc[plane - 1]) : qpq;
                const int qpav = (qpn + qpq + 1) >> 1;
                const int ia = min(max(qpav + mq->alpha_off, 0), 51), ib = min(max(qpav + mq->beta_off, 0), 51);
                ss->out.pl[plane].ab[2 * kind] = s_alpha[ia], ss->out.pl[plane].ab[2 * kind + 1] = s_beta[ib];
                ss->out.pl[plane].tc[kind][0] = s_tc0[ia][1], ss->out.pl[plane].tc[kind][1] = s_tc0[ia][2], ss->out.pl[plane].tc[kind][2] = s_tc0[ia][3];
                if (kind == 0) ss->out.pl[plane].pad = 0;
            }
            if (pd->save_col) { // lane li: block li's vector; lanes 0..3 also the reference of 8x8 quadrant li
                const bool inter = MB_IS_INTER(mq->type);
                const int q = ((li >> 3) << 1) | ((li & 3) >> 1);
                const bool l0 = inter && mq->ref[q] >= 0, l1 = inter && !l0 && two && mq->refslot1[q] >= 0;
                ss->col.mv[li][0] = l0 ? mq->mv[li][0] : (l1 ? ss->mv1[0].mv[li][0] : static_cast<int16_t>(0));
                ss->col.mv[li][1] = l0 ? mq->mv[li][1] : (l1 ? ss->mv1[0].mv[li][1] : static_cast<int16_t>(0));
                if (li < 4) {
                    const bool q0 = inter && mq->ref[li] >= 0, q1 = inter && !q0 && two && mq->refslot1[li] >= 0;
                    ss->col.refslot[li] = q0 ? mq->refslot[li] : (q1 ? mq->refslot1[li] : static_cast<int16_t>(-1));
                    ss->col.ref[li] = q0 ? mq->ref[li] : (q1 ? MBREC_REF1(mq)[li] : static_cast<int8_t>(-1));
                    ss->col.pad[li] = 0;
                }
            }
        }
        WAVE_SYNC();
        if (valid && !col_only && li < 5) reinterpret_cast<v4u *>(outs + mb)[li] = reinterpret_cast<const v4u *>(&ss->out)[li];
        if (valid && pd->save_col && li < 5) reinterpret_cast<v4u *>(reinterpret_cast<ColRec *>(pd->col_out) + mb)[li] = reinterpret_cast<const v4u *>(&ss->col)[li];
        WAVE_SYNC();
    }
}

// ---- k_dbprep_ip: the same DbPrm records and intra-mask bits for launches whose pictures have ONE reference list and leave no ColRec array ----
// (mi_dbprep_kernel_choice; I / P pictures without save_col -- every picture of a stream without B slices).  A LANE owns a macroblock and a WAVEFRONT a
// strip of the picture, 64 macroblock columns wide and `rows` macroblock rows high, which it walks downwards: an iteration is 64 consecutive macroblocks
// of one row, worked out with every instruction for 64 macroblocks, not 4, by a sixteenth of k_dbprep's wavefronts or fewer.
//   loads:   the 64 records are 8 KB in a row: eight 16-byte loads per lane, handed to the lanes through LDS with a record stride of 33 dwords (odd: the
//            dword reads of 64 lanes at the same field fall on different banks).  Slot 0 holds the record in front of the first one, so the left
//            neighbour of lane l is slot l and its own record slot l + 1.  The upper neighbour is the lane's own macroblock of the iteration before,
//            kept in 9 registers -- no record is fetched a second time as somebody's upper neighbour; only a strip's first row loads those 40 bytes.
//   bS:      per direction a 16-bit mask of "coefficients" (shifts and ORs of the nzmasks) and one of "far" (refslot per 8x8; vectors by packed
//            16-bit saturating subtract / max / subtract) with bit 4 * segment + edge; a nibble spread to four bytes is a dword of DbPrm::bs.
//   stores:  the 64 DbPrms are staged in LDS (16-byte writes at stride 80 are conflict-free) and leave as one contiguous 5120-byte block.
//   mask:    one ballot per iteration, ORed into the one or two words of the batch's bit mask the 64 macroblocks span.
#define IP_STRIDE 33                      /* dwords per staged record */
#define IP_WAVE_DWORDS (65 * IP_STRIDE + 3) /* 8592 bytes; the DbPrm stage (1280 dwords) reuses the front of it */
typedef uint16_t ip_us2 __attribute__((ext_vector_type(2)));
typedef int16_t ip_s2 __attribute__((ext_vector_type(2)));
// two vectors (x | y << 16) differ by >= 4 horizontally or >= vlim vertically; limm1 = 3 | (vlim - 1) << 16
__host__ __device__ __forceinline__ bool ip_mv_far(uint32_t a, uint32_t b, ip_us2 limm1) {
    const ip_s2 va = __builtin_bit_cast(ip_s2, a), vb = __builtin_bit_cast(ip_s2, b);
    // min(|a - b|, 32767) per component: the subtraction saturates, so vectors anywhere in the 16-bit range compare as their true difference does
    const ip_s2 m = __builtin_elementwise_max(__builtin_elementwise_sub_sat(va, vb), __builtin_elementwise_sub_sat(vb, va));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(ip_us2, m), limm1)) != 0u;
}
// bit i of a nibble -> byte i of a dword (0 / 1)
__host__ __device__ __forceinline__ uint32_t ip_spread(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }
// What a lane holds of its macroblock and the two neighbours, as the dwords of their MbRecs: h = dwords 0..3 (type, t8x8, qp, qpc | .. | nzmask, avail,
// dbf_idc | alpha_off, beta_off, slice_in_pic), r01 / r23 = dwords 9 / 10 (refslot), mv = dwords 12..27.  A neighbour outside the picture: anything
struct IpLane {
    uint32_t h[4], r01, r23, mv[16];   // the macroblock
    uint32_t l[4], lr01, lr23, lmv[4]; // the left neighbour; its vectors 3, 7, 11, 15
    uint32_t t[4], tr23, tmv[4];       // the upper neighbour; its vectors 12..15
    bool has_left, has_top;            // the neighbour is inside the picture
};
// The DbPrm of a macroblock as 20 dwords.  at / bt: alpha | tC0 for bS 1..3 << 8 by indexA; beta by indexB.  (Host code too:
// tools/dbprep_lane_check.hip checks the arithmetic against k_dbprep's rules without a device.)
__host__ __device__ __forceinline__ void ip_dbprm(const IpLane &in, bool fieldpic, const uint32_t *at_tab, const uint32_t *bt_tab, uint32_t o[20]) {
    const uint32_t h0 = in.h[0], h1 = in.h[1], h2 = in.h[2], h3 = in.h[3], l0 = in.l[0], l1 = in.l[1], t0 = in.t[0], t1 = in.t[1];
    const uint32_t type = h0 & 0xFFu, t8x8 = (h0 >> 8) & 0xFFu, nz = h2 & 0xFFFFu, dbf = h2 >> 24, slice = h3 >> 16;
    const int aoff = static_cast<int8_t>(h3 & 0xFFu), boff = static_cast<int8_t>((h3 >> 8) & 0xFFu);
    const uint32_t strong_t = fieldpic ? 3u : 4u; // bS of an intra macroblock's upper edge
    const ip_us2 limm1 = ip_us2{static_cast<uint16_t>(3), static_cast<uint16_t>(fieldpic ? 1 : 3)};
    // the neighbours that count: inside the picture and, with dbf_idc 2, of the same slice
    const bool use_l = in.has_left && !(dbf == 2u && (in.l[3] >> 16) != slice), use_t = in.has_top && !(dbf == 2u && (in.t[3] >> 16) != slice);
    const bool intra_q = type - 1u <= 3u, intra_l = (l0 & 0xFFu) - 1u <= 3u, intra_t = (t0 & 0xFFu) - 1u <= 3u;
    const bool ok = dbf != 1u, ok_odd = ok && !t8x8; // edges 1 and 3 are not transform edges of an 8x8-transform macroblock
    const uint32_t okm = (ok ? 0x00FF0000u : 0u) | (ok_odd ? 0xFF00FF00u : 0u);
    const uint32_t okm_v = okm | (ok && use_l ? 0xFFu : 0u), okm_h = okm | (ok && use_t ? 0xFFu : 0u);
    // intra: 3 on the inner edges, 4 on the macroblock edges (3 on the horizontal ones of a field picture)
    const uint32_t ovm_v = intra_q ? 0xFFFFFFFFu : (intra_l ? 0xFFu : 0u), ovv_v = intra_q ? 0x03030304u : (intra_l ? 4u : 0u);
    const uint32_t ovm_h = intra_q ? 0xFFFFFFFFu : (intra_t ? 0xFFu : 0u), ovv_h = intra_q ? (0x03030300u | strong_t) : (intra_t ? strong_t : 0u);
    // "coefficients", bit 4 * segment + edge: vertical edges straight from the raster masks, horizontal ones from the transposed mask
    uint32_t nzt = nz, tt;
    tt = (nzt ^ (nzt >> 3)) & 0x0A0Au, nzt ^= tt ^ (tt << 3);
    tt = (nzt ^ (nzt >> 6)) & 0x00CCu, nzt ^= tt ^ (tt << 6);
    const uint32_t cv = nz | ((nz << 1) & 0xEEEEu) | (((in.l[2] & 0xFFFFu) >> 3) & 0x1111u);
    const uint32_t tn = in.t[2] >> 12; // bits 0..3: blocks 12..15 of the upper neighbour -> bits 0, 4, 8, 12
    const uint32_t ch = nzt | ((nzt << 1) & 0xEEEEu) | (tn & 1u) | ((tn & 2u) << 3) | ((tn & 4u) << 6) | ((tn & 8u) << 9);
    // "far": another reference picture (per 8x8: only edges 0 and 2 separate two of them) or vectors apart
    const uint32_t r0 = in.r01 & 0xFFFFu, r1 = in.r01 >> 16, r2 = in.r23 & 0xFFFFu, r3 = in.r23 >> 16;
    uint32_t fv = (r0 != r1 ? 0x0044u : 0u) | (r2 != r3 ? 0x4400u : 0u) | ((in.lr01 >> 16) != r0 ? 0x0011u : 0u) | ((in.lr23 >> 16) != r2 ? 0x1100u : 0u);
    uint32_t fh = (r0 != r2 ? 0x0044u : 0u) | (r1 != r3 ? 0x4400u : 0u) | ((in.tr23 & 0xFFFFu) != r0 ? 0x0011u : 0u) | ((in.tr23 >> 16) != r1 ? 0x1100u : 0u);
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            fv |= ip_mv_far(e ? in.mv[k * 4 + e - 1] : in.lmv[k], in.mv[k * 4 + e], limm1) ? 1u << (k * 4 + e) : 0u;
            fh |= ip_mv_far(e ? in.mv[e * 4 + k - 4] : in.tmv[k], in.mv[e * 4 + k], limm1) ? 1u << (k * 4 + e) : 0u;
        }
    fv |= cv, fh |= ch;
#pragma unroll
    for (int k = 0; k < 4; k++) { // coefficients 2, far 1, else 0; then the intra rule; then the edges that are not filtered at all
        const uint32_t v = ip_spread((cv >> (4 * k)) & 0xFu) + ip_spread((fv >> (4 * k)) & 0xFu);
        const uint32_t h = ip_spread((ch >> (4 * k)) & 0xFu) + ip_spread((fh >> (4 * k)) & 0xFu);
        o[2 * k] = ((v & ~ovm_v) | ovv_v) & okm_v;
        o[2 * k + 1] = ((h & ~ovm_h) | ovv_h) & okm_h;
    }
    // 8.7.2.2 per plane: qPav with the left / no / the upper neighbour -> indexA, indexB -> the table rows
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const int qq = static_cast<int>(p == 0 ? (h0 >> 16) & 0xFFu : (p == 1 ? h0 >> 24 : h1 & 0xFFu));
        const int ql = use_l ? static_cast<int>(p == 0 ? (l0 >> 16) & 0xFFu : (p == 1 ? l0 >> 24 : l1 & 0xFFu)) : qq;
        const int qt = use_t ? static_cast<int>(p == 0 ? (t0 >> 16) & 0xFFu : (p == 1 ? t0 >> 24 : t1 & 0xFFu)) : qq;
        uint32_t at[3], bt[3];
#pragma unroll
        for (int kind = 0; kind < 3; kind++) {
            const int qpav = ((kind == 0 ? ql : (kind == 2 ? qt : qq)) + qq + 1) >> 1;
            const int ia = qpav + aoff, ib = qpav + boff;
            at[kind] = at_tab[ia < 0 ? 0 : (ia > 51 ? 51 : ia)], bt[kind] = bt_tab[ib < 0 ? 0 : (ib > 51 ? 51 : ib)];
        }
        o[8 + 4 * p] = (at[0] & 0xFFu) | bt[0] << 8 | (at[1] & 0xFFu) << 16 | bt[1] << 24;
        o[9 + 4 * p] = (at[2] & 0xFFu) | bt[2] << 8 | ((at[0] >> 8) & 0xFFFFu) << 16;
        o[10 + 4 * p] = (at[0] >> 24) | (at[1] & 0xFFFFFF00u);
        o[11 + 4 * p] = at[2] >> 8; // (the pad byte: 0)
    }
}
// grid = (strips per picture = ceil(wmb_max / 64) * ceil(hmb_max / rows), pictures rounded up to a multiple of 8), block = 64; rows: mi_dbprep_ip_rows()
extern "C" __global__ void __launch_bounds__(64) k_dbprep_ip(const uint32_t *pic_list, const PicDesc *pics, const DevTables *tab, const MbRec *mbrec, DbPrm *out,
                                                             unsigned long long *intramask, int n_pics, int chunks, int rows) {
    __shared__ __attribute__((aligned(16))) uint32_t st[IP_WAVE_DWORDS];
    __shared__ uint32_t s_at[52], s_b[52]; // alpha | tC0 for bS 1..3 << 8 (by indexA); beta (by indexB)
    const int lane = static_cast<int>(threadIdx.x);
    uint32_t pic, strip; // XCD-aware order: the record to the left of a strip comes out of the L2 that fetches it for the strip it belongs to
    xcd_pic_block(pic, strip);
    if (pic >= static_cast<uint32_t>(n_pics)) return;
    const PicDesc *pd = &pics[pic_list[pic]];
    const int wmb = static_cast<int>(pd->wmb), hmb = static_cast<int>(pd->hmb);
    const int col0 = static_cast<int>(strip % static_cast<uint32_t>(chunks)) * 64, row0 = static_cast<int>(strip / static_cast<uint32_t>(chunks)) * rows;
    if (col0 >= wmb || row0 >= hmb) return;
    if (lane < 52) {
        s_at[lane] = static_cast<uint32_t>(tab->alpha[lane]) | static_cast<uint32_t>(tab->tc0[lane][1]) << 8 | static_cast<uint32_t>(tab->tc0[lane][2]) << 16 |
                     static_cast<uint32_t>(tab->tc0[lane][3]) << 24;
        s_b[lane] = tab->beta[lane];
    }
    WAVE_SYNC();
    const MbRec *recs = mbrec + pd->mb_base;
    DbPrm *outs = out + pd->mb_base;
    const bool fieldpic = pd->field != 0;
    const int nvalid = min(64, wmb - col0), row_end = min(hmb, row0 + rows); // (uniform over the wavefront)
    const bool valid = lane < nvalid;
    const v4u z = v4u{0u, 0u, 0u, 0u};
    IpLane in;
    in.has_left = valid && col0 + lane > 0;
    // the strip's first row: the upper neighbour per lane (nothing above the picture's first row)
    {
        v4u th = z, tv = z;
        in.tr23 = 0;
        if (valid && row0 > 0) {
            const uint32_t *t = reinterpret_cast<const uint32_t *>(recs + ((row0 - 1) * wmb + col0 + lane));
            th = *reinterpret_cast<const v4u *>(t), in.tr23 = t[10], tv = *reinterpret_cast<const v4u *>(t + 24);
        }
        in.t[0] = th.x, in.t[1] = th.y, in.t[2] = th.z, in.t[3] = th.w;
        in.tmv[0] = tv.x, in.tmv[1] = tv.y, in.tmv[2] = tv.z, in.tmv[3] = tv.w;
    }
    for (int row = row0; row < row_end; row++) {
        const int mb0 = row * wmb + col0;
        in.has_top = valid && row > 0;
        // ---- loads: the 64 records (and the one in front of them) into LDS
        {
            const v4u *src = reinterpret_cast<const v4u *>(recs + mb0);
            v4u ld[8];
#pragma unroll
            for (int i = 0; i < 8; i++) ld[i] = i * 8 + (lane >> 3) < nvalid ? src[i * 64 + lane] : z;
            v4u lf = z;
            if (lane < 8 && col0 > 0) lf = reinterpret_cast<const v4u *>(recs + (mb0 - 1))[lane];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t *dst = st + (i * 8 + (lane >> 3) + 1) * IP_STRIDE + (lane & 7) * 4;
                dst[0] = ld[i].x, dst[1] = ld[i].y, dst[2] = ld[i].z, dst[3] = ld[i].w;
            }
            if (lane < 8) {
                uint32_t *dst = st + lane * 4;
                dst[0] = lf.x, dst[1] = lf.y, dst[2] = lf.z, dst[3] = lf.w;
            }
        }
        WAVE_SYNC();
        const uint32_t *own = st + (lane + 1) * IP_STRIDE, *lft = st + lane * IP_STRIDE;
#pragma unroll
        for (int i = 0; i < 4; i++) in.h[i] = own[i], in.l[i] = lft[i], in.lmv[i] = lft[15 + 4 * i];
        in.r01 = own[9], in.r23 = own[10], in.lr01 = lft[9], in.lr23 = lft[10];
#pragma unroll
        for (int i = 0; i < 16; i++) in.mv[i] = own[12 + i];
        WAVE_SYNC(); // the stage is free: the DbPrms go into its front
        // K3's work list: intra macroblocks and macroblocks no slice delivered
        {
            const uint32_t type = in.h[0] & 0xFFu;
            const unsigned long long bal = __ballot(valid && (MB_IS_INTRA(type) || type == MBT_NONE));
            if (lane == 0 && bal) {
                const unsigned long long gmb = pd->mb_base + static_cast<unsigned long long>(mb0);
                const int sh = static_cast<int>(gmb & 63);
                atomicOr(&intramask[gmb >> 6], bal << sh);
                if (sh && (bal >> (64 - sh))) atomicOr(&intramask[(gmb >> 6) + 1], bal >> (64 - sh));
            }
        }
        uint32_t o[20];
        ip_dbprm(in, fieldpic, s_at, s_b, o);
        v4u *stage = reinterpret_cast<v4u *>(st);
#pragma unroll
        for (int i = 0; i < 5; i++) stage[lane * 5 + i] = v4u{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
        WAVE_SYNC();
        v4u *dst = reinterpret_cast<v4u *>(outs + mb0);
#pragma unroll
        for (int i = 0; i < 5; i++)
            if (i * 64 + lane < nvalid * 5) dst[i * 64 + lane] = stage[i * 64 + lane];
        WAVE_SYNC();
        // this row is the next one's upper neighbour
#pragma unroll
        for (int i = 0; i < 4; i++) in.t[i] = in.h[i], in.tmv[i] = in.mv[12 + i];
        in.tr23 = in.r23;
    }
}
