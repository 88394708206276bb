// h264decode_amd/csrc/k_conceal.hip -- k_conceal: error concealment of lost macroblocks (h264mi_config.conceal_errors), gfx950.
//
// Runs on the entropy stream after a level's entropy launch and before that level's k_dbprep, over the pictures complete with the level
// (the list k_dbprep gets).  The LOST macroblocks of a picture are
//   (a) the macroblocks no slice delivered -- MBT_NONE records: a gap in front of a slice, the rest after an early end, a missing NAL unit --, and
//   (b) ALL macroblocks of a slice whose entropy status is non-zero, the ones it decoded before it noticed included (where a desynchronised
//       slice notices is a property of the kernel; the rule is a function of the stream).
// In a concealable picture (PicDesc::conceal_ref >= 0: a frame picture, not IDR, with a non-empty initial P list, 8.2.4.2.1) their records are
// rewritten as what a conforming decoder derives for the REPAIRED stream: the lost macroblocks coded as P slices of P_Skip macroblocks with one
// active reference and no list modification, slice_qp_delta 0, disable_deblocking_filter_idc 0, default weights.  In such a slice
//   - every P_Skip has the zero vector and refIdxL0 0 (8.4.1.1: a neighbour is unavailable, or is itself a zero-vector skip with refIdx 0) -- so
//     how the lost macroblocks are cut into slices does not matter;
//   - QP_Y is 26 + pic_init_qp_minus26 (SliceDesc::slice_qp of the picture's concealment descriptor), QP_C follows through the PPS offsets,
//     cbp 0, no residual;
//   - all edges are filtered (idc 0, offsets 0), and slice_in_pic is one no real slice has: an intact neighbour slice with idc 2 sees another slice;
//   - boundary strengths compare reference PICTURES and vectors as always: refslot = the concealment reference, refslot1 = -1, a zero MbMv1 entry
//     in pictures with B slices.
// slice_idx names the picture's concealment descriptor (slices[conceal_base + picture]: type P, wp_flag 0, identity weights), never the slice
// that failed or whose wavefront blanked a gap: K4 takes its weights from there.  Intact slices are untouched.
// Pictures that are not concealable keep their records as they are (MBT_NONE is painted mid-grey by K3, the host marks the stream).
// A FIELD picture (H264MI_CONCEAL_FIELDS) needs nothing of its own here: PicDesc::hmb is the field's, and conceal_ref carries the parity of the reference
// field the way every entry of a field list does (slot | MI_REF_PARITY) -- exactly the refslot words the entropy kernel writes for a P_Skip of a field P slice.
// A picture WITHOUT SLICES (PicDesc::n_slices 0) is a frame the host inserted for a wholly lost reference frame (H264MI_CONCEAL_PICTURES): every
// macroblock is lost, no slice status is read, nothing was written to its records before.  All of its boundary strengths come out 0 (one reference
// picture, zero vectors, no coefficients, no intra macroblock), so K5 filters nothing and the picture is an exact copy of its concealment reference.
// The same holds for a FIELD without slices, the complement the host inserts for a lone field (H264MI_CONCEAL_LONE_FIELDS): nothing of its own here
// either -- hmb is the field's, conceal_ref carries the parity, and K4 derives the chroma vector of a reference field of the other parity as for any
// field P_Skip.
//
// Cost when nothing is lost: per picture one workgroup that reads two status words and three SliceDesc words per slice and leaves
// (err == 0 && fill_from == first_mb && first_mb + n_mbs == end_mb for every slice).  Pictures with slice groups start from zeroed records and
// are walked, pictures without slices are written whole.
#include <hip/hip_runtime.h>
#include "mi_kernels.h"

typedef uint32_t cv4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void conceal_write(MbRec *rec, MbMv1 *mv1, uint32_t w0, uint32_t w1, uint32_t slots, uint32_t slice_idx) {
    cv4u *o = reinterpret_cast<cv4u *>(rec);
    const cv4u z = cv4u{0u, 0u, 0u, 0u};
    o[0] = cv4u{w0, w1, 0u, 0xFFFF0000u};       // type / t8x8 / qp / qpc | cbp .. i16mode | nzmask, avail, dbf_idc 0 | offsets 0, slice_in_pic 0xFFFF
    o[1] = z;                                   // ipm: ref_idx_l1 / mb_type as coded / sub_mb_type all 0, as a P_Skip record of the entropy kernel
    o[2] = cv4u{0u, slots, slots, slice_idx};   // ref_idx_l0 0 | refslot[4] | slice_idx
    o[3] = z, o[4] = z, o[5] = z, o[6] = z;     // the zero vector
    o[7] = cv4u{0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu}; // no coefficient blocks | refslot1 -1
    if (mv1) {
        cv4u *v = reinterpret_cast<cv4u *>(mv1);
        v[0] = z, v[1] = z, v[2] = z, v[3] = z;
    }
}

// grid = pictures of the list, block = 256.  cmap: [picture] -> where in cmap the (sorted) slice indices of the picture start (PicDesc::n_slices of
// them).  cstat: per picture of the batch the number of concealed macroblocks; every picture's word is written.
extern "C" __global__ void __launch_bounds__(256) k_conceal(const uint32_t *pic_list, const PicDesc *pics, const SliceDesc *slices, const uint32_t *cmap, uint32_t conceal_base,
                                                            const uint32_t *status, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, MbMv1 *mbmv1, uint32_t *cstat) {
    __shared__ uint32_t s_mbs;
    const int tid = static_cast<int>(threadIdx.x);
    const uint32_t pic = pic_list[blockIdx.x];
    const PicDesc *pd = &pics[pic];
    const int ref = pd->conceal_ref;
    const int nsl = static_cast<int>(pd->n_slices);
    const uint32_t *sl = cmap + cmap[pic];
    const bool fmo = pd->fmo != 0;
    int todo = 0;
    if (ref >= 0) {
        todo = fmo || nsl == 0 ? 1 : 0;
        for (int i = tid; i < nsl; i += 256) {
            const uint32_t s = sl[i];
            const SliceDesc *sd = &slices[s];
            if (status[8 * s] || sd->fill_from != sd->first_mb || sd->first_mb + status[8 * s + 1] != sd->end_mb) todo = 1;
        }
    }
    if (tid == 0) s_mbs = 0;
    if (!__syncthreads_or(todo)) {
        if (tid == 0) cstat[pic] = 0;
        return;
    }
    const int total = static_cast<int>(pd->wmb * pd->hmb);
    MbRec *recs = mbrec + pd->mb_base;
    MbMv1 *recs1 = pd->has_b && mbmv1 ? mbmv1 + pd->mb_base : nullptr;
    const SliceDesc *cd = &slices[conceal_base + pic];
    const int qp = cd->slice_qp;
    const uint32_t qc0 = tab->qpc[min(max(qp + pd->cqp_off[0], 0), 51)], qc1 = tab->qpc[min(max(qp + pd->cqp_off[1], 0), 51)];
    const uint32_t w0 = static_cast<uint32_t>(MBT_PSKIP) | static_cast<uint32_t>(qp) << 16 | qc0 << 24, w1 = qc1;
    const uint32_t slot = static_cast<uint16_t>(ref), slots = slot | slot << 16, cidx = conceal_base + pic;
    const uint8_t *sgmap = bitstream + pd->sgmap_off;
    uint32_t mine = 0;
    for (int i = 0; i < nsl; i++) {
        const uint32_t s = sl[i];
        const SliceDesc *sd = &slices[s];
        const uint32_t err = status[8 * s], n = status[8 * s + 1];
        const int first = static_cast<int>(sd->first_mb), from = static_cast<int>(sd->fill_from), end = min(static_cast<int>(sd->end_mb), total);
        if (err) { // (b): the slice's whole range (and the gap in front of it, which is (a))
            if (fmo) {
                if (first < total) {
                    const int grp = sgmap[first];
                    for (int mb = first + tid; mb < end; mb += 256)
                        if (sgmap[mb] == grp) conceal_write(recs + mb, recs1 ? recs1 + mb : nullptr, w0, w1, slots, cidx), mine++;
                }
            } else
                for (int mb = from + tid; mb < end; mb += 256) conceal_write(recs + mb, recs1 ? recs1 + mb : nullptr, w0, w1, slots, cidx), mine++;
        } else if (!fmo && (from != first || first + static_cast<int>(n) != end)) { // (a): what the wavefront blanked in its range
            for (int mb = from + tid; mb < end; mb += 256)
                if (recs[mb].type == MBT_NONE) conceal_write(recs + mb, recs1 ? recs1 + mb : nullptr, w0, w1, slots, cidx), mine++;
        }
    }
    if (nsl == 0) { // an inserted picture: all of it
        for (int mb = tid; mb < total; mb += 256) conceal_write(recs + mb, recs1 ? recs1 + mb : nullptr, w0, w1, slots, cidx), mine++;
    } else if (fmo) { // (a) with slice groups: whatever is still as the memset before the entropy launch left it
        __syncthreads();
        for (int mb = tid; mb < total; mb += 256)
            if (recs[mb].type == MBT_NONE) conceal_write(recs + mb, recs1 ? recs1 + mb : nullptr, w0, w1, slots, cidx), mine++;
    }
    if (mine) atomicAdd(&s_mbs, mine);
    __syncthreads();
    if (tid == 0) cstat[pic] = s_mbs;
}
