// tools/dbprep_lane_check.hip -- the per-lane arithmetic of k_dbprep_ip (ip_dbprm, k_dbprep.hip) against the rules of k_dbprep, on the HOST: no device needed.
// Random macroblock records -- plausible ones, near-identical neighbours (the 0 / 1 decisions), vectors over the whole 16-bit range, and plain garbage --
// with and without neighbours, frame and field pictures; every one of the 80 bytes of the DbPrm must agree.
// Build and run (tests/test_dbprep_lane_arith.py does):  hipcc -O2 -std=c++17 --offload-arch=gfx950 -I h264decode_amd/csrc -x hip tools/dbprep_lane_check.hip -o check && ./check [cases]
#include "k_dbprep.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint8_t alpha[52], beta[52], tc0[52][4];
// k_dbprep's prep_bs and its parameter code, lane by lane (li), written to `out`
static int ref_bs(const MbRec *mp, int pb, const MbRec *mq, int qb, int strong, int vlim) {
    const int q8p = ((pb >> 3) << 1) | ((pb & 3) >> 1), q8q = ((qb >> 3) << 1) | ((qb & 3) >> 1);
    const int tp = mp->type, tq = mq->type, nzp = mp->nzmask, nzq = mq->nzmask, rp = mp->refslot[q8p], rq = mq->refslot[q8q];
    const int vpx = mp->mv[pb][0], vpy = mp->mv[pb][1], vqx = mq->mv[qb][0], vqy = mq->mv[qb][1];
    const bool far = rp != rq || abs(vpx - vqx) >= 4 || abs(vpy - vqy) >= vlim;
    return (MB_IS_INTRA(tp) || MB_IS_INTRA(tq)) ? strong : ((((nzp >> pb) | (nzq >> qb)) & 1) ? 2 : (far ? 1 : 0));
}
static void ref_prm(const MbRec *mq, const MbRec *ml, const MbRec *mt, bool fieldpic, DbPrm *out) {
    memset(out, 0xEE, sizeof(*out));
    const int dbf = mq->dbf_idc;
    if (dbf == 2) {
        if (ml && ml->slice_in_pic != mq->slice_in_pic) ml = nullptr;
        if (mt && mt->slice_in_pic != mq->slice_in_pic) mt = nullptr;
    }
    for (int li = 0; li < 16; li++) {
        const int e = li >> 2, k = li & 3;
        const bool mb_edge = e == 0;
        const int qb0 = k * 4 + e, qb1 = li;
        const int pb0 = mb_edge ? k * 4 + 3 : qb0 - 1, pb1 = mb_edge ? 12 + k : qb1 - 4;
        const bool ok = dbf != 1 && !((e & 1) && mq->t8x8);
        const bool ok0 = ok && !(mb_edge && !ml), ok1 = ok && !(mb_edge && !mt);
        const MbRec *mp0 = mb_edge && ml ? ml : mq, *mp1 = mb_edge && mt ? mt : mq;
        const int vlim = fieldpic ? 2 : 4, strong0 = mb_edge ? 4 : 3, strong1 = mb_edge && !fieldpic ? 4 : 3;
        const int bs0 = ref_bs(mp0, pb0, mq, qb0, strong0, vlim), bs1 = ref_bs(mp1, pb1, mq, qb1, strong1, vlim);
        out->bs[k][0][e] = static_cast<uint8_t>(ok0 ? bs0 : 0), out->bs[k][1][e] = static_cast<uint8_t>(ok1 ? bs1 : 0);
        if (li < 9) {
            const int plane = li / 3, kind = li - plane * 3;
            const MbRec *mn = kind == 0 ? ml : (kind == 2 ? mt : nullptr);
            const int qpq = plane == 0 ? mq->qp : mq->qpc[plane - 1];
            const int qpn = mn ? (plane == 0 ? mn->qp : mn->qpc[plane - 1]) : qpq;
            const int qpav = (qpn + qpq + 1) >> 1;
            int ia = qpav + mq->alpha_off, ib = qpav + mq->beta_off;
            ia = ia < 0 ? 0 : (ia > 51 ? 51 : ia), ib = ib < 0 ? 0 : (ib > 51 ? 51 : ib);
            out->pl[plane].ab[2 * kind] = alpha[ia], out->pl[plane].ab[2 * kind + 1] = beta[ib];
            out->pl[plane].tc[kind][0] = tc0[ia][1], out->pl[plane].tc[kind][1] = tc0[ia][2], out->pl[plane].tc[kind][2] = tc0[ia][3];
            if (kind == 0) out->pl[plane].pad = 0;
        }
    }
}

static uint32_t rs = 12345;
static uint32_t rnd() { return (rs = rs * 1664525u + 1013904223u) >> 8; }
static int16_t rnd16() { return static_cast<int16_t>(rnd() & 0xFFFFu); }
// mode 0: one reference, vectors close together; 1: several references; 2: vectors anywhere in the 16-bit range; 3: every byte random
static void rnd_rec(MbRec *r, int mode) {
    for (size_t i = 0; i < sizeof(*r); i++) reinterpret_cast<uint8_t *>(r)[i] = static_cast<uint8_t>(rnd());
    if (mode == 3) return;
    r->type = rnd() % 13, r->t8x8 = rnd() & 1, r->qp = rnd() % 52, r->qpc[0] = rnd() % 52, r->qpc[1] = rnd() % 52;
    r->dbf_idc = rnd() % 3, r->slice_in_pic = rnd() % 3, r->nzmask = static_cast<uint16_t>((rnd() & 1) ? rnd() : (rnd() & rnd() & rnd()));
    r->alpha_off = static_cast<int8_t>(static_cast<int>(rnd() % 13) - 6), r->beta_off = static_cast<int8_t>(static_cast<int>(rnd() % 13) - 6);
    for (int i = 0; i < 4; i++) r->refslot[i] = static_cast<int16_t>(mode == 0 ? 2 : static_cast<int>(rnd() % 3) - 1);
    const int bx = rnd16() / 64, by = rnd16() / 64;
    for (int i = 0; i < 16; i++) {
        r->mv[i][0] = mode == 2 ? rnd16() : static_cast<int16_t>(bx + static_cast<int>(rnd() % 8) - 4);
        r->mv[i][1] = mode == 2 ? rnd16() : static_cast<int16_t>(by + static_cast<int>(rnd() % 8) - 4);
    }
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 400000;
    uint32_t at[52], bt[52];
    for (int i = 0; i < 52; i++) {
        alpha[i] = static_cast<uint8_t>(rnd()), beta[i] = static_cast<uint8_t>(rnd());
        for (int j = 0; j < 4; j++) tc0[i][j] = static_cast<uint8_t>(rnd());
        at[i] = alpha[i] | tc0[i][1] << 8 | tc0[i][2] << 16 | static_cast<uint32_t>(tc0[i][3]) << 24, bt[i] = beta[i];
    }
    long bad = 0;
    for (long iter = 0; iter < cases; iter++) {
        MbRec q, l, t;
        const int mode = static_cast<int>(iter % 4);
        rnd_rec(&q, mode), rnd_rec(&l, mode), rnd_rec(&t, mode);
        if (mode == 1 && (rnd() & 1)) { // near-identical inter neighbours with few coefficients: vector differences around the limits decide
            l = q, t = q;
            for (int i = 0; i < 16; i++) {
                l.mv[i][0] = static_cast<int16_t>(l.mv[i][0] + static_cast<int>(rnd() % 9) - 4), t.mv[i][1] = static_cast<int16_t>(t.mv[i][1] + static_cast<int>(rnd() % 9) - 4);
                const int c = rnd() & 1;
                q.mv[i][c] = static_cast<int16_t>(q.mv[i][c] + static_cast<int>(rnd() % 9) - 4);
            }
            q.nzmask = l.nzmask = t.nzmask = static_cast<uint16_t>(rnd() & rnd() & rnd() & rnd());
            q.type = l.type = t.type = MBT_P8x8;
        }
        const bool hl = (rnd() & 3) != 0, ht = (rnd() & 3) != 0, field = (rnd() & 1) != 0;
        DbPrm want;
        ref_prm(&q, hl ? &l : nullptr, ht ? &t : nullptr, field, &want);
        IpLane in;
        const uint32_t *qd = reinterpret_cast<const uint32_t *>(&q), *ld = reinterpret_cast<const uint32_t *>(&l), *td = reinterpret_cast<const uint32_t *>(&t);
        for (int i = 0; i < 4; i++) in.h[i] = qd[i], in.l[i] = ld[i], in.t[i] = td[i], in.lmv[i] = ld[15 + 4 * i], in.tmv[i] = td[24 + i];
        for (int i = 0; i < 16; i++) in.mv[i] = qd[12 + i];
        in.r01 = qd[9], in.r23 = qd[10], in.lr01 = ld[9], in.lr23 = ld[10], in.tr23 = td[10];
        in.has_left = hl, in.has_top = ht;
        if (!ht) memset(in.t, 0, sizeof(in.t)), memset(in.tmv, 0, sizeof(in.tmv)), in.tr23 = 0; // (the kernel loads nothing above the first row)
        uint32_t o[20];
        ip_dbprm(in, field, at, bt, o);
        if (memcmp(o, &want, sizeof(want)) && bad++ < 3) {
            printf("mismatch: case %ld mode %d left %d top %d field %d\n", iter, mode, hl, ht, field);
            for (int i = 0; i < 80; i++) printf("%02x%s", reinterpret_cast<const uint8_t *>(o)[i], i % 16 == 15 ? "\n" : " ");
            for (int i = 0; i < 80; i++) printf("%02x%s", reinterpret_cast<const uint8_t *>(&want)[i], i % 16 == 15 ? "\n" : " ");
        }
    }
    printf("%ld cases, %ld mismatches\n", cases, bad);
    return bad != 0;
}
