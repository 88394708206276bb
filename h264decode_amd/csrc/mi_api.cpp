// h264decode_amd/csrc/mi_api.cpp -- the C ABI of libh264mi.so (include/h264mi.h): host-side
// front end (NAL dispatch h264/server.go:113-166; where pictures go in a batch's tables, asking mi_dpb.cpp -- picture management 8.2 -- for
// slots, counts and lists), GPU launch sequence, and the read-back and query calls.  The output stage (K6 .. K9: pack, convert, scale, model-input
// tensors, and their device-free rule functions) is mi_output.cpp; the decoder's state, which both files work on, is mi_decoder.hpp.
//
// There is deliberately NO CPU pixel path in this library: every sample is produced by the HIP
// kernels in k_entropy.hip / k_recon.hip / k_deblock.hip.  If no device is usable the create call
// fails (H264MI_ENODEVICE).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <thread>
#include <functional>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/h264mi.h"
#include "mi_decoder.hpp"
#include "mi_tables.h"

// ---------------------------------------------------------------- device tables
static void put_vlc(uint16_t *lut, int bits, int len, uint32_t code, uint16_t value) {
    if (!len || len > bits) return;
    uint32_t base = code << (bits - len), n = 1u << (bits - len);
    for (uint32_t i = 0; i < n; i++) lut[base + i] = static_cast<uint16_t>((len << 8) | value);
}
// The CAVLC tables: direct-indexed first (every window of L bits -> len << 8 | value, from the code lists of mi_tables.h), then folded into the compact
// form the kernels keep in LDS (mi_types.h: MI_VLC_*).  `mismatches` (h264mi_internal_vlc_selftest): every window of every direct table is looked
// up in the compact one as the kernels do it, and run_before's closed form for zerosLeft > 6 is compared with its table.
static void build_vlc(uint16_t *c, int *mismatches) {
    std::vector<uint16_t> ct[3] = {std::vector<uint16_t>(1u << MI_VLC_CT0_L), std::vector<uint16_t>(1u << MI_VLC_CT1_L), std::vector<uint16_t>(1u << MI_VLC_CT2_L)};
    std::vector<uint16_t> ct3(64), cdc(1u << MI_VLC_CDC_L), tz(15u << MI_VLC_TZ_L), cdctz(24), run(7u << 11);
    const int ctl[3] = {MI_VLC_CT0_L, MI_VLC_CT1_L, MI_VLC_CT2_L}, ctbase[3] = {MI_VLC_CT0, MI_VLC_CT1, MI_VLC_CT2};
    for (int tc = 0; tc <= 16; tc++)
        for (int t1 = 0; t1 <= std::min(tc, 3); t1++) {
            const uint16_t v = static_cast<uint16_t>((tc << 2) | t1);
            for (int k = 0; k < 3; k++) put_vlc(ct[k].data(), ctl[k], mi_coeff_token_len[k][4 * tc + t1], mi_coeff_token_bits[k][4 * tc + t1], v);
            put_vlc(ct3.data(), 6, mi_coeff_token_len[3][4 * tc + t1], mi_coeff_token_bits[3][4 * tc + t1], v);
            if (tc <= 4) put_vlc(cdc.data(), MI_VLC_CDC_L, mi_chroma_dc_token_len[4 * tc + t1], mi_chroma_dc_token_bits[4 * tc + t1], v);
        }
    for (int tc = 1; tc <= 15; tc++)
        for (int z = 0; z <= 16 - tc && z < 16; z++)
            put_vlc(tz.data() + ((tc - 1) << MI_VLC_TZ_L), MI_VLC_TZ_L, mi_total_zeros_len[tc - 1][z], mi_total_zeros_bits[tc - 1][z], static_cast<uint16_t>(z));
    for (int tc = 1; tc <= 3; tc++)
        for (int z = 0; z <= 4 - tc; z++) put_vlc(cdctz.data() + 8 * (tc - 1), 3, mi_chroma_dc_total_zeros_len[tc - 1][z], mi_chroma_dc_total_zeros_bits[tc - 1][z], static_cast<uint16_t>(z));
    for (int zl = 1; zl <= 7; zl++)
        for (int r = 0; r < 15; r++) put_vlc(run.data() + ((zl - 1) << 11), 11, mi_run_len[zl - 1][r], mi_run_bits[zl - 1][r], static_cast<uint16_t>(r));
    memset(c, 0, sizeof(uint16_t) * MI_VLC_N);
    int bad = 0;
    // fold: the entry of group lz, suffix s is what the direct table says for the window 0^lz 1 s 0...; the code must end inside those bits
    auto fold = [&](const uint16_t *direct, int L, int S, uint16_t *out) {
        for (int lz = 0; lz <= L; lz++)
            for (uint32_t sfx = 0; sfx < (1u << S); sfx++) {
                uint32_t win = lz < L ? (1u << (31 - lz)) : 0u; // as a 32-bit window, MSB first
                if (lz + 1 < 32) win |= lz < L ? (sfx << (32 - S)) >> (lz + 1) : 0u;
                const uint16_t e = direct[win >> (32 - L)];
                if ((e >> 8) > lz + 1 + S && lz < L) bad++; // a code longer than the bits that select its entry
                out[(lz << S) | sfx] = e;
            }
    };
    for (int k = 0; k < 3; k++) fold(ct[k].data(), ctl[k], MI_VLC_CT_S, c + ctbase[k]);
    memcpy(c + MI_VLC_CT3, ct3.data(), 64 * sizeof(uint16_t));
    fold(cdc.data(), MI_VLC_CDC_L, MI_VLC_CDC_S, c + MI_VLC_CDC);
    for (int k = 0; k < 15; k++) fold(tz.data() + (k << MI_VLC_TZ_L), MI_VLC_TZ_L, MI_VLC_TZ_S, c + MI_VLC_TZ + k * MI_VLC_TZ_STRIDE);
    memcpy(c + MI_VLC_CDCTZ, cdctz.data(), 24 * sizeof(uint16_t));
    for (int zl = 1; zl <= 6; zl++)
        for (int i = 0; i < 8; i++) c[MI_VLC_RUN + 8 * (zl - 1) + i] = run[((zl - 1) << 11) + (i << 8)];
    if (!mismatches) return;
    // every window of every direct table, looked up the way the kernels do it
    auto check = [&](const uint16_t *direct, int L, int S, const uint16_t *folded) {
        for (uint32_t i = 0; i < (1u << L); i++) {
            const uint32_t w = i << (32 - L);
            const int lz = w ? __builtin_clz(w) : 32;
            if (folded[MI_VLC_INDEX(w, lz, L, S)] != direct[i]) bad++;
        }
    };
    for (int k = 0; k < 3; k++) check(ct[k].data(), ctl[k], MI_VLC_CT_S, c + ctbase[k]);
    check(cdc.data(), MI_VLC_CDC_L, MI_VLC_CDC_S, c + MI_VLC_CDC);
    for (int k = 0; k < 15; k++) check(tz.data() + (k << MI_VLC_TZ_L), MI_VLC_TZ_L, MI_VLC_TZ_S, c + MI_VLC_TZ + k * MI_VLC_TZ_STRIDE);
    for (int zl = 1; zl <= 6; zl++)
        for (uint32_t i = 0; i < 2048; i++) {
            const uint16_t e = run[((zl - 1) << 11) + i];
            if (e && c[MI_VLC_RUN + 8 * (zl - 1) + (i >> 8)] != e) bad++; // (codes of at most 3 bits; e == 0: a window no code matches)
            if (!e && c[MI_VLC_RUN + 8 * (zl - 1) + (i >> 8)] != 0) bad++;
        }
    for (uint32_t i = 0; i < 2048; i++) {
        const uint32_t w = i << 21;
        const int lz = w ? __builtin_clz(w) : 32;
        if (MI_RUN_BEFORE_LONG(w, lz) != run[(6u << 11) + i]) bad++;
    }
    *mismatches = bad;
}
#if defined(H264MI_TEST_HOOKS)
extern "C" int32_t h264mi_internal_vlc_selftest(void) {
    std::vector<uint16_t> c(MI_VLC_N);
    int bad = -1;
    build_vlc(c.data(), &bad);
    return bad;
}
#endif
static void build_tables(DevTables *t) {
    memset(t, 0, sizeof(*t));
    memcpy(t->range_lps, mi_range_lps, sizeof(t->range_lps));
    memcpy(t->trans_lps, mi_trans_lps, sizeof(t->trans_lps));
    // 9.3.1.1 (9-5): h264/cabac.go:118-121 PreCtxState, :158-164 split into pStateIdx / valMPS
    for (int set = 0; set < 4; set++)
        for (int qp = 0; qp < 52; qp++)
            for (int i = 0; i < MI_NCTX; i++) {
                int pre = ((mi_cabac_mn[set][i][0] * qp) >> 4) + mi_cabac_mn[set][i][1];
                pre = std::min(std::max(pre, 1), 126);
                // pStateIdx in bits 0..5, valMPS in bit 6: the state is a lane number as it stands (v_readlane takes its select modulo 64)
                t->ctx_init[set][qp][i] = pre <= 63 ? static_cast<uint8_t>(63 - pre) : static_cast<uint8_t>((pre - 64) | 64);
            }
    memcpy(t->sig8x8, mi_sig8x8_ctx, 63);
    memcpy(t->sig8x8_field, mi_sig8x8_field_ctx, 63);
    memcpy(t->last8x8, mi_last8x8_ctx, 63);
    memcpy(t->zigzag4, mi_zigzag4x4, 16);
    memcpy(t->zigzag8, mi_zigzag8x8, 64);
    memcpy(t->fieldscan4, mi_fieldscan4x4, 16);
    memcpy(t->fieldscan8, mi_fieldscan8x8, 64);
    memcpy(t->me_intra, mi_me_intra, 48), memcpy(t->me_intra + 48, mi_me_intra0, 16);
    memcpy(t->me_inter, mi_me_inter, 48), memcpy(t->me_inter + 48, mi_me_inter0, 16);
    memcpy(t->alpha, mi_alpha, 52);
    memcpy(t->beta, mi_beta, 52);
    for (int i = 0; i < 52; i++) {
        for (int b = 0; b < 3; b++) t->tc0[i][b + 1] = mi_tc0[i][b];
        t->qpc[i] = i < 30 ? static_cast<uint8_t>(i) : mi_qpc_tab[i - 30];
    }
    build_vlc(t->vlc_c, nullptr);
}
static void build_scaling(const uint8_t s4[6][16], const uint8_t s8[2][64], ScalingSet *o) { // 8.5.9
    for (int l = 0; l < 6; l++)
        for (int q = 0; q < 6; q++)
            for (int k = 0; k < 16; k++) {
                int r = mi_zigzag4x4[k], x = r & 3, y = r >> 2;
                int v = (!(x & 1) && !(y & 1)) ? mi_norm4x4[q][0] : (((x & 1) && (y & 1)) ? mi_norm4x4[q][1] : mi_norm4x4[q][2]);
                o->ls4[l][q][r] = static_cast<uint16_t>(s4[l][k] * v);
            }
    for (int l = 0; l < 2; l++)
        for (int q = 0; q < 6; q++)
            for (int k = 0; k < 64; k++) {
                int r = mi_zigzag8x8[k], x = r & 7, y = r >> 3, c;
                if (!(x & 3) && !(y & 3))
                    c = 0;
                else if ((x & 1) && (y & 1))
                    c = 1;
                else if ((x & 3) == 2 && (y & 3) == 2)
                    c = 2;
                else if ((!(y & 3) && (x & 1)) || ((y & 1) && !(x & 3)))
                    c = 3;
                else if ((!(y & 3) && (x & 3) == 2) || ((y & 3) == 2 && !(x & 3)))
                    c = 4;
                else
                    c = 5;
                o->ls8[l][q][r] = static_cast<uint16_t>(s8[l][k] * mi_norm8x8[q][c]);
            }
}

static int g_device = -1;

extern "C" const char *h264mi_last_error_string(void) { return last_error(); }
extern "C" const char *h264mi_version(void) { return "h264mi 0.1 (gfx950)"; }

extern "C" int32_t h264mi_annexb_scan(const uint8_t *buf, size_t len, h264mi_nal *out, int32_t cap, int32_t *n) {
    if (!buf || !out || !n || cap < 0) return H264MI_EINVAL;
    int cnt = 0;
    int r = annexb_scan(buf, len, out, cap, &cnt);
    *n = cnt;
    return r;
}
extern "C" int32_t h264mi_nal_parse(const uint8_t *nal, size_t len, h264mi_nal *hdr, uint8_t *rbsp, size_t *rbsp_len) { return nal_parse(nal, len, hdr, rbsp, rbsp_len); }
extern "C" int32_t h264mi_sps_parse(const uint8_t *rbsp, size_t len, h264mi_sps *sps) { return parse_sps(rbsp, len, sps); }
extern "C" int32_t h264mi_pps_parse(const h264mi_sps *sps, const uint8_t *rbsp, size_t len, h264mi_pps *pps) { return parse_pps(sps, rbsp, len, pps); }
extern "C" int32_t h264mi_pps_slice_group_ids(const h264mi_sps *sps, const uint8_t *rbsp, size_t len, uint8_t *ids, size_t cap, size_t *n) {
    h264mi_pps tmp;
    return parse_pps_ids(sps, rbsp, len, &tmp, ids, cap, n);
}
extern "C" int32_t h264mi_map_unit_to_slice_group_map(const h264mi_sps *sps, const h264mi_pps *pps, const uint8_t *ids, size_t n_ids, int32_t cycle, uint8_t *map, size_t cap,
                                                      size_t *n) {
    return map_unit_to_slice_group_map(sps, pps, ids, n_ids, cycle, map, cap, n);
}
extern "C" int32_t h264mi_mb_to_slice_group_map(const h264mi_sps *sps, const h264mi_pps *pps, const uint8_t *ids, size_t n_ids, int32_t cycle, int32_t field_pic, uint8_t *map,
                                                size_t cap, size_t *n) {
    return mb_to_slice_group_map(sps, pps, ids, n_ids, cycle, field_pic, map, cap, n);
}
extern "C" int32_t h264mi_next_mb_address(const uint8_t *map, size_t n_mbs, size_t n) { return next_mb_address(map, n_mbs, n); }
extern "C" int32_t h264mi_slice_header_parse(const h264mi_sps *sps, const h264mi_pps *pps, int32_t nal_ref_idc, int32_t nal_unit_type, const uint8_t *rbsp,
                                             size_t len, h264mi_slice_header *sh) {
    return parse_slice_header(sps, pps, nal_ref_idc, nal_unit_type, rbsp, len, sh);
}

extern "C" int32_t h264mi_init(int32_t device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available: the decode path needs a gfx950 GPU (there is no CPU fallback)");
        return H264MI_ENODEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (0..%d)", device, n - 1);
        return H264MI_EINVAL;
    }
    HIP_TRY(hipSetDevice(device));
    g_device = device;
    return H264MI_OK;
}

static void free_all(h264mi_decoder *d) {
    for (Stage &g : d->stage) {
        if (g.d_bits) hipFree(g.d_bits);
        if (g.h_bits) hipHostFree(g.h_bits);
        if (g.d_slices) hipFree(g.d_slices);
        if (g.h_slices) hipHostFree(g.h_slices);
        if (g.d_pics) hipFree(g.d_pics);
        if (g.h_pics) hipHostFree(g.h_pics);
        if (g.d_status) hipFree(g.d_status);
        if (g.h_status) hipHostFree(g.h_status);
        if (g.d_lists) hipFree(g.d_lists);
        if (g.h_lists) hipHostFree(g.h_lists);
        if (g.d_bext) hipFree(g.d_bext);
        if (g.h_bext) hipHostFree(g.h_bext);
        if (g.d_dpoc) hipFree(g.d_dpoc);
        if (g.h_dpoc) hipHostFree(g.h_dpoc);
        if (g.d_cmap) hipFree(g.d_cmap);
        if (g.h_cmap) hipHostFree(g.h_cmap);
        if (g.ev_upload) hipEventDestroy(g.ev_upload);
        if (g.ev_done) hipEventDestroy(g.ev_done);
    }
    for (int i = 0; i < MI_SETS; i++) {
        if (d->d_mbrec[i]) hipFree(d->d_mbrec[i]);
        if (d->d_mv1[i]) hipFree(d->d_mv1[i]);
        if (d->d_dbprm[i]) hipFree(d->d_dbprm[i]);
        if (d->d_imask[i]) hipFree(d->d_imask[i]);
        if (i == 0 && d->d_coef[0]) hipFree(d->d_coef[0]);
        if (i == 0 && d->d_pool_head) hipFree(d->d_pool_head);
        if (d->d_toprows[i]) hipFree(d->d_toprows[i]);
        if (d->ev_ent[i]) hipEventDestroy(d->ev_ent[i]);
        if (d->ev_col[i]) hipEventDestroy(d->ev_col[i]);
        if (d->ev_rec[i]) hipEventDestroy(d->ev_rec[i]);
    }
    for (int i = 0; i < 2; i++)
        if (d->ent_stream[i]) hipStreamDestroy(d->ent_stream[i]);
    if (d->rec_stream) hipStreamDestroy(d->rec_stream);
    if (d->ev_user) hipEventDestroy(d->ev_user);
    if (d->d_colrec) hipFree(d->d_colrec);
    if (d->d_backfill) hipFree(d->d_backfill);
    if (d->d_xring) hipFree(d->d_xring);
    if (d->d_xdone) hipFree(d->d_xdone);
    if (d->d_xctl) hipFree(d->d_xctl);
    if (d->h_xstatus) hipHostFree(d->h_xstatus);
    if (d->d_pools) hipFree(d->d_pools);
    for (DescTables &t : d->tables)
        for (int i = 0; i < 2; i++) {
            if (t.h[i]) hipHostFree(t.h[i]);
            if (t.d[i]) hipFree(t.d[i]);
            if (t.ev[i]) hipEventDestroy(t.ev[i]);
        }
    if (d->d_derived) hipFree(d->d_derived);
    if (d->d_frames) hipFree(d->d_frames);
    if (d->d_tables) hipFree(d->d_tables);
    if (d->h_tables) hipHostFree(d->h_tables);
    for (auto e : d->ev) hipEventDestroy(e);
    if (d->own_stream && d->stream) hipStreamDestroy(d->stream);
}

static int ensure_b_buffers(h264mi_decoder *d);

extern "C" int32_t h264mi_decoder_create(const h264mi_config *cfg_, h264mi_decoder **out) {
    if (!cfg_ || !out) return H264MI_EINVAL;
    // the caller's struct may be shorter (an older header) or longer (a newer one) than this build's: fields beyond either end are 0
    if (cfg_->struct_size < offsetof(h264mi_config, max_ref_frames) || cfg_->struct_size > 4096) {
        set_error("h264mi_decoder_create: h264mi_config.struct_size = %u (set it to sizeof(h264mi_config); the struct must be zero-initialised)", cfg_->struct_size);
        return H264MI_EINVAL;
    }
    h264mi_config cfg_copy;
    memset(&cfg_copy, 0, sizeof(cfg_copy));
    memcpy(&cfg_copy, cfg_, std::min<size_t>(cfg_->struct_size, sizeof(cfg_copy)));
    const h264mi_config *cfg = &cfg_copy;
    if (cfg->max_streams < 1 || cfg->max_width < 16 || cfg->max_height < 16 || cfg->max_frames_per_batch < 1) return H264MI_EINVAL;
    if ((cfg->conceal_errors & ~(H264MI_CONCEAL_SLICES | H264MI_CONCEAL_PICTURES | H264MI_CONCEAL_FIELDS | H264MI_CONCEAL_IDR | H264MI_CONCEAL_LONE_FIELDS)) ||
        (cfg->conceal_errors && !(cfg->conceal_errors & H264MI_CONCEAL_SLICES)) ||
        ((cfg->conceal_errors & H264MI_CONCEAL_LONE_FIELDS) && !(cfg->conceal_errors & H264MI_CONCEAL_FIELDS))) {
        set_error("h264mi_decoder_create: h264mi_config.conceal_errors = %d (0, or H264MI_CONCEAL_SLICES with or without H264MI_CONCEAL_PICTURES, H264MI_CONCEAL_FIELDS and "
                  "H264MI_CONCEAL_IDR: 0, 1, 3, 5, 7, 17, 19, 21, 23; H264MI_CONCEAL_LONE_FIELDS only together with H264MI_CONCEAL_FIELDS: 69, 71, 85, 87)",
                  cfg->conceal_errors);
        return H264MI_EINVAL;
    }
    int r = h264mi_init(cfg->device);
    if (r != H264MI_OK) return r;
    h264mi_decoder *d = new h264mi_decoder();
    d->cfg = *cfg;
    d->conceal = (cfg->conceal_errors & H264MI_CONCEAL_SLICES) != 0, d->conceal_pics = (cfg->conceal_errors & H264MI_CONCEAL_PICTURES) != 0;
    d->conceal_fields = (cfg->conceal_errors & H264MI_CONCEAL_FIELDS) != 0, d->conceal_idr = (cfg->conceal_errors & H264MI_CONCEAL_IDR) != 0;
    d->conceal_lone = (cfg->conceal_errors & H264MI_CONCEAL_LONE_FIELDS) != 0;
    if (d->cfg.max_slices_per_frame < 1) d->cfg.max_slices_per_frame = 1;
    d->Wmax = (cfg->max_width + 15) & ~15;
    d->Hmax = (cfg->max_height + 15) & ~15;
    if (d->Wmax > 8192 || d->Hmax > 5120) { // LDS row-state of K3 (320 rows x 512 columns of macroblocks) and K5 (96 row groups)
        set_error("h264mi_decoder_create: pictures larger than 8192x5120 are not supported");
        delete d;
        return H264MI_EUNSUPPORTED;
    }
    // frame slots per stream: the outputs of the batch being prepared and of the one before it (still being read or executed:
    // MI_STAGES batches are in flight), up to 16 reference pictures, and the picture under construction
    if (d->cfg.max_ref_frames < 1 || d->cfg.max_ref_frames > MI_MAX_REFS) d->cfg.max_ref_frames = MI_MAX_REFS;
    d->n_slots = MI_STAGES * cfg->max_frames_per_batch + d->cfg.max_ref_frames + 1;
    if (d->n_slots >= MI_REF_PARITY) { // (reference entries of field pictures keep the field's parity in bit 14 of the slot number)
        set_error("h264mi_decoder_create: max_frames_per_batch %d is too large (at most %d)", cfg->max_frames_per_batch, (MI_REF_PARITY - 18) / MI_STAGES);
        delete d;
        return H264MI_EINVAL;
    }
    d->slot_bytes = (static_cast<size_t>(d->Wmax) * d->Hmax * 3 / 2 + 255) & ~static_cast<size_t>(255);
    const int S = cfg->max_streams;
    d->st.resize(S);
    for (auto &s : d->st) s.dpb.slots.resize(d->n_slots);
    d->pics_cap = S * cfg->max_frames_per_batch;
    d->slices_cap = d->pics_cap * d->cfg.max_slices_per_frame;
    d->mb_cap = static_cast<uint64_t>(d->pics_cap) * (d->Wmax / 16) * (d->Hmax / 16);
    d->bits_cap = cfg->max_bitstream_bytes > 0 ? static_cast<size_t>(cfg->max_bitstream_bytes) : std::max<size_t>(static_cast<size_t>(d->pics_cap) * d->Wmax * d->Hmax / 2, 1 << 20);
    d->bits_cap = (d->bits_cap + 16 * static_cast<size_t>(d->slices_cap) + 8192 + 15) & ~static_cast<size_t>(15);
    auto fail = [&](int code) {
        free_all(d);
        delete d;
        return code;
    };
#define DEV_ALLOC(ptr, bytes)                      \
    do {                                           \
        const size_t _n = (bytes);                 \
        TRY_ALLOC(hipMalloc(&(ptr), _n));          \
        d->dev_bytes += _n;                        \
    } while (0)
#define TRY_ALLOC(x)                                                                 \
    do {                                                                             \
        hipError_t _e = (x);                                                         \
        if (_e != hipSuccess) {                                                      \
            set_error("%s failed: %s", #x, hipGetErrorString(_e));                   \
            return fail(_e == hipErrorOutOfMemory ? H264MI_ENOMEM : H264MI_EDEVICE); \
        }                                                                            \
    } while (0)
    if (cfg->hip_stream)
        d->stream = static_cast<hipStream_t>(cfg->hip_stream);
    else {
        TRY_ALLOC(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        d->own_stream = true;
    }
    // error concealment: one more SliceDesc per picture (what concealed macroblocks point at; it takes no entropy wavefront and does not count
    // against max_slices_per_frame), and behind the status words one counter per picture (k_conceal)
    const size_t slices_alloc = static_cast<size_t>(d->slices_cap) + (d->conceal ? d->pics_cap : 0);
    const size_t status_alloc = static_cast<size_t>(8) * d->slices_cap + (d->conceal ? static_cast<size_t>(d->pics_cap) : 0);
    for (Stage &g : d->stage) {
        DEV_ALLOC(g.d_bits, d->bits_cap);
        TRY_ALLOC(hipHostMalloc(&g.h_bits, d->bits_cap));
        DEV_ALLOC(g.d_slices, sizeof(SliceDesc) * slices_alloc);
        TRY_ALLOC(hipHostMalloc(&g.h_slices, sizeof(SliceDesc) * slices_alloc));
        DEV_ALLOC(g.d_pics, sizeof(PicDesc) * d->pics_cap);
        TRY_ALLOC(hipHostMalloc(&g.h_pics, sizeof(PicDesc) * d->pics_cap));
        DEV_ALLOC(g.d_status, sizeof(uint32_t) * status_alloc);
        TRY_ALLOC(hipHostMalloc(&g.h_status, sizeof(uint32_t) * status_alloc));
        DEV_ALLOC(g.d_dpoc, sizeof(int16_t) * 2 * MI_MAX_REFS * slices_alloc);
        TRY_ALLOC(hipHostMalloc(&g.h_dpoc, sizeof(int16_t) * 2 * MI_MAX_REFS * slices_alloc));
        if (d->conceal) {
            DEV_ALLOC(g.d_cmap, sizeof(uint32_t) * (static_cast<size_t>(d->pics_cap) + d->slices_cap));
            TRY_ALLOC(hipHostMalloc(&g.h_cmap, sizeof(uint32_t) * (static_cast<size_t>(d->pics_cap) + d->slices_cap)));
        }
        DEV_ALLOC(g.d_lists, sizeof(uint32_t) * 6 * d->pics_cap);
        TRY_ALLOC(hipHostMalloc(&g.h_lists, sizeof(uint32_t) * 6 * d->pics_cap));
        DEV_ALLOC(g.d_bext, sizeof(BSliceExt) * d->slices_cap);
        TRY_ALLOC(hipHostMalloc(&g.h_bext, sizeof(BSliceExt) * d->slices_cap));
        TRY_ALLOC(hipEventCreateWithFlags(&g.ev_upload, hipEventDisableTiming));
        TRY_ALLOC(hipEventCreateWithFlags(&g.ev_done, hipEventDisableTiming));
        g.out.resize(S);
        memset(&g.info, 0, sizeof(g.info));
    }
    {
        // Optional experiment knob: H264MI_ENT_CUS=n gives the entropy streams the first n compute units
        // and reconstruction the rest (hipExtStreamCreateWithCUMask).  Measured slower than sharing the
        // whole chip at every split tried (96..192 of 256), so the default is no partition.
        hipDeviceProp_t prop;
        TRY_ALLOC(hipGetDeviceProperties(&prop, cfg->device));
        const int ncu = prop.multiProcessorCount;
        int ent_cus = 0;
#if defined(H264MI_TEST_HOOKS) /* measurement switches of the hooks build (libh264mi_hooks.so) */
        if (const char *e = getenv("H264MI_ENT_LDS_PAD")) d->ent_lds_pad = static_cast<size_t>(atoi(e));
        if (const char *e = getenv("H264MI_ENT_CUS")) ent_cus = atoi(e);
#endif
        const int words = (ncu + 31) / 32;
        std::vector<uint32_t> me(words, 0), mr(words, 0);
        bool split = ent_cus > 0 && ent_cus < ncu;
        for (int i = 0; i < ncu; i++) {
            // interleave in blocks of 8 so that both partitions span all XCDs / shader engines
            const int k = i / 8;
            bool ent = split ? (((k + 1) * ent_cus / ncu) != (k * ent_cus / ncu)) : true;
            if (ent) me[i / 32] |= 1u << (i % 32);
            if (!ent || !split) mr[i / 32] |= 1u << (i % 32);
        }
        for (int i = 0; i < 2; i++) {
            if (split)
                TRY_ALLOC(hipExtStreamCreateWithCUMask(&d->ent_stream[i], words, me.data()));
            else
                TRY_ALLOC(hipStreamCreateWithFlags(&d->ent_stream[i], hipStreamNonBlocking));
        }
        if (split)
            TRY_ALLOC(hipExtStreamCreateWithCUMask(&d->rec_stream, words, mr.data()));
        else
            TRY_ALLOC(hipStreamCreateWithFlags(&d->rec_stream, hipStreamNonBlocking));
        TRY_ALLOC(hipEventCreateWithFlags(&d->ev_user, hipEventDisableTiming));
    }
    for (int i = 0; i < MI_SETS; i++) {
        DEV_ALLOC(d->d_mbrec[i], sizeof(MbRec) * d->mb_cap);
        DEV_ALLOC(d->d_dbprm[i], sizeof(DbPrm) * d->mb_cap);
        DEV_ALLOC(d->d_imask[i], sizeof(unsigned long long) * (d->mb_cap / 64 + 2));
        if (i == 0) {
            // Pool size.  The worst case is 26 blocks (832 bytes) per macroblock; real streams code a fraction of that (the
            // 1080p QP 28 bench streams: ~5 blocks per macroblock).  Small decoders get the worst case; large ones 8 blocks
            // per macroblock, at least 1 GiB -- a batch that needs more fails with H264MI_EDECODE ("coefficient pool
            // exhausted", code 40) instead of reserving 3 x 52 GB for a case that does not occur.  H264MI_COEF_BLOCKS_PER_MB overrides.
            const uint64_t worst = d->mb_cap * MI_COEF_BLOCKS + static_cast<uint64_t>(d->slices_cap + 1) * MI_COEF_CHUNK;
            uint64_t per_mb = 8;
            if (const char *e = getenv("H264MI_COEF_BLOCKS_PER_MB")) per_mb = static_cast<uint64_t>(std::min(std::max(atoi(e), 1), MI_COEF_BLOCKS));
            if (d->cfg.coef_blocks_per_mb > 0) per_mb = static_cast<uint64_t>(std::min<int>(d->cfg.coef_blocks_per_mb, MI_COEF_BLOCKS));
            // (an explicit coef_blocks_per_mb is taken at its word; the default has a floor of 1 GiB)
            const uint64_t typical = (d->cfg.coef_blocks_per_mb > 0 ? d->mb_cap * per_mb : std::max<uint64_t>(d->mb_cap * per_mb, (1ull << 30) / 32)) +
                                     static_cast<uint64_t>(d->slices_cap + 1) * MI_COEF_CHUNK;
            d->pool_blocks = std::min<uint64_t>(std::min<uint64_t>(worst, typical), 0xFFFF0000ull / MI_SETS);
            DEV_ALLOC(d->d_pool_head, sizeof(uint32_t) * MI_SETS);
        }
        // the MI_SETS pools are ONE allocation: a pass that ran out of residual blocks is repeated on its own with all of it (retry_exhausted)
        if (i == 0) DEV_ALLOC(d->d_coef[0], d->pool_blocks * 32 * MI_SETS);
        else d->d_coef[i] = d->d_coef[0] + static_cast<size_t>(i) * d->pool_blocks * 16;
        DEV_ALLOC(d->d_toprows[i], static_cast<size_t>(d->slices_cap) * (d->Wmax / 16) * MI_TOPROW_BYTES);
        TRY_ALLOC(hipEventCreateWithFlags(&d->ev_ent[i], hipEventDisableTiming));
        TRY_ALLOC(hipEventCreateWithFlags(&d->ev_col[i], hipEventDisableTiming));
        TRY_ALLOC(hipEventCreateWithFlags(&d->ev_rec[i], hipEventDisableTiming));
    }
    DEV_ALLOC(d->d_pools, sizeof(FramePool) * S);
    DEV_ALLOC(d->d_frames, d->slot_bytes * d->n_slots * S + 256); // (K4's unaligned dword loads may read 3 bytes past a plane)
    // 80 bytes per macroblock and frame slot: whatever a later B picture may need of a reference picture's motion (8.4.1.2.1)
    d->colrec_per_slot = static_cast<size_t>(d->Wmax / 16) * (d->Hmax / 16);
    // (the ColRec arrays themselves -- 12.9 GB for 256 streams of 1080p -- are allocated when the first B slice arrives: ensure_b_buffers)
    DEV_ALLOC(d->d_tables, sizeof(DevTables));
    TRY_ALLOC(hipHostMalloc(&d->h_tables, sizeof(DevTables)));
    // K5 keeps a whole macroblock row per in-flight group in dynamic LDS (up to 320 columns): opt in beyond 64 KB
    TRY_ALLOC(hipFuncSetAttribute(reinterpret_cast<const void *>(k_deblock), hipFuncAttributeMaxDynamicSharedMemorySize, MI_DEBLOCK_LDS_MAX));
    TRY_ALLOC(hipFuncSetAttribute(reinterpret_cast<const void *>(k_deblock_x), hipFuncAttributeMaxDynamicSharedMemorySize, MI_DEBLOCK_LDS_MAX));
    // cross-workgroup hand-off state of the banded kernels; H264MI_X_WGS = 0 switches them off, n: up to n workgroups per launch
    if (const char *e = getenv("H264MI_X_WGS")) d->x_max_wgs = std::min(std::max(atoi(e), 0), d->x_cap);
#if defined(H264MI_TEST_HOOKS)
    if (const char *e = getenv("H264MI_K5_WAVES")) d->k5_max_waves = std::min(std::max(atoi(e), 1), MI_DEBLOCK8_MAX_WAVES); // measurement: fewer wavefronts per picture in k_deblock
#endif
    // (test hook: where the launch epoch and the ticket counters start, so that a test can cross their 32-bit wrap)
    DEV_ALLOC(d->d_xring, static_cast<size_t>(d->x_cap) * (d->Wmax / 16) * 24 * sizeof(unsigned long long));
    DEV_ALLOC(d->d_xdone, static_cast<size_t>(d->x_cap3) * (d->Wmax / 16) * sizeof(uint32_t));
    DEV_ALLOC(d->d_xctl, 8 * 128);
    TRY_ALLOC(hipHostMalloc(&d->h_xstatus, sizeof(uint32_t)));
    *d->h_xstatus = 0;
    TRY_ALLOC(hipMemset(d->d_xring, 0, static_cast<size_t>(d->x_cap) * (d->Wmax / 16) * 24 * sizeof(unsigned long long)));
    TRY_ALLOC(hipMemset(d->d_xdone, 0, static_cast<size_t>(d->x_cap3) * (d->Wmax / 16) * sizeof(uint32_t)));
    TRY_ALLOC(hipMemset(d->d_xctl, 0, 8 * 128));
    build_tables(d->h_tables);
    d->h_pools.resize(S);
    for (int si = 0; si < S; si++) { // static per stream (kernels take the geometry of a picture from its PicDesc)
        FramePool &fp = d->h_pools[si];
        fp.base = reinterpret_cast<uint64_t>(d->d_frames) + static_cast<uint64_t>(si) * d->slot_bytes * d->n_slots;
        fp.slot_bytes = d->slot_bytes;
        fp.w = fp.h = 0;
        fp.n_slots = static_cast<uint32_t>(d->n_slots);
        fp.pad = 0;
    }
    TRY_ALLOC(hipMemcpy(d->d_pools, d->h_pools.data(), sizeof(FramePool) * S, hipMemcpyHostToDevice));
    // a deterministic background for macroblocks no slice covers
    TRY_ALLOC(hipMemsetAsync(d->d_frames, 128, d->slot_bytes * d->n_slots * S, d->stream));
    TRY_ALLOC(hipStreamSynchronize(d->stream));
#undef TRY_ALLOC
#undef DEV_ALLOC
    if (d->cfg.b_pictures) { // the caller expects B pictures: their buffers now, motion kept from the first picture on
        r = ensure_b_buffers(d);
        if (r != H264MI_OK) {
            free_all(d);
            delete d;
            return r;
        }
    }
    *out = d;
    return H264MI_OK;
}

extern "C" int32_t h264mi_decoder_destroy(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    for (int i = 0; i < 2; i++) hipStreamSynchronize(d->ent_stream[i]);
    hipStreamSynchronize(d->rec_stream);
    hipStreamSynchronize(d->stream);
    free_all(d);
    delete d;
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_set_stream(h264mi_decoder *d, void *s) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    hipStreamSynchronize(d->stream);
    if (d->own_stream) hipStreamDestroy(d->stream);
    d->own_stream = false;
    d->stream = static_cast<hipStream_t>(s);
    return H264MI_OK;
}
// Forget everything about a stream: parameter sets, reference pictures, POC / frame_num history, outputs.
static void reset_stream(StreamState &s, bool keep_parameter_sets) {
    s.dpb.reset();
    s.epoch++;
    s.cur_pic = -1, s.cur_slices = 0;
    s.n_pics_in_batch = 0;
    s.pending_drops = 0;
    s.ref_seq = StreamState::RefSeq();
    if (!keep_parameter_sets) {
        memset(s.sps_ok, 0, sizeof(s.sps_ok));
        memset(s.pps_ok, 0, sizeof(s.pps_ok));
        s.active_sps = -1, s.wmb = s.hmb = 0;
        s.need_idr = false, s.status = H264MI_OK;
    }
}
extern "C" int32_t h264mi_decoder_reset(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    for (auto &s : d->st) reset_stream(s, true);
    d->derived.clear();
    for (Stage &g : d->stage) {
        g.prepared = false;
        for (auto &o : g.out) o.clear();
    }
    return H264MI_OK;
}
extern "C" int32_t h264mi_stream_reset(h264mi_decoder *d, int32_t stream) {
    if (!d || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    reset_stream(d->st[stream], false);
    d->derived.clear(); // (all of them: a derived frame does not outlive the batch it was made from)
    for (Stage &g : d->stage) g.out[stream].clear();
    return H264MI_OK;
}
extern "C" int32_t h264mi_stream_status(h264mi_decoder *d, int32_t stream, int32_t *status) {
    if (!d || !status || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    *status = d->st[stream].status;
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_set_isolation(h264mi_decoder *d, int32_t on) {
    if (!d) return H264MI_EINVAL;
    d->isolate = on != 0;
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_memory(h264mi_decoder *d, int64_t *device_bytes) {
    if (!d || !device_bytes) return H264MI_EINVAL;
    *device_bytes = static_cast<int64_t>(d->dev_bytes);
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_unpinned_failures(h264mi_decoder *d, int64_t *n) {
    if (!d || !n) return H264MI_EINVAL;
    GUARD(d);
    *n = d->unpinned_failures;
    return H264MI_OK;
}

extern "C" int32_t h264mi_decoder_concealed(h264mi_decoder *d, int64_t *slices, int64_t *macroblocks) {
    if (!d || !slices || !macroblocks) return H264MI_EINVAL;
    *slices = d->concealed_slices, *macroblocks = d->concealed_mbs;
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_concealed_pictures(h264mi_decoder *d, int64_t *pictures) {
    if (!d || !pictures) return H264MI_EINVAL;
    *pictures = d->concealed_pics;
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_concealed_fields(h264mi_decoder *d, int64_t *fields) {
    if (!d || !fields) return H264MI_EINVAL;
    *fields = d->concealed_fields;
    return H264MI_OK;
}
extern "C" int32_t h264mi_frame_concealed(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t *n_macroblocks) {
    if (!d || !n_macroblocks || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL; // (H264MI_STREAM_DERIVED too)
    const Stage &g = d->stage[d->exec];
    if (frame < 0 || frame >= static_cast<int>(g.out[stream].size())) return H264MI_EINVAL;
    int32_t n = 0;
    if (d->conceal && g.executed && g.harvested)
        for (int pic : {g.out[stream][frame].pic, g.out[stream][frame].pic2})
            if (pic >= 0 && pic < g.n_pics) n += static_cast<int32_t>(g.h_status[8 * g.n_slices + pic]);
    *n_macroblocks = n;
    return H264MI_OK;
}

extern "C" int32_t h264mi_decoder_coef_pool(h264mi_decoder *d, int64_t *used_blocks, int64_t *capacity_blocks) {
    if (!d || !used_blocks || !capacity_blocks) return H264MI_EINVAL;
    uint32_t heads[MI_SETS] = {0};
    HIP_TRY(hipMemcpy(heads, d->d_pool_head, sizeof(heads), hipMemcpyDeviceToHost));
    uint32_t m = 0;
    for (int i = 0; i < MI_SETS; i++) m = std::max(m, heads[i]);
    *used_blocks = static_cast<int64_t>(m), *capacity_blocks = static_cast<int64_t>(d->pool_blocks);
    return H264MI_OK;
}
extern "C" int32_t h264mi_decoder_set_profiling(h264mi_decoder *d, int32_t on) {
    if (!d) return H264MI_EINVAL;
    d->profiling = on != 0;
    return H264MI_OK;
}

// ---------------------------------------------------------------- the pictures of a batch (picture management, 8.2: mi_dpb.cpp)
static void finish_picture(h264mi_decoder *d, int si) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    Dpb &dpb = s.dpb;
    if (dpb.cur_slot < 0) return;
    dpb.finish_picture(s.sps[s.active_sps]);
    PicDesc &pd = g.h_pics[s.cur_pic];
    pd.n_slices = static_cast<uint32_t>(s.cur_slices);
    if (dpb.cur_field) {
        // a field: the frame goes out when its second field is complete -- or, if that never comes, when the next picture starts (flush_pending_field)
        if (dpb.pend_slot < 0) {
            const Slot &f = dpb.slots[dpb.cur_slot];
            s.pend_out.poc = f.poc;
            s.pend_out.top_foc = f.fpoc[0], s.pend_out.bottom_foc = f.fpoc[1];
            // (pic_order_cnt_type 2 gives both fields of a reference frame one count, and output order is decoding order, 8.2.1.3: this picture is the second field)
            s.pend_out.first_parity = f.fpoc[0] != f.fpoc[1] ? f.fpoc[1] < f.fpoc[0] : 2 - dpb.cur_field;
            if (dpb.cur_second) s.pend_out.pic2 = s.cur_pic;
            g.out[si].push_back(s.pend_out);
        }
    } else if (!g.out[si].empty()) {
        OutFrame &o = g.out[si].back();
        const Slot &f = dpb.slots[dpb.cur_slot];
        o.poc = f.poc, o.top_foc = f.fpoc[0], o.bottom_foc = f.fpoc[1]; // operation 5 rewrites them (first_parity is from before: start_picture)
    }
    // Every macroblock of the picture belongs to exactly one slice wavefront (SliceDesc::fill_from / end_mb): order the
    // slices by first_mb (arbitrary slice order is legal in Baseline); a slice's range ends where the next one starts.
    std::vector<uint32_t> idx(pd.n_slices);
    for (uint32_t i = 0; i < pd.n_slices; i++) idx[i] = pd.first_slice + i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return g.h_slices[a].first_mb < g.h_slices[b].first_mb; });
    const uint32_t total = pd.wmb * pd.hmb;
    if (pd.fmo) {
        // slice groups: a slice ends where the next slice of ITS group starts; nothing is filled by the wavefronts (the records of
        // the whole picture are zeroed before the launch: launch_entropy)
        const uint8_t *map = g.h_bits + pd.sgmap_off;
        for (uint32_t i = 0; i < pd.n_slices; i++) {
            SliceDesc &sd = g.h_slices[idx[i]];
            sd.fill_from = sd.first_mb, sd.end_mb = total;
            for (uint32_t j = i + 1; j < pd.n_slices; j++)
                if (map[g.h_slices[idx[j]].first_mb] == map[sd.first_mb]) {
                    sd.end_mb = std::max(g.h_slices[idx[j]].first_mb, sd.first_mb);
                    break;
                }
        }
        g.fmo_pics.push_back(static_cast<uint32_t>(s.cur_pic));
    } else
        for (uint32_t i = 0; i < pd.n_slices; i++) {
            SliceDesc &sd = g.h_slices[idx[i]];
            sd.fill_from = i == 0 ? 0 : sd.first_mb;
            sd.end_mb = i + 1 < pd.n_slices ? std::max(g.h_slices[idx[i + 1]].first_mb, sd.first_mb) : total;
        }
    dpb.cur_slot = s.cur_pic = -1;
}

static int scaling_set_for(h264mi_decoder *d, const h264mi_pps &p);
static int start_picture(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_pps &pps, uint32_t pps_id, const h264mi_slice_header &sh, int type, bool second);

// Error concealment of a lone field (H264MI_CONCEAL_LONE_FIELDS; the rule: include/h264mi.h).  The frame in Dpb::pend_slot holds one field F and the
// other one is not coming: the field F' of the opposite parity is put in front of whatever revealed that (`next`: the picture, with the parameter
// sets it is decoded under; nullptr: an end-of-sequence / end-of-stream unit) as a picture WITHOUT SLICES -- the second field of F's frame, a picture
// of the batch like any other (PicDesc, records, PicOrderCnt, marking), all of whose macroblocks k_conceal writes as P_Skip copies of
// PicDesc::conceal_ref: entry 0 of the initial P list for fields built for F' (the field of F''s parity of the nearest reference frame that has one;
// F itself when there is none).  The header made up here is what the repaired stream's slices of F' say, as far as picture management looks.  Returns H264MI_OK (inserted: the frame went out
// complete), 1 (not concealable: the caller paints the rows grey as without the bit) or an error.
static int conceal_lone_field(h264mi_decoder *d, int si, const h264mi_sps *nsps, const h264mi_pps *npps, const h264mi_slice_header *next) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    // the parameter sets F was decoded under must still be the ones the stream stores
    if (s.pend_stale || s.pend_sps_id < 0 || s.pend_pps_id < 0 || !s.sps_ok[s.pend_sps_id] || !s.pps_ok[s.pend_pps_id] || s.pps[s.pend_pps_id].sps_id != s.pend_sps_id) return 1;
    const h264mi_sps &sps = s.sps[s.pend_sps_id];
    const h264mi_pps &pps = s.pps[s.pend_pps_id];
    const h264mi_slice_header &fh = s.dpb.first_sh; // F's first slice: F is the picture that was completed last
    const Slot &fs = s.dpb.slots[s.dpb.pend_slot];
    if (!fh.field_pic || fs.fields != (fh.bottom_field ? 2 : 1) || fs.frame_num != fh.frame_num) return 1;
    if (pps.entropy_coding_mode && !d->cfg.allow_unpinned_field_cabac) return 1;
    const int parity = fh.bottom_field ? 1 : 2; // of F' (Dpb::cur_field: 1 top, 2 bottom)
    const int ref0 = s.dpb.second_field_p_entry0(sps, fs.frame_num, parity);
    if (ref0 < 0 || s.dpb.slots[MI_REF_SLOT(ref0)].nonexisting) return 1;
    // F' -- and the revealing picture, which has to fit with the bit set wherever it fits with the bit clear -- in what the batch has left
    // (with H264MI_CONCEAL_PICTURES the revealing picture may open a frame_num gap as well: the frames conceal_frame_num_gap would insert with this bit
    // clear must still fit with it set, or the inserted field would turn a concealed gap into a refused stream)
    int gap = 0;
    if (next && d->conceal_pics && next->nal_unit_type != 5 && !nsps->gaps_in_frame_num_value_allowed) {
        const int max_fn = 1 << (nsps->log2_max_frame_num_minus4 + 4);
        const int prev_ref = fh.nal_ref_idc ? fs.frame_num : s.dpb.prev_ref_frame_num; // PrevRefFrameNum once F' is through
        if (next->frame_num != prev_ref) gap = (next->frame_num - (prev_ref + 1) % max_fn + max_fn) % max_fn;
        if (gap > H264MI_CONCEAL_MAX_GAP) gap = 0; // (not concealed either way)
    }
    const int need = (next ? 2 : 1) + gap;
    const uint64_t field_mbs = static_cast<uint64_t>(sps.pic_width_in_mbs) * (sps.pic_height_in_mbs / 2);
    const uint64_t next_mbs = next ? static_cast<uint64_t>(nsps->pic_width_in_mbs) * (next->field_pic ? nsps->pic_height_in_mbs / 2 : nsps->pic_height_in_mbs) : 0;
    if (s.n_pics_in_batch + need > d->cfg.max_frames_per_batch || g.n_pics + need > d->pics_cap) return 1;
    const uint64_t gap_mbs = gap ? static_cast<uint64_t>(gap) * nsps->pic_width_in_mbs * nsps->pic_height_in_mbs : 0;
    if (g.mb_used + field_mbs + next_mbs + gap_mbs > d->mb_cap) return 1;
    size_t cursor = g.map_cursor; // every picture's slice group map goes into the staging buffer (start_picture)
    for (int k = 0; k < need; k++) // F', the revealing picture, the frames of its gap
        if ((k ? npps : &pps)->num_slice_groups_minus1 > 0) {
            const size_t moff = (cursor + 15) & ~static_cast<size_t>(15), n_mbs = static_cast<size_t>(k == 0 ? field_mbs : (k == 1 ? next_mbs : gap_mbs / gap));
            if (moff + n_mbs + 4096 > d->bits_cap) return 1;
            cursor = moff + n_mbs;
        }
    if (scaling_set_for(d, pps) < 0) return 1;
    h264mi_slice_header f;
    memset(&f, 0, sizeof(f));
    f.pps_id = s.pend_pps_id, f.frame_num = fs.frame_num, f.nal_ref_idc = fh.nal_ref_idc, f.nal_unit_type = 1;
    f.field_pic = 1, f.bottom_field = fh.bottom_field ? 0 : 1;
    f.slice_group_change_cycle = fh.slice_group_change_cycle;
    if (sps.pic_order_count_type == 0) f.pic_order_cnt_lsb = (fh.pic_order_cnt_lsb + 1) % (1 << (sps.log2_max_pic_order_cnt_lsb_min4 + 4));
    f.num_ref_idx_active_override = 1;
    f.slice_qp_y = 26 + pps.pic_init_qp_minus26;
    const int drops = s.pending_drops; // slices with an unreadable header in front of the revealing picture belong to IT, not to the inserted field
    s.pending_drops = 0;
    int r = start_picture(d, si, sps, pps, static_cast<uint32_t>(s.pend_pps_id), f, 1, true);
    if (r == H264MI_OK && g.h_pics[s.cur_pic].conceal_ref != ref0) { // (cannot happen: the same list was built above)
        set_error("stream %d: the field inserted for a lone field has no reference", si);
        r = H264MI_EBITSTREAM;
    }
    if (r == H264MI_OK) finish_picture(d, si); // (both fields are through: the frame goes out there)
    s.pending_drops = drops;
    return r;
}

// A first field whose second field did not come: the frame goes out with one field decoded, the rows of the other parity painted mid-grey
// (at the start of the batch's reconstruction: whatever the slot held before must not show) -- or, with H264MI_CONCEAL_LONE_FIELDS and where
// that is possible, complete: conceal_lone_field.  `next`: the picture that follows, nullptr: none (an end-of-sequence / end-of-stream unit).
static int flush_pending_field(h264mi_decoder *d, int si, const h264mi_sps *nsps = nullptr, const h264mi_pps *npps = nullptr, const h264mi_slice_header *next = nullptr) {
    StreamState &s = d->st[si];
    if (s.dpb.pend_slot < 0) return H264MI_OK;
    if (d->conceal_lone) {
        const int r = conceal_lone_field(d, si, nsps, npps, next);
        if (r != 1) return r;
    }
    Stage &g = d->stage[d->prep];
    const Slot &f = s.dpb.slots[s.dpb.pend_slot];
    OutFrame o = s.pend_out;
    o.poc = f.poc;
    o.first_parity = f.fields == 1 ? 0 : 1; // the field there is; the missing one is reported with the same count
    o.top_foc = o.bottom_foc = f.fpoc[o.first_parity];
    g.out[si].push_back(o);
    g.grey.push_back({static_cast<uint32_t>(si), static_cast<uint32_t>(s.dpb.pend_slot), f.fields == 1 ? 1u : 0u, static_cast<uint32_t>(o.wmb * 16), static_cast<uint32_t>(o.hmb * 16)});
    s.dpb.pend_slot = -1;
    return H264MI_OK;
}

extern "C" int32_t h264mi_slice_starts_picture(const h264mi_sps *sps, const h264mi_slice_header *prev, const h264mi_slice_header *cur) {
    if (!sps || !prev || !cur) return H264MI_EINVAL;
    return new_picture(*sps, *prev, *cur) ? 1 : 0;
}

static int scaling_set_for(h264mi_decoder *d, const h264mi_pps &p) {
    ScalingSet tmp;
    build_scaling(p.scaling_list_4x4, p.scaling_list_8x8, &tmp);
    uint32_t &mine = d->scaling_used[d->prep];
    for (int i = 0; i < d->n_scaling; i++)
        if (!memcmp(&d->h_tables->scaling[i], &tmp, sizeof(tmp))) {
            mine |= 1u << i;
            return i;
        }
    // a new matrix: the next free entry, or one that only batches which have finished referred to (the batch of the other staging set
    // may still be executing: its entries stay as they are -- the upload rewrites them with the bytes they hold)
    int at = d->n_scaling < MI_MAX_SCALING_SETS ? d->n_scaling : -1;
    if (at < 0) {
        uint32_t busy = 0;
        for (int st = 0; st < MI_STAGES; st++) busy |= d->scaling_used[st];
        for (int i = 0; i < MI_MAX_SCALING_SETS && at < 0; i++)
            if (!(busy >> i & 1)) at = i;
        if (at < 0) return -1;
    } else
        d->n_scaling++;
    d->h_tables->scaling[at] = tmp;
    d->tables_dirty = true;
    mine |= 1u << at;
    return at;
}

// 8.2.5.2 decoding process for gaps in frame_num (h264/sps.go:311-312 parses the flag, nothing in the reference uses it): a
// non-IDR picture whose frame_num is neither PrevRefFrameNum nor its successor says that reference frames are missing.  With
// gaps_in_frame_num_value_allowed_flag every skipped value becomes a "non-existing" short-term frame that goes through the
// sliding window like a decoded one -- it pushes older frames out and takes its place in the initial lists, so that the
// indices of the surviving pictures come out as the encoder meant them.  Without the flag pictures were lost: the stream is
// refused (H264MI_EBITSTREAM; with isolation it alone leaves the batch and waits for its next IDR picture) rather than
// predicted from the wrong pictures.
static int fill_frame_num_gap(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_slice_header &sh) {
    Dpb &dpb = d->st[si].dpb;
    const int m = dpb.missing_frames(sps, sh), max_fn = 1 << (sps.log2_max_frame_num_minus4 + 4);
    if (!m) return H264MI_OK;
    if (!sps.gaps_in_frame_num_value_allowed) {
        set_error("stream %d: frame_num %d after %d: reference pictures are missing", si, sh.frame_num, dpb.prev_ref_frame_num);
        return H264MI_EBITSTREAM;
    }
    for (int k = 0; k < m; k++)
        if (!dpb.add_nonexisting_frame(sps, (dpb.prev_ref_frame_num + 1) % max_fn)) {
            set_error("stream %d: frame pool exhausted", si);
            return H264MI_ECAPACITY;
        }
    return H264MI_OK;
}

// Per level of a batch: which k_dbprep kernel runs on the pictures complete with it (mi_dbprep_kernel_choice), from what their descriptors say now
static void choose_dbprep_kernels(Stage &g) {
    g.prep_kernel.assign(g.prep_n.size(), MI_DBPREP_K_GENERIC);
    for (size_t l = 0; l < g.prep_n.size(); l++) {
        int n_has_b = 0, n_save_col = 0;
        for (uint32_t i = 0; i < g.prep_n[l]; i++) {
            const PicDesc &pd = g.h_pics[g.h_lists[g.prep_off[l] + i]];
            n_has_b += pd.has_b != 0, n_save_col += pd.save_col != 0;
        }
        g.prep_kernel[l] = mi_dbprep_kernel_choice(n_has_b, n_save_col);
#if defined(H264MI_TEST_HOOKS) /* measurement: the general kernel everywhere, as before there was a kernel for I / P launches */
        if (const char *e = getenv("H264MI_DBPREP_GENERIC"))
            if (atoi(e)) g.prep_kernel[l] = MI_DBPREP_K_GENERIC;
#endif
    }
}

// What only B pictures need exists once the first B slice has been seen: the list-1 vector arrays (64 bytes per macroblock and
// buffer set) and the ColRec arrays (80 bytes per macroblock and frame slot: the motion direct prediction reads).  Reference
// pictures decoded BEFORE that moment have left no ColRec; the ones of the batch before this one -- where RefPicList1[0] of a
// stream's first B picture can still come from -- are filled in now from that batch's records, which are still resident
// (MI_STAGES staging sets, MI_SETS record sets).  Older ones cannot be: direct prediction from them sees an intra picture.
static int ensure_b_buffers(h264mi_decoder *d) {
    for (int i = 0; i < MI_SETS; i++)
        if (!d->d_mv1[i]) {
            hipError_t e = hipMalloc(&d->d_mv1[i], sizeof(MbMv1) * d->mb_cap);
            if (e != hipSuccess) {
                set_error("hipMalloc of the list-1 vector array failed: %s", hipGetErrorString(e));
                return e == hipErrorOutOfMemory ? H264MI_ENOMEM : H264MI_EDEVICE;
            }
            d->dev_bytes += sizeof(MbMv1) * d->mb_cap;
        }
    if (d->d_colrec) return H264MI_OK;
    // allocate, initialise, and only then publish: a failure half-way must not leave an array behind that the next call takes for ready
    const size_t S = d->st.size(), bytes = sizeof(ColRec) * d->colrec_per_slot * d->n_slots * S;
    ColRec *colrec = nullptr;
    uint32_t *backfill = nullptr;
    hipError_t e = hipMalloc(&colrec, bytes);
    if (e == hipSuccess) e = hipMalloc(&backfill, sizeof(uint32_t) * d->pics_cap);
    hipStream_t up = d->ent_stream[d->pass & 1];
    if (e == hipSuccess) e = hipMemsetAsync(colrec, 0xFF, bytes, up); // refslot / ref -1 everywhere: "intra" (never read: Slot::col_valid guards every use)
    if (e != hipSuccess) {
        if (colrec) hipFree(colrec);
        if (backfill) hipFree(backfill);
        set_error("setting up the co-located motion arrays failed: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? H264MI_ENOMEM : H264MI_EDEVICE;
    }
    d->d_colrec = colrec, d->d_backfill = backfill;
    d->dev_bytes += bytes + sizeof(uint32_t) * d->pics_cap;
    // The reference pictures of the batch executed last -- where RefPicList1[0] of a stream's first B picture can still come from -- get their
    // ColRec arrays now, from that batch's records: only if that batch is the one prepared before this one, its record set is known, and it has
    // FINISHED (its descriptor table is rewritten here; a pass still in flight would read it).  Anything older stays without (col_valid).
    Stage &pv = d->stage[(d->prep + MI_STAGES - 1) % MI_STAGES];
    if (MI_STAGES > 1 && pv.executed && d->pass > 0 && d->last_exec_stage == (d->prep + MI_STAGES - 1) % MI_STAGES) {
        HIP_TRY(hipEventSynchronize(pv.ev_done)); // once per decoder
        std::vector<uint32_t> list;
        auto want = [&](size_t si, const OutFrame &o, int pic, int par) {
            if (pic < 0 || pic >= pv.n_pics) return;
            Slot &sl = d->st[si].dpb.slots[o.slot];
            pv.h_pics[pic].save_col = 1;
            pv.h_pics[pic].col_out = reinterpret_cast<uint64_t>(d->d_colrec + (si * d->n_slots + o.slot) * d->colrec_per_slot + (par ? d->colrec_per_slot / 2 : 0));
            sl.col_valid[par] = true;
            list.push_back(static_cast<uint32_t>(pic));
        };
        for (size_t si = 0; si < S; si++)
            for (const OutFrame &o : pv.out[si])
                if (d->st[si].dpb.slots[o.slot].ref) { // still a reference picture: a B picture may point at it
                    for (int pic : {o.pic, o.pic2})
                        if (pic >= 0 && pic < pv.n_pics) want(si, o, pic, pv.h_pics[pic].field == 2 ? 1 : 0);
                }
        if (!list.empty()) {
            const int pset = d->last_exec_set;
            choose_dbprep_kernels(pv); // (that batch executed again writes these ColRec arrays itself: its pictures are flagged save_col now)
            HIP_TRY(hipMemcpyAsync(pv.d_pics, pv.h_pics, sizeof(PicDesc) * pv.n_pics, hipMemcpyHostToDevice, up));
            HIP_TRY(hipMemcpyAsync(d->d_backfill, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice, up));
            HIP_TRY(hipStreamSynchronize(up)); // (`list` is pageable host memory; once per decoder)
            hipLaunchKernelGGL(k_dbprep, dim3((pv.mbs_max + MI_DBPREP_MBS - 1) / MI_DBPREP_MBS, (static_cast<uint32_t>(list.size()) + 7u) & ~7u), dim3(256), 0, up, d->d_backfill,
                               pv.d_pics, d->d_tables, d->d_mbrec[pset], d->d_mv1[pset], d->d_dbprm[pset], 1, d->d_imask[pset], static_cast<int>(list.size()));
        }
    }
    return H264MI_OK;
}

// The pictures of this batch that live in the frame slot a list entry names (a frame, or either field: whichever of them this batch decodes) have to
// be reconstructed (deblocked) before picture `pic`, which predicts from it: Stage::pic_wave
static void wave_after(Stage &g, const Dpb &dpb, int pic, int entry) {
    if (entry < 0) return;
    const Slot &rs = dpb.slots[MI_REF_SLOT(entry)]; // (frame pictures never set the parity bit)
    for (int p : {rs.pic, rs.fpic[0], rs.fpic[1]})
        if (p >= 0 && p != pic && p < static_cast<int>(g.pic_wave.size())) g.pic_wave[pic] = std::max(g.pic_wave[pic], g.pic_wave[p] + 1);
}

// PicOrderCnt of a reference list entry: a field's own count in a field picture (entries name fields: slot | MI_REF_PARITY), the frame's otherwise
static int list_entry_poc(const Dpb &dpb, int e, bool fieldpic) {
    return fieldpic ? dpb.slots[MI_REF_SLOT(e)].fpoc[(e & MI_REF_PARITY) ? 1 : 0] : dpb.slots[e].poc;
}

// The first slice of a new picture (`sh`, of NAL unit type `type`; second: the second field of the frame in Dpb::pend_slot): its frame slot, its place
// in the batch's tables, its PicDesc and the frame it goes out as.  The picture is then under construction (Dpb::cur_slot, StreamState::cur_*) until finish_picture.
static int start_picture(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_pps &pps, uint32_t pps_id, const h264mi_slice_header &sh, int type, bool second) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    const int wmb = sps.pic_width_in_mbs, hmb = sps.pic_height_in_mbs, hmb_pic = sh.field_pic ? hmb / 2 : hmb;
    // (a field counts as a picture of its own against max_frames_per_batch: include/h264mi.h)
    if (s.n_pics_in_batch >= d->cfg.max_frames_per_batch || g.n_pics >= d->pics_cap) {
        set_error("stream %d: more than %d pictures in one batch", si, d->cfg.max_frames_per_batch);
        return H264MI_ECAPACITY;
    }
    int r, slot = second ? s.dpb.pend_slot : s.dpb.first_free_slot();
    if (slot < 0) {
        set_error("stream %d: frame pool exhausted", si);
        return H264MI_ECAPACITY;
    }
    if (g.mb_used + static_cast<uint64_t>(wmb) * hmb_pic > d->mb_cap) {
        set_error("macroblock record pool exhausted");
        return H264MI_ECAPACITY;
    }
    // Error concealment of an IDR frame picture (H264MI_CONCEAL_IDR; the rule: include/h264mi.h): its concealment reference is entry 0 of the initial P
    // list of a frame picture with frame_num (PrevRefFrameNum + 1) mod MaxFrameNum -- what the picture predicts from in the repaired stream, where it is
    // a non-IDR picture that ends in memory management operation 5 --, looked up now: before the picture takes its slot and long before its marking
    // drops the references (Dpb::finish_picture).  The slot named stays put for the batch: it is held, or a picture of this batch.  The references
    // must have been decoded under an SPS this picture could still predict under (MaxFrameNum: the previous sequence's, which is then this one's).
    StreamState::RefSeq seq;
    seq.wmb = wmb, seq.hmb = hmb, seq.chroma_format = sps.chroma_format, seq.frame_mbs_only = sps.frame_mbs_only, seq.log2_max_frame_num_minus4 = sps.log2_max_frame_num_minus4;
    int idr_ref = -1;
    if (d->conceal_idr && type == 5 && !sh.field_pic && !second && seq == s.ref_seq) {
        const int best = s.dpb.initial_p_entry0(sps, (s.dpb.prev_ref_frame_num + 1) % (1 << (sps.log2_max_frame_num_minus4 + 4)), 0);
        if (best >= 0 && !s.dpb.slots[best].nonexisting) idr_ref = best;
    }
    s.ref_seq = seq;
    s.cur_pic = g.n_pics++;
    s.cur_slices = 0;
    s.cur_first_mbs.clear();
    s.dpb.begin_picture(sps, sh, slot, second, s.cur_pic);
    const Slot &sl = s.dpb.slots[slot];
    PicDesc &pd = g.h_pics[s.cur_pic];
    memset(&pd, 0, sizeof(pd));
    pd.stream = si, pd.slot = slot, pd.wmb = wmb, pd.hmb = hmb_pic;
    // where the picture lives in its frame slot: a field picture in the rows of its parity (PicDesc)
    pd.field = static_cast<uint8_t>(s.dpb.cur_field);
    pd.pitch = static_cast<uint32_t>(wmb * 16 * (sh.field_pic ? 2 : 1)), pd.plane = static_cast<uint32_t>(wmb * 16) * static_cast<uint32_t>(hmb * 16);
    pd.inv_wmb = wmb > 1 ? static_cast<uint32_t>((1ull << 32) / static_cast<uint32_t>(wmb)) + 1u : 0u; // (one macroblock column: mi_types.h)
    pd.pool_base = d->h_pools[si].base, pd.slot_bytes = d->slot_bytes, pd.n_slots = static_cast<uint32_t>(d->n_slots);
    g.pic_level.resize(g.n_pics, 0), g.pic_save_col.resize(g.n_pics, 0), g.pic_wave.resize(g.n_pics, 0), g.pic_init_qp.resize(g.n_pics, 26);
    g.pic_dropped.resize(g.n_pics, 0), g.pic_dropped[s.cur_pic] = 0;
    g.pic_level[s.cur_pic] = 0, g.pic_save_col[s.cur_pic] = 0, g.pic_wave[s.cur_pic] = 0;
    g.pic_init_qp[s.cur_pic] = static_cast<uint8_t>(std::min(std::max(26 + pps.pic_init_qp_minus26, 0), 51));
    pd.conceal_ref = -1;
    if (d->conceal && type != 5 && (!sh.field_pic || d->conceal_fields)) {
        // Error concealment: the picture is concealable when the initial P list, built for THIS picture whatever the types of its slices, is not
        // empty; its entry 0 is what lost macroblocks are copied from.  A field picture's (H264MI_CONCEAL_FIELDS) is a field -- the first field of the
        // same frame, if this is its second field and that one is a short-term reference --, written like every entry of a field list as
        // slot | parity (MI_REF_PARITY).  (A frame inferred by the frame_num gap process holds no samples: not concealable.)
        const int best = s.dpb.initial_p_entry0(sps, sh.frame_num, s.dpb.cur_field);
        if (best >= 0 && !s.dpb.slots[MI_REF_SLOT(best)].nonexisting) {
            pd.conceal_ref = static_cast<int16_t>(best);
            // ... and the picture is reconstructed behind it when this batch decodes it: a non-IDR I picture would otherwise be in wave 0, and the
            // MODIFIED lists of a P picture's slices need not hold this entry
            wave_after(g, s.dpb, s.cur_pic, best);
        }
    }
    if (idr_ref >= 0) { // ... and like a non-IDR I picture that is concealable, the IDR picture is reconstructed behind its concealment reference, damaged or not
        pd.conceal_ref = static_cast<int16_t>(idr_ref);
        wave_after(g, s.dpb, s.cur_pic, idr_ref);
    }
    // K11: the picture order counts of the picture and of its concealment reference as they are NOW (the slot named may be another picture's by the end
    // of the batch, and operation 5 rewrites this picture's): what the concealment pseudo-slice reports (h264mi_frame_ref_pocs, slice -1)
    g.pic_conceal_poc.resize(g.n_pics);
    g.pic_conceal_poc[s.cur_pic] = {sh.field_pic ? sl.fpoc[sh.bottom_field ? 1 : 0] : sl.poc, pd.conceal_ref >= 0 ? list_entry_poc(s.dpb, pd.conceal_ref, sh.field_pic != 0) : 0};
    if (s.pending_drops) { // slices without a readable header in front of this picture's first good one: lost slices of it, if it can be concealed
        const int n = s.pending_drops, e = s.pending_drop_err;
        s.pending_drops = 0;
        if (pd.conceal_ref < 0 || s.pending_drop_type != (type == 5 ? 5 : 1)) { // (a dropped unit of the other kind was no slice of this picture)
            set_error("stream %d: a slice header does not parse, in a picture that cannot be concealed", si);
            return e;
        }
        g.pic_dropped[s.cur_pic] = static_cast<uint16_t>(std::min(n, 65535));
    }
    pd.mb_base = g.mb_used;
    g.mb_used += static_cast<uint64_t>(wmb) * hmb_pic;
    pd.first_slice = g.n_slices;
    pd.cabac = pps.entropy_coding_mode, pd.t8x8_mode = pps.transform_8x8_mode, pd.cip = pps.constrained_intra_pred;
    pd.mono = sps.chroma_format == 0;
    pd.weighted_pred = pps.weighted_pred;
    pd.cqp_off[0] = static_cast<int8_t>(pps.chroma_qp_index_offset), pd.cqp_off[1] = static_cast<int8_t>(pps.second_chroma_qp_index_offset);
    pd.is_intra_only = 1;
    int ss = scaling_set_for(d, pps);
    if (ss < 0) {
        set_error("more than %d distinct scaling matrices in flight", MI_MAX_SCALING_SETS);
        return H264MI_ECAPACITY;
    }
    pd.scaling_set = static_cast<uint8_t>(ss);
    pd.order = s.n_pics_in_batch++;
    if (pps.num_slice_groups_minus1 > 0) { // FMO: this picture's macroblock-to-slice-group map travels with the bitstream (8.2.2; h264/slice.go:134-158)
        const size_t n_mbs = static_cast<size_t>(wmb) * hmb_pic, moff = (g.map_cursor + 15) & ~static_cast<size_t>(15);
        if (moff + n_mbs + 4096 > d->bits_cap) {
            set_error("bitstream staging buffer too small for the slice group maps (%zu bytes)", d->bits_cap);
            return H264MI_ECAPACITY;
        }
        r = mb_to_slice_group_map(&sps, &pps, s.sg_ids[pps_id].data(), s.sg_ids[pps_id].size(), sh.slice_group_change_cycle, sh.field_pic ? 1 : 0, g.h_bits + moff, n_mbs, nullptr);
        if (r != H264MI_OK) return r;
        pd.fmo = 1, pd.sgmap_off = static_cast<uint32_t>(moff);
        g.map_cursor = moff + n_mbs;
        g.bits_end = std::max(g.bits_end, g.map_cursor);
    }
    if (!second) { // the frame this picture belongs to, as it will be shown: pushed now (frame picture), or when its fields are through (finish_picture / flush_pending_field)
        OutFrame of{slot, wmb, hmb, crop_unit_x(&sps) * sps.frame_crop_left_offset, crop_unit_y(&sps) * sps.frame_crop_top_offset, sps.width, sps.height, sl.poc, sh.frame_num,
                    sh.nal_ref_idc, sh.nal_unit_type == 5, s.cur_pic, sh.nal_unit_type == 5};
        if (sh.nal_ref_idc && sh.adaptive_ref_pic_marking_mode_flag)
            for (int k = 0; k < sh.n_memory_management_control_operations; k++)
                if (sh.memory_management_control_operation[k] == 5) of.new_sequence = 1;
        // (a frame picture: both counts are known now; a frame of two fields gets them when it goes out: finish_picture / flush_pending_field)
        of.field_coded = sh.field_pic != 0, of.top_foc = sl.fpoc[0], of.bottom_foc = sl.fpoc[1], of.first_parity = !sh.field_pic && sl.fpoc[1] < sl.fpoc[0];
        if (sps.vui_parameters_present && sps.video_signal_type_present) {
            of.video_full_range = sps.video_full_range;
            if (sps.color_description_present) of.matrix_coefficients = sps.matrix_coefficients;
        }
        if (sh.field_pic)
            s.pend_out = of, s.pend_sps_id = pps.sps_id, s.pend_pps_id = static_cast<int>(pps_id), s.pend_stale = false;
        else
            g.out[si].push_back(of);
    }
    g.wmb_max = std::max(g.wmb_max, wmb);
    g.hmb_max = std::max(g.hmb_max, hmb_pic);
    g.mbs_max = std::max(g.mbs_max, wmb * hmb_pic);
    g.info.n_macroblocks += static_cast<int64_t>(wmb) * hmb_pic;
    if (si == 0) g.info.width = sps.width, g.info.height = sps.height, g.info.coded_width = wmb * 16, g.info.coded_height = hmb * 16;
    return H264MI_OK;
}

// Error concealment of wholly lost reference frames (H264MI_CONCEAL_PICTURES; the rule: include/h264mi.h).  `sh` is the first slice of a picture that is
// not the second field of the frame before it.  Where fill_frame_num_gap would refuse the stream -- frame_num skips values and the SPS does not allow
// gaps -- and the gap is concealable, one frame picture WITHOUT SLICES per missing frame_num is put in front of the revealing picture: a picture of the
// batch like any other (slot, PicDesc, records, output frame, POC, sliding window), all of whose macroblocks k_conceal writes as P_Skip copies of
// PicDesc::conceal_ref -- which of the second inserted picture on is the inserted picture before it.  Returns H264MI_OK (inserted), 1 (no gap, or not
// concealable: the caller goes on as without the bit) or an error.
static int conceal_frame_num_gap(h264mi_decoder *d, int si, const h264mi_sps &sps, const h264mi_pps &pps, uint32_t pps_id, const h264mi_slice_header &sh) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    const int m = s.dpb.missing_frames(sps, sh);
    if (!m || sps.gaps_in_frame_num_value_allowed || m > H264MI_CONCEAL_MAX_GAP) return 1;
    const int max_fn = 1 << (sps.log2_max_frame_num_minus4 + 4), first = (s.dpb.prev_ref_frame_num + 1) % max_fn;
    const int ref0 = s.dpb.initial_p_entry0(sps, first, 0);
    if (ref0 < 0 || s.dpb.slots[ref0].nonexisting) return 1;
    // the m pictures and the revealing one must fit into what the batch has left (a slot taken by a picture of this batch stays taken until the next
    // prepare, so counting the free ones now is exact)
    const uint64_t frame_mbs = static_cast<uint64_t>(sps.pic_width_in_mbs) * sps.pic_height_in_mbs;
    if (s.n_pics_in_batch + m + 1 > d->cfg.max_frames_per_batch || g.n_pics + m + 1 > d->pics_cap || s.dpb.free_slots() < m + 1) return 1;
    if (g.mb_used + frame_mbs * m + (sh.field_pic ? frame_mbs / 2 : frame_mbs) > d->mb_cap) return 1;
    if (pps.num_slice_groups_minus1 > 0) { // every picture's slice group map goes into the staging buffer (start_picture)
        size_t cursor = g.map_cursor;
        for (int k = 0; k <= m; k++) {
            const size_t moff = (cursor + 15) & ~static_cast<size_t>(15);
            if (moff + frame_mbs + 4096 > d->bits_cap) return 1;
            cursor = moff + frame_mbs;
        }
    }
    if (scaling_set_for(d, pps) < 0) return 1;
    const int drops = s.pending_drops; // slices with an unreadable header in front of `sh` belong to ITS picture, not to an inserted one
    s.pending_drops = 0;
    for (int k = 0; k < m; k++) {
        h264mi_slice_header f; // what the repaired stream's slices of this frame say, as far as picture management looks
        memset(&f, 0, sizeof(f));
        f.pps_id = static_cast<int32_t>(pps_id), f.frame_num = (first + k) % max_fn, f.nal_ref_idc = 1, f.nal_unit_type = 1;
        f.slice_group_change_cycle = sh.slice_group_change_cycle;
        if (sps.pic_order_count_type == 0) f.pic_order_cnt_lsb = (s.dpb.prev_poc_lsb + 2) % (1 << (sps.log2_max_pic_order_cnt_lsb_min4 + 4));
        f.num_ref_idx_active_override = 1;
        f.slice_qp_y = 26 + pps.pic_init_qp_minus26;
        int r = start_picture(d, si, sps, pps, pps_id, f, 1, false);
        if (r != H264MI_OK) return r;
        if (g.h_pics[s.cur_pic].conceal_ref < 0) { // (cannot happen: entry 0 was looked up above, and from then on it is the picture inserted before)
            set_error("stream %d: frame_num %d after %d: reference pictures are missing", si, sh.frame_num, s.dpb.prev_ref_frame_num);
            return H264MI_EBITSTREAM;
        }
        finish_picture(d, si);
    }
    s.pending_drops = drops;
    return H264MI_OK;
}

// one slice NAL of stream `si`
// `off` / `rlen`: where batch_prepare's parallel pass put the slice's RBSP in the pinned staging buffer (16-byte aligned)
static int add_slice(h264mi_decoder *d, int si, size_t off, size_t rlen, int ref_idc, int type) {
    StreamState &s = d->st[si];
    Stage &g = d->stage[d->prep];
    if (g.n_slices >= d->slices_cap) {
        set_error("more than %d slices in the batch", d->slices_cap);
        return H264MI_ECAPACITY;
    }
    uint8_t *rbsp = g.h_bits + off;
    // peek pps id: first_mb_in_slice, slice_type, pic_parameter_set_id
    BitReader br(rbsp, rlen);
    br.ue();
    br.ue();
    uint32_t pps_id = br.ue();
    if (pps_id > 255 || !s.pps_ok[pps_id]) {
        set_error("stream %d: slice refers to missing PPS %u", si, pps_id);
        return H264MI_EBITSTREAM;
    }
    const h264mi_pps &pps = s.pps[pps_id];
    if (!s.sps_ok[pps.sps_id]) {
        set_error("stream %d: PPS %u refers to missing SPS %d", si, pps_id, pps.sps_id);
        return H264MI_EBITSTREAM;
    }
    const h264mi_sps &sps = s.sps[pps.sps_id];
    h264mi_slice_header sh;
    int r = parse_slice_header(&sps, &pps, ref_idc, type, rbsp, rlen, &sh);
    if (r != H264MI_OK) {
        // error concealment: a damaged slice header is a lost slice -- its macroblocks stay undelivered and k_conceal fills them in -- but only in a
        // picture that is concealable; anywhere else it fails the stream as without the mode.  Which picture a slice without a header belongs to is not
        // known: it is taken for a slice of the picture under construction if that one is of its kind -- a unit of type 1: a non-IDR picture, a unit of
        // type 5 (tolerated with H264MI_CONCEAL_IDR only): an IDR picture --, else, or if there is none, of the picture the next slice starts (decided there).
        if (d->conceal && (type == 1 || (type == 5 && d->conceal_idr)) && !s.need_idr && (r == H264MI_EBITSTREAM || r == H264MI_EINVAL)) {
            if (s.dpb.cur_slot < 0 || (s.dpb.first_sh.nal_unit_type == 5) != (type == 5)) {
                s.pending_drop_type = s.pending_drops && s.pending_drop_type != type ? -1 : type;
                s.pending_drops++, s.pending_drop_err = r;
                return H264MI_OK;
            }
            if (g.h_pics[s.cur_pic].conceal_ref >= 0) {
                g.pic_dropped[s.cur_pic]++;
                return H264MI_OK;
            }
        }
        return r;
    }
    if (sh.redundant_pic_cnt > 0) return H264MI_OK; // redundant pictures are dropped
    if (s.need_idr) { // after an error nothing can be trusted before the next IDR picture
        if (type != 5) return H264MI_OK;
        s.need_idr = false;
    }
    const int st = sh.slice_type % 5;
    if (st > 2) {
        set_error("stream %d: slice_type %d is out of scope (SP / SI slices)", si, sh.slice_type);
        return H264MI_EUNSUPPORTED;
    }
    // chroma_format_idc 0 (monochrome; h264/sps.go:226-243 ChromaFormat, h264/slice.go:179-219 SubWidthC / SubHeightC): the entropy kernels leave out the
    // chroma syntax (PicDesc::mono), and nothing else changes -- the frame pool starts out at 128, intra chroma prediction is the DC of planes that are
    // 128 everywhere, inter prediction copies 128, the residual is zero and the filters leave constants alone: the chroma planes a 4:2:0 display expects
    if (sps.chroma_format > 1 || sps.bit_depth_luma_minus8 || sps.bit_depth_chroma_minus8 || sps.qprime_y_zero_transform_bypass) {
        set_error("stream %d: only 4:2:0 and monochrome 8-bit streams are supported (chroma_format_idc %d; 4:2:2 / 4:4:4 and more than 8 bits are out of scope)", si, sps.chroma_format);
        return H264MI_EUNSUPPORTED;
    }
    // frame_mbs_only_flag = 0 (h264/sps.go:316-322): the pictures are frames (decoded like progressive ones: map units are two macroblock rows
    // high, crop units double) or field pictures (h264/slice.go:867-872: field_pic_flag / bottom_field_flag; PAFF), in any mix.
    // Macroblock-adaptive frame/field coding (MBAFF, h264/slice.go:563-568, 624-634) is not implemented.
    if (!sps.frame_mbs_only && sps.mb_adaptive_frame_field) {
        set_error("stream %d: macroblock-adaptive frame/field coding (MBAFF) is out of scope", si);
        return H264MI_EUNSUPPORTED;
    }
    if (sh.field_pic) {
        if (pps.entropy_coding_mode && !d->cfg.allow_unpinned_field_cabac) {
            // ctxIdx 277..398 and 436..459 (significant_coeff_flag / last_significant_coeff_flag of field-coded blocks, Tables 9-19 .. 9-24): the values in
            // this library's tables were written down without the standard at hand and nothing on its build machine pins them (mi_cabac_mn.cpp) -- a
            // decoder with wrong tables produces plausible, wrong pictures, so it takes an explicit request (h264mi_config.allow_unpinned_field_cabac)
            set_error("stream %d: field pictures with CABAC are refused: the context initialisation values of field-coded blocks (ctxIdx 277-398, 436-459) in "
                      "this library's tables are unpinned (h264mi_config.allow_unpinned_field_cabac = 1 decodes with them); CAVLC field pictures are decoded", si);
            return H264MI_EUNSUPPORTED;
        }
        if (ref_idc && type != 5 && sh.adaptive_ref_pic_marking_mode_flag)
            for (int k = 0; k < sh.n_memory_management_control_operations; k++)
                if (sh.memory_management_control_operation[k] != 1) {
                    set_error("stream %d: memory_management_control_operation %d in a field picture is out of scope (operation 1 is implemented)", si,
                              sh.memory_management_control_operation[k]);
                    return H264MI_EUNSUPPORTED;
                }
    }
    if (sps.max_num_ref_frames > d->cfg.max_ref_frames) {
        set_error("stream %d: max_num_ref_frames %d exceeds the configured max_ref_frames %d", si, sps.max_num_ref_frames, d->cfg.max_ref_frames);
        return H264MI_ECAPACITY;
    }
    const int wmb = sps.pic_width_in_mbs, hmb = sps.pic_height_in_mbs; // of the frame
    const int hmb_pic = sh.field_pic ? hmb / 2 : hmb;                   // of this picture (h264/slice.go:159-176 PicHeightInMbs)
    if (wmb * 16 > d->Wmax || hmb * 16 > d->Hmax || hmb > 320) {
        set_error("stream %d: %dx%d exceeds the configured maximum %dx%d", si, wmb * 16, hmb * 16, d->Wmax, d->Hmax);
        return H264MI_ECAPACITY;
    }
    // (7.4.1.2.4 cannot tell two pictures apart whose headers agree -- e.g. POC type 2 and the frame_num 1 that follows a memory
    // management operation 5 in a picture with frame_num 1 --: a slice that starts where a slice of the current picture already
    // started begins a new picture whatever the headers say.  Not "first_mb_in_slice == 0": with slice groups or arbitrary slice
    // order that slice may come late.)
    const bool restarts = std::find(s.cur_first_mbs.begin(), s.cur_first_mbs.end(), sh.first_mb_in_slice) != s.cur_first_mbs.end();
    if (s.dpb.cur_slot >= 0 && (restarts || new_picture(sps, s.dpb.first_sh, sh))) finish_picture(d, si);
    if (s.active_sps != pps.sps_id || s.wmb != wmb || s.hmb != hmb) { // (re)activate: new sequence geometry
        if (sh.nal_unit_type != 5 && s.active_sps >= 0 && (s.wmb != wmb || s.hmb != hmb)) {
            set_error("stream %d: picture size changes without an IDR", si);
            return H264MI_EBITSTREAM;
        }
        r = flush_pending_field(d, si, &sps, &pps, &sh); // (a lone first field of the old sequence goes out before anything of the new one)
        if (r != H264MI_OK) return r;
        s.active_sps = pps.sps_id, s.wmb = wmb, s.hmb = hmb;
    }
    if (s.dpb.cur_slot < 0) { // first slice of a new picture
        // the second field of the frame whose first field was the previous picture (7.4.1.2.4, 3.30 / 3.31): opposite parity, same frame_num, not
        // an IDR picture, reference or not like the first one
        bool second = false;
        if (s.dpb.pend_slot >= 0) {
            const Slot &f = s.dpb.slots[s.dpb.pend_slot];
            if (sh.field_pic && type != 5 && f.fields == (sh.bottom_field ? 1 : 2) && f.frame_num == sh.frame_num && (f.ref != 0) == (ref_idc != 0))
                second = true;
            else if ((r = flush_pending_field(d, si, &sps, &pps, &sh)) != H264MI_OK)
                return r;
        }
        if (!second) {
            r = d->conceal_pics ? conceal_frame_num_gap(d, si, sps, pps, pps_id, sh) : 1;
            if (r == 1) r = fill_frame_num_gap(d, si, sps, sh);
            if (r != H264MI_OK) return r;
        }
        r = start_picture(d, si, sps, pps, pps_id, sh, type, second);
        if (r != H264MI_OK) return r;
    }
    if (s.cur_slices >= d->cfg.max_slices_per_frame) {
        set_error("stream %d: more than %d slices in a frame", si, d->cfg.max_slices_per_frame);
        return H264MI_ECAPACITY;
    }
    if (sh.first_mb_in_slice >= wmb * hmb_pic) return H264MI_EBITSTREAM;
    s.cur_first_mbs.push_back(sh.first_mb_in_slice);
    PicDesc &pd = g.h_pics[s.cur_pic];
    SliceDesc &sd = g.h_slices[g.n_slices];
    memset(&sd, 0, sizeof(sd));
    sd.rbsp_off = static_cast<uint32_t>(off), sd.rbsp_size = static_cast<uint32_t>(rlen);
    sd.data_bit_off = static_cast<uint32_t>(sh.slice_data_bit_offset);
    {
        size_t n = rlen;
        while (n > 0 && rbsp[n - 1] == 0) n--;
        sd.stop_bit = n ? static_cast<uint32_t>((n - 1) * 8 + 7 - __builtin_ctz(rbsp[n - 1])) : 0;
    }
    sd.pic_idx = s.cur_pic, sd.first_mb = sh.first_mb_in_slice;
    sd.slice_type = static_cast<uint8_t>(st);
    sd.cabac_init_idc = static_cast<uint8_t>(sh.cabac_init), sd.slice_qp = static_cast<uint8_t>(sh.slice_qp_y);
    sd.num_ref_idx_active = static_cast<uint8_t>(st != 2 ? sh.num_ref_idx_l0_active_minus1 + 1 : 0);
    sd.alpha_off = static_cast<int8_t>(2 * sh.slice_alpha_c0_offset_div2), sd.beta_off = static_cast<int8_t>(2 * sh.slice_beta_offset_div2);
    sd.dbf_idc = static_cast<uint8_t>(sh.disable_deblocking_filter);
    sd.slice_in_pic = static_cast<uint16_t>(s.cur_slices);
    for (int i = 0; i < MI_MAX_REFS; i++) sd.ref_slot[i] = -1;
    int level = 0;
    if (st != 2) {
        pd.is_intra_only = 0;
        const bool bslice = st == 1;
        const bool explicit_wp = bslice ? pps.weighted_bipred == 1 : pps.weighted_pred != 0;
        BSliceExt bx;
        memset(&bx, 0, sizeof(bx));
        r = s.dpb.build_ref_lists(sps, sh, bslice, sd.ref_slot, bx.ref_slot1);
        if (r != H264MI_OK) return r;
        for (int i = 0; i <= sh.num_ref_idx_l0_active_minus1 && i < MI_MAX_REFS; i++) wave_after(g, s.dpb, s.cur_pic, sd.ref_slot[i]);
        if (bslice)
            for (int i = 0; i <= sh.num_ref_idx_l1_active_minus1 && i < MI_MAX_REFS; i++) wave_after(g, s.dpb, s.cur_pic, bx.ref_slot1[i]);
        sd.wp_flag = static_cast<uint8_t>(explicit_wp);
        sd.luma_log2_denom = static_cast<uint8_t>(sh.luma_log2_weight_denom), sd.chroma_log2_denom = static_cast<uint8_t>(sh.chroma_log2_weight_denom);
        for (int i = 0; i < MI_MAX_REFS; i++) {
            sd.wp_lw[i] = static_cast<int16_t>(explicit_wp ? sh.luma_weight_l0[i] : 1), sd.wp_lo[i] = static_cast<int16_t>(sh.luma_offset_l0[i]);
            for (int j = 0; j < 2; j++)
                sd.wp_cw[i][j] = static_cast<int16_t>(explicit_wp ? sh.chroma_weight_l0[i][j] : 1), sd.wp_co[i][j] = static_cast<int16_t>(sh.chroma_offset_l0[i][j]);
        }
        if (bslice) {
            r = ensure_b_buffers(d);
            if (r != H264MI_OK) return r;
            pd.has_b = 1;
            // PicOrderCnt of the current picture and of a list entry: a field's own count in a field picture (entries name fields), the frame's otherwise
            const bool fieldpic = sh.field_pic != 0;
            const Slot &cur = s.dpb.slots[s.dpb.cur_slot];
            const int cur_poc = fieldpic ? cur.fpoc[sh.bottom_field ? 1 : 0] : cur.poc;
            auto entry_slot = [&](int e) -> const Slot & { return s.dpb.slots[fieldpic ? MI_REF_SLOT(e) : e]; };
            auto entry_poc = [&](int e) { return fieldpic ? entry_slot(e).fpoc[(e & MI_REF_PARITY) ? 1 : 0] : entry_slot(e).poc; };
            const int n0 = sh.num_ref_idx_l0_active_minus1 + 1, n1 = sh.num_ref_idx_l1_active_minus1 + 1;
            bx.num_ref_idx_l1_active = static_cast<uint8_t>(n1);
            bx.direct_spatial = static_cast<uint8_t>(sh.direct_spatial_mv_pred), bx.direct_8x8_inference = static_cast<uint8_t>(sps.direct_8x8_inference);
            bx.wp_mode = static_cast<uint8_t>(pps.weighted_bipred);
            for (int i = 0; i < MI_MAX_REFS; i++) {
                bx.wp_lw1[i] = static_cast<int16_t>(explicit_wp ? sh.luma_weight_l1[i] : 1), bx.wp_lo1[i] = static_cast<int16_t>(sh.luma_offset_l1[i]);
                for (int j = 0; j < 2; j++)
                    bx.wp_cw1[i][j] = static_cast<int16_t>(explicit_wp ? sh.chroma_weight_l1[i][j] : 1), bx.wp_co1[i][j] = static_cast<int16_t>(sh.chroma_offset_l1[i][j]);
            }
            // POC distances: DistScaleFactor of temporal direct prediction (8.4.1.2.3) per refIdxL0 against RefPicList1[0], and the
            // implicit bi-prediction weights (8.4.2.3.1) per (refIdxL0, refIdxL1)
            auto dist_scale = [&](int slot0, int slot1, bool *copy) {
                const Slot &p0 = entry_slot(slot0);
                const int poc0 = entry_poc(slot0), poc1 = entry_poc(slot1);
                const int tb = std::min(std::max(cur_poc - poc0, -128), 127), td = std::min(std::max(poc1 - poc0, -128), 127);
                *copy = td == 0 || p0.ref == 2;
                if (td == 0) return 256;
                const int tx = (16384 + std::abs(td / 2)) / td;
                return std::min(std::max((tb * tx + 32) >> 6, -1024), 1023);
            };
            const int col_slot = bx.ref_slot1[0];
            for (int i = 0; i < MI_MAX_REFS; i++) {
                bool copy = true;
                int dsf = 256;
                if (i < n0 && sd.ref_slot[i] >= 0 && col_slot >= 0) dsf = dist_scale(sd.ref_slot[i], col_slot, &copy);
                bx.dist_scale[i] = static_cast<int16_t>(copy ? 256 : dsf);
                for (int j = 0; j < MI_MAX_REFS; j++) {
                    int w1 = 32;
                    if (i < n0 && j < n1 && sd.ref_slot[i] >= 0 && bx.ref_slot1[j] >= 0) {
                        bool cp;
                        const int f = dist_scale(sd.ref_slot[i], bx.ref_slot1[j], &cp) >> 2;
                        const int td = entry_poc(bx.ref_slot1[j]) - entry_poc(sd.ref_slot[i]);
                        if (td != 0 && entry_slot(sd.ref_slot[i]).ref != 2 && entry_slot(bx.ref_slot1[j]).ref != 2 && f >= -64 && f <= 128) w1 = f;
                    }
                    bx.implicit_w1[i][j] = static_cast<int16_t>(w1);
                }
            }
            // the co-located picture: its motion record array, and when its slices are entropy-decoded relative to this one
            level = 1;
            if (col_slot >= 0) {
                const Slot &cs = entry_slot(col_slot);
                const int cslot = fieldpic ? MI_REF_SLOT(col_slot) : col_slot, cpar = fieldpic && (col_slot & MI_REF_PARITY) ? 1 : 0;
                // the co-located picture must have the structure of the current one (8.4.1.2.1's frame-from-field-pair and field-from-frame
                // cases, with their vertical vector scaling, are not implemented)
                if (cs.field_coded != fieldpic && !cs.nonexisting) {
                    set_error("stream %d: a B %s whose RefPicList1[0] was coded as %s is out of scope (direct prediction across picture structures)", si,
                              fieldpic ? "field" : "frame picture", cs.field_coded ? "field pictures" : "a frame picture");
                    return H264MI_EUNSUPPORTED;
                }
                // a field's motion: the second half of the frame slot's array for the bottom field (a field has half the frame's macroblocks)
                bx.col = reinterpret_cast<uint64_t>(d->d_colrec + (static_cast<size_t>(si) * d->n_slots + cslot) * d->colrec_per_slot + (cpar ? d->colrec_per_slot / 2 : 0));
                bx.col_short = cs.ref == 1;
                const int cpic = fieldpic ? cs.fpic[cpar] : cs.pic;
                if (cpic >= 0) {
                    level = g.pic_level[cpic] + 1;
                    g.pic_save_col[cpic] = 1;
                } else if (!cs.col_valid[cpar] && !cs.nonexisting) {
                    // decoded by an earlier batch, before this decoder kept motion (the arrays exist from the first B slice on, ensure_b_buffers):
                    // direct prediction from it would silently see an intra picture
                    set_error("stream %d: the co-located picture of a B slice was decoded before the decoder's first B slice; its motion was not kept", si);
                    return H264MI_EUNSUPPORTED;
                }
            }
            sd.bext = static_cast<uint32_t>(g.n_bext);
            g.h_bext[g.n_bext++] = bx;
        }
    }
    { // K11: the picture order counts the lists were built with, before a memory management operation 5 of this picture rewrites them
        g.slice_refs.resize(g.n_slices + 1);
        Stage::SliceRefs &sr = g.slice_refs[g.n_slices];
        memset(&sr, 0, sizeof(sr));
        const bool fieldpic = sh.field_pic != 0;
        const Slot &cur = s.dpb.slots[s.dpb.cur_slot];
        sr.cur_poc = fieldpic ? cur.fpoc[sh.bottom_field ? 1 : 0] : cur.poc;
        const int16_t *lists[2] = {st != 2 ? sd.ref_slot : nullptr, st == 1 ? g.h_bext[sd.bext].ref_slot1 : nullptr};
        const int active[2] = {sh.num_ref_idx_l0_active_minus1 + 1, sh.num_ref_idx_l1_active_minus1 + 1};
        for (int l = 0; l < 2; l++) {
            if (!lists[l]) continue;
            sr.n[l] = static_cast<uint8_t>(std::min(std::max(active[l], 0), MI_MAX_REFS));
            for (int i = 0; i < sr.n[l]; i++) sr.poc[l][i] = lists[l][i] >= 0 ? list_entry_poc(s.dpb, lists[l][i], fieldpic) : sr.cur_poc;
        }
    }
    g.pic_level[s.cur_pic] = std::max(g.pic_level[s.cur_pic], level);
    g.slice_level.resize(g.n_slices + 1);
    g.slice_level[g.n_slices] = level;
    g.bits_used = std::max(g.bits_used, off + rlen);
    g.bits_end = std::max(g.bits_end, g.bits_used);
    g.n_slices++;
    s.cur_slices++;
    return H264MI_OK;
}

// What the entropy kernels reported for the slices of an executed batch (its status copy has arrived: the caller waited for
// ev_done or synchronised the streams).  A failed slice marks its stream: the pictures from there on are damaged, its references
// are dropped and nothing of it is decoded before its next IDR picture.  Called from h264mi_batch_sync for every batch that
// has been executed since the last look, and from h264mi_batch_prepare when it takes a staging set back -- so in the pipelined
// pattern (execute(k); prepare(k + 1); execute(k + 1); ...) a failure of batch k is acted upon before batch k + 2 is parsed.
static int harvest_status(h264mi_decoder *d, Stage &g) {
    if (!g.executed || g.harvested) return H264MI_OK;
    g.harvested = true;
    int result = H264MI_OK;
    for (int i = 0; i < g.n_slices; i++)
        if (g.h_status[8 * i]) {
            const SliceDesc &sd = g.h_slices[i];
            StreamState &s = d->st[g.h_pics[sd.pic_idx].stream];
            // the stream was reset (h264mi_decoder_reset / h264mi_stream_reset: a new connection took the slot, or the caller started over) after this
            // batch was prepared: what failed in it is not a property of what the slot decodes now
            if (g.h_pics[sd.pic_idx].stream < g.epochs.size() && g.epochs[g.h_pics[sd.pic_idx].stream] != s.epoch) continue;
            // error concealment: k_conceal has rewritten every macroblock of the slice as a copy from the picture's concealment reference; the picture
            // is a reference like any other, the stream goes on
            const bool field_cabac = g.h_pics[sd.pic_idx].field != 0 && g.h_pics[sd.pic_idx].cabac != 0;
            if (field_cabac) d->unpinned_failures++; // what a wrong value in the unpinned context tables looks like: the slice does not end on end_of_slice_flag where it should
            if (d->conceal && g.h_pics[sd.pic_idx].conceal_ref >= 0) {
                d->concealed_slices++;
                continue;
            }
            if (result == H264MI_OK)
                set_error("entropy kernel: slice %d (picture %u, stream %u) failed with code %u after %u macroblocks%s", i, sd.pic_idx, g.h_pics[sd.pic_idx].stream,
                          g.h_status[8 * i], g.h_status[8 * i + 1],
                          field_cabac ? " -- a CABAC field picture: the context values of field-coded blocks are unpinned (h264mi_config.allow_unpinned_field_cabac)" : "");
            if (s.status == H264MI_OK || s.status_batch != &g) { // first failure of the stream in this batch
                s.status = H264MI_EDECODE, s.status_batch = &g;
                s.dpb.drop_references();
                s.need_idr = true;
            }
            result = H264MI_EDECODE;
        }
    if (d->conceal) // the counter k_conceal left behind the status words: concealed macroblocks per picture; and the slices dropped for their header
        for (int p = 0; p < g.n_pics; p++)
            if (g.h_pics[p].stream >= g.epochs.size() || g.epochs[g.h_pics[p].stream] == d->st[g.h_pics[p].stream].epoch)
                d->concealed_mbs += g.h_status[8 * g.n_slices + p], d->concealed_slices += g.pic_dropped[p],
                    // (only an inserted picture has no slice -- a frame: conceal_frame_num_gap, a field: flush_pending_field)
                    d->concealed_pics += g.h_pics[p].n_slices == 0 && g.h_pics[p].conceal_ref >= 0 && g.h_pics[p].field == 0,
                    d->concealed_fields += g.h_pics[p].n_slices == 0 && g.h_pics[p].conceal_ref >= 0 && g.h_pics[p].field != 0;
    return result;
}

extern "C" int32_t h264mi_batch_prepare(h264mi_decoder *d, int32_t n_streams, const uint8_t *const *bufs, const size_t *lens, h264mi_batch_info *info) {
    if (!d || n_streams < 0 || n_streams > static_cast<int>(d->st.size()) || (n_streams && (!bufs || !lens))) return H264MI_EINVAL;
    GUARD(d);
    auto t0 = std::chrono::steady_clock::now();
    // The next staging set; the batch that used it last (MI_STAGES batches ago) must have finished executing.  The batch
    // prepared before this one may still be executing: nothing it uses is touched here.
    const int prev_stage = d->prep;
    d->prep = (d->prep + 1) % MI_STAGES;
    Stage &g = d->stage[d->prep];
    if (g.executed) {
        HIP_TRY(hipEventSynchronize(g.ev_done));
        (void)harvest_status(d, g); // a batch nobody synchronised on: its failures still mark their streams (need_idr) before this parse
    }
    g.prepared = false, g.executed = false;
    d->scaling_used[d->prep] = 0; // (the batch that filled this staging set before has finished: its LevelScale sets may go to new matrices)
    g.n_slices = g.n_pics = 0;
    g.bits_used = 0, g.mb_used = 0, g.wmb_max = 0, g.hmb_max = 0, g.mbs_max = 0;
    g.map_cursor = g.bits_end = 0;
    g.fmo_pics.clear();
    g.grey.clear();
    g.epochs.resize(d->st.size());
    for (size_t si = 0; si < d->st.size(); si++) g.epochs[si] = d->st[si].epoch;
    g.n_bext = 0;
    g.pic_level.clear(), g.slice_level.clear(), g.pic_save_col.clear(), g.pic_wave.clear(), g.pic_init_qp.clear(), g.pic_dropped.clear(), g.slice_refs.clear(), g.pic_conceal_poc.clear();
    memset(&g.info, 0, sizeof(g.info));
    for (size_t si = 0; si < d->st.size(); si++) {
        StreamState &s = d->st[si];
        s.dpb.begin_batch(); // reference pictures at batch start, and a first field waiting for its second one, stay put for the whole batch
        if (s.dpb.pend_slot >= 0) s.pend_out.pic = -1; // (that field was decoded by an earlier batch now)
        // the frames of the batch prepared before this one stay readable (and, if it is still executing, writable)
        if (MI_STAGES > 1)
            for (const OutFrame &o : d->stage[prev_stage].out[si]) s.dpb.slots[o.slot].held = true;
        g.out[si].clear();
        s.n_pics_in_batch = 0;
        s.cur_pic = -1;
        s.status = H264MI_OK;
    }
    // ---- pass 1 (parallel over streams): Annex-B scan ----
    const int n_threads = std::max(1, std::min<int>({static_cast<int>(std::thread::hardware_concurrency()), 16, n_streams}));
    std::vector<std::vector<h264mi_nal>> all_nals(n_streams);
    std::vector<int> n_nals(n_streams, 0);
    auto parallel_for = [&](int count, const std::function<void(int)> &fn) {
        if (n_threads <= 1 || count <= 1) {
            for (int i = 0; i < count; i++) fn(i);
            return;
        }
        std::atomic<int> next(0);
        std::vector<std::thread> pool;
        for (int t = 0; t < std::min(n_threads, count); t++)
            pool.emplace_back([&] {
                for (int i = next.fetch_add(1); i < count; i = next.fetch_add(1)) fn(i);
            });
        for (auto &t : pool) t.join();
    };
    parallel_for(n_streams, [&](int si) {
        if (!bufs[si] || !lens[si]) return;
        std::vector<h264mi_nal> &v = all_nals[si];
        v.resize(1024);
        int n = 0;
        while (annexb_scan(bufs[si], lens[si], v.data(), static_cast<int>(v.size()), &n) == H264MI_ECAPACITY) v.resize(v.size() * 4);
        n_nals[si] = n;
    });
    // ---- pass 2 (serial, trivial): staging offsets of the slice NALs; the escaped length bounds the RBSP length ----
    struct Staged {
        int si, nal;
        size_t off, rlen;
    };
    std::vector<Staged> staged;
    std::vector<std::vector<int>> staged_of(n_streams); // [stream][nal] -> index into staged or -1
    {
        size_t cursor = 0;
        for (int si = 0; si < n_streams; si++) {
            staged_of[si].assign(n_nals[si], -1);
            for (int i = 0; i < n_nals[si]; i++) {
                const h264mi_nal &nal = all_nals[si][i];
                if (nal.type != 1 && nal.type != 5) continue;
                const size_t off = (cursor + 15) & ~static_cast<size_t>(15);
                if (off + nal.num_bytes + 4096 > d->bits_cap) {
                    set_error("bitstream staging buffer too small (%zu bytes)", d->bits_cap);
                    return H264MI_ECAPACITY;
                }
                staged_of[si][i] = static_cast<int>(staged.size());
                staged.push_back({si, i, off, 0});
                cursor = off + nal.num_bytes;
            }
        }
        g.map_cursor = cursor; // slice group maps (FMO pictures) go behind the last slice
    }
    // ---- pass 3 (parallel over slices): remove emulation prevention straight into the pinned staging buffer ----
    parallel_for(static_cast<int>(staged.size()), [&](int k) {
        Staged &sg = staged[k];
        const h264mi_nal &nal = all_nals[sg.si][sg.nal];
        sg.rlen = unescape(bufs[sg.si] + nal.offset + 1, nal.num_bytes - 1, g.h_bits + sg.off);
    });
    // ---- pass 4 (serial): parameter sets, slice headers, DPB / POC / reference lists, descriptors ----
    int first_error = H264MI_OK;
    for (int si = 0; si < n_streams; si++) {
        if (!bufs[si] || !lens[si]) continue;
        StreamState &s = d->st[si];
        const std::vector<h264mi_nal> &nals = all_nals[si];
        const int n = n_nals[si];
        std::vector<uint8_t> tmp;
        // what this stream adds to the batch sits at the tail of every table: a failing stream is taken out again
        const int pics0 = g.n_pics, slices0 = g.n_slices, bext0 = g.n_bext;
        const uint64_t mb0 = g.mb_used;
        const int64_t info_mb0 = g.info.n_macroblocks;
        int r = H264MI_OK;
        for (int i = 0; i < n && r == H264MI_OK; i++) {
            const h264mi_nal &nal = nals[i];
            const uint8_t *p = bufs[si] + nal.offset;
            switch (nal.type) {
            case 7: {
                tmp.resize(nal.num_bytes);
                size_t rl = unescape(p + 1, nal.num_bytes - 1, tmp.data());
                h264mi_sps sps;
                r = parse_sps(tmp.data(), rl, &sps);
                if (r == H264MI_OK) {
                    if (s.dpb.cur_slot >= 0) finish_picture(d, si);
                    if (d->conceal_lone && s.dpb.pend_slot >= 0 && sps.id == s.pend_sps_id && memcmp(&s.sps[sps.id], &sps, sizeof(sps))) s.pend_stale = true;
                    s.sps[sps.id] = sps, s.sps_ok[sps.id] = true;
                }
                break;
            }
            case 8: {
                tmp.resize(nal.num_bytes);
                size_t rl = unescape(p + 1, nal.num_bytes - 1, tmp.data());
                BitReader br(tmp.data(), rl);
                br.ue();
                uint32_t sid = br.ue();
                if (sid > 31 || !s.sps_ok[sid]) {
                    set_error("stream %d: PPS refers to missing SPS %u", si, sid);
                    r = H264MI_EBITSTREAM;
                    break;
                }
                h264mi_pps pps;
                std::vector<uint8_t> ids(static_cast<size_t>(s.sps[sid].pic_width_in_mbs_minus1 + 1) * (s.sps[sid].pic_height_in_map_units_minus1 + 1));
                size_t n_ids = 0;
                r = parse_pps_ids(&s.sps[sid], tmp.data(), rl, &pps, ids.data(), ids.size(), &n_ids);
                if (r == H264MI_OK) {
                    if (s.dpb.cur_slot >= 0) finish_picture(d, si);
                    ids.resize(n_ids);
                    if (d->conceal_lone && s.dpb.pend_slot >= 0 && pps.id == s.pend_pps_id && (memcmp(&s.pps[pps.id], &pps, sizeof(pps)) || s.sg_ids[pps.id] != ids)) s.pend_stale = true;
                    s.pps[pps.id] = pps, s.pps_ok[pps.id] = true;
                    s.sg_ids[pps.id] = std::move(ids);
                }
                break;
            }
            case 1:
            case 5: {
                const Staged &sg = staged[staged_of[si][i]];
                r = add_slice(d, si, sg.off, sg.rlen, nal.ref_idc, nal.type);
                break;
            }
            case 9:
            case 10:
            case 11:
                if (s.dpb.cur_slot >= 0) finish_picture(d, si);
                if (nal.type != 9) r = flush_pending_field(d, si); // end of sequence / end of stream: no second field will follow a lone first one
                break;
            case 2:
            case 3:
            case 4: // slice data partitions A / B / C (Extended profile; h264/nalUnit.go:14-16 names them): ignoring them would drop pictures without a word
                set_error("stream %d: slice data partitioning (nal_unit_type %d, Extended profile) is out of scope", si, nal.type);
                r = H264MI_EUNSUPPORTED;
                break;
            default: break; // SEI, filler, the extension units of SVC / MVC / 3D-AVC streams (14, 15, 20, 21: the base layer is decoded) ... (h264/server.go:147-164 ignores them too)
            }
        }
        if (r != H264MI_OK) {
            // The stream leaves the batch: its pictures, slices and records are dropped, its references are forgotten
            // (nothing is decodable before its next IDR picture); the other streams are not affected.
            g.n_pics = pics0, g.n_slices = slices0, g.mb_used = mb0, g.info.n_macroblocks = info_mb0;
            g.n_bext = bext0;
            g.pic_level.resize(pics0), g.pic_save_col.resize(pics0), g.pic_wave.resize(pics0), g.slice_level.resize(slices0), g.pic_init_qp.resize(pics0), g.pic_dropped.resize(pics0), g.slice_refs.resize(slices0), g.pic_conceal_poc.resize(pics0);
            while (!g.fmo_pics.empty() && static_cast<int>(g.fmo_pics.back()) >= pics0) g.fmo_pics.pop_back();
            g.grey.erase(std::remove_if(g.grey.begin(), g.grey.end(), [&](const Stage::GreyFill &f) { return static_cast<int>(f.stream) == si; }), g.grey.end());
            reset_stream(s, true);
            g.out[si].clear();
            s.need_idr = true;
            s.status = r;
            if (first_error == H264MI_OK) first_error = r;
            if (!d->isolate) return r;
            continue;
        }
        if (s.dpb.cur_slot >= 0) finish_picture(d, si);
    }
    // A reference picture that outlives the batch may become the co-located picture of a B picture of a later batch: its
    // motion is kept too (8.4.1.2.1).
    g.pic_level.resize(g.n_pics, 0), g.pic_save_col.resize(g.n_pics, 0), g.pic_wave.resize(g.n_pics, 0), g.slice_level.resize(g.n_slices, 0);
    g.pic_init_qp.resize(g.n_pics, 26), g.pic_dropped.resize(g.n_pics, 0);
    g.slice_refs.resize(g.n_slices), g.pic_conceal_poc.resize(g.n_pics);
    for (int si = 0; si < n_streams; si++)
        for (const Slot &sl : d->st[si].dpb.slots)
            if (sl.ref)
                for (int pic : {sl.pic, sl.fpic[0], sl.fpic[1]})
                    if (pic >= 0 && pic < g.n_pics) g.pic_save_col[pic] = 1;
    // Slice order = launch order: by level (see Stage), and inside a level longest-processing-time-first -- the entropy
    // kernels run one slice per workgroup and workgroups are dispatched in index order, so the biggest slices (I pictures)
    // must start first.
    int n_levels = 1;
    {
        std::vector<int> order(g.n_slices);
        for (int i = 0; i < g.n_slices; i++) order[i] = i, n_levels = std::max(n_levels, g.slice_level[i] + 1);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
            if (g.slice_level[x] != g.slice_level[y]) return g.slice_level[x] < g.slice_level[y];
            return g.h_slices[x].rbsp_size > g.h_slices[y].rbsp_size;
        });
        std::vector<SliceDesc> tmp(g.h_slices, g.h_slices + g.n_slices);
        std::vector<int> lv(g.slice_level);
        std::vector<Stage::SliceRefs> refs(g.slice_refs); // (MbRec::slice_idx indexes the sorted table: K11's table goes with it)
        for (int i = 0; i < g.n_slices; i++) g.h_slices[i] = tmp[order[i]], g.slice_level[i] = lv[order[i]], g.slice_refs[i] = refs[order[i]];
        g.level_first.assign(n_levels + 1, g.n_slices);
        for (int i = g.n_slices - 1; i >= 0; i--) g.level_first[g.slice_level[i]] = i;
        for (int l = n_levels - 1; l >= 0; l--) g.level_first[l] = std::min(g.level_first[l], g.level_first[l + 1]);
        int n_mode[2] = {0, 0}; // level 0 by entropy coding mode: CAVLC, CABAC slices
        for (int i = g.level_first[0]; i < g.level_first[1]; i++) n_mode[g.h_pics[g.h_slices[i].pic_idx].cabac != 0]++;
        g.ent_kernel = mi_entropy_kernel_choice(n_mode[1], n_mode[0], !g.fmo_pics.empty());
#if defined(H264MI_TEST_HOOKS) /* measurement: the general kernel for CABAC launches too, as before there was a CABAC-only build */
        if (const char *e = getenv("H264MI_ENT_GENERIC"))
            if (atoi(e) && g.ent_kernel == MI_ENT_K_CABAC) g.ent_kernel = MI_ENT_K_GENERAL;
#endif
    }
    if (d->conceal) {
        // Error concealment.  Behind the slices of the batch one SliceDesc per picture -- what MbRec::slice_idx of a concealed macroblock names, so that
        // K4 finds neither the explicit weights of the slice that failed nor those of the slice whose wavefront blanked a gap: type P, wp_flag 0 and
        // identity weights (the one-list K4 chooses explicit weighting per picture: denominators 0, weight 1, offset 0 give the default prediction
        // exactly; the two-list K4 sees a slice that is not a B slice and has no wp_flag: default), QP_Y from the PPS, all edges filtered, and a
        // slice_in_pic no real slice has.  And the picture -> slices map of the sorted table (k_conceal).
        for (int p = 0; p < g.n_pics; p++) {
            SliceDesc &cd = g.h_slices[g.n_slices + p];
            memset(&cd, 0, sizeof(cd));
            cd.pic_idx = static_cast<uint32_t>(p);
            cd.slice_type = 0, cd.slice_qp = g.pic_init_qp[p], cd.num_ref_idx_active = 1;
            cd.slice_in_pic = 0xFFFF;
            for (int i = 0; i < MI_MAX_REFS; i++) {
                cd.ref_slot[i] = static_cast<int16_t>(i == 0 ? g.h_pics[p].conceal_ref : -1);
                cd.wp_lw[i] = 1, cd.wp_cw[i][0] = cd.wp_cw[i][1] = 1;
            }
        }
        // ... and K11's view of them: one active entry, the concealment reference, where the picture has one
        g.slice_refs.resize(g.n_slices + g.n_pics);
        for (int p = 0; p < g.n_pics; p++) {
            Stage::SliceRefs &sr = g.slice_refs[g.n_slices + p];
            memset(&sr, 0, sizeof(sr));
            sr.cur_poc = g.pic_conceal_poc[p].cur, sr.n[0] = g.h_pics[p].conceal_ref >= 0, sr.poc[0][0] = g.pic_conceal_poc[p].ref;
        }
        uint32_t at = static_cast<uint32_t>(g.n_pics);
        for (int p = 0; p < g.n_pics; p++) g.h_cmap[p] = at, at += g.h_pics[p].n_slices;
        std::vector<uint32_t> fill(g.h_cmap, g.h_cmap + g.n_pics);
        for (int i = 0; i < g.n_slices; i++) g.h_cmap[fill[g.h_slices[i].pic_idx]++] = static_cast<uint32_t>(i);
    }
    // picture "waves": pictures that do not predict from one another are reconstructed side by side -- wave 0 holds the pictures that read no
    // picture of this batch (intra pictures wherever they stand in their stream; pictures whose references an earlier batch decoded), wave n + 1
    // the pictures whose latest reference is of wave n (Stage::pic_wave; with I P P P ... that is the k-th picture of every stream, with
    // I B B P ... the B pictures share the wave of the P picture that follows them in decoding order, an all-intra stream is one wave).  Per wave:
    // all pictures (K3), the inter pictures without / the pictures with B slices (K4 / K4 two-list), the pictures without B slices (K5; with: K5 two-list)
    size_t nw = 0;
    for (int i = 0; i < g.n_pics; i++) nw = std::max<size_t>(nw, static_cast<size_t>(g.pic_wave[i]) + 1);
    g.waves.assign(nw, {});
    g.waves_inter.assign(nw, {});
    for (int i = 0; i < g.n_pics; i++) {
        g.waves[g.pic_wave[i]].push_back(i);
        // (error concealment: the concealed macroblocks of a picture whose delivered slices are all I slices are inter macroblocks -- K4 must see it)
        if (!g.h_pics[i].is_intra_only || g.h_pics[i].conceal_ref >= 0) g.waves_inter[g.pic_wave[i]].push_back(i);
    }
    g.wave_off.clear();
    g.wave_inter_off.clear();
    g.wave_b_off.assign(nw, 0), g.wave_b_n.assign(nw, 0), g.wave_p_off.assign(nw, 0), g.wave_p_n.assign(nw, 0), g.wave_nb_off.assign(nw, 0), g.wave_nb_n.assign(nw, 0);
    uint32_t pos = 0;
    for (size_t w = 0; w < nw; w++) {
        g.wave_off.push_back(pos);
        for (uint32_t p : g.waves[w]) g.h_lists[pos++] = p;
        g.wave_inter_off.push_back(pos);
        g.wave_p_off[w] = pos;
        for (uint32_t p : g.waves_inter[w])
            if (!g.h_pics[p].has_b) g.h_lists[pos++] = p;
        g.wave_p_n[w] = pos - g.wave_p_off[w];
        g.wave_b_off[w] = pos;
        for (uint32_t p : g.waves[w])
            if (g.h_pics[p].has_b) g.h_lists[pos++] = p;
        g.wave_b_n[w] = pos - g.wave_b_off[w];
        g.wave_nb_off[w] = pos;
        for (uint32_t p : g.waves[w])
            if (!g.h_pics[p].has_b) g.h_lists[pos++] = p;
        g.wave_nb_n[w] = pos - g.wave_nb_off[w];
    }
    g.colsave_n.assign(n_levels, 0), g.prep_off.assign(n_levels, 0), g.prep_n.assign(n_levels, 0);
    for (int l = 0; l < n_levels; l++) {
        g.prep_off[l] = pos;
        for (int i = 0; i < g.n_pics; i++)
            if (g.pic_level[i] == l) {
                g.h_lists[pos++] = i;
                PicDesc &pd = g.h_pics[i];
                pd.save_col = g.pic_save_col[i] && d->d_colrec != nullptr; // (no B slice seen yet: nothing to keep, see ensure_b_buffers)
                const int par = pd.field == 2 ? 1 : 0; // (a bottom field's motion: the second half of its frame slot's array)
                pd.col_out = d->d_colrec ? reinterpret_cast<uint64_t>(d->d_colrec + (static_cast<size_t>(pd.stream) * d->n_slots + pd.slot) * d->colrec_per_slot +
                                                                      (par ? d->colrec_per_slot / 2 : 0))
                                         : 0;
                if (pd.save_col) d->st[pd.stream].dpb.slots[pd.slot].col_valid[par] = true; // (the slot is this picture's until the next prepare at least: held)
                g.colsave_n[l] += pd.save_col;
            }
        g.prep_n[l] = pos - g.prep_off[l];
    }
    choose_dbprep_kernels(g);
    // K11's device table: PicOrderCnt(entry) - PicOrderCnt(current picture) per slice of the table, list and entry, clamped to int16; 0 behind the active entries
    for (size_t i = 0; i < g.slice_refs.size(); i++)
        for (int l = 0; l < 2; l++)
            for (int e = 0; e < MI_MAX_REFS; e++) {
                const Stage::SliceRefs &sr = g.slice_refs[i];
                const int64_t dp = e < sr.n[l] ? static_cast<int64_t>(sr.poc[l][e]) - sr.cur_poc : 0;
                g.h_dpoc[(i * 2 + l) * MI_MAX_REFS + e] = static_cast<int16_t>(std::min<int64_t>(std::max<int64_t>(dp, -32768), 32767));
            }
    // Uploads go to the entropy stream the next execute will use: in order with that pass's entropy kernel, and not behind
    // the batch that is still executing (the caller's stream waits for its reconstruction).  No stream of their own: the
    // runtime multiplexes streams onto 4 hardware queues by default, and a fifth stream ended up sharing a queue with one of
    // the kernel streams, which serialised entropy decoding and reconstruction of consecutive passes.
    hipStream_t up = d->ent_stream[d->pass & 1];
    if (g.n_slices || g.n_pics) {
        const size_t end = std::max(g.bits_used, g.bits_end); // (bits_end: behind the slice group maps of FMO pictures, if any)
        size_t nbytes = std::min(d->bits_cap, ((end + 15) & ~static_cast<size_t>(15)) + 4096);
        memset(g.h_bits + end, 0, nbytes - end);
        HIP_TRY(hipMemcpyAsync(g.d_bits, g.h_bits, nbytes, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(g.d_slices, g.h_slices, sizeof(SliceDesc) * (g.n_slices + (d->conceal ? g.n_pics : 0)), hipMemcpyHostToDevice, up));
        if (d->conceal) HIP_TRY(hipMemcpyAsync(g.d_cmap, g.h_cmap, sizeof(uint32_t) * (g.n_pics + g.n_slices), hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(g.d_pics, g.h_pics, sizeof(PicDesc) * g.n_pics, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(g.d_lists, g.h_lists, sizeof(uint32_t) * pos, hipMemcpyHostToDevice, up));
        if (g.n_bext) HIP_TRY(hipMemcpyAsync(g.d_bext, g.h_bext, sizeof(BSliceExt) * g.n_bext, hipMemcpyHostToDevice, up));
        if (g.ev_side) { // a K11 launch on the caller's stream may still be reading this set's table (the batch before last)
            HIP_TRY(hipStreamWaitEvent(up, g.ev_side, 0));
            g.ev_side = nullptr;
        }
        if (!g.slice_refs.empty()) HIP_TRY(hipMemcpyAsync(g.d_dpoc, g.h_dpoc, sizeof(int16_t) * 2 * MI_MAX_REFS * g.slice_refs.size(), hipMemcpyHostToDevice, up));
    }
    if (d->tables_dirty) {
        // a new PPS added a LevelScale set: the table only grows, so the batch still executing keeps seeing its own sets.
        // (h_tables is pinned and rewritten only by the next prepare, which cannot start its copy before this one is done:
        // same stream.)
        HIP_TRY(hipMemcpyAsync(d->d_tables, d->h_tables, sizeof(DevTables), hipMemcpyHostToDevice, up));
        d->tables_dirty = false;
    }
    HIP_TRY(hipEventRecord(g.ev_upload, up));
    g.info.n_frames = 0; // frames that go out with this batch (a frame coded as two field pictures counts once, where its second field is)
    for (const auto &o : g.out) g.info.n_frames += static_cast<int32_t>(o.size());
    g.info.n_slices = g.n_slices, g.info.bitstream_bytes = static_cast<int64_t>(g.bits_used);
    g.info.host_prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = g.info;
    g.prepared = true;
    return H264MI_OK;
}

static hipEvent_t next_event(h264mi_decoder *d, size_t &idx, int kind) {
    if (idx >= d->ev.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        d->ev.push_back(e);
        d->ev_kind.push_back(kind);
    }
    d->ev_kind[idx] = kind;
    return d->ev[idx++];
}

// One pass over a prepared batch.  exclusive: the pass runs alone (the caller has drained every stream), serialised on the decoder's stream, with
// record set 0 and ALL of the residual pool -- how a batch that ran out of residual blocks is repeated (retry_exhausted).
static int execute_stage(h264mi_decoder *d, int stage_idx, bool exclusive);

extern "C" int32_t h264mi_batch_execute(h264mi_decoder *d) {
    if (!d || !d->stage[d->prep].prepared) {
        set_error("h264mi_batch_execute: no prepared batch");
        return H264MI_EINVAL;
    }
    d->exec = d->prep; // sync and the frame accessors refer to this batch from now on
    d->derived.clear(); // derived frames are functions of the frames this pass rewrites
    d->stage[d->exec].retried = false;
    return execute_stage(d, d->exec, false);
}

static int execute_stage(h264mi_decoder *d, int stage_idx, bool exclusive) {
    if (exclusive) d->pass += (MI_SETS - d->pass % MI_SETS) % MI_SETS; // record set 0
    d->last_exec_stage = stage_idx, d->last_exec_set = static_cast<int>(d->pass % MI_SETS);
    d->dbprep_launches[0] = d->dbprep_launches[1] = 0;
    Stage &g = d->stage[stage_idx];
    if (!g.n_slices && !g.n_pics && g.grey.empty()) return H264MI_OK; // (pictures without slices: inserted for a lone field that an end-of-sequence unit revealed)
    GUARD(d);
    // frames that went out with one field decoded (flush_pending_field): the rows of the field that never came are painted mid-grey
    auto grey_fills = [&](hipStream_t st) -> hipError_t { // the first error, if any: a frame that was not painted must not go out as if it were
        for (const Stage::GreyFill &f : g.grey) {
            uint8_t *base = d->d_frames + (static_cast<size_t>(f.stream) * d->n_slots + f.slot) * d->slot_bytes;
            const size_t W = f.w, H = f.h, plane = W * H;
            hipError_t e = hipMemset2DAsync(base + f.parity * W, 2 * W, 128, W, H / 2, st);
            if (e == hipSuccess) e = hipMemset2DAsync(base + plane + f.parity * (W / 2), W, 128, W / 2, H / 4, st);
            if (e == hipSuccess) e = hipMemset2DAsync(base + plane + plane / 4 + f.parity * (W / 2), W, 128, W / 2, H / 4, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    if (!g.n_slices && !g.n_pics) { // nothing to decode: a chunk that only ended a sequence and thereby sent a lone first field out
        HIP_TRY(grey_fills(d->stream));
        HIP_TRY(hipEventRecord(g.ev_done, d->stream));
        g.executed = true, g.harvested = true;
        return H264MI_OK;
    }
    size_t ei = 0;
    const bool prof = d->profiling || exclusive; // (an exclusive pass takes the serialised path of the profiling mode; its event marks are harmless)
    const uint32_t pool_blocks = static_cast<uint32_t>(exclusive ? std::min<uint64_t>(d->pool_blocks * MI_SETS, 0xFFFF0000ull) : d->pool_blocks);
    auto mark = [&](int kind) {
        if (prof) hipEventRecord(next_event(d, ei, kind), d->stream);
    };
    // Pass n uses buffer set n&1.  Entropy runs on its own stream so that the entropy kernels of
    // pass n+1 overlap the reconstruction kernels of pass n; set reuse is fenced by events.
    const int set = static_cast<int>(d->pass % MI_SETS);
    hipStream_t es = d->ent_stream[d->pass & 1];
    MbRec *mbrec = d->d_mbrec[set];
    int16_t *coef = d->d_coef[set];
    // Entropy decoding, level by level (Stage::level_first): k_entropy or one of its builds (Stage::ent_kernel) for the I / P slices, k_entropy_b for each level of B
    // slices, and after each level k_dbprep for the pictures complete with it (K5's parameters; the ColRec arrays later B slices ask for).
    // `done`: recorded after the last level's k_dbprep -- what the reconstruction kernels wait for.
    auto launch_entropy = [&](hipStream_t st, size_t lds_pad, bool fence_prev_pass, hipEvent_t done) {
        const int n_levels = static_cast<int>(g.level_first.size()) - 1;
        // pictures with slice groups: a slice's macroblocks are scattered, so its wavefront cannot blank "its" range for what it
        // does not decode (SliceDesc::fill_from) -- all records of such a picture start out as MBT_NONE instead
        for (uint32_t pi : g.fmo_pics) hipMemsetAsync(mbrec + g.h_pics[pi].mb_base, 0, sizeof(MbRec) * g.h_pics[pi].wmb * g.h_pics[pi].hmb, st);
        hipMemsetAsync(d->d_imask[set], 0, sizeof(unsigned long long) * (g.mb_used / 64 + 2), st); // k_dbprep ORs K3's work list into it
        for (int lv = 0; lv < n_levels; lv++) {
            const int first = g.level_first[lv], n = g.level_first[lv + 1] - first;
            // ColRec arrays cross passes: B slices read what the previous pass's k_dbprep wrote, and this pass's k_dbprep may
            // rewrite the record array of a frame slot (released meanwhile) that the previous pass's B slices still read.  So
            // everything after the I/P launch waits for the previous pass's entropy stream -- the I/P launch itself does not
            // (it neither reads nor writes ColRec arrays), it overlaps the previous pass's B launches; batches without B slices on
            // both sides never wait.
            auto fence = [&] {
                if (fence_prev_pass) hipStreamWaitEvent(st, d->ev_col[(d->pass - 1) % MI_SETS], 0);
                fence_prev_pass = false;
            };
            if (lv > 0) fence();
            if (n > 0) {
                if (lv == 0)
                    hipLaunchKernelGGL(g.ent_kernel == MI_ENT_K_FMO ? k_entropy_f : (g.ent_kernel == MI_ENT_K_CABAC ? k_entropy_c : k_entropy), dim3(n), dim3(64), lds_pad, st, g.d_slices, g.d_pics, g.d_bits, d->d_tables, mbrec, coef, d->d_pool_head + set,
                                       pool_blocks, g.d_status, d->d_toprows[set], g.wmb_max, static_cast<uint32_t>(first));
                else
                    hipLaunchKernelGGL(k_entropy_b, dim3(n), dim3(64), 0, st, g.d_slices, g.d_pics, g.d_bits, d->d_tables, mbrec, coef, d->d_pool_head + set,
                                       pool_blocks, g.d_status, d->d_toprows[set], g.wmb_max, static_cast<uint32_t>(first), g.d_bext, d->d_mv1[set]);
            }
            // the pictures complete with this level: K5's strengths and filter parameters, and the motion later B slices (the next
            // level's, or a later batch's) take their direct prediction from
            if (g.colsave_n[lv]) fence();
            // error concealment: the lost macroblocks of these pictures become decodable records before anything downstream reads them
            if (d->conceal && g.prep_n[lv])
                hipLaunchKernelGGL(k_conceal, dim3(g.prep_n[lv]), dim3(256), 0, st, g.d_lists + g.prep_off[lv], g.d_pics, g.d_slices, g.d_cmap, static_cast<uint32_t>(g.n_slices),
                                   g.d_status, g.d_bits, d->d_tables, mbrec, d->d_mv1[set], g.d_status + 8 * static_cast<size_t>(g.n_slices));
            if (g.prep_n[lv]) {
                if (g.prep_kernel[lv] == MI_DBPREP_K_IP) {
                    const int chunks = std::max(1, (g.wmb_max + 63) / 64), hmax = std::max(1, g.hmb_max);
                    const int rows = d->dbprep_rows > 0 ? std::min(d->dbprep_rows, hmax) : mi_dbprep_ip_rows(static_cast<int>(g.prep_n[lv]), g.wmb_max, hmax);
                    hipLaunchKernelGGL(k_dbprep_ip, dim3(static_cast<uint32_t>(chunks * ((hmax + rows - 1) / rows)), (g.prep_n[lv] + 7u) & ~7u), dim3(64), 0, st,
                                       g.d_lists + g.prep_off[lv], g.d_pics, d->d_tables, mbrec, d->d_dbprm[set], d->d_imask[set], static_cast<int>(g.prep_n[lv]), chunks, rows);
                } else
                    hipLaunchKernelGGL(k_dbprep, dim3((g.mbs_max + MI_DBPREP_MBS - 1) / MI_DBPREP_MBS, (g.prep_n[lv] + 7u) & ~7u), dim3(256), 0, st, g.d_lists + g.prep_off[lv], g.d_pics,
                                       d->d_tables, mbrec, d->d_mv1[set], d->d_dbprm[set], 0, d->d_imask[set], static_cast<int>(g.prep_n[lv]));
                d->dbprep_launches[g.prep_kernel[lv]]++;
            }
            if (lv == n_levels - 1 && done) hipEventRecord(done, st);
        }
    };
    if (prof) { // profiling serialises the two stages on one stream so that HIP-event intervals are per kernel
        HIP_TRY(hipStreamWaitEvent(d->stream, g.ev_upload, 0));
        mark(-1);
        HIP_TRY(hipMemsetAsync(d->d_pool_head + set, 0, sizeof(uint32_t), d->stream));
        launch_entropy(d->stream, 0, false, nullptr);
        mark(0);
    } else {
        HIP_TRY(hipStreamWaitEvent(es, g.ev_upload, 0));
        // a K11 launch on the caller's stream reads the records of the pass executed last; the pass that rewrites that set runs on this entropy stream
        // again (two passes on: the streams alternate), and nothing else orders it behind the caller's stream
        if (d->last_side) HIP_TRY(hipStreamWaitEvent(es, d->last_side, 0));
        if (d->pass >= MI_SETS) { // pass n-MI_SETS finished reading this set: its reconstruction kernels and its entropy stream
            HIP_TRY(hipStreamWaitEvent(es, d->ev_rec[set], 0));
            HIP_TRY(hipStreamWaitEvent(es, d->ev_col[set], 0));
        }
        HIP_TRY(hipMemsetAsync(d->d_pool_head + set, 0, sizeof(uint32_t), es));
        launch_entropy(es, d->ent_lds_pad, (g.n_bext || d->last_pass_had_b) && d->pass > 0, d->ev_ent[set]);
        d->last_pass_had_b = g.n_bext > 0;
        HIP_TRY(hipEventRecord(d->ev_col[set], es)); // entropy stream through with this pass
        HIP_TRY(hipStreamWaitEvent(d->rec_stream, d->ev_ent[set], 0));
    }
    d->last_side = nullptr; // (the serialised path runs on the caller's stream, behind the launch)
    hipStream_t rs = prof ? d->stream : d->rec_stream;
    if (d->last_pack && !prof) { // a pack launch may still be reading frames this pass rewrites (the same batch executed again)
        HIP_TRY(hipStreamWaitEvent(rs, d->last_pack, 0));
        d->last_pack = nullptr;
    }
    // tag of a banded launch's hand-off words: no earlier launch on the same rings has used it (the rings start out zero, and
    // are zeroed again should the counter ever wrap)
    auto next_epoch = [&]() {
        if (++d->x_epoch == 0) {
            hipMemsetAsync(d->d_xring, 0, static_cast<size_t>(d->x_cap) * (d->Wmax / 16) * 24 * sizeof(unsigned long long), rs);
            hipMemsetAsync(d->d_xdone, 0, static_cast<size_t>(d->x_cap3) * (d->Wmax / 16) * sizeof(uint32_t), rs);
            d->x_epoch = 1;
        }
        return d->x_epoch;
    };
    HIP_TRY(grey_fills(rs));
    for (size_t w = 0; w < g.waves.size(); w++) {
        const uint32_t n = static_cast<uint32_t>(g.waves[w].size()), ni = g.wave_p_n[w], nbp = g.wave_b_n[w];
        if (!n) continue;
        int grp_log2 = 0; // K4 workgroups per picture: the largest picture's count of four-macroblock groups, rounded up to a power of two
        while ((4 << grp_log2) < g.mbs_max) grp_log2++;
        if (ni) {
            const uint32_t nb = ni << grp_log2;
            hipLaunchKernelGGL(k_inter, dim3(((nb + MI_K4_WG - 1) / MI_K4_WG + 7) & ~7u), dim3(64 * MI_K4_WG), 0, rs, g.d_lists + g.wave_p_off[w], g.d_pics, g.d_slices, d->d_tables, mbrec, coef, grp_log2,
                               static_cast<int>(nb));
            mark(1);
        }
        if (nbp) {
            const uint32_t nb = nbp << grp_log2;
            hipLaunchKernelGGL(k_inter_b, dim3(((nb + MI_K4_WG - 1) / MI_K4_WG + 7) & ~7u), dim3(64 * MI_K4_WG), 0, rs, g.d_lists + g.wave_b_off[w], g.d_pics, g.d_slices, d->d_tables, mbrec, coef, grp_log2,
                               static_cast<int>(nb), g.d_bext, d->d_mv1[set]);
            mark(1);
        }
        // K3 / K5 keep a picture inside one workgroup when the launch has pictures enough to fill the chip; otherwise the
        // banded kernels spread each picture over up to x_max_wgs / pictures workgroups (mi_intra_bands / mi_deblock_bands)
        // (K3 of a launch WITHOUT intra-only pictures -- the few intra macroblocks of P / B pictures -- is bound by the row with the most
        // of them: there the banded kernel also puts several wavefronts on a row)
        int nb3 = 1, nw3 = MI_INTRA_WAVES, wpr3 = 1;
        bool has_ipic = false;
        for (uint32_t pi : g.waves[w]) has_ipic |= g.h_pics[pi].is_intra_only != 0;
        mi_intra_bands(static_cast<int>(n), g.hmb_max, d->x_max_wgs, !has_ipic, &nb3, &nw3, &wpr3);
        if (nb3 > 1) {
            hipLaunchKernelGGL(k_intra_x, dim3(n * nb3), dim3(nw3 * 64), 0, rs, g.d_lists + g.wave_off[w], g.d_pics, d->d_pools, d->d_tables, mbrec, coef, d->d_xdone,
                               next_epoch(), nb3, d->d_xctl + 32, d->x_tk3, g.wmb_max, d->d_xctl + 64, wpr3, d->d_imask[set]);
            d->x_tk3 += n * nb3;
        } else
            hipLaunchKernelGGL(k_intra, dim3(n), dim3(MI_INTRA_WAVES * 64), 0, rs, g.d_lists + g.wave_off[w], g.d_pics, d->d_pools, d->d_tables, mbrec, coef, d->d_imask[set]);
        mark(2);
        int dbw = 1, dbring = 16, dbring_last = 16, dbbufs = 1, nb5 = 1, roles = 1;
        mi_deblock_bands(static_cast<int>(n), g.wmb_max, g.hmb_max, d->x_max_wgs, &nb5, &dbw, &dbring, &roles);
        if (nb5 > 1) {
            hipLaunchKernelGGL(k_deblock_x, dim3(n * nb5), dim3(dbw * 64), mi_deblock_lds_bytes_banded(dbw, dbring), rs, g.d_lists + g.wave_off[w], g.d_pics,
                               d->d_dbprm[set], dbring, 0, 1, d->d_xring, next_epoch(), nb5, d->d_xctl, d->x_tk5, g.wmb_max, d->d_xctl + 64, roles);
            d->x_tk5 += n * nb5;
        } else {
            mi_deblock8_plan(g.wmb_max, g.hmb_max, &dbw, &dbring, &dbring_last, &dbbufs, d->k5_max_waves);
            hipLaunchKernelGGL(k_deblock, dim3(n), dim3(dbw * 64), mi_deblock8_lds_bytes(dbw, dbring, dbring_last, dbbufs), rs, g.d_lists + g.wave_off[w], g.d_pics,
                               d->d_dbprm[set], dbring, dbring_last, dbbufs, d->d_xctl + 64);
        }
        mark(3);
    }
    HIP_TRY(hipEventRecord(d->ev_rec[set], rs));
    if (!prof) HIP_TRY(hipStreamWaitEvent(d->stream, d->ev_rec[set], 0)); // the caller's stream sees the finished pass
    d->pass++;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(g.h_status, g.d_status, sizeof(uint32_t) * (8 * static_cast<size_t>(g.n_slices) + (d->conceal ? static_cast<size_t>(g.n_pics) : 0)), hipMemcpyDeviceToHost,
                           d->stream)); // (error concealment: k_conceal's counters travel with the status words)
    HIP_TRY(hipMemcpyAsync(d->h_xstatus, d->d_xctl + 64, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipEventRecord(g.ev_done, d->stream)); // d->stream has waited for the reconstruction kernels: the batch's buffers are idle after this
    g.executed = true, g.harvested = false;
    d->ev_used = d->profiling ? ei : 0;
    return H264MI_OK;
}

// A pass whose slices ran out of residual blocks (entropy status 40: the pool holds 8 blocks per macroblock by default, the worst case is 26) is
// repeated once, alone, with the pools of all record sets as one -- three times the room -- before anything is held against its streams.
// Only the batch executed LAST is repeated: a batch executed after the exhausted one has already written its pictures into frame slots the
// exhausted batch's first pictures predict from (slots that became free while it ran), so repeating the older batch would predict from the
// younger one's samples and report success; in that case the exhaustion is held against the streams as any other entropy failure
// (a caller that pipelines execute(n), prepare(n + 1), execute(n + 1), sync sizes its pool -- h264mi_config.coef_blocks_per_mb -- or
// synchronises per batch).  Called by h264mi_batch_sync with every stream drained.
static int retry_exhausted(h264mi_decoder *d) {
    Stage &g = d->stage[d->exec]; // the batch executed last
    if (!g.executed || g.harvested || g.retried) return H264MI_OK;
    bool exhausted = false;
    for (int i = 0; i < g.n_slices && !exhausted; i++) exhausted = g.h_status[8 * i] == 40;
    if (!exhausted) return H264MI_OK;
    g.retried = true;
    const int r = execute_stage(d, d->exec, true);
    if (r != H264MI_OK) return r;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return H264MI_OK;
}

extern "C" int32_t h264mi_batch_sync(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    for (int i = 0; i < 2; i++) HIP_TRY(hipStreamSynchronize(d->ent_stream[i]));
    HIP_TRY(hipStreamSynchronize(d->rec_stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (d->profiling && d->ev_used >= 2) {
        size_t n = d->ev_used;
        double acc[4] = {0, 0, 0, 0};
        for (auto &v : d->launch_ms) v.clear();
        for (size_t i = 1; i < n && i < d->ev.size(); i++) {
            float ms = 0;
            hipEventElapsedTime(&ms, d->ev[i - 1], d->ev[i]);
            int k = d->ev_kind[i];
            if (k >= 0 && k < 4) acc[k] += ms, d->launch_ms[k].push_back(ms);
        }
        float tot = 0;
        hipEventElapsedTime(&tot, d->ev[0], d->ev[n - 1]);
        for (int k = 0; k < 4; k++) d->k_ms[k] = acc[k];
        d->k_ms[4] = tot;
    }
#if defined(H264MI_TEST_HOOKS)
    if (getenv("H264MI_SLICE_STATS")) { // diagnostics: per-slice entropy time (100 MHz ticks) and bin count (MI_ENT_STATS builds)
        Stage &g = d->stage[d->exec];
        for (int i = 0; i < g.n_slices && i < 64; i++)
            fprintf(stderr, "slice %d type %d bytes %u mbs %u us %.1f bins %u | Mclk fill %.1f syntax %.1f residual %.1f writeout %.1f\n", i, g.h_slices[i].slice_type,
                    g.h_slices[i].rbsp_size, g.h_status[8 * i + 1], g.h_status[8 * i + 2] * 0.01, g.h_status[8 * i + 3], g.h_status[8 * i + 4] * 16e-6,
                    g.h_status[8 * i + 5] * 16e-6, g.h_status[8 * i + 6] * 16e-6, g.h_status[8 * i + 7] * 16e-6);
        fprintf(stderr, "last slice type %d bytes %u mbs %u us %.1f bins %u\n", g.h_slices[g.n_slices - 1].slice_type, g.h_slices[g.n_slices - 1].rbsp_size,
                g.h_status[8 * (g.n_slices - 1) + 1], g.h_status[8 * (g.n_slices - 1) + 2] * 0.01, g.h_status[8 * (g.n_slices - 1) + 3]);
    }
    if (getenv("H264MI_SLICE_TIMELINE")) { // diagnostics (-DMI_ENT_STATS=3 builds): when the slices of each type started and ended within the pass
        Stage &g = d->stage[d->exec];
        uint32_t t0 = 0xFFFFFFFFu;
        for (int i = 0; i < g.n_slices; i++) t0 = std::min(t0, g.h_status[8 * i + 4]);
        for (int ty = 0; ty < 3; ty++) {
            int n = 0;
            double first_end = 1e30, last_start = 0, last_end = 0, sum = 0;
            for (int i = 0; i < g.n_slices; i++)
                if (g.h_slices[i].slice_type % 5 == ty) {
                    const double a = (g.h_status[8 * i + 4] - t0) * 0.01, b = (g.h_status[8 * i + 5] - t0) * 0.01;
                    n++, sum += b - a, first_end = std::min(first_end, b), last_start = std::max(last_start, a), last_end = std::max(last_end, b);
                }
            if (n) fprintf(stderr, "timeline: slice type %d: %d slices, mean %.1f us, first end %.1f, last start %.1f, last end %.1f us\n", ty, n, sum / n, first_end, last_start, last_end);
            if (n > 64) { // slices in 20 ms buckets of their end, split into those that started with the launch and the late ones, with their mean durations
                int cnt[2][16] = {};
                double dur[2][16] = {};
                for (int i = 0; i < g.n_slices; i++)
                    if (g.h_slices[i].slice_type % 5 == ty) {
                        const double a = (g.h_status[8 * i + 4] - t0) * 0.01, b = (g.h_status[8 * i + 5] - t0) * 0.01;
                        const int late = a > 5000.0, k = std::min(15, static_cast<int>(b / 20000.0));
                        cnt[late][k]++, dur[late][k] += b - a;
                    }
                for (int late = 0; late < 2; late++)
                    for (int k = 0; k < 16; k++)
                        if (cnt[late][k]) fprintf(stderr, "timeline:   %s, end in %3d..%3d ms: %5d slices, mean duration %.1f ms\n", late ? "late start" : "first wave", 20 * k, 20 * k + 20, cnt[late][k], dur[late][k] / cnt[late][k] * 1e-3);
            }
        }
    }
#endif
    if (*d->h_xstatus) { // a banded kernel gave up waiting for its neighbour workgroup: the pictures of that launch are wrong
        set_error("reconstruction hand-off timed out (code 0x%08x)", *d->h_xstatus);
        *d->h_xstatus = 0;
        HIP_TRY(hipMemset(d->d_xctl + 64, 0, sizeof(uint32_t)));
        return H264MI_EDEVICE;
    }
    {
        const int r = retry_exhausted(d); // (leaves every stream drained again)
        if (r != H264MI_OK) return r;
    }
    // every batch executed since the last look (pipelined callers synchronise once for several), the most recent one last
    int result = H264MI_OK;
    for (int k = 1; k <= MI_STAGES; k++) {
        const int r = harvest_status(d, d->stage[(d->exec + k) % MI_STAGES]);
        if (r != H264MI_OK) result = r;
    }
    return d->isolate ? H264MI_OK : result;
}

extern "C" int32_t h264mi_decode_batch(h264mi_decoder *d, int32_t n, const uint8_t *const *bufs, const size_t *lens, h264mi_batch_info *info) {
    int r = h264mi_batch_prepare(d, n, bufs, lens, info);
    if (r != H264MI_OK) return r;
    r = h264mi_batch_execute(d);
    if (r != H264MI_OK) return r;
    return h264mi_batch_sync(d);
}

extern "C" int32_t h264mi_last_kernel_times(h264mi_decoder *d, double ms[5]) {
    if (!d || !ms) return H264MI_EINVAL;
    for (int i = 0; i < 5; i++) ms[i] = d->k_ms[i];
    return H264MI_OK;
}

extern "C" int32_t h264mi_last_launch_times(h264mi_decoder *d, int32_t kernel, float *ms, int32_t cap, int32_t *n) {
    if (!d || !n || kernel < 0 || kernel > 3 || cap < 0 || (cap && !ms)) return H264MI_EINVAL;
    const std::vector<float> &v = d->launch_ms[kernel];
    for (int i = 0; i < cap && i < static_cast<int>(v.size()); i++) ms[i] = v[i];
    *n = static_cast<int32_t>(v.size());
    return H264MI_OK;
}

extern "C" int32_t h264mi_stream_frame_count(h264mi_decoder *d, int32_t stream, int32_t *n) {
    if (d && n && stream == H264MI_STREAM_DERIVED) {
        *n = static_cast<int32_t>(d->derived.size());
        return H264MI_OK;
    }
    if (!d || !n || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    *n = static_cast<int32_t>(d->stage[d->exec].out[stream].size());
    return H264MI_OK;
}

int frame_ptrs(h264mi_decoder *d, int stream, int frame, uint8_t **y, const OutFrame **of) {
    if (d && stream == H264MI_STREAM_DERIVED) {
        if (frame < 0 || frame >= static_cast<int>(d->derived.size())) return H264MI_EINVAL;
        *of = &d->derived[frame].of;
        *y = d->d_derived + d->derived[frame].off;
        return H264MI_OK;
    }
    if (!d || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    const std::vector<OutFrame> &out = d->stage[d->exec].out[stream];
    if (frame < 0 || frame >= static_cast<int>(out.size())) return H264MI_EINVAL;
    *of = &out[frame];
    *y = d->d_frames + (static_cast<size_t>(stream) * d->n_slots + out[frame].slot) * d->slot_bytes;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_device_planes(h264mi_decoder *d, int32_t stream, int32_t frame, void **y, void **cb, void **cr, int32_t *pitch_y, int32_t *pitch_c,
                                              int32_t *cw, int32_t *ch) {
    if (stream == H264MI_STREAM_DERIVED) return H264MI_EINVAL; // a derived frame is reached through the output calls only
    uint8_t *p;
    const OutFrame *of;
    int r = frame_ptrs(d, stream, frame, &p, &of);
    if (r != H264MI_OK) return r;
    const int W = of->wmb * 16, H = of->hmb * 16;
    if (y) *y = p;
    if (cb) *cb = p + static_cast<size_t>(W) * H;
    if (cr) *cr = p + static_cast<size_t>(W) * H * 5 / 4;
    if (pitch_y) *pitch_y = W;
    if (pitch_c) *pitch_c = W / 2;
    if (cw) *cw = W;
    if (ch) *ch = H;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_get_info(h264mi_decoder *d, int32_t stream, int32_t frame, h264mi_frame_info *fi) {
    uint8_t *p;
    const OutFrame *of;
    int r = frame_ptrs(d, stream, frame, &p, &of);
    if (r != H264MI_OK) return r;
    if (!fi) return H264MI_EINVAL;
    fi->width = of->width, fi->height = of->height, fi->coded_width = of->wmb * 16, fi->coded_height = of->hmb * 16;
    fi->crop_x = of->crop_x, fi->crop_y = of->crop_y;
    fi->pic_order_cnt = of->poc, fi->frame_num = of->frame_num, fi->nal_ref_idc = of->nal_ref_idc, fi->idr = of->idr;
    fi->new_sequence = of->new_sequence;
    return H264MI_OK;
}

extern "C" int32_t h264mi_stream_output_order(h264mi_decoder *d, int32_t stream, int32_t *order, int32_t cap, int32_t *n) {
    if (!d || !n || stream < 0 || stream >= static_cast<int>(d->st.size()) || cap < 0 || (cap && !order)) return H264MI_EINVAL;
    const std::vector<OutFrame> &out = d->stage[d->exec].out[stream];
    std::vector<int> idx(out.size()), seq(out.size());
    int cur = 0;
    for (size_t i = 0; i < out.size(); i++) {
        if (i && out[i].new_sequence) cur++;
        idx[i] = static_cast<int>(i), seq[i] = cur;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return seq[a] != seq[b] ? seq[a] < seq[b] : out[a].poc < out[b].poc; });
    *n = static_cast<int32_t>(out.size());
    for (int i = 0; i < cap && i < static_cast<int>(idx.size()); i++) order[i] = idx[i];
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_read(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t crop, uint8_t *dst, size_t cap) {
    uint8_t *p;
    const OutFrame *of;
    int x0, y0, w, h;
    int r = frame_ptrs(d, stream, frame, &p, &of);
    if (r != H264MI_OK) return r;
    if (!dst || (stream == H264MI_STREAM_DERIVED && !crop)) return H264MI_EINVAL; // (only the display rectangle of a derived frame is written)
    GUARD(d);
    const int W = of->wmb * 16, H = of->hmb * 16;
    crop_rect(of, crop, &x0, &y0, &w, &h);
    if (cap < H264MI_I420_SIZE(w, h)) return H264MI_ECAPACITY;
    HIP_TRY(hipStreamSynchronize(d->stream));
    HIP_TRY(hipMemcpy2D(dst, w, p + static_cast<size_t>(y0) * W + x0, W, w, h, hipMemcpyDeviceToHost));
    const uint8_t *cb = p + static_cast<size_t>(W) * H, *cr = cb + static_cast<size_t>(W) * H / 4;
    const int wc = (w + 1) / 2, hc = (h + 1) / 2; // (odd only for monochrome streams: x0 + w <= W, so x0 / 2 + wc <= W / 2)
    uint8_t *o = dst + static_cast<size_t>(w) * h;
    HIP_TRY(hipMemcpy2D(o, wc, cb + static_cast<size_t>(y0 / 2) * (W / 2) + x0 / 2, W / 2, wc, hc, hipMemcpyDeviceToHost));
    o += static_cast<size_t>(wc) * hc;
    HIP_TRY(hipMemcpy2D(o, wc, cr + static_cast<size_t>(y0 / 2) * (W / 2) + x0 / 2, W / 2, wc, hc, hipMemcpyDeviceToHost));
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_colour(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t *matrix_coefficients, int32_t *video_full_range) {
    uint8_t *p;
    const OutFrame *of;
    int r = frame_ptrs(d, stream, frame, &p, &of);
    if (r != H264MI_OK) return r;
    if (matrix_coefficients) *matrix_coefficients = of->matrix_coefficients;
    if (video_full_range) *video_full_range = of->video_full_range;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_fields(h264mi_decoder *d, int32_t stream, int32_t frame, h264mi_field_info *out) {
    uint8_t *p;
    const OutFrame *of;
    int r = frame_ptrs(d, stream, frame, &p, &of);
    if (r != H264MI_OK) return r;
    if (!out) return H264MI_EINVAL;
    out->field_coded = of->field_coded, out->top_field_order_cnt = of->top_foc, out->bottom_field_order_cnt = of->bottom_foc, out->first_parity = of->first_parity;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_ref_pocs(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t slice, int32_t list, int32_t *cur_poc, int32_t *pocs, int32_t cap,
                                         int32_t *n) {
    if (!d || !n || cap < 0 || (cap && !pocs) || (list != 0 && list != 1) || stream == H264MI_STREAM_DERIVED) return H264MI_EINVAL;
    uint8_t *p;
    const OutFrame *of;
    int r = frame_ptrs(d, stream, frame, &p, &of);
    if (r != H264MI_OK) return r;
    if (of->field_coded) {
        set_error("frame %d of stream %d was coded as two field pictures: reference lists of field pictures are not reported", frame, stream);
        return H264MI_EUNSUPPORTED;
    }
    const Stage &g = d->stage[d->exec];
    int idx = -1;
    if (slice == -1) {
        if (!d->conceal || static_cast<size_t>(g.n_slices + of->pic) >= g.slice_refs.size()) { // no concealment: no pseudo-slice, no reference
            if (cur_poc) *cur_poc = of->pic >= 0 && static_cast<size_t>(of->pic) < g.pic_conceal_poc.size() ? g.pic_conceal_poc[of->pic].cur : of->poc;
            *n = 0;
            return H264MI_OK;
        }
        idx = g.n_slices + of->pic;
    } else {
        for (int i = 0; i < g.n_slices && idx < 0; i++)
            if (static_cast<int>(g.h_slices[i].pic_idx) == of->pic && g.h_slices[i].slice_in_pic == slice) idx = i;
        if (slice < 0 || idx < 0) {
            set_error("frame %d of stream %d has no slice %d", frame, stream, slice);
            return H264MI_EINVAL;
        }
    }
    const Stage::SliceRefs &sr = g.slice_refs[idx];
    if (cur_poc) *cur_poc = sr.cur_poc;
    *n = sr.n[list];
    for (int i = 0; i < sr.n[list] && i < cap; i++) pocs[i] = sr.poc[list][i];
    return cap < sr.n[list] ? H264MI_ECAPACITY : H264MI_OK;
}

extern "C" int32_t h264mi_frame_read_mbrecs(h264mi_decoder *d, int32_t stream, int32_t frame, uint8_t *rec, size_t cap) {
    if (!d || !rec || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    GUARD(d);
    Stage &g = d->stage[d->exec];
    for (int i = 0; i < g.n_pics; i++) {
        const PicDesc &pd = g.h_pics[i];
        if (static_cast<int>(pd.stream) == stream && static_cast<int>(pd.order) == frame) {
            size_t n = static_cast<size_t>(pd.wmb) * pd.hmb * sizeof(MbRec);
            if (cap < n) return H264MI_ECAPACITY;
            HIP_TRY(hipStreamSynchronize(d->stream));
            HIP_TRY(hipMemcpy(rec, d->d_mbrec[last_record_set(d)] + pd.mb_base, n, hipMemcpyDeviceToHost));
            return H264MI_OK;
        }
    }
    return H264MI_EINVAL;
}

extern "C" int32_t h264mi_frame_read_mbmv1(h264mi_decoder *d, int32_t stream, int32_t frame, uint8_t *mv1, size_t cap) {
    if (!d || !mv1 || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    GUARD(d);
    Stage &g = d->stage[d->exec];
    const int set = last_record_set(d);
    for (int i = 0; i < g.n_pics; i++) {
        const PicDesc &pd = g.h_pics[i];
        if (static_cast<int>(pd.stream) == stream && static_cast<int>(pd.order) == frame) {
            size_t n = static_cast<size_t>(pd.wmb) * pd.hmb * sizeof(MbMv1);
            if (cap < n) return H264MI_ECAPACITY;
            HIP_TRY(hipStreamSynchronize(d->stream));
            if (!pd.has_b || !d->d_mv1[set]) { // no B slice in the picture: there are no list-1 vectors
                memset(mv1, 0, n);
                return H264MI_OK;
            }
            HIP_TRY(hipMemcpy(mv1, d->d_mv1[set] + pd.mb_base, n, hipMemcpyDeviceToHost));
            return H264MI_OK;
        }
    }
    return H264MI_EINVAL;
}

#if defined(H264MI_TEST_HOOKS)
// ---- test and measurement hooks: built into libh264mi_hooks.so only (csrc/Makefile); the product library exports the ABI of include/h264mi.h and nothing else ----
// 1 while an output launch (K6 .. K9, mi_output.cpp) is recorded that the next pass has to wait for before it rewrites frames (last_pack), else 0
extern "C" int32_t h264mi_internal_pack_pending(h264mi_decoder *d, int32_t *pending) {
    if (!d || !pending) return H264MI_EINVAL;
    *pending = d->last_pack ? 1 : 0;
    return H264MI_OK;
}

// 1 while a side-information launch (K11) is recorded that the next pass's entropy stream has to wait for (last_side), else 0
extern "C" int32_t h264mi_internal_side_pending(h264mi_decoder *d, int32_t *pending) {
    if (!d || !pending) return H264MI_EINVAL;
    *pending = d->last_side ? 1 : 0;
    return H264MI_OK;
}

// Not part of the public ABI: fills every intermediate buffer (macroblock records, coefficient blocks, row state) with
// 0xFF so that a test can prove that no kernel depends on what an earlier batch -- or the allocator -- left there.
extern "C" int32_t h264mi_internal_poison(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    for (int i = 0; i < 2; i++) HIP_TRY(hipStreamSynchronize(d->ent_stream[i]));
    HIP_TRY(hipStreamSynchronize(d->rec_stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    for (int i = 0; i < MI_SETS; i++) {
        HIP_TRY(hipMemset(d->d_mbrec[i], 0xFF, sizeof(MbRec) * d->mb_cap));
        if (i == 0) HIP_TRY(hipMemset(d->d_coef[0], 0xFF, d->pool_blocks * 32 * MI_SETS));
        HIP_TRY(hipMemset(d->d_toprows[i], 0xFF, static_cast<size_t>(d->slices_cap) * (d->Wmax / 16) * MI_TOPROW_BYTES));
        if (d->d_mv1[i]) HIP_TRY(hipMemset(d->d_mv1[i], 0xFF, sizeof(MbMv1) * d->mb_cap));
    }
    if (d->d_colrec) HIP_TRY(hipMemset(d->d_colrec, 0xFF, sizeof(ColRec) * d->colrec_per_slot * d->n_slots * d->st.size()));
    HIP_TRY(hipDeviceSynchronize());
    return H264MI_OK;
}

// Not part of the public ABI: lets the CPU test-suite check the K5 launch plan (wavefronts, hand-off ring depth,
// dynamic LDS) without a GPU -- a wrong plan would deadlock the kernel, see mi_deblock8_plan().
extern "C" int32_t h264mi_internal_deblock_plan(int32_t wmb, int32_t hmb, int32_t *nwaves, int32_t *ring, int32_t *ring_last, int32_t *last_bufs, int64_t *lds_bytes) {
    if (!nwaves || !ring || !ring_last || !last_bufs || !lds_bytes || wmb < 1 || hmb < 1) return H264MI_EINVAL;
    int w = 1, r = 1, rl = 1, nb = 1;
    mi_deblock8_plan(wmb, hmb, &w, &r, &rl, &nb);
    *nwaves = w, *ring = r, *ring_last = rl, *last_bufs = nb, *lds_bytes = static_cast<int64_t>(mi_deblock8_lds_bytes(w, r, rl, nb));
    return H264MI_OK;
}

// Not part of the public ABI: which I/P entropy kernel a level 0 of n_cabac CABAC and n_cavlc CAVLC slices runs on (mi_entropy_kernel_choice):
// 0 k_entropy, 1 k_entropy_f, 2 k_entropy_c.
extern "C" int32_t h264mi_internal_entropy_kernel_choice(int32_t n_cabac, int32_t n_cavlc, int32_t slice_groups) {
    return mi_entropy_kernel_choice(n_cabac, n_cavlc, slice_groups != 0);
}

// Not part of the public ABI: which k_dbprep kernel runs on a level's pictures, n_has_b of them with B slices and n_save_col leaving a ColRec array
// (mi_dbprep_kernel_choice): 0 k_dbprep, 1 k_dbprep_ip.
extern "C" int32_t h264mi_internal_dbprep_kernel_choice(int32_t n_has_b, int32_t n_save_col) { return mi_dbprep_kernel_choice(n_has_b, n_save_col); }

// Not part of the public ABI: macroblock rows per wavefront of k_dbprep_ip for the launches to come (0: the rule, mi_dbprep_ip_rows) -- short test
// streams never have pictures enough for the rule to choose strips of more than one row
extern "C" int32_t h264mi_internal_set_dbprep_rows(h264mi_decoder *d, int32_t rows) {
    if (!d || rows < 0) return H264MI_EINVAL;
    d->dbprep_rows = rows;
    return H264MI_OK;
}
// ... and the rule itself
extern "C" int32_t h264mi_internal_dbprep_ip_rows(int32_t n_pics, int32_t wmb_max, int32_t hmb_max) { return mi_dbprep_ip_rows(n_pics, wmb_max, hmb_max); }

// Not part of the public ABI: the batch executed last once more through k_dbprep -- its records are still resident in its set --, over the same picture
// lists, into scratch buffers, and what the pass itself produced compared with that: the bytes of the DbPrm records of its pictures and of the intra mask
// that differ.  launches_ip / launches_generic: the k_dbprep_ip / k_dbprep launches of that pass.
extern "C" int32_t h264mi_internal_dbprep_check(h264mi_decoder *d, int32_t *launches_ip, int32_t *launches_generic, int64_t *mismatching_bytes) {
    if (!d || !launches_ip || !launches_generic || !mismatching_bytes || d->last_exec_stage < 0) return H264MI_EINVAL;
    GUARD(d);
    HIP_TRY(hipDeviceSynchronize());
    const Stage &g = d->stage[d->last_exec_stage];
    const int set = d->last_exec_set;
    *launches_ip = d->dbprep_launches[MI_DBPREP_K_IP], *launches_generic = d->dbprep_launches[MI_DBPREP_K_GENERIC];
    *mismatching_bytes = 0;
    if (!g.mb_used) return H264MI_OK;
    const size_t mask_bytes = sizeof(unsigned long long) * (g.mb_used / 64 + 2);
    DbPrm *prm = nullptr;
    unsigned long long *mask = nullptr;
    hipError_t e = hipMalloc(&prm, sizeof(DbPrm) * g.mb_used);
    if (e == hipSuccess) e = hipMalloc(&mask, mask_bytes);
    if (e == hipSuccess) e = hipMemset(prm, 0xA5, sizeof(DbPrm) * g.mb_used);
    if (e == hipSuccess) e = hipMemset(mask, 0, mask_bytes);
    for (size_t lv = 0; e == hipSuccess && lv < g.prep_n.size(); lv++)
        if (g.prep_n[lv]) {
            // (the ColRec arrays of save_col pictures are written once more, with the same bytes)
            hipLaunchKernelGGL(k_dbprep, dim3((g.mbs_max + MI_DBPREP_MBS - 1) / MI_DBPREP_MBS, (g.prep_n[lv] + 7u) & ~7u), dim3(256), 0, d->stream, g.d_lists + g.prep_off[lv],
                               g.d_pics, d->d_tables, d->d_mbrec[set], d->d_mv1[set], prm, 0, mask, static_cast<int>(g.prep_n[lv]));
            e = hipGetLastError();
        }
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    std::vector<uint8_t> a, b;
    auto differ = [&](const void *x, const void *y, size_t n) {
        a.resize(n), b.resize(n);
        if (e == hipSuccess) e = hipMemcpy(a.data(), x, n, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(b.data(), y, n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return;
        for (size_t i = 0; i < n; i++) *mismatching_bytes += a[i] != b[i];
    };
    for (size_t lv = 0; lv < g.prep_n.size(); lv++)
        for (uint32_t i = 0; i < g.prep_n[lv]; i++) {
            const PicDesc &pd = g.h_pics[g.h_lists[g.prep_off[lv] + i]];
            differ(d->d_dbprm[set] + pd.mb_base, prm + pd.mb_base, sizeof(DbPrm) * pd.wmb * pd.hmb);
        }
    differ(d->d_imask[set], mask, mask_bytes);
    if (prm) hipFree(prm);
    if (mask) hipFree(mask);
    if (e != hipSuccess) {
        set_error("h264mi_internal_dbprep_check failed: %s", hipGetErrorString(e));
        return H264MI_EDEVICE;
    }
    return H264MI_OK;
}

// Not part of the public ABI: the phase clocks a -DMI_DB_STATS build of the banded deblocking kernels leaves (zero otherwise); reading clears them
extern "C" int32_t h264mi_internal_deblock_phase_clocks(h264mi_decoder *d, uint32_t out[12]) {
    if (!d || !out) return H264MI_EINVAL;
    GUARD(d);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d->d_xctl + 64 + 8, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(d->d_xctl + 64 + 8, 0, 12 * sizeof(uint32_t)));
    return H264MI_OK;
}

// Not part of the public ABI: start and end (100 MHz ticks) of the row groups of the first picture of the last K5 launch (-DMI_DB_STATS builds)
extern "C" int32_t h264mi_internal_deblock_group_times(h264mi_decoder *d, uint32_t out[128]) { // [0..31] start / end per group, [32 + 8 g + i] when group g began step 16 i
    if (!d || !out) return H264MI_EINVAL;
    GUARD(d);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d->d_xctl + 64 + 32, 128 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return H264MI_OK;
}

// Not part of the public ABI: the banded launch plan of K5 / K3 (mi_deblock_bands, mi_intra_bands) for the CPU model test.
extern "C" int32_t h264mi_internal_band_plan(int32_t n_pics, int32_t wmb, int32_t hmb, int32_t max_wgs, int32_t *k5_bands, int32_t *k5_waves, int32_t *k5_ring,
                                             int64_t *k5_lds, int32_t *k3_bands, int32_t *k3_waves) {
    if (!k5_bands || !k5_waves || !k5_ring || !k5_lds || !k3_bands || !k3_waves || n_pics < 1 || wmb < 1 || hmb < 1) return H264MI_EINVAL;
    int nb = 1, nw = 1, ring = 1, b3 = 1, w3 = 1, roles = 1;
    mi_deblock_bands(n_pics, wmb, hmb, max_wgs, &nb, &nw, &ring, &roles);
    int wpr = 1;
    mi_intra_bands(n_pics, hmb, max_wgs, false, &b3, &w3, &wpr);
    // (the model test works on groups: the kernel runs `roles` wavefronts on each, which follow the same protocol side by side)
    *k5_bands = nb, *k5_waves = nw / roles, *k5_ring = ring, *k5_lds = static_cast<int64_t>(mi_deblock_lds_bytes_banded(nw, ring));
    *k3_bands = b3, *k3_waves = w3;
    return H264MI_OK;
}

// Not part of the public ABI: the epoch / ticket counters of the banded kernels set to a value shortly before their 32-bit wrap
// (tests/test_gpu_parity.py::test_gpu_banded_kernels_across_the_epoch_wrap)
extern "C" int32_t h264mi_internal_set_epoch(h264mi_decoder *d, uint32_t v) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    for (int i = 0; i < 2; i++) HIP_TRY(hipStreamSynchronize(d->ent_stream[i]));
    HIP_TRY(hipStreamSynchronize(d->rec_stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    d->x_epoch = d->x_tk5 = d->x_tk3 = v;
    // the device-side ticket counters stand where the host's bases do
    HIP_TRY(hipMemcpy(d->d_xctl, &d->x_tk5, sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->d_xctl + 32, &d->x_tk3, sizeof(uint32_t), hipMemcpyHostToDevice));
    return H264MI_OK;
}

// Not part of the public ABI: what picture management (8.2) made of the batch prepared last, for one stream, as text -- its pictures, slices
// (reference lists as raw entries, parity bit included) and output frames, then the frame slots that are references or held and the stream's
// POC / frame_num history (tools/host_dpb_trace.cpp; tests/test_host_dpb_trace.py pins the text).  Reads plain data only: it calls nothing of
// picture management, so a change of that code cannot change what it prints about the same state.  `len`: bytes the whole text needs (without
// the terminating 0); H264MI_ECAPACITY if that is more than cap - 1.
extern "C" int32_t h264mi_internal_dpb_trace(h264mi_decoder *d, int32_t stream, char *buf, size_t cap, size_t *len) {
    if (!d || !buf || !len || !cap || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    const Stage &g = d->stage[d->prep];
    const StreamState &s = d->st[stream];
    size_t n = 0;
    auto put = [&](const char *fmt, auto... args) {
        const int k = snprintf(n < cap ? buf + n : nullptr, n < cap ? cap - n : 0, fmt, args...);
        if (k > 0) n += static_cast<size_t>(k);
    };
    auto put_list = [&](const char *name, const int16_t *v, int count) {
        put(" %s=", name);
        for (int i = 0; i < count && i < MI_MAX_REFS; i++) put(i ? ",%d" : "%d", v[i]);
    };
    for (int p = 0; p < g.n_pics; p++) {
        const PicDesc &pd = g.h_pics[p];
        if (static_cast<int>(pd.stream) != stream) continue;
        const Slot &sl = s.dpb.slots[pd.slot];
        put("pic %d slot=%u field=%d poc=%d fpoc=%d,%d frame_num=%d wave=%d level=%d conceal_ref=%d n_slices=%u dropped=%d\n", p, pd.slot, pd.field, sl.poc, sl.fpoc[0], sl.fpoc[1],
            sl.frame_num, g.pic_wave[p], g.pic_level[p], pd.conceal_ref, pd.n_slices, g.pic_dropped[p]);
    }
    for (int i = 0; i < g.n_slices; i++) {
        const SliceDesc &sd = g.h_slices[i];
        if (static_cast<int>(g.h_pics[sd.pic_idx].stream) != stream) continue;
        put("slice pic=%u first_mb=%u type=%d fill_from=%u end_mb=%u", sd.pic_idx, sd.first_mb, sd.slice_type, sd.fill_from, sd.end_mb);
        put_list("l0", sd.ref_slot, sd.num_ref_idx_active);
        if (sd.slice_type == 1) {
            const BSliceExt &bx = g.h_bext[sd.bext];
            put_list("l1", bx.ref_slot1, bx.num_ref_idx_l1_active);
            put_list("dist_scale", bx.dist_scale, sd.num_ref_idx_active);
            put(" col_short=%d", bx.col_short);
        }
        put("%s", "\n");
    }
    for (const OutFrame &o : g.out[stream])
        put("out slot=%d wmb=%d hmb=%d crop=%d,%d size=%dx%d poc=%d frame_num=%d nal_ref_idc=%d idr=%d pic=%d new_sequence=%d pic2=%d\n", o.slot, o.wmb, o.hmb, o.crop_x, o.crop_y,
            o.width, o.height, o.poc, o.frame_num, o.nal_ref_idc, o.idr, o.pic, o.new_sequence, o.pic2);
    for (size_t i = 0; i < s.dpb.slots.size(); i++) {
        const Slot &sl = s.dpb.slots[i];
        if (sl.ref || sl.held)
            put("slot %zu ref=%d long_idx=%d frame_num=%d fields=%d funref=%d nonexisting=%d field_coded=%d poc=%d held=%d\n", i, sl.ref, sl.long_idx, sl.frame_num, sl.fields,
                sl.funref, sl.nonexisting, sl.field_coded, sl.poc, sl.held);
    }
    put("state prev_ref_frame_num=%d prev_poc_msb=%d prev_poc_lsb=%d prev_frame_num=%d prev_frame_num_offset=%d pend_slot=%d need_idr=%d\n", s.dpb.prev_ref_frame_num, s.dpb.prev_poc_msb,
        s.dpb.prev_poc_lsb, s.dpb.prev_frame_num, s.dpb.prev_frame_num_offset, s.dpb.pend_slot, s.need_idr);
    *len = n;
    if (n >= cap) return H264MI_ECAPACITY;
    return H264MI_OK;
}
#endif /* H264MI_TEST_HOOKS */
