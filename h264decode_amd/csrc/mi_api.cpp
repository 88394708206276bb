// h264decode_amd/csrc/mi_api.cpp -- the C ABI of libh264mi.so (include/h264mi.h) outside a batch: the device tables, the thin parser exports, init,
// create / destroy / reset, the counters, and the read-back and query calls of the frame accessors.  What a slice NAL does to the picture under
// construction is mi_picture.cpp (NAL dispatch h264/server.go:113-166; asking mi_dpb.cpp -- picture management 8.2 -- for slots, counts and lists);
// prepare, the GPU launch sequence and sync are mi_batch.cpp; the output stage (K6 .. K11) is mi_output.cpp; test hooks and measurement switches are
// mi_hooks.cpp.  The decoder's state, which all of them work on, is mi_decoder.hpp.
//
// There is deliberately NO CPU pixel path in this library: every sample is produced by the HIP
// kernels of the k_*.hip files (decoded by k_entropy / k_recon / k_inter / k_deblock, brought into the caller's
// layout by k_pack and the rest of the output stage).  If no device is usable the create call fails (H264MI_ENODEVICE).
#include <hip/hip_runtime.h>
#include <algorithm>
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
void build_vlc(uint16_t *c, int *mismatches) {
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
void build_scaling(const uint8_t s4[6][16], const uint8_t s8[2][64], ScalingSet *o) { // 8.5.9
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
    auto each = [](auto release, auto... ps) { ((ps ? (void)release(ps) : (void)0), ...); }; // release(p) for every p that is set
    for (Stage &g : d->stage) {
        each(hipFree, g.d_bits, g.d_slices, g.d_pics, g.d_status, g.d_lists, g.d_bext, g.d_dpoc, g.d_cmap);
        each(hipHostFree, g.h_bits, g.h_slices, g.h_pics, g.h_status, g.h_lists, g.h_bext, g.h_dpoc, g.h_cmap);
        each(hipEventDestroy, g.ev_upload, g.ev_done);
    }
    for (int i = 0; i < MI_SETS; i++) {
        each(hipFree, d->d_mbrec[i], d->d_mv1[i], d->d_dbprm[i], d->d_imask[i], d->d_toprows[i]);
        each(hipEventDestroy, d->ev_ent[i], d->ev_col[i], d->ev_rec[i]);
    }
    each(hipStreamDestroy, d->ent_stream[0], d->ent_stream[1], d->rec_stream);
    for (DescTables &t : d->tables) each(hipFree, t.d[0], t.d[1]), each(hipHostFree, t.h[0], t.h[1]), each(hipEventDestroy, t.ev[0], t.ev[1]);
    each(hipFree, d->d_coef[0], d->d_pool_head, d->d_colrec, d->d_backfill, d->d_xring, d->d_xdone, d->d_xctl, d->d_pools, d->d_derived, d->hist[HIST_DEINT].arena, d->hist[HIST_STATS].arena, d->d_jpeg_ivl, d->d_frames, d->d_tables);
    each(hipHostFree, d->h_xstatus, d->h_tables);
    each(hipEventDestroy, d->ev_user);
    for (auto e : d->ev) hipEventDestroy(e);
    if (d->own_stream && d->stream) hipStreamDestroy(d->stream);
}

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
        d->n_cus = ncu;
        int ent_cus = 0;
        hook_create_entropy(d, &ent_cus);
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
            // (h264mi_decoder_coef_pool reports the largest of the MI_SETS heads: those of sets that have not run yet must read 0, not what the allocation held)
            TRY_ALLOC(hipMemset(d->d_pool_head, 0, sizeof(uint32_t) * MI_SETS));
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
    hook_create_k5(d);
    hook_create_pass_group(d);
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
        if (r != H264MI_OK) return fail(r);
    }
    *out = d;
    return H264MI_OK;
}

extern "C" int32_t h264mi_decoder_destroy(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    (void)drain(d);
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
void reset_stream(StreamState &s, bool keep_parameter_sets) {
    s.dpb.reset();
    s.epoch++;
    s.cur_pic = -1, s.cur_slices = 0;
    s.n_pics_in_batch = 0;
    s.pending_drops = 0;
    s.ref_seq = StreamState::RefSeq();
    s.sei = {0, 0, 0, 0, 0}, s.decoded_any = s.lead = s.skipping = false; // random access: the stream waits for an entry point again
    if (!keep_parameter_sets) {
        s.ra = {0, 0, 0};
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
    for (HistorySet &hs : d->hist)
        for (FrameHistory &fh : hs.slots) fh.valid = false;
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
    for (HistorySet &hs : d->hist)
        if (stream < static_cast<int>(hs.slots.size())) hs.slots[stream].valid = false;
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
extern "C" int32_t h264mi_decoder_set_random_access(h264mi_decoder *d, int32_t mode) {
    if (!d || (mode != H264MI_RA_OFF && mode != H264MI_RA_RECOVERY_POINT)) return H264MI_EINVAL;
    d->random_access = mode == H264MI_RA_RECOVERY_POINT;
    return H264MI_OK;
}
extern "C" int32_t h264mi_sei_recovery_point(const uint8_t *nal, size_t n, h264mi_recovery_point *out) { return sei_recovery_point(nal, n, out); }
extern "C" int32_t h264mi_stream_random_access_stats(h264mi_decoder *d, int32_t stream, h264mi_random_access_stats *s) {
    if (!d || !s || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL; // (H264MI_STREAM_DERIVED too)
    *s = d->st[stream].ra;
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

extern "C" int32_t h264mi_slice_starts_picture(const h264mi_sps *sps, const h264mi_slice_header *prev, const h264mi_slice_header *cur) {
    if (!sps || !prev || !cur) return H264MI_EINVAL;
    return new_picture(*sps, *prev, *cur) ? 1 : 0;
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
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
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
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
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
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
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
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
    if (matrix_coefficients) *matrix_coefficients = of->matrix_coefficients;
    if (video_full_range) *video_full_range = of->video_full_range;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_fields(h264mi_decoder *d, int32_t stream, int32_t frame, h264mi_field_info *out) {
    uint8_t *p;
    const OutFrame *of;
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
    if (!out) return H264MI_EINVAL;
    out->field_coded = of->field_coded, out->top_field_order_cnt = of->top_foc, out->bottom_field_order_cnt = of->bottom_foc, out->first_parity = of->first_parity;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_entry(h264mi_decoder *d, int32_t stream, int32_t frame, h264mi_frame_entry_info *info) {
    if (!info || stream == H264MI_STREAM_DERIVED) return H264MI_EINVAL;
    uint8_t *p;
    const OutFrame *of;
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
    info->recovery_point = of->rp.found, info->recovery_frame_cnt = of->rp.recovery_frame_cnt, info->exact_match_flag = of->rp.exact_match_flag;
    info->broken_link_flag = of->rp.broken_link_flag, info->changing_slice_group_idc = of->rp.changing_slice_group_idc, info->entry = of->entry;
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_ref_pocs(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t slice, int32_t list, int32_t *cur_poc, int32_t *pocs, int32_t cap,
                                         int32_t *n) {
    if (!d || !n || cap < 0 || (cap && !pocs) || (list != 0 && list != 1) || stream == H264MI_STREAM_DERIVED) return H264MI_EINVAL;
    uint8_t *p;
    const OutFrame *of;
    if (const int r = frame_ptrs(d, stream, frame, &p, &of)) return r;
    if (of->field_coded) {
        set_error("frame %d of stream %d was coded as two field pictures: reference lists of field pictures are not reported", frame, stream);
        return H264MI_EUNSUPPORTED;
    }
    const Stage &g = d->stage[d->exec];
    int idx = -1;
    if (slice == -1) {
        if (!d->conceal || static_cast<size_t>(g.n_slices + of->pic) >= g.slices.size()) { // no concealment: no pseudo-slice, no reference
            if (cur_poc) *cur_poc = of->pic >= 0 && of->pic < g.n_pics ? g.pics[of->pic].conceal_poc.cur : of->poc;
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
    const Stage::SliceRefs &sr = g.slices[idx].refs;
    if (cur_poc) *cur_poc = sr.cur_poc;
    *n = sr.n[list];
    for (int i = 0; i < sr.n[list] && i < cap; i++) pocs[i] = sr.poc[list][i];
    return cap < sr.n[list] ? H264MI_ECAPACITY : H264MI_OK;
}

// picture `order` (in decoding order) of stream `stream` in the batch executed last, or nullptr
static const PicDesc *find_picture(const h264mi_decoder *d, int stream, int order) {
    const Stage &g = d->stage[d->exec];
    for (int i = 0; i < g.n_pics; i++)
        if (static_cast<int>(g.h_pics[i].stream) == stream && static_cast<int>(g.h_pics[i].order) == order) return &g.h_pics[i];
    return nullptr;
}

extern "C" int32_t h264mi_frame_read_mbrecs(h264mi_decoder *d, int32_t stream, int32_t frame, uint8_t *rec, size_t cap) {
    if (!d || !rec || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    GUARD(d);
    const PicDesc *pd = find_picture(d, stream, frame);
    if (!pd) return H264MI_EINVAL;
    const size_t n = static_cast<size_t>(pd->wmb) * pd->hmb * sizeof(MbRec);
    if (cap < n) return H264MI_ECAPACITY;
    HIP_TRY(hipStreamSynchronize(d->stream));
    HIP_TRY(hipMemcpy(rec, d->d_mbrec[last_record_set(d)] + pd->mb_base, n, hipMemcpyDeviceToHost));
    return H264MI_OK;
}

extern "C" int32_t h264mi_frame_read_mbmv1(h264mi_decoder *d, int32_t stream, int32_t frame, uint8_t *mv1, size_t cap) {
    if (!d || !mv1 || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    GUARD(d);
    const int set = last_record_set(d);
    const PicDesc *pd = find_picture(d, stream, frame);
    if (!pd) return H264MI_EINVAL;
    const size_t n = static_cast<size_t>(pd->wmb) * pd->hmb * sizeof(MbMv1);
    if (cap < n) return H264MI_ECAPACITY;
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (!pd->has_b || !d->d_mv1[set]) { // no B slice in the picture: there are no list-1 vectors
        memset(mv1, 0, n);
        return H264MI_OK;
    }
    HIP_TRY(hipMemcpy(mv1, d->d_mv1[set] + pd->mb_base, n, hipMemcpyDeviceToHost));
    return H264MI_OK;
}
