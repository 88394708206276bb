// h264decode_amd/csrc/mi_kernels.h -- kernel entry points (HIP, gfx950) and launch helpers.
#pragma once
#include <hip/hip_runtime.h>
#include "mi_types.h"

// K1/K2: one slice per wavefront.  grid = #slices, block = 64; toprows = 12 dwords per MB column per slice.
extern "C" __global__ void k_entropy(const SliceDesc *slices, const PicDesc *pics, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, int16_t *coefs,
                                     uint32_t *pool_head, uint32_t pool_blocks, uint32_t *status, uint32_t *toprows, int wmb_max, uint32_t slice_base);
// the same with the slice-group walk of 8.2.2 (k_entropy_f.hip): for launches that hold a picture with more than one slice group
extern "C" __global__ void k_entropy_f(const SliceDesc *slices, const PicDesc *pics, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, int16_t *coefs,
                                       uint32_t *pool_head, uint32_t pool_blocks, uint32_t *status, uint32_t *toprows, int wmb_max, uint32_t slice_base);
// the same with the entropy coding mode fixed to CABAC (k_entropy_c.hip): for launches whose slices are all CABAC-coded
extern "C" __global__ void k_entropy_c(const SliceDesc *slices, const PicDesc *pics, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, int16_t *coefs,
                                       uint32_t *pool_head, uint32_t pool_blocks, uint32_t *status, uint32_t *toprows, int wmb_max, uint32_t slice_base);
// the CABAC-only kernel with transform_8x8_mode = 0 and 4:2:0 fixed as well (k_entropy_m.hip): for all-CABAC launches of batches without an 8x8 or monochrome picture
extern "C" __global__ void k_entropy_m(const SliceDesc *slices, const PicDesc *pics, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, int16_t *coefs,
                                       uint32_t *pool_head, uint32_t pool_blocks, uint32_t *status, uint32_t *toprows, int wmb_max, uint32_t slice_base);
// the same for B slices (k_entropy_b.hip): two reference lists, direct prediction from the ColRec array of RefPicList1[0]; toprows = 18 dwords per column
extern "C" __global__ void k_entropy_b(const SliceDesc *slices, const PicDesc *pics, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, int16_t *coefs,
                                       uint32_t *pool_head, uint32_t pool_blocks, uint32_t *status, uint32_t *toprows, int wmb_max, uint32_t slice_base,
                                       const BSliceExt *bexts, MbMv1 *mbmv1);
#define MI_TOPROW_BYTES 72 /* per macroblock column per slice (the B kernel's TopInfo; the I/P kernel uses 48 of them) */
#ifndef MI_K4_WG
#define MI_K4_WG 1 /* wavefronts (groups of four macroblocks) per workgroup of k_inter / k_inter_b: grid = ceil(n_blocks / MI_K4_WG) rounded up to a multiple of 8 (measured: 2 and 4 are slower, profiles/r05_k4_budget.txt) */
#endif
// K4 (k_inter.hip): inter macroblocks of a set of pictures (one per stream), one lane per 4x4 block, four macroblocks per wavefront.
// n_blocks = #pictures << groups_per_pic_log2 (groups of four macroblocks per picture, rounded up to a power of two: no division in the kernel);
// grid = n_blocks rounded up to a multiple of 8 (XCD-aware block order), block = 64
extern "C" __global__ void k_inter(const uint32_t *pic_list, const PicDesc *pics, const SliceDesc *slices, const DevTables *tab, const MbRec *mbrec, const int16_t *coefs,
                                   int groups_per_pic_log2, int n_blocks);
// K4 for pictures with B slices: two lists per block (MbRec::refslot1, MbMv1), default / explicit / implicit weighting
extern "C" __global__ void k_inter_b(const uint32_t *pic_list, const PicDesc *pics, const SliceDesc *slices, const DevTables *tab, const MbRec *mbrec,
                                     const int16_t *coefs, int groups_per_pic_log2, int n_blocks, const BSliceExt *bexts, const MbMv1 *mbmv1);
// K3: intra macroblocks, one workgroup per picture, one wavefront per macroblock row (2-D wavefront order).
extern "C" __global__ void k_intra(const uint32_t *pic_list, const PicDesc *pics, const FramePool *pools, const DevTables *tab, const MbRec *mbrec,
                                   const int16_t *coefs, const unsigned long long *intramask);
// K3 spread over `nbands` workgroups per picture: grid = pictures * nbands, block = 64 * wavefronts per band (<= MI_INTRA_WAVES);
// xdone: pictures * nbands * wmb_max flag words; epoch / ticket as for k_deblock_x
extern "C" __global__ void k_intra_x(const uint32_t *pic_list, const PicDesc *pics, const FramePool *pools, const DevTables *tab, const MbRec *mbrec,
                                     const int16_t *coefs, uint32_t *xdone, uint32_t epoch, int nbands, uint32_t *ticket, uint32_t ticket_base, int wmb_max,
                                     uint32_t *xstatus, int waves_per_row, const unsigned long long *intramask);
// k_dbprep (k_dbprep.hip): boundary strengths + alpha / beta / tC0 of every macroblock of a batch (DbPrm), so that K5 -- one serial dependency chain per
// picture -- has none of that work in its steps, and K3's work list (one bit per intra or undelivered macroblock).  Two kernels write the same bytes:
//   k_dbprep     any picture: one or two reference lists; for the pictures flagged PicDesc::save_col also their ColRec array (the motion later B
//                pictures take their direct prediction from); col_only: the one-off ColRec back-fill.  16 lanes per macroblock.
//                grid = (ceil(mbs_max / MI_DBPREP_MBS), pictures of the list rounded up to a multiple of 8), block = 256.
//   k_dbprep_ip  launches without a picture that has B slices or leaves a ColRec array (mi_dbprep_kernel_choice): one lane per macroblock, one wavefront
//                per strip of 64 macroblock columns x `rows` macroblock rows (mi_dbprep_ip_rows).
//                grid = (ceil(wmb_max / 64) * ceil(hmb_max / rows), pictures of the list rounded up to a multiple of 8), block = 64.
#ifndef MI_DBPREP_MBS
#define MI_DBPREP_MBS 64
#endif
extern "C" __global__ void k_dbprep(const uint32_t *pic_list, const PicDesc *pics, const DevTables *tab, const MbRec *mbrec, const MbMv1 *mbmv1, DbPrm *out, int col_only, unsigned long long *intramask, int n_pics);
extern "C" __global__ void k_dbprep_ip(const uint32_t *pic_list, const PicDesc *pics, const DevTables *tab, const MbRec *mbrec, DbPrm *out, unsigned long long *intramask, int n_pics,
                                       int chunks, int rows);
// k_conceal (k_conceal.hip): error concealment -- between a level's entropy launch and its k_dbprep, the lost macroblocks of the concealable pictures of
// the list (MBT_NONE records; every macroblock of a slice with a non-zero status) become zero-vector P_Skip records that point at PicDesc::conceal_ref
// and at the picture's concealment SliceDesc (slices[conceal_base + picture]).  grid = pictures of the list, block = 256.
// cmap: [picture] -> start, within cmap, of the picture's slice indices; cstat: [p] concealed macroblocks of picture p
extern "C" __global__ void k_conceal(const uint32_t *pic_list, const PicDesc *pics, const SliceDesc *slices, const uint32_t *cmap, uint32_t conceal_base,
                                     const uint32_t *status, const uint8_t *bitstream, const DevTables *tab, MbRec *mbrec, MbMv1 *mbmv1, uint32_t *cstat);
// K5 (k_deblock.hip): in-loop deblocking, one workgroup per picture, one wavefront per group of 8 macroblock rows, 8 lanes per macroblock
// (two lines per lane, packed 16-bit arithmetic).  block = 64 * nwaves, dynamic LDS = mi_deblock8_lds_bytes(nwaves, ring, ring_last, last_bufs);
// (nwaves, ring, ring_last, last_bufs) from mi_deblock8_plan()
// xstatus: a wavefront that gives up waiting for its neighbour (4 s) leaves a code there; a -DMI_DB_STATS build adds the phase clocks of its step loop to xstatus[8..19]
extern "C" __global__ void k_deblock(const uint32_t *pic_list, const PicDesc *pics, const DbPrm *dbprm, int ring, int ring_last, int last_bufs, uint32_t *xstatus);
#define MI_DEBLOCK8_MAX_WAVES 8      /* 512 threads: two wavefronts on a SIMD, up to 256 VGPRs each (the kernel holds 84 of them as landing registers of its loads) */
#define MI_DEBLOCK8_MAX_GROUPS 64    /* hmb <= 320 + slack */
#define MI_DEBLOCK8_HDR_BYTES 512    /* sizeof(Db8Shared) */
#define MI_DEBLOCK8_TILE_BYTES 1568  /* the LDS window of a sub-row: four macroblock columns of luma (1024) and chroma (512) + 32 (bank stagger) */
#define MI_DEBLOCK8_WAVE_BYTES (9 * MI_DEBLOCK8_TILE_BYTES + 2 * 8 * 80) /* 8 sub-rows + rows 12..15 of the row above the first; the DbPrm stage (two steps x 8 macroblocks) */
static inline size_t mi_deblock8_lds_bytes(int nwaves, int ring, int ring_last, int last_bufs) {
    return MI_DEBLOCK8_HDR_BYTES + static_cast<size_t>(nwaves) * MI_DEBLOCK8_WAVE_BYTES + (static_cast<size_t>(nwaves - 1) * ring + static_cast<size_t>(ring_last) * last_bufs) * 96;
}
// K5 spread over `nbands` workgroups per picture (k_deblock_x.hip): grid = pictures * nbands, block = 64 * (largest band's group count),
// dynamic LDS = mi_deblock_lds_bytes_banded().  xring: pictures * nbands * wmb_max * 24 granules of 8 bytes; epoch: a value no earlier
// launch on this ring has used (never 0); ticket / ticket_base: a counter that only ever grows and its value before this launch.
extern "C" __global__ void k_deblock_x(const uint32_t *pic_list, const PicDesc *pics, const DbPrm *dbprm, int ring, int ring_last, int last_bufs,
                                       unsigned long long *xring, uint32_t epoch, int nbands, uint32_t *ticket, uint32_t ticket_base, int wmb_max, uint32_t *xstatus,
                                       int roles);
#ifndef MI_DEBLOCK_MAX_WAVES
#define MI_DEBLOCK_MAX_WAVES 12    /* the banded kernel: LDS: 6 KB of row state per wavefront + its hand-off ring */
#endif
#define MI_DEBLOCK_HDR_BYTES 1552  /* sizeof(DbShared) rounded up to 16 */
#define MI_DEBLOCK_WAVE_BYTES 4800 /* 4 sub-rows: sample tiles, the macroblock's DbPrm, the bottom rows for the sub-row below */
#define MI_DEBLOCK_SLOT_BYTES 96
#define MI_DEBLOCK_LDS_MAX (160 * 1024)
// banded builds: one ring region per wavefront (the last one stages what goes to the global ring) + the staging slot of the band above
static inline size_t mi_deblock_lds_bytes_banded(int nwaves, int ring, int wave_bytes = MI_DEBLOCK_WAVE_BYTES) {
    return MI_DEBLOCK_HDR_BYTES + static_cast<size_t>(nwaves) * wave_bytes + (static_cast<size_t>(nwaves) * ring + 1) * MI_DEBLOCK_SLOT_BYTES;
}
// How a launch of n_pics pictures of up to wmb x hmb macroblocks is spread over the chip.  nbands = 1: the one-workgroup kernels.
// Otherwise every band is one round of at most MI_DEBLOCK_MAX_WAVES groups, and pictures * bands stays within `max_wgs`
// workgroups (all of them can be resident at once; the ticket order makes the hand-off safe even if they are not).
static inline void mi_deblock_bands(int n_pics, int wmb, int hmb, int max_wgs, int *nbands, int *nwaves, int *ring, int *roles) {
    const int ngroups = (hmb + 3) / 4;
    int nb = n_pics > 0 ? max_wgs / n_pics : 1;
    if (nb > ngroups) nb = ngroups;
    if (nb < 2 || (ngroups + nb - 1) / nb > MI_DEBLOCK_MAX_WAVES) nb = 1;
    const int per_band = (ngroups + nb - 1) / nb;
    // two wavefronts per group (luma | chroma) while every wavefront of the launch can still have a SIMD to itself (1024 of them)
    *roles = (nb > 1 && 2 * per_band <= MI_DEBLOCK_MAX_WAVES && 2 * n_pics * ngroups <= 1280) ? 2 : 1;
    *nbands = nb;
    *nwaves = per_band * *roles;
    *ring = wmb < 16 ? (wmb > 0 ? wmb : 1) : 16;
}
// Wavefront count and hand-off ring depths of k_deblock for pictures of wmb x hmb macroblocks.  Wavefront w runs the 8-row groups
// w, w + nwaves, ...; group g hands rows 12..15 of its last macroblock row to group g + 1 through the ring region of its wavefront.  A group may
// run at most `depth` columns ahead of the group below it.  Groups of one round run side by side, 8 steps apart, so a
// short ring is enough between them; but the reader of the LAST wavefront's groups is wavefront 0 in the NEXT round, which
// only starts when it has finished a whole row -- that ring (ring_last) holds a whole row, otherwise the last wavefront
// (and through back-pressure every wavefront above it) would wait for wavefront 0.  From three rounds on that ring is
// double-buffered by round: the last wavefront's group of round r must not wait until wavefront 0 has read ALL of round
// r - 1's ring, because wavefront 0's group of round r can only finish when the groups below it -- up to the last
// wavefront's, through the short rings -- make progress: with a single buffer wide pictures deadlock.  As many wavefronts as fit.
// 1080p (120 x 68): 9 groups on 8 wavefronts (MI_DEBLOCK8_MAX_WAVES), two rounds -- the ninth group is wavefront 0's second --, so ring_last = wmb.
static inline void mi_deblock8_plan(int wmb, int hmb, int *nwaves, int *ring, int *ring_last, int *last_bufs, int max_waves = MI_DEBLOCK8_MAX_WAVES) {
    const int ngroups = (hmb + 7) / 8;
    const int w1 = wmb > 0 ? wmb : 1;
    for (int nw = ngroups < max_waves ? ngroups : max_waves; nw >= 1; nw--) {
        const int rounds = (ngroups + nw - 1) / nw;
        const int r = w1 < 16 ? w1 : 16;
        const int rl = rounds > 1 ? w1 : r;
        const int nb = rounds > 2 ? 2 : 1;
        if (mi_deblock8_lds_bytes(nw, r, rl, nb) <= MI_DEBLOCK_LDS_MAX) {
            *nwaves = nw, *ring = r, *ring_last = rl, *last_bufs = nb;
            return;
        }
    }
    *nwaves = 1, *ring = 1, *ring_last = w1, *last_bufs = 2; // 2 x 512 columns x 96 bytes + one wavefront always fit
}
// Which build of the I/P entropy kernel level 0 of a batch runs on: the slice-group build if a picture of the batch has slice groups (it reads the
// mode per slice); else the CABAC-only build if every slice of the level is CABAC-coded; else -- one CAVLC slice is enough -- the general one.
// (An empty level 0, a batch of B slices only, launches nothing: any id will do.)  Of the CABAC-only builds the Main one, when no picture of the batch
// has the 8x8 transform switched on (PicDesc::t8x8_mode) or is monochrome (n_t8x8_mono, known when the batch is prepared like the slices' modes): every
// Main stream, and every High stream whose PPS leaves transform_8x8_mode_flag off; one such picture sends the launch to the CABAC-only kernel.
enum { MI_ENT_K_GENERAL = 0, MI_ENT_K_FMO = 1, MI_ENT_K_CABAC = 2, MI_ENT_K_MAIN = 3 };
static inline int mi_entropy_kernel_choice(int n_cabac, int n_cavlc, bool slice_groups, int n_t8x8_mono) {
    if (slice_groups) return MI_ENT_K_FMO;
    if (n_cavlc != 0 || n_cabac <= 0) return MI_ENT_K_GENERAL;
    return n_t8x8_mono == 0 ? MI_ENT_K_MAIN : MI_ENT_K_CABAC;
}
// Wavefronts of an I/P entropy build that a SIMD holds (amdgpu_waves_per_eu of the build: 512 VGPRs / 80, the slice-group build 512 / 102): with the
// chip's CUs x 4 SIMDs the resident capacity that mi_pass_group compares a launch with.
static inline int mi_entropy_waves_per_simd(int ent_kernel) { return ent_kernel == MI_ENT_K_FMO ? 5 : 6; }
// Pass groups: how many consecutive passes over a batch release their entropy stages together (execute_stage: the gate), 0 = every pass on its own,
// behind the reconstruction of pass n - MI_SETS only.  A level-0 launch of more slices than the chip holds wavefronts (capacity) runs a second,
// underfilled round, and while it runs no reconstruction workgroup becomes resident ("Pass pipeline"): there the stages of
// consecutive passes time-slice, and two entropy launches side by side fill each other's tail.  Not grouped: a launch that fits (its slice chains
// already overlap across passes) and a batch with B slices (its levels are fenced between passes).  pics_per_launch (the batch's mean pictures per
// reconstruction launch) decides nothing yet: no measurement has shown banded launches -- few pictures, each spread over several workgroups -- losing
// behind a group.  The group may not be larger than MI_SETS: the gate is an event of a record set.
#define MI_PASS_GROUP_DEFAULT 2
static inline int mi_pass_group(int n_slices0, int capacity, int pics_per_launch, bool has_b) {
    (void)pics_per_launch;
    if (has_b || capacity <= 0 || n_slices0 <= capacity) return 0;
    return MI_PASS_GROUP_DEFAULT;
}
// Which k_dbprep kernel runs on the pictures complete with a level: the one-lane-per-macroblock kernel if none of them has B slices (n_has_b) and none
// leaves a ColRec array (n_save_col); else -- one such picture is enough -- the general one.
enum { MI_DBPREP_K_GENERIC = 0, MI_DBPREP_K_IP = 1 };
static inline int mi_dbprep_kernel_choice(int n_has_b, int n_save_col) { return (n_has_b == 0 && n_save_col == 0) ? MI_DBPREP_K_IP : MI_DBPREP_K_GENERIC; }
// Macroblock rows per wavefront of k_dbprep_ip.  A wavefront that walks down its strip takes a row's upper neighbours from its own registers, so the
// higher the strips, the fewer records are fetched twice -- whole columns once the launch has wavefronts enough without cutting them (twice the 4096
// the chip holds at four per SIMD); a launch of few pictures is cut into as many strips as that takes, down to single rows.
#define MI_DBPREP_IP_WAVES 8192
static inline int mi_dbprep_ip_rows(int n_pics, int wmb_max, int hmb_max) {
    const long columns = static_cast<long>(n_pics > 0 ? n_pics : 1) * ((wmb_max + 63) / 64 > 0 ? (wmb_max + 63) / 64 : 1);
    long bands = (MI_DBPREP_IP_WAVES + columns - 1) / columns; // strips per column the target asks for
    if (bands > hmb_max) bands = hmb_max;
    if (bands < 1) bands = 1;
    return static_cast<int>((hmb_max + bands - 1) / bands);
}
// K6: crop + tight pack of a list of frames into I420; grid = (frames, ceil((h_max + 2 * ceil(h_max / 2)) / rows_per_block)), block = 256
typedef struct {
    uint64_t src;     // Y plane of the frame (coded size W x H; Cb at + W*H, Cr at + W*H*5/4)
    uint64_t dst_off; // byte offset of the packed frame in the destination buffer
    uint32_t W, H, x0, y0, w, h;
} PackDesc;
extern "C" __global__ void k_pack(const PackDesc *descs, uint8_t *dst, int rows_per_block);
// K7 (k_convert.hip): crop + convert a list of frames to NV12 / RGB24 / planar RGB by the integer rule of include/h264mi.h;
// grid = (frames, ceil(ceil(h_max / 2) / pairs_per_block)), block = 256; a thread owns two luma rows x 16 columns
typedef struct {
    uint64_t src;     // as PackDesc
    uint64_t dst_off; // byte offset of the converted frame in the destination buffer
    uint32_t W, H, x0, y0, w, h;
    uint32_t format;   // H264MI_FMT_NV12 / _RGB24 / _RGBP
    uint32_t cset;     // row of the coefficient table: 2 * (matrix - 1) + full range (unused for NV12)
    uint32_t bilinear; // chroma upsampling: 0 nearest, 1 bilinear (unused for NV12)
    uint32_t pad;
} ConvDesc;
extern "C" __global__ void k_convert(const ConvDesc *descs, uint8_t *dst, int pairs_per_block);
// K8 (k_scale.hip): crop + scale a list of frames to ONE output size ow x oh + convert, by the integer rule of include/h264mi.h ("Scaled output");
// grid = (frames, ceil(ceil(oh / 2) / pairs_per_block)), block = 256; a thread owns two OUTPUT luma rows x 16 columns and the chroma under them
typedef struct {
    uint64_t src;     // as PackDesc
    uint64_t dst_off; // byte offset of the scaled frame in the destination buffer
    uint32_t W, H, x0, y0, w, h; // the source: coded size, crop origin, display size
    uint32_t format;   // H264MI_FMT_I420 / _NV12 / _RGB24 / _RGBP
    uint32_t cset;     // as ConvDesc (unused for I420 and NV12)
    uint32_t bilinear; // chroma upsampling of the SCALED chroma planes, as ConvDesc
    uint32_t filter;   // H264MI_SCALE_BILINEAR / _AREA (uniform per launch: it selects the kernel)
    // bilinear, per axis (luma x, luma y, chroma x, chroma y): step = (n_in << 16) / n_out and the half-step offset (step >> 1) - 32768,
    // computed once per frame on the host: the kernel divides nothing in this mode
    uint32_t step[4];
    int32_t half[4];
} ScaleDesc;
extern "C" __global__ void k_scale(const ScaleDesc *descs, uint8_t *dst, int ow, int oh, int pairs_per_block);      // H264MI_SCALE_BILINEAR
extern "C" __global__ void k_scale_area(const ScaleDesc *descs, uint8_t *dst, int ow, int oh, int pairs_per_block); // H264MI_SCALE_AREA
// K9 (k_tensor.hip): a list of (frame, region) items -> model-input tensors of ONE canvas size, by the rule of include/h264mi.h ("Model input"): the
// region scaled to sw x sh (K8's rule), converted to RGB (K7's rule), placed at (px, py) of the out_w x out_h canvas, the rest of it `pad`; every 8-bit
// value mapped to u8 / f16 / bf16 / f32.  grid = (items, chunks of pairs_per_block row pairs), block = 256; a thread owns two rows x 8 columns of the
// canvas, counted from the picture's origin (so that rows 2j, 2j + 1 and columns 2k, 2k + 1 of the SCALED frame stay together, whatever px and py are)
typedef struct {
    uint64_t src;     // as PackDesc
    uint64_t dst_off; // byte offset of the item in the destination buffer
    uint32_t W, H;    // coded size
    uint32_t x0, y0;  // origin of the region in the coded planes: the crop origin + the region's (even) origin in the display frame
    uint32_t w, h;    // size of the region
    uint32_t sw, sh, px, py; // the picture: size and place in the canvas (h264mi_fit_rect)
    uint32_t cset;     // as ConvDesc
    uint32_t bilinear; // chroma upsampling of the SCALED chroma planes, as ConvDesc
    uint32_t step[4];  // as ScaleDesc, for region size -> picture size
    int32_t half[4];
} TensorDesc;
typedef struct { // uniform per launch; scale, bias and pad by channel POSITION (colour 2 - position under H264MI_TENSOR_BGR)
    int32_t ow, oh;          // the canvas
    int32_t dtype;           // H264MI_DT_*
    int32_t hwc;             // 0: H264MI_FMT_RGBP (three planes), 1: H264MI_FMT_RGB24
    int32_t bgr;             // swap R and B
    int32_t pairs_per_block;
    uint32_t pad[3];
    float scale[3], bias[3];
} TensorParams;
extern "C" __global__ void k_tensor(const TensorDesc *descs, uint8_t *dst, TensorParams P);      // H264MI_SCALE_BILINEAR
extern "C" __global__ void k_tensor_area(const TensorDesc *descs, uint8_t *dst, TensorParams P); // H264MI_SCALE_AREA
// K10 (k_deint.hip): a list of (frame, mode, parity) items -> deinterlaced frames, by the rule of include/h264mi.h ("Deinterlaced output"), each into a
// frame slot of its source's coded size (the same layout: K6 .. K9 read it like a frame of the pool); only the display rectangle is written.
// grid = (items, ceil((ceil(h_max / 2) + ceil(ceil(h_max / 2) / 2)) / pairs_per_block)), block = 256; a thread owns two rows x 16 columns of one plane
typedef struct {
    uint64_t src;     // as PackDesc
    uint64_t dst_off; // byte offset of the derived frame's slot in the arena
    uint32_t W, H, x0, y0, w, h;
    uint32_t mode;   // H264MI_DEINT_FIELD / _BLEND / _EDGE
    uint32_t parity; // 0 / 1, resolved
} DeintDesc;
extern "C" __global__ void k_deint(const DeintDesc *descs, uint8_t *dst, int pairs_per_block);
// K10, motion-adaptive (k_deint_motion.hip): a list of (frame, predecessor, spatial mode, parity) items -> deinterlaced frames, by the rule of
// include/h264mi.h ("Motion-adaptive deinterlacing"); slots, grid and thread item as k_deint.  The predecessor has the source's layout: a frame of the
// pool, or a stream's history slot
typedef struct {
    uint64_t src;     // as PackDesc
    uint64_t dst_off; // as DeintDesc
    uint32_t W, H, x0, y0, w, h;
    uint32_t mode;   // H264MI_DEINT_FIELD / _EDGE: what a missing row is without motion information, and what it is pulled from
    uint32_t parity; // 0 / 1, resolved
    uint64_t prev;   // Y plane of the predecessor (the same coded size and display rectangle); 0: none -- the frame is mode's frame
} DeintMotionDesc;
extern "C" __global__ void k_deint_motion(const DeintMotionDesc *descs, uint8_t *dst, int pairs_per_block);
// K11 (k_side.hip): a list of frames -> planes of macroblock side information per 4x4 luma block, by the rule of include/h264mi.h ("Macroblock side
// information"): a re-layout of the pictures' MbRec / MbMv1 records, no sample is read.  grid = (items, ceil(macroblock rows the largest grid touches /
// rows_per_block)), block = 256; one lane per macroblock, four cells (8 bytes) per store on the aligned path
typedef struct {
    uint64_t rec;     // first MbRec of the picture, in the record set of the last executed pass
    uint64_t mv1;     // first MbMv1 of the picture; 0: the picture has no B slices
    uint64_t dpoc;    // the batch's table of picture order count differences: int16 [n_slices][2 lists][16 entries], indexed by MbRec::slice_idx
    uint64_t dst_off; // byte offset of the item in the destination buffer
    uint32_t wmb, hmb;  // the picture in macroblocks
    uint32_t bx0, by0;  // coded 4x4 block of cell (0, 0): crop_x >> 2, crop_y >> 2
    uint32_t gw, gh;    // the grid
    uint32_t n_slices;  // rows of the dpoc table (a record that names none of them reads 0)
    uint32_t vec;       // 1: bx0 % 4 == 0, gw % 4 == 0 and the item's first byte is 8-byte aligned -- a macroblock's four cells of a row are one store
} SideDesc;
extern "C" __global__ void k_side(const SideDesc *descs, uint8_t *dst, uint32_t planes, int rows_per_block);
// K12 (k_stats.hip): a list of (frame, predecessor) items -> one h264mi_frame_stats record each and, with a grid, planes of per-cell sums behind it, by
// the rule of include/h264mi.h ("Frame statistics").  The project's one reduction: the host clears the destination range, blocks add their partial
// results with integer atomics.  grid = (items, mi_stats_blocks(h_max)), block = 256; a block takes a band of MI_STATS_LUMA_ROWS luma rows -- whole
// cell rows of every cell size -- or MI_STATS_CHROMA_ROWS rows of the Cb-then-Cr row space; a thread item is 8 rows x 16 columns of one plane
#define MI_STATS_LUMA_ROWS 64    /* a multiple of the largest cell */
#define MI_STATS_CHROMA_ROWS 128 /* of ceil(hc / 8) * 8 rows of Cb followed by as many of Cr */
typedef struct {
    uint64_t src;     // as PackDesc
    uint64_t dst_off; // byte offset of the item (its record; the planes follow) in the destination buffer
    uint32_t W, H, x0, y0, w, h;
    uint64_t prev;   // Y plane of the predecessor (the same coded size and display rectangle); 0: none
    uint32_t gw, gh; // the grid; 0, 0: none
    // what the blocks of an item tell each other, zero when the table is uploaded: a minimum cannot be accumulated into a cleared field, so each block
    // adds 255 - (its smallest sample) to inv_min with an atomic maximum, and the block that draws the last ticket writes min_y and the record's constants
    uint32_t inv_min, ticket;
} StatsDesc;
__host__ __device__ static inline int mi_stats_luma_blocks(int h) { return (h + MI_STATS_LUMA_ROWS - 1) / MI_STATS_LUMA_ROWS; }
__host__ __device__ static inline int mi_stats_chroma_blocks(int h) { return (2 * (((h + 1) / 2 + 7) / 8 * 8) + MI_STATS_CHROMA_ROWS - 1) / MI_STATS_CHROMA_ROWS; }
static inline int mi_stats_blocks(int h) { return mi_stats_luma_blocks(h) + mi_stats_chroma_blocks(h); } // (monotonic in h: a launch is sized by its tallest item)
// The 32-bit partial sums.  A thread's: its share of a band, ceil(rows / 8 * groups / 256) thread items of 128 samples, of at most 255 * 255 each; a
// block's sums of samples, of differences and its counts (the squares are reduced in 64 bits): rows * width * 255.  At H264MI_SCALE_MAX = 16384:
#define MI_STATS_MAX_AXIS 16384
static_assert((MI_STATS_CHROMA_ROWS / 8 * (MI_STATS_MAX_AXIS / 16) / 256 + 1) * 128ull * 255 * 255 < (1ull << 32) && MI_STATS_CHROMA_ROWS >= MI_STATS_LUMA_ROWS,
              "a thread's 32-bit partial sum of squares overflows");
static_assert(static_cast<unsigned long long>(MI_STATS_CHROMA_ROWS) * MI_STATS_MAX_AXIS * 255 < (1ull << 32), "a block's 32-bit sums overflow");
extern "C" __global__ void k_stats(StatsDesc *descs, uint8_t *dst, uint32_t cell_log2, uint32_t planes, uint32_t thresh);
// K13 (k_jpeg.hip): a list of frames -> baseline JPEG files, one per slot of the destination, by the rule of include/h264mi.h ("JPEG snapshots").  A
// one-wavefront workgroup owns a restart interval; the grid is flat over the intervals of all items (JpegDesc::ivl_base ascends: a workgroup finds its
// item by bisection).  Three launches: k_jpeg_size leaves every interval's stuffed byte length in the interval table, k_jpeg_scan turns the lengths of an
// item into offsets inside its slot and writes the item's h264mi_jpeg_result, k_jpeg_write encodes again and stores header, intervals, markers.
// The table of a launch: one JpegParams, then the JpegDescs
#define MI_JPEG_HDR_MAX 640      /* the longest header (4:2:0: 629 bytes) */
#define MI_JPEG_BLOCK_BITS 1660  /* the most bits a block can take: DC 11 + 11, 63 x (16 + 10) for AC -- the derivation is h264mi_jpeg_size's */
#define MI_JPEG_BUF_WORDS 256    /* the wavefront's bit buffer in LDS: 4 words a lane; it is flushed once a worst-case block may no longer fit */
static_assert(MI_JPEG_BUF_WORDS * 32 >= 2 * MI_JPEG_BLOCK_BITS + 64, "the bit buffer must hold a block behind the flush threshold");
typedef struct {
    uint64_t y, cb, cr;   // first sample of the display rectangle in each plane (cb, cr unused for mono)
    uint64_t slot_off;    // byte offset of the item's slot in the destination
    uint32_t ystride, cstride;
    uint32_t w, h;        // display size; chroma planes are ceil(w / 2) x ceil(h / 2)
    uint32_t mono, full;  // one component; limited -> full range
    uint32_t mcus_w, n_mcus; // MCUs per row, MCUs in all
    uint32_t restart, n_int; // MCUs per restart interval (resolved), intervals
    uint32_t ivl_base;    // the item's first entry of the interval table
    uint32_t pad;
} JpegDesc;
typedef struct {
    uint16_t q[2][64];       // quantisation tables, natural order
    uint32_t dc[2][12];      // Huffman codes by symbol: length << 16 | code
    uint32_t ac[2][256];
    uint8_t hdr[2][MI_JPEG_HDR_MAX]; // SOI .. SOS for 4:2:0 and for mono, with zero size and restart interval
    uint32_t hdr_len[2], sof_off[2], dri_off[2]; // length; where height (2 bytes, then width) and the restart interval go
    uint32_t n_items, slot_bytes;
} JpegParams;
extern "C" __global__ void k_jpeg_size(const uint8_t *table, uint32_t *ivl, uint32_t total);
extern "C" __global__ void k_jpeg_scan(const uint8_t *table, uint32_t *ivl, uint8_t *dst);
extern "C" __global__ void k_jpeg_write(const uint8_t *table, const uint32_t *ivl, uint8_t *dst, uint32_t total);

#ifndef MI_INTRA_WAVES
#define MI_INTRA_WAVES 16 /* 1024 threads, 128 VGPRs per wavefront: the kernels need 120 once nothing lane-dependent is hoisted out of the macroblock loop */
#endif

// K3 over several workgroups per picture: bands of about 4 macroblock rows, as many as keep pictures * bands within max_wgs;
// nbands = 1: the one-workgroup kernel.  p_only (no intra-only picture in the launch): bands of 3 rows with up to 4 wavefronts
// per row -- the few intra macroblocks of a P / B picture are dealt round-robin to them (k_intra_x, waves_per_row).
static inline void mi_intra_bands(int n_pics, int hmb, int max_wgs, bool p_only, int *nbands, int *nwaves, int *wpr) {
    int nb = n_pics > 0 ? max_wgs / n_pics : 1;
    const int want = (hmb + (p_only ? 2 : 3)) / (p_only ? 3 : 4);
    if (nb > want) nb = want;
    if (nb < 2) nb = 1;
    const int rows = (hmb + nb - 1) / nb, slots = rows < MI_INTRA_WAVES ? rows : MI_INTRA_WAVES;
    int w = (nb > 1 && p_only) ? MI_INTRA_WAVES / slots : 1;
    if (w > 4) w = 4;
    if (w < 1) w = 1;
    *nbands = nb;
    *wpr = w;
    *nwaves = nb > 1 ? slots * w : MI_INTRA_WAVES;
}
