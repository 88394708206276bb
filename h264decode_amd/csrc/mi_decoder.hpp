// h264decode_amd/csrc/mi_decoder.hpp -- the decoder's host state and what the host files share: mi_api.cpp (tables, create / destroy / reset, counters,
// frame accessors), mi_picture.cpp (what a slice NAL does to the picture under construction), mi_batch.cpp (prepare, execute, sync), mi_output.cpp (the
// output stage) and mi_hooks.cpp (test hooks and measurement switches).  Internal: nothing here is part of the ABI of include/h264mi.h, and nothing
// depends on the hooks build.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/h264mi.h"
#include "mi_dpb.hpp"
#include "mi_kernels.h"
#include "mi_parse.hpp"

using namespace mi;

#ifndef MI_SETS
#define MI_SETS 3 /* record / coefficient sets: a pass may run two passes ahead of the reconstruction that frees its set (a fourth set bought 1 % for 28 GB) */
#endif

#define HIP_TRY(x)                                                                          \
    do {                                                                                    \
        hipError_t _e = (x);                                                                \
        if (_e != hipSuccess) {                                                             \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
            return H264MI_EDEVICE;                                                          \
        }                                                                                   \
    } while (0)

// ---------------------------------------------------------------- per-stream host state
struct OutFrame { // a decoded picture of the current batch, with the geometry it was coded with
    int slot, wmb, hmb, crop_x, crop_y, width, height;
    int poc, frame_num, nal_ref_idc, idr, pic;
    int new_sequence; // IDR picture or memory_management_control_operation 5: picture order counts start over
    int pic2 = -1;    // a frame coded as two field pictures: `pic` / `pic2` are the first / second field's PicDesc (-1: decoded by an earlier batch, or never)
    int matrix_coefficients = 2, video_full_range = 0; // of the picture's own SPS (E.2.1: "unspecified" / 0 where it does not carry them): h264mi_frame_colour
    // h264mi_frame_fields: coded as two field pictures (one of them may be missing or concealed); TopFieldOrderCnt / BottomFieldOrderCnt (8.2.1, after a
    // possible operation 5; a missing field's is the other one's); which parity comes first (taken before operation 5 rewrites the counts)
    int field_coded = 0, top_foc = 0, bottom_foc = 0, first_parity = 0;
    // h264mi_frame_entry: the recovery point SEI message of the picture's access unit (a frame of two fields: the first field's), and whether the
    // stream entered here after waiting (random access)
    h264mi_recovery_point rp = {0, 0, 0, 0, 0};
    int entry = 0;
    int mono = 0; // chroma_format_idc 0 of the picture's own SPS: K13 writes one component
};
struct StreamState {
    h264mi_sps sps[32];
    h264mi_pps pps[256];
    std::vector<uint8_t> sg_ids[256]; // slice_group_id[] of the PPSs with slice_group_map_type 6 (h264/pps.go:23)
    std::vector<int32_t> cur_first_mbs; // first_mb_in_slice of the slices of the current picture
    uint32_t epoch = 0;                 // bumped by every reset of the stream: failures of batches prepared before it are nobody's business any more
    bool sps_ok[32] = {}, pps_ok[256] = {};
    int active_sps = -1;
    int wmb = 0, hmb = 0;
    Dpb dpb; // frame slots, POC / frame_num history, the picture under construction (dpb.cur_slot >= 0) and its frame slot: mi_dpb.hpp
    int cur_pic = -1, cur_slices = 0; // the picture under construction: its PicDesc, slices so far
    // The frame that waits in dpb.pend_slot for its second field goes out -- once -- when that field is complete, or with one field decoded (the
    // rows of the other one mid-grey) when something else follows: another picture, an end-of-sequence / end-of-stream NAL unit, a reset.
    OutFrame pend_out;
    int n_pics_in_batch = 0;
    int status = H264MI_OK; // of this stream in the current batch (h264mi_stream_status)
    const void *status_batch = nullptr; // the batch whose entropy kernels set `status` (harvest_status)
    bool need_idr = false;  // after an error: nothing is decodable before the next IDR picture
    // error concealment: slice NAL units with an unparsable header that arrived while no picture was under construction -- they belong to the picture
    // the next slice starts, and are tolerated only if that picture turns out to be concealable (add_slice); that slice may come with a later chunk
    int pending_drops = 0, pending_drop_err = H264MI_OK;
    int pending_drop_type = 0; // ... their nal_unit_type (1 or 5; -1: both kinds): tolerated only in a picture of that kind (H264MI_CONCEAL_IDR)
    // error concealment of lone fields (H264MI_CONCEAL_LONE_FIELDS): the parameter sets the first field in dpb.pend_slot was decoded under, and whether
    // the stream has stored other content under one of those ids since (the inserted field needs the ones its frame was decoded with)
    int pend_sps_id = -1, pend_pps_id = -1;
    bool pend_stale = false;
    // error concealment of IDR pictures (H264MI_CONCEAL_IDR): what of the SPS the stream's reference frames were decoded under must still hold for an
    // IDR picture to predict from them -- picture size in macroblocks, chroma_format_idc, frame_mbs_only_flag, log2_max_frame_num_minus4 (start_picture)
    struct RefSeq {
        int wmb = -1, hmb = 0, chroma_format = 0, frame_mbs_only = 0, log2_max_frame_num_minus4 = 0;
        bool operator==(const RefSeq &o) const {
            return wmb == o.wmb && hmb == o.hmb && chroma_format == o.chroma_format && frame_mbs_only == o.frame_mbs_only && log2_max_frame_num_minus4 == o.log2_max_frame_num_minus4;
        }
    } ref_seq;
    // Random access (h264mi_decoder_set_random_access; the rule: include/h264mi.h).  sei: the recovery point of the SEI NAL unit parsed last (either
    // mode), which the next picture that starts takes and clears.  decoded_any: a picture has started since create / the resets -- with the mode on a
    // stream without one, or a marked one (need_idr), waits for an entry point.  lead: pictures with a PicOrderCnt below lead_poc -- that of the non-IDR
    // entry picture -- are leading pictures and are skipped; skipping / skip_sh: the slices of the leading picture being skipped (its first one).
    h264mi_recovery_point sei = {0, 0, 0, 0, 0};
    bool decoded_any = false, lead = false, skipping = false;
    int lead_poc = 0;
    h264mi_slice_header skip_sh;
    h264mi_random_access_stats ra = {0, 0, 0}; // counted in prepare; a chunk that fails takes its counts with it (parse_streams)
};

// Everything one prepared batch owns: the pinned staging buffers and their device mirrors, the descriptors, the launch
// lists and the output frame lists.  There are MI_STAGES of them, so that h264mi_batch_prepare(n + 1) -- host parsing and
// the H2D copies -- runs while batch n is still executing (h264/server.go:144-145 reads its connection in an endless loop).
#ifndef MI_STAGES
#define MI_STAGES 2
#endif
struct Stage {
    uint8_t *d_bits = nullptr, *h_bits = nullptr;
    size_t bits_used = 0;
    size_t map_cursor = 0, bits_end = 0; // slice group maps of FMO pictures follow the slices in the staging buffer; bits_end: what must be uploaded
    std::vector<uint32_t> fmo_pics;      // pictures whose records are zeroed before the entropy kernels run
    struct GreyFill { uint32_t stream, slot, parity, w, h; }; // a frame that went out with one field decoded: the rows of the other parity are painted mid-grey
    std::vector<GreyFill> grey;
    std::vector<uint32_t> epochs;        // StreamState::epoch of every stream when this batch was prepared
    SliceDesc *d_slices = nullptr, *h_slices = nullptr;
    PicDesc *d_pics = nullptr, *h_pics = nullptr;
    uint32_t *d_status = nullptr, *h_status = nullptr, *d_lists = nullptr, *h_lists = nullptr;
    BSliceExt *d_bext = nullptr, *h_bext = nullptr; // one per B slice
    int n_bext = 0;
    int ent_kernel = MI_ENT_K_GENERAL;       // the I/P entropy kernel of level 0 (mi_entropy_kernel_choice), decided when the batch is prepared
    int pass_group = 0;                      // passes over this batch whose entropy stages are released together (mi_pass_group; 0: ungrouped), decided with it
    int n_slices = 0, n_pics = 0, wmb_max = 0, hmb_max = 0, mbs_max = 0;
    uint64_t mb_used = 0;
    // ---- the batch's host-side facts: one record per picture, per slice, per reconstruction wave and per entropy level
    struct ConcealPoc { int32_t cur, ref; };
    struct Pic { // [n_pics], beside h_pics
        int level = 0;  // the latest level among its slices
        int wave = 0;   // reconstruction wave: 0 for a picture that reads no picture of this batch, else 1 + the latest wave among its references
        uint8_t save_col = 0; // the picture's motion is kept for later direct prediction (k_dbprep writes its ColRec array)
        uint8_t init_qp = 26; // error concealment: 26 + pic_init_qp_minus26 of the picture's PPS (QP_Y of its concealment SliceDesc)
        uint16_t dropped = 0; // error concealment: slice NAL units whose header did not parse and that were dropped as lost (add_slice)
        ConcealPoc conceal_poc = {0, 0}; // K11: its count and its concealment reference's when it starts: what the pseudo-slice reports (start_picture)
    };
    // B pictures take their direct-mode motion from RefPicList1[0], so that picture's slices must have been entropy-decoded
    // first: slices are launched by level -- 0: I and P slices (k_entropy), n: B slices whose co-located picture is of level
    // n - 1 or older than the batch (k_entropy_b) -- and the slice table is ordered by level.
    // K11 (side information): the picture order counts a slice's reference lists were built with (add_slice; h264mi_frame_ref_pocs), and the device
    // mirror k_side reads: the differences entry - current, clamped to int16, [slice][list][16], uploaded with the batch's other descriptors.
    // ev_side: the last k_side launch that read this set's mirror (an event of the family's descriptor tables), which the next upload into it waits for
    struct SliceRefs {
        int32_t cur_poc, poc[2][MI_MAX_REFS];
        uint8_t n[2]; // active entries per list
    };
    struct Slice { // beside h_slices: in parse order until the table is sorted, the concealment pseudo-slices (one per picture) behind the real ones
        int level = 0;
        SliceRefs refs = {};
    };
    struct ListRange { uint32_t off = 0, n = 0; }; // pictures, as a range of h_lists / d_lists
    struct Wave { ListRange all, p, b; }; // all pictures (K3, K5) / the inter pictures without B slices (k_inter) / the pictures with B slices (k_inter_b)
    struct Level {
        int first = 0, n = 0;   // its slices in the sorted table
        uint32_t colsave_n = 0; // pictures whose ColRec array k_dbprep writes (what the cross-pass fence looks at)
        ListRange prep;         // the pictures whose last slice is of this level: k_conceal and k_dbprep run on them after the level
        int prep_kernel = MI_DBPREP_K_GENERIC; // ... and the k_dbprep kernel that does (mi_dbprep_kernel_choice)
    };
    std::vector<Pic> pics;
    std::vector<Slice> slices;
    std::vector<Wave> waves;
    std::vector<Level> levels;
    int16_t *d_dpoc = nullptr, *h_dpoc = nullptr;
    hipEvent_t ev_side = nullptr;
    uint32_t *d_cmap = nullptr, *h_cmap = nullptr; // error concealment: per picture where its slices are in the sorted slice table (k_conceal)
    std::vector<std::vector<OutFrame>> out; // per stream: frames of this batch in decoding order
    uint64_t seq = 0; // which h264mi_batch_prepare made this batch, counted from 1 (h264mi_decoder::prep_seq): what a history (HistorySet) is dated by
    bool prepared = false, executed = false;
    bool harvested = true; // the entropy kernels' per-slice status words of the last execute have been looked at (harvest_status)
    bool retried = false;  // the batch has been repeated with the whole residual pool (retry_exhausted)
    h264mi_batch_info info;
    hipEvent_t ev_upload = nullptr; // H2D copies of this batch are complete
    hipEvent_t ev_done = nullptr;   // the last pass over this batch has finished (nothing reads or writes its buffers any more)
    // What a stream adds to the batch sits at the tail of every table: a mark taken before its parse, and a stream that fails is taken out again
    struct Mark { int n_pics, n_slices, n_bext; uint64_t mb_used; int64_t info_mbs; size_t n_fmo, n_grey; };
    Mark mark() const { return {n_pics, n_slices, n_bext, mb_used, info.n_macroblocks, fmo_pics.size(), grey.size()}; }
    void truncate(const Mark &m, int stream) {
        n_pics = m.n_pics, n_slices = m.n_slices, n_bext = m.n_bext, mb_used = m.mb_used, info.n_macroblocks = m.info_mbs;
        pics.resize(m.n_pics), slices.resize(m.n_slices), fmo_pics.resize(m.n_fmo), grey.resize(m.n_grey);
        out[stream].clear();
    }
};

// The descriptor tables of one output kernel family: two pinned tables and their device mirrors, used alternately, each fenced by an event -- an
// output call does not wait for the stream (the batch it reads may still be executing, and the next execute may be enqueued right behind it)
struct DescTables {
    void *h[2] = {nullptr, nullptr}, *d[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0}; // bytes
    hipEvent_t ev[2] = {nullptr, nullptr};
    int slot = 0;
};
enum { OUT_PACK, OUT_CONVERT, OUT_SCALE, OUT_TENSOR, OUT_DEINT, OUT_SIDE, OUT_DEINT_MOTION, OUT_STATS, OUT_JPEG, OUT_FAMILIES }; // K6, K7, K8, K9, K10, K11, K10 motion-adaptive, K12, K13

// A derived (deinterlaced) frame: frame k of the pseudo-stream H264MI_STREAM_DERIVED.  `of`: its source's OutFrame (what the accessors report); off: its
// slot in the arena, in the layout of a frame slot of the source's coded size; prev: what it was made from besides its source (h264mi_derived_prev) -- a
// frame of the source's stream, H264MI_DEINT_PREV_NONE (every frame of the spatial modes) or H264MI_DEINT_PREV_HISTORY
struct DerivedFrame {
    OutFrame of;
    size_t off;
    int prev = H264MI_DEINT_PREV_NONE;
};
// A stream's history -- the source of its last frame in output order of the last batch that a batch call took one from, in the stream's slot of the
// arena.  valid: cleared by the resets; batch: Stage::seq of that batch (the history serves the batch prepared right after it and no other); of: the
// frame's geometry, which a frame that takes it as its predecessor must share
struct FrameHistory {
    bool valid = false;
    uint64_t batch = 0;
    OutFrame of;
};
// The histories of one consumer: one frame slot per stream (slot_bytes each), allocated by the first call that takes a history and kept.  Each consumer
// has its own -- h264mi_batch_deinterlace_motion (K10, motion-adaptive) and h264mi_batch_stats_device (K12) -- so that two calls in one batch each date
// their own slot: with one shared slot the second call of the next batch would find the first one's date and no predecessor
enum { HIST_DEINT, HIST_STATS, HIST_KINDS };
struct HistorySet {
    uint8_t *arena = nullptr;
    std::vector<FrameHistory> slots;
};

struct h264mi_decoder {
    h264mi_config cfg;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<StreamState> st;
    int Wmax = 0, Hmax = 0, n_slots = 0;
    size_t slot_bytes = 0;
    Stage stage[MI_STAGES];
    int prep = 0;  // stage of the most recent h264mi_batch_prepare
    int exec = 0;  // stage of the most recent h264mi_batch_execute: what sync and the frame accessors refer to
    size_t bits_cap = 0;
    uint32_t *d_toprows[MI_SETS] = {}; // entropy kernels' row-above neighbour state: 48 B per MB column per slice
    int slices_cap = 0, pics_cap = 0;
    // Passes are pipelined: the entropy kernels of passes n+1 / n+2 (two private streams, alternating)
    // overlap the reconstruction kernels of pass n (on `stream`); each pass owns one of MI_SETS
    // MbRec / coefficient buffer sets, fenced by events.
    MbRec *d_mbrec[MI_SETS] = {};
    DbPrm *d_dbprm[MI_SETS] = {};        // k_dbprep -> K5: boundary strengths and filter parameters, same indexing as d_mbrec
    unsigned long long *d_imask[MI_SETS] = {}; // k_dbprep -> K3: one bit per macroblock of the batch (same indexing), set for what K3 reconstructs
    MbMv1 *d_mv1[MI_SETS] = {};          // list-1 vectors, same indexing as d_mbrec; allocated when the first B slice arrives
    ColRec *d_colrec = nullptr;          // per stream and frame slot: the motion a picture leaves for later direct prediction
    size_t colrec_per_slot = 0;          // ColRecs per frame slot
    int16_t *d_coef[MI_SETS] = {};       // coefficient pools: 32-byte blocks, only the blocks that carry anything (MbRec::coef_off / coef_mask)
    uint32_t *d_pool_head = nullptr;     // MI_SETS counters: next free block of each pool, reset before every entropy launch
    uint64_t pool_blocks = 0;            // blocks per pool
    hipStream_t ent_stream[2] = {nullptr, nullptr};
    hipStream_t rec_stream = nullptr; // K3-K5; the caller's stream only brackets a pass with events
    hipEvent_t ev_user = nullptr;
    hipEvent_t ev_ent[MI_SETS] = {}, ev_rec[MI_SETS] = {}, ev_col[MI_SETS] = {};
    uint64_t pass = 0; // execute() counter
    // Pass groups (mi_pass_group): the entropy stages of up to Stage::pass_group consecutive passes are released together, behind the reconstruction
    // of everything before the group.  group_left: passes that may still join the open group (0: none is open); group_gate: ev_rec of the last pass
    // executed before the group opened (nullptr for the first group of a decoder), which every entropy launch of the group waits for besides its
    // set's own fences; group_gate_pass: that pass (-1: none).  last_rec_pass: the pass that recorded an ev_rec last (-1: none yet).
    int group_left = 0;
    hipEvent_t group_gate = nullptr;
    int64_t group_gate_pass = -1, last_rec_pass = -1;
    int64_t last_pass_gate = -1;  // the gate of the pass executed last (-1: it waited for none), for the test hooks
    int pass_group_force = -1;    // 0 / 2 / 3: instead of the plan for batches without B slices; -1: the plan (set by the hooks build only)
    int n_cus = 0;                // compute units of the device
    int last_exec_stage = -1, last_exec_set = 0; // staging set and record set of the most recent execute (ensure_b_buffers)
    bool last_pass_had_b = false;
    int dbprep_launches[2] = {0, 0};     // launches of the last execute by kernel (MI_DBPREP_K_*), for the test hooks
    int dbprep_rows = 0;                 // macroblock rows per wavefront of k_dbprep_ip; 0: mi_dbprep_ip_rows (set by a test hook only)
    uint64_t mb_cap = 0;
    uint64_t dev_bytes = 0;              // device memory this decoder holds (h264mi_decoder_memory)
    uint32_t *d_backfill = nullptr;      // picture list of the one-off ColRec back-fill (first B slice of a decoder)
    FramePool *d_pools = nullptr;
    std::vector<FramePool> h_pools;
    uint8_t *d_frames = nullptr;
    DevTables *d_tables = nullptr, *h_tables = nullptr;
    int n_scaling = 0;
    uint32_t scaling_used[MI_STAGES] = {}; // bit i: the batch of that staging set refers to DevTables::scaling[i]
    bool tables_dirty = true;
    size_t ent_lds_pad = 0; // dynamic LDS requested (and not used) by k_entropy: caps its wavefronts per CU, see h264mi_decoder_create
    bool conceal = false; // h264mi_config.conceal_errors: lost macroblocks of concealable pictures are copied from a reference picture (k_conceal)
    bool conceal_pics = false; // ... bit H264MI_CONCEAL_PICTURES: wholly lost reference frames are inserted as pictures without slices (conceal_frame_num_gap)
    bool conceal_fields = false; // ... bit H264MI_CONCEAL_FIELDS: field pictures are concealable too
    bool conceal_idr = false; // ... bit H264MI_CONCEAL_IDR: IDR frame pictures that still have a reference frame are concealable too
    bool conceal_lone = false; // ... bit H264MI_CONCEAL_LONE_FIELDS: the missing field of a frame is inserted as a picture without slices (flush_pending_field)
    int64_t concealed_slices = 0, concealed_mbs = 0; // totals since create (h264mi_decoder_concealed)
    int64_t concealed_pics = 0;                      // (h264mi_decoder_concealed_pictures)
    int64_t concealed_fields = 0;                    // (h264mi_decoder_concealed_fields)
    bool isolate = false; // h264mi_decoder_set_isolation: a broken stream does not fail the batch
    bool random_access = false; // h264mi_decoder_set_random_access: streams start and resume at recovery points too (add_slice)
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_kind;
    size_t ev_used = 0;
    double k_ms[5] = {0, 0, 0, 0, 0};
    // Launches with fewer pictures than the chip has CUs spread a picture over several workgroups (k_intra_x, k_deblock_x,
    // k_deblock_x): hand-off rings / flags in global memory, a ticket counter per kernel family, a give-up word
    unsigned long long *d_xring = nullptr; // K5: x_cap * (Wmax / 16) * 24 granules
    uint32_t *d_xdone = nullptr;           // K3: x_cap * (Wmax / 16) flag words
    int k5_max_waves = MI_DEBLOCK8_MAX_WAVES;
    int64_t unpinned_failures = 0; // slices of CABAC field pictures that failed in the entropy kernel (h264mi_decoder_unpinned_failures)
    uint32_t *d_xctl = nullptr, *h_xstatus = nullptr; // [0] K5 tickets, [32] K3 tickets, [64] give-up code (128-byte lines of their own)
    uint32_t x_epoch = 0, x_tk5 = 0, x_tk3 = 0;
    int x_max_wgs = 256, x_cap = 512, x_cap3 = 512; // workgroups per launch: default; capacity of the K5 ring; of the K3 flag array
    DescTables tables[OUT_FAMILIES]; // of K6 .. K10, a set each: a convert call does not wait for a pack call's table
    hipEvent_t last_pack = nullptr; // the most recent output launch (K6 .. K10): the reconstruction of a later pass may rewrite the frames it reads
    // the most recent side-information launch (K11): it reads the macroblock records of the pass executed last, which the entropy stream of a later pass
    // rewrites -- the next execute makes its entropy stream wait for it (the set's own fences, ev_rec / ev_col, know nothing of the caller's stream)
    hipEvent_t last_side = nullptr;
    // K10: the derived frames of the last h264mi_items_deinterlace / h264mi_batch_deinterlace call (emptied by execute and the resets) and their arena,
    // which grows to the largest call and is kept
    std::vector<DerivedFrame> derived;
    uint8_t *d_derived = nullptr;
    size_t derived_cap = 0;
    HistorySet hist[HIST_KINDS]; // K10, motion-adaptive, and K12: a history each
    // K13: the interval table (a length, then an offset, per restart interval of a call), allocated by the first call that launches, grown to the largest
    // call and kept
    uint32_t *d_jpeg_ivl = nullptr;
    size_t jpeg_ivl_cap = 0; // entries
    uint64_t prep_seq = 0; // h264mi_batch_prepare calls so far
    std::vector<float> launch_ms[4]; // duration of every launch of the last profiled pass, per kernel
};

// hipSetDevice is per-thread state: every entry point that takes a decoder selects the decoder's device for the
// duration of the call and restores the caller's afterwards (callers may be pool threads or migrating goroutines).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(const h264mi_decoder *d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d->cfg.device) ok = hipSetDevice(d->cfg.device) == hipSuccess;
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define GUARD(d)                                                        \
    DeviceGuard guard_(d);                                              \
    if (!guard_.ok) {                                                   \
        set_error("hipSetDevice(%d) failed", (d)->cfg.device);          \
        return H264MI_EDEVICE;                                          \
    }

// the record set (d_mbrec / d_mv1 / ...) of the pass executed last: what the frame accessors and K11 read.  A batch that h264mi_batch_sync repeated
// for want of residual blocks (retry_exhausted) ran again in set 0 and moved the pass counter there, so this follows it
static inline int last_record_set(const h264mi_decoder *d) { return static_cast<int>((d->pass + MI_SETS - 1) % MI_SETS); }
// where the picture in frame slot `slot` of stream `stream` leaves its motion (ColRec): a bottom field's (par 1) in the second half of the slot's array
static inline uint64_t colrec_of(const h264mi_decoder *d, size_t stream, size_t slot, int par) {
    return reinterpret_cast<uint64_t>(d->d_colrec + (stream * d->n_slots + slot) * d->colrec_per_slot + (par ? d->colrec_per_slot / 2 : 0));
}
void build_vlc(uint16_t *c, int *mismatches); // ---- mi_api.cpp
void build_scaling(const uint8_t s4[6][16], const uint8_t s8[2][64], ScalingSet *o);
void reset_stream(StreamState &s, bool keep_parameter_sets);
// ---- mi_picture.cpp: one slice NAL of stream `si`, staged at `off` / `rlen`; the picture under construction is complete; a lone first field goes out
int add_slice(h264mi_decoder *d, int si, size_t off, size_t rlen, int ref_idc, int type);
void finish_picture(h264mi_decoder *d, int si);
int flush_pending_field(h264mi_decoder *d, int si, const h264mi_sps *nsps = nullptr, const h264mi_pps *npps = nullptr, const h264mi_slice_header *next = nullptr);
int ensure_b_buffers(h264mi_decoder *d); // ---- mi_batch.cpp
int drain(h264mi_decoder *d); // both entropy streams, the reconstruction stream and the caller's stream have run dry
// ---- mi_hooks.cpp: the measurement switches of the hooks build, called where they act; in the product build they do nothing
void hook_create_entropy(h264mi_decoder *d, int *ent_cus); // H264MI_ENT_LDS_PAD, H264MI_ENT_CUS
void hook_create_k5(h264mi_decoder *d);                    // H264MI_K5_WAVES
void hook_create_pass_group(h264mi_decoder *d);            // H264MI_PASS_GROUP
int hook_entropy_kernel(int chosen);                       // H264MI_ENT_GENERIC
int hook_dbprep_kernel(int chosen);                        // H264MI_DBPREP_GENERIC
void hook_after_sync(const h264mi_decoder *d);             // H264MI_SLICE_STATS, H264MI_SLICE_TIMELINE
// frame `frame` of stream `stream` of the last executed batch: its Y plane in the frame pool and its geometry (mi_api.cpp); of the pseudo-stream
// H264MI_STREAM_DERIVED: derived frame `frame`, its Y plane in the arena and its SOURCE's geometry
int frame_ptrs(h264mi_decoder *d, int stream, int frame, uint8_t **y, const OutFrame **of);
// the picture's own geometry (a new SPS may have activated later in the same batch): the coded frame, or its display rectangle (mi_output.cpp)
void crop_rect(const OutFrame *of, int crop, int *x0, int *y0, int *w, int *h);
