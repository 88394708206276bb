// h264decode_amd/csrc/mi_batch.cpp -- a batch from the caller's buffers to decoded frames: h264mi_batch_prepare (scan, stage, parse -- every slice NAL
// goes through mi_picture.cpp --, order the slices, build the launch lists, upload), h264mi_batch_execute (the GPU launch sequence: entropy levels on
// the entropy streams, reconstruction waves on the reconstruction stream) and h264mi_batch_sync (wait, retry, what the entropy kernels reported).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#include "mi_decoder.hpp"

// Per level of a batch: which k_dbprep kernel runs on the pictures complete with it (mi_dbprep_kernel_choice), from what their descriptors say now
static void choose_dbprep_kernels(Stage &g) {
    for (Stage::Level &lv : g.levels) {
        int n_has_b = 0, n_save_col = 0;
        for (uint32_t i = 0; i < lv.prep.n; i++) {
            const PicDesc &pd = g.h_pics[g.h_lists[lv.prep.off + i]];
            n_has_b += pd.has_b != 0, n_save_col += pd.save_col != 0;
        }
        lv.prep_kernel = hook_dbprep_kernel(mi_dbprep_kernel_choice(n_has_b, n_save_col));
    }
}

// What only B pictures need exists once the first B slice has been seen: the list-1 vector arrays (64 bytes per macroblock and
// buffer set) and the ColRec arrays (80 bytes per macroblock and frame slot: the motion direct prediction reads).  Reference
// pictures decoded BEFORE that moment have left no ColRec; the ones of the batch before this one -- where RefPicList1[0] of a
// stream's first B picture can still come from -- are filled in now from that batch's records, which are still resident
// (MI_STAGES staging sets, MI_SETS record sets).  Older ones cannot be: direct prediction from them sees an intra picture.
int ensure_b_buffers(h264mi_decoder *d) {
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
            pv.h_pics[pic].col_out = colrec_of(d, si, o.slot, par);
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
                d->concealed_mbs += g.h_status[8 * g.n_slices + p], d->concealed_slices += g.pics[p].dropped,
                    // (only an inserted picture has no slice -- a frame: conceal_frame_num_gap, a field: flush_pending_field)
                    d->concealed_pics += g.h_pics[p].n_slices == 0 && g.h_pics[p].conceal_ref >= 0 && g.h_pics[p].field == 0,
                    d->concealed_fields += g.h_pics[p].n_slices == 0 && g.h_pics[p].conceal_ref >= 0 && g.h_pics[p].field != 0;
    return result;
}

// ---------------------------------------------------------------- h264mi_batch_prepare, step by step
// The next staging set is taken back: everything the batch that used it last left in it goes, and every stream starts a batch
static void reset_staging_set(h264mi_decoder *d, Stage &g, int prev_stage) {
    g.prepared = false, g.executed = false;
    d->scaling_used[d->prep] = 0; // (the batch that filled this staging set before has finished: its LevelScale sets may go to new matrices)
    g.n_slices = g.n_pics = g.n_bext = 0;
    g.bits_used = 0, g.mb_used = 0, g.wmb_max = 0, g.hmb_max = 0, g.mbs_max = 0;
    g.map_cursor = g.bits_end = 0;
    g.epochs.resize(d->st.size());
    g.pics.clear(), g.slices.clear(), g.waves.clear(), g.levels.clear(), g.fmo_pics.clear(), g.grey.clear();
    memset(&g.info, 0, sizeof(g.info));
    for (size_t si = 0; si < d->st.size(); si++) {
        StreamState &s = d->st[si];
        g.epochs[si] = s.epoch;
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
}

// What passes 1 to 3 leave for the parse: every stream's NAL units, and where the RBSP of every slice NAL stands in the pinned staging buffer
struct Staged { int si, nal; size_t off, rlen; };
struct Scan {
    std::vector<std::vector<h264mi_nal>> nals;
    std::vector<Staged> staged;
    std::vector<size_t> first; // [stream]: its first entry of `staged`; the others follow in NAL order
};
static int scan_and_stage(h264mi_decoder *d, Stage &g, int n_streams, const uint8_t *const *bufs, const size_t *lens, Scan &sc) {
    // ---- pass 1 (parallel over streams): Annex-B scan ----
    const int n_threads = std::max(1, std::min<int>({static_cast<int>(std::thread::hardware_concurrency()), 16, n_streams}));
    sc.nals.resize(n_streams), sc.first.resize(n_streams);
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
        std::vector<h264mi_nal> &v = sc.nals[si];
        v.resize(1024);
        int n = 0;
        while (annexb_scan(bufs[si], lens[si], v.data(), static_cast<int>(v.size()), &n) == H264MI_ECAPACITY) v.resize(v.size() * 4);
        v.resize(n);
    });
    // ---- pass 2 (serial, trivial): staging offsets of the slice NALs; the escaped length bounds the RBSP length ----
    size_t cursor = 0;
    for (int si = 0; si < n_streams; si++) {
        sc.first[si] = sc.staged.size();
        for (size_t i = 0; i < sc.nals[si].size(); i++) {
            const h264mi_nal &nal = sc.nals[si][i];
            if (nal.type != 1 && nal.type != 5) continue;
            const size_t off = (cursor + 15) & ~static_cast<size_t>(15);
            if (off + nal.num_bytes + 4096 > d->bits_cap) {
                set_error("bitstream staging buffer too small (%zu bytes)", d->bits_cap);
                return H264MI_ECAPACITY;
            }
            sc.staged.push_back({si, static_cast<int>(i), off, 0});
            cursor = off + nal.num_bytes;
        }
    }
    g.map_cursor = cursor; // slice group maps (FMO pictures) go behind the last slice
    // ---- pass 3 (parallel over slices): remove emulation prevention straight into the pinned staging buffer ----
    parallel_for(static_cast<int>(sc.staged.size()), [&](int k) {
        Staged &sg = sc.staged[k];
        const h264mi_nal &nal = sc.nals[sg.si][sg.nal];
        sg.rlen = unescape(bufs[sg.si] + nal.offset + 1, nal.num_bytes - 1, g.h_bits + sg.off);
    });
    return H264MI_OK;
}

// The NAL units of one stream, in order: parameter sets, slice headers, DPB / POC / reference lists, descriptors.  The first error ends it
static int parse_stream(h264mi_decoder *d, int si, const uint8_t *buf, const Scan &sc) {
    StreamState &s = d->st[si];
    std::vector<uint8_t> tmp;
    size_t next_slice = sc.first[si];
    int r = H264MI_OK;
    for (size_t i = 0; i < sc.nals[si].size() && r == H264MI_OK; i++) {
        const h264mi_nal &nal = sc.nals[si][i];
        const uint8_t *p = buf + nal.offset;
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
            const Staged &sg = sc.staged[next_slice++];
            r = add_slice(d, si, sg.off, sg.rlen, nal.ref_idc, nal.type);
            break;
        }
        case 6: { // SEI: the recovery point message (D.1.7), for the picture that starts next; every other payload, and a unit that does not parse, is passed over
            h264mi_recovery_point rp;
            if (sei_recovery_point(p, nal.num_bytes, &rp) == H264MI_OK && rp.found) s.sei = rp;
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
    return r;
}

// ---- pass 4 (serial): every stream's parse.  A stream that fails leaves the batch -- its pictures, slices and records are dropped, its references
// are forgotten (nothing is decodable before its next IDR picture) --; with isolation the other streams are not affected
static int parse_streams(h264mi_decoder *d, Stage &g, int n_streams, const uint8_t *const *bufs, const size_t *lens, const Scan &sc) {
    for (int si = 0; si < n_streams; si++) {
        if (!bufs[si] || !lens[si]) continue;
        StreamState &s = d->st[si];
        const Stage::Mark mark = g.mark();
        const h264mi_random_access_stats ra = s.ra;
        const int r = parse_stream(d, si, bufs[si], sc);
        if (r != H264MI_OK) {
            g.truncate(mark, si);
            reset_stream(s, true);
            s.ra = ra; // (random access: the entry state of the chunk goes with its pictures, and what was counted in it)
            s.need_idr = true;
            s.status = r;
            if (!d->isolate) return r;
            continue;
        }
        if (s.dpb.cur_slot >= 0) finish_picture(d, si);
    }
    // A reference picture that outlives the batch may become the co-located picture of a B picture of a later batch: its
    // motion is kept too (8.4.1.2.1).
    for (int si = 0; si < n_streams; si++)
        for (const Slot &sl : d->st[si].dpb.slots)
            if (sl.ref)
                for (int pic : {sl.pic, sl.fpic[0], sl.fpic[1]})
                    if (pic >= 0 && pic < g.n_pics) g.pics[pic].save_col = 1;
    return H264MI_OK;
}

// Slice order = launch order: by level (see Stage), and inside a level longest-processing-time-first -- the entropy
// kernels run one slice per workgroup and workgroups are dispatched in index order, so the biggest slices (I pictures)
// must start first.  (MbRec::slice_idx indexes the sorted table: the records beside it, K11's among them, go with it.)
static void order_slices_by_level(Stage &g) {
    int n_levels = 1;
    std::vector<int> order(g.n_slices);
    for (int i = 0; i < g.n_slices; i++) order[i] = i, n_levels = std::max(n_levels, g.slices[i].level + 1);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        if (g.slices[x].level != g.slices[y].level) return g.slices[x].level < g.slices[y].level;
        return g.h_slices[x].rbsp_size > g.h_slices[y].rbsp_size;
    });
    const std::vector<SliceDesc> desc(g.h_slices, g.h_slices + g.n_slices);
    const std::vector<Stage::Slice> rec(g.slices);
    g.levels.assign(n_levels, Stage::Level());
    for (int i = 0; i < g.n_slices; i++) g.h_slices[i] = desc[order[i]], g.slices[i] = rec[order[i]], g.levels[g.slices[i].level].n++;
    for (int l = 1; l < n_levels; l++) g.levels[l].first = g.levels[l - 1].first + g.levels[l - 1].n;
    int n_mode[2] = {0, 0}; // level 0 by entropy coding mode: CAVLC, CABAC slices
    for (int i = 0; i < g.levels[0].n; i++) n_mode[g.h_pics[g.h_slices[i].pic_idx].cabac != 0]++;
    int n_t8x8_mono = 0; // pictures of the batch with the 8x8 transform switched on, or monochrome: none in a batch of Main streams
    for (int p = 0; p < g.n_pics; p++) n_t8x8_mono += g.h_pics[p].t8x8_mode != 0 || g.h_pics[p].mono != 0;
    g.ent_kernel = hook_entropy_kernel(mi_entropy_kernel_choice(n_mode[1], n_mode[0], !g.fmo_pics.empty(), n_t8x8_mono));
}

// Error concealment.  Behind the slices of the batch one SliceDesc per picture -- what MbRec::slice_idx of a concealed macroblock names, so that
// K4 finds neither the explicit weights of the slice that failed nor those of the slice whose wavefront blanked a gap: type P, wp_flag 0 and
// identity weights (the one-list K4 chooses explicit weighting per picture: denominators 0, weight 1, offset 0 give the default prediction
// exactly; the two-list K4 sees a slice that is not a B slice and has no wp_flag: default), QP_Y from the PPS, all edges filtered, and a
// slice_in_pic no real slice has.  And the picture -> slices map of the sorted table (k_conceal).
static void concealment_tables(Stage &g) {
    g.slices.resize(g.n_slices + g.n_pics); // ... and K11's view of them: one active entry, the concealment reference, where the picture has one
    for (int p = 0; p < g.n_pics; p++) {
        SliceDesc &cd = g.h_slices[g.n_slices + p];
        memset(&cd, 0, sizeof(cd));
        cd.pic_idx = static_cast<uint32_t>(p);
        cd.slice_type = 0, cd.slice_qp = g.pics[p].init_qp, cd.num_ref_idx_active = 1;
        cd.slice_in_pic = 0xFFFF;
        for (int i = 0; i < MI_MAX_REFS; i++) {
            cd.ref_slot[i] = static_cast<int16_t>(i == 0 ? g.h_pics[p].conceal_ref : -1);
            cd.wp_lw[i] = 1, cd.wp_cw[i][0] = cd.wp_cw[i][1] = 1;
        }
        Stage::SliceRefs &sr = g.slices[g.n_slices + p].refs;
        memset(&sr, 0, sizeof(sr));
        sr.cur_poc = g.pics[p].conceal_poc.cur, sr.n[0] = g.h_pics[p].conceal_ref >= 0, sr.poc[0][0] = g.pics[p].conceal_poc.ref;
    }
    uint32_t at = static_cast<uint32_t>(g.n_pics);
    for (int p = 0; p < g.n_pics; p++) g.h_cmap[p] = at, at += g.h_pics[p].n_slices;
    std::vector<uint32_t> fill(g.h_cmap, g.h_cmap + g.n_pics);
    for (int i = 0; i < g.n_slices; i++) g.h_cmap[fill[g.h_slices[i].pic_idx]++] = static_cast<uint32_t>(i);
}

// picture "waves": pictures that do not predict from one another are reconstructed side by side -- wave 0 holds the pictures that read no
// picture of this batch (intra pictures wherever they stand in their stream; pictures whose references an earlier batch decoded), wave n + 1
// the pictures whose latest reference is of wave n (Stage::Pic::wave; with I P P P ... that is the k-th picture of every stream, with
// I B B P ... the B pictures share the wave of the P picture that follows them in decoding order, an all-intra stream is one wave).  Per wave:
// all pictures (K3, K5), the inter pictures without / the pictures with B slices (K4 / K4 two-list): three ranges of h_lists (Stage::Wave)
// ... and per level the pictures complete with it (k_conceal, k_dbprep).  Returns the entries of h_lists in use
static uint32_t launch_lists(h264mi_decoder *d, Stage &g) {
    size_t nw = 0;
    for (int i = 0; i < g.n_pics; i++) nw = std::max<size_t>(nw, static_cast<size_t>(g.pics[i].wave) + 1);
    g.waves.assign(nw, Stage::Wave());
    std::vector<std::vector<uint32_t>> of_wave(nw);
    for (int i = 0; i < g.n_pics; i++) of_wave[g.pics[i].wave].push_back(i);
    uint32_t pos = 0;
    // one range of a wave: its pictures, in batch order, that `take` says belong
    auto range = [&](size_t w, auto take) {
        Stage::ListRange r{pos, 0};
        for (uint32_t i : of_wave[w])
            if (take(g.h_pics[i])) g.h_lists[pos++] = i;
        r.n = pos - r.off;
        return r;
    };
    for (size_t w = 0; w < nw; w++) {
        g.waves[w].all = range(w, [](const PicDesc &) { return true; });
        // (error concealment: the concealed macroblocks of a picture whose delivered slices are all I slices are inter macroblocks -- K4 must see it)
        g.waves[w].p = range(w, [](const PicDesc &pd) { return (!pd.is_intra_only || pd.conceal_ref >= 0) && !pd.has_b; });
        g.waves[w].b = range(w, [](const PicDesc &pd) { return pd.has_b != 0; });
    }
    for (size_t l = 0; l < g.levels.size(); l++) {
        Stage::Level &lv = g.levels[l];
        lv.prep.off = pos;
        for (int i = 0; i < g.n_pics; i++)
            if (g.pics[i].level == static_cast<int>(l)) {
                g.h_lists[pos++] = i;
                PicDesc &pd = g.h_pics[i];
                pd.save_col = g.pics[i].save_col && d->d_colrec != nullptr; // (no B slice seen yet: nothing to keep, see ensure_b_buffers)
                const int par = pd.field == 2 ? 1 : 0;
                pd.col_out = d->d_colrec ? colrec_of(d, pd.stream, pd.slot, par) : 0;
                if (pd.save_col) d->st[pd.stream].dpb.slots[pd.slot].col_valid[par] = true; // (the slot is this picture's until the next prepare at least: held)
                lv.colsave_n += pd.save_col;
            }
        lv.prep.n = pos - lv.prep.off;
    }
    choose_dbprep_kernels(g);
    return pos;
}

// Uploads go to the entropy stream the next execute will use: in order with that pass's entropy kernel, and not behind
// the batch that is still executing (the caller's stream waits for its reconstruction).  No stream of their own: the
// runtime multiplexes streams onto 4 hardware queues by default, and a fifth stream ended up sharing a queue with one of
// the kernel streams, which serialised entropy decoding and reconstruction of consecutive passes.
static int upload(h264mi_decoder *d, Stage &g, uint32_t n_lists) {
    // K11's device table: PicOrderCnt(entry) - PicOrderCnt(current picture) per slice of the table, list and entry, clamped to int16; 0 behind the active entries
    for (size_t i = 0; i < g.slices.size(); i++)
        for (int l = 0; l < 2; l++)
            for (int e = 0; e < MI_MAX_REFS; e++) {
                const Stage::SliceRefs &sr = g.slices[i].refs;
                const int64_t dp = e < sr.n[l] ? static_cast<int64_t>(sr.poc[l][e]) - sr.cur_poc : 0;
                g.h_dpoc[(i * 2 + l) * MI_MAX_REFS + e] = static_cast<int16_t>(std::min<int64_t>(std::max<int64_t>(dp, -32768), 32767));
            }
    hipStream_t up = d->ent_stream[d->pass & 1];
    if (g.n_slices || g.n_pics) {
        const size_t end = std::max(g.bits_used, g.bits_end); // (bits_end: behind the slice group maps of FMO pictures, if any)
        size_t nbytes = std::min(d->bits_cap, ((end + 15) & ~static_cast<size_t>(15)) + 4096);
        memset(g.h_bits + end, 0, nbytes - end);
        HIP_TRY(hipMemcpyAsync(g.d_bits, g.h_bits, nbytes, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(g.d_slices, g.h_slices, sizeof(SliceDesc) * (g.n_slices + (d->conceal ? g.n_pics : 0)), hipMemcpyHostToDevice, up));
        if (d->conceal) HIP_TRY(hipMemcpyAsync(g.d_cmap, g.h_cmap, sizeof(uint32_t) * (g.n_pics + g.n_slices), hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(g.d_pics, g.h_pics, sizeof(PicDesc) * g.n_pics, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(g.d_lists, g.h_lists, sizeof(uint32_t) * n_lists, hipMemcpyHostToDevice, up));
        if (g.n_bext) HIP_TRY(hipMemcpyAsync(g.d_bext, g.h_bext, sizeof(BSliceExt) * g.n_bext, hipMemcpyHostToDevice, up));
        if (g.ev_side) { // a K11 launch on the caller's stream may still be reading this set's table (the batch before last)
            HIP_TRY(hipStreamWaitEvent(up, g.ev_side, 0));
            g.ev_side = nullptr;
        }
        if (!g.slices.empty()) HIP_TRY(hipMemcpyAsync(g.d_dpoc, g.h_dpoc, sizeof(int16_t) * 2 * MI_MAX_REFS * g.slices.size(), hipMemcpyHostToDevice, up));
    }
    if (d->tables_dirty) {
        // a new PPS added a LevelScale set: the table only grows, so the batch still executing keeps seeing its own sets.
        // (h_tables is pinned and rewritten only by the next prepare, which cannot start its copy before this one is done:
        // same stream.)
        HIP_TRY(hipMemcpyAsync(d->d_tables, d->h_tables, sizeof(DevTables), hipMemcpyHostToDevice, up));
        d->tables_dirty = false;
    }
    HIP_TRY(hipEventRecord(g.ev_upload, up));
    return H264MI_OK;
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
    reset_staging_set(d, g, prev_stage);
    g.seq = ++d->prep_seq;
    Scan sc;
    int r = scan_and_stage(d, g, n_streams, bufs, lens, sc);
    if (r == H264MI_OK) r = parse_streams(d, g, n_streams, bufs, lens, sc);
    if (r != H264MI_OK) return r;
    order_slices_by_level(g);
    if (d->conceal) concealment_tables(g);
    r = upload(d, g, launch_lists(d, g));
    if (r != H264MI_OK) return r;
    {
        int launches = 0, pics = 0; // pictures per reconstruction launch: the mean over the batch's waves
        for (const Stage::Wave &W : g.waves) launches += W.all.n > 0, pics += static_cast<int>(W.all.n);
        g.pass_group = mi_pass_group(g.levels.empty() ? 0 : g.levels[0].n, d->n_cus * 4 * mi_entropy_waves_per_simd(g.ent_kernel), launches ? pics / launches : 0, g.n_bext > 0);
    }
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
    // Pass n uses record set n % MI_SETS and entropy stream n & 1.  Entropy runs on a stream of its own so that the entropy kernels of
    // passes n+1 and n+2 run ahead of the reconstruction kernels of pass n; set reuse is fenced by events.
    const int set = static_cast<int>(d->pass % MI_SETS);
    // Pass groups (mi_pass_group): the entropy stages of G consecutive passes start together, behind the reconstruction of every pass before the
    // group -- the gate, ev_rec of the last pass executed before the group opened.  EVERY pass of the group waits for it: the host enqueues far
    // ahead, and a later pass of the group that waited for pass n - MI_SETS alone would start inside the previous group's reconstruction and keep
    // its workgroups off the chip.  The gate only adds ordering behind strictly earlier passes.  G <= MI_SETS, so the gate's event is not
    // recorded again before the group's last pass has enqueued its wait (its own ev_rec is the first of that set since).  A serialised pass
    // (profiling, exclusive) and a pass whose plan says "ungrouped" close the open group.
    int group = g.pass_group;
    if (d->pass_group_force >= 0 && !g.n_bext) group = d->pass_group_force;
    if (prof || group <= 0) d->group_left = 0;
    else {
        if (d->group_left <= 0) d->group_left = std::min(group, MI_SETS), d->group_gate = d->last_rec_pass >= 0 ? d->ev_rec[d->last_rec_pass % MI_SETS] : nullptr, d->group_gate_pass = d->last_rec_pass;
        d->group_left--;
    }
    const bool gated = !prof && group > 0 && d->group_gate;
    d->last_pass_gate = gated ? d->group_gate_pass : -1;
    hipStream_t es = d->ent_stream[d->pass & 1];
    MbRec *mbrec = d->d_mbrec[set];
    int16_t *coef = d->d_coef[set];
    // Entropy decoding, level by level (Stage::levels): k_entropy or one of its builds (Stage::ent_kernel) for the I / P slices, k_entropy_b for each level of B
    // slices, and after each level k_dbprep for the pictures complete with it (K5's parameters; the ColRec arrays later B slices ask for).
    // `done`: recorded after the last level's k_dbprep -- what the reconstruction kernels wait for.
    auto launch_entropy = [&](hipStream_t st, size_t lds_pad, bool fence_prev_pass, hipEvent_t done) {
        const int n_levels = static_cast<int>(g.levels.size());
        // pictures with slice groups: a slice's macroblocks are scattered, so its wavefront cannot blank "its" range for what it
        // does not decode (SliceDesc::fill_from) -- all records of such a picture start out as MBT_NONE instead
        for (uint32_t pi : g.fmo_pics) hipMemsetAsync(mbrec + g.h_pics[pi].mb_base, 0, sizeof(MbRec) * g.h_pics[pi].wmb * g.h_pics[pi].hmb, st);
        hipMemsetAsync(d->d_imask[set], 0, sizeof(unsigned long long) * (g.mb_used / 64 + 2), st); // k_dbprep ORs K3's work list into it
        for (int lv = 0; lv < n_levels; lv++) {
            const Stage::Level &L = g.levels[lv];
            const int first = L.first, n = L.n;
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
                    hipLaunchKernelGGL(g.ent_kernel == MI_ENT_K_FMO ? k_entropy_f : (g.ent_kernel == MI_ENT_K_MAIN ? k_entropy_m : (g.ent_kernel == MI_ENT_K_CABAC ? k_entropy_c : k_entropy)), dim3(n), dim3(64), lds_pad, st, g.d_slices, g.d_pics, g.d_bits, d->d_tables, mbrec, coef, d->d_pool_head + set,
                                       pool_blocks, g.d_status, d->d_toprows[set], g.wmb_max, static_cast<uint32_t>(first));
                else
                    hipLaunchKernelGGL(k_entropy_b, dim3(n), dim3(64), 0, st, g.d_slices, g.d_pics, g.d_bits, d->d_tables, mbrec, coef, d->d_pool_head + set,
                                       pool_blocks, g.d_status, d->d_toprows[set], g.wmb_max, static_cast<uint32_t>(first), g.d_bext, d->d_mv1[set]);
            }
            // the pictures complete with this level: K5's strengths and filter parameters, and the motion later B slices (the next
            // level's, or a later batch's) take their direct prediction from
            if (L.colsave_n) fence();
            // error concealment: the lost macroblocks of these pictures become decodable records before anything downstream reads them
            if (d->conceal && L.prep.n)
                hipLaunchKernelGGL(k_conceal, dim3(L.prep.n), dim3(256), 0, st, g.d_lists + L.prep.off, g.d_pics, g.d_slices, g.d_cmap, static_cast<uint32_t>(g.n_slices),
                                   g.d_status, g.d_bits, d->d_tables, mbrec, d->d_mv1[set], g.d_status + 8 * static_cast<size_t>(g.n_slices));
            if (L.prep.n) {
                if (L.prep_kernel == MI_DBPREP_K_IP) {
                    const int chunks = std::max(1, (g.wmb_max + 63) / 64), hmax = std::max(1, g.hmb_max);
                    const int rows = d->dbprep_rows > 0 ? std::min(d->dbprep_rows, hmax) : mi_dbprep_ip_rows(static_cast<int>(L.prep.n), g.wmb_max, hmax);
                    hipLaunchKernelGGL(k_dbprep_ip, dim3(static_cast<uint32_t>(chunks * ((hmax + rows - 1) / rows)), (L.prep.n + 7u) & ~7u), dim3(64), 0, st,
                                       g.d_lists + L.prep.off, g.d_pics, d->d_tables, mbrec, d->d_dbprm[set], d->d_imask[set], static_cast<int>(L.prep.n), chunks, rows);
                } else
                    hipLaunchKernelGGL(k_dbprep, dim3((g.mbs_max + MI_DBPREP_MBS - 1) / MI_DBPREP_MBS, (L.prep.n + 7u) & ~7u), dim3(256), 0, st, g.d_lists + L.prep.off, g.d_pics,
                                       d->d_tables, mbrec, d->d_mv1[set], d->d_dbprm[set], 0, d->d_imask[set], static_cast<int>(L.prep.n));
                d->dbprep_launches[L.prep_kernel]++;
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
        if (gated) HIP_TRY(hipStreamWaitEvent(es, d->group_gate, 0));
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
    for (const Stage::Wave &W : g.waves) {
        const uint32_t n = W.all.n, ni = W.p.n, nbp = W.b.n;
        if (!n) continue;
        int grp_log2 = 0; // K4 workgroups per picture: the largest picture's count of four-macroblock groups, rounded up to a power of two
        while ((4 << grp_log2) < g.mbs_max) grp_log2++;
        if (ni) {
            const uint32_t nb = ni << grp_log2;
            hipLaunchKernelGGL(k_inter, dim3(((nb + MI_K4_WG - 1) / MI_K4_WG + 7) & ~7u), dim3(64 * MI_K4_WG), 0, rs, g.d_lists + W.p.off, g.d_pics, g.d_slices, d->d_tables, mbrec, coef, grp_log2,
                               static_cast<int>(nb));
            mark(1);
        }
        if (nbp) {
            const uint32_t nb = nbp << grp_log2;
            hipLaunchKernelGGL(k_inter_b, dim3(((nb + MI_K4_WG - 1) / MI_K4_WG + 7) & ~7u), dim3(64 * MI_K4_WG), 0, rs, g.d_lists + W.b.off, g.d_pics, g.d_slices, d->d_tables, mbrec, coef, grp_log2,
                               static_cast<int>(nb), g.d_bext, d->d_mv1[set]);
            mark(1);
        }
        // K3 / K5 keep a picture inside one workgroup when the launch has pictures enough to fill the chip; otherwise the
        // banded kernels spread each picture over up to x_max_wgs / pictures workgroups (mi_intra_bands / mi_deblock_bands)
        // (K3 of a launch WITHOUT intra-only pictures -- the few intra macroblocks of P / B pictures -- is bound by the row with the most
        // of them: there the banded kernel also puts several wavefronts on a row)
        int nb3 = 1, nw3 = MI_INTRA_WAVES, wpr3 = 1;
        bool has_ipic = false;
        for (uint32_t i = 0; i < n; i++) has_ipic |= g.h_pics[g.h_lists[W.all.off + i]].is_intra_only != 0;
        mi_intra_bands(static_cast<int>(n), g.hmb_max, d->x_max_wgs, !has_ipic, &nb3, &nw3, &wpr3);
        if (nb3 > 1) {
            hipLaunchKernelGGL(k_intra_x, dim3(n * nb3), dim3(nw3 * 64), 0, rs, g.d_lists + W.all.off, g.d_pics, d->d_pools, d->d_tables, mbrec, coef, d->d_xdone,
                               next_epoch(), nb3, d->d_xctl + 32, d->x_tk3, g.wmb_max, d->d_xctl + 64, wpr3, d->d_imask[set]);
            d->x_tk3 += n * nb3;
        } else
            hipLaunchKernelGGL(k_intra, dim3(n), dim3(MI_INTRA_WAVES * 64), 0, rs, g.d_lists + W.all.off, g.d_pics, d->d_pools, d->d_tables, mbrec, coef, d->d_imask[set]);
        mark(2);
        int dbw = 1, dbring = 16, dbring_last = 16, dbbufs = 1, nb5 = 1, roles = 1;
        mi_deblock_bands(static_cast<int>(n), g.wmb_max, g.hmb_max, d->x_max_wgs, &nb5, &dbw, &dbring, &roles);
        if (nb5 > 1) {
            hipLaunchKernelGGL(k_deblock_x, dim3(n * nb5), dim3(dbw * 64), mi_deblock_lds_bytes_banded(dbw, dbring), rs, g.d_lists + W.all.off, g.d_pics,
                               d->d_dbprm[set], dbring, 0, 1, d->d_xring, next_epoch(), nb5, d->d_xctl, d->x_tk5, g.wmb_max, d->d_xctl + 64, roles);
            d->x_tk5 += n * nb5;
        } else {
            mi_deblock8_plan(g.wmb_max, g.hmb_max, &dbw, &dbring, &dbring_last, &dbbufs, d->k5_max_waves);
            hipLaunchKernelGGL(k_deblock, dim3(n), dim3(dbw * 64), mi_deblock8_lds_bytes(dbw, dbring, dbring_last, dbbufs), rs, g.d_lists + W.all.off, g.d_pics,
                               d->d_dbprm[set], dbring, dbring_last, dbbufs, d->d_xctl + 64);
        }
        mark(3);
    }
    HIP_TRY(hipEventRecord(d->ev_rec[set], rs));
    d->last_rec_pass = static_cast<int64_t>(d->pass);
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

int drain(h264mi_decoder *d) {
    for (hipStream_t st : {d->ent_stream[0], d->ent_stream[1], d->rec_stream, d->stream}) HIP_TRY(hipStreamSynchronize(st));
    return H264MI_OK;
}

extern "C" int32_t h264mi_batch_sync(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    if (const int r = drain(d)) return r;
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
    hook_after_sync(d);
    if (*d->h_xstatus) { // a banded kernel gave up waiting for its neighbour workgroup: the pictures of that launch are wrong
        set_error("reconstruction hand-off timed out (code 0x%08x)", *d->h_xstatus);
        *d->h_xstatus = 0;
        HIP_TRY(hipMemset(d->d_xctl + 64, 0, sizeof(uint32_t)));
        return H264MI_EDEVICE;
    }
    if (const int r = retry_exhausted(d)) return r; // (leaves every stream drained again)
    // every batch executed since the last look (pipelined callers synchronise once for several), the most recent one last
    int result = H264MI_OK;
    for (int k = 1; k <= MI_STAGES; k++) {
        const int r = harvest_status(d, d->stage[(d->exec + k) % MI_STAGES]);
        if (r != H264MI_OK) result = r;
    }
    return d->isolate ? H264MI_OK : result;
}

extern "C" int32_t h264mi_decode_batch(h264mi_decoder *d, int32_t n, const uint8_t *const *bufs, const size_t *lens, h264mi_batch_info *info) {
    if (const int r = h264mi_batch_prepare(d, n, bufs, lens, info)) return r;
    if (const int r = h264mi_batch_execute(d)) return r;
    return h264mi_batch_sync(d);
}
