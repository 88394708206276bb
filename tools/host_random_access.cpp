// tools/host_random_access.cpp -- TEST TOOLING: the host side of libh264mi built against tools/hoststub (a null device: kernels are not run) decodes
// one Annex-B file with h264mi_decoder_set_random_access(mode) and prints what picture management made of it.  The file is fed in chunks that end at
// the byte offsets given (the rest goes in a last chunk; no offsets: one chunk).  Per chunk one line "P prepare_result stream_status" -- a chunk
// that fails ends the run --, then per frame in decoding order
//   "F frame_num pic_order_cnt nal_ref_idc idr new_sequence field_coded | recovery_point recovery_frame_cnt exact_match broken_link slice_group_idc entry"
// and per slice of a frame picture "S slice cur_poc n0 pocs of list 0 ... | n1 pocs of list 1 ..." (h264mi_frame_ref_pocs); at the end
//   "T entries skipped_waiting_nals skipped_leading_pictures".
// tests/test_random_access_host.py holds a stream cut at its entry points against the whole stream, on the CPU.
#include "h264mi.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: host_random_access stream.h264 max_width max_height max_frames mode [chunk_end ...]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf(len);
    if (fread(buf.data(), 1, len, f) != static_cast<size_t>(len)) return 2;
    fclose(f);
    h264mi_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.max_streams = 1, cfg.max_width = atoi(argv[2]), cfg.max_height = atoi(argv[3]), cfg.max_frames_per_batch = atoi(argv[4]);
    cfg.max_slices_per_frame = 64, cfg.max_bitstream_bytes = len + 4096;
    cfg.b_pictures = 1; // (chunks of one access unit: the motion of a co-located picture is kept from the start, not from the first B slice on)
    h264mi_decoder *dec = nullptr;
    if (h264mi_decoder_create(&cfg, &dec) != 0) { fprintf(stderr, "create: %s\n", h264mi_last_error_string()); return 1; }
    const int32_t mode_result = h264mi_decoder_set_random_access(dec, atoi(argv[5]));
    if (mode_result != 0) { printf("M %d\n", mode_result); return 0; }
    std::vector<long> ends;
    for (int i = 6; i < argc; i++) ends.push_back(atol(argv[i]));
    ends.push_back(len);
    long at = 0;
    for (long end : ends) {
        if (end <= at || end > len) continue;
        const uint8_t *bufs[1] = {buf.data() + at};
        size_t lens[1] = {static_cast<size_t>(end - at)};
        at = end;
        h264mi_batch_info info;
        int32_t r = h264mi_batch_prepare(dec, 1, bufs, lens, &info), st = 0;
        h264mi_stream_status(dec, 0, &st);
        printf("P %d %d\n", r, st);
        if (r != 0 || st != 0) {
            fprintf(stderr, "prepare: %d, stream status %d: %s\n", r, st, h264mi_last_error_string());
            break;
        }
        if (h264mi_batch_execute(dec) != 0 || h264mi_batch_sync(dec) != 0) { fprintf(stderr, "execute: %s\n", h264mi_last_error_string()); return 1; }
        int32_t n = 0;
        h264mi_stream_frame_count(dec, 0, &n);
        for (int i = 0; i < n; i++) {
            h264mi_frame_info fi;
            h264mi_field_info fl;
            h264mi_frame_entry_info en;
            if (h264mi_frame_get_info(dec, 0, i, &fi) != 0 || h264mi_frame_fields(dec, 0, i, &fl) != 0 || h264mi_frame_entry(dec, 0, i, &en) != 0) return 1;
            printf("F %d %d %d %d %d %d | %d %d %d %d %d %d\n", fi.frame_num, fi.pic_order_cnt, fi.nal_ref_idc, fi.idr, fi.new_sequence, fl.field_coded, en.recovery_point,
                   en.recovery_frame_cnt, en.exact_match_flag, en.broken_link_flag, en.changing_slice_group_idc, en.entry);
            int32_t cur = 0, cnt = 0, pocs[32];
            for (int s = 0; !fl.field_coded; s++) {
                if (h264mi_frame_ref_pocs(dec, 0, i, s, 0, &cur, pocs, 32, &cnt) != 0) break; // no such slice: the picture's slices are through
                printf("S %d %d %d", s, cur, cnt);
                for (int k = 0; k < cnt; k++) printf(" %d", pocs[k]);
                if (h264mi_frame_ref_pocs(dec, 0, i, s, 1, &cur, pocs, 32, &cnt) != 0) return 1;
                printf(" | %d", cnt);
                for (int k = 0; k < cnt; k++) printf(" %d", pocs[k]);
                printf("\n");
            }
        }
    }
    h264mi_random_access_stats ra;
    if (h264mi_stream_random_access_stats(dec, 0, &ra) != 0) return 1;
    printf("T %lld %lld %lld\n", static_cast<long long>(ra.entries), static_cast<long long>(ra.skipped_waiting_nals), static_cast<long long>(ra.skipped_leading_pictures));
    h264mi_decoder_destroy(dec);
    return 0;
}
