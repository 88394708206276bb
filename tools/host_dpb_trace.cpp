// tools/host_dpb_trace.cpp -- TEST TOOLING: the host side of libh264mi, hooks build, against tools/hoststub (a null device: kernels are
// not run) decodes one or more Annex-B files, one batch per file on the same decoder, and prints after every batch what picture
// management made of it (h264mi_internal_dpb_trace: pictures, slices with their reference lists, output frames, the reference / held
// frame slots and the POC / frame_num history).  A batch that is refused prints its status code and message instead and ends the
// run: refusals are part of the behaviour tests/test_host_dpb_trace.py pins.
#include "h264mi.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int32_t h264mi_internal_dpb_trace(h264mi_decoder *, int32_t stream, char *buf, size_t cap, size_t *len);

int main(int argc, char **argv) {
    if (argc < 8) { fprintf(stderr, "usage: host_dpb_trace max_width max_height max_frames max_slices conceal_errors allow_unpinned_field_cabac stream.h264...\n"); return 2; }
    std::vector<std::vector<uint8_t>> files;
    size_t longest = 0;
    for (int a = 7; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        long len = ftell(f);
        fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> buf(len);
        if (fread(buf.data(), 1, len, f) != static_cast<size_t>(len)) return 2;
        fclose(f);
        longest = buf.size() > longest ? buf.size() : longest;
        files.push_back(std::move(buf));
    }
    h264mi_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.max_streams = 1, cfg.max_width = atoi(argv[1]), cfg.max_height = atoi(argv[2]), cfg.max_frames_per_batch = atoi(argv[3]);
    cfg.max_slices_per_frame = atoi(argv[4]), cfg.max_bitstream_bytes = static_cast<int64_t>(longest) + 4096;
    cfg.conceal_errors = atoi(argv[5]), cfg.allow_unpinned_field_cabac = atoi(argv[6]);
    h264mi_decoder *dec = nullptr;
    if (h264mi_decoder_create(&cfg, &dec) != 0) { fprintf(stderr, "create: %s\n", h264mi_last_error_string()); return 1; }
    std::vector<char> text(1 << 16);
    for (size_t b = 0; b < files.size(); b++) {
        printf("batch %zu\n", b);
        const uint8_t *bufs[1] = {files[b].data()};
        size_t lens[1] = {files[b].size()};
        h264mi_batch_info info;
        int32_t r = h264mi_batch_prepare(dec, 1, bufs, lens, &info), st = 0;
        h264mi_stream_status(dec, 0, &st);
        if (r != 0 || st != 0) {
            printf("refused prepare=%d status=%d: %s\n", r, st, h264mi_last_error_string());
            break;
        }
        if (h264mi_batch_execute(dec) != 0 || h264mi_batch_sync(dec) != 0) { fprintf(stderr, "execute: %s\n", h264mi_last_error_string()); return 1; }
        size_t len = 0;
        while ((r = h264mi_internal_dpb_trace(dec, 0, text.data(), text.size(), &len)) == H264MI_ECAPACITY) text.resize(len + 1);
        if (r != 0) return 1;
        fwrite(text.data(), 1, len, stdout);
    }
    h264mi_decoder_destroy(dec);
    return 0;
}
