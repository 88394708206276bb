// tools/host_dpb_trace.cpp -- TEST TOOLING: the host side of libh264mi, hooks build, against tools/hoststub (a null device: kernels are
// not run) decodes one or more Annex-B files, one batch per file on the same decoder, and prints after every batch what prepare
// made of it (h264mi_internal_dpb_trace: pictures, slices with their reference lists, output frames, the reference / held
// frame slots and the POC / frame_num history, then the batch's launch lists, levels and per-batch choices).  A batch that is refused
// prints its status code and message instead and ends the run: refusals are part of the behaviour tests/test_host_dpb_trace.py pins.
// With -sN in front of the files a batch is N files, one per stream of a decoder with N streams and isolation on: every stream's trace
// is printed under a "stream k" line, a refused stream's status and message first -- it leaves the batch, the run goes on.
#include "h264mi.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int32_t h264mi_internal_dpb_trace(h264mi_decoder *, int32_t stream, char *buf, size_t cap, size_t *len);

int main(int argc, char **argv) {
    int first = 7, S = 1;
    if (argc > 7 && !strncmp(argv[7], "-s", 2)) S = atoi(argv[7] + 2), first = 8;
    if (argc < first + 1 || S < 1 || (argc - first) % S) {
        fprintf(stderr, "usage: host_dpb_trace max_width max_height max_frames max_slices conceal_errors allow_unpinned_field_cabac [-sSTREAMS] stream.h264...\n");
        return 2;
    }
    const bool multi = first == 8;
    std::vector<std::vector<uint8_t>> files;
    size_t longest = 0;
    for (int a = first; a < argc; a++) {
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
    cfg.max_streams = S, cfg.max_width = atoi(argv[1]), cfg.max_height = atoi(argv[2]), cfg.max_frames_per_batch = atoi(argv[3]);
    cfg.max_slices_per_frame = atoi(argv[4]), cfg.max_bitstream_bytes = static_cast<int64_t>(longest + 4096) * S;
    cfg.conceal_errors = atoi(argv[5]), cfg.allow_unpinned_field_cabac = atoi(argv[6]);
    h264mi_decoder *dec = nullptr;
    if (h264mi_decoder_create(&cfg, &dec) != 0) { fprintf(stderr, "create: %s\n", h264mi_last_error_string()); return 1; }
    if (multi) h264mi_decoder_set_isolation(dec, 1);
    std::vector<char> text(1 << 16);
    for (size_t b = 0; b < files.size() / S; b++) {
        printf("batch %zu\n", b);
        std::vector<const uint8_t *> bufs(S);
        std::vector<size_t> lens(S);
        for (int k = 0; k < S; k++) bufs[k] = files[b * S + k].data(), lens[k] = files[b * S + k].size();
        h264mi_batch_info info;
        int32_t r = h264mi_batch_prepare(dec, S, bufs.data(), lens.data(), &info), st = 0;
        h264mi_stream_status(dec, 0, &st);
        if (r != 0 || (st != 0 && !multi)) {
            printf("refused prepare=%d status=%d: %s\n", r, st, h264mi_last_error_string());
            break;
        }
        if (h264mi_batch_execute(dec) != 0 || h264mi_batch_sync(dec) != 0) { fprintf(stderr, "execute: %s\n", h264mi_last_error_string()); return 1; }
        for (int k = 0; k < S; k++) {
            if (multi) {
                printf("stream %d\n", k);
                h264mi_stream_status(dec, k, &st);
                if (st != 0) printf("left status=%d: %s\n", st, h264mi_last_error_string()); // (the message of the last refusal: the cases refuse one stream)
            }
            size_t len = 0;
            while ((r = h264mi_internal_dpb_trace(dec, k, text.data(), text.size(), &len)) == H264MI_ECAPACITY) text.resize(len + 1);
            if (r != 0) return 1;
            fwrite(text.data(), 1, len, stdout);
        }
    }
    h264mi_decoder_destroy(dec);
    return 0;
}
