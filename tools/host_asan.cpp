// tools/host_asan.cpp -- TEST TOOLING: drives the host side of libh264mi (built against tools/hoststub: a null device,
// kernels not run) under AddressSanitizer / UBSan with intact and damaged streams, in the call orders a client uses:
// prepare / execute / sync in chunks of whole access units, several streams side by side, per-stream resets, isolation
// on and off, frame queries and read-back.  Built and run by tools/host_asan.sh.
#include "h264mi.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

static std::vector<uint8_t> slurp(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(n);
    if (fread(v.data(), 1, n, f) != static_cast<size_t>(n)) v.clear();
    fclose(f);
    return v;
}

// cut positions in front of the NAL units that may begin an access unit (SPS, or a slice with first_mb_in_slice == 0)
static std::vector<size_t> au_cuts(const std::vector<uint8_t> &s) {
    std::vector<h264mi_nal> nals(8192);
    int32_t n = 0;
    h264mi_annexb_scan(s.data(), s.size(), nals.data(), static_cast<int32_t>(nals.size()), &n);
    std::vector<size_t> cuts;
    bool in_ps = false;
    for (int i = 0; i < n; i++) {
        const uint8_t *p = s.data() + nals[i].offset;
        const int type = p[0] & 31;
        const bool ps = type == 7 || type == 8 || type == 6 || type == 9;
        const bool first_slice = (type == 1 || type == 5) && nals[i].num_bytes > 1 && (p[1] & 0x80);
        if ((ps && !in_ps) || (first_slice && !in_ps)) {
            size_t o = nals[i].offset;
            while (o > 0 && s[o - 1] == 0) o--;  // back over the start code
            if (o >= 1 && s[o] == 0) cuts.push_back(o);
            else if (nals[i].offset >= 3) cuts.push_back(nals[i].offset - 3);
        }
        in_ps = ps;
    }
    if (cuts.empty() || cuts[0] != 0) cuts.insert(cuts.begin(), 0);
    cuts.push_back(s.size());
    return cuts;
}

static std::vector<std::vector<uint8_t>> streams;
static std::atomic<long> batches{0}, ok_streams{0}, failed_streams{0}, frames{0}, refused{0}, concealing{0};
static std::atomic<long> codes[64];

// one client: `iters` decoders one after the other, each fed its own random mix of streams
static void client(int iters, unsigned seed) {
    std::mt19937 rng(seed);
    std::mt19937 crng(seed ^ 0x5bd1e995u); // error concealment is drawn from a generator of its own: everything else a seed draws stays what it was
    std::mt19937 trng(seed ^ 0x9e3779b9u); // ... and so are the model-input (K9) calls
    static const int conceal_values[] = {0, 0, 0, 1, 3, 5, 7, 17, 19, 21, 23}; // every legal value of h264mi_config.conceal_errors
    std::vector<uint8_t> pix(4 << 20);
    for (int it = 0; it < iters; it++) {
        const int ns = 1 + rng() % 4;
        h264mi_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = rng() % 8 == 0 ? offsetof(h264mi_config, b_pictures) : sizeof cfg; // (now and then a caller built against this header before `b_pictures` was added)
        if (rng() % 5 == 0) cfg.b_pictures = 1;
        cfg.max_streams = ns;
        const bool tight = rng() % 3 == 0;  // a decoder sized too small for some of what it will be given
        cfg.max_width = tight ? 64 + 16 * (rng() % 12) : 352;
        cfg.max_height = tight ? 64 + 16 * (rng() % 10) : 288;
        cfg.max_frames_per_batch = 1 + rng() % 8;
        cfg.max_slices_per_frame = tight ? 1 + rng() % 40 : 64;
        cfg.max_bitstream_bytes = tight ? 4096 << (rng() % 9) : 4 << 20;
        if (rng() % 4 == 0) cfg.max_ref_frames = 1 + rng() % 16;
        if (rng() % 4 == 0) cfg.coef_blocks_per_mb = 1 + rng() % 26;
        const int conceal = conceal_values[crng() % (sizeof conceal_values / sizeof conceal_values[0])];
        if (cfg.struct_size == sizeof cfg) cfg.conceal_errors = conceal; // (the short struct of an older caller ends in front of the field)
        h264mi_decoder *dec = nullptr;
        if (h264mi_decoder_create(&cfg, &dec) != 0 || !dec) { refused++; continue; }
        if (cfg.conceal_errors) concealing++;
        if (rng() % 3 == 0) h264mi_decoder_set_isolation(dec, rng() & 1);
        // per stream: a (possibly damaged) copy and its cut list
        std::vector<std::vector<uint8_t>> data(ns);
        std::vector<std::vector<size_t>> cuts(ns);
        std::vector<size_t> pos(ns, 0);
        const bool damage = it % 3 != 0;
        for (int s = 0; s < ns; s++) {
            data[s] = streams[rng() % streams.size()];
            cuts[s] = au_cuts(data[s]);
            if (damage && rng() % 4 != 0) {
                const int flips = 1 + rng() % 10;
                for (int k = 0; k < flips; k++) data[s][rng() % data[s].size()] ^= 1u << (rng() % 8);
                if (rng() % 5 == 0) {  // splice a window of another stream in
                    const auto &o = streams[rng() % streams.size()];
                    size_t l = 1 + rng() % std::min<size_t>(o.size(), 600), so = rng() % (o.size() - l + 1), d = rng() % data[s].size();
                    l = std::min(l, data[s].size() - d);
                    memcpy(data[s].data() + d, o.data() + so, l);
                }
            }
        }
        for (int round = 0; round < 40; round++) {
            std::vector<const uint8_t *> bufs(ns, nullptr);
            std::vector<size_t> lens(ns, 0);
            bool any = false;
            for (int s = 0; s < ns; s++) {
                if (pos[s] + 1 >= cuts[s].size() || rng() % 7 == 0) continue;
                size_t take = 1 + rng() % cfg.max_frames_per_batch;
                if (rng() % 9 == 0) take += 3;  // sometimes more than the decoder was sized for
                size_t e = std::min(pos[s] + take, cuts[s].size() - 1);
                bufs[s] = data[s].data() + cuts[s][pos[s]];
                lens[s] = cuts[s][e] - cuts[s][pos[s]];
                if (damage && rng() % 11 == 0 && lens[s] > 8) lens[s] -= 1 + rng() % 7;  // a chunk cut short
                pos[s] = e;
                any = true;
            }
            if (!any) break;
            h264mi_batch_info info;
            int32_t r = h264mi_batch_prepare(dec, ns, bufs.data(), lens.data(), &info);
            batches++;
            if (r == 0) {
                h264mi_batch_execute(dec);
                if (rng() % 3) h264mi_batch_sync(dec);
            }
            for (int s = 0; s < ns; s++) {
                int32_t st = 0, nf = 0;
                h264mi_stream_status(dec, s, &st);
                if (st == 0) ok_streams++; else failed_streams++;
                codes[st <= 0 && st > -64 ? -st : 63]++;
                if (h264mi_stream_frame_count(dec, s, &nf) != 0) continue;
                frames += nf;
                int32_t order[64], no = 0;
                h264mi_stream_output_order(dec, s, order, 64, &no);
                for (int f = 0; f < nf + 1; f++) {  // one past the end on purpose
                    h264mi_frame_info fi;
                    if (h264mi_frame_get_info(dec, s, f, &fi) != 0) continue;
                    if (rng() % 4 == 0) h264mi_frame_read(dec, s, f, rng() & 1, pix.data(), rng() % 5 ? pix.size() : 1000);
                }
                // K7's host side (descriptor tables, AUTO per frame, sizes, capacity); the choices come from nf, not from rng(): the sequence above stays what it was
                size_t conv = 0;
                int32_t mc = 0, fr = 0;
                h264mi_frame_colour(dec, s, nf / 2, &mc, &fr);
                h264mi_batch_convert_device(dec, (nf & 1) ? s : -1, 1 + nf % 3, nf % 3 ? (nf & 2) * 16 : 0, pix.data(), (nf & 4) ? pix.size() : 1000, &conv);
                h264mi_frame_convert_device(dec, s, nf - 1, 3, H264MI_CSC_BT601 | H264MI_CSC_FULL_RANGE, pix.data(), pix.size());
                // K8's host side (sizes, filters, area's downscale-only and 32-bit checks, AUTO per frame, capacity), chosen from nf in the same way
                h264mi_batch_scale_device(dec, (nf & 1) ? s : -1, nf % 4, nf % 4 >= 2 ? (nf & 2) * 16 : 0, 1 + (nf * 37) % 300, 1 + (nf * 53) % 200, nf & 1, pix.data(),
                                          (nf & 4) ? pix.size() : 1000, &conv);
                h264mi_frame_scale_device(dec, s, nf - 1, 0, 0, 16384, 1, H264MI_SCALE_BILINEAR, pix.data(), pix.size());
                h264mi_frame_scale_device(dec, s, 0, 3, H264MI_CSC_BT709, 8, 8, 2 - (nf & 3), pix.data(), pix.size());
                // K9's host side (spec validation, regions, placement, area's checks per item, AUTO per item, alignment, capacity): random specs, most
                // of them legal, and items that are legal, one past the frame, at odd origins, of other streams and frames; short and full capacity
                {
                    h264mi_tensor_spec sp;
                    memset(&sp, 0, sizeof sp);
                    sp.format = trng() % 8 ? 2 + trng() % 2 : static_cast<int32_t>(trng() % 6) - 1;
                    sp.dtype = trng() % 8 ? trng() % 4 : static_cast<int32_t>(trng() % 7) - 2;
                    sp.csc = trng() % 8 ? (trng() % 3) | ((trng() & 1) * 32) : static_cast<int32_t>(trng() % 64);
                    sp.out_w = trng() % 16 ? 1 + trng() % 700 : static_cast<int32_t>(trng() % 16387) - 1;
                    sp.out_h = trng() % 16 ? 1 + trng() % 700 : static_cast<int32_t>(trng() % 16387) - 1;
                    sp.filter = trng() % 16 ? trng() % 2 : 2, sp.fit = trng() % 16 ? trng() % 2 : -1, sp.flags = trng() % 16 ? trng() % 2 : 2;
                    for (int c = 0; c < 3; c++) {
                        sp.pad[c] = static_cast<uint8_t>(trng());
                        sp.scale[c] = sp.dtype == H264MI_DT_U8 && trng() % 8 ? 1.0f : trng() % 32 ? 1.0f / (1 + trng() % 255) : INFINITY;
                        sp.bias[c] = sp.dtype == H264MI_DT_U8 && trng() % 8 ? 0.0f : trng() % 32 ? -0.5f * (trng() % 5) : NAN;
                    }
                    size_t one = 0, got = 0;
                    h264mi_tensor_size(&sp, &one);
                    h264mi_frame_info fi;
                    memset(&fi, 0, sizeof fi);
                    const bool have = nf > 0 && h264mi_frame_get_info(dec, s, 0, &fi) == 0 && fi.width > 0 && fi.height > 0;
                    std::vector<h264mi_tensor_item> items(trng() % 6);
                    for (auto &it : items) {
                        it.stream = trng() % 16 ? s : static_cast<int32_t>(trng() % (ns + 2)) - 1;
                        it.frame = trng() % 16 ? static_cast<int32_t>(trng() % (nf + 1)) : -1; // nf: one past the end
                        const int W = have ? fi.width : 16, H = have ? fi.height : 16;
                        switch (trng() % 6) {
                        case 0: it.x = it.y = it.w = it.h = 0; break;
                        case 1: it.x = 2 * (trng() % ((W + 1) / 2)), it.y = 2 * (trng() % ((H + 1) / 2)), it.w = W - it.x + 1, it.h = H - it.y; break; // one past the right edge
                        case 2: it.x = 1, it.y = 0, it.w = 1, it.h = 1; break;                                                                   // an odd origin
                        case 3: it.x = 0, it.y = 0, it.w = 0, it.h = 1 + trng() % H; break;
                        default: it.x = 2 * (trng() % ((W + 1) / 2)), it.y = 2 * (trng() % ((H + 1) / 2)), it.w = 1 + trng() % (W - it.x), it.h = 1 + trng() % (H - it.y); break;
                        }
                    }
                    const size_t cap = trng() % 3 ? pix.size() : (one * items.size() ? one * items.size() - 1 : 0);
                    h264mi_items_tensor_device(dec, &sp, items.data(), static_cast<int32_t>(items.size()), pix.data() + (trng() % 8 ? 0 : 1 + trng() % 3), cap, &got);
                    h264mi_batch_tensor_device(dec, trng() % 2 ? s : -1, &sp, pix.data(), trng() % 3 ? pix.size() : 1000, &got);
                    int32_t px, py, sw, sh;
                    h264mi_fit_rect(trng() % 3, 1 + trng() % 16384, 1 + trng() % 16384, 1 + trng() % 16384, static_cast<int32_t>(trng() % 16386), &px, &py, &sw, &sh);
                }
                if (rng() % 13 == 0) h264mi_stream_reset(dec, s);
            }
            if (rng() % 29 == 0) h264mi_decoder_reset(dec);
        }
        h264mi_decoder_destroy(dec);
    }
}

int main(int argc, char **argv) {
    // H264MI_HOST_THREADS=N: N clients side by side, each with its own decoders (what the library promises: decoders are independent;
    // the interesting run is the ThreadSanitizer build, SAN=thread in tools/host_asan.sh)
    if (argc < 4) { fprintf(stderr, "usage: host_asan iterations seed stream.h264...\n"); return 2; }
    const int iters = atoi(argv[1]);
    const unsigned seed = static_cast<unsigned>(atoi(argv[2]));
    for (int i = 3; i < argc; i++) { streams.push_back(slurp(argv[i])); if (streams.back().empty()) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; } }
    const char *nt = getenv("H264MI_HOST_THREADS");
    const int threads = nt ? std::max(1, atoi(nt)) : 1;
    if (threads == 1)
        client(iters, seed);
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++) pool.emplace_back(client, (iters + threads - 1) / threads, seed * 7919u + static_cast<unsigned>(t));
        for (auto &t : pool) t.join();
    }
    printf("host asan: %d decoders (%ld refused), %ld batches, stream results %ld ok / %ld failed, %ld frames\n", iters, refused.load(), batches.load(), ok_streams.load(),
           failed_streams.load(), frames.load());
    printf("decoders with error concealment: %ld\n", concealing.load());
    printf("stream status histogram:");
    for (int i = 0; i < 64; i++) if (codes[i].load()) printf(" %d:%ld", -i, codes[i].load());
    printf("\n");
    return 0;
}
