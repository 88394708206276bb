/*
 * examples/h264mi_decode.c -- the C ABI from plain C: decode an Annex-B file to raw I420 on the GPU.
 *
 *   h264mi_decode in.h264 out.yuv [frames_per_batch] [--random-access] [--conceal...] [--nv12 | --rgb] [--scale WxH[:area] | --tensor WxH] [--deinterlace field|blend|edge|motion|motion-edge] [--field-rate] [--stats] [--jpeg PREFIX [--quality N]]
 *
 * --nv12 / --rgb write NV12 / tight R, G, B bytes instead of I420: the frames are converted on the device (h264mi_batch_convert_device into a
 * device buffer, matrix and range from each frame's own SPS) and copied to the host from there.  --scale WxH writes every frame at W x H instead of
 * its display size (h264mi_batch_scale_device: bilinear, or the area filter with ":area"; I420 unless --nv12 / --rgb is given).  --tensor WxH writes
 * every frame as a model-input item instead (h264mi_batch_tensor_device): letterboxed into a W x H canvas on grey (114, 114, 114), float32 in three
 * planes R, G, B, each value v / 255 (scale 1 / 255, bias 0), bilinear, matrix and range from each frame's own SPS.  --deinterlace MODE deinterlaces
 * every frame on the device first (h264mi_batch_deinterlace: the first field's parity is kept) and writes the derived frames -- through whichever of
 * the paths above is chosen -- instead of the woven ones; with --field-rate two per frame, the first field's then the second's.  --deinterlace motion /
 * motion-edge are the motion-adaptive modes that pull from field / edge (h264mi_batch_deinterlace_motion with H264MI_DEINT_HISTORY): a frame is
 * deinterlaced against the frame before it in output order, and the first frame of a batch against the last one of the batch before, so a file decoded
 * in several batches (frames_per_batch) comes out as if it had been decoded in one.  --stats prints one line per decoded frame to stdout, in decoding
 * order: its mean luma, its mean absolute luma difference against the frame before it in output order, and how many luma samples changed by more than 8
 * (h264mi_batch_stats_device with H264MI_STATS_HISTORY -- on the first batch too, or no later batch had a predecessor for its first frame).  --jpeg PREFIX
 * writes every frame (with --deinterlace: every derived frame) as a baseline JPEG file PREFIX%05d.jpg as well, encoded on the device
 * (h264mi_batch_jpeg_device, H264MI_JPEG_RANGE_AUTO; --quality N, 1 .. 100, default 90): a slot of the header plus w * h / 2 bytes per frame, and a
 * second call with the size they asked for if frames report H264MI_JPEG_TRUNCATED.  The HIP
 * calls of these paths are the only HIP this file needs; they are declared below, so it still builds without the HIP headers.
 *
 * The file includes nothing but include/h264mi.h and the C library.
 *
 * What a Go/cgo (or any FFI) caller does is exactly this sequence: cut the byte
 * stream at access units, hand whole access units to h264mi_decode_batch, read the frames back.
 * The access-unit cut below is the same rule as AccessUnitSplitter in h264decode_amd/h264.py
 * (a new picture starts at an access unit delimiter, at a parameter set / SEI that follows a
 * slice, or at the first slice of a new picture: h264mi_slice_starts_picture on the parsed slice
 * headers, or a slice that starts where a slice of the current picture already started -- with
 * slice groups or arbitrary slice order "first_mb_in_slice == 0" is not that test).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h264mi.h"

/* The three HIP runtime calls of --nv12 / --rgb, declared by hand so that the file builds with gcc and without the HIP headers
 * (hip/hip_runtime_api.h: hipError_t and hipMemcpyKind are enums, int-sized in the C ABI; 0 = hipSuccess, hipMemcpyDeviceToHost = 2).  The program
 * therefore links the HIP runtime itself (examples/Makefile), which the I420 path alone would not need: libh264mi.so brings it along anyway. */
extern int hipMalloc(void **ptr, size_t size);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind);
extern int hipFree(void *ptr);

static int fail(const char *what, int code) {
    fprintf(stderr, "%s failed: %d (%s)\n", what, code, h264mi_last_error_string());
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s in.h264 out.yuv [frames_per_batch] [--random-access] [--conceal | --conceal-all | --conceal-idr | --conceal-lone-fields] [--nv12 | --rgb] [--scale WxH[:area] | --tensor WxH] [--deinterlace field|blend|edge|motion|motion-edge] [--field-rate] [--stats] [--jpeg PREFIX [--quality N]]\n", argv[0]);
        return 2;
    }
    const char *jpeg_prefix = NULL; /* --jpeg PREFIX [--quality N] (the last arguments of all): every frame as PREFIX%05d.jpg too */
    int jpeg_quality = 90;
    if (argc > 6 && !strcmp(argv[argc - 2], "--quality") && !strcmp(argv[argc - 4], "--jpeg")) jpeg_quality = atoi(argv[argc - 1]), argc -= 2;
    if (argc > 4 && !strcmp(argv[argc - 2], "--jpeg")) jpeg_prefix = argv[argc - 1], argc -= 2;
    int stats = 0; /* --stats (the last argument before those): the frame statistics of every batch, on stdout */
    if (argc > 3 && !strcmp(argv[argc - 1], "--stats")) stats = 1, argc--;
    int deint = -1, deint_rate = 1, deint_motion = 0; /* --deinterlace MODE and --field-rate (the last arguments of all): derived frames instead of the woven ones */
    if (argc > 3 && !strcmp(argv[argc - 1], "--field-rate")) deint_rate = 2, argc--;
    if (argc > 4 && !strcmp(argv[argc - 2], "--deinterlace")) {
        const char *m = argv[argc - 1];
        deint_motion = !strncmp(m, "motion", 6); /* motion: pulled from field; motion-edge: from edge */
        if (deint_motion) m = !strcmp(m, "motion") ? "field" : !strcmp(m, "motion-edge") ? "edge" : "";
        deint = !strcmp(m, "field") ? H264MI_DEINT_FIELD : !strcmp(m, "blend") ? H264MI_DEINT_BLEND : !strcmp(m, "edge") ? H264MI_DEINT_EDGE : -1;
        if (deint < 0) {
            fprintf(stderr, "--deinterlace %s: expected field, blend, edge, motion or motion-edge\n", argv[argc - 1]);
            return 2;
        }
        argc -= 2;
    }
    if (deint < 0 && deint_rate == 2) {
        fprintf(stderr, "--field-rate needs --deinterlace\n");
        return 2;
    }
    int scale_w = 0, scale_h = 0, scale_filter = H264MI_SCALE_BILINEAR; /* --scale WxH[:area] (the last two arguments): every frame at W x H */
    if (argc > 4 && !strcmp(argv[argc - 2], "--scale")) {
        char tail[8] = "";
        const int got = sscanf(argv[argc - 1], "%dx%d%7s", &scale_w, &scale_h, tail);
        if (got < 2 || scale_w < 1 || scale_h < 1 || (got == 3 && strcmp(tail, ":area"))) {
            fprintf(stderr, "--scale %s: expected WxH or WxH:area\n", argv[argc - 1]);
            return 2;
        }
        if (got == 3) scale_filter = H264MI_SCALE_AREA;
        argc -= 2;
    }
    h264mi_tensor_spec tensor; /* --tensor WxH (the last two arguments, instead of --scale): every frame as a letterboxed float32 CHW item */
    memset(&tensor, 0, sizeof(tensor));
    if (!scale_w && argc > 4 && !strcmp(argv[argc - 2], "--tensor")) {
        char tail[2] = "";
        if (sscanf(argv[argc - 1], "%dx%d%1s", &tensor.out_w, &tensor.out_h, tail) != 2 || tensor.out_w < 1 || tensor.out_h < 1) {
            fprintf(stderr, "--tensor %s: expected WxH\n", argv[argc - 1]);
            return 2;
        }
        tensor.format = H264MI_FMT_RGBP, tensor.dtype = H264MI_DT_F32, tensor.csc = H264MI_CSC_AUTO;
        tensor.filter = H264MI_SCALE_BILINEAR, tensor.fit = H264MI_FIT_LETTERBOX;
        for (int c = 0; c < 3; c++) tensor.pad[c] = 114, tensor.scale[c] = 1.0f / 255.0f, tensor.bias[c] = 0.0f;
        argc -= 2;
    }
    int format = H264MI_FMT_I420; /* --nv12 / --rgb (last argument but for --scale): the output format */
    if (argc > 3 && !strcmp(argv[argc - 1], "--nv12")) format = H264MI_FMT_NV12, argc--;
    else if (argc > 3 && !strcmp(argv[argc - 1], "--rgb")) format = H264MI_FMT_RGB24, argc--;
    int conceal = 0; /* --conceal (last argument but for the format): h264mi_config.conceal_errors */
    if (argc > 3 && !strcmp(argv[argc - 1], "--conceal")) conceal = H264MI_CONCEAL_SLICES, argc--;
    /* --conceal-all: wholly lost reference frames and slices of field pictures are concealed too */
    else if (argc > 3 && !strcmp(argv[argc - 1], "--conceal-all")) conceal = H264MI_CONCEAL_SLICES | H264MI_CONCEAL_PICTURES | H264MI_CONCEAL_FIELDS, argc--;
    /* --conceal-idr: all of that, and slices of IDR frame pictures that still have a reference frame */
    else if (argc > 3 && !strcmp(argv[argc - 1], "--conceal-idr"))
        conceal = H264MI_CONCEAL_SLICES | H264MI_CONCEAL_PICTURES | H264MI_CONCEAL_FIELDS | H264MI_CONCEAL_IDR, argc--;
    /* --conceal-lone-fields: what --conceal-all conceals, and the wholly lost field of a frame coded as two field pictures */
    else if (argc > 3 && !strcmp(argv[argc - 1], "--conceal-lone-fields"))
        conceal = H264MI_CONCEAL_SLICES | H264MI_CONCEAL_PICTURES | H264MI_CONCEAL_FIELDS | H264MI_CONCEAL_LONE_FIELDS, argc--;
    /* --random-access (last argument but for the concealment): a file that starts in the middle of a stream -- cut from a broadcast, or read from a seek
     * position on -- is decoded from its first recovery point on (h264mi_decoder_set_random_access); without it only from an IDR picture on */
    int random_access = 0;
    if (argc > 3 && !strcmp(argv[argc - 1], "--random-access")) random_access = 1, argc--;
    const int per_batch = argc > 3 ? atoi(argv[3]) : 30;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("fopen", -1);
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *buf = (uint8_t *)malloc((size_t)len);
    if (fread(buf, 1, (size_t)len, f) != (size_t)len) return fail("fread", -1);
    fclose(f);

    /* NAL table + picture size from the first SPS */
    int32_t cap = 1 << 16, n = 0, r;
    h264mi_nal *nals = (h264mi_nal *)malloc(sizeof(h264mi_nal) * (size_t)cap);
    while ((r = h264mi_annexb_scan(buf, (size_t)len, nals, cap, &n)) == H264MI_ECAPACITY) {
        cap *= 4;
        nals = (h264mi_nal *)realloc(nals, sizeof(h264mi_nal) * (size_t)cap);
    }
    if (r != H264MI_OK) return fail("h264mi_annexb_scan", r);
    h264mi_sps sps;
    memset(&sps, 0, sizeof(sps));
    for (int i = 0; i < n; i++)
        if (nals[i].type == 7) {
            uint8_t *rbsp = (uint8_t *)malloc((size_t)nals[i].num_bytes);
            size_t rl = 0;
            h264mi_nal hdr;
            if ((r = h264mi_nal_parse(buf + nals[i].offset, (size_t)nals[i].num_bytes, &hdr, rbsp, &rl)) != H264MI_OK) return fail("h264mi_nal_parse", r);
            if ((r = h264mi_sps_parse(rbsp, rl, &sps)) != H264MI_OK) return fail("h264mi_sps_parse", r);
            free(rbsp);
            break;
        }
    if (!sps.width) return fail("no SPS found", H264MI_EBITSTREAM);

    h264mi_config cfg = H264MI_CONFIG_INIT; /* zero-initialised, struct_size = this build's sizeof */
    cfg.max_streams = 1, cfg.max_width = sps.width, cfg.max_height = sps.height;
    /* (frames inserted for lost pictures count against max_frames_per_batch: headroom for the longest gap that is concealed) */
    cfg.max_frames_per_batch = per_batch + (conceal & H264MI_CONCEAL_PICTURES ? H264MI_CONCEAL_MAX_GAP : 0), cfg.max_slices_per_frame = 32, cfg.max_bitstream_bytes = len + (1 << 20);
    cfg.conceal_errors = conceal;
    h264mi_decoder *dec = NULL;
    if ((r = h264mi_decoder_create(&cfg, &dec)) != H264MI_OK) return fail("h264mi_decoder_create", r);
    if (random_access && (r = h264mi_decoder_set_random_access(dec, H264MI_RA_RECOVERY_POINT)) != H264MI_OK) return fail("h264mi_decoder_set_random_access", r);

    FILE *out = fopen(argv[2], "wb");
    const size_t fsz = H264MI_I420_SIZE(sps.width, sps.height);
    uint8_t *frame = NULL;
    size_t frame_cap = 0;
    void *dev = NULL; /* --nv12 / --rgb: the converted frames of a batch on the device */
    size_t dev_cap = 0;
    void *sdev = NULL; /* --stats: the records of a batch on the device, and their host copy */
    h264mi_frame_stats *srec = NULL;
    size_t sdev_cap = 0;
    void *jdev = NULL; /* --jpeg: results and slots of a batch on the device, and their host copy */
    uint8_t *jhost = NULL;
    size_t jdev_cap = 0, jslot = 0;
    long jpeg_total = 0;
    long stats_total = 0; /* frames reported so far (total counts what is written: two per frame with --field-rate) */
    const h264mi_stats_spec sspec = {0, 0, 8, 0}; /* no grid; changed_y counts |S - P| > 8 */
    long total = 0;
    int start = 0, pics = 0, seen_vcl = 0;
    /* parameter sets by id and the slices of the current picture, for the picture-boundary test */
    static h264mi_sps sps_tab[32];
    static h264mi_pps pps_tab[256];
    static uint8_t sps_ok[32], pps_ok[256];
    static h264mi_slice_header first_hdr, hdr;
    static int32_t first_mbs[1024];
    int n_first = 0, have_first = 0;
    uint8_t *rb = (uint8_t *)malloc((size_t)len + 16);
    for (int i = 0; i <= n; i++) {
        int cut = i == n;
        if (!cut) {
            const int t = nals[i].type;
            const uint8_t *p = buf + nals[i].offset;
            size_t rl = 0;
            h264mi_nal nh;
            if (t == 7 || t == 8) {
                if (h264mi_nal_parse(p, (size_t)nals[i].num_bytes, &nh, rb, &rl) == H264MI_OK) {
                    if (t == 7) {
                        h264mi_sps tmp;
                        if (h264mi_sps_parse(rb, rl, &tmp) == H264MI_OK && tmp.id >= 0 && tmp.id < 32) sps_tab[tmp.id] = tmp, sps_ok[tmp.id] = 1;
                    } else
                        for (int k = 0; k < 32; k++) { /* seq_parameter_set_id is inside: let every SPS try */
                            h264mi_pps tmp;
                            if (sps_ok[k] && h264mi_pps_parse(&sps_tab[k], rb, rl, &tmp) == H264MI_OK && tmp.sps_id == k && tmp.id >= 0 && tmp.id < 256) {
                                pps_tab[tmp.id] = tmp, pps_ok[tmp.id] = 1;
                                break;
                            }
                        }
                }
            }
            if (t == 1 || t == 5) {
                int new_pic = -1;
                if (h264mi_nal_parse(p, (size_t)nals[i].num_bytes, &nh, rb, &rl) == H264MI_OK)
                    for (int k = 0; k < 256 && new_pic < 0; k++) /* pic_parameter_set_id is inside: let every PPS try */
                        if (pps_ok[k] && sps_ok[pps_tab[k].sps_id] &&
                            h264mi_slice_header_parse(&sps_tab[pps_tab[k].sps_id], &pps_tab[k], nh.ref_idc, nh.type, rb, rl, &hdr) == H264MI_OK && hdr.pps_id == k) {
                            new_pic = 0;
                            for (int m = 0; m < n_first; m++) new_pic |= first_mbs[m] == hdr.first_mb_in_slice;
                            if (have_first && h264mi_slice_starts_picture(&sps_tab[pps_tab[k].sps_id], &first_hdr, &hdr) == 1) new_pic = 1;
                        }
                if (new_pic < 0) { /* parameter sets unknown: first_mb_in_slice == 0 */
                    new_pic = (p[1] & 0x80) != 0;
                    memset(&hdr, 0, sizeof(hdr));
                    hdr.first_mb_in_slice = new_pic ? 0 : -1;
                }
                if (new_pic && seen_vcl) cut = 1;
                if (cut || !seen_vcl) n_first = 0, have_first = 0;
                if (!have_first) first_hdr = hdr, have_first = 1;
                if (n_first < 1024) first_mbs[n_first++] = hdr.first_mb_in_slice;
            } else if ((t >= 6 && t <= 9) && seen_vcl)
                cut = 1, n_first = 0, have_first = 0;
        }
        if (cut && seen_vcl) {
            pics++;
            seen_vcl = 0;
            if (pics == per_batch || i == n) { /* decode nals[start .. i) */
                const size_t b0 = (size_t)nals[start].offset >= 4 ? (size_t)nals[start].offset - 4 : 0; /* include the start code */
                const size_t b1 = i == n ? (size_t)len : (size_t)nals[i].offset - 3;
                const uint8_t *ptr = buf + b0;
                const size_t l = b1 - b0;
                h264mi_batch_info info;
                if ((r = h264mi_decode_batch(dec, 1, &ptr, &l, &info)) != H264MI_OK) return fail("h264mi_decode_batch", r);
                int32_t k = 0, src = 0; /* src: the stream the frames are taken from */
                h264mi_stream_frame_count(dec, 0, &k);
                if (stats) { /* one launch makes the records of the batch (without a grid a record is an item); the size query as for the formats below */
                    size_t bytes = 0;
                    r = h264mi_batch_stats_device(dec, 0, &sspec, H264MI_STATS_HISTORY, sdev ? sdev : (void *)nals, 0, &bytes);
                    if (r != H264MI_OK && r != H264MI_ECAPACITY) return fail("h264mi_batch_stats_device", r);
                    if (bytes > sdev_cap) {
                        if (sdev) hipFree(sdev);
                        if (hipMalloc(&sdev, sdev_cap = bytes) != 0) return fail("hipMalloc", H264MI_ENOMEM);
                        srec = (h264mi_frame_stats *)realloc(srec, bytes);
                    }
                    if (bytes && (r = h264mi_batch_stats_device(dec, 0, &sspec, H264MI_STATS_HISTORY, sdev, sdev_cap, &bytes)) != H264MI_OK) return fail("h264mi_batch_stats_device", r);
                    if ((r = h264mi_batch_sync(dec)) != H264MI_OK) return fail("h264mi_batch_sync", r);
                    if (bytes && hipMemcpy(srec, sdev, bytes, 2 /* hipMemcpyDeviceToHost */) != 0) return fail("hipMemcpy", H264MI_EDEVICE);
                    for (size_t q = 0; q < bytes / sizeof(h264mi_frame_stats); q++) {
                        const h264mi_frame_stats *s = &srec[q];
                        const double px = (double)s->w * s->h;
                        printf("stats %ld: mean_y %.3f sad_y/px %.3f changed_y %u (sum_y %llu sad_y %llu has_prev %u)\n", stats_total + (long)q, (double)s->sum_y / px, (double)s->sad_y / px,
                               s->changed_y, (unsigned long long)s->sum_y, (unsigned long long)s->sad_y, s->has_prev);
                    }
                    stats_total += (long)(bytes / sizeof(h264mi_frame_stats));
                }
                if (deint >= 0) { /* one launch makes the derived frames of the batch: frames 0 .. k - 1 of the pseudo-stream */
                    if (deint_motion) { /* with the history: the batch's first frame in output order is pulled from the last one of the batch before */
                        if ((r = h264mi_batch_deinterlace_motion(dec, 0, deint, deint_rate, H264MI_DEINT_HISTORY, &k)) != H264MI_OK) return fail("h264mi_batch_deinterlace_motion", r);
                    } else if ((r = h264mi_batch_deinterlace(dec, 0, deint, deint_rate, &k)) != H264MI_OK)
                        return fail("h264mi_batch_deinterlace", r);
                    src = H264MI_STREAM_DERIVED;
                }
                if (jpeg_prefix && k > 0) { /* three launches make the files of the batch; a second round if a slot was too small */
                    const h264mi_jpeg_spec jspec = {jpeg_quality, H264MI_JPEG_RANGE_AUTO, 0, 0};
                    size_t hb = 0;
                    if ((r = h264mi_jpeg_size(&jspec, info.coded_width, info.coded_height, 0, &hb, NULL)) != H264MI_OK) return fail("h264mi_jpeg_size", r);
                    if (!jslot) jslot = (hb + (size_t)info.coded_width * info.coded_height / 2 + 15) & ~(size_t)15;
                    for (int round = 0; round < 2; round++) {
                        const size_t head = ((size_t)16 * k + 255) & ~(size_t)255;
                        size_t bytes = head + (size_t)k * jslot, need_slot = 0;
                        if (bytes > jdev_cap) {
                            if (jdev) hipFree(jdev);
                            if (hipMalloc(&jdev, jdev_cap = bytes) != 0) return fail("hipMalloc", H264MI_ENOMEM);
                            jhost = (uint8_t *)realloc(jhost, bytes);
                        }
                        if ((r = h264mi_batch_jpeg_device(dec, src, &jspec, jslot, jdev, jdev_cap, &bytes)) != H264MI_OK) return fail("h264mi_batch_jpeg_device", r);
                        if ((r = h264mi_batch_sync(dec)) != H264MI_OK) return fail("h264mi_batch_sync", r);
                        if (hipMemcpy(jhost, jdev, bytes, 2 /* hipMemcpyDeviceToHost */) != 0) return fail("hipMemcpy", H264MI_EDEVICE);
                        const h264mi_jpeg_result *res = (const h264mi_jpeg_result *)jhost;
                        for (int q = 0; q < k; q++)
                            if (res[q].status == H264MI_JPEG_TRUNCATED && res[q].bytes > need_slot) need_slot = res[q].bytes;
                        if (need_slot && round == 0) { /* the size they asked for; it stays for the batches to come */
                            jslot = (need_slot + 15) & ~(size_t)15;
                            continue;
                        }
                        for (int q = 0; q < k; q++) {
                            char name[1024];
                            snprintf(name, sizeof name, "%s%05ld.jpg", jpeg_prefix, jpeg_total + q);
                            FILE *jf = fopen(name, "wb");
                            if (!jf || res[q].status != 0) return fail(name, H264MI_EINVAL);
                            fwrite(jhost + head + (size_t)q * jslot, 1, res[q].bytes, jf);
                            fclose(jf);
                        }
                        break;
                    }
                    jpeg_total += k;
                }
                const size_t need = H264MI_I420_SIZE(info.coded_width, info.coded_height);
                if (need > frame_cap) frame = (uint8_t *)realloc(frame, frame_cap = need);
                if (tensor.out_w) { /* one launch makes the items of the batch; the size query as below */
                    size_t bytes = 0;
                    r = h264mi_batch_tensor_device(dec, src, &tensor, dev ? dev : (void *)frame, 0, &bytes);
                    if (r != H264MI_OK && r != H264MI_ECAPACITY) return fail("h264mi_batch_tensor_device", r);
                    if (bytes > dev_cap) {
                        if (dev) hipFree(dev);
                        if (hipMalloc(&dev, dev_cap = bytes) != 0) return fail("hipMalloc", H264MI_ENOMEM);
                    }
                    if (bytes > frame_cap) frame = (uint8_t *)realloc(frame, frame_cap = bytes);
                    if (bytes && (r = h264mi_batch_tensor_device(dec, src, &tensor, dev, dev_cap, &bytes)) != H264MI_OK) return fail("h264mi_batch_tensor_device", r);
                    if ((r = h264mi_batch_sync(dec)) != H264MI_OK) return fail("h264mi_batch_sync", r);
                    if (bytes && hipMemcpy(frame, dev, bytes, 2 /* hipMemcpyDeviceToHost */) != 0) return fail("hipMemcpy", H264MI_EDEVICE);
                    fwrite(frame, 1, bytes, out);
                } else if (format != H264MI_FMT_I420 || scale_w) { /* one launch converts (and scales) the batch; csc 0: matrix and range of each frame's own SPS, nearest chroma */
                    size_t bytes = 0;
                    /* the size query: with cap 0 the call resolves and sizes every frame, sets bytes, launches nothing and returns H264MI_ECAPACITY (or
                     * H264MI_OK for an empty batch) -- the destination is never touched, it only has to be non-NULL, so before the device buffer exists
                     * the host buffer's address stands in for it */
                    const char *what = scale_w ? "h264mi_batch_scale_device" : "h264mi_batch_convert_device";
                    r = scale_w ? h264mi_batch_scale_device(dec, src, format, H264MI_CSC_AUTO, scale_w, scale_h, scale_filter, dev ? dev : (void *)frame, 0, &bytes)
                                : h264mi_batch_convert_device(dec, src, format, H264MI_CSC_AUTO, dev ? dev : (void *)frame, 0, &bytes);
                    if (r != H264MI_OK && r != H264MI_ECAPACITY) return fail(what, r);
                    if (bytes > dev_cap) {
                        if (dev) hipFree(dev);
                        if (hipMalloc(&dev, dev_cap = bytes) != 0) return fail("hipMalloc", H264MI_ENOMEM);
                    }
                    if (bytes > frame_cap) frame = (uint8_t *)realloc(frame, frame_cap = bytes);
                    if (bytes) {
                        r = scale_w ? h264mi_batch_scale_device(dec, src, format, H264MI_CSC_AUTO, scale_w, scale_h, scale_filter, dev, dev_cap, &bytes)
                                    : h264mi_batch_convert_device(dec, src, format, H264MI_CSC_AUTO, dev, dev_cap, &bytes);
                        if (r != H264MI_OK) return fail(what, r);
                    }
                    if ((r = h264mi_batch_sync(dec)) != H264MI_OK) return fail("h264mi_batch_sync", r); /* the launch is asynchronous on the decoder's stream */
                    if (bytes && hipMemcpy(frame, dev, bytes, 2 /* hipMemcpyDeviceToHost */) != 0) return fail("hipMemcpy", H264MI_EDEVICE);
                    fwrite(frame, 1, bytes, out);
                } else
                    for (int fidx = 0; fidx < k; fidx++) {
                        if ((r = h264mi_frame_read(dec, src, fidx, 1, frame, frame_cap)) != H264MI_OK) return fail("h264mi_frame_read", r);
                        fwrite(frame, 1, fsz, out);
                    }
                total += k;
                start = i, pics = 0;
            }
        }
        if (i < n && (nals[i].type == 1 || nals[i].type == 5)) seen_vcl = 1;
    }
    fclose(out);
    if (conceal) { /* the totals live in the decoder: ask before it is destroyed */
        int64_t cs = 0, cm = 0;
        if (h264mi_decoder_concealed(dec, &cs, &cm) == H264MI_OK) fprintf(stderr, "concealed: %lld slices, %lld macroblocks\n", (long long)cs, (long long)cm);
        if ((conceal & H264MI_CONCEAL_PICTURES) && h264mi_decoder_concealed_pictures(dec, &cs) == H264MI_OK) fprintf(stderr, "concealed: %lld pictures\n", (long long)cs);
        if ((conceal & H264MI_CONCEAL_LONE_FIELDS) && h264mi_decoder_concealed_fields(dec, &cs) == H264MI_OK) fprintf(stderr, "concealed: %lld fields\n", (long long)cs);
    }
    if (dev) hipFree(dev);
    if (sdev) hipFree(sdev);
    if (jdev) hipFree(jdev);
    h264mi_decoder_destroy(dec);
    fprintf(stderr, "%s: %ld frames %dx%d -> %s\n", h264mi_version(), total, sps.width, sps.height, argv[2]);
    return 0;
}
