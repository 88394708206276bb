// h264decode_amd/csrc/mi_output.cpp -- the output stage of libh264mi.so: what leaves the frame pool on the device.  K6 (k_pack: tight I420), K7
// (k_convert: NV12 / RGB), K8 (k_scale: resized) and K9 (k_tensor: model input) over a list of frames of the last executed batch, K10 (k_deint and
// k_deint_motion: deinterlaced frames, which K6 .. K9 read like frames of the batch), and the device-free rule functions of include/h264mi.h that say what those
// kernels compute (h264mi_output_size, _csc_resolve, _scale_taps, _fit_rect, _tensor_size, _deint_rows, _deint_motion_pixel, _side_size), and K11 (k_side: the macroblock
// records of the batch as planes of side information), and K12 (k_stats: sums, a histogram and differences against a predecessor, per frame and per
// cell of a grid -- h264mi_stats_size and the statistics history), and K13 (k_jpeg: baseline JPEG files of frames, and the rule functions
// h264mi_jpeg_quant_table, _jpeg_block, _jpeg_size over k_jpeg_rule.h).  The nine kernel families share ONE launch discipline (stage_descs / fence_launch
// below); each has descriptor tables of its own.
// (the reference has no output process: h264/server.go:113-166 stops at the parsed slice)
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>
#include "mi_decoder.hpp"
#include "k_jpeg_rule.h"

void crop_rect(const OutFrame *of, int crop, int *x0, int *y0, int *w, int *h) {
    *x0 = *y0 = 0, *w = of->wmb * 16, *h = of->hmb * 16;
    if (crop) *x0 = of->crop_x, *y0 = of->crop_y, *w = of->width, *h = of->height;
}

// ---------------------------------------------------------------- the launch discipline of K6 .. K10
// Every call checks, resolves and sizes all of its frames first: a call that fails launches nothing and waits for nothing.  Then the descriptors go
// through the family's next table (stage_descs), one launch on the decoder's stream takes them all, and the launch is fenced (fence_launch).
typedef std::vector<std::pair<int, int>> FrameList; // (stream, frame)

// every frame of `stream`, or of all streams (-1), of the last executed batch; of H264MI_STREAM_DERIVED: every derived frame
static FrameList batch_frames(const h264mi_decoder *d, int stream) {
    FrameList frames;
    if (stream == H264MI_STREAM_DERIVED) {
        for (int f = 0; f < static_cast<int>(d->derived.size()); f++) frames.push_back({stream, f});
        return frames;
    }
    const Stage &g = d->stage[d->exec];
    for (int si = 0; si < static_cast<int>(g.out.size()); si++)
        if (stream < 0 || stream == si)
            for (int f = 0; f < static_cast<int>(g.out[si].size()); f++) frames.push_back({si, f});
    return frames;
}

// `stream` of a batch call: -1, a stream of the decoder, or the pseudo-stream of the derived frames
static bool batch_stream_ok(const h264mi_decoder *d, int stream) {
    return stream == H264MI_STREAM_DERIVED || (stream >= -1 && stream < static_cast<int>(d->st.size()));
}

// what every descriptor begins with: the frame's planes and coded size, the rectangle read, the place in the destination
template <class T> static void set_source(T &ds, const uint8_t *p, const OutFrame *of, int x0, int y0, int w, int h, size_t off) {
    ds.src = reinterpret_cast<uint64_t>(p), ds.dst_off = off;
    ds.W = of->wmb * 16, ds.H = of->hmb * 16, ds.x0 = x0, ds.y0 = y0, ds.w = w, ds.h = h;
}

// the descriptors of a call (at least one) into the next table of `t`, on their way to the device; *dev: where the kernel reads them
template <class T> static int stage_descs(h264mi_decoder *d, DescTables &t, const std::vector<T> &descs, const T **dev) {
    const int ps = t.slot ^= 1;
    if (!t.ev[ps]) HIP_TRY(hipEventCreateWithFlags(&t.ev[ps], hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(t.ev[ps])); // the launch that used this table (two calls ago) has read it
    const size_t bytes = sizeof(T) * descs.size();
    if (bytes > t.cap[ps]) {
        if (t.h[ps]) hipHostFree(t.h[ps]);
        if (t.d[ps]) hipFree(t.d[ps]);
        t.h[ps] = nullptr, t.d[ps] = nullptr, t.cap[ps] = 0;
        const size_t n = sizeof(T) * std::max<size_t>(descs.size(), 64);
        HIP_TRY(hipHostMalloc(&t.h[ps], n));
        HIP_TRY(hipMalloc(&t.d[ps], n));
        t.cap[ps] = n;
    }
    memcpy(t.h[ps], descs.data(), bytes);
    // (in order on the decoder's stream, which has waited for the reconstruction of the last executed pass: h264mi_batch_execute)
    HIP_TRY(hipMemcpyAsync(t.d[ps], t.h[ps], bytes, hipMemcpyHostToDevice, d->stream));
    *dev = static_cast<const T *>(t.d[ps]);
    return H264MI_OK;
}

// after the launch that reads the table stage_descs gave out: the table's event, which is also what the next pass waits for before it rewrites what the
// launch reads -- frames (last_pack: K6 .. K10) or macroblock records (last_side: K11)
static int fence_launch(h264mi_decoder *d, DescTables &t, hipEvent_t h264mi_decoder::*fence = &h264mi_decoder::last_pack) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t.ev[t.slot], d->stream));
    d->*fence = t.ev[t.slot];
    return H264MI_OK;
}
#define TRY(x)                        \
    do {                              \
        const int r_ = (x);           \
        if (r_ != H264MI_OK) return r_; \
    } while (0)

// ---------------------------------------------------------------- argument checks shared by the rule functions and the launches
// `names`: the formats of `allowed` (bit 1 << H264MI_FMT_*) as the message lists them
static int check_format(const char *what, int format, unsigned allowed, const char *names) {
    if (format >= 0 && format < 32 && ((allowed >> format) & 1)) return H264MI_OK;
    set_error("%s format %d: not %s", what, format, names);
    return H264MI_EINVAL;
}
static int check_filter(int filter) {
    if (filter == H264MI_SCALE_BILINEAR || filter == H264MI_SCALE_AREA) return H264MI_OK;
    set_error("scale filter %d: not H264MI_SCALE_BILINEAR or H264MI_SCALE_AREA", filter);
    return H264MI_EINVAL;
}
static int check_fit(int fit) {
    if (fit == H264MI_FIT_STRETCH || fit == H264MI_FIT_LETTERBOX) return H264MI_OK;
    set_error("fit %d: not H264MI_FIT_STRETCH or H264MI_FIT_LETTERBOX", fit);
    return H264MI_EINVAL;
}
static int check_size(const char *what, int w, int h) {
    if (w >= 1 && w <= H264MI_SCALE_MAX && h >= 1 && h <= H264MI_SCALE_MAX) return H264MI_OK;
    set_error("%s size %d x %d: both must be 1 .. %d", what, w, h, H264MI_SCALE_MAX);
    return H264MI_EINVAL;
}
// is csc legal at all (whatever the frames are, and if there are none)
static int check_csc(int csc) {
    int probe;
    return h264mi_csc_resolve(csc, 1, 0, 16, 16, &probe);
}
// H264MI_SCALE_AREA from w x h to ow x oh (the `dst`): it only scales down, and the largest weighted sum and its rounding term must fit 32 bits.
// src_fmt ...: how the message names the source, its size included
__attribute__((format(printf, 6, 7))) static int check_area(int w, int h, int ow, int oh, const char *dst, const char *src_fmt, ...) {
    const uint64_t px = static_cast<uint64_t>(w) * h;
    const bool up = ow > w || oh > h;
    if (!up && 255 * px + (px >> 1) < (static_cast<uint64_t>(1) << 32)) return H264MI_OK;
    char src[160];
    va_list ap;
    va_start(ap, src_fmt);
    vsnprintf(src, sizeof src, src_fmt, ap);
    va_end(ap);
    if (up) {
        set_error("H264MI_SCALE_AREA only scales down: %s, the %s %d x %d", src, dst, ow, oh);
        return H264MI_EINVAL;
    }
    set_error("H264MI_SCALE_AREA sums in 32 bits and needs 255 * w * h + ((w * h) >> 1) < 2^32: %s", src);
    return H264MI_EUNSUPPORTED;
}

// the coefficient set and the chroma mode of a resolved csc (0: a format that converts nothing), as the descriptors carry them
static void csc_fields(int res, uint32_t *cset, uint32_t *bilinear) {
    *cset = res ? 2 * ((res & 15) - 1) + ((res & H264MI_CSC_FULL_RANGE) ? 1 : 0) : 0;
    *bilinear = (res & H264MI_CSC_CHROMA_BILINEAR) ? 1 : 0;
}

// ---------------------------------------------------------------- tight I420 (K6)
static int pack_frames(h264mi_decoder *d, const FrameList &frames, void *dst, size_t cap, size_t *bytes) {
    GUARD(d);
    std::vector<PackDesc> descs(frames.size());
    size_t off = 0;
    int hmax = 0;
    for (size_t i = 0; i < frames.size(); i++) {
        uint8_t *p;
        const OutFrame *of;
        int x0, y0, w, h;
        TRY(frame_ptrs(d, frames[i].first, frames[i].second, &p, &of));
        crop_rect(of, 1, &x0, &y0, &w, &h);
        set_source(descs[i], p, of, x0, y0, w, h, off);
        off += H264MI_I420_SIZE(w, h);
        hmax = std::max(hmax, h);
    }
    if (bytes) *bytes = off;
    if (off > cap) return H264MI_ECAPACITY;
    if (frames.empty()) return H264MI_OK;
    DescTables &t = d->tables[OUT_PACK];
    const PackDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    const int rows_per_block = 32;
    hipLaunchKernelGGL(k_pack, dim3(static_cast<uint32_t>(frames.size()), (hmax + 2 * ((hmax + 1) / 2) + rows_per_block - 1) / rows_per_block), dim3(256), 0, d->stream, dev,
                       static_cast<uint8_t *>(dst), rows_per_block);
    return fence_launch(d, t);
}

extern "C" int32_t h264mi_frame_pack_device(h264mi_decoder *d, int32_t stream, int32_t frame, void *dst, size_t cap) {
    if (!d || !dst) return H264MI_EINVAL;
    return pack_frames(d, {{stream, frame}}, dst, cap, nullptr);
}

extern "C" int32_t h264mi_batch_pack_device(h264mi_decoder *d, int32_t stream, void *dst, size_t cap, size_t *bytes) {
    if (!d || !dst || !batch_stream_ok(d, stream)) return H264MI_EINVAL;
    return pack_frames(d, batch_frames(d, stream), dst, cap, bytes);
}

// ---------------------------------------------------------------- output formats (K7): the rule of include/h264mi.h
extern "C" int32_t h264mi_output_size(int32_t format, int32_t w, int32_t h, size_t *bytes) {
    if (!bytes || w <= 0 || h <= 0) return H264MI_EINVAL;
    switch (format) {
    case H264MI_FMT_I420:
    case H264MI_FMT_NV12: *bytes = H264MI_I420_SIZE(w, h); return H264MI_OK;
    case H264MI_FMT_RGB24:
    case H264MI_FMT_RGBP: *bytes = static_cast<size_t>(3) * w * h; return H264MI_OK;
    }
    set_error("unknown output format %d", format);
    return H264MI_EINVAL;
}

extern "C" int32_t h264mi_csc_resolve(int32_t csc, int32_t matrix_coefficients, int32_t video_full_range, int32_t width, int32_t height, int32_t *resolved) {
    if (!resolved) return H264MI_EINVAL;
    int matrix = csc & 15;
    if (csc < 0 || (csc & ~(15 | H264MI_CSC_FULL_RANGE | H264MI_CSC_CHROMA_BILINEAR)) || matrix > H264MI_CSC_BT709) {
        set_error("csc %d: not a matrix (0 auto, 1 BT.601, 2 BT.709) with H264MI_CSC_FULL_RANGE / H264MI_CSC_CHROMA_BILINEAR", csc);
        return H264MI_EINVAL;
    }
    int full = csc & H264MI_CSC_FULL_RANGE;
    if (matrix == H264MI_CSC_AUTO) {
        if (full) {
            set_error("H264MI_CSC_FULL_RANGE needs an explicit matrix: with H264MI_CSC_AUTO the range comes from the stream");
            return H264MI_EINVAL;
        }
        switch (matrix_coefficients) {
        case 1: matrix = H264MI_CSC_BT709; break;
        case 5:
        case 6: matrix = H264MI_CSC_BT601; break;
        case 2: matrix = (width >= 1280 || height > 576) ? H264MI_CSC_BT709 : H264MI_CSC_BT601; break;
        default:
            set_error("matrix_coefficients %d of the stream is not BT.601 / BT.709 (1, 2, 5, 6): pass an explicit matrix (H264MI_CSC_BT601 / H264MI_CSC_BT709)", matrix_coefficients);
            return H264MI_EUNSUPPORTED;
        }
        full = video_full_range ? H264MI_CSC_FULL_RANGE : 0;
    }
    *resolved = matrix | full | (csc & H264MI_CSC_CHROMA_BILINEAR);
    return H264MI_OK;
}

static int convert_frames(h264mi_decoder *d, const FrameList &frames, int format, int csc, void *dst, size_t cap, size_t *bytes) {
    TRY(check_format("output", format, 1u << H264MI_FMT_NV12 | 1u << H264MI_FMT_RGB24 | 1u << H264MI_FMT_RGBP, "H264MI_FMT_NV12, _RGB24 or _RGBP"));
    if (format == H264MI_FMT_NV12 && csc != 0) {
        set_error("H264MI_FMT_NV12 converts nothing: csc must be 0, not %d", csc);
        return H264MI_EINVAL;
    }
    TRY(check_csc(csc));
    GUARD(d);
    std::vector<ConvDesc> descs(frames.size());
    size_t off = 0;
    int hmax = 0;
    for (size_t i = 0; i < frames.size(); i++) {
        uint8_t *p;
        const OutFrame *of;
        int x0, y0, w, h, res = 0;
        TRY(frame_ptrs(d, frames[i].first, frames[i].second, &p, &of));
        crop_rect(of, 1, &x0, &y0, &w, &h);
        if (format != H264MI_FMT_NV12) TRY(h264mi_csc_resolve(csc, of->matrix_coefficients, of->video_full_range, w, h, &res));
        ConvDesc &cv = descs[i];
        set_source(cv, p, of, x0, y0, w, h, off);
        cv.format = format, cv.pad = 0;
        csc_fields(res, &cv.cset, &cv.bilinear);
        size_t sz = 0;
        h264mi_output_size(format, w, h, &sz);
        off += sz;
        hmax = std::max(hmax, h);
    }
    if (bytes) *bytes = off;
    if (off > cap) return H264MI_ECAPACITY;
    if (frames.empty()) return H264MI_OK;
    DescTables &t = d->tables[OUT_CONVERT];
    const ConvDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    const int pairs_per_block = 8; // 1080p: 8 x 120 items of 2 x 16 pixels for 256 threads, 68 blocks per frame
    hipLaunchKernelGGL(k_convert, dim3(static_cast<uint32_t>(frames.size()), ((hmax + 1) / 2 + pairs_per_block - 1) / pairs_per_block), dim3(256), 0, d->stream, dev,
                       static_cast<uint8_t *>(dst), pairs_per_block);
    return fence_launch(d, t);
}

extern "C" int32_t h264mi_frame_convert_device(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t format, int32_t csc, void *dst, size_t cap) {
    if (!d || !dst) return H264MI_EINVAL;
    return convert_frames(d, {{stream, frame}}, format, csc, dst, cap, nullptr);
}

extern "C" int32_t h264mi_batch_convert_device(h264mi_decoder *d, int32_t stream, int32_t format, int32_t csc, void *dst, size_t cap, size_t *bytes) {
    if (!d || !dst || !batch_stream_ok(d, stream)) return H264MI_EINVAL;
    return convert_frames(d, batch_frames(d, stream), format, csc, dst, cap, bytes);
}

// ---------------------------------------------------------------- scaled output (K8): the rule of include/h264mi.h, "Scaled output"
// bilinear: position of output index i on an axis of n_in samples scaled to n_out -- a in the high bits, f in bits 8 .. 15
static inline void bilinear_axis(int n_in, int n_out, uint32_t *step, int32_t *half) {
    *step = (static_cast<uint32_t>(n_in) << 16) / static_cast<uint32_t>(n_out); // n_in <= 16384: fits
    *half = static_cast<int32_t>(*step >> 1) - 32768;
}
// the four axes of a frame of w x h scaled to ow x oh: luma x, luma y, chroma x, chroma y
static void bilinear_axes(int w, int h, int ow, int oh, uint32_t step[4], int32_t half[4]) {
    bilinear_axis(w, ow, &step[0], &half[0]);
    bilinear_axis(h, oh, &step[1], &half[1]);
    bilinear_axis((w + 1) / 2, (ow + 1) / 2, &step[2], &half[2]);
    bilinear_axis((h + 1) / 2, (oh + 1) / 2, &step[3], &half[3]);
}

extern "C" int32_t h264mi_scale_taps(int32_t filter, int32_t n_in, int32_t n_out, int32_t i, int32_t *first, int32_t *count, int32_t *weights, int32_t cap) {
    if (!first || !count || !weights || cap < 0) return H264MI_EINVAL;
    TRY(check_filter(filter));
    if (n_in < 1 || n_in > H264MI_SCALE_MAX || n_out < 1 || n_out > H264MI_SCALE_MAX || i < 0 || i >= n_out) {
        set_error("scale taps: n_in %d, n_out %d must be 1 .. %d and 0 <= i (%d) < n_out", n_in, n_out, H264MI_SCALE_MAX, i);
        return H264MI_EINVAL;
    }
    if (filter == H264MI_SCALE_BILINEAR) {
        uint32_t step;
        int32_t half;
        bilinear_axis(n_in, n_out, &step, &half);
        const int32_t P = std::min(std::max(static_cast<int32_t>(i * step) + half, 0), (n_in - 1) << 16);
        *first = P >> 16, *count = 2;
        if (cap < 2) return H264MI_ECAPACITY;
        const int32_t f = (P >> 8) & 255;
        weights[0] = 256 - f, weights[1] = f;
        return H264MI_OK;
    }
    if (n_out > n_in) {
        set_error("H264MI_SCALE_AREA only scales down: %d -> %d", n_in, n_out);
        return H264MI_EINVAL;
    }
    const int32_t lo = i * n_in, hi = lo + n_in; // <= 2^28
    const int32_t k0 = lo / n_out, k1 = (hi - 1) / n_out;
    *first = k0, *count = k1 - k0 + 1;
    if (cap < *count) return H264MI_ECAPACITY;
    for (int32_t k = k0; k <= k1; k++) weights[k - k0] = std::min(hi, (k + 1) * n_out) - std::max(lo, k * n_out);
    return H264MI_OK;
}

static int scale_frames(h264mi_decoder *d, const FrameList &frames, int format, int csc, int ow, int oh, int filter, void *dst, size_t cap, size_t *bytes) {
    TRY(check_format("output", format, 1u << H264MI_FMT_I420 | 1u << H264MI_FMT_NV12 | 1u << H264MI_FMT_RGB24 | 1u << H264MI_FMT_RGBP, "H264MI_FMT_I420, _NV12, _RGB24 or _RGBP"));
    const bool plain = format == H264MI_FMT_I420 || format == H264MI_FMT_NV12;
    if (plain && csc != 0) {
        set_error("H264MI_FMT_I420 and H264MI_FMT_NV12 convert nothing: csc must be 0, not %d", csc);
        return H264MI_EINVAL;
    }
    TRY(check_filter(filter));
    TRY(check_size("output", ow, oh));
    TRY(check_csc(csc));
    GUARD(d);
    std::vector<ScaleDesc> descs(frames.size());
    size_t one = 0, off = 0;
    h264mi_output_size(format, ow, oh, &one);
    for (size_t i = 0; i < frames.size(); i++) {
        uint8_t *p;
        const OutFrame *of;
        int x0, y0, w, h, res = 0;
        TRY(frame_ptrs(d, frames[i].first, frames[i].second, &p, &of));
        crop_rect(of, 1, &x0, &y0, &w, &h);
        if (filter == H264MI_SCALE_AREA) TRY(check_area(w, h, ow, oh, "output", "frame %d of stream %d is %d x %d", frames[i].second, frames[i].first, w, h));
        // from the frame's SPS and its display (source) size, never from the output size
        if (!plain) TRY(h264mi_csc_resolve(csc, of->matrix_coefficients, of->video_full_range, w, h, &res));
        ScaleDesc &sc = descs[i];
        set_source(sc, p, of, x0, y0, w, h, off);
        sc.format = format, sc.filter = filter;
        csc_fields(res, &sc.cset, &sc.bilinear);
        bilinear_axes(w, h, ow, oh, sc.step, sc.half);
        off += one;
    }
    if (bytes) *bytes = off;
    if (off > cap) return H264MI_ECAPACITY;
    if (frames.empty()) return H264MI_OK;
    DescTables &t = d->tables[OUT_SCALE];
    const ScaleDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    // about 256 items of 2 x 16 output pixels per block: 640 wide: 6 row pairs x 40 groups; 224 wide: 18 x 14
    const int ngroups = (ow + 15) / 16, npairs = (oh + 1) / 2;
    const int pairs_per_block = std::max(1, std::min(256 / ngroups, npairs));
    const dim3 grid(static_cast<uint32_t>(frames.size()), (npairs + pairs_per_block - 1) / pairs_per_block);
    if (filter == H264MI_SCALE_AREA) hipLaunchKernelGGL(k_scale_area, grid, dim3(256), 0, d->stream, dev, static_cast<uint8_t *>(dst), ow, oh, pairs_per_block);
    else hipLaunchKernelGGL(k_scale, grid, dim3(256), 0, d->stream, dev, static_cast<uint8_t *>(dst), ow, oh, pairs_per_block);
    return fence_launch(d, t);
}

extern "C" int32_t h264mi_frame_scale_device(h264mi_decoder *d, int32_t stream, int32_t frame, int32_t format, int32_t csc, int32_t out_w, int32_t out_h, int32_t filter,
                                             void *dst, size_t cap) {
    if (!d || !dst) return H264MI_EINVAL;
    return scale_frames(d, {{stream, frame}}, format, csc, out_w, out_h, filter, dst, cap, nullptr);
}

extern "C" int32_t h264mi_batch_scale_device(h264mi_decoder *d, int32_t stream, int32_t format, int32_t csc, int32_t out_w, int32_t out_h, int32_t filter, void *dst,
                                             size_t cap, size_t *bytes) {
    if (!d || !dst || !batch_stream_ok(d, stream)) return H264MI_EINVAL;
    return scale_frames(d, batch_frames(d, stream), format, csc, out_w, out_h, filter, dst, cap, bytes);
}

// ---------------------------------------------------------------- model input (K9): the rule of include/h264mi.h, "Model input"
extern "C" int32_t h264mi_fit_rect(int32_t fit, int32_t w, int32_t h, int32_t out_w, int32_t out_h, int32_t *px, int32_t *py, int32_t *sw, int32_t *sh) {
    if (!px || !py || !sw || !sh) return H264MI_EINVAL;
    TRY(check_fit(fit));
    if (w < 1 || w > H264MI_SCALE_MAX || h < 1 || h > H264MI_SCALE_MAX || out_w < 1 || out_w > H264MI_SCALE_MAX || out_h < 1 || out_h > H264MI_SCALE_MAX) {
        set_error("fit rect: source %d x %d and canvas %d x %d must all be 1 .. %d", w, h, out_w, out_h, H264MI_SCALE_MAX);
        return H264MI_EINVAL;
    }
    if (fit == H264MI_FIT_STRETCH) {
        *px = 0, *py = 0, *sw = out_w, *sh = out_h;
        return H264MI_OK;
    }
    if (w * out_h >= h * out_w) { // the width fills the canvas; products <= 2^28, the rounded quotient's numerator <= 2 * 2^28 + 2^14
        *sw = out_w, *sh = std::min(std::max((2 * h * out_w + w) / (2 * w), 1), out_h);
    } else {
        *sh = out_h, *sw = std::min(std::max((2 * w * out_h + h) / (2 * h), 1), out_w);
    }
    *px = (out_w - *sw) >> 1, *py = (out_h - *sh) >> 1;
    return H264MI_OK;
}

static inline int tensor_elem_size(int dtype) { return dtype == H264MI_DT_U8 ? 1 : dtype == H264MI_DT_F32 ? 4 : 2; }

extern "C" int32_t h264mi_tensor_size(const h264mi_tensor_spec *spec, size_t *bytes) {
    if (!spec || !bytes) return H264MI_EINVAL;
    TRY(check_format("tensor", spec->format, 1u << H264MI_FMT_RGBP | 1u << H264MI_FMT_RGB24, "H264MI_FMT_RGBP or H264MI_FMT_RGB24"));
    if (spec->dtype != H264MI_DT_U8 && spec->dtype != H264MI_DT_F16 && spec->dtype != H264MI_DT_BF16 && spec->dtype != H264MI_DT_F32) {
        set_error("tensor dtype %d: not H264MI_DT_U8, _F16, _BF16 or _F32", spec->dtype);
        return H264MI_EINVAL;
    }
    TRY(check_csc(spec->csc));
    TRY(check_size("tensor", spec->out_w, spec->out_h));
    TRY(check_filter(spec->filter));
    TRY(check_fit(spec->fit));
    if (spec->flags & ~H264MI_TENSOR_BGR) {
        set_error("tensor flags 0x%x: only H264MI_TENSOR_BGR is defined", static_cast<unsigned>(spec->flags));
        return H264MI_EINVAL;
    }
    for (int c = 0; c < 3; c++) {
        if (!std::isfinite(spec->scale[c]) || !std::isfinite(spec->bias[c])) {
            set_error("tensor scale[%d] = %g, bias[%d] = %g: both must be finite", c, static_cast<double>(spec->scale[c]), c, static_cast<double>(spec->bias[c]));
            return H264MI_EINVAL;
        }
        if (spec->dtype == H264MI_DT_U8 && (spec->scale[c] != 1.0f || spec->bias[c] != 0.0f)) {
            set_error("H264MI_DT_U8 maps nothing: scale[%d] must be 1 and bias[%d] 0, not %g and %g", c, c, static_cast<double>(spec->scale[c]), static_cast<double>(spec->bias[c]));
            return H264MI_EINVAL;
        }
    }
    *bytes = static_cast<size_t>(3) * spec->out_w * spec->out_h * tensor_elem_size(spec->dtype);
    return H264MI_OK;
}

static int tensor_items(h264mi_decoder *d, const h264mi_tensor_spec *spec, const h264mi_tensor_item *items, size_t n, void *dst, size_t cap, size_t *bytes) {
    size_t one = 0;
    TRY(h264mi_tensor_size(spec, &one));
    const int es = tensor_elem_size(spec->dtype), ow = spec->out_w, oh = spec->out_h;
    if (reinterpret_cast<uintptr_t>(dst) % es) {
        set_error("tensor destination %p: not aligned to the element size %d", dst, es);
        return H264MI_EINVAL;
    }
    GUARD(d);
    std::vector<TensorDesc> descs(n);
    size_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const h264mi_tensor_item &it = items[i];
        uint8_t *p;
        const OutFrame *of;
        int x0, y0, w, h, res = 0;
        const int r = frame_ptrs(d, it.stream, it.frame, &p, &of);
        if (r != H264MI_OK) {
            set_error("tensor item %zu: no frame %d of stream %d in the last executed batch", i, it.frame, it.stream);
            return r;
        }
        crop_rect(of, 1, &x0, &y0, &w, &h);
        int rx = it.x, ry = it.y, rw = it.w, rh = it.h;
        if (rw == 0 && rh == 0) rw = w, rh = h; // the whole frame (legal from the origin (0, 0) only)
        if (rx < 0 || ry < 0 || (rx & 1) || (ry & 1) || rw < 1 || rh < 1 || rx > w - rw || ry > h - rh) {
            set_error("tensor item %zu: region (%d, %d, %d, %d) of frame %d of stream %d (%d x %d): the origin must be even and non-negative, the size at least 1 x 1, all of it inside the frame",
                      i, it.x, it.y, it.w, it.h, it.frame, it.stream, w, h);
            return H264MI_EINVAL;
        }
        int px, py, sw, sh;
        TRY(h264mi_fit_rect(spec->fit, rw, rh, ow, oh, &px, &py, &sw, &sh));
        if (spec->filter == H264MI_SCALE_AREA) TRY(check_area(rw, rh, sw, sh, "picture", "item %zu, region %d x %d of frame %d of stream %d", i, rw, rh, it.frame, it.stream));
        // from the frame's SPS and its DISPLAY size, never from the region or the canvas
        TRY(h264mi_csc_resolve(spec->csc, of->matrix_coefficients, of->video_full_range, w, h, &res));
        TensorDesc &td = descs[i];
        set_source(td, p, of, x0 + rx, y0 + ry, rw, rh, off); // rx, ry even: (x0 + rx) / 2 = x0 / 2 + rx / 2
        td.sw = sw, td.sh = sh, td.px = px, td.py = py;
        csc_fields(res, &td.cset, &td.bilinear);
        bilinear_axes(rw, rh, sw, sh, td.step, td.half);
        off += one;
    }
    if (bytes) *bytes = off;
    if (off > cap) return H264MI_ECAPACITY;
    if (n == 0) return H264MI_OK;
    DescTables &t = d->tables[OUT_TENSOR];
    const TensorDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    TensorParams P;
    const bool bgr = (spec->flags & H264MI_TENSOR_BGR) != 0;
    P.ow = ow, P.oh = oh, P.dtype = spec->dtype, P.hwc = spec->format == H264MI_FMT_RGB24, P.bgr = bgr;
    for (int p = 0; p < 3; p++) { // by channel position
        const int c = bgr ? 2 - p : p;
        P.pad[p] = spec->pad[c], P.scale[p] = spec->scale[c], P.bias[p] = spec->bias[c];
    }
    // about 256 thread items of 2 rows x 8 columns per block; a picture that does not start on a thread item's boundary needs one more group and row pair
    const int ngroups = (ow + 7) / 8 + 1, npairs = (oh + 1) / 2 + 1;
    P.pairs_per_block = std::max(1, std::min(256 / ngroups, npairs));
    const dim3 grid(static_cast<uint32_t>(n), (npairs + P.pairs_per_block - 1) / P.pairs_per_block);
    if (spec->filter == H264MI_SCALE_AREA) hipLaunchKernelGGL(k_tensor_area, grid, dim3(256), 0, d->stream, dev, static_cast<uint8_t *>(dst), P);
    else hipLaunchKernelGGL(k_tensor, grid, dim3(256), 0, d->stream, dev, static_cast<uint8_t *>(dst), P);
    return fence_launch(d, t);
}

extern "C" int32_t h264mi_items_tensor_device(h264mi_decoder *d, const h264mi_tensor_spec *spec, const h264mi_tensor_item *items, int32_t n, void *dst, size_t cap,
                                              size_t *bytes) {
    if (!d || !spec || !dst || n < 0 || (n > 0 && !items)) return H264MI_EINVAL;
    return tensor_items(d, spec, items, static_cast<size_t>(n), dst, cap, bytes);
}

extern "C" int32_t h264mi_batch_tensor_device(h264mi_decoder *d, int32_t stream, const h264mi_tensor_spec *spec, void *dst, size_t cap, size_t *bytes) {
    if (!d || !spec || !dst || !batch_stream_ok(d, stream)) return H264MI_EINVAL;
    std::vector<h264mi_tensor_item> items;
    for (const std::pair<int, int> &f : batch_frames(d, stream)) items.push_back({f.first, f.second, 0, 0, 0, 0});
    return tensor_items(d, spec, items.data(), items.size(), dst, cap, bytes);
}

// ---------------------------------------------------------------- deinterlaced output (K10): the rule of include/h264mi.h, "Deinterlaced output"
static int check_deint(int mode, int parity) {
    if (mode != H264MI_DEINT_FIELD && mode != H264MI_DEINT_BLEND && mode != H264MI_DEINT_EDGE) {
        set_error("deinterlace mode %d: not H264MI_DEINT_FIELD, _BLEND or _EDGE", mode);
        return H264MI_EINVAL;
    }
    if ((parity != 0 && parity != 1) || (mode == H264MI_DEINT_BLEND && parity != 0)) {
        set_error("deinterlace parity %d: not 0 or 1%s", parity, mode == H264MI_DEINT_BLEND ? " (H264MI_DEINT_BLEND ignores it: it must be 0)" : "");
        return H264MI_EINVAL;
    }
    return H264MI_OK;
}

extern "C" int32_t h264mi_deint_rows(int32_t mode, int32_t parity, int32_t n_rows, int32_t y, int32_t *kept, int32_t *up, int32_t *dn) {
    if (!kept || !up || !dn) return H264MI_EINVAL;
    TRY(check_deint(mode, parity));
    if (n_rows < 1 || n_rows > H264MI_SCALE_MAX || y < 0 || y >= n_rows) {
        set_error("deinterlace rows: n_rows %d must be 1 .. %d and 0 <= y (%d) < n_rows", n_rows, H264MI_SCALE_MAX, y);
        return H264MI_EINVAL;
    }
    if (mode == H264MI_DEINT_BLEND) {
        *kept = 0, *up = std::max(y - 1, 0), *dn = std::min(y + 1, n_rows - 1);
        return H264MI_OK;
    }
    int u = y - 1, v = y + 1;
    if (u < 0) u = v;
    if (v >= n_rows) v = u;
    if ((y & 1) == parity || u < 0 || u >= n_rows) { // kept, or neither neighbour exists (one row, parity 1)
        *kept = 1, *up = *dn = y;
        return H264MI_OK;
    }
    *kept = 0, *up = u, *dn = v;
    return H264MI_OK;
}

// room for `bytes` of derived frames: the arena grows to the largest call and is kept.  On failure the arena, and so the previous list, is as it was
static int reserve_derived(h264mi_decoder *d, size_t bytes) {
    if (bytes <= d->derived_cap) return H264MI_OK;
    uint8_t *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("deinterlace: no device memory for %zu bytes of derived frames", bytes);
        return H264MI_ENOMEM;
    }
    // only display rectangles are ever written: the rest of a slot stays zero.  The old arena goes once nothing on the stream reads it any more
    if (hipMemsetAsync(p, 0, bytes, d->stream) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess) {
        hipFree(p);
        set_error("deinterlace: clearing the arena of derived frames failed");
        return H264MI_EDEVICE;
    }
    if (d->d_derived) hipFree(d->d_derived);
    d->dev_bytes += bytes - d->derived_cap;
    d->d_derived = p, d->derived_cap = bytes;
    d->derived.clear(); // (the caller replaces the list; it never outlives its arena)
    return H264MI_OK;
}

static int deint_items(h264mi_decoder *d, int mode, const h264mi_deint_item *items, size_t n, int32_t *n_derived) {
    TRY(check_deint(mode, 0));
    GUARD(d);
    std::vector<DeintDesc> descs(n);
    std::vector<DerivedFrame> next(n);
    size_t off = 0;
    int hmax = 0;
    for (size_t i = 0; i < n; i++) {
        const h264mi_deint_item &it = items[i];
        uint8_t *p;
        const OutFrame *of;
        int x0, y0, w, h;
        if (it.stream == H264MI_STREAM_DERIVED || frame_ptrs(d, it.stream, it.frame, &p, &of) != H264MI_OK) {
            set_error("deinterlace item %zu: no frame %d of stream %d in the last executed batch (a derived frame cannot be a source)", i, it.frame, it.stream);
            return H264MI_EINVAL;
        }
        const int parity = it.parity == H264MI_DEINT_PARITY_FIRST && mode != H264MI_DEINT_BLEND ? of->first_parity : it.parity;
        if (check_deint(mode, parity) != H264MI_OK) {
            set_error("deinterlace item %zu: parity %d is not 0, 1 or H264MI_DEINT_PARITY_FIRST (with H264MI_DEINT_BLEND: not 0)", i, it.parity);
            return H264MI_EINVAL;
        }
        crop_rect(of, 1, &x0, &y0, &w, &h);
        DeintDesc &dd = descs[i];
        set_source(dd, p, of, x0, y0, w, h, off);
        dd.mode = mode, dd.parity = parity;
        next[i].of = *of, next[i].off = off;
        off += (static_cast<size_t>(dd.W) * dd.H * 3 / 2 + 255) & ~static_cast<size_t>(255); // a frame slot of the source's coded size
        hmax = std::max(hmax, h);
    }
    if (n) TRY(reserve_derived(d, off));
    if (n_derived) *n_derived = static_cast<int32_t>(n);
    // from here on the arena is rewritten: the previous list is gone whatever happens (the launches that read it are ahead of this one on the stream)
    d->derived.clear();
    if (n == 0) return H264MI_OK;
    DescTables &t = d->tables[OUT_DEINT];
    const DeintDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    const int pairs_per_block = 8; // 1080p: 8 x 120 items of 2 x 16 samples for 256 threads, 102 blocks per frame
    const int hc = (hmax + 1) / 2, npairs = (hmax + 1) / 2 + (hc + 1) / 2;
    hipLaunchKernelGGL(k_deint, dim3(static_cast<uint32_t>(n), (npairs + pairs_per_block - 1) / pairs_per_block), dim3(256), 0, d->stream, dev, d->d_derived, pairs_per_block);
    TRY(fence_launch(d, t));
    d->derived.swap(next);
    return H264MI_OK;
}

extern "C" int32_t h264mi_items_deinterlace(h264mi_decoder *d, int32_t mode, const h264mi_deint_item *items, int32_t n, int32_t *n_derived) {
    if (!d || n < 0 || (n > 0 && !items)) return H264MI_EINVAL;
    return deint_items(d, mode, items, static_cast<size_t>(n), n_derived);
}

extern "C" int32_t h264mi_batch_deinterlace(h264mi_decoder *d, int32_t stream, int32_t mode, int32_t rate, int32_t *n_derived) {
    if (!d || stream < -1 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    TRY(check_deint(mode, 0));
    if ((rate != 1 && rate != 2) || (mode == H264MI_DEINT_BLEND && rate != 1)) {
        set_error("deinterlace rate %d: not 1 or 2%s", rate, mode == H264MI_DEINT_BLEND ? " (H264MI_DEINT_BLEND has no parity: it needs rate 1)" : "");
        return H264MI_EINVAL;
    }
    std::vector<h264mi_deint_item> items;
    for (const std::pair<int, int> &f : batch_frames(d, stream)) {
        uint8_t *p;
        const OutFrame *of;
        TRY(frame_ptrs(d, f.first, f.second, &p, &of));
        const int first = mode == H264MI_DEINT_BLEND ? 0 : of->first_parity;
        items.push_back({f.first, f.second, first});
        if (rate == 2) items.push_back({f.first, f.second, 1 - first});
    }
    return deint_items(d, mode, items.data(), items.size(), n_derived);
}

// ---------------------------------------------------------------- motion-adaptive deinterlacing (K10, second kernel): the rule of include/h264mi.h
extern "C" int32_t h264mi_deint_motion_pixel(const uint8_t s[3], const uint8_t p[3], int32_t sp, int32_t *out) {
    if (!s || !out) return H264MI_EINVAL;
    if (sp < 0 || sp > 255) {
        set_error("motion-adaptive pixel: the spatial value %d is not 0 .. 255", sp);
        return H264MI_EINVAL;
    }
    if (!p) {
        *out = sp;
        return H264MI_OK;
    }
    int m = 0;
    for (int i = 0; i < 3; i++) m = std::max(m, std::abs(static_cast<int>(s[i]) - static_cast<int>(p[i])));
    const int t = s[1];
    *out = std::min(std::max(sp, t - m), t + m);
    return H264MI_OK;
}

static int check_deint_motion(int mode) {
    if (mode == H264MI_DEINT_FIELD || mode == H264MI_DEINT_EDGE) return H264MI_OK;
    set_error("motion-adaptive deinterlace mode %d: not H264MI_DEINT_FIELD or _EDGE (H264MI_DEINT_BLEND has no parity)", mode);
    return H264MI_EINVAL;
}
// coded size and display rectangle
static bool same_geometry(const OutFrame *a, const OutFrame *b) {
    return a->wmb == b->wmb && a->hmb == b->hmb && a->crop_x == b->crop_x && a->crop_y == b->crop_y && a->width == b->width && a->height == b->height;
}
// The histories (HistorySet): `which` is HIST_DEINT (K10, motion-adaptive) or HIST_STATS (K12); both follow one rule, in an arena each
static const char *const HIST_NAMES[HIST_KINDS] = {"deinterlace", "frame statistics"};
static_assert(H264MI_STATS_PREV_NONE == H264MI_DEINT_PREV_NONE && H264MI_STATS_PREV_HISTORY == H264MI_DEINT_PREV_HISTORY, "output_predecessors serves both");
// may frame `of` of stream `si` of the last executed batch take the stream's history as its predecessor
static bool history_valid(const h264mi_decoder *d, int which, int si, const OutFrame *of) {
    const HistorySet &hs = d->hist[which];
    if (!hs.arena || si < 0 || si >= static_cast<int>(hs.slots.size())) return false;
    const FrameHistory &fh = hs.slots[si];
    return fh.valid && fh.batch + 1 == d->stage[d->exec].seq && same_geometry(&fh.of, of);
}
// the arena of the histories: a frame slot per stream, zero-filled on the decoder's stream (ahead of everything that reads or writes it).  On failure
// everything is as it was
static int reserve_history(h264mi_decoder *d, int which) {
    HistorySet &hs = d->hist[which];
    if (hs.arena) return H264MI_OK;
    const size_t bytes = d->st.size() * d->slot_bytes;
    uint8_t *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no device memory for %zu bytes of history (a frame slot per stream)", HIST_NAMES[which], bytes);
        return H264MI_ENOMEM;
    }
    if (hipMemsetAsync(p, 0, bytes, d->stream) != hipSuccess) {
        hipFree(p);
        set_error("%s: clearing the arena of the histories failed", HIST_NAMES[which]);
        return H264MI_EDEVICE;
    }
    hs.arena = p, d->dev_bytes += bytes;
    hs.slots.assign(d->st.size(), FrameHistory());
    return H264MI_OK;
}
// take: (stream, frame) whose source becomes the stream's history, behind the launch that may read it on the decoder's stream and inside its fence: the
// whole coded frame, so that a slot has the layout of the frame it stands for
static int take_history(h264mi_decoder *d, int which, const FrameList &take) {
    HistorySet &hs = d->hist[which];
    for (const std::pair<int, int> &f : take) {
        uint8_t *p;
        const OutFrame *of;
        TRY(frame_ptrs(d, f.first, f.second, &p, &of));
        FrameHistory &fh = hs.slots[f.first];
        fh.valid = false;
        HIP_TRY(hipMemcpyAsync(hs.arena + static_cast<size_t>(f.first) * d->slot_bytes, p, static_cast<size_t>(of->wmb) * of->hmb * 384, hipMemcpyDeviceToDevice, d->stream));
        fh.valid = true, fh.batch = d->stage[d->exec].seq, fh.of = *of;
    }
    return H264MI_OK;
}
// prev[f] of every frame f (decoding order) of stream si of the last executed batch, nf > 0 of them: the frame before it in output order, none where that
// one's geometry differs; the first one: the history, if `history` and it is valid.  *last: the last frame in output order
static int output_predecessors(h264mi_decoder *d, int which, int si, bool history, std::vector<int32_t> &prev, int *last) {
    const std::vector<OutFrame> &out = d->stage[d->exec].out[si];
    const int nf = static_cast<int>(out.size());
    std::vector<int32_t> order(nf);
    int32_t k;
    prev.assign(nf, H264MI_DEINT_PREV_NONE);
    TRY(h264mi_stream_output_order(d, si, order.data(), nf, &k));
    for (int i = 0; i < nf; i++) {
        const OutFrame *of = &out[order[i]];
        if (i) prev[order[i]] = same_geometry(of, &out[order[i - 1]]) ? order[i - 1] : H264MI_DEINT_PREV_NONE;
        else prev[order[i]] = history && history_valid(d, which, si, of) ? H264MI_DEINT_PREV_HISTORY : H264MI_DEINT_PREV_NONE;
    }
    *last = order[nf - 1];
    return H264MI_OK;
}

// take: (stream, frame) whose source becomes the stream's history, behind the launch on the decoder's stream and inside its fence
static int motion_items(h264mi_decoder *d, int mode, const h264mi_deint_motion_item *items, size_t n, int32_t *n_derived, const FrameList &take) {
    TRY(check_deint_motion(mode));
    GUARD(d);
    std::vector<DeintMotionDesc> descs(n);
    std::vector<DerivedFrame> next(n);
    size_t off = 0;
    int hmax = 0;
    for (size_t i = 0; i < n; i++) {
        const h264mi_deint_motion_item &it = items[i];
        uint8_t *p, *pp = nullptr;
        const OutFrame *of, *pof;
        int x0, y0, w, h;
        if (it.stream == H264MI_STREAM_DERIVED || frame_ptrs(d, it.stream, it.frame, &p, &of) != H264MI_OK) {
            set_error("deinterlace item %zu: no frame %d of stream %d in the last executed batch (a derived frame cannot be a source)", i, it.frame, it.stream);
            return H264MI_EINVAL;
        }
        const int parity = it.parity == H264MI_DEINT_PARITY_FIRST ? of->first_parity : it.parity;
        if (parity != 0 && parity != 1) {
            set_error("deinterlace item %zu: parity %d is not 0, 1 or H264MI_DEINT_PARITY_FIRST", i, it.parity);
            return H264MI_EINVAL;
        }
        if (it.prev_frame == H264MI_DEINT_PREV_HISTORY) {
            if (!history_valid(d, HIST_DEINT, it.stream, of)) {
                set_error("deinterlace item %zu: stream %d has no valid history for frame %d (none was taken in the batch before, or its size differs, or a reset came in between)",
                          i, it.stream, it.frame);
                return H264MI_EINVAL;
            }
            pp = d->hist[HIST_DEINT].arena + static_cast<size_t>(it.stream) * d->slot_bytes;
        } else if (it.prev_frame != H264MI_DEINT_PREV_NONE) {
            if (frame_ptrs(d, it.stream, it.prev_frame, &pp, &pof) != H264MI_OK) {
                set_error("deinterlace item %zu: prev_frame %d is not a frame of stream %d in the last executed batch, H264MI_DEINT_PREV_NONE or _PREV_HISTORY", i, it.prev_frame,
                          it.stream);
                return H264MI_EINVAL;
            }
            if (!same_geometry(of, pof)) {
                set_error("deinterlace item %zu: frames %d and %d of stream %d differ in coded size or display rectangle", i, it.frame, it.prev_frame, it.stream);
                return H264MI_EINVAL;
            }
        }
        crop_rect(of, 1, &x0, &y0, &w, &h);
        DeintMotionDesc &dd = descs[i];
        set_source(dd, p, of, x0, y0, w, h, off);
        dd.mode = mode, dd.parity = parity, dd.prev = reinterpret_cast<uint64_t>(pp);
        next[i].of = *of, next[i].off = off, next[i].prev = it.prev_frame;
        off += (static_cast<size_t>(dd.W) * dd.H * 3 / 2 + 255) & ~static_cast<size_t>(255); // a frame slot of the source's coded size
        hmax = std::max(hmax, h);
    }
    if (n) TRY(reserve_derived(d, off));
    if (n_derived) *n_derived = static_cast<int32_t>(n);
    d->derived.clear(); // (as in deint_items: from here on the arena is rewritten)
    if (n == 0) return H264MI_OK;
    DescTables &t = d->tables[OUT_DEINT_MOTION];
    const DeintMotionDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    const int pairs_per_block = 8; // as k_deint
    const int hc = (hmax + 1) / 2, npairs = (hmax + 1) / 2 + (hc + 1) / 2;
    hipLaunchKernelGGL(k_deint_motion, dim3(static_cast<uint32_t>(n), (npairs + pairs_per_block - 1) / pairs_per_block), dim3(256), 0, d->stream, dev, d->d_derived,
                       pairs_per_block);
    TRY(take_history(d, HIST_DEINT, take)); // behind the launch that may read them
    TRY(fence_launch(d, t));
    d->derived.swap(next);
    return H264MI_OK;
}

extern "C" int32_t h264mi_items_deinterlace_motion(h264mi_decoder *d, int32_t mode, const h264mi_deint_motion_item *items, int32_t n, int32_t *n_derived) {
    if (!d || n < 0 || (n > 0 && !items)) return H264MI_EINVAL;
    return motion_items(d, mode, items, static_cast<size_t>(n), n_derived, {});
}

extern "C" int32_t h264mi_batch_deinterlace_motion(h264mi_decoder *d, int32_t stream, int32_t mode, int32_t rate, int32_t flags, int32_t *n_derived) {
    if (!d || stream < -1 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    TRY(check_deint_motion(mode));
    if (rate != 1 && rate != 2) {
        set_error("deinterlace rate %d: not 1 or 2", rate);
        return H264MI_EINVAL;
    }
    if (flags & ~H264MI_DEINT_HISTORY) {
        set_error("deinterlace flags 0x%x: only H264MI_DEINT_HISTORY is defined", static_cast<unsigned>(flags));
        return H264MI_EINVAL;
    }
    const bool history = (flags & H264MI_DEINT_HISTORY) != 0;
    if (history) {
        GUARD(d);
        TRY(reserve_history(d, HIST_DEINT));
    }
    std::vector<h264mi_deint_motion_item> items;
    FrameList take;
    const Stage &g = d->stage[d->exec];
    for (int si = 0; si < static_cast<int>(g.out.size()); si++) {
        const int nf = static_cast<int>(g.out[si].size());
        if ((stream >= 0 && stream != si) || nf == 0) continue;
        std::vector<int32_t> prev;
        int last;
        TRY(output_predecessors(d, HIST_DEINT, si, history, prev, &last));
        for (int f = 0; f < nf; f++) {
            const int first = g.out[si][f].first_parity;
            items.push_back({si, f, first, prev[f]});
            if (rate == 2) items.push_back({si, f, 1 - first, prev[f]});
        }
        if (history) take.push_back({si, last});
    }
    return motion_items(d, mode, items.data(), items.size(), n_derived, take);
}

extern "C" int32_t h264mi_derived_prev(h264mi_decoder *d, int32_t k, int32_t *prev) {
    if (!d || !prev || k < 0 || k >= static_cast<int>(d->derived.size())) return H264MI_EINVAL;
    *prev = d->derived[k].prev;
    return H264MI_OK;
}

// ---------------------------------------------------------------- macroblock side information (K11): the rule of include/h264mi.h
static_assert(H264MI_MB_NONE == MBT_NONE && H264MI_MB_I4x4 == MBT_I4x4 && H264MI_MB_I8x8 == MBT_I8x8 && H264MI_MB_I16x16 == MBT_I16x16 && H264MI_MB_IPCM == MBT_IPCM &&
                  H264MI_MB_P16x16 == MBT_P16x16 && H264MI_MB_P16x8 == MBT_P16x8 && H264MI_MB_P8x16 == MBT_P8x16 && H264MI_MB_P8x8 == MBT_P8x8 &&
                  H264MI_MB_PSKIP == MBT_PSKIP && H264MI_MB_B == MBT_B && H264MI_MB_BDIRECT == MBT_BDIRECT && H264MI_MB_BSKIP == MBT_BSKIP,
              "the public macroblock classes are the TYPE plane's values: MBT_* of mi_types.h as the records carry them");
static inline int popcount12(int planes) { return __builtin_popcount(static_cast<unsigned>(planes)); }

extern "C" int32_t h264mi_side_size(int32_t planes, int32_t w, int32_t h, int32_t *gw, int32_t *gh, size_t *bytes) {
    if (planes <= 0 || (planes & ~H264MI_SIDE_ALL)) {
        set_error("side planes 0x%x: not a non-empty set of H264MI_SIDE_* bits", static_cast<unsigned>(planes));
        return H264MI_EINVAL;
    }
    TRY(check_size("side information frame", w, h));
    const int cw = (w + 3) / 4, ch = (h + 3) / 4;
    if (gw) *gw = cw;
    if (gh) *gh = ch;
    if (bytes) *bytes = static_cast<size_t>(2) * cw * ch * popcount12(planes);
    return H264MI_OK;
}

static int side_items(h264mi_decoder *d, int planes, const h264mi_side_item *items, size_t n, void *dst, size_t cap, size_t *bytes) {
    size_t probe;
    TRY(h264mi_side_size(planes, 4, 4, nullptr, nullptr, &probe)); // is `planes` legal at all (whatever the frames are, and if there are none)
    if (reinterpret_cast<uintptr_t>(dst) % 2) {
        set_error("side information destination %p: not aligned to 2 bytes", dst);
        return H264MI_EINVAL;
    }
    GUARD(d);
    const Stage &g = d->stage[d->exec];
    const int set = last_record_set(d);
    std::vector<SideDesc> descs(n);
    size_t off = 0;
    int nmx_max = 1, nmy_max = 1;
    for (size_t i = 0; i < n; i++) {
        const h264mi_side_item &it = items[i];
        uint8_t *p;
        const OutFrame *of;
        if (it.stream == H264MI_STREAM_DERIVED || frame_ptrs(d, it.stream, it.frame, &p, &of) != H264MI_OK) {
            set_error("side information item %zu: no frame %d of stream %d in the last executed batch (a derived frame has no macroblocks)", i, it.frame, it.stream);
            return H264MI_EINVAL;
        }
        if (of->field_coded || of->pic < 0 || of->pic >= g.n_pics) {
            set_error("side information item %zu: frame %d of stream %d was coded as two field pictures: a grid for field pictures is not implemented", i, it.frame, it.stream);
            return H264MI_EUNSUPPORTED;
        }
        const PicDesc &pd = g.h_pics[of->pic];
        int x0, y0, w, h, gw, gh;
        size_t one;
        crop_rect(of, 1, &x0, &y0, &w, &h);
        TRY(h264mi_side_size(planes, w, h, &gw, &gh, &one));
        SideDesc &sd = descs[i];
        sd.rec = reinterpret_cast<uint64_t>(d->d_mbrec[set] + pd.mb_base);
        sd.mv1 = pd.has_b && d->d_mv1[set] ? reinterpret_cast<uint64_t>(d->d_mv1[set] + pd.mb_base) : 0;
        sd.dpoc = reinterpret_cast<uint64_t>(g.d_dpoc), sd.n_slices = static_cast<uint32_t>(g.slices.size());
        sd.dst_off = off;
        sd.wmb = pd.wmb, sd.hmb = pd.hmb, sd.bx0 = static_cast<uint32_t>(x0 >> 2), sd.by0 = static_cast<uint32_t>(y0 >> 2);
        sd.gw = static_cast<uint32_t>(gw), sd.gh = static_cast<uint32_t>(gh);
        // (the display rectangle lies inside the coded picture, so every cell does: bx0 + gw <= 4 wmb, by0 + gh <= 4 hmb)
        sd.vec = sd.bx0 % 4 == 0 && gw % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) + off) % 8 == 0;
        nmx_max = std::max(nmx_max, static_cast<int>(((sd.bx0 + gw - 1) >> 2) - (sd.bx0 >> 2)) + 1);
        nmy_max = std::max(nmy_max, static_cast<int>(((sd.by0 + gh - 1) >> 2) - (sd.by0 >> 2)) + 1);
        off += one;
    }
    if (bytes) *bytes = off;
    if (off > cap) return H264MI_ECAPACITY;
    if (n == 0) return H264MI_OK;
    DescTables &t = d->tables[OUT_SIDE];
    const SideDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    // one lane per macroblock: about 256 macroblocks per block, whole macroblock rows (1080p: 2 rows of 120)
    const int rows_per_block = std::max(1, std::min(256 / nmx_max, nmy_max));
    hipLaunchKernelGGL(k_side, dim3(static_cast<uint32_t>(n), (nmy_max + rows_per_block - 1) / rows_per_block), dim3(256), 0, d->stream, dev, static_cast<uint8_t *>(dst),
                       static_cast<uint32_t>(planes), rows_per_block);
    TRY(fence_launch(d, t, &h264mi_decoder::last_side));
    d->stage[d->exec].ev_side = d->last_side; // (the batch's table of picture order count differences: its next upload waits for this launch)
    return H264MI_OK;
}

extern "C" int32_t h264mi_items_side_device(h264mi_decoder *d, int32_t planes, const h264mi_side_item *items, int32_t n, void *dst, size_t cap, size_t *bytes) {
    if (!d || !dst || n < 0 || (n > 0 && !items)) return H264MI_EINVAL;
    return side_items(d, planes, items, static_cast<size_t>(n), dst, cap, bytes);
}

extern "C" int32_t h264mi_batch_side_device(h264mi_decoder *d, int32_t stream, int32_t planes, void *dst, size_t cap, size_t *bytes) {
    if (!d || !dst || stream < -1 || stream >= static_cast<int>(d->st.size())) { // (H264MI_STREAM_DERIVED too: a derived frame has no macroblocks)
        if (stream == H264MI_STREAM_DERIVED) set_error("side information: the derived frames have no macroblocks");
        return H264MI_EINVAL;
    }
    std::vector<h264mi_side_item> items;
    for (const std::pair<int, int> &f : batch_frames(d, stream)) items.push_back({f.first, f.second});
    return side_items(d, planes, items.data(), items.size(), dst, cap, bytes);
}

// ---------------------------------------------------------------- frame statistics (K12): the rule of include/h264mi.h, "Frame statistics"
static_assert(sizeof(h264mi_frame_stats) == 1120 && offsetof(h264mi_frame_stats, min_y) == 64 && offsetof(h264mi_frame_stats, hist_y) == 96,
              "the record of include/h264mi.h: 8 x uint64_t, 8 x uint32_t, 256 x uint32_t, no padding");
static_assert(MI_STATS_MAX_AXIS == H264MI_SCALE_MAX, "the overflow bounds of mi_kernels.h are stated for the largest frame h264mi_stats_size accepts");

extern "C" int32_t h264mi_stats_size(const h264mi_stats_spec *spec, int32_t w, int32_t h, int32_t *gw, int32_t *gh, size_t *bytes) {
    if (!spec) return H264MI_EINVAL;
    const int cell = spec->cell, planes = spec->planes;
    const bool grid = cell == 8 || cell == 16 || cell == 32 || cell == 64;
    if ((!grid && cell != 0) || (planes & ~(H264MI_STATS_CELL_SUM | H264MI_STATS_CELL_SAD)) || (cell == 0) != (planes == 0)) {
        set_error("statistics grid: cell %d with planes 0x%x: cell must be 8, 16, 32 or 64 with a non-empty set of H264MI_STATS_CELL_* bits, or 0 with planes 0", cell,
                  static_cast<unsigned>(planes));
        return H264MI_EINVAL;
    }
    if (spec->thresh < 0 || spec->thresh > 255 || spec->flags != 0) {
        set_error("statistics spec: thresh %d must be 0 .. 255 and flags 0x%x must be 0", spec->thresh, static_cast<unsigned>(spec->flags));
        return H264MI_EINVAL;
    }
    TRY(check_size("statistics frame", w, h));
    const int cw = grid ? (w + cell - 1) / cell : 0, ch = grid ? (h + cell - 1) / cell : 0;
    if (gw) *gw = cw;
    if (gh) *gh = ch;
    if (bytes) *bytes = sizeof(h264mi_frame_stats) + ((static_cast<size_t>(4) * cw * ch * popcount12(planes) + 15) & ~static_cast<size_t>(15));
    return H264MI_OK;
}

// take: as motion_items', for the statistics history; its arena is reserved here, once the call can no longer be refused
static int stats_items(h264mi_decoder *d, const h264mi_stats_spec *spec, const h264mi_stats_item *items, size_t n, void *dst, size_t cap, size_t *bytes,
                       const FrameList &take) {
    TRY(h264mi_stats_size(spec, 1, 1, nullptr, nullptr, nullptr)); // is the spec legal at all (whatever the frames are, and if there are none)
    if (reinterpret_cast<uintptr_t>(dst) % 16) {
        set_error("statistics destination %p: not aligned to 16 bytes", dst);
        return H264MI_EINVAL;
    }
    GUARD(d);
    std::vector<StatsDesc> descs(n);
    size_t off = 0;
    int hmax = 0;
    for (size_t i = 0; i < n; i++) {
        const h264mi_stats_item &it = items[i];
        uint8_t *p, *pp = nullptr;
        const OutFrame *of, *pof;
        if (frame_ptrs(d, it.stream, it.frame, &p, &of) != H264MI_OK) {
            set_error("statistics item %zu: no frame %d of stream %d in the last executed batch", i, it.frame, it.stream);
            return H264MI_EINVAL;
        }
        if (it.prev_frame == H264MI_STATS_PREV_HISTORY) {
            if (it.stream == H264MI_STREAM_DERIVED || !history_valid(d, HIST_STATS, it.stream, of)) {
                set_error("statistics item %zu: stream %d has no valid history for frame %d (none was taken in the batch before, or its size differs, or a reset came in between; "
                          "a derived frame has none)", i, it.stream, it.frame);
                return H264MI_EINVAL;
            }
            pp = d->hist[HIST_STATS].arena + static_cast<size_t>(it.stream) * d->slot_bytes;
        } else if (it.prev_frame != H264MI_STATS_PREV_NONE) {
            if (frame_ptrs(d, it.stream, it.prev_frame, &pp, &pof) != H264MI_OK) {
                set_error("statistics item %zu: prev_frame %d is not a frame of stream %d in the last executed batch, H264MI_STATS_PREV_NONE or _PREV_HISTORY", i, it.prev_frame,
                          it.stream);
                return H264MI_EINVAL;
            }
            if (!same_geometry(of, pof)) {
                set_error("statistics item %zu: frames %d and %d of stream %d differ in coded size or display rectangle", i, it.frame, it.prev_frame, it.stream);
                return H264MI_EINVAL;
            }
        }
        int x0, y0, w, h, gw, gh;
        size_t one;
        crop_rect(of, 1, &x0, &y0, &w, &h);
        TRY(h264mi_stats_size(spec, w, h, &gw, &gh, &one));
        StatsDesc &sd = descs[i];
        set_source(sd, p, of, x0, y0, w, h, off);
        sd.prev = reinterpret_cast<uint64_t>(pp), sd.gw = static_cast<uint32_t>(gw), sd.gh = static_cast<uint32_t>(gh);
        sd.inv_min = 0, sd.ticket = 0;
        off += one;
        hmax = std::max(hmax, h);
    }
    if (bytes) *bytes = off;
    if (off > cap) return H264MI_ECAPACITY;
    if (n == 0) return H264MI_OK;
    if (!take.empty()) TRY(reserve_history(d, HIST_STATS)); // only now: a call that is refused or too small for its destination (a size query) allocates nothing
    DescTables &t = d->tables[OUT_STATS];
    const StatsDesc *dev;
    TRY(stage_descs(d, t, descs, &dev));
    // the blocks ADD to what is there: records and planes start from zero.  (The overflow bounds of the partial sums: the static_asserts of mi_kernels.h)
    HIP_TRY(hipMemsetAsync(dst, 0, off, d->stream));
    int cell_log2 = 0;
    while (spec->cell >> (cell_log2 + 1)) cell_log2++;
    hipLaunchKernelGGL(k_stats, dim3(static_cast<uint32_t>(n), static_cast<uint32_t>(mi_stats_blocks(hmax))), dim3(256), 0, d->stream, const_cast<StatsDesc *>(dev),
                       static_cast<uint8_t *>(dst), static_cast<uint32_t>(cell_log2), static_cast<uint32_t>(spec->planes), static_cast<uint32_t>(spec->thresh));
    TRY(take_history(d, HIST_STATS, take)); // behind the launch that may read them
    return fence_launch(d, t);
}

extern "C" int32_t h264mi_items_stats_device(h264mi_decoder *d, const h264mi_stats_spec *spec, const h264mi_stats_item *items, int32_t n, void *dst, size_t cap,
                                             size_t *bytes) {
    if (!d || !spec || !dst || n < 0 || (n > 0 && !items)) return H264MI_EINVAL;
    return stats_items(d, spec, items, static_cast<size_t>(n), dst, cap, bytes, {});
}

// the items of the batch call and, with `take`, the frames whose sources become the histories
static int stats_plan(h264mi_decoder *d, int stream, int flags, std::vector<h264mi_stats_item> &items, FrameList *take) {
    if (stream < -1 || stream >= static_cast<int>(d->st.size())) {
        if (stream == H264MI_STREAM_DERIVED) set_error("statistics plan: the derived frames have no output order; name them through h264mi_items_stats_device");
        return H264MI_EINVAL;
    }
    if (flags & ~H264MI_STATS_HISTORY) {
        set_error("statistics flags 0x%x: only H264MI_STATS_HISTORY is defined", static_cast<unsigned>(flags));
        return H264MI_EINVAL;
    }
    const bool history = (flags & H264MI_STATS_HISTORY) != 0;
    const Stage &g = d->stage[d->exec];
    for (int si = 0; si < static_cast<int>(g.out.size()); si++) {
        const int nf = static_cast<int>(g.out[si].size());
        if ((stream >= 0 && stream != si) || nf == 0) continue;
        std::vector<int32_t> prev;
        int last;
        TRY(output_predecessors(d, HIST_STATS, si, history, prev, &last));
        for (int f = 0; f < nf; f++) items.push_back({si, f, prev[f]});
        if (history && take) take->push_back({si, last});
    }
    return H264MI_OK;
}

extern "C" int32_t h264mi_batch_stats_plan(h264mi_decoder *d, int32_t stream, int32_t flags, h264mi_stats_item *items, int32_t cap, int32_t *n) {
    if (!d || !n || cap < 0 || (cap > 0 && !items)) return H264MI_EINVAL;
    std::vector<h264mi_stats_item> plan;
    TRY(stats_plan(d, stream, flags, plan, nullptr));
    *n = static_cast<int32_t>(plan.size());
    if (plan.size() > static_cast<size_t>(cap)) return H264MI_ECAPACITY;
    std::copy(plan.begin(), plan.end(), items);
    return H264MI_OK;
}

extern "C" int32_t h264mi_batch_stats_device(h264mi_decoder *d, int32_t stream, const h264mi_stats_spec *spec, int32_t flags, void *dst, size_t cap, size_t *bytes) {
    if (!d || !spec || !dst) return H264MI_EINVAL;
    TRY(h264mi_stats_size(spec, 1, 1, nullptr, nullptr, nullptr));
    std::vector<h264mi_stats_item> plan;
    FrameList take;
    TRY(stats_plan(d, stream, flags, plan, &take));
    return stats_items(d, spec, plan.data(), plan.size(), dst, cap, bytes, take);
}

// ---------------------------------------------------------------- JPEG snapshots (K13): the rule of include/h264mi.h, "JPEG snapshots"
static_assert(sizeof(h264mi_jpeg_result) == 16 && sizeof(JpegDesc) % 8 == 0 && sizeof(JpegParams) % 8 == 0, "the destination's records; descriptors follow the parameters aligned");

extern "C" int32_t h264mi_jpeg_quant_table(int32_t quality, int32_t chroma, uint16_t q[64]) {
    if (!q || quality < 1 || quality > 100 || (chroma != 0 && chroma != 1)) return H264MI_EINVAL;
    for (int i = 0; i < 64; i++) q[i] = static_cast<uint16_t>(jpeg_q(quality, chroma, i));
    return H264MI_OK;
}

extern "C" int32_t h264mi_jpeg_block(const uint8_t s[64], const uint16_t q[64], int16_t level[64]) {
    if (!s || !q || !level) return H264MI_EINVAL;
    for (int i = 0; i < 64; i++)
        if (q[i] < 1 || q[i] > 255) return H264MI_EINVAL;
    int16_t x[64], rt[64]; // rt: the row pass, transposed
    for (int i = 0; i < 64; i++) x[i] = static_cast<int16_t>(s[i] - 128);
    for (int y = 0; y < 8; y++)
        for (int k = 0; k < 8; k++) rt[8 * k + y] = static_cast<int16_t>(jpeg_row_term(x + 8 * y, k));
    for (int v = 0; v < 8; v++)
        for (int k = 0; k < 8; k++) level[8 * v + k] = static_cast<int16_t>(jpeg_level(jpeg_col_term(rt + 8 * k, v), q[8 * v + k]));
    return H264MI_OK;
}

static int check_jpeg_spec(const h264mi_jpeg_spec *spec, bool auto_ok) {
    if (spec->quality < 1 || spec->quality > 100) {
        set_error("JPEG quality %d: not 1 .. 100", spec->quality);
        return H264MI_EINVAL;
    }
    if (spec->range != H264MI_JPEG_RANGE_KEEP && spec->range != H264MI_JPEG_RANGE_FULL && !(auto_ok && spec->range == H264MI_JPEG_RANGE_AUTO)) {
        set_error("JPEG range %d: not H264MI_JPEG_RANGE_KEEP or _FULL%s", spec->range, auto_ok ? " or _AUTO" : " (_AUTO needs a stream: there is none behind caller-held frames)");
        return H264MI_EINVAL;
    }
    if (spec->restart_mcus < 0 || spec->restart_mcus > 65535 || spec->flags != 0) {
        set_error("JPEG spec: restart_mcus %d must be 0 .. 65535 and flags 0x%x must be 0", spec->restart_mcus, static_cast<unsigned>(spec->flags));
        return H264MI_EINVAL;
    }
    return H264MI_OK;
}

// the segments of a header in file order; `sof`, `dri`: where the size and the restart interval go
static size_t jpeg_header(int quality, bool mono, uint8_t *o, uint32_t *sof, uint32_t *dri) {
    size_t n = 0;
    auto put = [&](std::initializer_list<int> b) { for (int v : b) o[n++] = static_cast<uint8_t>(v); };
    put({0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < (mono ? 1 : 2); t++) {
        put({0xff, 0xdb, 0, 67, t});
        for (int z = 0; z < 64; z++) o[n++] = static_cast<uint8_t>(jpeg_q(quality, t, jpeg_zigzag(z)));
    }
    const int nc = mono ? 1 : 3;
    put({0xff, 0xc0, 0, 8 + 3 * nc, 8});
    *sof = static_cast<uint32_t>(n);
    put({0, 0, 0, 0, nc});
    for (int c = 0; c < nc; c++) put({c + 1, c == 0 && !mono ? 0x22 : 0x11, c ? 1 : 0});
    for (int t = 0; t < (mono ? 1 : 2); t++)
        for (int ac = 0; ac < 2; ac++) {
            int nv;
            const uint8_t *bits = jpeg_huff_bits(ac, t), *vals = jpeg_huff_vals(ac, t, &nv);
            put({0xff, 0xc4, 0, 19 + nv, ac << 4 | t});
            memcpy(o + n, bits, 16), n += 16;
            memcpy(o + n, vals, nv), n += nv;
        }
    put({0xff, 0xdd, 0, 4});
    *dri = static_cast<uint32_t>(n);
    put({0, 0, 0xff, 0xda, 0, 6 + 2 * nc, nc});
    for (int c = 0; c < nc; c++) put({c + 1, c ? 0x11 : 0x00});
    put({0, 63, 0});
    return n;
}
static const size_t JPEG_HEADER_BYTES[2] = {629, 334}; // 4:2:0, mono (jpeg_core checks them against jpeg_header)

// MCUs per row, MCUs, MCUs per interval, intervals of a w x h item
static void jpeg_geometry(const h264mi_jpeg_spec *spec, int w, int h, bool mono, uint32_t *mcus_w, uint32_t *n_mcus, uint32_t *restart, uint32_t *n_int) {
    const int mcu = mono ? 8 : 16;
    *mcus_w = static_cast<uint32_t>((w + mcu - 1) / mcu);
    *n_mcus = *mcus_w * static_cast<uint32_t>((h + mcu - 1) / mcu);
    *restart = spec->restart_mcus ? static_cast<uint32_t>(spec->restart_mcus) : *mcus_w;
    *n_int = (*n_mcus + *restart - 1) / *restart;
}

extern "C" int32_t h264mi_jpeg_size(const h264mi_jpeg_spec *spec, int32_t w, int32_t h, int32_t mono, size_t *header_bytes, size_t *bound_bytes) {
    if (!spec) return H264MI_EINVAL;
    TRY(check_jpeg_spec(spec, true));
    TRY(check_size("JPEG frame", w, h));
    uint32_t mcus_w, n_mcus, restart, n_int;
    jpeg_geometry(spec, w, h, mono != 0, &mcus_w, &n_mcus, &restart, &n_int);
    const size_t hdr = JPEG_HEADER_BYTES[mono ? 1 : 0];
    if (header_bytes) *header_bytes = hdr;
    // (the largest: 1024 x 1024 MCUs of 6 blocks, 2 596 274 176 bytes with an interval per MCU)
    if (bound_bytes) *bound_bytes = (hdr + static_cast<size_t>(2 * ((MI_JPEG_BLOCK_BITS + 7) / 8)) * n_mcus * (mono ? 1 : 6) + static_cast<size_t>(2) * n_int + 15) & ~static_cast<size_t>(15);
    return H264MI_OK;
}

// the interval table holds `entries`; on failure everything is as it was
static int reserve_jpeg_intervals(h264mi_decoder *d, size_t entries) {
    if (entries <= d->jpeg_ivl_cap) return H264MI_OK;
    uint32_t *p = nullptr;
    if (hipMalloc(&p, 4 * entries) != hipSuccess) {
        (void)hipGetLastError();
        set_error("JPEG: no device memory for the interval table (%zu bytes)", 4 * entries);
        return H264MI_ENOMEM;
    }
    if (d->d_jpeg_ivl) hipFree(d->d_jpeg_ivl); // (waits for the launches that use it)
    d->dev_bytes += 4 * entries - 4 * d->jpeg_ivl_cap;
    d->d_jpeg_ivl = p, d->jpeg_ivl_cap = entries;
    return H264MI_OK;
}

// descs: source, size, mono and full of every item; the rest is filled in here
static int jpeg_core(h264mi_decoder *d, const h264mi_jpeg_spec *spec, std::vector<JpegDesc> &descs, size_t slot_bytes, void *dst, size_t cap, size_t *bytes) {
    const size_t n = descs.size();
    const size_t res_bytes = (16 * n + 255) & ~static_cast<size_t>(255);
    uint64_t total_int = 0;
    for (size_t i = 0; i < n; i++) {
        JpegDesc &jd = descs[i];
        if (slot_bytes < JPEG_HEADER_BYTES[jd.mono]) {
            set_error("JPEG item %zu: slot_bytes %zu is below the header's %zu bytes", i, slot_bytes, JPEG_HEADER_BYTES[jd.mono]);
            return H264MI_EINVAL;
        }
        jpeg_geometry(spec, static_cast<int>(jd.w), static_cast<int>(jd.h), jd.mono != 0, &jd.mcus_w, &jd.n_mcus, &jd.restart, &jd.n_int);
        jd.slot_off = res_bytes + i * slot_bytes, jd.ivl_base = static_cast<uint32_t>(total_int), jd.pad = 0;
        total_int += jd.n_int;
    }
    if (bytes) *bytes = n ? res_bytes + n * slot_bytes : 0;
    if (n && res_bytes + n * slot_bytes > cap) return H264MI_ECAPACITY;
    if (n == 0) return H264MI_OK;
    if (total_int >= (static_cast<uint64_t>(1) << 31) || n >= (static_cast<size_t>(1) << 31)) {
        set_error("JPEG: %llu restart intervals in one call: split it", static_cast<unsigned long long>(total_int));
        return H264MI_EUNSUPPORTED;
    }
    TRY(reserve_jpeg_intervals(d, static_cast<size_t>(total_int))); // only now: a call that is refused or too small for its destination allocates nothing
    std::vector<uint8_t> table(sizeof(JpegParams) + sizeof(JpegDesc) * n);
    JpegParams P;
    memset(&P, 0, sizeof P);
    for (int t = 0; t < 2; t++) {
        for (int i = 0; i < 64; i++) P.q[t][i] = static_cast<uint16_t>(jpeg_q(spec->quality, t, i));
        jpeg_huff_codes(0, t, P.dc[t], 12);
        jpeg_huff_codes(1, t, P.ac[t], 256);
        P.hdr_len[t] = static_cast<uint32_t>(jpeg_header(spec->quality, t == 1, P.hdr[t], &P.sof_off[t], &P.dri_off[t]));
        if (P.hdr_len[t] != JPEG_HEADER_BYTES[t]) {
            set_error("JPEG: internal error: a header of %u bytes", P.hdr_len[t]);
            return H264MI_EDEVICE;
        }
    }
    P.n_items = static_cast<uint32_t>(n), P.slot_bytes = static_cast<uint32_t>(std::min<size_t>(slot_bytes, 0xfffffff0u)); // (no item is longer: h264mi_jpeg_size)
    memcpy(table.data(), &P, sizeof P);
    memcpy(table.data() + sizeof P, descs.data(), sizeof(JpegDesc) * n);
    DescTables &t = d->tables[OUT_JPEG];
    const uint8_t *dev;
    TRY(stage_descs(d, t, table, &dev));
    const uint32_t total = static_cast<uint32_t>(total_int);
    hipLaunchKernelGGL(k_jpeg_size, dim3(total), dim3(64), 0, d->stream, dev, d->d_jpeg_ivl, total);
    hipLaunchKernelGGL(k_jpeg_scan, dim3(static_cast<uint32_t>(n)), dim3(64), 0, d->stream, dev, d->d_jpeg_ivl, static_cast<uint8_t *>(dst));
    hipLaunchKernelGGL(k_jpeg_write, dim3(total), dim3(64), 0, d->stream, dev, d->d_jpeg_ivl, static_cast<uint8_t *>(dst), total);
    return fence_launch(d, t);
}

static int check_jpeg_dst(size_t slot_bytes, const void *dst) {
    if (slot_bytes % 16) {
        set_error("JPEG slot_bytes %zu: not a multiple of 16", slot_bytes);
        return H264MI_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(dst) % 16) {
        set_error("JPEG destination %p: not aligned to 16 bytes", dst);
        return H264MI_EINVAL;
    }
    return H264MI_OK;
}

static int jpeg_items(h264mi_decoder *d, const h264mi_jpeg_spec *spec, const h264mi_jpeg_item *items, size_t n, size_t slot_bytes, void *dst, size_t cap, size_t *bytes) {
    TRY(check_jpeg_spec(spec, true));
    TRY(check_jpeg_dst(slot_bytes, dst));
    GUARD(d);
    std::vector<JpegDesc> descs(n);
    for (size_t i = 0; i < n; i++) {
        uint8_t *p;
        const OutFrame *of;
        if (frame_ptrs(d, items[i].stream, items[i].frame, &p, &of) != H264MI_OK) {
            set_error("JPEG item %zu: no frame %d of stream %d in the last executed batch", i, items[i].frame, items[i].stream);
            return H264MI_EINVAL;
        }
        int x0, y0, w, h;
        crop_rect(of, 1, &x0, &y0, &w, &h);
        TRY(check_size("JPEG frame", w, h));
        const size_t W = static_cast<size_t>(of->wmb) * 16, H = static_cast<size_t>(of->hmb) * 16;
        JpegDesc &jd = descs[i];
        memset(&jd, 0, sizeof jd);
        jd.y = reinterpret_cast<uint64_t>(p + static_cast<size_t>(y0) * W + x0);
        jd.cb = reinterpret_cast<uint64_t>(p + W * H + static_cast<size_t>(y0 / 2) * (W / 2) + x0 / 2), jd.cr = jd.cb + W * H / 4;
        jd.ystride = static_cast<uint32_t>(W), jd.cstride = static_cast<uint32_t>(W / 2);
        jd.w = static_cast<uint32_t>(w), jd.h = static_cast<uint32_t>(h), jd.mono = of->mono ? 1 : 0;
        jd.full = spec->range == H264MI_JPEG_RANGE_FULL || (spec->range == H264MI_JPEG_RANGE_AUTO && of->video_full_range == 0);
    }
    return jpeg_core(d, spec, descs, slot_bytes, dst, cap, bytes);
}

extern "C" int32_t h264mi_items_jpeg_device(h264mi_decoder *d, const h264mi_jpeg_spec *spec, const h264mi_jpeg_item *items, int32_t n, size_t slot_bytes, void *dst, size_t cap,
                                            size_t *bytes) {
    if (!d || !spec || !dst || n < 0 || (n > 0 && !items)) return H264MI_EINVAL;
    return jpeg_items(d, spec, items, static_cast<size_t>(n), slot_bytes, dst, cap, bytes);
}

extern "C" int32_t h264mi_batch_jpeg_device(h264mi_decoder *d, int32_t stream, const h264mi_jpeg_spec *spec, size_t slot_bytes, void *dst, size_t cap, size_t *bytes) {
    if (!d || !spec || !dst || !batch_stream_ok(d, stream)) return H264MI_EINVAL;
    std::vector<h264mi_jpeg_item> items;
    for (const std::pair<int, int> &f : batch_frames(d, stream)) items.push_back({f.first, f.second});
    return jpeg_items(d, spec, items.data(), items.size(), slot_bytes, dst, cap, bytes);
}

extern "C" int32_t h264mi_i420_jpeg_device(h264mi_decoder *d, const h264mi_jpeg_spec *spec, const void *src, int32_t w, int32_t h, int32_t mono, int32_t n, size_t slot_bytes,
                                           void *dst, size_t cap, size_t *bytes) {
    if (!d || !spec || !dst || n < 0 || (n > 0 && !src)) return H264MI_EINVAL;
    TRY(check_jpeg_spec(spec, false));
    TRY(check_size("JPEG frame", w, h));
    TRY(check_jpeg_dst(slot_bytes, dst));
    GUARD(d);
    std::vector<JpegDesc> descs(static_cast<size_t>(n));
    const size_t cw = (static_cast<size_t>(w) + 1) / 2, ch = (static_cast<size_t>(h) + 1) / 2;
    for (size_t i = 0; i < descs.size(); i++) {
        JpegDesc &jd = descs[i];
        memset(&jd, 0, sizeof jd);
        jd.y = reinterpret_cast<uint64_t>(static_cast<const uint8_t *>(src) + i * H264MI_I420_SIZE(w, h));
        jd.cb = jd.y + static_cast<size_t>(w) * h, jd.cr = jd.cb + cw * ch;
        jd.ystride = static_cast<uint32_t>(w), jd.cstride = static_cast<uint32_t>(cw);
        jd.w = static_cast<uint32_t>(w), jd.h = static_cast<uint32_t>(h), jd.mono = mono ? 1 : 0, jd.full = spec->range == H264MI_JPEG_RANGE_FULL;
    }
    return jpeg_core(d, spec, descs, slot_bytes, dst, cap, bytes);
}
