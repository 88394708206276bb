// h264decode_amd/csrc/mi_hooks.cpp -- the one file that knows about the hooks build.  Compiled twice (csrc/Makefile): for libh264mi.so the measurement
// switches below do nothing and no h264mi_internal_* entry point exists; with -DH264MI_TEST_HOOKS, for libh264mi_hooks.so, the switches read their
// environment variables where the product calls them, and the entry points the tests and tools use are exported.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mi_decoder.hpp"
#if defined(H264MI_TEST_HOOKS) && defined(__HIP__)
#include "k_deblock_edge.h" // filter_edge: the edge function of k_deblock_x
#include "k_deblock_pk.h"   // pk_luma_edge / pk_chroma_edge: the edge functions of k_deblock
#endif

#if !defined(H264MI_TEST_HOOKS)
void hook_create_entropy(h264mi_decoder *, int *) {}
void hook_create_k5(h264mi_decoder *) {}
void hook_create_pass_group(h264mi_decoder *) {}
int hook_entropy_kernel(int chosen) { return chosen; }
int hook_dbprep_kernel(int chosen) { return chosen; }
void hook_after_sync(const h264mi_decoder *) {}
#else
// ---- measurement switches ----
void hook_create_entropy(h264mi_decoder *d, int *ent_cus) {
    if (const char *e = getenv("H264MI_ENT_LDS_PAD")) d->ent_lds_pad = static_cast<size_t>(atoi(e));
    if (const char *e = getenv("H264MI_ENT_CUS")) *ent_cus = atoi(e);
}
void hook_create_k5(h264mi_decoder *d) { // fewer wavefronts per picture in k_deblock
    if (const char *e = getenv("H264MI_K5_WAVES")) d->k5_max_waves = std::min(std::max(atoi(e), 1), MI_DEBLOCK8_MAX_WAVES);
}
void hook_create_pass_group(h264mi_decoder *d) { // 0 / 2 / 3 instead of the plan (mi_pass_group) for batches without B slices
    const char *e = getenv("H264MI_PASS_GROUP");
    const int v = e ? atoi(e) : -1;
    if (v == 0 || v == 2 || v == 3) d->pass_group_force = v;
}
int hook_entropy_kernel(int chosen) { // 1: the general kernel for CABAC launches too, as before there was a CABAC-only build; 2: k_entropy_c for Main launches, as before there was a Main build
    const char *e = getenv("H264MI_ENT_GENERIC");
    const int v = e ? atoi(e) : 0;
    if (v == 2) return chosen == MI_ENT_K_MAIN ? MI_ENT_K_CABAC : chosen;
    return v && (chosen == MI_ENT_K_CABAC || chosen == MI_ENT_K_MAIN) ? MI_ENT_K_GENERAL : chosen;
}
int hook_dbprep_kernel(int chosen) { // the general kernel everywhere, as before there was a kernel for I / P launches
    const char *e = getenv("H264MI_DBPREP_GENERIC");
    return e && atoi(e) ? MI_DBPREP_K_GENERIC : chosen;
}
void hook_after_sync(const h264mi_decoder *d) {
    const Stage &g = d->stage[d->exec];
    if (getenv("H264MI_SLICE_STATS")) { // diagnostics: per-slice entropy time (100 MHz ticks) and bin count (MI_ENT_STATS builds)
        for (int i = 0; i < g.n_slices && i < 64; i++)
            fprintf(stderr, "slice %d type %d bytes %u mbs %u us %.1f bins %u | Mclk fill %.1f syntax %.1f residual %.1f writeout %.1f\n", i, g.h_slices[i].slice_type,
                    g.h_slices[i].rbsp_size, g.h_status[8 * i + 1], g.h_status[8 * i + 2] * 0.01, g.h_status[8 * i + 3], g.h_status[8 * i + 4] * 16e-6,
                    g.h_status[8 * i + 5] * 16e-6, g.h_status[8 * i + 6] * 16e-6, g.h_status[8 * i + 7] * 16e-6);
        fprintf(stderr, "last slice type %d bytes %u mbs %u us %.1f bins %u\n", g.h_slices[g.n_slices - 1].slice_type, g.h_slices[g.n_slices - 1].rbsp_size,
                g.h_status[8 * (g.n_slices - 1) + 1], g.h_status[8 * (g.n_slices - 1) + 2] * 0.01, g.h_status[8 * (g.n_slices - 1) + 3]);
    }
    if (getenv("H264MI_SLICE_TIMELINE")) { // diagnostics (-DMI_ENT_STATS=3 builds): when the slices of each type started and ended within the pass
        uint32_t t0 = 0xFFFFFFFFu;
        for (int i = 0; i < g.n_slices; i++) t0 = std::min(t0, g.h_status[8 * i + 4]);
        for (int ty = 0; ty < 3; ty++) {
            int n = 0;
            double first_end = 1e30, last_start = 0, last_end = 0, sum = 0;
            for (int i = 0; i < g.n_slices; i++)
                if (g.h_slices[i].slice_type % 5 == ty) {
                    const double a = (g.h_status[8 * i + 4] - t0) * 0.01, b = (g.h_status[8 * i + 5] - t0) * 0.01;
                    n++, sum += b - a, first_end = std::min(first_end, b), last_start = std::max(last_start, a), last_end = std::max(last_end, b);
                }
            if (n) fprintf(stderr, "timeline: slice type %d: %d slices, mean %.1f us, first end %.1f, last start %.1f, last end %.1f us\n", ty, n, sum / n, first_end, last_start, last_end);
            if (n > 64) { // slices in 20 ms buckets of their end, split into those that started with the launch and the late ones, with their mean durations
                int cnt[2][16] = {};
                double dur[2][16] = {};
                for (int i = 0; i < g.n_slices; i++)
                    if (g.h_slices[i].slice_type % 5 == ty) {
                        const double a = (g.h_status[8 * i + 4] - t0) * 0.01, b = (g.h_status[8 * i + 5] - t0) * 0.01;
                        const int late = a > 5000.0, k = std::min(15, static_cast<int>(b / 20000.0));
                        cnt[late][k]++, dur[late][k] += b - a;
                    }
                for (int late = 0; late < 2; late++)
                    for (int k = 0; k < 16; k++)
                        if (cnt[late][k]) fprintf(stderr, "timeline:   %s, end in %3d..%3d ms: %5d slices, mean duration %.1f ms\n", late ? "late start" : "first wave", 20 * k, 20 * k + 20, cnt[late][k], dur[late][k] / cnt[late][k] * 1e-3);
            }
        }
    }
}

// ---- test and measurement hooks: the product library exports the ABI of include/h264mi.h and nothing else ----
extern "C" int32_t h264mi_internal_vlc_selftest(void) {
    std::vector<uint16_t> c(MI_VLC_N);
    int bad = -1;
    build_vlc(c.data(), &bad);
    return bad;
}
// 1 while an output launch (K6 .. K9, mi_output.cpp) is recorded that the next pass has to wait for before it rewrites frames (last_pack), else 0
extern "C" int32_t h264mi_internal_pack_pending(h264mi_decoder *d, int32_t *pending) {
    if (!d || !pending) return H264MI_EINVAL;
    *pending = d->last_pack ? 1 : 0;
    return H264MI_OK;
}

// 1 while a side-information launch (K11) is recorded that the next pass's entropy stream has to wait for (last_side), else 0
extern "C" int32_t h264mi_internal_side_pending(h264mi_decoder *d, int32_t *pending) {
    if (!d || !pending) return H264MI_EINVAL;
    *pending = d->last_side ? 1 : 0;
    return H264MI_OK;
}

// Not part of the public ABI: fills every intermediate buffer (macroblock records, coefficient blocks, row state) with
// 0xFF so that a test can prove that no kernel depends on what an earlier batch -- or the allocator -- left there.
extern "C" int32_t h264mi_internal_poison(h264mi_decoder *d) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    if (const int r = drain(d)) return r;
    for (int i = 0; i < MI_SETS; i++) {
        HIP_TRY(hipMemset(d->d_mbrec[i], 0xFF, sizeof(MbRec) * d->mb_cap));
        if (i == 0) HIP_TRY(hipMemset(d->d_coef[0], 0xFF, d->pool_blocks * 32 * MI_SETS));
        HIP_TRY(hipMemset(d->d_toprows[i], 0xFF, static_cast<size_t>(d->slices_cap) * (d->Wmax / 16) * MI_TOPROW_BYTES));
        if (d->d_mv1[i]) HIP_TRY(hipMemset(d->d_mv1[i], 0xFF, sizeof(MbMv1) * d->mb_cap));
    }
    if (d->d_colrec) HIP_TRY(hipMemset(d->d_colrec, 0xFF, sizeof(ColRec) * d->colrec_per_slot * d->n_slots * d->st.size()));
    HIP_TRY(hipDeviceSynchronize());
    return H264MI_OK;
}

// Not part of the public ABI: lets the CPU test-suite check the K5 launch plan (wavefronts, hand-off ring depth,
// dynamic LDS) without a GPU -- a wrong plan would deadlock the kernel, see mi_deblock8_plan().
extern "C" int32_t h264mi_internal_deblock_plan(int32_t wmb, int32_t hmb, int32_t *nwaves, int32_t *ring, int32_t *ring_last, int32_t *last_bufs, int64_t *lds_bytes) {
    if (!nwaves || !ring || !ring_last || !last_bufs || !lds_bytes || wmb < 1 || hmb < 1) return H264MI_EINVAL;
    int w = 1, r = 1, rl = 1, nb = 1;
    mi_deblock8_plan(wmb, hmb, &w, &r, &rl, &nb);
    *nwaves = w, *ring = r, *ring_last = rl, *last_bufs = nb, *lds_bytes = static_cast<int64_t>(mi_deblock8_lds_bytes(w, r, rl, nb));
    return H264MI_OK;
}

// Not part of the public ABI: which I/P entropy kernel a level 0 of n_cabac CABAC and n_cavlc CAVLC slices runs on (mi_entropy_kernel_choice):
// 0 k_entropy, 1 k_entropy_f, 2 k_entropy_c.  (The choice as far as the coding mode and the slice groups decide it: of the two CABAC-only builds it names k_entropy_c.)
extern "C" int32_t h264mi_internal_entropy_kernel_choice(int32_t n_cabac, int32_t n_cavlc, int32_t slice_groups) {
    const int k = mi_entropy_kernel_choice(n_cabac, n_cavlc, slice_groups != 0, 0);
    return k == MI_ENT_K_MAIN ? MI_ENT_K_CABAC : k;
}
// The whole choice: n_t8x8_mono pictures of the batch have the 8x8 transform switched on or are monochrome.  3 k_entropy_m.
extern "C" int32_t h264mi_internal_entropy_kernel_choice4(int32_t n_cabac, int32_t n_cavlc, int32_t slice_groups, int32_t n_t8x8_mono) {
    return mi_entropy_kernel_choice(n_cabac, n_cavlc, slice_groups != 0, n_t8x8_mono);
}

// Not part of the public ABI: which k_dbprep kernel runs on a level's pictures, n_has_b of them with B slices and n_save_col leaving a ColRec array
// (mi_dbprep_kernel_choice): 0 k_dbprep, 1 k_dbprep_ip.
extern "C" int32_t h264mi_internal_dbprep_kernel_choice(int32_t n_has_b, int32_t n_save_col) { return mi_dbprep_kernel_choice(n_has_b, n_save_col); }

// Not part of the public ABI: macroblock rows per wavefront of k_dbprep_ip for the launches to come (0: the rule, mi_dbprep_ip_rows) -- short test
// streams never have pictures enough for the rule to choose strips of more than one row
extern "C" int32_t h264mi_internal_set_dbprep_rows(h264mi_decoder *d, int32_t rows) {
    if (!d || rows < 0) return H264MI_EINVAL;
    d->dbprep_rows = rows;
    return H264MI_OK;
}
// Not part of the public ABI: wavefronts per picture of k_deblock for the launches to come, clamped as hook_create_k5 clamps H264MI_K5_WAVES -- short
// test pictures never have groups enough for a wavefront's second and third round over a picture, nor for the two-buffer plan of the last ring
extern "C" int32_t h264mi_internal_set_k5_waves(h264mi_decoder *d, int32_t n) {
    if (!d) return H264MI_EINVAL;
    d->k5_max_waves = std::min(std::max(static_cast<int>(n), 1), MI_DEBLOCK8_MAX_WAVES);
    return H264MI_OK;
}

// Not part of the public ABI: the pass-group plan (mi_pass_group) of a batch with n_slices0 level-0 slices on a chip that holds `capacity` entropy
// wavefronts, pics_per_launch pictures per reconstruction launch, with or without B slices: 0 ungrouped, else the passes per group
extern "C" int32_t h264mi_internal_pass_group_plan(int32_t n_slices0, int32_t capacity, int32_t pics_per_launch, int32_t has_b) {
    return mi_pass_group(n_slices0, capacity, pics_per_launch, has_b != 0);
}
// Not part of the public ABI: passes per group for the executes to come, whatever the plan says -- 0, 2 or 3; -1: the plan again.  A batch with B slices
// stays ungrouped.  (Short test streams never oversubscribe the chip.)
extern "C" int32_t h264mi_internal_set_pass_group(h264mi_decoder *d, int32_t g) {
    if (!d || !(g == -1 || g == 0 || g == 2 || g == 3)) return H264MI_EINVAL;
    d->pass_group_force = g;
    return H264MI_OK;
}
// Not part of the public ABI, reports only: the pass counter of the pass executed last, and the pass whose reconstruction (ev_rec) its entropy stage
// was gated on as a member of a group (-1: none -- an ungrouped or serialised pass, or a pass of a decoder's first group)
extern "C" int32_t h264mi_internal_pass_waits(h264mi_decoder *d, int64_t *pass, int64_t *gate_pass) {
    if (!d || !pass || !gate_pass) return H264MI_EINVAL;
    *pass = static_cast<int64_t>(d->pass) - 1, *gate_pass = d->last_pass_gate;
    return H264MI_OK;
}

// Not part of the public ABI: the edge functions of the two K5 kernel families alone on the device, on n lines of samples with their parameters
// (tests/test_deblock_edges.py compares with 8.7.2.3 / 8.7.2.4 written in numpy).  No decoder: host arrays in, one launch, host arrays out.
// samples / out: n x 8 bytes p3 p2 p1 p0 q0 q1 q2 q3 (luma) or n x 4 bytes p1 p0 q0 q1 (chroma); bs / alpha / beta / tc0: n bytes each.
// impl 0: pk_luma_edge<MBEDGE> / pk_chroma_edge<MBEDGE> (k_deblock_pk.h): lines 2k and 2k + 1 are the two halves of lane k % 64 of wavefront k / 64.
//   A luma lane has one bS, alpha, beta and tC0 (lane_on / lane_strong are per lane): a pair that differs is H264MI_EINVAL.  A chroma lane has one bS;
//   its halves are the Cb and the Cr line and carry their own alpha, beta and tC0 (+ 1, as at k_deblock's call sites).
// impl 1: filter_edge<Q, CHROMA, N> (k_deblock_edge.h), line k on lane k % 64 of wavefront k / 64, in the instantiations k_deblock_x uses: luma N = 20 with
//   Q = 4 (macroblock edge) or 8 / 12 / 16 by wavefront (inner edges), chroma N = 12 with Q = 4 or 8.
// n: a multiple of 128.  bS 0..4, 4 on macroblock edges only.
#if defined(__HIP__)
template <bool MBEDGE, bool CHROMA>
__global__ void __launch_bounds__(64) k_edge_probe_pk(const uint8_t *samples, const uint8_t *bs, const uint8_t *alpha, const uint8_t *beta, const uint8_t *tc0, uint8_t *out) {
    const uint32_t l0 = 2u * (blockIdx.x * 64u + threadIdx.x), l1 = l0 + 1u; // the lane's two lines; the grid covers n / 2 lanes exactly
    const uint32_t b = bs[l0], on = b != 0u ? ~0u : 0u, strong = b == 4u ? ~0u : 0u;
    auto pair = [](const uint8_t *a, uint32_t i, uint32_t j) { return pk2{static_cast<short>(a[i]), static_cast<short>(a[j])}; };
    if (CHROMA) {
        pk2 v[4];
        for (uint32_t i = 0; i < 4; i++) v[i] = pair(samples, l0 * 4 + i, l1 * 4 + i);
        pk_chroma_edge<MBEDGE>(v[0], v[1], v[2], v[3], pair(alpha, l0, l1), pair(beta, l0, l1), pair(tc0, l0, l1) + pk_splat(1), on, MBEDGE ? strong : 0u);
        for (uint32_t i = 0; i < 4; i++) out[l0 * 4 + i] = static_cast<uint8_t>(v[i].x), out[l1 * 4 + i] = static_cast<uint8_t>(v[i].y);
    } else {
        pk2 v[8];
        for (uint32_t i = 0; i < 8; i++) v[i] = pair(samples, l0 * 8 + i, l1 * 8 + i);
        pk_luma_edge<MBEDGE>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], pk_splat(alpha[l0]), pk_splat(beta[l0]), pk_splat(tc0[l0]), on, MBEDGE ? strong : 0u);
        for (uint32_t i = 0; i < 8; i++) out[l0 * 8 + i] = static_cast<uint8_t>(v[i].x), out[l1 * 8 + i] = static_cast<uint8_t>(v[i].y);
    }
}
template <int Q, bool CHROMA, int N>
__device__ __forceinline__ void edge_probe_line(const uint8_t *samples, uint8_t *out, uint32_t l, int bs, int alpha, int beta, int tc0) {
    constexpr int H = CHROMA ? 2 : 4; // samples on each side of the edge
    int px[N];
    for (int i = 0; i < N; i++) px[i] = 0;
    for (int i = 0; i < 2 * H; i++) px[Q - H + i] = samples[l * (2 * H) + i];
    filter_edge<Q, CHROMA>(px, bs, alpha, beta, tc0);
    for (int i = 0; i < 2 * H; i++) out[l * (2 * H) + i] = static_cast<uint8_t>(px[Q - H + i]);
}
template <bool MBEDGE, bool CHROMA>
__global__ void __launch_bounds__(64) k_edge_probe_x(const uint8_t *samples, const uint8_t *bs, const uint8_t *alpha, const uint8_t *beta, const uint8_t *tc0, uint8_t *out) {
    const uint32_t l = blockIdx.x * 64u + threadIdx.x; // the grid covers n lines exactly
    const int b = bs[l], a = alpha[l], be = beta[l], t = tc0[l];
    if (CHROMA) {
        if (MBEDGE) edge_probe_line<4, true, 12>(samples, out, l, b, a, be, t);
        else edge_probe_line<8, true, 12>(samples, out, l, b, a, be, t);
    } else if (MBEDGE)
        edge_probe_line<4, false, 20>(samples, out, l, b, a, be, t);
    else {
        const uint32_t e = blockIdx.x % 3u; // wave-uniform: filter_edge holds ballots
        if (e == 0) edge_probe_line<8, false, 20>(samples, out, l, b, a, be, t);
        else if (e == 1) edge_probe_line<12, false, 20>(samples, out, l, b, a, be, t);
        else edge_probe_line<16, false, 20>(samples, out, l, b, a, be, t);
    }
}
#endif
extern "C" int32_t h264mi_internal_deblock_edge_probe(int32_t impl, int32_t chroma, int32_t mb_edge, const uint8_t *samples, const uint8_t *bs, const uint8_t *alpha,
                                                      const uint8_t *beta, const uint8_t *tc0, uint8_t *out, int64_t n) {
    if (!samples || !bs || !alpha || !beta || !tc0 || !out || impl < 0 || impl > 1 || n < 128 || n % 128 != 0 || n > (int64_t(1) << 24)) return H264MI_EINVAL;
    for (int64_t i = 0; i < n; i++)
        if (bs[i] > 4 || (bs[i] == 4 && !mb_edge)) return H264MI_EINVAL;
    if (impl == 0)
        for (int64_t i = 0; i < n; i += 2)
            if (bs[i] != bs[i + 1] || (!chroma && (alpha[i] != alpha[i + 1] || beta[i] != beta[i + 1] || tc0[i] != tc0[i + 1]))) return H264MI_EINVAL;
#if defined(__HIP__)
    const size_t un = static_cast<size_t>(n), line = chroma ? 4 : 8;
    uint8_t *dev = nullptr; // samples | out | bs | alpha | beta | tc0
    hipError_t e = hipMalloc(&dev, un * (2 * line + 4));
    uint8_t *d_s = dev, *d_o = dev + un * line, *d_p = dev + un * 2 * line;
    if (e == hipSuccess) e = hipMemcpy(d_s, samples, un * line, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_o, 0xA5, un * line);
    const uint8_t *prm[4] = {bs, alpha, beta, tc0};
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipMemcpy(d_p + un * k, prm[k], un, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid(static_cast<uint32_t>(impl == 0 ? un / 128 : un / 64)), block(64);
#define PROBE(K, M, C) hipLaunchKernelGGL((K<M, C>), grid, block, 0, 0, d_s, d_p, d_p + un, d_p + 2 * un, d_p + 3 * un, d_o)
        if (impl == 0) {
            if (mb_edge) { if (chroma) PROBE(k_edge_probe_pk, true, true); else PROBE(k_edge_probe_pk, true, false); }
            else { if (chroma) PROBE(k_edge_probe_pk, false, true); else PROBE(k_edge_probe_pk, false, false); }
        } else {
            if (mb_edge) { if (chroma) PROBE(k_edge_probe_x, true, true); else PROBE(k_edge_probe_x, true, false); }
            else { if (chroma) PROBE(k_edge_probe_x, false, true); else PROBE(k_edge_probe_x, false, false); }
        }
#undef PROBE
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_o, un * line, hipMemcpyDeviceToHost);
    if (dev) hipFree(dev);
    if (e != hipSuccess) {
        set_error("h264mi_internal_deblock_edge_probe failed: %s", hipGetErrorString(e));
        return H264MI_EDEVICE;
    }
    return H264MI_OK;
#else
    set_error("h264mi_internal_deblock_edge_probe: this build holds no device code");
    return H264MI_ENODEVICE;
#endif
}

// ... and the rule itself
extern "C" int32_t h264mi_internal_dbprep_ip_rows(int32_t n_pics, int32_t wmb_max, int32_t hmb_max) { return mi_dbprep_ip_rows(n_pics, wmb_max, hmb_max); }

// Not part of the public ABI: the batch executed last once more through k_dbprep -- its records are still resident in its set --, over the same picture
// lists, into scratch buffers, and what the pass itself produced compared with that: the bytes of the DbPrm records of its pictures and of the intra mask
// that differ.  launches_ip / launches_generic: the k_dbprep_ip / k_dbprep launches of that pass.
extern "C" int32_t h264mi_internal_dbprep_check(h264mi_decoder *d, int32_t *launches_ip, int32_t *launches_generic, int64_t *mismatching_bytes) {
    if (!d || !launches_ip || !launches_generic || !mismatching_bytes || d->last_exec_stage < 0) return H264MI_EINVAL;
    GUARD(d);
    HIP_TRY(hipDeviceSynchronize());
    const Stage &g = d->stage[d->last_exec_stage];
    const int set = d->last_exec_set;
    *launches_ip = d->dbprep_launches[MI_DBPREP_K_IP], *launches_generic = d->dbprep_launches[MI_DBPREP_K_GENERIC];
    *mismatching_bytes = 0;
    if (!g.mb_used) return H264MI_OK;
    const size_t mask_bytes = sizeof(unsigned long long) * (g.mb_used / 64 + 2);
    DbPrm *prm = nullptr;
    unsigned long long *mask = nullptr;
    hipError_t e = hipMalloc(&prm, sizeof(DbPrm) * g.mb_used);
    if (e == hipSuccess) e = hipMalloc(&mask, mask_bytes);
    if (e == hipSuccess) e = hipMemset(prm, 0xA5, sizeof(DbPrm) * g.mb_used);
    if (e == hipSuccess) e = hipMemset(mask, 0, mask_bytes);
    for (size_t lv = 0; e == hipSuccess && lv < g.levels.size(); lv++)
        if (const uint32_t n = g.levels[lv].prep.n) {
            // (the ColRec arrays of save_col pictures are written once more, with the same bytes)
            hipLaunchKernelGGL(k_dbprep, dim3((g.mbs_max + MI_DBPREP_MBS - 1) / MI_DBPREP_MBS, (n + 7u) & ~7u), dim3(256), 0, d->stream, g.d_lists + g.levels[lv].prep.off,
                               g.d_pics, d->d_tables, d->d_mbrec[set], d->d_mv1[set], prm, 0, mask, static_cast<int>(n));
            e = hipGetLastError();
        }
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    std::vector<uint8_t> a, b;
    auto differ = [&](const void *x, const void *y, size_t n) {
        a.resize(n), b.resize(n);
        if (e == hipSuccess) e = hipMemcpy(a.data(), x, n, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(b.data(), y, n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return;
        for (size_t i = 0; i < n; i++) *mismatching_bytes += a[i] != b[i];
    };
    for (const Stage::Level &lv : g.levels)
        for (uint32_t i = 0; i < lv.prep.n; i++) {
            const PicDesc &pd = g.h_pics[g.h_lists[lv.prep.off + i]];
            differ(d->d_dbprm[set] + pd.mb_base, prm + pd.mb_base, sizeof(DbPrm) * pd.wmb * pd.hmb);
        }
    differ(d->d_imask[set], mask, mask_bytes);
    if (prm) hipFree(prm);
    if (mask) hipFree(mask);
    if (e != hipSuccess) {
        set_error("h264mi_internal_dbprep_check failed: %s", hipGetErrorString(e));
        return H264MI_EDEVICE;
    }
    return H264MI_OK;
}

// Not part of the public ABI: the phase clocks a -DMI_DB_STATS build of the banded deblocking kernels leaves (zero otherwise); reading clears them
extern "C" int32_t h264mi_internal_deblock_phase_clocks(h264mi_decoder *d, uint32_t out[12]) {
    if (!d || !out) return H264MI_EINVAL;
    GUARD(d);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d->d_xctl + 64 + 8, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(d->d_xctl + 64 + 8, 0, 12 * sizeof(uint32_t)));
    return H264MI_OK;
}

// Not part of the public ABI: start and end (100 MHz ticks) of the row groups of the first picture of the last K5 launch (-DMI_DB_STATS builds)
extern "C" int32_t h264mi_internal_deblock_group_times(h264mi_decoder *d, uint32_t out[128]) { // [0..31] start / end per group, [32 + 8 g + i] when group g began step 16 i
    if (!d || !out) return H264MI_EINVAL;
    GUARD(d);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d->d_xctl + 64 + 32, 128 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return H264MI_OK;
}

// Not part of the public ABI: the banded launch plan of K5 / K3 (mi_deblock_bands, mi_intra_bands) for the CPU model test.
extern "C" int32_t h264mi_internal_band_plan(int32_t n_pics, int32_t wmb, int32_t hmb, int32_t max_wgs, int32_t *k5_bands, int32_t *k5_waves, int32_t *k5_ring,
                                             int64_t *k5_lds, int32_t *k3_bands, int32_t *k3_waves) {
    if (!k5_bands || !k5_waves || !k5_ring || !k5_lds || !k3_bands || !k3_waves || n_pics < 1 || wmb < 1 || hmb < 1) return H264MI_EINVAL;
    int nb = 1, nw = 1, ring = 1, b3 = 1, w3 = 1, roles = 1;
    mi_deblock_bands(n_pics, wmb, hmb, max_wgs, &nb, &nw, &ring, &roles);
    int wpr = 1;
    mi_intra_bands(n_pics, hmb, max_wgs, false, &b3, &w3, &wpr);
    // (the model test works on groups: the kernel runs `roles` wavefronts on each, which follow the same protocol side by side)
    *k5_bands = nb, *k5_waves = nw / roles, *k5_ring = ring, *k5_lds = static_cast<int64_t>(mi_deblock_lds_bytes_banded(nw, ring));
    *k3_bands = b3, *k3_waves = w3;
    return H264MI_OK;
}

// Not part of the public ABI: the launch plan of K3 alone (mi_intra_bands), with p_only as execute_batch() passes it for a launch without an
// intra-only picture.  bands 1 = k_intra, more = k_intra_x with `wpr` wavefronts per row; row0 = the first macroblock row of band `band` as
// k_intra_x cuts a picture of hmb rows (band * hmb / bands).  Reports, changes nothing.
extern "C" int32_t h264mi_internal_intra_plan(int32_t n_pics, int32_t hmb, int32_t max_wgs, int32_t p_only, int32_t band, int32_t *bands, int32_t *waves, int32_t *wpr, int32_t *row0) {
    if (!bands || !waves || !wpr || !row0 || n_pics < 1 || hmb < 1 || band < 0) return H264MI_EINVAL;
    int nb = 1, nw = 1, w = 1;
    mi_intra_bands(n_pics, hmb, max_wgs, p_only != 0, &nb, &nw, &w);
    *bands = nb, *waves = nw, *wpr = w, *row0 = band < nb ? band * hmb / nb : hmb;
    return H264MI_OK;
}

// Not part of the public ABI: the epoch / ticket counters of the banded kernels set to a value shortly before their 32-bit wrap
// (tests/test_gpu_parity.py::test_gpu_banded_kernels_across_the_epoch_wrap)
extern "C" int32_t h264mi_internal_set_epoch(h264mi_decoder *d, uint32_t v) {
    if (!d) return H264MI_EINVAL;
    GUARD(d);
    if (const int r = drain(d)) return r;
    d->x_epoch = d->x_tk5 = d->x_tk3 = v;
    // the device-side ticket counters stand where the host's bases do
    HIP_TRY(hipMemcpy(d->d_xctl, &d->x_tk5, sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->d_xctl + 32, &d->x_tk3, sizeof(uint32_t), hipMemcpyHostToDevice));
    return H264MI_OK;
}

// Not part of the public ABI: what picture management (8.2) made of the batch prepared last, for one stream, as text -- its pictures, slices
// (reference lists as raw entries, parity bit included) and output frames, then the frame slots that are references or held and the stream's
// POC / frame_num history (tools/host_dpb_trace.cpp; tests/test_host_dpb_trace.py pins the text).  Reads plain data only: it calls nothing of
// picture management, so a change of that code cannot change what it prints about the same state.  `len`: bytes the whole text needs (without
// the terminating 0); H264MI_ECAPACITY if that is more than cap - 1.
extern "C" int32_t h264mi_internal_dpb_trace(h264mi_decoder *d, int32_t stream, char *buf, size_t cap, size_t *len) {
    if (!d || !buf || !len || !cap || stream < 0 || stream >= static_cast<int>(d->st.size())) return H264MI_EINVAL;
    const Stage &g = d->stage[d->prep];
    const StreamState &s = d->st[stream];
    // how this function reads the batch's host tables: per picture, per slice of the sorted table, per wave and per level (ranges of h_lists)
    struct Range { uint32_t off, n; };
    auto wave_of_pic = [&](int p) { return g.pics[p].wave; };
    auto level_of_pic = [&](int p) { return g.pics[p].level; };
    auto pic_dropped = [&](int p) { return static_cast<int>(g.pics[p].dropped); };
    auto pic_init_qp = [&](int p) { return static_cast<int>(g.pics[p].init_qp); };
    auto pic_conceal_poc = [&](int p) { return g.pics[p].conceal_poc; };
    auto level_of_slice = [&](int i) { return g.slices[i].level; };
    auto slice_refs = [&](int i) -> const Stage::SliceRefs & { return g.slices[i].refs; };
    const int n_waves = static_cast<int>(g.waves.size()), n_levels = static_cast<int>(g.levels.size());
    auto wave_all = [&](int w) { return Range{g.waves[w].all.off, g.waves[w].all.n}; };
    auto wave_p = [&](int w) { return Range{g.waves[w].p.off, g.waves[w].p.n}; };
    auto wave_b = [&](int w) { return Range{g.waves[w].b.off, g.waves[w].b.n}; };
    auto level_first = [&](int l) { return l < n_levels ? g.levels[l].first : g.n_slices; }; // (l == n_levels: the end of the table)
    auto level_prep = [&](int l) { return Range{g.levels[l].prep.off, g.levels[l].prep.n}; };
    auto level_colsave_n = [&](int l) { return g.levels[l].colsave_n; };
    auto level_prep_kernel = [&](int l) { return g.levels[l].prep_kernel; };
    size_t n = 0;
    auto put = [&](const char *fmt, auto... args) {
        const int k = snprintf(n < cap ? buf + n : nullptr, n < cap ? cap - n : 0, fmt, args...);
        if (k > 0) n += static_cast<size_t>(k);
    };
    auto put_list = [&](const char *name, const auto *v, int count) {
        put(" %s=", name);
        for (int i = 0; i < count; i++) put(i ? ",%lld" : "%lld", static_cast<long long>(v[i]));
    };
    auto put_refs = [&](const Stage::SliceRefs &sr) {
        put(" cur_poc=%d", sr.cur_poc);
        put_list("poc0", sr.poc[0], sr.n[0]);
        put_list("poc1", sr.poc[1], sr.n[1]);
    };
    auto put_range = [&](const char *name, Range r) { put_list(name, g.h_lists + r.off, static_cast<int>(r.n)); };
    for (int p = 0; p < g.n_pics; p++) {
        const PicDesc &pd = g.h_pics[p];
        if (static_cast<int>(pd.stream) != stream) continue;
        const Slot &sl = s.dpb.slots[pd.slot];
        put("pic %d slot=%u field=%d poc=%d fpoc=%d,%d frame_num=%d wave=%d level=%d conceal_ref=%d n_slices=%u dropped=%d", p, pd.slot, pd.field, sl.poc, sl.fpoc[0], sl.fpoc[1],
            sl.frame_num, wave_of_pic(p), level_of_pic(p), pd.conceal_ref, pd.n_slices, pic_dropped(p));
        put(" mb_base=%llu save_col=%d init_qp=%d conceal_poc=%d,%d\n", static_cast<unsigned long long>(pd.mb_base), pd.save_col, pic_init_qp(p), pic_conceal_poc(p).cur,
            pic_conceal_poc(p).ref);
    }
    for (int i = 0; i < g.n_slices; i++) {
        const SliceDesc &sd = g.h_slices[i];
        if (static_cast<int>(g.h_pics[sd.pic_idx].stream) != stream) continue;
        put("slice pic=%u first_mb=%u type=%d fill_from=%u end_mb=%u", sd.pic_idx, sd.first_mb, sd.slice_type, sd.fill_from, sd.end_mb);
        put_list("l0", sd.ref_slot, std::min<int>(sd.num_ref_idx_active, MI_MAX_REFS));
        if (sd.slice_type == 1) {
            const BSliceExt &bx = g.h_bext[sd.bext];
            put_list("l1", bx.ref_slot1, std::min<int>(bx.num_ref_idx_l1_active, MI_MAX_REFS));
            put_list("dist_scale", bx.dist_scale, std::min<int>(sd.num_ref_idx_active, MI_MAX_REFS));
            put(" col_short=%d", bx.col_short);
        }
        put(" level=%d", level_of_slice(i));
        put_refs(slice_refs(i));
        put("%s", "\n");
    }
    if (d->conceal) // the pseudo-slice of every picture (behind the real slices of the table) and where k_conceal finds the picture's slices
        for (int p = 0; p < g.n_pics; p++) {
            if (static_cast<int>(g.h_pics[p].stream) != stream) continue;
            put("conceal pic=%d", p);
            put_refs(slice_refs(g.n_slices + p));
            put(" cmap=%u", g.h_cmap[p]);
            put_list("slices", g.h_cmap + g.h_cmap[p], static_cast<int>(g.h_pics[p].n_slices));
            put("%s", "\n");
        }
    for (const OutFrame &o : g.out[stream])
        put("out slot=%d wmb=%d hmb=%d crop=%d,%d size=%dx%d poc=%d frame_num=%d nal_ref_idc=%d idr=%d pic=%d new_sequence=%d pic2=%d\n", o.slot, o.wmb, o.hmb, o.crop_x, o.crop_y,
            o.width, o.height, o.poc, o.frame_num, o.nal_ref_idc, o.idr, o.pic, o.new_sequence, o.pic2);
    for (size_t i = 0; i < s.dpb.slots.size(); i++) {
        const Slot &sl = s.dpb.slots[i];
        if (sl.ref || sl.held)
            put("slot %zu ref=%d long_idx=%d frame_num=%d fields=%d funref=%d nonexisting=%d field_coded=%d poc=%d held=%d\n", i, sl.ref, sl.long_idx, sl.frame_num, sl.fields,
                sl.funref, sl.nonexisting, sl.field_coded, sl.poc, sl.held);
    }
    put("state prev_ref_frame_num=%d prev_poc_msb=%d prev_poc_lsb=%d prev_frame_num=%d prev_frame_num_offset=%d pend_slot=%d need_idr=%d\n", s.dpb.prev_ref_frame_num, s.dpb.prev_poc_msb,
        s.dpb.prev_poc_lsb, s.dpb.prev_frame_num, s.dpb.prev_frame_num_offset, s.dpb.pend_slot, s.need_idr);
    // the batch as a whole (every stream's pictures): the launch lists by their contents, the levels, and what is decided once per batch
    for (int w = 0; w < n_waves; w++) {
        put("wave %d", w);
        put_range("all", wave_all(w)), put_range("p", wave_p(w)), put_range("b", wave_b(w));
        put("%s", "\n");
    }
    for (int l = 0; l < n_levels; l++) {
        put("level %d first_slice=%d n_slices=%d", l, level_first(l), level_first(l + 1) - level_first(l));
        put_range("prep", level_prep(l));
        put(" colsave_n=%u prep_kernel=%d\n", level_colsave_n(l), level_prep_kernel(l));
    }
    // (ent_kernel: the choice as far as coding mode and slice groups decide it, as the three-argument entry above -- this trace pins picture management
    // and the batch's tables against tests/golden/dpb_trace_md5.json, not which of the two CABAC-only builds runs; h264mi_internal_entropy_kernel_choice4 says that)
    put("tables ent_kernel=%d wmb_max=%d hmb_max=%d mbs_max=%d n_bext=%d", g.ent_kernel == MI_ENT_K_MAIN ? MI_ENT_K_CABAC : g.ent_kernel, g.wmb_max, g.hmb_max, g.mbs_max, g.n_bext);
    put_list("fmo_pics", g.fmo_pics.data(), static_cast<int>(g.fmo_pics.size()));
    put("%s", " grey=");
    for (size_t i = 0; i < g.grey.size(); i++) put(i ? ",%u:%u:%u:%ux%u" : "%u:%u:%u:%ux%u", g.grey[i].stream, g.grey[i].slot, g.grey[i].parity, g.grey[i].w, g.grey[i].h);
    put("%s", "\n");
    *len = n;
    if (n >= cap) return H264MI_ECAPACITY;
    return H264MI_OK;
}
#endif /* H264MI_TEST_HOOKS */
