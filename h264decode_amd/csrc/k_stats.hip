// h264decode_amd/csrc/k_stats.hip -- K12: the statistics of a list of frames, each against a predecessor frame of the same size or none (the rule of
// include/h264mi.h, "Frame statistics"): one h264mi_frame_stats record per item and, with a grid, planes of per-cell sums behind it.  The project's one
// reduction.  The structure is K10's: blockIdx.x = item, blockIdx.y = a band of rows, a thread owns 16 columns -- here of 8 rows, a thread item of 128
// samples -- and there are the two paths of the other output kernels: 16-byte loads where the source's pointer, the predecessor's, the origin and the
// width allow (1080p: always; load16 of k_deint_rule.h), single bytes otherwise (bytes outside the width read as zero in both frames: they add to no sum).
// A band is MI_STATS_LUMA_ROWS luma rows, whole cell rows of every cell size and anchored at the display origin, so a cell belongs to ONE block; or
// MI_STATS_CHROMA_ROWS rows of the Cb-then-Cr row space.  Sums are dot products of packed bytes (against 0x01010101, and against the word itself for
// the squares), the absolute differences are v_sad_u8's; for squares and the count the differences are formed in packed 16-bit lanes and put back into
// bytes.  Partial sums stay in 32 bits while they cannot overflow (the static_asserts of mi_kernels.h), cross the lanes of a wavefront in 64 bits, and
// leave it as one atomic per field and wavefront.
// EXACTNESS.  The host clears the destination range ahead of the launch; every block ADDS its partial results with integer atomics (max_y: an atomic
// maximum).  Integer addition and maximum are associative and commutative, so the result does not depend on the order in which blocks, wavefronts or
// lanes arrive: the records are exact and the same from run to run.  min_y cannot start from a cleared field: the blocks take the maximum of
// 255 - (their smallest sample) in StatsDesc::inv_min, and the block that draws the item's last ticket writes min_y and the record's constants.  Only
// read-modify-write atomics carry values between blocks; each block waits for its own before it draws its ticket.
// HISTOGRAM.  256 bins per wavefront in LDS (4 KB a block), added up and flushed with one global atomic per non-empty bin.  The hazard is contention:
// 64 lanes that hold the same value serialise on one bin.  MI_STATS_HIST selects what is done about it (profiles/k12_stats.txt has the comparison):
//   0  nothing: one copy per wavefront
//   1  four interleaved copies per wavefront (lane & 3), 16 KB a block: a conflict is a quarter as deep, every add pays the wider index
//   2  a ballot of equal values: a word that every lane of the wavefront holds alike is counted once, by one lane, with the lane count (and in one add
//      where its four bytes are alike); other words take path 0.  A flat picture then costs 1 add per word and wavefront instead of 256 colliding ones.
// Measured once each, 1920 frames of 1080p, record only: natural content 1.49 / 1.31 / 1.49 ms; flat frames 13.3 / 3.6 / 1.24 ms (K6 over the same frames:
// 2.4 ms).  2 is the default: it turns the worst case into the cheapest one at no measurable cost elsewhere, and keeps the LDS at 4 KB.
// Plain C++ and vector memory instructions only: no inline assembly.
#include "mi_kernels.h"
#include "k_deint_rule.h" // load16; pack4, byte_of
#include "../../include/h264mi.h"

#ifndef MI_STATS_HIST
#define MI_STATS_HIST 2
#endif
#define STATS_COPIES (MI_STATS_HIST == 1 ? 4 : 1)
#define STATS_LDS_WORDS (4 * 256 * STATS_COPIES) /* four wavefronts */

#define RLX __ATOMIC_RELAXED
#define AGENT __HIP_MEMORY_SCOPE_AGENT
#define WGRP __HIP_MEMORY_SCOPE_WORKGROUP

typedef short pk16 __attribute__((ext_vector_type(2)));
template <bool ODD> __device__ static __forceinline__ pk16 lanes_of(uint32_t w) { return __builtin_bit_cast(pk16, __builtin_amdgcn_perm(0u, w, ODD ? 0x0c030c01u : 0x0c020c00u)); }
// |a - b| of the four bytes of two words, as bytes again (in the order 0, 2, 1, 3: every use is a sum over the four)
__device__ static __forceinline__ uint32_t absdiff4(uint32_t a, uint32_t b) {
    const pk16 ae = lanes_of<false>(a), be = lanes_of<false>(b), ao = lanes_of<true>(a), bo = lanes_of<true>(b);
    const pk16 e = __builtin_elementwise_max(ae, be) - __builtin_elementwise_min(ae, be), o = __builtin_elementwise_max(ao, bo) - __builtin_elementwise_min(ao, bo);
    return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}
// how many of the four bytes of d exceed t (0 .. 255): byte + (255 - t) carries into bit 8 of its 16-bit lane exactly then
__device__ static __forceinline__ uint32_t count_above(uint32_t d, uint32_t bias2) {
    return static_cast<uint32_t>(__builtin_popcount(((d & 0x00ff00ffu) + bias2) & 0x01000100u) + __builtin_popcount((((d >> 8) & 0x00ff00ffu) + bias2) & 0x01000100u));
}

template <class T> __device__ static __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ static __forceinline__ void add64(uint64_t *p, uint64_t v) {
    if (v) __hip_atomic_fetch_add(p, v, RLX, AGENT);
}
__device__ static __forceinline__ void add32(uint32_t *p, uint32_t v) {
    if (v) __hip_atomic_fetch_add(p, v, RLX, AGENT);
}

// the byte path's word: bytes 0 .. v - 1 of p (v <= 0: none, v >= 4: all four), zero beyond them -- what lies outside the width adds to no sum, in either frame
__device__ static __forceinline__ uint32_t word4(const uint8_t *p, int v) {
    const uint32_t b0 = v > 0 ? p[0] : 0u, b1 = v > 1 ? p[1] : 0u, b2 = v > 2 ? p[2] : 0u, b3 = v > 3 ? p[3] : 0u;
    return pack4(b0, b1, b2, b3);
}

// one word of a luma row into the wavefront's histogram: its first v bytes (v >= 4: all four)
__device__ static __forceinline__ void hist4(uint32_t *hw, uint32_t w, int v, int lane) {
#if MI_STATS_HIST == 2
    const uint32_t first = __builtin_amdgcn_readfirstlane(w);
    const unsigned long long here = __builtin_amdgcn_ballot_w64(true);
    if (__builtin_amdgcn_ballot_w64(w == first && v >= 4) == here) { // (uniform: every active lane holds `first`, whole)
        if (lane == __builtin_ctzll(here)) {
            const uint32_t cnt = static_cast<uint32_t>(__builtin_popcountll(here));
            if (first == (first & 255u) * 0x01010101u) {
                __hip_atomic_fetch_add(&hw[first & 255u], 4 * cnt, RLX, WGRP);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) __hip_atomic_fetch_add(&hw[byte_of(first, j)], cnt, RLX, WGRP);
            }
        }
        return;
    }
#endif
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (j < v) {
#if MI_STATS_HIST == 1
            __hip_atomic_fetch_add(&hw[byte_of(w, j) * 4 + (lane & 3)], 1u, RLX, WGRP);
#else
            __hip_atomic_fetch_add(&hw[byte_of(w, j)], 1u, RLX, WGRP);
#endif
        }
}

// what a thread accumulates over its thread items
struct Acc {
    uint32_t sum, sum2, sad, sse, chg;
};

// rows r0 .. r0 + nr - 1 (nr <= 8), columns x .. x + n - 1 (n <= 16) of one display plane (row r at sp + r * pitch; the predecessor's at pp alike).
// LUMA: squares, the count, the histogram and the cells; chroma: the two sums only.  half[2]: the sums of columns 0 .. 7 and 8 .. 15, for the cells
template <bool VEC, bool PREV, bool LUMA>
__device__ static __forceinline__ void stats_item(const uint8_t *sp, const uint8_t *pp, int pitch, int r0, int nr, int x, int n, uint32_t bias2, uint32_t *hw, int lane, Acc &acc,
                                                  uint32_t hsum[2], uint32_t hsad[2]) {
    hsum[0] = hsum[1] = hsad[0] = hsad[1] = 0;
    const uint8_t *s = sp + static_cast<size_t>(r0) * pitch + x, *p = pp + static_cast<size_t>(r0) * pitch + x;
    for (int r = 0; r < nr; r++, s += pitch, p += pitch) {
        uint32_t a[4], b[4];
        if (VEC) {
            load16<true>(s, 16, a);
            if (PREV) load16<true>(p, 16, b);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!VEC) { // a word at a time: sixteen byte loads of each frame in flight at once cost more registers than the kernel has
                a[k] = word4(s + 4 * k, n - 4 * k);
                if (PREV) b[k] = word4(p + 4 * k, n - 4 * k);
            }
            hsum[k >> 1] = __builtin_amdgcn_udot4(a[k], 0x01010101u, hsum[k >> 1], false);
            if (LUMA) acc.sum2 = __builtin_amdgcn_udot4(a[k], a[k], acc.sum2, false);
            if (PREV) {
                hsad[k >> 1] = __builtin_amdgcn_sad_u8(a[k], b[k], hsad[k >> 1]);
                if (LUMA) {
                    const uint32_t d = absdiff4(a[k], b[k]);
                    acc.sse = __builtin_amdgcn_udot4(d, d, acc.sse, false);
                    acc.chg += count_above(d, bias2);
                }
            }
            if (LUMA) hist4(hw, a[k], VEC ? 4 : n - 4 * k, lane);
        }
    }
    acc.sum += hsum[0] + hsum[1];
    if (PREV) acc.sad += hsad[0] + hsad[1];
}

template <bool PREV>
__device__ static __forceinline__ void stats_block(StatsDesc *sdp, const StatsDesc &sd, uint8_t *dst, uint32_t cell_log2, uint32_t planes, uint32_t thresh, uint32_t *lds) {
    const int w = static_cast<int>(sd.w), h = static_cast<int>(sd.h), W = static_cast<int>(sd.W), H = static_cast<int>(sd.H);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2, Wc = W / 2;
    const int nb_y = mi_stats_luma_blocks(h), nb_c = mi_stats_chroma_blocks(h);
    const int b = static_cast<int>(blockIdx.y);
    if (b >= nb_y + nb_c) return; // (a launch is sized by its tallest item)
    const uint8_t *src = reinterpret_cast<const uint8_t *>(sd.src), *prev = PREV ? reinterpret_cast<const uint8_t *>(sd.prev) : src; // (prev: never read without PREV)
    h264mi_frame_stats *rec = reinterpret_cast<h264mi_frame_stats *>(dst + sd.dst_off);
    uint32_t *plane0 = reinterpret_cast<uint32_t *>(rec + 1);
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    // W is a multiple of 16, so luma rows stay aligned when the origin is; chroma rows, planes and origin need the same of W / 2, x0 / 2 and ceil(w / 2)
    const bool vec_y = ((sd.src | sd.prev | sd.x0 | sd.w) & 15) == 0;
    const bool vec_c = vec_y && ((sd.W | sd.x0 | sd.w) & 31) == 0;
    const uint32_t bias2 = (255u - thresh) * 0x00010001u;
    Acc acc = {0, 0, 0, 0, 0};
    uint32_t hsum[2], hsad[2];
    if (b < nb_y) {
        for (int i = tid; i < STATS_LDS_WORDS; i += 256) lds[i] = 0;
        __syncthreads();
        uint32_t *hw = lds + wave * 256 * STATS_COPIES;
        const int ng = (w + 15) / 16, row0 = b * MI_STATS_LUMA_ROWS;
        const int items = (min(MI_STATS_LUMA_ROWS, h - row0) + 7) / 8 * ng;
        const size_t org = static_cast<size_t>(sd.y0) * W + sd.x0;
        uint32_t *csum = plane0, *csad = plane0 + ((planes & H264MI_STATS_CELL_SUM) ? sd.gw * sd.gh : 0);
        for (int i = tid; i < items; i += 256) {
            const int r0 = row0 + 8 * (i / ng), x = 16 * (i % ng);
            const int nr = min(8, h - r0), n = min(16, w - x);
            if (vec_y) stats_item<true, PREV, true>(src + org, prev + org, W, r0, nr, x, 16, bias2, hw, lane, acc, hsum, hsad);
            else stats_item<false, PREV, true>(src + org, prev + org, W, r0, nr, x, n, bias2, hw, lane, acc, hsum, hsad);
            if (planes) { // the item's 8 rows lie in one cell row; its 16 columns in one cell, or in two of cell size 8 (the second one only if it has a column)
                const uint32_t at = static_cast<uint32_t>(r0 >> cell_log2) * sd.gw + static_cast<uint32_t>(x >> cell_log2);
                const bool two = cell_log2 == 3;
                if (planes & H264MI_STATS_CELL_SUM) {
                    add32(csum + at, two ? hsum[0] : hsum[0] + hsum[1]);
                    if (two && n > 8) add32(csum + at + 1, hsum[1]);
                }
                if (PREV && (planes & H264MI_STATS_CELL_SAD)) {
                    add32(csad + at, two ? hsad[0] : hsad[0] + hsad[1]);
                    if (two && n > 8) add32(csad + at + 1, hsad[1]);
                }
            }
        }
        // the fields: across the wavefront in 64 bits, then one atomic per field and wavefront
        const uint64_t s1 = wave_sum<uint64_t>(acc.sum), s2 = wave_sum<uint64_t>(acc.sum2);
        if (lane == 0) add64(&rec->sum_y, s1), add64(&rec->sum_y2, s2);
        if (PREV) {
            const uint64_t d1 = wave_sum<uint64_t>(acc.sad), d2 = wave_sum<uint64_t>(acc.sse);
            const uint32_t ch = wave_sum<uint32_t>(acc.chg);
            if (lane == 0) add64(&rec->sad_y, d1), add64(&rec->sse_y, d2), add32(&rec->changed_y, ch);
        }
        // the histogram: bin `tid` of the four wavefronts; the block's smallest and largest sample from the bins that are not empty
        __syncthreads();
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
#if MI_STATS_HIST == 1
            c += lds[k * 1024 + 4 * tid] + lds[k * 1024 + 4 * tid + 1] + lds[k * 1024 + 4 * tid + 2] + lds[k * 1024 + 4 * tid + 3];
#else
            c += lds[k * 256 + tid];
#endif
        }
        add32(&rec->hist_y[tid], c);
        const unsigned long long full = __builtin_amdgcn_ballot_w64(c != 0);
        __syncthreads(); // (every bin has been read: the words are reused)
        if (lane == 0) {
            lds[2 * wave] = full ? static_cast<uint32_t>(64 * wave + __builtin_ctzll(full)) : 255u;
            lds[2 * wave + 1] = full ? static_cast<uint32_t>(64 * wave + 63 - __builtin_clzll(full)) : 0u;
        }
        __syncthreads();
    } else {
        // chroma: MI_STATS_CHROMA_ROWS rows of the row space [ceil(hc / 8) * 8 rows of Cb][as many of Cr]; an item lies in one plane
        const int nc8 = (hc + 7) / 8, ng = (wc + 15) / 16, o0 = (b - nb_y) * (MI_STATS_CHROMA_ROWS / 8);
        const int items = min(MI_STATS_CHROMA_ROWS / 8, 2 * nc8 - o0) * ng;
        Acc cr = {0, 0, 0, 0, 0};
        for (int i = tid; i < items; i += 256) {
            const int o = o0 + i / ng, x = 16 * (i % ng);
            const int c = o >= nc8, r0 = 8 * (o - c * nc8);
            const int nr = min(8, hc - r0), n = min(16, wc - x);
            const size_t org = static_cast<size_t>(W) * H + static_cast<size_t>(c) * Wc * (H / 2) + static_cast<size_t>(sd.y0 / 2) * Wc + sd.x0 / 2;
            Acc &to = c ? cr : acc;
            if (vec_c) stats_item<true, PREV, false>(src + org, prev + org, Wc, r0, nr, x, 16, bias2, nullptr, lane, to, hsum, hsad);
            else stats_item<false, PREV, false>(src + org, prev + org, Wc, r0, nr, x, n, bias2, nullptr, lane, to, hsum, hsad);
        }
        const uint64_t sb = wave_sum<uint64_t>(acc.sum), sr = wave_sum<uint64_t>(cr.sum);
        if (lane == 0) add64(&rec->sum_cb, sb), add64(&rec->sum_cr, sr);
        if (PREV) {
            const uint64_t db = wave_sum<uint64_t>(acc.sad), dr = wave_sum<uint64_t>(cr.sad);
            if (lane == 0) add64(&rec->sad_cb, db), add64(&rec->sad_cr, dr);
        }
    }
    // the ticket.  Thread 0's own atomics on inv_min and max_y have returned before it draws (it uses what they return); what the last block reads back
    // is inv_min alone, through an atomic as well
    if (tid == 0) {
        uint32_t seen = 0;
        if (b < nb_y) {
            const uint32_t lo = min(min(lds[0], lds[2]), min(lds[4], lds[6])), hi = max(max(lds[1], lds[3]), max(lds[5], lds[7]));
            seen = __hip_atomic_fetch_max(&sdp->inv_min, 255u - lo, RLX, AGENT);
            seen |= __hip_atomic_fetch_max(&rec->max_y, hi, RLX, AGENT);
        }
        const uint32_t total = static_cast<uint32_t>(nb_y + nb_c);
        const uint32_t drawn = __hip_atomic_fetch_add(&sdp->ticket, 1u + (seen & 0x80000000u), RLX, AGENT); // (seen < 256: the term is 0, and orders the draw behind the two)
        if (drawn == total - 1) {
            // (added to cleared fields like everything else, so that no plain store shares a cache line with another block's atomics)
            const uint32_t inv = __hip_atomic_fetch_max(&sdp->inv_min, 0u, RLX, AGENT);
            add32(&rec->min_y, 255u - inv);
            add32(&rec->has_prev, PREV ? 1u : 0u);
            add32(&rec->w, sd.w), add32(&rec->h, sd.h), add32(&rec->gw, sd.gw), add32(&rec->gh, sd.gh);
        }
    }
}

extern "C" __global__ void __launch_bounds__(256, 4) k_stats(StatsDesc *descs, uint8_t *dst, uint32_t cell_log2, uint32_t planes, uint32_t thresh) {
    __shared__ uint32_t lds[STATS_LDS_WORDS];
    const StatsDesc sd = descs[blockIdx.x];
    if (sd.prev) stats_block<true>(&descs[blockIdx.x], sd, dst, cell_log2, planes, thresh, lds);
    else stats_block<false>(&descs[blockIdx.x], sd, dst, cell_log2, planes, thresh, lds);
}
