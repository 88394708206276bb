// h264decode_amd/csrc/k_jpeg.hip -- K13: baseline JPEG files of a list of frames (the rule of include/h264mi.h, "JPEG snapshots"; one copy of the
// arithmetic: k_jpeg_rule.h).  A one-wavefront workgroup owns a restart interval and walks its blocks; a lane owns a coefficient.
// BLOCK.  Lane 8y + x loads sample (x, y) of the block (coordinates clamped to the plane: the replicated edge), applies the range rule and leaves x - 128
// in LDS.  Row pass: lane 8y + k reads row y (one 16-byte LDS read) and forms r[y][k] against its row k of M, which it holds in registers; r goes back to
// LDS transposed, so that the column pass of lane 8v + k reads r[0 .. 7][k] as 16 bytes too and forms c[v][k] against row v of M.  The level is the
// rule's division; a shuffle by the zigzag permutation then gives lane z the level of zigzag position z.
// CODES.  One 64-bit ballot of the non-zero AC levels gives lane z its run (z - 1 - the highest set bit below z), hence its ZRL count, its (run, size)
// code and its magnitude bits: at most 3 x 11 + 16 + 10 = 59 bits, a 64-bit word per lane.  Lane 0 codes the DC difference, lane 63 the EOB when its own
// level is zero.  A wavefront prefix sum of the lengths gives every lane its bit offset, and the lanes OR their bits, most significant first, into the
// wavefront's bit buffer in LDS (MI_JPEG_BUF_WORDS words; at most three words per lane).
// FLUSH.  Before a block that might not fit (MI_JPEG_BLOCK_BITS), and at the end of the interval behind the pad bits: lane i takes bytes 16 i .. 16 i + 15
// of the buffer, counts them and their 0xFF bytes, a second prefix sum gives its place in the output, and it stores its bytes, each 0xFF followed by 0x00.
// k_jpeg_size counts only; k_jpeg_write stores, and only into items that k_jpeg_scan found to fit their slot -- every store is checked against the
// slot's end all the same.  Plain C++ and vector memory instructions only: no inline assembly.
// What bounds it: the serial walk of the blocks of an interval by one wavefront -- two LDS round trips, a shuffle, a ballot and a prefix sum of 6 steps
// per block, all dependent -- not memory (profiles/k13_jpeg.txt).
#include "mi_kernels.h"
#include "k_jpeg_rule.h"
#include "../../include/h264mi.h"

#define JPEG_LDS_BYTES (4 * MI_JPEG_BUF_WORDS + 4 * 512 + 4 * 32 + 2 * 64 + 2 * 64) /* bit buffer, AC codes, DC codes, samples, row pass: 3456 */

struct alignas(16) JpegLds {
    uint32_t buf[MI_JPEG_BUF_WORDS];
    uint32_t ac[2][256];
    uint32_t dc[2][16];
    int16_t xs[64];
    int16_t rt[64];
};
static_assert(sizeof(JpegLds) == JPEG_LDS_BYTES, "the LDS size the file states");

typedef short short8 __attribute__((ext_vector_type(8)));

template <class T> __device__ static __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

struct JpegWave {
    uint32_t pos;     // bits in the buffer
    uint32_t written; // bytes of the interval so far, stuffing included
};

// bytes 0 .. nbytes - 1 of the bit buffer leave it (nbytes is a multiple of 4, or the buffer's whole content at the end of the interval)
template <bool WRITE> __device__ static __forceinline__ void jpeg_flush(JpegLds &L, JpegWave &W, uint32_t nbytes, uint8_t *out, const uint8_t *lim, int lane) {
    __syncthreads();
    const uint4 w4 = reinterpret_cast<const uint4 *>(L.buf)[lane];
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    const int vb = min(max(static_cast<int>(nbytes) - 16 * lane, 0), 16);
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
        if (i < vb) cnt += 1 + (b == 255u);
    }
    const int incl = wave_incl_scan(cnt, lane);
    if (WRITE) {
        uint8_t *p = out + W.written + (incl - cnt);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t b = (w[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
            if (i < vb) {
                if (p < lim) *p = static_cast<uint8_t>(b);
                p++;
                if (b == 255u) {
                    if (p < lim) *p = 0;
                    p++;
                }
            }
        }
    }
    W.written += static_cast<uint32_t>(__shfl(incl, 63));
    const uint32_t remw = nbytes >> 2;
    const uint32_t rem = remw < MI_JPEG_BUF_WORDS ? L.buf[remw] : 0u;
    __syncthreads();
    reinterpret_cast<uint4 *>(L.buf)[lane] = make_uint4(lane == 0 ? rem : 0u, 0u, 0u, 0u);
    W.pos -= 8 * nbytes;
    __syncthreads();
}

template <bool WRITE> __device__ static __forceinline__ void jpeg_interval(const uint8_t *table, uint32_t *ivl, uint8_t *dst, uint32_t total) {
    __shared__ JpegLds L;
    const int lane = static_cast<int>(threadIdx.x);
    const uint32_t g = blockIdx.x;
    if (g >= total) return;
    const JpegParams *P = reinterpret_cast<const JpegParams *>(table);
    const JpegDesc *descs = reinterpret_cast<const JpegDesc *>(table + sizeof(JpegParams));
    uint32_t lo = 0, hi = P->n_items - 1;
    while (lo < hi) { // the last item whose first interval is not behind g
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (descs[mid].ivl_base <= g) lo = mid;
        else hi = mid - 1;
    }
    const JpegDesc D = descs[lo];
    const uint32_t j = g - D.ivl_base;
    if (j >= D.n_int) return;
    uint8_t *slot = dst + D.slot_off;
    const uint8_t *lim = slot + P->slot_bytes;
    if (WRITE && reinterpret_cast<const h264mi_jpeg_result *>(dst)[lo].status != 0) return; // it does not fit: nothing of it is written
    uint8_t *out = slot + (WRITE ? ivl[g] : 0u);

    for (int i = lane; i < 512; i += 64) (&L.ac[0][0])[i] = (&P->ac[0][0])[i];
    if (lane < 24) L.dc[lane / 12][lane % 12] = P->dc[lane / 12][lane % 12];
    reinterpret_cast<uint4 *>(L.buf)[lane] = make_uint4(0u, 0u, 0u, 0u);
    const int row = lane >> 3, col = lane & 7;
    int mk[8], mv[8];
#pragma unroll
    for (int n = 0; n < 8; n++) mk[n] = jpeg_m(col, n), mv[n] = jpeg_m(row, n);
    const int q0 = P->q[0][lane], q1 = P->q[1][lane];
    const int zz = jpeg_zigzag(lane);
    __syncthreads();

    JpegWave W = {0u, 0u};
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const uint32_t m_end = min((j + 1) * D.restart, D.n_mcus);
    const int nb = D.mono ? 1 : 6;
    const int cw = static_cast<int>((D.w + 1) >> 1), ch = static_cast<int>((D.h + 1) >> 1);
    for (uint32_t m = j * D.restart; m < m_end; m++) {
        const int mx = static_cast<int>(m % D.mcus_w), my = static_cast<int>(m / D.mcus_w);
        for (int b = 0; b < nb; b++) {
            const int comp = b < 4 ? 0 : b - 3;
            const uint8_t *plane = reinterpret_cast<const uint8_t *>(comp == 0 ? D.y : comp == 1 ? D.cb : D.cr);
            const int stride = static_cast<int>(comp == 0 ? D.ystride : D.cstride);
            const int pw = comp == 0 ? static_cast<int>(D.w) : cw, ph = comp == 0 ? static_cast<int>(D.h) : ch;
            const int bx = D.mono ? mx : comp == 0 ? 2 * mx + (b & 1) : mx, by = D.mono ? my : comp == 0 ? 2 * my + (b >> 1) : my;
            if (W.pos + MI_JPEG_BLOCK_BITS > 32u * MI_JPEG_BUF_WORDS) jpeg_flush<WRITE>(L, W, (W.pos >> 5) * 4, out, lim, lane);
            // ---- the block rule
            const int px = min(8 * bx + col, pw - 1), py = min(8 * by + row, ph - 1);
            int s = plane[static_cast<size_t>(py) * stride + px];
            if (D.full) s = comp == 0 ? jpeg_full_y(s) : jpeg_full_c(s);
            L.xs[lane] = static_cast<int16_t>(s - 128);
            __syncthreads();
            const short8 xr = reinterpret_cast<const short8 *>(L.xs)[row];
            int a = 0;
#pragma unroll
            for (int n = 0; n < 8; n++) a += mk[n] * xr[n];
            L.rt[8 * col + row] = static_cast<int16_t>((a + 128) >> 8);
            __syncthreads();
            const short8 rk = reinterpret_cast<const short8 *>(L.rt)[col];
            int c = 0;
#pragma unroll
            for (int y = 0; y < 8; y++) c += mv[y] * rk[y];
            const int lvl = jpeg_level(c, comp == 0 ? q0 : q1);
            const int lz = __shfl(lvl, zz); // lane z: the level at zigzag position z
            // ---- its codes
            const int tab = comp == 0 ? 0 : 1;
            const int dcv = __builtin_amdgcn_readfirstlane(lz);
            const int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
            if (comp == 0) pred0 = dcv;
            else if (comp == 1) pred1 = dcv;
            else pred2 = dcv;
            const unsigned long long nzm = __ballot(lz != 0) & ~1ull;
            unsigned long long bits = 0;
            int len = 0;
            const int v = lane == 0 ? lz - pred : lz;
            const int sz = 32 - __clz(abs(v));
            const uint32_t mag = static_cast<uint32_t>(v < 0 ? v - 1 : v) & ((1u << sz) - 1u);
            if (lane == 0) {
                const uint32_t e = L.dc[tab][sz];
                bits = e & 0xffffu, len = static_cast<int>(e >> 16);
                bits = bits << sz | mag, len += sz;
            } else if (lz != 0) {
                const unsigned long long below = nzm & ((1ull << lane) - 1ull);
                const int run = lane - 1 - (below ? 63 - __clzll(below) : 0);
                const uint32_t zrl = L.ac[tab][0xf0];
                for (int k = run >> 4; k > 0; k--) bits = bits << (zrl >> 16) | (zrl & 0xffffu), len += static_cast<int>(zrl >> 16);
                const uint32_t e = L.ac[tab][(run & 15) << 4 | sz];
                bits = bits << (e >> 16) | (e & 0xffffu), len += static_cast<int>(e >> 16);
                bits = bits << sz | mag, len += sz;
            } else if (lane == 63) {
                const uint32_t e = L.ac[tab][0]; // EOB
                bits = e & 0xffffu, len = static_cast<int>(e >> 16);
            }
            const int incl = wave_incl_scan(len, lane);
            if (len) {
                const uint32_t start = W.pos + static_cast<uint32_t>(incl - len);
                const unsigned long long left = bits << (64 - len);
                const uint32_t w0 = start >> 5, sh = start & 31u;
                const uint32_t a0 = static_cast<uint32_t>(left >> (32u + sh)), a1 = static_cast<uint32_t>(left >> sh);
                const uint32_t a2 = sh ? static_cast<uint32_t>(left) << (32u - sh) : 0u;
                if (a0 && w0 < MI_JPEG_BUF_WORDS) atomicOr(&L.buf[w0], a0);
                if (a1 && w0 + 1 < MI_JPEG_BUF_WORDS) atomicOr(&L.buf[w0 + 1], a1);
                if (a2 && w0 + 2 < MI_JPEG_BUF_WORDS) atomicOr(&L.buf[w0 + 2], a2);
            }
            W.pos += static_cast<uint32_t>(__shfl(incl, 63));
        }
    }
    // ---- pad 1-bits to a byte boundary (they lie in one byte, so in one word), the rest of the buffer, the marker
    const uint32_t pad = (8u - (W.pos & 7u)) & 7u;
    if (pad && lane == 0) atomicOr(&L.buf[W.pos >> 5], ((1u << pad) - 1u) << (32u - (W.pos & 31u) - pad));
    W.pos += pad;
    jpeg_flush<WRITE>(L, W, W.pos >> 3, out, lim, lane);
    if (!WRITE) {
        if (lane == 0) ivl[g] = W.written;
        return;
    }
    if (lane == 0) {
        uint8_t *p = out + W.written;
        if (p + 2 <= lim) p[0] = 0xff, p[1] = static_cast<uint8_t>(j + 1 < D.n_int ? 0xd0u + (j & 7u) : 0xd9u); // RST(j mod 8), or EOI
    }
    if (j == 0) { // the header: the template of the launch with the item's size and restart interval
        const int t = D.mono ? 1 : 0;
        const uint32_t n = P->hdr_len[t], so = P->sof_off[t], ro = P->dri_off[t];
        for (uint32_t i = static_cast<uint32_t>(lane); i < n; i += 64) {
            uint32_t b = P->hdr[t][i];
            if (i == so) b = D.h >> 8;
            if (i == so + 1) b = D.h & 255u;
            if (i == so + 2) b = D.w >> 8;
            if (i == so + 3) b = D.w & 255u;
            if (i == ro) b = D.restart >> 8;
            if (i == ro + 1) b = D.restart & 255u;
            if (slot + i < lim) slot[i] = static_cast<uint8_t>(b);
        }
    }
}

extern "C" __global__ void __launch_bounds__(64) k_jpeg_size(const uint8_t *table, uint32_t *ivl, uint32_t total) { jpeg_interval<false>(table, ivl, nullptr, total); }

extern "C" __global__ void __launch_bounds__(64) k_jpeg_write(const uint8_t *table, const uint32_t *ivl, uint8_t *dst, uint32_t total) {
    jpeg_interval<true>(table, const_cast<uint32_t *>(ivl), dst, total);
}

// one wavefront per item: the lengths of its intervals become their offsets in the slot (behind the header, two marker bytes behind every interval),
// and the item's result: the length of the file, whether it fits its slot, the size SOF0 carries
extern "C" __global__ void __launch_bounds__(64) k_jpeg_scan(const uint8_t *table, uint32_t *ivl, uint8_t *dst) {
    const int lane = static_cast<int>(threadIdx.x);
    const JpegParams *P = reinterpret_cast<const JpegParams *>(table);
    const uint32_t item = blockIdx.x;
    if (item >= P->n_items) return;
    const JpegDesc D = reinterpret_cast<const JpegDesc *>(table + sizeof(JpegParams))[item];
    uint32_t at = P->hdr_len[D.mono ? 1 : 0];
    for (uint32_t base = 0; base < D.n_int; base += 64) {
        const uint32_t k = base + static_cast<uint32_t>(lane);
        const uint32_t len = k < D.n_int ? ivl[D.ivl_base + k] + 2u : 0u; // (32 bits suffice: a file is shorter than h264mi_jpeg_size's bound, which is)
        const uint32_t incl = wave_incl_scan(len, lane);
        if (k < D.n_int) ivl[D.ivl_base + k] = at + (incl - len);
        at += __shfl(incl, 63);
    }
    if (lane == 0) {
        h264mi_jpeg_result r;
        r.bytes = at, r.status = at > P->slot_bytes ? H264MI_JPEG_TRUNCATED : 0u, r.w = D.w, r.h = D.h;
        reinterpret_cast<h264mi_jpeg_result *>(dst)[item] = r;
    }
}
