// h264decode_amd/csrc/k_pack.hip -- K6: crop + pack to tight I420, gfx950.  Launched by mi_output.cpp, like the rest of the output stage.
#include <hip/hip_runtime.h>
#include <cstddef>
#include "mi_kernels.h"

// One launch packs any number of frames (a whole batch): blockIdx.x = frame, blockIdx.y = a chunk of its rows (luma rows,
// then the Cb rows, then the Cr rows).  A thread moves 16 bytes when source and destination rows are 16-byte aligned
// (1080p: always), single bytes otherwise.
extern "C" __global__ void __launch_bounds__(256) k_pack(const PackDesc *descs, uint8_t *dst, int rows_per_block) {
    const PackDesc pd = descs[blockIdx.x];
    const int w = static_cast<int>(pd.w), h = static_cast<int>(pd.h), W = static_cast<int>(pd.W), H = static_cast<int>(pd.H);
    const int wc = (w + 1) / 2, hc = (h + 1) / 2; // chroma plane of the packed frame (H264MI_I420_SIZE; odd w or h: monochrome streams only)
    const int nrows = h + 2 * hc; // h luma rows + hc Cb rows + hc Cr rows
    const uint8_t *src = reinterpret_cast<const uint8_t *>(pd.src);
    uint8_t *out = dst + pd.dst_off;
    const int r0 = static_cast<int>(blockIdx.y) * rows_per_block, r1 = min(r0 + rows_per_block, nrows);
    for (int r = r0; r < r1; r++) {
        const uint8_t *s;
        uint8_t *d;
        int n;
        if (r < h) {
            s = src + static_cast<size_t>(r + pd.y0) * W + pd.x0, d = out + static_cast<size_t>(r) * w, n = w;
        } else {
            const int c = r - h >= hc, rc = r - h - c * hc;
            s = src + static_cast<size_t>(W) * H + static_cast<size_t>(c) * (W / 2) * (H / 2) + static_cast<size_t>(rc + pd.y0 / 2) * (W / 2) + pd.x0 / 2;
            d = out + static_cast<size_t>(w) * h + static_cast<size_t>(c) * wc * hc + static_cast<size_t>(rc) * wc, n = wc;
        }
        if ((((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) && (n & 15) == 0) {
            for (int i = static_cast<int>(threadIdx.x) * 16; i < n; i += 256 * 16) *reinterpret_cast<uint4 *>(d + i) = *reinterpret_cast<const uint4 *>(s + i);
        } else {
            for (int i = static_cast<int>(threadIdx.x); i < n; i += 256) d[i] = s[i];
        }
    }
}
