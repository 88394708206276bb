// h264decode_amd/csrc/k_common.h -- what more than one decode-path kernel file needs (K1 entropy .. K5 deblocking, k_dbprep), gfx950.
// Macros, typedefs and __device__ helpers only, so that a file which is also compiled for the host (k_dbprep.hip: tools/dbprep_lane_check.hip)
// can include it.  The output stage (k_output_rule.h and the kernels that include it) has its own helpers and does not use this header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "mi_kernels.h"

// The lanes of ONE wavefront exchange data through LDS: no s_barrier and no wait for outstanding global stores (what __syncthreads()
// implies) -- LDS operations of a wavefront are processed in issue order, so ordering the instructions is enough.
#define WAVE_SYNC()                                            \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

// Makes a value opaque to the compiler: a lane-dependent value (the lane number, as a rule) refreshed through it at the top of a loop keeps the
// lane-dependent addresses of the body from being hoisted out of the loop -- dozens of loop-invariant addresses would otherwise live in
// registers for the whole kernel, or be spilled.
#define OPAQUE(x) asm volatile("" : "+v"(x))

// Frame memory (and every other buffer whose address arrives as an integer: PicDesc::pool_base) goes through explicit address-space-1
// pointers, best with a wave-uniform base and a 32-bit per-lane offset.  A pointer made from an integer is generic -- flat_load / flat_store,
// which are slower, count against the LDS wait counter as well (every LDS fence would wait for the sample stores) and are kept as 64-bit
// per-lane pointers in registers for the whole kernel.
typedef __attribute__((address_space(1))) uint8_t g8;
typedef __attribute__((address_space(1))) uint16_t g16;
typedef __attribute__((address_space(1))) uint32_t g32;
typedef uint32_t v4u __attribute__((ext_vector_type(4))); // native vectors: assignable across address spaces (HIP's uint4 is a struct)
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) v4u g_uint4;
typedef __attribute__((address_space(1))) v2u g_uint2;
#define GLD16(base, off) (*reinterpret_cast<const g_uint4 *>((base) + (off)))
#define GLD8(base, off) (*reinterpret_cast<const g_uint2 *>((base) + (off)))
#define GST16(base, off, v) (*reinterpret_cast<g_uint4 *>((base) + (off)) = (v))
#define GST8(base, off, v) (*reinterpret_cast<g_uint2 *>((base) + (off)) = (v))

// diagnostic build (-DMI_DB_STATS) of the deblocking kernels: shader clocks per phase of the step loop, summed over one wavefront's steps, added to
// xstatus[8 + phase] by the wavefront of group 0 of every picture (tools/deblock_phase_probe.py); k_deblock gets the status words as an extra
// argument in that build
#if defined(MI_DB_STATS)
#define STAMP(k) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); st_acc[k] += static_cast<uint32_t>(now_ - st_last); st_last = now_; } while (0)
#else
#define STAMP(k) do { } while (0)
#endif

// four samples <-> one dword, sample 0 in the low byte
__device__ __forceinline__ void unpack4(uint32_t w, int &a, int &b, int &c, int &d) {
    a = static_cast<int>(w & 255u), b = static_cast<int>(__builtin_amdgcn_ubfe(w, 8, 8)), c = static_cast<int>(__builtin_amdgcn_ubfe(w, 16, 8)), d = static_cast<int>(w >> 24);
}
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {
    return static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 8) | (static_cast<uint32_t>(c) << 16) | (static_cast<uint32_t>(d) << 24);
}

// XCD-aware order of a grid of (blocks per picture, pictures rounded up to a multiple of 8): workgroups are dealt round-robin to the 8 XCDs, each
// with its own L2, and a macroblock's neighbours are records another workgroup of the picture loads as its own -- so an XCD takes WHOLE
// pictures (picture p goes to XCD p mod 8), and the neighbour comes out of the L2 that fetched it a moment ago.
__device__ __forceinline__ void xcd_pic_block(uint32_t &pic, uint32_t &blk) {
    const uint32_t w = blockIdx.y * gridDim.x + blockIdx.x, in_xcd = w >> 3;
    pic = (in_xcd / gridDim.x) * 8u + (w & 7u), blk = in_xcd % gridDim.x;
}

// The picture's place in its frame slot (PicDesc): base = the slot's first byte; y / cb / cr = byte offsets of the picture's first luma / Cb / Cr
// row.  A field picture lives in the rows of its parity: PicDesc::pitch -- the bytes from one luma row of the PICTURE to the next -- is twice the
// frame's, and the bottom field starts one frame row in (half a frame row in the chroma planes).
// (A constructor, not a function that returns the struct: filled in place, the kernels compile to the instructions they had with these
// four lines written out; returned by value, the address arithmetic moves and with it the deblocking kernels' scalar register allocation.)
struct PicPlace {
    g8 *base;
    uint32_t y, cb, cr;
    __device__ __forceinline__ explicit PicPlace(const PicDesc *pd) {
        base = (g8 *)(pd->pool_base + static_cast<uint64_t>(pd->slot) * pd->slot_bytes);
        y = pd->field == 2 ? pd->pitch >> 1 : 0u;
        cb = pd->plane + (y >> 1), cr = cb + (pd->plane >> 2);
    }
};
