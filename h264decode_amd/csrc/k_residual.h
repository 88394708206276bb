// h264decode_amd/csrc/k_residual.h -- residual decoding shared by K3 (k_recon.hip) and K4 (k_inter.hip): the scaling of 8.5.12.1 / 8.5.13
// and the 1-D inverse transforms of 8.5.12.2 / 8.5.13, gfx950.  A caller runs a transform over the rows, then over the columns, and rounds
// with (x + 32) >> 6.  (Clip1 is NOT here: K3's clip255 is a plain clamp, K4's is opaque to the compiler on purpose -- see k_inter.hip.)
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void inv4(int d0, int d1, int d2, int d3, int &o0, int &o1, int &o2, int &o3) {
    int e0 = d0 + d2, e1 = d0 - d2, e2 = (d1 >> 1) - d3, e3 = d1 + (d3 >> 1);
    o0 = e0 + e3, o1 = e1 + e2, o2 = e1 - e2, o3 = e0 - e3;
}
__device__ __forceinline__ void inv8(const int *d, int *o) {
    int e0 = d[0] + d[4], e1 = -d[3] + d[5] - d[7] - (d[7] >> 1), e2 = d[0] - d[4], e3 = d[1] + d[7] - d[3] - (d[3] >> 1);
    int e4 = (d[2] >> 1) - d[6], e5 = -d[1] + d[7] + d[5] + (d[5] >> 1), e6 = d[2] + (d[6] >> 1), e7 = d[3] + d[5] + d[1] + (d[1] >> 1);
    int f0 = e0 + e6, f1 = e1 + (e7 >> 2), f2 = e2 + e4, f3 = e3 + (e5 >> 2);
    int f4 = e2 - e4, f5 = (e3 >> 2) - e5, f6 = e0 - e6, f7 = e7 - (e1 >> 2);
    o[0] = f0 + f7, o[1] = f2 + f5, o[2] = f4 + f3, o[3] = f6 + f1;
    o[4] = f6 - f1, o[5] = f4 - f3, o[6] = f2 - f5, o[7] = f0 - f7;
}
__device__ __forceinline__ int scale4(int c, int ls, int qp) { // 8.5.12.1
    int per = qp / 6;
    return per >= 4 ? (c * ls) << (per - 4) : (c * ls + (1 << (3 - per))) >> (4 - per);
}
__device__ __forceinline__ int scale8(int c, int ls, int qp) { // 8.5.13
    int per = qp / 6;
    return per >= 6 ? (c * ls) << (per - 6) : (c * ls + (1 << (5 - per))) >> (6 - per);
}
