// h264decode_amd/csrc/k_jpeg_rule.h -- the ONE copy of the JPEG rule of include/h264mi.h ("JPEG snapshots"): the quantisation tables, the integer block
// rule (forward DCT and quantisation), the range rule, the zigzag order and the Annex K.3.3 Huffman tables, as host / device functions.  K13
// (k_jpeg.hip) evaluates them a coefficient per lane, h264mi_jpeg_block (mi_output.cpp) is the host face of the same functions, and the host builds the
// code tables and the file header from the same arrays.  Everything is static and inlined; tables are function-local constants so that both sides see them.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif
#define JPEG_HD __host__ __device__ static inline

// M[k][n] = rint(16384 * a_k * cos((2n + 1) k pi / 16)), a_0 = sqrt(1/8), a_k = 1/2 otherwise: row k.  Row k is even in n for even k, odd for odd k
JPEG_HD int jpeg_m(int k, int n) {
    const int16_t m[8][4] = {{5793, 5793, 5793, 5793}, {8035, 6811, 4551, 1598},  {7568, 3135, -3135, -7568}, {6811, -1598, -8035, -4551},
                             {5793, -5793, -5793, 5793}, {4551, -8035, 1598, 6811}, {3135, -7568, 7568, -3135}, {1598, -4551, 6811, -8035}};
    return n < 4 ? m[k][n] : ((k & 1) ? -m[k][7 - n] : m[k][7 - n]);
}

// natural index (8 * row + column) of zigzag position z
JPEG_HD int jpeg_zigzag(int z) {
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[z];
}

// Annex K.1, natural order: table 0 luminance, table 1 chrominance
JPEG_HD int jpeg_base_q(int chroma, int i) {
    const uint8_t base[2][64] = {{16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
                                 {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    return base[chroma][i];
}
// the IJG scaling: quality 1 .. 100
JPEG_HD int jpeg_q(int quality, int chroma, int i) {
    const int sc = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (jpeg_base_q(chroma, i) * sc + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

// the block rule, one coefficient at a time.  Row pass: r[y][k] = (sum over n of M[k][n] * x[y][n] + 128) >> 8 (arithmetic), |r| <= 23172
JPEG_HD int jpeg_row_term(const int16_t x[8], int k) {
    int a = 0;
    for (int n = 0; n < 8; n++) a += jpeg_m(k, n) * x[n];
    return (a + 128) >> 8;
}
// column pass: c[v][k] = sum over y of M[v][y] * r[y][k] -- rk: r[0 .. 7][k].  |c| <= 46344 * 23172 < 1.08e9
JPEG_HD int jpeg_col_term(const int16_t rk[8], int v) {
    int a = 0;
    for (int y = 0; y < 8; y++) a += jpeg_m(v, y) * rk[y];
    return a;
}
// level = sign(c) * ((|c| + (Q << 19)) div (Q << 20)), Q 1 .. 255: the sum stays below 1.08e9 + 1.34e8 < 2^31
JPEG_HD int jpeg_level(int c, int q) {
    const uint32_t a = static_cast<uint32_t>(c < 0 ? -c : c);
    const int l = static_cast<int>((a + (static_cast<uint32_t>(q) << 19)) / (static_cast<uint32_t>(q) << 20));
    return c < 0 ? -l : l;
}

// the range rule: limited -> full, per plane
JPEG_HD int jpeg_full_y(int y) {
    const int c = y < 16 ? 16 : y > 235 ? 235 : y;
    return (255 * (c - 16) + 109) / 219;
}
JPEG_HD int jpeg_full_c(int v) {
    const int c = (v < 16 ? 16 : v > 240 ? 240 : v) - 128;
    const int m = (255 * (c < 0 ? -c : c) + 112) / 224;
    const int o = c < 0 ? 128 - m : 128 + m;
    return o < 0 ? 0 : o > 255 ? 255 : o;
}

// magnitude category of a DC difference or an AC level: the number of bits of |v| (0 for 0)
JPEG_HD int jpeg_category(int v) {
    uint32_t a = static_cast<uint32_t>(v < 0 ? -v : v);
    int s = 0;
    while (a) s++, a >>= 1;
    return s;
}

// ---- Annex K.3.3: BITS (codes per length 1 .. 16) and HUFFVAL of the four tables; table = 2 * ac + chroma.  Host side only (the device gets the codes)
static inline const uint8_t *jpeg_huff_bits(int ac, int chroma) {
    static const uint8_t bits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                        {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                        {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    return bits[2 * ac + chroma];
}
static inline const uint8_t *jpeg_huff_vals(int ac, int chroma, int *n) {
    static const uint8_t dc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac0[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
        0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
        0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
        0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
        0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
        0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    static const uint8_t ac1[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
        0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
        0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
        0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
        0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    *n = ac ? 162 : 12;
    return ac ? (chroma ? ac1 : ac0) : dc;
}
// the codes of a table by symbol (Annex C.2): out[symbol] = length << 16 | code; symbols without a code stay 0
static inline void jpeg_huff_codes(int ac, int chroma, uint32_t *out, int n_out) {
    int n;
    const uint8_t *bits = jpeg_huff_bits(ac, chroma), *vals = jpeg_huff_vals(ac, chroma, &n);
    for (int i = 0; i < n_out; i++) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++, code <<= 1)
        for (int i = 0; i < bits[len - 1]; i++, k++, code++) out[vals[k]] = static_cast<uint32_t>(len) << 16 | code;
}
