// The tile body of the batched bicubic resize, shared by resize_cubic_batch_u8_kernel (resize_ops.hip), patch_cut_kernel
// (patch_ops.hip) and resize_cubic_batch_nv12_kernel (color_ops.hip): all run THIS code on a device job record, so a patch is bit for
// bit the resize of its window and the resize of an NV12 surface bit for bit the resize of its converted frame.  The including file
// turns floating-point contraction off (the coefficient arithmetic must give the bits NumPy gives).
#pragma once
#include "common.hpp"

#define RSZ_THREADS 256
#define RSZ_TW 64
#define RSZ_TH 16
#define RSZ_COEF_BITS 11
typedef const __attribute__((address_space(1))) unsigned char* rsz_gsrc_t;
typedef __attribute__((address_space(1))) unsigned char* rsz_gdst_t;
typedef __attribute__((address_space(1))) u32x4* rsz_gdst4_t;
typedef __attribute__((address_space(1))) unsigned int* rsz_gdst1_t;

struct ResizeJobDev {                   // device record of one job (96 bytes)
    const unsigned char* src;
    unsigned char* dst;                 // dst + dst_off
    double scale_x, scale_y;            // vw / dw, vh / dh
    int row_bytes;                      // sw * c
    int cx0, cy0, cw, ch, pad_l, pad_t, vw, vh, dh, dw, pad_value, tiles_x, pad[3];    // pad: free for the writer of the record (dbx_patch_plan: frame, kind, 0)
};
static_assert(sizeof(ResizeJobDev) == 96, "ResizeJobDev layout");

// Destination index d of an axis with vn virtual source samples: coefficients a[0..3] of the taps s-1 .. s+2 and, per tap, the byte
// offset of its sample along that axis (index clamped to [0, vn - 1], then moved into the crop: c0 + index - pad0, times stride) or
// -1 when the clamped index lies in the padding.
__device__ __forceinline__ void cubic_taps(int d, double scale, int vn, int pad0, int cn, int c0, int stride, short* a, int* off) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    const float A = -0.75f;
    float c[4];
    c[0] = ((A * (f + 1.0f) - 5.0f * A) * (f + 1.0f) + 8.0f * A) * (f + 1.0f) - 4.0f * A;
    c[1] = ((A + 2.0f) * f - (A + 3.0f)) * f * f + 1.0f;
    c[2] = ((A + 2.0f) * (1.0f - f) - (A + 3.0f)) * (1.0f - f) * (1.0f - f) + 1.0f;
    c[3] = 1.0f - c[0] - c[1] - c[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = (int)rintf(c[k] * (float)(1 << RSZ_COEF_BITS));             // nearest, ties to even; no sum correction
        a[k] = (short)(q < -32768 ? -32768 : (q > 32767 ? 32767 : q));
        int v = s - 1 + k;
        v = (v < 0 ? 0 : (v > vn - 1 ? vn - 1 : v)) - pad0;
        off[k] = (v < 0 || v >= cn) ? -1 : (c0 + v) * stride;
    }
}

// nb bytes of one tile row from LDS to global memory at g, by lanes q of 16: L holds byte b of the row at L[shift + b], shift = g & 15,
// so that the row's aligned 16-byte words are stored as such; a word that is only partly inside the row (at most the first and the
// last) falls back to its whole dwords, then to bytes, so no byte outside [g, g + nb) is written.
__device__ __forceinline__ void rsz_store_row(rsz_gdst_t g, const unsigned char* L, int nb, int q16) {
    const int shift = (int)((size_t)g & 15), end = shift + nb;
    const rsz_gdst_t gw = g - shift;                   // 16-byte aligned; byte b of the row is gw[shift + b] = L[shift + b]
    for (int k = q16; 16 * k < end; k += 16) {
        const int b0 = 16 * k;
        if (b0 >= shift && b0 + 16 <= end) {
            reinterpret_cast<rsz_gdst4_t>(gw)[k] = reinterpret_cast<const u32x4*>(L)[k];
        } else {
            for (int j = b0; j < b0 + 16; j += 4) {
                if (j >= shift && j + 4 <= end) {
                    reinterpret_cast<rsz_gdst1_t>(gw)[j >> 2] = reinterpret_cast<const unsigned int*>(L)[j >> 2];
                } else {
                    for (int q = j < shift ? shift : j; q < j + 4 && q < end; ++q) gw[q] = L[q];
                }
            }
        }
    }
}

// One RSZ_TH x RSZ_TW tile at (x0, y0) of job J's destination, written behind `dst_base` (the job's [dh][dw][C] block).  All
// RSZ_THREADS threads of the workgroup call it.
//   1. Tables: the first RSZ_TW threads make the four 16-bit coefficients and the four source byte offsets (or -1: padding) of
//      their column, the next RSZ_TH threads those of their row -- once per tile, in LDS, not per pixel or per channel.
//   2. Pixels: the 64 lanes of a wave make 64 CONSECUTIVE pixels of one destination row, so the byte gathers of one load
//      instruction lie in one source row within a span of 64 * scale_x pixels; each wave makes RSZ_TH / 4 rows.  The column table
//      sits in registers for all rows, the row table is a wave-uniform LDS read.  The bytes go to LDS, each tile row placed at the
//      offset its global address has inside a 16-byte word.
//   3. Stores: 16 lanes per tile row store the row's aligned 16-byte words; a word that is only partly inside the row (at most
//      the first and the last) falls back to its whole dwords, then to bytes, so no byte outside the job's block is written.
// Source and destination go through global-address-space pointers (global_load / global_store, not flat).
// The taps come from a SOURCE POLICY `src`: C, the channel count; col_stride() / row_stride(), what one step along an axis adds to a
// tap's offset; fetch(yo, xo, px), the C values of the tap at row offset yo and column offset xo, made ONCE per tap.  RszSrcU8 is the
// interleaved uint8 image the resize and the patch cutter read; color_ops.hip adds the NV12 surface, whose fetch converts the tap.
template <int C_> struct RszSrcU8 {
    static constexpr int C = C_;
    rsz_gsrc_t src;
    int row_bytes;
    __device__ __forceinline__ RszSrcU8(const ResizeJobDev* J) : src((rsz_gsrc_t)J->src), row_bytes(J->row_bytes) {}
    __device__ __forceinline__ int col_stride() const { return C; }
    __device__ __forceinline__ int row_stride() const { return row_bytes; }
    __device__ __forceinline__ void fetch(int yo, int xo, int* px) const {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) px[ch] = (int)src[yo + xo + ch];
    }
};

template <class Src>
__device__ __forceinline__ void resize_tile_body(const ResizeJobDev* __restrict__ J, unsigned char* dst_base, int x0, int y0, const Src src) {
    constexpr int C = Src::C;
    constexpr int ROW = RSZ_TW * C + 16;               // a tile row in LDS: its bytes after a shift of 0..15
    __shared__ __attribute__((aligned(16))) unsigned char stage[RSZ_TH][ROW];
    __shared__ short col_a[RSZ_TW][4], row_a[RSZ_TH][4];
    __shared__ int col_o[RSZ_TW][4], row_o[RSZ_TH][4];
    const int tid = threadIdx.x;
    const int dh = J->dh, dw = J->dw;
    if (tid < RSZ_TW) {
        const int x = x0 + tid < dw ? x0 + tid : dw - 1;
        cubic_taps(x, J->scale_x, J->vw, J->pad_l, J->cw, J->cx0, src.col_stride(), col_a[tid], col_o[tid]);
    } else if (tid < RSZ_TW + RSZ_TH) {
        const int r = tid - RSZ_TW, y = y0 + r < dh ? y0 + r : dh - 1;
        cubic_taps(y, J->scale_y, J->vh, J->pad_t, J->ch, J->cy0, src.row_stride(), row_a[r], row_o[r]);
    }
    __syncthreads();
    const rsz_gdst_t dst = (rsz_gdst_t)dst_base;
    {
        const int lane = tid & 63, wave = tid >> 6, x = x0 + lane;
        const int pv = J->pad_value;
        int a[4], xo[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = col_a[lane][k]; xo[k] = col_o[lane][k]; }
#pragma unroll
        for (int i = 0; i < RSZ_TH / 4; ++i) {
            const int r = wave * (RSZ_TH / 4) + i, y = y0 + r;
            if (y >= dh || x >= dw) continue;
            // |acc| <= 255 * (1.375 * 2048)^2 = 2.02e9 < 2^31: 1.375 is the largest absolute coefficient sum (at f = 0.5), and the
            // same bound holds for every partial sum, so 32 bits hold in any order of summation.
            int acc[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] = 0;
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const int b = row_a[r][ky], yo = row_o[r][ky];
                int h[C];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) h[ch] = 0;
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    int px[C];
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) px[ch] = pv;
                    if ((xo[kx] | yo) >= 0) src.fetch(yo, xo[kx], px);
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) h[ch] += a[kx] * px[ch];
                }
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[ch] += b * h[ch];
            }
            const int shift = (int)((size_t)(dst + ((long long)y * dw + x0) * C) & 15);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const int v = (acc[ch] + (1 << (2 * RSZ_COEF_BITS - 1))) >> (2 * RSZ_COEF_BITS);       // arithmetic shift
                stage[r][shift + lane * C + ch] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
    }
    __syncthreads();
    const int r = tid >> 4, y = y0 + r;
    if (y >= dh) return;
    const int nb = (dw - x0 < RSZ_TW ? dw - x0 : RSZ_TW) * C;
    rsz_store_row(dst + ((long long)y * dw + x0) * C, stage[r], nb, tid & 15);
}
