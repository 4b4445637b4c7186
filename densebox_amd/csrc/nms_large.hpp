// The greedy NMS for up to 4096 rows as device functions: the order by a bitonic sort of (score key, row) pairs, the suppression matrix
// by many workgroups, the greedy walk by one wave.  Shared by post_ops.hip (dbx_detect_thresh_batch, dbx_nms_large,
// dbx_merge_nms_thresh_batch) and tile_ops.hip (dbx_tile_nms_batch), so order, ties, the +1 pixel IoU and the NaN handling cannot drift
// apart.  Both files compile with `#pragma clang fp contract(off)`: `areas[i] + areas[j] - w*h` rounds the product before the
// subtraction, as NumPy does.
#pragma once
#include "common.hpp"

#define DET_THREADS 1024
#define THR_MAX_DETS 4096
#define NMSL_THREADS 256

static __host__ __device__ inline long long thr_up256(long long v) { return (v + 255) / 256 * 256; }

// Rows [64 rb, 64 rb + 64) (in NMS order: position p is row order[p] of dets) of the n x nw suppression matrix, the words at or right of
// the diagonal: bit q of row p (q > p) = box p suppresses box q, nms_block's expression.  Words left of the diagonal are never written
// and never read.  NMSL_THREADS threads: lane = row, the four waves share the words; a wave stages the 64 column boxes of its word
// in LDS (10 KB in all) and every lane reads them back as broadcasts.
__device__ __forceinline__ void nmsl_mask_rows(const double* dets, int dc, const int* order, int n, double thresh,
                                               unsigned long long* mask, int nw_stride, int rb) {
    __shared__ double cb[NMSL_THREADS / 64][5][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = rb * 64 + lane, nw = (n + 63) >> 6;
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0, ai = 0;
    if (p < n) {
        const double* d = dets + (size_t)order[p] * dc;
        x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3];
        ai = (x2 - x1 + 1) * (y2 - y1 + 1);
    }
    for (int w0 = rb; w0 < nw; w0 += NMSL_THREADS / 64) {            // (uniform trip count: the barriers are reached by every wave)
        const int w = w0 + wv, q0 = 64 * w + lane;
        if (q0 < n) {
            const double* d = dets + (size_t)order[q0] * dc;
            const double u1 = d[0], v1 = d[1], u2 = d[2], v2 = d[3];
            cb[wv][0][lane] = u1; cb[wv][1][lane] = v1; cb[wv][2][lane] = u2; cb[wv][3][lane] = v2;
            cb[wv][4][lane] = (u2 - u1 + 1) * (v2 - v1 + 1);
        }
        __syncthreads();
        if (w < nw && p < n) {
            unsigned long long bits = 0ull;
            const int cn = min(64, n - 64 * w);
            for (int c = 0; c < cn; ++c) {
                if (64 * w + c <= p) continue;
                const double xx1 = fmax(x1, cb[wv][0][c]), yy1 = fmax(y1, cb[wv][1][c]), xx2 = fmin(x2, cb[wv][2][c]), yy2 = fmin(y2, cb[wv][3][c]);
                const double ww = fmax(0.0, xx2 - xx1 + 1), hh = fmax(0.0, yy2 - yy1 + 1);
                const double inter = ww * hh;
                const double ovr = inter / (ai + cb[wv][4][c] - inter);
                if (!(ovr <= thresh)) bits |= 1ull << c;             // NaN is dropped, like np.where(ovr <= t)
            }
            mask[(size_t)p * nw_stride + w] = bits;
        }
        __syncthreads();
    }
}

// The greedy walk by ONE wave: lane w holds word w of the removed set, the matrix rows come in blocks of 32 with the next block's loads
// in flight while this one is walked.  keep[0] = count, keep[1..] = kept rows in NMS order.
__device__ __forceinline__ void nmsl_sweep(const unsigned long long* mask, int nw_stride, const int* order, int n, int* keep) {
    const int lane = threadIdx.x & 63, nw = (n + 63) >> 6;
    unsigned long long removed = 0ull, cur[32], nxt[32];
    int cnt = 0, ord_c = 0, ord_n = 0;
#pragma unroll
    for (int r = 0; r < 32; ++r) cur[r] = (lane < nw && r < n) ? mask[(size_t)r * nw_stride + lane] : 0ull;
    if (lane < 32 && lane < n) ord_c = order[lane];
    for (int p0 = 0; p0 < n; p0 += 32) {
        const int p1 = p0 + 32;
#pragma unroll
        for (int r = 0; r < 32; ++r) nxt[r] = (lane < nw && lane >= (p1 >> 6) && p1 + r < n) ? mask[(size_t)(p1 + r) * nw_stride + lane] : 0ull;
        ord_n = (lane < 32 && p1 + lane < n) ? order[p1 + lane] : 0;
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int pos = p0 + r;
            if (pos < n) {
                const unsigned long long word = __shfl(removed, pos >> 6);
                if (!((word >> (pos & 63)) & 1ull)) {              // (uniform) box `pos` survives
                    const int row = __shfl(ord_c, r);
                    if (lane == 0) keep[1 + cnt] = row;
                    ++cnt;
                    removed |= cur[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 32; ++r) cur[r] = nxt[r];
        ord_c = ord_n;
    }
    if (lane == 0) keep[0] = cnt;
}

// The order comes from a bitonic sort of (score key, row) pairs in LDS (48 KB): key = the float64 score's bits made order-preserving,
// -0 == +0, every NaN the largest; larger key first, the higher row first among equal keys -- nms_block's rank for every input.
__device__ __forceinline__ unsigned long long nmsl_score_key(double sc) {
    if (sc != sc) return ~0ull;
    if (sc == 0.0) return 0x8000000000000000ull;
    const unsigned long long u = (unsigned long long)__double_as_longlong(sc);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
// bitonic sort of the (key, row) pairs [0, P2) in LDS by a DET_THREADS-wide workgroup into that order (a barrier in front is the caller's)
__device__ __forceinline__ void nmsl_sort_pairs(unsigned long long* key, int* row, int P2) {
    for (int size = 2; size <= P2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P2 >> 1); t += DET_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const unsigned long long x = key[i], y = key[j];
                const int ri = row[i], rj = row[j];
                const bool i_less = x < y || (x == y && ri < rj);
                if (((i & size) == 0) == i_less) { key[i] = y; key[j] = x; row[i] = rj; row[j] = ri; }
            }
            __syncthreads();
        }
}
