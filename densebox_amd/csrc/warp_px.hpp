// The perspective arithmetic the rectification kernels (post_ops.hip) and the geometric patch augmentation (warp_aug_ops.hip) share:
// cv2's PUBLISHED getPerspectiveTransform / warpPerspective algorithm (imgwarp.cpp), for device and host alike.  Every includer
// compiles with fp contraction off (the pragma below holds for the rest of the translation unit), so all of them do the same operations
// in the same order and round the same way.
#pragma once
#pragma clang fp contract(off)
#include <cmath>
#include <cstddef>

// The 8x8 solve of cv2.getPerspectiveTransform on double corner values: false where a pivot fails the test.  One function for the host
// entry point and the crop kernel, so both do the same operations in the same order.  Every index is a loop counter (the pivot row is
// found by comparing the counter with piv), so the device copy keeps A in registers once the loops are unrolled.
__host__ __device__ static inline bool perspective_solve(const double* s, const double* d, double* m9) {
    double A[8][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double sx = s[2 * i], sy = s[2 * i + 1], dx = d[2 * i], dy = d[2 * i + 1];
        const double r0[9] = {sx, sy, 1, 0, 0, 0, -sx * dx, -sy * dx, dx};
        const double r1[9] = {0, 0, 0, sx, sy, 1, -sx * dy, -sy * dy, dy};
#pragma unroll
        for (int j = 0; j < 9; ++j) { A[i][j] = r0[j]; A[i + 4][j] = r1[j]; }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {                      // Gaussian elimination, partial pivoting (DECOMP_LU)
        int piv = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double v = fabs(A[r][c]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > 2.220446049250313e-16)) return false;
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            if (r == piv) {
#pragma unroll
                for (int j = 0; j < 9; ++j) { const double t = A[c][j]; A[c][j] = A[r][j]; A[r][j] = t; }
            }
        }
        const double dd = -1.0 / A[c][c];
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] * dd;
#pragma unroll
            for (int j = c + 1; j < 9; ++j) A[r][j] += f * A[c][j];
        }
    }
    double x[8];
#pragma unroll
    for (int r = 7; r >= 0; --r) {
        double acc = A[r][8];
#pragma unroll
        for (int j = r + 1; j < 8; ++j) acc -= A[r][j] * x[j];
        x[r] = acc / A[r][r];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) m9[i] = x[i];
    m9[8] = 1.0;
    return true;
}

// One output pixel of the warp at canvas coordinate (x, y): the inverse map in fp64, the source coordinate rounded to 1/32 pixel,
// 15-bit bilinear weights; channel ch of the result in byte ch.  BORDER 0: a neighbour outside the source contributes byte ch of `fill`
// (cv2's BORDER_CONSTANT); BORDER 1: the neighbour coordinates are clamped into the source (BORDER_REPLICATE).  Whatever `im` holds, no
// read leaves the sh x sw source: a tap is read only after its bounds test (BORDER 0) or its clamp (BORDER 1).
template <int BORDER, typename SrcPtr>
__host__ __device__ __forceinline__ unsigned int warp_px_u8_border(const double* im, SrcPtr src, int sh, int sw, int c, int x, int y,
                                                                   unsigned int fill) {
    const double X0 = im[0] * x + im[1] * y + im[2], Y0 = im[3] * x + im[4] * y + im[5];
    double W = im[6] * x + im[7] * y + im[8];
    W = W != 0.0 ? 32.0 / W : 0.0;
    const double fX = fmax(-2147483648.0, fmin(2147483647.0, X0 * W)), fY = fmax(-2147483648.0, fmin(2147483647.0, Y0 * W));
    const int X = (int)rint(fX), Y = (int)rint(fY);                          // cvRound: nearest, ties to even
    const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    unsigned int px = 0;
    if (BORDER == 0) {
        const bool x0 = sx >= 0 && sx < sw, x1 = sx + 1 >= 0 && sx + 1 < sw, y0 = sy >= 0 && sy < sh, y1 = sy + 1 >= 0 && sy + 1 < sh;
        for (int ch = 0; ch < c; ++ch) {
            const int f = (int)((fill >> (8 * ch)) & 255u);
            const int p00 = (x0 && y0) ? src[((size_t)sy * sw + sx) * c + ch] : f;
            const int p01 = (x1 && y0) ? src[((size_t)sy * sw + sx + 1) * c + ch] : f;
            const int p10 = (x0 && y1) ? src[((size_t)(sy + 1) * sw + sx) * c + ch] : f;
            const int p11 = (x1 && y1) ? src[((size_t)(sy + 1) * sw + sx + 1) * c + ch] : f;
            const int v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
            px |= (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * ch);
        }
    } else {
        const int cx0 = sx < 0 ? 0 : (sx > sw - 1 ? sw - 1 : sx), cx1 = sx + 1 < 0 ? 0 : (sx + 1 > sw - 1 ? sw - 1 : sx + 1);
        const int cy0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy), cy1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        for (int ch = 0; ch < c; ++ch) {
            const int p00 = src[((size_t)cy0 * sw + cx0) * c + ch], p01 = src[((size_t)cy0 * sw + cx1) * c + ch];
            const int p10 = src[((size_t)cy1 * sw + cx0) * c + ch], p11 = src[((size_t)cy1 * sw + cx1) * c + ch];
            const int v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
            px |= (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * ch);
        }
    }
    return px;
}

// The zero border of the rectification kernels: both of them call it, so the batched one writes what the single-image one writes, bit
// for bit.
template <typename SrcPtr>
__host__ __device__ __forceinline__ unsigned int warp_px_u8(const double* im, SrcPtr src, int sh, int sw, int c, int x, int y) {
    return warp_px_u8_border<0>(im, src, sh, sw, c, x, y, 0u);
}

// dst -> src map: the inverse of the 3x3 src -> dst map m, cofactor form in double.  False when the determinant is zero.
__host__ __device__ static inline bool warp_inverse(const double* m, double* im) {
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (det == 0.0) return false;
    const double d = 1.0 / det;
    im[0] = (m[4] * m[8] - m[5] * m[7]) * d; im[1] = (m[2] * m[7] - m[1] * m[8]) * d; im[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    im[3] = (m[5] * m[6] - m[3] * m[8]) * d; im[4] = (m[0] * m[8] - m[2] * m[6]) * d; im[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    im[6] = (m[3] * m[7] - m[4] * m[6]) * d; im[7] = (m[1] * m[6] - m[0] * m[7]) * d; im[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    return true;
}
