// The geometry of zones (zone_ops.hip), compiled for the device and the host alike: the anchor of a box, the side of a directed line, the
// crossing of a line by a move and the even-odd point-in-polygon test, as include/densebox_hip.h states them.  Coordinates are quarter
// pixels in int32, every product is int64; the anchor is float64 with one IEEE operation per written operation, so the file that includes
// this header turns floating-point contraction off first.
#pragma once
#include <cmath>

#define ZONE_COORD_MAX 1048576          // 2^20: the bound on |v| of a configured coordinate, and (exclusive) of a box value with an anchor
#define ZONE_MAX_VERTS 16

struct ZoneAnchor { int ok, x, y; };

__host__ __device__ static inline bool zone_usable(double v) { return fabs(v) < 1048576.0; }      // false for NaN and the infinities

// kind 0: the centre; kind 1: the middle of the bottom edge.  |x|, |y| < 2^22 + 1.
__host__ __device__ static inline ZoneAnchor zone_anchor(double x1, double y1, double x2, double y2, int kind) {
    ZoneAnchor a;
    a.ok = zone_usable(x1) && zone_usable(y1) && zone_usable(x2) && zone_usable(y2);
    a.x = a.y = 0;
    if (a.ok) {
        a.x = (int)floor((x1 + x2) * 2.0 + 0.5);
        a.y = kind == 0 ? (int)floor((y1 + y2) * 2.0 + 0.5) : (int)floor(y2 * 4.0 + 0.5);
    }
    return a;
}

__host__ __device__ static inline long long zone_cross(long long ux, long long uy, long long vx, long long vy) { return ux * vy - uy * vx; }

// side(P) of the line A -> B: cross(B - A, P - A) >= 0
__host__ __device__ static inline bool zone_side(int ax, int ay, int bx, int by, int px, int py) {
    return zone_cross((long long)bx - ax, (long long)by - ay, (long long)px - ax, (long long)py - ay) >= 0;
}

// The move P0 -> P1 against the line A -> B: -1 no crossing, 0 forward (side false -> true), 1 backward.
__host__ __device__ static inline int zone_crossing(int ax, int ay, int bx, int by, int x0, int y0, int x1, int y1) {
    const bool s0 = zone_side(ax, ay, bx, by, x0, y0), s1 = zone_side(ax, ay, bx, by, x1, y1);
    if (s0 == s1) return -1;
    const long long mx = (long long)x1 - x0, my = (long long)y1 - y0;
    const bool ta = zone_cross(mx, my, (long long)ax - x0, (long long)ay - y0) >= 0;
    const bool tb = zone_cross(mx, my, (long long)bx - x0, (long long)by - y0) >= 0;
    if (ta == tb) return -1;
    return s1 ? 0 : 1;
}

// Even-odd rule over the n <= 16 vertices xy[0..2n-1] (x, y interleaved), edge i -> i + 1 (mod n), half-open in y.
__host__ __device__ static inline bool zone_inside(const int* xy, int n, int px, int py) {
    n = n < 0 ? 0 : (n > ZONE_MAX_VERTS ? ZONE_MAX_VERTS : n);
    int odd = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const long long xi = xy[2 * i], yi = xy[2 * i + 1], xj = xy[2 * j], yj = xy[2 * j + 1];
        if ((yi > py) == (yj > py)) continue;
        const long long d = yj - yi, l = (px - xi) * d, r = (xj - xi) * (py - yi);
        odd ^= d > 0 ? l < r : l > r;
    }
    return odd != 0;
}
