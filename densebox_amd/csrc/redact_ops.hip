// Plate redaction behind the decode and the tracking update: the frame with every kept row's plate -- and every coasting track's
// predicted box, for the frames in which the detector missed it -- filled, pixelated or blurred by ONE launch (dbx_redact_batch).  No
// reference counterpart; include/densebox_hip.h states the semantics, tests/redact_ref.py restates them in NumPy.  All arithmetic is
// integer behind one float64 add per coordinate.  The region build, the coverage test and the value rules are __host__ __device__
// functions, and dbx_redact_host applies them to one frame on the CPU.
#include <vector>

#include "common.hpp"
#include "det_frame.hpp"
#include "frame_tile.hpp"

#define RED_TW 64                    // a tile: 64 x 16 pixels, 4 per thread; the copy moves a row segment with 16 lanes
#define RED_TH 16
#define RED_MAX_SLOTS 1024
#define RED_MAX_TRACKS 256
#define RED_MAX_CELL 32
#define RED_MAX_RADIUS 16

static_assert(sizeof(dbx_redact_style) == 40 && offsetof(dbx_redact_style, method) == 4 && offsetof(dbx_redact_style, coast) == 28 &&
              offsetof(dbx_redact_style, min_score) == 32, "dbx_redact_style is 40 bytes");

// ---------------------------------------------------------------------------------------------------------------- regions
// A region as the pixels test it: 52 bytes of LDS.  x0..y1: the box region, or the quad's bounding rectangle, clipped to the frame
// (never empty); g: the quad's G_0..G_3 in quarter pixels (x, y interleaved); quad: 1 when g counts.
struct RedEnt { int x0, x1, y0, y1; int g[8]; int quad; };

__host__ __device__ static inline bool red_landmark(double v) { return fabs(v) < 1048576.0; }     // |v| < 2^20: false for NaN and the infinities
__host__ __device__ static inline long long red_sgn(long long v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }

// The box region of (x1, y1, x2, y2) = bx[0..3] on an h x w frame; false when a value is not usable or nothing of it is in the frame.
__host__ __device__ static inline bool red_box(const double* bx, const dbx_redact_style& st, int h, int w, RedEnt& e) {
    const double v0 = bx[0], v1 = bx[1], v2 = bx[2], v3 = bx[3];
    if (!(tile_usable(v0) && tile_usable(v1) && tile_usable(v2) && tile_usable(v3))) return false;
    const long long X1 = (int)(v0 + 0.5), Y1 = (int)(v1 + 0.5), X2 = (int)(v2 + 0.5), Y2 = (int)(v3 + 0.5);
    const long long L = tile_min(X1, X2), R = tile_max(X1, X2), Tp = tile_min(Y1, Y2), Bt = tile_max(Y1, Y2);
    const long long gx = st.grow + ((R - L + 1) * st.grow_pct) / 100, gy = st.grow + ((Bt - Tp + 1) * st.grow_pct) / 100;
    const long long xa = tile_max(L - gx, 0ll), xb = tile_min(R + gx, (long long)w - 1);
    const long long ya = tile_max(Tp - gy, 0ll), yb = tile_min(Bt + gy, (long long)h - 1);
    if (xa > xb || ya > yb) return false;
    e.x0 = (int)xa; e.x1 = (int)xb; e.y0 = (int)ya; e.y1 = (int)yb;
#pragma unroll
    for (int q = 0; q < 8; ++q) e.g[q] = 0;
    e.quad = 0;
    return true;
}

// The quad region of the landmarks lm[0..7]: 0 when the row falls back to its box, 1 when e holds the region, -1 when the quad's
// bounding rectangle misses the frame.
__host__ __device__ static inline int red_quad(const double* lm, const dbx_redact_style& st, int h, int w, RedEnt& e) {
    long long px[4], py[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double vx = lm[2 * q], vy = lm[2 * q + 1];
        if (!red_landmark(vx) || !red_landmark(vy)) return 0;
        px[q] = (int)(vx + 0.5); py[q] = (int)(vy + 0.5);
    }
    long long shoelace = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) shoelace += px[q] * py[(q + 1) & 3] - px[(q + 1) & 3] * py[q];
    if (shoelace == 0) return 0;
    const long long sx = px[0] + px[1] + px[2] + px[3], sy = py[0] + py[1] + py[2] + py[3];
    long long xlo = 0, xhi = 0, ylo = 0, yhi = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long dx = 4 * px[q] - sx, dy = 4 * py[q] - sy;
        const long long gx = 4 * px[q] + (dx * st.grow_pct) / 100 + 4 * st.grow * red_sgn(dx);
        const long long gy = 4 * py[q] + (dy * st.grow_pct) / 100 + 4 * st.grow * red_sgn(dy);
        e.g[2 * q] = (int)gx; e.g[2 * q + 1] = (int)gy;                 // |G| < 2^24
        xlo = q ? tile_min(xlo, gx) : gx; xhi = q ? tile_max(xhi, gx) : gx;
        ylo = q ? tile_min(ylo, gy) : gy; yhi = q ? tile_max(yhi, gy) : gy;
    }
    // a covered pixel has xlo <= 4x <= xhi: floor(xlo / 4) <= x <= floor(xhi / 4)
    const long long xa = tile_max(xlo >> 2, 0ll), xb = tile_min(xhi >> 2, (long long)w - 1);
    const long long ya = tile_max(ylo >> 2, 0ll), yb = tile_min(yhi >> 2, (long long)h - 1);
    if (xa > xb || ya > yb) return -1;
    e.x0 = (int)xa; e.x1 = (int)xb; e.y0 = (int)ya; e.y1 = (int)yb;
    e.quad = 1;
    return 1;
}

// The region of a decoded row d of det_cols columns; false when it has none in the frame.
__host__ __device__ static inline bool red_row_region(const double* d, int det_cols, const dbx_redact_style& st, int h, int w, RedEnt& e) {
    if (d[4] < st.min_score) return false;                             // (a NaN score is redacted)
    if (!(tile_usable(d[0]) && tile_usable(d[1]) && tile_usable(d[2]) && tile_usable(d[3]))) return false;
    if (st.shape == 1 && det_cols == 13) {
        const int q = red_quad(d + 5, st, h, w, e);
        if (q) return q > 0;
    }
    return red_box(d, st, h, w, e);
}

// The region of track slot t: a coasting track's box.  id and age are data, never indices.
__host__ __device__ static inline bool red_track_region(const dbx_track* t, const dbx_redact_style& st, int h, int w, RedEnt& e) {
    const int id = t->id, age = t->age;
    if (id < 0 || age < 1 || age > st.coast) return false;
    return red_box(t->box, st, h, w, e);
}

// Whether the point (X, Y), in quarter pixels, is inside the triangle G_i G_j G_k of g.
__host__ __device__ static inline bool red_tri(const int* g, int i, int j, int k, long long X, long long Y) {
    const long long ax = g[2 * i], ay = g[2 * i + 1], bx = g[2 * j], by = g[2 * j + 1], cx = g[2 * k], cy = g[2 * k + 1];
    const long long area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    if (area2 == 0) return false;
    const long long s = area2 > 0 ? 1 : -1;
    const long long e0 = (bx - ax) * (Y - ay) - (by - ay) * (X - ax);
    const long long e1 = (cx - bx) * (Y - by) - (cy - by) * (X - bx);
    const long long e2 = (ax - cx) * (Y - cy) - (ay - cy) * (X - cx);
    return s * e0 >= 0 && s * e1 >= 0 && s * e2 >= 0;
}

__host__ __device__ static inline bool red_covers(const RedEnt& e, int x, int y) {
    if (x < e.x0 || x > e.x1 || y < e.y0 || y > e.y1) return false;
    if (!e.quad) return true;
    const long long X = 4ll * x, Y = 4ll * y;
    return red_tri(e.g, 0, 1, 2, X, Y) || red_tri(e.g, 0, 2, 3, X, Y);
}

// ---------------------------------------------------------------------------------------------------------------- values
__host__ __device__ static inline int red_round_div(int sum, int n) { return (sum + n / 2) / n; }
__host__ __device__ static inline int red_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the cell [a, b) of coordinate v on an axis of `lim` pixels
__host__ __device__ static inline void red_cell(int s, int v, int lim, int& a, int& b) {
    a = s * (v / s);
    b = (int)tile_min((long long)a + s, (long long)lim);
}

// pixelate and blur straight from the image (the kernel stages the same sums in LDS)
__host__ __device__ static inline int red_pixelate_px(const uint8_t* src, int h, int w, int c, int s, int x, int y, int ch) {
    int xa, xb, ya, yb, sum = 0;
    red_cell(s, x, w, xa, xb);
    red_cell(s, y, h, ya, yb);
    for (int yy = ya; yy < yb; ++yy)
        for (int xx = xa; xx < xb; ++xx) sum += src[((size_t)yy * w + xx) * c + ch];
    return red_round_div(sum, (xb - xa) * (yb - ya));
}
__host__ __device__ static inline int red_blur_px(const uint8_t* src, int h, int w, int c, int r, int x, int y, int ch) {
    int sum = 0;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) sum += src[((size_t)red_clamp(y + dy, 0, h - 1) * w + red_clamp(x + dx, 0, w - 1)) * c + ch];
    return red_round_div(sum, (2 * r + 1) * (2 * r + 1));
}

// ---------------------------------------------------------------------------------------------------------------- LDS sizes
static size_t red_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t red_list_bytes(int cap) { return red_up16((size_t)cap * sizeof(RedEnt)); }
__host__ __device__ static inline size_t red_halo_bytes(int r, int c) {
    return (((size_t)(RED_TW + 2 * r) * (RED_TH + 2 * r) * c) + 15) & ~(size_t)15;
}
static size_t red_work_bytes(const dbx_redact_style& st, int c) {
    if (st.method == 1) return red_up16((size_t)((RED_TW - 1) / st.cell + 2) * ((RED_TH - 1) / st.cell + 2) * 4);
    if (st.method == 2) return red_halo_bytes(st.radius, c) + red_up16((size_t)(RED_TH + 2 * st.radius) * RED_TW * c * 2);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the kernel
struct RedArgs {
    const dbx_overlay_frame* frames; const double* dets; const int* keep; const int* prefix; const dbx_track* tracks;
    long long det_rows;
    dbx_redact_style st;
    int c, det_cols, slots, stream0, max_tracks, cap, tiles_x, max_h, max_w;
    unsigned list_bytes;
};

// One workgroup per 64 x 16 tile of a frame (grid: the tiles of a max_h x max_w frame, batch), walked as frame_tile.hpp says.  The
// candidates are the frame's kept rows, then the stream's track slots, and their regions are a union: the list's order does not
// matter.  For a tile that some region meets, the tile's cell means (pixelate) or its halo and horizontal window sums (blur) are staged
// in LDS from src, and every pixel takes its value when a region covers it and src's otherwise.
__global__ __launch_bounds__(TILE_THREADS) void redact_batch_kernel(const RedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char red_sm[];
    RedEnt* list = (RedEnt*)red_sm;
    unsigned char* work = red_sm + a.list_bytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, c = a.c, method = a.st.method;
    FrameTile t;
    if (!tile_open<RED_TW, RED_TH>(a.frames, a.tiles_x, a.max_h, a.max_w, t)) return;              // uniform, as every return below
    const dbx_overlay_frame fm = t.fm;
    if (method != 0 && fm.dst == fm.src) return;
    const int x0 = t.x0, y0 = t.y0, rows = t.rows, cols = t.cols;

    const DetFrame fr = det_frame(a.keep, a.prefix, b, a.slots, a.det_rows);
    const bool coasting = a.tracks && a.st.coast > 0;
    const dbx_track* tr = coasting ? a.tracks + (size_t)(a.stream0 + b) * a.max_tracks : nullptr;
    const int total = fr.k + (coasting ? a.max_tracks : 0);            // at most slots + max_tracks = cap
    const int cnt = tile_collect(list, total, [&](int i, RedEnt& e) {
        bool hit = false;
        if (i < fr.k) {
            const int r = fr.kl[1 + i];
            if (r >= 0 && r < fr.n) hit = red_row_region(a.dets + (size_t)(fr.r0 + r) * a.det_cols, a.det_cols, a.st, fm.h, fm.w, e);
        } else {
            hit = red_track_region(tr + (i - fr.k), a.st, fm.h, fm.w, e);
        }
        return hit && tile_meets(t, e.x0, e.x1, e.y0, e.y1);
    });
    if (cnt == 0) {
        tile_copy_through<RED_TW>(t, c);
        return;
    }

    // pixelate: the rounded mean of every cell that meets the tile, channel ch in byte ch of cellv[cell]
    unsigned* cellv = (unsigned*)work;
    const int s = a.st.cell, cx0 = x0 / s, cy0 = y0 / s, ncx = (x0 + cols - 1) / s - cx0 + 1, ncy = (y0 + rows - 1) / s - cy0 + 1;
    // blur: the tile with its halo [rows + 2r][cols + 2r][c] and the horizontal window sums [rows + 2r][cols][c]
    const int r = a.st.radius, hw = cols + 2 * r, hh = rows + 2 * r;
    const unsigned short* hsum = (const unsigned short*)(work + red_halo_bytes(r, c));
    if (method == 1) {
        int G = 1;                                                 // lanes per cell
        while (G < s * s && G < 64) G <<= 1;
        const int per_wave = 64 / G, sub = lane & (G - 1), ncell = ncx * ncy;
        for (int base = wave * per_wave; base < ncell; base += (TILE_THREADS / 64) * per_wave) {     // uniform within a wave
            const int cell = base + lane / G;
            int s0 = 0, s1 = 0, s2 = 0, s3 = 0, n = 1;
            if (cell < ncell) {
                int xa, xb, ya, yb;
                red_cell(s, (cx0 + cell % ncx) * s, fm.w, xa, xb);
                red_cell(s, (cy0 + cell / ncx) * s, fm.h, ya, yb);
                const int cw = xb - xa;
                n = cw * (yb - ya);
                for (int p = sub; p < n; p += G) {
                    const uint8_t* q = fm.src + ((size_t)(ya + p / cw) * fm.w + (xa + p % cw)) * c;
                    s0 += q[0];
                    if (c > 1) s1 += q[1];
                    if (c > 2) s2 += q[2];
                    if (c > 3) s3 += q[3];
                }
            }
            for (int mk = G >> 1; mk; mk >>= 1) {
                s0 += __shfl_xor(s0, mk); s1 += __shfl_xor(s1, mk); s2 += __shfl_xor(s2, mk); s3 += __shfl_xor(s3, mk);
            }
            if (cell < ncell && sub == 0)
                cellv[cell] = (unsigned)red_round_div(s0, n) | (unsigned)red_round_div(s1, n) << 8 | (unsigned)red_round_div(s2, n) << 16 |
                              (unsigned)red_round_div(s3, n) << 24;
        }
        __syncthreads();
    } else if (method == 2) {
        uint8_t* hal = work;
        unsigned short* hs = (unsigned short*)(work + red_halo_bytes(r, c));
        for (int i = tid; i < hw * hh; i += TILE_THREADS) {
            const int ly = i / hw, lx = i - ly * hw;
            const uint8_t* q = fm.src + ((size_t)red_clamp(y0 + ly - r, 0, fm.h - 1) * fm.w + red_clamp(x0 + lx - r, 0, fm.w - 1)) * c;
            for (int ch = 0; ch < c; ++ch) hal[(size_t)i * c + ch] = q[ch];
        }
        __syncthreads();
        for (int i = tid; i < hh * cols * c; i += TILE_THREADS) {
            const int ch = i % c, lx = (i / c) % cols, ly = i / (c * cols);
            const uint8_t* q = hal + ((size_t)ly * hw + lx) * c + ch;
            int sum = 0;
            for (int k = 0; k <= 2 * r; ++k) sum += q[k * c];
            hs[i] = (unsigned short)sum;                           // at most 33 * 255
        }
        __syncthreads();
    }

    // The pixels, by a loop of the kernel's own: as a shared skeleton over a lambda the same inner loops came out in another block
    // order, and blur, whose covered pixels cost most, measured 0.8 % slower (profiles/r21_frame_tile.txt).
    unsigned col;                                                  // color[ch] in byte ch
    __builtin_memcpy(&col, a.st.color, 4);
    const int area = (2 * r + 1) * (2 * r + 1);
    const bool copying = fm.dst != fm.src;
    for (int p = tid; p < RED_TW * RED_TH; p += TILE_THREADS) {
        const int lx = p & (RED_TW - 1), ly = p / RED_TW;
        if (lx >= cols || ly >= rows) continue;
        const int x = x0 + lx, y = y0 + ly;
        bool cov = false;
        for (int k = 0; k < cnt && !cov; ++k) cov = red_covers(list[k], x, y);
        const size_t o = ((size_t)y * fm.w + x) * c;
        if (!cov) {
            for (int ch = 0; copying && ch < c; ++ch) fm.dst[o + ch] = fm.src[o + ch];
            continue;
        }
        if (method == 1) col = cellv[(y / s - cy0) * ncx + (x / s - cx0)];
        for (int ch = 0; ch < c; ++ch) {
            int v = (int)(col >> (8 * ch)) & 255;
            if (method == 2) {
                int sum = 0;
                for (int k = 0; k <= 2 * r; ++k) sum += hsum[((size_t)(ly + k) * cols + lx) * c + ch];
                v = red_round_div(sum, area);
            }
            fm.dst[o + ch] = (uint8_t)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- entry points
static int red_style_check(const char* fn, const dbx_redact_style* st) {
    DBX_REQUIRE(st, "%s: null style", fn);
    DBX_REQUIRE(st->method >= 0 && st->method <= 2, "%s: method=%d must be 0 (fill), 1 (pixelate) or 2 (blur)", fn, st->method);
    DBX_REQUIRE(st->shape >= 0 && st->shape <= 1, "%s: shape=%d must be 0 (box) or 1 (quad)", fn, st->shape);
    DBX_REQUIRE(st->cell >= 2 && st->cell <= RED_MAX_CELL, "%s: cell=%d must be 2..%d", fn, st->cell, RED_MAX_CELL);
    DBX_REQUIRE(st->radius >= 1 && st->radius <= RED_MAX_RADIUS, "%s: radius=%d must be 1..%d", fn, st->radius, RED_MAX_RADIUS);
    DBX_REQUIRE(st->grow >= 0 && st->grow <= 64, "%s: grow=%d must be 0..64", fn, st->grow);
    DBX_REQUIRE(st->grow_pct >= 0 && st->grow_pct <= 100, "%s: grow_pct=%d must be 0..100", fn, st->grow_pct);
    DBX_REQUIRE(st->coast >= 0, "%s: coast=%d is negative", fn, st->coast);
    DBX_REQUIRE(st->min_score == st->min_score, "%s: min_score is NaN", fn);
    return DBX_OK;
}

extern "C" int dbx_redact_batch(const dbx_overlay_frame* frames, int32_t batch, int32_t c, int32_t max_h, int32_t max_w, const double* dets,
                                int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix, int32_t slots,
                                const dbx_track* tracks, int32_t streams, int32_t stream0, int32_t max_tracks,
                                const dbx_redact_style* style, void* stream) {
    static_assert(sizeof(dbx_overlay_frame) == 24 && sizeof(dbx_track) == 104, "dbx_overlay_frame is 24 bytes, dbx_track 104");
    static_assert(sizeof(RedEnt) == 52, "a collected region is 52 bytes of LDS");
    const char* fn = "redact_batch";
    int rc = det_rows_check(fn, det_cols, det_rows, prefix, batch, slots, RED_MAX_SLOTS);
    if (rc == DBX_OK) rc = tile_dims_check(fn, c, max_h, max_w);
    if (rc == DBX_OK) rc = red_style_check(fn, style);
    if (rc != DBX_OK) return rc;
    if (tracks) {
        DBX_REQUIRE(stream0 >= 0 && (int64_t)stream0 + batch <= streams, "%s: streams %d..%lld do not fit the %d of the table", fn, stream0,
                    (long long)stream0 + batch - 1, streams);
        DBX_REQUIRE(max_tracks >= 1 && max_tracks <= RED_MAX_TRACKS, "%s: max_tracks=%d must be 1..%d", fn, max_tracks, RED_MAX_TRACKS);
    }
    DBX_REQUIRE(frames && dets && keep, "%s: null argument", fn);
    RedArgs a;
    dim3 grid;
    rc = tile_grid<RED_TW, RED_TH>(fn, max_h, max_w, batch, &grid, &a.tiles_x);
    if (rc != DBX_OK || batch == 0) return rc;
    const bool coasting = tracks && style->coast > 0;
    const int cap = slots + (coasting ? max_tracks : 0);
    const size_t lds = red_list_bytes(cap) + red_work_bytes(*style, c);
    dbx_redact_style worst = *style;
    worst.method = 2; worst.radius = RED_MAX_RADIUS;
    rc = tile_lds_limit<redact_batch_kernel>(lds, red_list_bytes(RED_MAX_SLOTS + RED_MAX_TRACKS) + red_work_bytes(worst, 4));
    if (rc != DBX_OK) return rc;
    a.frames = frames; a.dets = dets; a.keep = keep; a.prefix = prefix; a.tracks = coasting ? tracks : nullptr;
    a.det_rows = det_rows; a.st = *style; a.c = c; a.det_cols = det_cols; a.slots = slots; a.stream0 = stream0; a.max_tracks = max_tracks;
    a.cap = cap; a.max_h = max_h; a.max_w = max_w; a.list_bytes = (unsigned)red_list_bytes(cap);
    hipLaunchKernelGGL(redact_batch_kernel, grid, dim3(TILE_THREADS), lds, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_redact_host(const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t c, const double* rows, int32_t det_cols,
                               int32_t n, const int32_t* keep, int32_t k, const dbx_track* tracks, int32_t ntracks,
                               const dbx_redact_style* style) {
    const char* fn = "redact_host";
    DBX_REQUIRE(det_cols == 5 || det_cols == 13, "%s: det_cols=%d must be 5 or 13", fn, det_cols);
    DBX_REQUIRE(h >= 1 && w >= 1, "%s: a frame of %d x %d pixels is empty", fn, w, h);
    DBX_REQUIRE(n >= 0 && k >= 0, "%s: n=%d and k=%d must not be negative", fn, n, k);
    DBX_REQUIRE(c >= 1 && c <= 4, "%s: c=%d must be 1..4", fn, c);
    const int rc = red_style_check(fn, style);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(!tracks || (ntracks >= 1 && ntracks <= RED_MAX_TRACKS), "%s: ntracks=%d must be 1..%d", fn, ntracks, RED_MAX_TRACKS);
    DBX_REQUIRE(src && dst && (rows || n == 0) && (keep || k == 0), "%s: null argument", fn);
    DBX_REQUIRE(dst != src || style->method == 0, "%s: dst == src is allowed for fill only", fn);
    const dbx_redact_style st = *style;
    std::vector<RedEnt> list;
    RedEnt e;
    for (int i = 0; i < tile_min(k, n); ++i) {
        const int r = keep[i];
        if (r >= 0 && r < n && red_row_region(rows + (size_t)r * det_cols, det_cols, st, h, w, e)) list.push_back(e);
    }
    for (int t = 0; tracks && st.coast > 0 && t < ntracks; ++t)
        if (red_track_region(tracks + t, st, h, w, e)) list.push_back(e);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            bool cov = false;
            for (size_t q = 0; q < list.size() && !cov; ++q) cov = red_covers(list[q], x, y);
            const size_t o = ((size_t)y * w + x) * c;
            for (int ch = 0; ch < c; ++ch) {
                int v = src[o + ch];
                if (cov) v = st.method == 0 ? st.color[ch] : (st.method == 1 ? red_pixelate_px(src, h, w, c, st.cell, x, y, ch)
                                                                             : red_blur_px(src, h, w, c, st.radius, x, y, ch));
                if (cov || dst != src) dst[o + ch] = (uint8_t)v;
            }
        }
    return DBX_OK;
}
