// Tiled detection: the plan of a large frame (dbx_tile_grid, host) and the stitch of the tiles' rows per frame on the device --
// dbx_tile_rows_batch maps the rows of a forward chunk to source-frame coordinates and marks the ones their tile owns,
// dbx_tile_nms_batch packs the owned rows of every frame and runs the large NMS (nms_large.hpp, the code dbx_nms_large runs) over them.
// The mapped coordinates and the ownership sums are one IEEE operation per written operation so that NumPy gives the same bits:
// floating-point contraction is OFF in this file, for the device and for the host pass (dbx_tile_host runs the same functions).
#pragma clang fp contract(off)
#include "common.hpp"
#include "nms_large.hpp"

#include <cmath>
#include <cstddef>

#define TILE_THREADS 256
#define TILE_MAX_PLAN (1 << 20)          // tiles of one plan / one call

static_assert(sizeof(dbx_tile) == 64 && offsetof(dbx_tile, frame) == 0 && offsetof(dbx_tile, x0) == 4 && offsetof(dbx_tile, y0) == 8 &&
              offsetof(dbx_tile, side) == 12 && offsetof(dbx_tile, cw) == 16 && offsetof(dbx_tile, ch) == 20 &&
              offsetof(dbx_tile, scale) == 24 && offsetof(dbx_tile, lo2x) == 32 && offsetof(dbx_tile, hi2x) == 40 &&
              offsetof(dbx_tile, lo2y) == 48 && offsetof(dbx_tile, hi2y) == 56, "dbx_tile is 64 bytes");

// ---------------------------------------------------------------------------------------------------------------- the shared rules
// one column of a tile row in source-frame coordinates (merge_map_col's expression): x columns 0, 2, 5, 7, 9, 11, y columns 1, 3, 6, 8,
// 10, 12, the score copied; off = -origin
__host__ __device__ static inline double tile_map_col(double v, int col, double scale, double off_x, double off_y) {
    if (col == 4) return v;
    const bool is_x = col < 4 ? !(col & 1) : (col & 1);
    return v * scale - (is_x ? off_x : off_y);
}

// the mark of a MAPPED box: the doubled centre inside the tile's half-open core; every comparison with a NaN is false
__host__ __device__ static inline int tile_owned(double x1, double y1, double x2, double y2, const dbx_tile& t, int rule) {
    if (rule == DBX_TILE_RULE_NONE) return 1;
    const double sx = x1 + x2, sy = y1 + y2;
    return (t.lo2x <= sx && sx < t.hi2x && t.lo2y <= sy && sy < t.hi2y) ? 1 : 0;
}

__host__ __device__ static inline int tile_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the staging area: pairs [n_tiles][2] int32 | marks [n_tiles][rpt] int32 | rows [n_tiles][rpt][dc] float64, each part to 256 bytes
struct TileStage { long long marks, rows, total; };
static __host__ __device__ inline TileStage tile_stage(int n_tiles, int rpt, int dc) {
    TileStage S;
    S.marks = thr_up256((long long)n_tiles * 8);
    S.rows = S.marks + thr_up256((long long)n_tiles * rpt * 4);
    S.total = S.rows + thr_up256((long long)n_tiles * rpt * dc * 8);
    return S;
}
// one frame's NMS slice: order [nmax] int32 (to 256 bytes) | matrix [nmax][ceil(nmax / 64)] words
struct TileSlice { long long mask, total; int nw; };
static __host__ __device__ inline TileSlice tile_slice(int nmax) {
    TileSlice L;
    L.nw = (nmax + 63) / 64;
    L.mask = thr_up256((long long)nmax * 4);
    L.total = L.mask + thr_up256((long long)nmax * L.nw * 8);
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- the plan
static inline int tile_axis_count(int L, int S, int D) { return L <= S ? 1 : (int)(((long long)L - S + D - 1) / D) + 1; }
static inline int tile_axis_start(int L, int S, int D, int i) {
    if (L <= S) return 0;
    const long long s = (long long)i * D;
    return (int)(s < (long long)L - S ? s : (long long)L - S);
}

extern "C" int dbx_tile_grid(int32_t h, int32_t w, int32_t src, int32_t overlap, dbx_tile* out, int32_t cap) {
    const char* fn = "tile_grid";
    DBX_REQUIRE(h >= 1 && w >= 1, "%s: frame size %d x %d must be positive", fn, h, w);
    DBX_REQUIRE(src >= 1, "%s: src=%d must be at least 1", fn, src);
    DBX_REQUIRE(overlap >= 0, "%s: overlap=%d is negative", fn, overlap);
    DBX_REQUIRE(2 * (int64_t)overlap <= src, "%s: overlap=%d is more than half of src=%d (a point would lie in three windows of an axis)", fn,
                overlap, src);
    const int D = src - overlap;
    const int nx = tile_axis_count(w, src, D), ny = tile_axis_count(h, src, D);
    DBX_REQUIRE((int64_t)nx * ny <= TILE_MAX_PLAN, "%s: %lld tiles exceed %d", fn, (long long)nx * ny, TILE_MAX_PLAN);
    const int n = nx * ny;
    if (!out) return n;
    DBX_REQUIRE(cap >= n, "%s: cap=%d is below the %d tiles of the plan", fn, cap, n);
    for (int iy = 0; iy < ny; ++iy) {
        const int y0 = tile_axis_start(h, src, D, iy);
        for (int ix = 0; ix < nx; ++ix) {
            const int x0 = tile_axis_start(w, src, D, ix);
            dbx_tile& t = out[(size_t)iy * nx + ix];
            t.frame = 0; t.x0 = x0; t.y0 = y0; t.side = src;
            t.cw = w - x0 < src ? w - x0 : src;
            t.ch = h - y0 < src ? h - y0 : src;
            t.scale = 1.0;
            // doubled midpoint of the overlap with the neighbour: s_i + S + s_(i+1)
            t.lo2x = ix == 0 ? -INFINITY : (double)((long long)tile_axis_start(w, src, D, ix - 1) + src + x0);
            t.hi2x = ix == nx - 1 ? INFINITY : (double)((long long)x0 + src + tile_axis_start(w, src, D, ix + 1));
            t.lo2y = iy == 0 ? -INFINITY : (double)((long long)tile_axis_start(h, src, D, iy - 1) + src + y0);
            t.hi2y = iy == ny - 1 ? INFINITY : (double)((long long)y0 + src + tile_axis_start(h, src, D, iy + 1));
        }
    }
    return n;
}

// The host-side requirements on a call's table for entry point `fn`: frames > 0 also bounds the frame indices.  max_tiles: the largest
// number of tiles of one frame.
static int tile_table_check(const char* fn, const dbx_tile* tiles, int32_t n_tiles, int32_t frames, int32_t rows_per_tile, int32_t det_cols,
                            int32_t* max_tiles) {
    DBX_REQUIRE(n_tiles >= 1 && n_tiles <= TILE_MAX_PLAN, "%s: n_tiles=%d must be 1..%d", fn, n_tiles, TILE_MAX_PLAN);
    DBX_REQUIRE(det_cols == 5 || det_cols == 13, "%s: det_cols=%d must be 5 or 13", fn, det_cols);
    DBX_REQUIRE(rows_per_tile >= 1 && rows_per_tile <= THR_MAX_DETS, "%s: rows_per_tile=%d must be 1..%d", fn, rows_per_tile, THR_MAX_DETS);
    DBX_REQUIRE(tiles, "%s: null argument", fn);
    DBX_REQUIRE((int64_t)n_tiles * rows_per_tile <= 0x7fffffff / 16, "%s: n_tiles * rows_per_tile = %lld rows do not fit the packed arena's int32 prefix",
                fn, (long long)n_tiles * rows_per_tile);
    int run = 0, longest = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const dbx_tile& q = tiles[t];
        DBX_REQUIRE(std::isfinite(q.scale) && q.scale > 0.0, "%s: tile %d has scale %g (finite and positive needed)", fn, t, q.scale);
        DBX_REQUIRE(q.x0 >= 0 && q.y0 >= 0, "%s: tile %d has a negative origin (%d, %d)", fn, t, q.x0, q.y0);
        DBX_REQUIRE(!std::isnan(q.lo2x) && !std::isnan(q.hi2x) && !std::isnan(q.lo2y) && !std::isnan(q.hi2y), "%s: tile %d has a NaN core bound",
                    fn, t);
        DBX_REQUIRE(q.frame >= 0 && (frames <= 0 || q.frame < frames), "%s: tile %d has frame %d outside 0..%d", fn, t, q.frame, frames - 1);
        DBX_REQUIRE(t == 0 || q.frame >= tiles[t - 1].frame, "%s: tile %d has frame %d behind frame %d (the frame indices must not decrease)", fn,
                    t, q.frame, t ? tiles[t - 1].frame : 0);
        run = (t > 0 && q.frame == tiles[t - 1].frame) ? run + 1 : 1;
        DBX_REQUIRE((int64_t)run * rows_per_tile <= THR_MAX_DETS, "%s: frame %d has more than %d tiles x rows_per_tile=%d = %d rows (the NMS's bound)",
                    fn, q.frame, THR_MAX_DETS / rows_per_tile, rows_per_tile, THR_MAX_DETS);
        longest = run > longest ? run : longest;
    }
    *max_tiles = longest;
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- rows of a chunk
struct TileRowsArgs {
    const double* rows; const int* counts; const dbx_tile* tiles; unsigned char* stage;
    int n_tiles, t0, rpt, dc, rule;
};

// One workgroup per tile of the chunk.  No LDS but one counter.  t0 + blockIdx.x < n_tiles is the host's check; the delivered count is
// device data and clamped.
__global__ __launch_bounds__(TILE_THREADS) void tile_rows_kernel(const TileRowsArgs a) {
    __shared__ int s_owned;
    const int i = blockIdx.x, tid = threadIdx.x, t = a.t0 + i;
    const TileStage S = tile_stage(a.n_tiles, a.rpt, a.dc);
    const dbx_tile tl = a.tiles[t];
    const int cnt = a.counts ? tile_clamp(a.counts[2 * i], 0, a.rpt) : a.rpt;
    if (tid == 0) s_owned = 0;
    __syncthreads();
    const double off_x = -(double)tl.x0, off_y = -(double)tl.y0;
    const double* src = a.rows + (size_t)i * a.rpt * a.dc;
    double* dst = (double*)(a.stage + S.rows) + (size_t)t * a.rpt * a.dc;
    int* marks = (int*)(a.stage + S.marks) + (size_t)t * a.rpt;
    for (int e = tid; e < cnt * a.dc; e += TILE_THREADS) {
        const int r = e / a.dc, col = e - r * a.dc;
        dst[e] = tile_map_col(src[e], col, tl.scale, off_x, off_y);
    }
    int mine = 0;
    for (int r = tid; r < cnt; r += TILE_THREADS) {
        const double* q = src + (size_t)r * a.dc;
        const int m = tile_owned(tile_map_col(q[0], 0, tl.scale, off_x, off_y), tile_map_col(q[1], 1, tl.scale, off_x, off_y),
                                 tile_map_col(q[2], 2, tl.scale, off_x, off_y), tile_map_col(q[3], 3, tl.scale, off_x, off_y), tl, a.rule);
        marks[r] = m;
        mine += m;
    }
    if (mine) atomicAdd(&s_owned, mine);
    __syncthreads();
    if (tid == 0) {
        int* pairs = (int*)a.stage;
        pairs[2 * t] = cnt; pairs[2 * t + 1] = s_owned;
    }
}

extern "C" int64_t dbx_tile_stage_bytes(int32_t n_tiles, int32_t rows_per_tile, int32_t det_cols) {
    if (n_tiles < 1 || n_tiles > TILE_MAX_PLAN || rows_per_tile < 1 || rows_per_tile > THR_MAX_DETS || (det_cols != 5 && det_cols != 13) ||
        (int64_t)n_tiles * rows_per_tile > 0x7fffffff / 16)
        return -1;
    return tile_stage(n_tiles, rows_per_tile, det_cols).total;
}

extern "C" int dbx_tile_rows_batch(const double* rows, const int32_t* counts, const dbx_tile* tiles, const dbx_tile* tiles_dev,
                                   int32_t n_tiles, int32_t t0, int32_t n, int32_t rows_per_tile, int32_t det_cols, int32_t rule,
                                   void* stage, void* stream) {
    const char* fn = "tile_rows_batch";
    int32_t max_tiles = 0;
    const int rc = tile_table_check(fn, tiles, n_tiles, 0, rows_per_tile, det_cols, &max_tiles);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(n >= 1, "%s: n=%d must be positive", fn, n);
    DBX_REQUIRE(t0 >= 0 && (int64_t)t0 + n <= n_tiles, "%s: tiles %d..%lld are not all in 0..%d", fn, t0, (long long)t0 + n - 1, n_tiles - 1);
    DBX_REQUIRE(rule == DBX_TILE_RULE_NONE || rule == DBX_TILE_RULE_CORE, "%s: rule=%d must be 0 (none) or 1 (core)", fn, rule);
    DBX_REQUIRE(rows && tiles_dev && stage, "%s: null argument", fn);
    TileRowsArgs a;
    a.rows = rows; a.counts = counts; a.tiles = tiles_dev; a.stage = (unsigned char*)stage;
    a.n_tiles = n_tiles; a.t0 = t0; a.rpt = rows_per_tile; a.dc = det_cols; a.rule = rule;
    hipLaunchKernelGGL(tile_rows_kernel, dim3((unsigned)n), dim3(TILE_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- pack + NMS
struct TileNmsArgs {
    const dbx_tile* tiles; const unsigned char* stage;
    double* out_dets; int* out_keep; int* out_tile; int* out_counts;
    unsigned char* slices;
    double thresh;
    int n_tiles, frames, rpt, dc, max_tiles, keep_behind_rows;
};

// One workgroup per frame.  The table and the staging area are device data: the frame's tiles are counted, not looked up, the pairs
// are clamped, and every packed position is checked against the frame's own row count, so whatever they hold the launch stays inside
// its buffers.  LDS: the 48 KB of (key, row) pairs nmsl_sort_pairs takes, and a few counters.
//   1. first_b = #{t: frame_t < b}, T_b = #{t: frame_t == b} (clamped to max_tiles); P[b] and the call's total from the owned counts.
//   2. the frame's slots, 1024 at a time in (tile, row) order: a ballot prefix gives every owned row its packed position; the thread
//      copies the row, files the (nmsl_score_key, packed row) pair and writes the tile index.
//   3. nmsl_sort_pairs -> the NMS order of the frame's slice.
__global__ __launch_bounds__(DET_THREADS) void tile_pack_kernel(const TileNmsArgs a) {
    __shared__ unsigned long long key[THR_MAX_DETS];
    __shared__ int row[THR_MAX_DETS];
    __shared__ int s_first, s_T, s_pre, s_mine, s_tot;
    __shared__ int wsum[DET_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const TileStage S = tile_stage(a.n_tiles, a.rpt, a.dc);
    const int* pairs = (const int*)a.stage;
    const int* marks = (const int*)(a.stage + S.marks);
    const double* rows = (const double*)(a.stage + S.rows);
    if (tid == 0) { s_first = 0; s_T = 0; s_pre = 0; s_mine = 0; s_tot = 0; }
    __syncthreads();
    {
        int first = 0, T = 0, pre = 0, mine = 0, tot = 0;
        for (int t = tid; t < a.n_tiles; t += DET_THREADS) {
            const int f = a.tiles[t].frame, own = tile_clamp(pairs[2 * t + 1], 0, a.rpt);
            tot += own;
            if (f < b) { ++first; pre += own; } else if (f == b) { ++T; mine += own; }
        }
        atomicAdd(&s_first, first); atomicAdd(&s_T, T); atomicAdd(&s_pre, pre); atomicAdd(&s_mine, mine); atomicAdd(&s_tot, tot);
    }
    __syncthreads();
    const int first = s_first, T = min(s_T, a.max_tiles), pre = s_pre, tot = s_tot;     // first + T <= n_tiles
    const int m = min(s_mine, T * a.rpt);                                               // <= max_tiles * rpt <= THR_MAX_DETS
    for (int i = tid; i < T; i += DET_THREADS) {
        const int t = first + i;
        a.out_counts[2 * t] = tile_clamp(pairs[2 * t], 0, a.rpt);
        a.out_counts[2 * t + 1] = tile_clamp(pairs[2 * t + 1], 0, a.rpt);
    }
    int* const prefix = a.out_counts + 2 * (size_t)a.n_tiles;
    if (tid == 0) { prefix[b] = pre; if (b == a.frames - 1) prefix[a.frames] = tot; }
    if (m == 0) return;
    int P2 = 2;
    while (P2 < m) P2 <<= 1;
    // every position holds a row of the frame before the packing fills it in (padding: below -inf's key, behind every row)
    for (int i = tid; i < P2; i += DET_THREADS) { key[i] = 0ull; row[i] = i < m ? i : -1; }
    __syncthreads();
    double* const o = a.out_dets + (size_t)pre * a.dc;            // pre + m <= tot <= n_tiles * rpt, the capacity
    int* const ot = a.out_tile + pre;
    const int slots = T * a.rpt;
    int base = 0;
    for (int c0 = 0; c0 < slots; c0 += DET_THREADS) {             // (uniform trip count)
        const int s = c0 + tid;
        bool own = false;
        int t = 0, r = 0;
        if (s < slots) {
            const int tl = s / a.rpt;
            r = s - tl * a.rpt;
            t = first + tl;
            own = r < tile_clamp(pairs[2 * t], 0, a.rpt) && marks[(size_t)t * a.rpt + r] != 0;
        }
        const unsigned long long mb = __ballot(own);
        if (lane == 0) wsum[wave] = __popcll(mb);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < DET_THREADS / 64; ++w) { off += w < wave ? wsum[w] : 0; total += wsum[w]; }
        if (own) {
            const int u = base + off + __popcll(mb & below);
            if (u < m) {
                const double* q = rows + ((size_t)t * a.rpt + r) * a.dc;
                for (int col = 0; col < a.dc; ++col) o[(size_t)u * a.dc + col] = q[col];
                key[u] = nmsl_score_key(q[4]);
                ot[u] = t;
            }
        }
        base += total;
        __syncthreads();                                         // wsum is rewritten by the next round; key is read by the sort
    }
    nmsl_sort_pairs(key, row, P2);
    int* const order = (int*)(a.slices + (size_t)b * tile_slice(a.max_tiles * a.rpt).total);
    for (int i = tid; i < m; i += DET_THREADS) order[i] = row[i];
}

__global__ __launch_bounds__(NMSL_THREADS) void tile_mask_kernel(const TileNmsArgs a) {
    const int rb = blockIdx.x, b = blockIdx.y;
    const int* const prefix = a.out_counts + 2 * (size_t)a.n_tiles;
    const int pre = prefix[b], m = min(prefix[b + 1] - pre, a.max_tiles * a.rpt);
    if (64 * rb >= m) return;
    const TileSlice L = tile_slice(a.max_tiles * a.rpt);
    unsigned char* const s = a.slices + (size_t)b * L.total;
    nmsl_mask_rows(a.out_dets + (size_t)pre * a.dc, a.dc, (const int*)s, m, a.thresh, (unsigned long long*)(s + L.mask), L.nw, rb);
}

__global__ __launch_bounds__(64) void tile_sweep_kernel(const TileNmsArgs a) {
    const int b = blockIdx.x;
    const int* const prefix = a.out_counts + 2 * (size_t)a.n_tiles;
    const int pre = prefix[b], m = min(prefix[b + 1] - pre, a.max_tiles * a.rpt), tot = prefix[a.frames];
    int* const keep = (a.keep_behind_rows ? (int*)(a.out_dets + (size_t)tot * a.dc) : a.out_keep) + (size_t)pre + b;
    const TileSlice L = tile_slice(a.max_tiles * a.rpt);
    const unsigned char* s = a.slices + (size_t)b * L.total;
    nmsl_sweep((const unsigned long long*)(s + L.mask), L.nw, (const int*)s, m, keep);
}

extern "C" int64_t dbx_tile_nms_batch_workspace_bytes(int32_t frames, int32_t max_tiles, int32_t rows_per_tile) {
    if (frames < 1 || max_tiles < 1 || rows_per_tile < 1 || rows_per_tile > THR_MAX_DETS || (int64_t)max_tiles * rows_per_tile > THR_MAX_DETS)
        return -1;
    return (int64_t)frames * tile_slice(max_tiles * rows_per_tile).total;
}

extern "C" int dbx_tile_nms_batch(const dbx_tile* tiles, const dbx_tile* tiles_dev, int32_t n_tiles, int32_t frames, int32_t rows_per_tile,
                                  int32_t det_cols, double nms_thresh, const void* stage, double* out_dets, int32_t* out_keep,
                                  int32_t* out_tile, int32_t* out_counts, void* workspace, void* stream) {
    const char* fn = "tile_nms_batch";
    DBX_REQUIRE(frames >= 1, "%s: frames=%d must be positive", fn, frames);
    int32_t max_tiles = 0;
    const int rc = tile_table_check(fn, tiles, n_tiles, frames, rows_per_tile, det_cols, &max_tiles);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(!std::isnan(nms_thresh) && nms_thresh >= 0.0, "%s: nms_thresh=%g must be a number >= 0", fn, nms_thresh);
    DBX_REQUIRE(tiles_dev && stage && out_dets && out_keep && out_tile && out_counts && workspace, "%s: null argument", fn);
    TileNmsArgs a;
    a.tiles = tiles_dev; a.stage = (const unsigned char*)stage;
    a.out_dets = out_dets; a.out_keep = out_keep; a.out_tile = out_tile; a.out_counts = out_counts;
    a.slices = (unsigned char*)workspace;
    a.thresh = nms_thresh;
    a.n_tiles = n_tiles; a.frames = frames; a.rpt = rows_per_tile; a.dc = det_cols; a.max_tiles = max_tiles;
    a.keep_behind_rows = (const void*)out_keep == (const void*)out_dets;
    hipLaunchKernelGGL(tile_pack_kernel, dim3((unsigned)frames), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(tile_mask_kernel, dim3((unsigned)((max_tiles * rows_per_tile + 63) / 64), (unsigned)frames), dim3(NMSL_THREADS), 0,
                       (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(tile_sweep_kernel, dim3((unsigned)frames), dim3(64), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host side
extern "C" int dbx_tile_host(int32_t op, int64_t n, const dbx_tile* tiles, int32_t n_tiles, const int32_t* tile_of, const double* rows,
                             int32_t det_cols, int32_t rule, double* out_rows, int32_t* out_marks) {
    const char* fn = "tile_host";
    DBX_REQUIRE(op == 0 || op == 1, "%s: op=%d must be 0 (map) or 1 (map + mark)", fn, op);
    DBX_REQUIRE(n >= 0, "%s: n=%lld is negative", fn, (long long)n);
    DBX_REQUIRE(det_cols == 5 || det_cols == 13, "%s: det_cols=%d must be 5 or 13", fn, det_cols);
    DBX_REQUIRE(rule == DBX_TILE_RULE_NONE || rule == DBX_TILE_RULE_CORE, "%s: rule=%d must be 0 (none) or 1 (core)", fn, rule);
    DBX_REQUIRE(n_tiles >= 1, "%s: n_tiles=%d must be positive", fn, n_tiles);
    if (n == 0) return DBX_OK;
    DBX_REQUIRE(tiles && tile_of && rows && out_rows && (op == 0 || out_marks), "%s: null argument", fn);
    for (int64_t i = 0; i < n; ++i)
        DBX_REQUIRE(tile_of[i] >= 0 && tile_of[i] < n_tiles, "%s: row %lld names tile %d outside 0..%d", fn, (long long)i, tile_of[i], n_tiles - 1);
    for (int64_t i = 0; i < n; ++i) {
        const dbx_tile& tl = tiles[tile_of[i]];
        const double off_x = -(double)tl.x0, off_y = -(double)tl.y0;
        const double* q = rows + i * det_cols;
        double* o = out_rows + i * det_cols;
        for (int col = 0; col < det_cols; ++col) o[col] = tile_map_col(q[col], col, tl.scale, off_x, off_y);
        if (op == 1) out_marks[i] = tile_owned(o[0], o[1], o[2], o[3], tl, rule);
    }
    return DBX_OK;
}
