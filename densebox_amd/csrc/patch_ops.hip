// Training patches sampled and cut on the device (include/densebox_hip.h, "training patch sampling"): the geometry half of the
// reference's patch cutters (gen_pos_patch, process_plate.py:167-352; the negative path of gen_pure_neg_patches, :711-749) as ONE
// workgroup (dbx_patch_plan) and the pixel half as the batched resize's tile body over the records that workgroup wrote
// (dbx_patch_cut).  The geometry is float64 in the reference's order of operations and must give the bits CPython gives, so
// floating-point contraction is OFF in this file.
//
// The counter-based hash of draw number j of candidate i (unsigned 64-bit, wrapping):
//     mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
//     h = mix(mix(seed + 0x9E3779B97F4A7C15 * (counter + 1)) + 0xD1B54A32D192ED03 * (i + 1) + 0x8CB92BA72F3D8DD7 * (j + 1))
// k = h >> 11 is the 53-bit draw: a uniform is -1.0 + 2.0 * (k * 2^-53), an integer in a range of r values is k mod r.
#pragma clang fp contract(off)
#include "common.hpp"
#include "patch_hash.hpp"
#include "patch_stage.hpp"
#include "resize_tile.hpp"

#include <math.h>

static_assert(sizeof(dbx_patch_job) == sizeof(ResizeJobDev), "dbx_patch_job is the resize kernel's device record");
static_assert(offsetof(dbx_patch_job, row_bytes) == offsetof(ResizeJobDev, row_bytes) &&
              offsetof(dbx_patch_job, tiles_x) == offsetof(ResizeJobDev, tiles_x) &&
              offsetof(dbx_patch_job, frame) == offsetof(ResizeJobDev, pad), "dbx_patch_job layout");
static_assert(sizeof(dbx_patch_geom) == 72 && sizeof(dbx_patch_plan_io) == 136, "patch ABI layouts");

#define PATCH_TILES_X ((DBX_PATCH_SIDE + RSZ_TW - 1) / RSZ_TW)
#define PATCH_TILES (PATCH_TILES_X * ((DBX_PATCH_SIDE + RSZ_TH - 1) / RSZ_TH))

// int(x + 0.5) of the reference: truncation toward zero; saturated where a Python int would go on growing
__host__ __device__ inline int patch_round(double x) {
    const double y = x + 0.5;
    if (!(y > -1.0e9)) return -1000000000;          // also NaN, which finite inputs and non-zero sides cannot make
    if (y > 1.0e9) return 1000000000;
    return (int)y;
}

// format_4_vertices on v[4][2] (annotation order): s = (left-up, right-up, right-down, left-down).  False where the reference raises
// IndexError, which is exactly when two vertices are equal by value: an equal pair inside the left or the right pair empties
// `[x for x in pts if x != up]`, and an equal pair across them leaves fewer than two right points.
__host__ __device__ inline bool patch_sort_vertices(const int* v, int s[4][2]) {
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (v[2 * a] == v[2 * b] && v[2 * a + 1] == v[2 * b + 1]) return false;
    int ord[4] = {0, 1, 2, 3};                        // stable insertion sort on x
    for (int a = 1; a < 4; ++a) {
        const int o = ord[a];
        int b = a;
        while (b > 0 && v[2 * ord[b - 1]] > v[2 * o]) { ord[b] = ord[b - 1]; --b; }
        ord[b] = o;
    }
    const int l0 = ord[0], l1 = ord[1];               // the left pair in sorted order
    int r0 = -1, r1 = -1;                             // the right pair in annotation order
    for (int a = 0; a < 4; ++a)
        if (a != l0 && a != l1) { if (r0 < 0) r0 = a; else r1 = a; }
    const int lu = v[2 * l1 + 1] < v[2 * l0 + 1] ? l1 : l0, ld = lu == l0 ? l1 : l0;     // stable: the first wins a tie on y
    const int ru = v[2 * r1 + 1] < v[2 * r0 + 1] ? r1 : r0, rd = ru == r0 ? r1 : r0;
    s[0][0] = v[2 * lu]; s[0][1] = v[2 * lu + 1];
    s[1][0] = v[2 * ru]; s[1][1] = v[2 * ru + 1];
    s[2][0] = v[2 * rd]; s[2][1] = v[2 * rd + 1];
    s[3][0] = v[2 * ld]; s[3][1] = v[2 * ld + 1];
    return true;
}

__host__ __device__ inline void patch_geom_clear(dbx_patch_geom* g, int status) {
    g->status = status; g->x0 = g->y0 = g->x1 = g->y1 = 0; g->reserved = 0;
    for (int k = 0; k < 12; ++k) g->labels[k] = 0;
}

// gen_pos_patch on one plate of a W x H frame
__host__ __device__ inline void patch_positive(int W, int H, const int* verts, double d0, double d1, double radius, dbx_patch_geom* g) {
    patch_geom_clear(g, 0);
    for (int a = 0; a < 4; ++a)
        if (verts[2 * a] < 0 || verts[2 * a] > W - 1 || verts[2 * a + 1] < 0 || verts[2 * a + 1] > H - 1) { g->status = 4; return; }
    int s[4][2];
    if (!patch_sort_vertices(verts, s) || !(fabs(d0) <= 1.0e100) || !(fabs(d1) <= 1.0e100)) { g->status = 2; return; }
    const int bx0 = s[0][0] < s[3][0] ? s[0][0] : s[3][0], bx1 = s[1][0] > s[2][0] ? s[1][0] : s[2][0];
    const int by0 = s[0][1] < s[1][1] ? s[0][1] : s[1][1], by1 = s[3][1] > s[2][1] ? s[3][1] : s[2][1];
    const int cx = patch_round((double)(bx0 + bx1) * 0.5), cy = patch_round((double)(by0 + by1) * 0.5);
    const double bw = (double)(bx1 - bx0), bh = (double)(by1 - by0);
    const double off_x = d0 * radius, off_y = d1 * radius;
    double pw = 4.0 * bw, ph = 4.0 * bh;
    double ox = (double)cx - pw * 0.5 - off_x, oy = (double)cy - ph * 0.5 - off_y;
    double ex = ox + pw, ey = oy + ph;
    if (ox < 0 || oy < 0) {
        ox = ox >= 0 ? ox : 0.0;
        oy = oy >= 0 ? oy : 0.0;
        pw = ex - ox; ph = ey - oy;
    }
    if (ex >= (double)W || ey >= (double)H) {
        ex = ex < (double)W ? ex : (double)(W - 1);
        ey = ey < (double)H ? ey : (double)(H - 1);
        pw = ex - ox; ph = ey - oy;
    }
    if (pw == 0.0 || ph == 0.0) { g->status = 2; return; }
    const double side = (double)DBX_PATCH_SIDE;
    g->labels[0] = patch_round((((double)bx0 - ox) / pw) * side); g->labels[1] = patch_round((((double)by0 - oy) / ph) * side);
    g->labels[2] = patch_round((((double)bx1 - ox) / pw) * side); g->labels[3] = patch_round((((double)by1 - oy) / ph) * side);
    for (int a = 0; a < 4; ++a) {
        g->labels[4 + 2 * a] = patch_round((((double)s[a][0] - ox) / pw) * side);
        g->labels[5 + 2 * a] = patch_round((((double)s[a][1] - oy) / ph) * side);
    }
    const int* L = g->labels + 4;                       // lu, ru, rd, ld
    if (L[0] < 8 || L[1] < 8 || L[2] > W - 8 || L[3] < 8 || L[4] > W - 8 || L[5] > H - 8 || L[6] < 8 || L[7] > H - 8) {
        patch_geom_clear(g, 1);
        return;
    }
    g->x0 = patch_round(ox); g->y0 = patch_round(oy); g->x1 = patch_round(ex); g->y1 = patch_round(ey);
    if (g->x1 <= g->x0 || g->y1 <= g->y0) g->status = 3;
}

// the negative crop centred on (d0, d1) of a W x H frame with n_verts plates (8 integers each): intersect_small
__host__ __device__ inline void patch_negative(int W, int H, const int* verts, int n_verts, int stride, double d0, double d1, int th,
                                               dbx_patch_geom* g) {
    patch_geom_clear(g, 0);
    if (W < DBX_PATCH_SIDE + 1 || H < DBX_PATCH_SIDE + 1 || !(d0 >= 120.0 && d0 < (double)(W - 120)) ||
        !(d1 >= 120.0 && d1 < (double)(H - 120)) || d0 != (double)(int)d0 || d1 != (double)(int)d1) {
        g->status = 5;
        return;
    }
    const int cx = (int)d0, cy = (int)d1;
    int s[4][2];
    for (int p = 0; p < n_verts; ++p)                   // every plate is formatted before intersect_small runs: any raise wins
        if (!patch_sort_vertices(verts + (size_t)p * stride, s)) { g->status = 2; return; }
    for (int p = 0; p < n_verts; ++p) {
        patch_sort_vertices(verts + (size_t)p * stride, s);
        const int iw = (s[2][0] < cx + 120 ? s[2][0] : cx + 120) - (s[0][0] > cx - 120 ? s[0][0] : cx - 120);
        const int ih = (s[2][1] < cy + 120 ? s[2][1] : cy + 120) - (s[0][1] > cy - 120 ? s[0][1] : cy - 120);
        if (iw < 0 || ih < 0) break;                    // "return True" at the first plate that does not overlap
        if ((long long)iw * ih > (long long)th) { g->status = 6; return; }
    }
    g->x0 = cx - 120; g->y0 = cy - 120; g->x1 = cx + 120; g->y1 = cy + 120;
}

__host__ __device__ inline bool patch_frame_usable(const dbx_crop_frame& f, int c) {
    return f.src && f.sh > 0 && f.sw > 0 && (long long)f.sh * f.sw * c <= 0x7fffffffLL;
}

// One workgroup.  Pass k handles the candidates k * PATCH_THREADS + tid, so a pass is a contiguous run of candidates and its ballot
// scan plus the running total of the passes before it IS the exclusive scan in candidate order.
__global__ __launch_bounds__(PATCH_THREADS) void patch_plan_kernel(dbx_patch_plan_io io, int n_frames, int n_plates, int c, int M, int n,
                                                                    double neg_frac, double radius, int th) {
    __shared__ int wave_total[PATCH_THREADS / 64];
    __shared__ int tally[DBX_PATCH_NSTATUS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool device_mode = io.cand == nullptr;
    const int64_t seed = device_mode ? io.state[0] : 0, counter = device_mode ? io.state[1] : 0;
    if (tid < DBX_PATCH_NSTATUS) tally[tid] = 0;
    __syncthreads();
    int running = 0;
    for (int base = 0; base < M; base += PATCH_THREADS) {
        const int i = base + tid;
        dbx_patch_geom g;
        int kind = 0, index = 0, frame = -1;
        double d0 = 0.0, d1 = 0.0;
        if (i < M) {
            if (device_mode) {
                kind = (n_plates == 0 || patch_unit(patch_hash(seed, counter, i, 0)) < neg_frac) ? 1 : 0;
                index = (int)((patch_hash(seed, counter, i, 1) >> 11) % (uint64_t)(kind ? n_frames : n_plates));
            } else {
                kind = io.cand[2 * i]; index = io.cand[2 * i + 1];
                d0 = io.draws[2 * i]; d1 = io.draws[2 * i + 1];
            }
            if (kind < 0 || kind > 1 || index < 0 || index >= (kind ? n_frames : n_plates)) {
                patch_geom_clear(&g, 2);
            } else {
                frame = kind ? index : io.plates[9 * index];
                if (frame < 0 || frame >= n_frames) {
                    patch_geom_clear(&g, 2);
                } else {
                    const dbx_crop_frame f = io.frames[frame];
                    if (!patch_frame_usable(f, c)) {
                        patch_geom_clear(&g, 4);
                    } else if (kind == 0) {
                        if (device_mode) {
                            d0 = -1.0 + 2.0 * patch_unit(patch_hash(seed, counter, i, 2));
                            d1 = -1.0 + 2.0 * patch_unit(patch_hash(seed, counter, i, 3));
                        }
                        patch_positive(f.sw, f.sh, io.plates + 9 * index + 1, d0, d1, radius, &g);
                    } else {
                        if (device_mode && f.sw > DBX_PATCH_SIDE && f.sh > DBX_PATCH_SIDE) {
                            d0 = (double)(120 + (int)((patch_hash(seed, counter, i, 2) >> 11) % (uint64_t)(f.sw - DBX_PATCH_SIDE)));
                            d1 = (double)(120 + (int)((patch_hash(seed, counter, i, 3) >> 11) % (uint64_t)(f.sh - DBX_PATCH_SIDE)));
                        }
                        int p0 = io.plate0[frame], p1 = io.plate0[frame + 1];
                        if (p0 < 0) p0 = 0;
                        if (p1 > n_plates) p1 = n_plates;
                        patch_negative(f.sw, f.sh, io.plates + 9 * (size_t)p0 + 1, p1 > p0 ? p1 - p0 : 0, 9, d0, d1, th, &g);
                    }
                }
            }
        } else {
            patch_geom_clear(&g, 1);
        }
        const bool accept = i < M && g.status == 0;
        const unsigned long long mask = __ballot(accept);
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        int rank = running + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < PATCH_THREADS / 64; ++w) {
            if (w < wave) rank += wave_total[w];
            running += wave_total[w];
        }
        if (i < M) {
            const int status = accept && rank >= n ? 7 : g.status;
            io.status[i] = status;
            io.slot[i] = accept ? rank : -1;
            io.cand_out[2 * i] = kind; io.cand_out[2 * i + 1] = index;
            io.draws_out[2 * i] = d0; io.draws_out[2 * i + 1] = d1;
            atomicAdd(&tally[status], 1);
            if (status == 0) {
                const dbx_crop_frame f = io.frames[frame];
                dbx_patch_job J;
                J.src = f.src; J.dst = nullptr;
                J.cx0 = g.x0; J.cy0 = g.y0; J.cw = g.x1 - g.x0; J.ch = g.y1 - g.y0;
                J.scale_x = (double)J.cw / (double)DBX_PATCH_SIDE; J.scale_y = (double)J.ch / (double)DBX_PATCH_SIDE;
                J.row_bytes = f.sw * c;
                J.pad_l = 0; J.pad_t = 0; J.vw = J.cw; J.vh = J.ch; J.dh = DBX_PATCH_SIDE; J.dw = DBX_PATCH_SIDE; J.pad_value = 0;
                J.tiles_x = PATCH_TILES_X; J.frame = frame; J.kind = kind; J.reserved = 0;
                io.jobs[rank] = J;
                patch_write_labels(g.labels, rank, io.labels, io.bbox, io.vertices, io.label, kind != 0);
            }
        }
        __syncthreads();                               // wave_total is rewritten by the next pass
    }
    if (tid < DBX_PATCH_NSTATUS) io.tally[tid] = tally[tid];
    if (tid == 0) {
        *io.count = running < n ? running : n;
        if (device_mode) io.state[1] = counter + 1;     // every thread read the counter before the first barrier
    }
}

// Workgroup t: tile t % 60 of slot t / 60 -- every job has the same 4 x 15 tiles, so there is no prefix table to search.
template <int C>
__global__ __launch_bounds__(RSZ_THREADS) void patch_cut_kernel(const ResizeJobDev* __restrict__ jobs, const int* __restrict__ count, int n,
                                                                unsigned char* __restrict__ patches) {
    const PatchPart wg = patch_part<PATCH_TILES>(count, n);
    if (wg.slot >= wg.count) return;                   // uniform over the workgroup
    const int slot = wg.slot, tt = wg.part;
    const int x0 = (tt % PATCH_TILES_X) * RSZ_TW, y0 = (tt / PATCH_TILES_X) * RSZ_TH;
    resize_tile_body(jobs + slot, patches + (size_t)slot * DBX_PATCH_SIDE * DBX_PATCH_SIDE * C, x0, y0, RszSrcU8<C>(jobs + slot));
}

extern "C" int dbx_patch_plan(const dbx_patch_plan_io* io, int32_t n_frames, int32_t n_plates, int32_t c, int32_t M, int32_t n,
                              double neg_frac, double offset_radius, int32_t th, void* stream) {
    DBX_REQUIRE(io, "patch_plan: null io");
    DBX_REQUIRE(n_frames >= 1, "patch_plan: n_frames=%d must be at least 1", n_frames);
    DBX_REQUIRE(n_plates >= 0, "patch_plan: n_plates=%d is negative", n_plates);
    DBX_REQUIRE(c >= 1 && c <= 4, "patch_plan: c=%d must be 1..4", c);
    DBX_REQUIRE(M >= 0 && M <= DBX_PATCH_MAX_CAND, "patch_plan: M=%d must be 0..%d", M, DBX_PATCH_MAX_CAND);
    DBX_REQUIRE(n >= 1, "patch_plan: n=%d must be at least 1", n);
    DBX_REQUIRE(neg_frac >= 0.0 && neg_frac <= 1.0, "patch_plan: neg_frac=%g must lie in [0, 1]", neg_frac);
    DBX_REQUIRE(offset_radius >= 0.0 && offset_radius <= 1.0e9, "patch_plan: offset_radius=%g must be finite and not negative",
                offset_radius);
    DBX_REQUIRE(th >= 0, "patch_plan: th=%d is negative", th);
    DBX_REQUIRE((io->cand == nullptr) == (io->draws == nullptr), "patch_plan: cand and draws must both be given (injected mode) or both be null");
    DBX_REQUIRE(io->cand || io->state, "patch_plan: null state in device mode");
    DBX_REQUIRE(io->frames && io->plate0 && (io->plates || n_plates == 0), "patch_plan: null table");
    DBX_REQUIRE(io->jobs && io->labels && io->bbox && io->vertices && io->label && io->count && io->tally, "patch_plan: null output");
    DBX_REQUIRE(M == 0 || (io->status && io->slot && io->cand_out && io->draws_out), "patch_plan: null per-candidate output");
    hipLaunchKernelGGL(patch_plan_kernel, dim3(1), dim3(PATCH_THREADS), 0, (hipStream_t)stream, *io, n_frames, n_plates, c, M, n, neg_frac,
                       offset_radius, th);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_patch_cut(const dbx_patch_job* jobs, const int32_t* count, int32_t n, int32_t c, uint8_t* patches, void* stream) {
    DBX_REQUIRE(n >= 1 && n <= (1 << 24) / PATCH_TILES, "patch_cut: n=%d must be 1..%d", n, (1 << 24) / PATCH_TILES);
    DBX_REQUIRE(c >= 1 && c <= 4, "patch_cut: c=%d must be 1..4", c);
    DBX_REQUIRE(jobs && count && patches, "patch_cut: null argument");
    const ResizeJobDev* dj = (const ResizeJobDev*)jobs;
    const dim3 grid((unsigned)n * PATCH_TILES), block(RSZ_THREADS);
    PATCH_WITH_C(c, hipLaunchKernelGGL(patch_cut_kernel<C>, grid, block, 0, (hipStream_t)stream, dj, count, n, patches));
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_patch_plan_host(int32_t kind, int32_t W, int32_t H, const int32_t* verts, int32_t n_verts, double d0, double d1,
                                   double offset_radius, int32_t th, dbx_patch_geom* out) {
    DBX_REQUIRE(out, "patch_plan_host: null out");
    DBX_REQUIRE(kind == 0 || kind == 1, "patch_plan_host: kind=%d must be 0 (positive) or 1 (negative)", kind);
    DBX_REQUIRE(kind == 0 ? n_verts == 1 : n_verts >= 0, "patch_plan_host: n_verts=%d (1 for a positive, >= 0 for a negative)", n_verts);
    DBX_REQUIRE(verts || n_verts == 0, "patch_plan_host: null verts");
    DBX_REQUIRE(W >= 1 && H >= 1, "patch_plan_host: frame %d x %d must be positive", W, H);
    DBX_REQUIRE(th >= 0, "patch_plan_host: th=%d is negative", th);
    DBX_REQUIRE(offset_radius >= 0.0 && offset_radius <= 1.0e9, "patch_plan_host: offset_radius=%g must be finite and not negative",
                offset_radius);
    if (kind == 0) patch_positive(W, H, verts, d0, d1, offset_radius, out);
    else patch_negative(W, H, verts, n_verts, 8, d0, d1, th, out);
    return DBX_OK;
}

extern "C" int dbx_patch_draw(int64_t seed, int64_t counter, int32_t i0, int32_t count, uint64_t* out) {
    DBX_REQUIRE(out, "patch_draw: null out");
    DBX_REQUIRE(count >= 0 && i0 >= 0, "patch_draw: i0=%d, count=%d must not be negative", i0, count);
    for (int r = 0; r < count; ++r)
        for (int j = 0; j < 4; ++j) out[4 * (size_t)r + j] = patch_hash(seed, counter, i0 + r, j);
    return DBX_OK;
}

extern "C" int dbx_patch_check_tables(const int32_t* plates, int32_t n_plates, const int32_t* plate0, int32_t n_frames, const int32_t* cand,
                                      int32_t M) {
    DBX_REQUIRE(n_frames >= 1, "patch_check_tables: n_frames=%d must be at least 1", n_frames);
    DBX_REQUIRE(n_plates >= 0, "patch_check_tables: n_plates=%d is negative", n_plates);
    DBX_REQUIRE(plate0 && (plates || n_plates == 0), "patch_check_tables: null table");
    for (int p = 0; p < n_plates; ++p) {
        const int f = plates[9 * (size_t)p];
        DBX_REQUIRE(f >= 0 && f < n_frames, "patch_check_tables: plate %d names frame %d of %d", p, f, n_frames);
        DBX_REQUIRE(p == 0 || f >= plates[9 * (size_t)(p - 1)], "patch_check_tables: plates are not sorted by frame (plate %d: frame %d after frame %d)",
                    p, f, plates[9 * (size_t)(p - 1)]);
    }
    int p = 0;
    for (int f = 0; f <= n_frames; ++f) {
        while (p < n_plates && plates[9 * (size_t)p] < f) ++p;
        DBX_REQUIRE(plate0[f] == p, "patch_check_tables: plate0[%d]=%d, but the plates of frame %d start at row %d", f, plate0[f], f, p);
    }
    if (cand) {
        DBX_REQUIRE(M >= 0 && M <= DBX_PATCH_MAX_CAND, "patch_check_tables: M=%d must be 0..%d", M, DBX_PATCH_MAX_CAND);
        for (int i = 0; i < M; ++i) {
            const int kind = cand[2 * i], index = cand[2 * i + 1];
            DBX_REQUIRE(kind == 0 || kind == 1, "patch_check_tables: candidate %d has kind %d (0: positive, 1: negative)", i, kind);
            DBX_REQUIRE(index >= 0 && index < (kind ? n_frames : n_plates), "patch_check_tables: candidate %d (%s) has index %d of %d", i,
                        kind ? "negative" : "positive", index, kind ? n_frames : n_plates);
        }
    }
    return DBX_OK;
}
