// Zones behind the tracker: a region-of-interest filter on the keep lists in front of dbx_track_update_batch (dbx_zone_filter_keep), line
// crossings and region events of the tracks behind it (dbx_zone_update_batch) and the events of the call collected in a device arena
// (dbx_zone_append).  The geometry is zone_geom.hpp's, integer but for the anchor, whose float64 results are one IEEE operation per
// written operation so that NumPy gives the same bits: floating-point contraction is OFF in this file.
#pragma clang fp contract(off)
#include "common.hpp"
#include "det_frame.hpp"
#include "zone_geom.hpp"

#include <cstddef>

#define ZONE_MAX_SLOTS 1024
#define ZONE_MAX_TRACKS 256
#define ZONE_THREADS 256
#define ZONE_N 8                         // lines, regions and mask polygons per stream
#define ZONE_EVENTS_PER_SLOT 24          // 8 ended inside + 8 crossings + 8 transitions
#define ZONE_POLY_WORDS 34
#define ZONE_CFG_WORDS 580

static_assert(sizeof(dbx_zone_line) == 16 && sizeof(dbx_zone_poly) == 136 && offsetof(dbx_zone_poly, xy) == 8, "dbx_zone_poly is 136 bytes");
static_assert(sizeof(dbx_zone_config) == 2320 && offsetof(dbx_zone_config, lines) == 16 && offsetof(dbx_zone_config, regions) == 144 &&
              offsetof(dbx_zone_config, masks) == 1232, "dbx_zone_config is 2320 bytes");
static_assert(sizeof(dbx_zone_state) == 32 && offsetof(dbx_zone_state, inside) == 16, "dbx_zone_state is 32 bytes");
static_assert(sizeof(dbx_zone_event) == 32 && offsetof(dbx_zone_event, ax) == 24, "dbx_zone_event is 32 bytes");
static_assert(sizeof(dbx_zone_config) == ZONE_CFG_WORDS * 4 && sizeof(dbx_zone_poly) == ZONE_POLY_WORDS * 4, "word counts");

__device__ static inline int zone_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A table in device memory is data: a polygon's vertex count is clamped to 0..16 and every coordinate to +-2^20 on the way to LDS, so
// the geometry's int64 products stay exact whatever the table holds.  w: the word's index within the dbx_zone_poly.
__device__ static inline int zone_poly_word(int w, int v) {
    return w == 0 ? zone_clamp(v, 0, ZONE_MAX_VERTS) : (w == 1 ? v : zone_clamp(v, -ZONE_COORD_MAX, ZONE_COORD_MAX));
}

// ---------------------------------------------------------------------------------------------------------------- filter
struct ZoneFilterArgs {
    const double* dets; const int* keep; const int* prefix; const dbx_zone_config* config;
    int* keep_out; int* stats;
    long long det_rows;
    int det_cols, slots, stream0, anchor;
};

// One workgroup per frame.  LDS: the stream's 8 mask polygons (1088 bytes) and four wave totals.  The list is walked 256 positions at a
// time; a ballot prefix per chunk keeps the survivors in order.
__global__ __launch_bounds__(ZONE_THREADS) void zone_filter_kernel(const ZoneFilterArgs a) {
    __shared__ int masks[ZONE_N * ZONE_POLY_WORDS];
    __shared__ int wsum[ZONE_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const dbx_zone_config* cfg = a.config + (size_t)(a.stream0 + b);
    const int nm = zone_clamp(cfg->n_masks, 0, ZONE_N);
    const int* src = (const int*)cfg->masks;
    for (int i = tid; i < ZONE_N * ZONE_POLY_WORDS; i += ZONE_THREADS) masks[i] = zone_poly_word(i % ZONE_POLY_WORDS, src[i]);
    __syncthreads();
    bool has_inc = false;
    for (int m = 0; m < ZONE_N; ++m) has_inc |= m < nm && masks[m * ZONE_POLY_WORDS + 1] != 1;

    const DetFrame fr = det_frame(a.keep, a.prefix, b, a.slots, a.det_rows);
    bool good = true;                                    // a corrupt prefix pair: the frame has no list, and none is written
    if (a.prefix) {
        const long long p0 = a.prefix[b], p1 = a.prefix[b + 1];
        good = p0 >= 0 && p1 >= p0 && p1 <= a.det_rows;
    }
    const int ext = (int)(fr.n < a.slots ? fr.n : a.slots);       // the list positions det_frame allows
    int* out = a.keep_out + (fr.kl - a.keep);
    int after = 0;
    if (nm == 0) {
        for (int i = tid; i < fr.k; i += ZONE_THREADS) out[1 + i] = fr.kl[1 + i];
        after = fr.k;
    } else {
        for (int c0 = 0; c0 < fr.k; c0 += ZONE_THREADS) {
            const int i = c0 + tid;
            bool pass = false;
            int r = 0;
            if (i < fr.k) {
                r = fr.kl[1 + i];
                if (r >= 0 && r < fr.n) {
                    const double* d = a.dets + (size_t)(fr.r0 + r) * a.det_cols;
                    const ZoneAnchor p = zone_anchor(d[0], d[1], d[2], d[3], a.anchor);
                    if (p.ok) {
                        bool inc = false, exc = false;
                        for (int m = 0; m < ZONE_N; ++m) {
                            if (m >= nm) break;
                            const int* poly = masks + m * ZONE_POLY_WORDS;
                            const bool in = zone_inside(poly + 2, poly[0], p.x, p.y);
                            if (poly[1] == 1) exc |= in; else inc |= in;
                        }
                        pass = (!has_inc || inc) && !exc;
                    }
                }
            }
            const unsigned long long m_p = __ballot(pass);
            if (lane == 0) wsum[wave] = __popcll(m_p);
            __syncthreads();
            int off = 0, total = 0;
            for (int w = 0; w < ZONE_THREADS / 64; ++w) { off += w < wave ? wsum[w] : 0; total += wsum[w]; }
            if (pass) out[1 + after + off + __popcll(m_p & below)] = r;
            after += total;
            __syncthreads();                             // wsum is rewritten by the next chunk
        }
    }
    if (good) {
        for (int i = after + tid; i < ext; i += ZONE_THREADS) out[1 + i] = 0;
        if (tid == 0) out[0] = after;
    }
    if (tid == 0) { a.stats[2 * b] = fr.k; a.stats[2 * b + 1] = after; }
}

static int zone_streams_check(const char* fn, int32_t batch, int32_t streams, int32_t stream0) {
    DBX_REQUIRE(stream0 >= 0 && streams >= 0 && (int64_t)stream0 + batch <= streams, "%s: streams %d..%lld are not all in 0..%d", fn, stream0,
                (long long)stream0 + batch - 1, streams - 1);
    return DBX_OK;
}

extern "C" int dbx_zone_filter_keep(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                                    int32_t batch, int32_t slots, const dbx_zone_config* config, int32_t streams, int32_t stream0,
                                    int32_t anchor, int32_t* keep_out, int32_t* stats, void* stream) {
    const char* fn = "zone_filter_keep";
    int rc = det_rows_check(fn, det_cols, det_rows, prefix, batch, slots, ZONE_MAX_SLOTS);
    if (rc != DBX_OK) return rc;
    rc = zone_streams_check(fn, batch, streams, stream0);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(anchor == 0 || anchor == 1, "%s: anchor=%d must be 0 (centre) or 1 (bottom)", fn, anchor);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(dets && keep && config && keep_out && stats, "%s: null argument", fn);
    DBX_REQUIRE(keep_out != keep, "%s: keep_out must not be keep", fn);
    ZoneFilterArgs a;
    a.dets = dets; a.keep = keep; a.prefix = prefix; a.config = config; a.keep_out = keep_out; a.stats = stats;
    a.det_rows = det_rows; a.det_cols = det_cols; a.slots = slots; a.stream0 = stream0; a.anchor = anchor;
    hipLaunchKernelGGL(zone_filter_kernel, dim3((unsigned)batch), dim3(ZONE_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- update
struct ZoneUpdateArgs {
    const dbx_track* tracks; const int* headers; const dbx_zone_config* config;
    dbx_zone_state* state; long long* line_counts; long long* region_counts;
    dbx_zone_event* staged; int* staged_count;
    int stream0, max_tracks, min_hits, anchor, commit;
};

__device__ static inline void zone_emit(dbx_zone_event* e, int stream, int id, int kind, int index, int frame, int hits, int ax, int ay) {
    int4* q = (int4*)e;                                  // 32 bytes, 32-byte aligned
    q[0] = make_int4(stream, id, kind, index);
    q[1] = make_int4(frame, hits, ax, ay);
}

// One workgroup per frame, one thread per track slot (max_tracks rounded up to whole waves).  LDS: the stream's table (2320 bytes), the
// 40 counter deltas of the frame and four wave totals.  Every thread works out its slot's events as bit masks, an inclusive scan over
// the workgroup gives the slot its place in the frame's staging, and the events go out in slot order.
__global__ __launch_bounds__(ZONE_MAX_TRACKS) void zone_update_kernel(const ZoneUpdateArgs a) {
    __shared__ int cfg[ZONE_CFG_WORDS];
    __shared__ int ctr[ZONE_N * 5];
    __shared__ int wtot[ZONE_MAX_TRACKS / 64];
    const int T = a.max_tracks, b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, s = a.stream0 + b;
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int* src = (const int*)(a.config + (size_t)s);
    for (int i = tid; i < ZONE_CFG_WORDS; i += nt) {
        const int v = src[i];
        int o;
        if (i < 4) o = zone_clamp(v, 0, ZONE_N);
        else if (i < 36) o = zone_clamp(v, -ZONE_COORD_MAX, ZONE_COORD_MAX);
        else o = zone_poly_word((i - 36) % ZONE_POLY_WORDS, v);
        cfg[i] = o;
    }
    if (tid < ZONE_N * 5) ctr[tid] = 0;
    __syncthreads();
    const int nl = cfg[0], nr = cfg[1];
    const int* lines = cfg + 4;
    const int* regions = cfg + 36;
    const int f = a.headers[(size_t)s * 4] - 1;
    const bool own = tid < T;
    dbx_zone_state st;
    st.owner_id = -1; st.has_prev = 0; st.px = 0; st.py = 0; st.inside = 0;
    st.reserved[0] = st.reserved[1] = st.reserved[2] = 0;
    int id = -1, hits = 0;
    const dbx_track* trk = a.tracks + (size_t)s * T + tid;
    if (own) { st = a.state[(size_t)s * T + tid]; id = trk->id; hits = trk->hits; }

    // 1  the owner left the slot
    unsigned ended = 0;
    const int old_id = st.owner_id, old_x = st.px, old_y = st.py;
    if (own && st.owner_id >= 0 && id != st.owner_id) {
        ended = (unsigned)st.inside & 0xffu;
        st.owner_id = -1; st.has_prev = 0; st.px = 0; st.py = 0; st.inside = 0;
    }
    // 2, 3  crossings and transitions of a live slot that qualifies
    unsigned fwd = 0, bwd = 0, trans = 0;
    ZoneAnchor p;
    p.ok = 0; p.x = p.y = 0;
    if (own && id >= 0 && hits >= a.min_hits) {
        if (id != st.owner_id) { st.owner_id = id; st.has_prev = 0; st.inside = 0; }
        p = zone_anchor(trk->box[0], trk->box[1], trk->box[2], trk->box[3], a.anchor);
        if (p.ok) {
            if (st.has_prev) {
                for (int l = 0; l < ZONE_N; ++l) {
                    if (l >= nl) break;
                    const int c = zone_crossing(lines[4 * l], lines[4 * l + 1], lines[4 * l + 2], lines[4 * l + 3], st.px, st.py, p.x, p.y);
                    if (c == 0) fwd |= 1u << l;
                    if (c == 1) bwd |= 1u << l;
                }
            }
            for (int r = 0; r < ZONE_N; ++r) {
                if (r >= nr) break;
                const int* poly = regions + r * ZONE_POLY_WORDS;
                const unsigned in = zone_inside(poly + 2, poly[0], p.x, p.y) ? 1u : 0u;
                if (in != (((unsigned)st.inside >> r) & 1u)) trans |= 1u << r;
            }
            st.inside = (int)((unsigned)st.inside ^ trans);
            st.px = p.x; st.py = p.y; st.has_prev = 1;
        } else {
            st.has_prev = 0;
        }
    }
    const int mine = __popc(ended) + __popc(fwd | bwd) + __popc(trans);
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < nw; ++w) { base += w < wave ? wtot[w] : 0; total += wtot[w]; }
    if (a.commit && own) {
        // base + incl <= 24 * (tid + 1) <= 24 * max_tracks: inside the frame's staging
        dbx_zone_event* e = a.staged + (size_t)b * T * ZONE_EVENTS_PER_SLOT + base + incl - mine;
        for (int r = 0; r < ZONE_N; ++r)
            if (ended >> r & 1u) {
                zone_emit(e++, s, old_id, 4, r, f, 0, old_x, old_y);
                atomicAdd(&ctr[16 + 3 * r + 1], 1); atomicAdd(&ctr[16 + 3 * r + 2], -1);
            }
        for (int l = 0; l < ZONE_N; ++l)
            if ((fwd | bwd) >> l & 1u) {
                const int k = bwd >> l & 1u;
                zone_emit(e++, s, id, k, l, f, hits, p.x, p.y);
                atomicAdd(&ctr[2 * l + k], 1);
            }
        for (int r = 0; r < ZONE_N; ++r)
            if (trans >> r & 1u) {
                const int now = (unsigned)st.inside >> r & 1u;
                zone_emit(e++, s, id, now ? 2 : 3, r, f, hits, p.x, p.y);
                atomicAdd(&ctr[16 + 3 * r + (now ? 0 : 1)], 1); atomicAdd(&ctr[16 + 3 * r + 2], now ? 1 : -1);
            }
        a.state[(size_t)s * T + tid] = st;
    }
    __syncthreads();
    if (a.commit) {                                      // this workgroup is the only one that touches stream s
        if (tid < 16) a.line_counts[(size_t)s * 16 + tid] += ctr[tid];
        else if (tid < 40) a.region_counts[(size_t)s * 24 + tid - 16] += ctr[tid];
        if (tid == 0) a.staged_count[b] = total;
    }
}

extern "C" int dbx_zone_update_batch(const dbx_track* tracks, const int32_t* headers, const dbx_zone_config* config, dbx_zone_state* state,
                                     int64_t* line_counts, int64_t* region_counts, int32_t batch, int32_t streams, int32_t stream0,
                                     int32_t max_tracks, int32_t min_hits, int32_t anchor, dbx_zone_event* staged, int32_t* staged_count,
                                     int32_t commit, void* stream) {
    const char* fn = "zone_update_batch";
    DBX_REQUIRE(batch >= 0, "%s: batch=%d is negative", fn, batch);
    const int rc = zone_streams_check(fn, batch, streams, stream0);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(max_tracks >= 1 && max_tracks <= ZONE_MAX_TRACKS, "%s: max_tracks=%d must be 1..%d", fn, max_tracks, ZONE_MAX_TRACKS);
    DBX_REQUIRE(min_hits >= 1, "%s: min_hits=%d must be at least 1", fn, min_hits);
    DBX_REQUIRE(anchor == 0 || anchor == 1, "%s: anchor=%d must be 0 (centre) or 1 (bottom)", fn, anchor);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(tracks && headers && config && state && line_counts && region_counts && staged && staged_count, "%s: null argument", fn);
    ZoneUpdateArgs a;
    a.tracks = tracks; a.headers = headers; a.config = config; a.state = state; a.line_counts = (long long*)line_counts;
    a.region_counts = (long long*)region_counts; a.staged = staged; a.staged_count = staged_count;
    a.stream0 = stream0; a.max_tracks = max_tracks; a.min_hits = min_hits; a.anchor = anchor; a.commit = commit != 0;
    const unsigned threads = (unsigned)((max_tracks + 63) / 64 * 64);
    hipLaunchKernelGGL(zone_update_kernel, dim3((unsigned)batch), dim3(threads), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- append
struct ZoneAppendArgs {
    const dbx_zone_event* staged; const int* staged_count;
    dbx_zone_event* events; long long* state;
    long long capacity;
    int batch, max_tracks;
};

// dbx_track_append's walk: ONE workgroup, the frames in order with the same running cursor in every thread, so the events land in frame
// order, then staging order.  The state is read by every thread before the barrier and written by thread 0 behind it.
__global__ __launch_bounds__(ZONE_THREADS) void zone_append_kernel(const ZoneAppendArgs a) {
    const int tid = threadIdx.x, room = a.max_tracks * ZONE_EVENTS_PER_SLOT;
    const long long start = a.state[0];
    long long cur = start;
    for (int b = 0; b < a.batch; ++b) {
        const int c = a.staged_count[b];
        const int n = c < 0 ? 0 : (c > room ? room : c);
        for (int j = tid; j < n; j += ZONE_THREADS) {
            const long long at = cur + j;
            if (at >= 0 && at < a.capacity) {
                const int4* src = (const int4*)(a.staged + (size_t)b * room + j);
                int4* dst = (int4*)(a.events + at);
                dst[0] = src[0]; dst[1] = src[1];
            }
        }
        cur += n;
    }
    __syncthreads();
    if (tid == 0) {
        const long long kept = cur < a.capacity ? cur : a.capacity;
        a.state[0] = kept;
        a.state[1] += cur - kept;
        a.state[2] += cur - start;
    }
}

extern "C" int dbx_zone_append(const dbx_zone_event* staged, const int32_t* staged_count, int32_t batch, int32_t max_tracks,
                               dbx_zone_event* events, int64_t capacity, int64_t* state, void* stream) {
    const char* fn = "zone_append";
    DBX_REQUIRE(batch >= 0, "%s: batch=%d is negative", fn, batch);
    DBX_REQUIRE(max_tracks >= 1 && max_tracks <= ZONE_MAX_TRACKS, "%s: max_tracks=%d must be 1..%d", fn, max_tracks, ZONE_MAX_TRACKS);
    DBX_REQUIRE(capacity >= 0, "%s: capacity=%lld is negative", fn, (long long)capacity);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(staged && staged_count && state && (events || capacity == 0), "%s: null argument", fn);
    ZoneAppendArgs a;
    a.staged = staged; a.staged_count = staged_count; a.events = events; a.state = (long long*)state; a.capacity = capacity;
    a.batch = batch; a.max_tracks = max_tracks;
    hipLaunchKernelGGL(zone_append_kernel, dim3(1), dim3(ZONE_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int zone_poly_check(const char* fn, const char* what, int i, const dbx_zone_poly& p, bool mask) {
    DBX_REQUIRE(p.n >= 3 && p.n <= ZONE_MAX_VERTS, "%s: %s %d has %d vertices, not 3..%d", fn, what, i, p.n, ZONE_MAX_VERTS);
    DBX_REQUIRE(mask ? (p.role == 0 || p.role == 1) : p.role == 0, "%s: %s %d has role %d", fn, what, i, p.role);
    for (int v = 0; v < 2 * p.n; ++v)
        DBX_REQUIRE(p.xy[v] >= -ZONE_COORD_MAX && p.xy[v] <= ZONE_COORD_MAX, "%s: %s %d has a coordinate %d beyond 2^20 quarter pixels", fn,
                    what, i, p.xy[v]);
    return DBX_OK;
}

extern "C" int dbx_zone_check_config(const dbx_zone_config* config) {
    const char* fn = "zone_check_config";
    DBX_REQUIRE(config, "%s: null argument", fn);
    const dbx_zone_config& c = *config;
    DBX_REQUIRE(c.n_lines >= 0 && c.n_lines <= ZONE_N, "%s: n_lines=%d must be 0..%d", fn, c.n_lines, ZONE_N);
    DBX_REQUIRE(c.n_regions >= 0 && c.n_regions <= ZONE_N, "%s: n_regions=%d must be 0..%d", fn, c.n_regions, ZONE_N);
    DBX_REQUIRE(c.n_masks >= 0 && c.n_masks <= ZONE_N, "%s: n_masks=%d must be 0..%d", fn, c.n_masks, ZONE_N);
    for (int l = 0; l < c.n_lines; ++l) {
        const dbx_zone_line& q = c.lines[l];
        const int v[4] = {q.ax, q.ay, q.bx, q.by};
        for (int k = 0; k < 4; ++k)
            DBX_REQUIRE(v[k] >= -ZONE_COORD_MAX && v[k] <= ZONE_COORD_MAX, "%s: line %d has a coordinate %d beyond 2^20 quarter pixels", fn, l,
                        v[k]);
        DBX_REQUIRE(q.ax != q.bx || q.ay != q.by, "%s: line %d has A == B", fn, l);
    }
    for (int r = 0; r < c.n_regions; ++r) {
        const int rc = zone_poly_check(fn, "region", r, c.regions[r], false);
        if (rc != DBX_OK) return rc;
    }
    for (int m = 0; m < c.n_masks; ++m) {
        const int rc = zone_poly_check(fn, "mask", m, c.masks[m], true);
        if (rc != DBX_OK) return rc;
    }
    return DBX_OK;
}

extern "C" int dbx_zone_host(int32_t op, int64_t n, const double* boxes, const int32_t* ints, int32_t* out) {
    const char* fn = "zone_host";
    DBX_REQUIRE(op >= 0 && op <= 4, "%s: op=%d must be 0..4", fn, op);
    DBX_REQUIRE(n >= 0, "%s: n=%lld is negative", fn, (long long)n);
    if (n == 0) return DBX_OK;
    DBX_REQUIRE(out && (op <= 1 ? boxes != nullptr : ints != nullptr), "%s: null argument", fn);
    for (int64_t i = 0; i < n; ++i) {
        if (op <= 1) {
            const double* q = boxes + 4 * i;
            const ZoneAnchor p = zone_anchor(q[0], q[1], q[2], q[3], op);
            out[3 * i] = p.ok; out[3 * i + 1] = p.x; out[3 * i + 2] = p.y;
        } else if (op == 2) {
            const int32_t* q = ints + 6 * i;
            out[i] = zone_side(q[0], q[1], q[2], q[3], q[4], q[5]) ? 1 : 0;
        } else if (op == 3) {
            const int32_t* q = ints + 8 * i;
            out[i] = zone_crossing(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
        } else {
            const int32_t* q = ints + 35 * i;
            out[i] = zone_inside(q + 3, q[2], q[0], q[1]) ? 1 : 0;
        }
    }
    return DBX_OK;
}
