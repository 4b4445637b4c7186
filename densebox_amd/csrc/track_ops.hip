// Multi-stream tracking by detection behind decode + NMS: one independent tracker per camera stream, its state on the device, updated by
// one launch per batch (dbx_track_update_batch) and the retired tracks of the call collected in a device arena (dbx_track_append).  The
// IoU is the NMS's (post_ops.hip) and every float64 result is one IEEE operation per written operation, so NumPy gives the same bits:
// floating-point contraction is OFF in this file.
#pragma clang fp contract(off)
#include "common.hpp"
#include "det_frame.hpp"

#include <cmath>

#define TRACK_MAX_SLOTS 1024
#define TRACK_MAX_TRACKS 256
#define TRACK_APPEND_THREADS 256
#define TRACK_NONE 0x7fffffff

struct TrackArgs {
    const double* dets; const int* keep; const int* prefix;
    int* headers; dbx_track* tracks;
    int* track_id; int* track_slot; int* track_hits; dbx_track* retired; int* tally;
    long long det_rows;
    double iou_thresh, alpha, beta, birth_score;
    int det_cols, slots, stream0, max_tracks, max_age;
};

// One workgroup per frame, one thread per track slot (max_tracks rounded up to whole waves), the slot's record in the thread's registers
// from the first read of the table to its one write.  LDS holds what threads exchange: per list position the box, the score and the
// slot the position ended up with (44 bytes: 44 KB at slots = 1024), per track slot its place in the free list, the position born into
// it and its id and hits after the update (16 bytes: 4 KB at max_tracks = 256).
//   A  every live slot predicts in registers.
//   B  the claim walk, sequential in i: every unclaimed live slot computes its overlap with row i (the row is an LDS broadcast), a
//      butterfly over the wave and, with more than one wave, one barrier over double-buffered wave results give every thread the same
//      winner (largest overlap, lowest slot on ties); the winner's thread claims.
//   C  every live slot updates in registers; retired records go out in ascending slot order by a ballot and the waves' totals.
//   D  the j-th unmatched detection that may be born (list order, a ballot prefix per chunk of positions) takes the j-th free slot
//      (ascending, slots freed in C included): what the sequential walk gives, since both sides only ever take the lowest one left.
__global__ __launch_bounds__(TRACK_MAX_TRACKS) void track_update_batch_kernel(const TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red_v[2][TRACK_MAX_TRACKS / 64];
    __shared__ int red_s[2][TRACK_MAX_TRACKS / 64];
    __shared__ int wsum[4][TRACK_MAX_TRACKS / 64];       // per wave: retired, free, claimed slots; eligible positions of a chunk
    __shared__ int cnt[2];                               // unborn, counted positions
    const int S = a.slots, T = a.max_tracks, b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    double* dx1 = sm, * dy1 = sm + S, * dx2 = sm + 2 * S, * dy2 = sm + 3 * S, * dsc = sm + 4 * S;
    int* asg = (int*)(sm + 5 * S);                       // -2 not counted, -1 no track (yet), else the slot
    int* freel = asg + S;
    int* born = freel + T;
    int* lid = born + T;
    int* lhits = lid + T;

    int* hdr = a.headers + (size_t)(a.stream0 + b) * 4;
    dbx_track* tab = a.tracks + (size_t)(a.stream0 + b) * T;
    const int f = hdr[0], next_id = hdr[1], unborn0 = hdr[2];      // read by every thread here, written by thread 0 behind the last barrier
    const bool own = tid < T;
    dbx_track t;
    t.id = -1;
    if (own) t = tab[tid];
    const int id0 = t.id;
    const bool live = own && id0 >= 0;

    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const DetFrame fr = det_frame(a.keep, a.prefix, b, S, a.det_rows);
    int counted = 0;
    for (int i = tid; i < fr.k; i += nt) {
        const int r = fr.kl[1 + i];
        if (r < 0 || r >= fr.n) { asg[i] = -2; continue; }        // a keep entry outside the frame's rows: not a detection, not counted
        const double* d = a.dets + (size_t)(fr.r0 + r) * a.det_cols;
        dx1[i] = d[0]; dy1[i] = d[1]; dx2[i] = d[2]; dy2[i] = d[3]; dsc[i] = d[4];
        asg[i] = -1;
        ++counted;
    }
    if (counted) atomicAdd(&cnt[1], counted);
    // A
    double p[4] = {0.0, 0.0, 0.0, 0.0}, par = 0.0;
    if (live) {
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = t.box[c] + t.vel[c];
        par = (p[2] - p[0] + 1) * (p[3] - p[1] + 1);
    }
    __syncthreads();
    // B
    int claim = -1, it = 0;
    for (int i = 0; i < fr.k; ++i) {
        if (asg[i] == -2) continue;                                // uniform: every thread reads the same word
        double v = -INFINITY;
        int s = TRACK_NONE;
        if (live && claim < 0) {
            const double x1 = dx1[i], y1 = dy1[i], x2 = dx2[i], y2 = dy2[i];
            const double ad = (x2 - x1 + 1) * (y2 - y1 + 1);
            const double xx1 = fmax(p[0], x1), yy1 = fmax(p[1], y1), xx2 = fmin(p[2], x2), yy2 = fmin(p[3], y2);
            const double w = fmax(0.0, xx2 - xx1 + 1), h = fmax(0.0, yy2 - yy1 + 1);
            const double inter = w * h;
            const double ovr = inter / (par + ad - inter);
            if (ovr > -INFINITY) { v = ovr; s = tid; }             // a NaN never wins
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const double ov = __shfl_xor(v, off);
            const int os = __shfl_xor(s, off);
            if (ov > v || (ov == v && os < s)) { v = ov; s = os; }
        }
        if (nw > 1) {                                              // the buffer of executed step `it` is rewritten in step it + 2, behind
            const int buf = it & 1;                                // the barrier of step it + 1
            if (lane == 0) { red_v[buf][wave] = v; red_s[buf][wave] = s; }
            __syncthreads();
            v = red_v[buf][0]; s = red_s[buf][0];
            for (int w = 1; w < nw; ++w) {
                const double ov = red_v[buf][w];
                const int os = red_s[buf][w];
                if (ov > v || (ov == v && os < s)) { v = ov; s = os; }
            }
        }
        ++it;
        if (s == tid && v > a.iou_thresh) { claim = i; asg[i] = tid; }     // strict
    }
    __syncthreads();
    // C
    bool retire = false;
    if (live) {
        if (claim >= 0) {
            const double q[4] = {dx1[claim], dy1[claim], dx2[claim], dy2[claim]};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double r = q[c] - p[c];
                t.box[c] = p[c] + a.alpha * r;
                t.vel[c] = t.vel[c] + a.beta * r;
            }
            const double sc = dsc[claim];
            t.score = sc;
            if (sc > t.best_score) { t.best_score = sc; t.best_frame = f; }
            t.hits += 1; t.age = 0; t.last_frame = f;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) t.box[c] = p[c];
            t.age += 1;
            retire = t.age > a.max_age;
        }
    }
    const unsigned long long m_ret = __ballot(retire);
    if (retire) t.id = -1;                                         // the record goes out with the id it lived under, below
    const bool isfree = own && t.id < 0;
    const unsigned long long m_free = __ballot(isfree), m_clm = __ballot(claim >= 0);
    if (lane == 0) { wsum[0][wave] = __popcll(m_ret); wsum[1][wave] = __popcll(m_free); wsum[2][wave] = __popcll(m_clm); }
    if (own) born[tid] = -1;
    __syncthreads();
    int ret_off = 0, n_ret = 0, free_off = 0, n_free = 0, n_matched = 0;
    for (int w = 0; w < nw; ++w) {
        ret_off += w < wave ? wsum[0][w] : 0; n_ret += wsum[0][w];
        free_off += w < wave ? wsum[1][w] : 0; n_free += wsum[1][w];
        n_matched += wsum[2][w];
    }
    const int frank = free_off + __popcll(m_free & below);         // this slot's place among the free ones, ascending
    if (isfree) freel[frank] = tid;
    if (retire) {
        dbx_track out = t;
        out.id = id0;
        a.retired[(size_t)b * T + ret_off + __popcll(m_ret & below)] = out;
    }
    __syncthreads();
    // D
    int ebase = 0, unb = 0;
    for (int c0 = 0; c0 < fr.k; c0 += nt) {
        const int i = c0 + tid;
        const bool unm = i < fr.k && asg[i] == -1;
        bool elig = false;
        if (unm) elig = isfinite(dx1[i]) && isfinite(dy1[i]) && isfinite(dx2[i]) && isfinite(dy2[i]) && dsc[i] >= a.birth_score;
        const unsigned long long m_e = __ballot(elig);
        if (lane == 0) wsum[3][wave] = __popcll(m_e);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < nw; ++w) { off += w < wave ? wsum[3][w] : 0; total += wsum[3][w]; }
        if (elig) {
            const int j = ebase + off + __popcll(m_e & below);
            if (j < n_free) { const int s = freel[j]; born[s] = i; asg[i] = s; }
            else ++unb;
        } else if (unm) {
            ++unb;
        }
        ebase += total;
        __syncthreads();                                           // wsum[3] is rewritten by the next chunk; born and asg are read below
    }
    const int n_born = ebase < n_free ? ebase : n_free;
    if (unb) atomicAdd(&cnt[0], unb);
    if (isfree && born[tid] >= 0) {
        const int i = born[tid];
        t.box[0] = dx1[i]; t.box[1] = dy1[i]; t.box[2] = dx2[i]; t.box[3] = dy2[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) t.vel[c] = 0.0;
        t.score = t.best_score = dsc[i];
        t.id = next_id + frank;
        t.hits = 1; t.age = 0;
        t.first_frame = t.last_frame = t.best_frame = f;
    }
    if (own) { tab[tid] = t; lid[tid] = t.id; lhits[tid] = t.hits; }
    __syncthreads();
    for (int i = tid; i < S; i += nt) {
        const size_t o = (size_t)b * S + i;
        if (i >= fr.k) { a.track_id[o] = -2; a.track_slot[o] = -1; continue; }
        const int s = asg[i];
        a.track_id[o] = s >= 0 ? lid[s] : (s == -2 ? -2 : -1);
        a.track_slot[o] = s >= 0 ? s : -1;
        a.track_hits[o] = s >= 0 ? lhits[s] : 0;
    }
    if (tid == 0) {
        int* q = a.tally + (size_t)b * 6;
        q[0] = cnt[1]; q[1] = n_matched; q[2] = n_born; q[3] = cnt[0]; q[4] = n_ret; q[5] = T - n_free + n_born;
        hdr[0] = f + 1; hdr[1] = next_id + n_born; hdr[2] = unborn0 + cnt[0];
    }
}

static size_t track_lds_bytes(int slots, int max_tracks) { return ((size_t)slots * (5 * 8 + 4) + (size_t)max_tracks * 16 + 15) & ~(size_t)15; }

extern "C" int dbx_track_update_batch(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                                      int32_t batch, int32_t slots, int32_t* headers, dbx_track* tracks, int32_t streams, int32_t stream0,
                                      int32_t max_tracks, double iou_thresh, int32_t max_age, double alpha, double beta, double birth_score,
                                      int32_t* track_id, int32_t* track_slot, int32_t* track_hits, dbx_track* retired, int32_t* tally,
                                      void* stream) {
    static_assert(sizeof(dbx_track) == 104, "dbx_track is 104 bytes");
    const char* fn = "track_update_batch";
    const int rc = det_rows_check(fn, det_cols, det_rows, prefix, batch, slots, TRACK_MAX_SLOTS);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(stream0 >= 0 && streams >= 0 && (int64_t)stream0 + batch <= streams, "%s: streams %d..%lld are not all in 0..%d", fn, stream0,
                (long long)stream0 + batch - 1, streams - 1);
    DBX_REQUIRE(max_tracks >= 1 && max_tracks <= TRACK_MAX_TRACKS, "%s: max_tracks=%d must be 1..%d", fn, max_tracks, TRACK_MAX_TRACKS);
    DBX_REQUIRE(max_age >= 0, "%s: max_age=%d is negative", fn, max_age);
    DBX_REQUIRE(!std::isnan(iou_thresh) && !std::isnan(alpha) && !std::isnan(beta) && !std::isnan(birth_score),
                "%s: iou_thresh, alpha, beta and birth_score must not be NaN", fn);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(dets && keep && headers && tracks && track_id && track_slot && track_hits && retired && tally, "%s: null argument", fn);
    TrackArgs a;
    a.dets = dets; a.keep = keep; a.prefix = prefix; a.headers = headers; a.tracks = tracks;
    a.track_id = track_id; a.track_slot = track_slot; a.track_hits = track_hits; a.retired = retired; a.tally = tally;
    a.det_rows = det_rows; a.iou_thresh = iou_thresh; a.alpha = alpha; a.beta = beta; a.birth_score = birth_score;
    a.det_cols = det_cols; a.slots = slots; a.stream0 = stream0; a.max_tracks = max_tracks; a.max_age = max_age;
    const unsigned threads = (unsigned)((max_tracks + 63) / 64 * 64);
    hipLaunchKernelGGL(track_update_batch_kernel, dim3((unsigned)batch), dim3(threads), track_lds_bytes(slots, max_tracks), (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

struct TrackAppendArgs {
    const dbx_track* retired; const int* tally;
    dbx_track_record* records; long long* state;
    long long capacity;
    int batch, max_tracks, stream0;
};

// ONE workgroup walks the frames in order with the same running cursor in every thread, a thread per retired record of the frame
// (at most 256), so the records land in frame order, then `retired` order, whatever the scheduling.  The state is read by every thread
// before the first barrier and written by thread 0 behind the last one.
__global__ __launch_bounds__(TRACK_APPEND_THREADS) void track_append_kernel(const TrackAppendArgs a) {
    const int tid = threadIdx.x, T = a.max_tracks;
    const long long start = a.state[0];
    long long cur = start;
    for (int b = 0; b < a.batch; ++b) {
        const int c = a.tally[(size_t)b * 6 + 4];
        const int n = c < 0 ? 0 : (c > T ? T : c);
        for (int j = tid; j < n; j += TRACK_APPEND_THREADS) {
            const long long at = cur + j;
            if (at >= 0 && at < a.capacity) {
                // thirteen 8-byte words of the track behind one that holds (stream, reserved = 0): no copy of the record on the stack
                const unsigned long long* src = (const unsigned long long*)(a.retired + (size_t)b * T + j);
                unsigned long long* dst = (unsigned long long*)(a.records + at);
                dst[0] = (unsigned long long)(unsigned)(a.stream0 + b);
#pragma unroll
                for (int w = 0; w < 13; ++w) dst[1 + w] = src[w];
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

extern "C" int dbx_track_append(const dbx_track* retired, const int32_t* tally, int32_t batch, int32_t max_tracks, int32_t stream0,
                                dbx_track_record* records, int64_t capacity, int64_t* state, void* stream) {
    static_assert(sizeof(dbx_track_record) == 112, "dbx_track_record is 112 bytes");
    const char* fn = "track_append";
    DBX_REQUIRE(batch >= 0, "%s: batch=%d is negative", fn, batch);
    DBX_REQUIRE(stream0 >= 0, "%s: stream0=%d is negative", fn, stream0);
    DBX_REQUIRE(max_tracks >= 1 && max_tracks <= TRACK_MAX_TRACKS, "%s: max_tracks=%d must be 1..%d", fn, max_tracks, TRACK_MAX_TRACKS);
    DBX_REQUIRE(capacity >= 0, "%s: capacity=%lld is negative", fn, (long long)capacity);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(retired && tally && state && (records || capacity == 0), "%s: null argument", fn);
    TrackAppendArgs a;
    a.retired = retired; a.tally = tally; a.records = records; a.state = (long long*)state; a.capacity = capacity;
    a.batch = batch; a.max_tracks = max_tracks; a.stream0 = stream0;
    hipLaunchKernelGGL(track_append_kernel, dim3(1), dim3(TRACK_APPEND_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
