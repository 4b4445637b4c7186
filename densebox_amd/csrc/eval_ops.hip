// On-device evaluation behind decode + NMS: detections matched to ground truth (dbx_match_gt_batch) and the (score, TP / FP) records of a
// whole labelled set accumulated in a device arena (dbx_eval_append).  The IoU is the NMS's (post_ops.hip) and must give NumPy's bits,
// so floating-point contraction is OFF in this file: `area_d + area_g - w * h` rounds the product before the subtraction.
#pragma clang fp contract(off)
#include "common.hpp"
#include "det_frame.hpp"

#include <cmath>

#define EVAL_MAX_SLOTS 4096
#define EVAL_MATCH_THREADS 256
#define EVAL_APPEND_THREADS 1024
#define EVAL_NO_CLAIM 0x7fffffff

struct MatchArgs {
    const double* dets; const int* keep; const int* prefix;
    const double* gt; const int* gt_counts; const unsigned char* gt_ignore;
    int* status; int* gt_index; double* iou; double* lm_err; int* tally;
    long long det_rows;
    double iou_thresh;
    int det_cols, slots, gt_cols, max_gt;
};

// One workgroup per frame.  The frame's GT boxes, their areas, ignore flags and one claim word per GT sit in LDS (45 bytes per GT: 45 KB
// at max_gt = 1024).  Pass 1: every list position finds its best GT on its own (jmax does not depend on which GTs are taken) and, when it
// matches a GT that is not ignored, lowers that GT's claim word to its position with an LDS atomicMin.  Pass 2, behind one barrier: a
// position is the TP of its GT when the claim word holds its own number -- the first claimant in list order, what the sequential VOC walk
// marks -- and a duplicate FP otherwise.  A thread re-reads in pass 2 only what it wrote itself in pass 1.
__global__ __launch_bounds__(EVAL_MATCH_THREADS) void match_gt_batch_kernel(const MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ int cnt[4];                     // TP, FP, ignored, GT without the ignore flag
    const int G = a.max_gt, b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    double* gx1 = sm, * gy1 = sm + G, * gx2 = sm + 2 * G, * gy2 = sm + 3 * G, * gar = sm + 4 * G;
    int* claim = (int*)(sm + 5 * G);
    unsigned char* gig = (unsigned char*)(claim + G);
    const int gc = a.gt_counts[b];
    const int g = gc < 0 ? 0 : (gc > G ? G : gc);
    const double* gt = a.gt + (size_t)b * G * a.gt_cols;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    int ngt = 0;
    for (int j = tid; j < g; j += nt) {
        const double* q = gt + (size_t)j * a.gt_cols;
        const double x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
        gx1[j] = x1; gy1[j] = y1; gx2[j] = x2; gy2[j] = y2;
        gar[j] = (x2 - x1 + 1) * (y2 - y1 + 1);
        claim[j] = EVAL_NO_CLAIM;
        const unsigned char ig = a.gt_ignore ? (a.gt_ignore[(size_t)b * G + j] != 0) : 0;
        gig[j] = ig;
        ngt += ig ? 0 : 1;
    }
    if (ngt) atomicAdd(&cnt[3], ngt);
    __syncthreads();
    const DetFrame f = det_frame(a.keep, a.prefix, b, a.slots, a.det_rows);
    const int dc = a.det_cols;
    const double nan = __builtin_nan("");
    for (int i = tid; i < a.slots; i += nt) {
        const size_t o = (size_t)b * a.slots + i;
        if (i >= f.k) { a.status[o] = -2; a.gt_index[o] = -1; continue; }
        const int r = f.kl[1 + i];
        if (r < 0 || r >= f.n) {               // a keep entry outside the frame's rows: not a detection, not counted
            a.status[o] = -2; a.gt_index[o] = -1; a.iou[o] = nan;
            if (a.lm_err) a.lm_err[o] = nan;
            continue;
        }
        const double* d = a.dets + (size_t)(f.r0 + r) * dc;
        const double x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
        const double ad = (x2 - x1 + 1) * (y2 - y1 + 1);
        double best = -INFINITY;
        int jm = -1;
        for (int j = 0; j < g; ++j) {          // every lane reads the same LDS word: a broadcast
            const double xx1 = fmax(x1, gx1[j]), yy1 = fmax(y1, gy1[j]), xx2 = fmin(x2, gx2[j]), yy2 = fmin(y2, gy2[j]);
            const double w = fmax(0.0, xx2 - xx1 + 1), h = fmax(0.0, yy2 - yy1 + 1);
            const double inter = w * h;
            const double ovr = inter / (ad + gar[j] - inter);
            if (ovr > best) { best = ovr; jm = j; }        // strict: the lowest index keeps a tie, NaN never wins
        }
        const bool matched = best > a.iou_thresh;          // strict, as the VOC devkit; implies jm >= 0
        const int st = !matched ? 0 : (gig[jm] ? -1 : 1);
        if (st == 1) atomicMin(&claim[jm], i);
        a.status[o] = st; a.gt_index[o] = matched ? jm : -1; a.iou[o] = best;
    }
    __syncthreads();
    int tp = 0, fp = 0, ign = 0;
    for (int i = tid; i < f.k; i += nt) {
        const size_t o = (size_t)b * a.slots + i;
        int st = a.status[o];
        if (st == -2) continue;
        const int jm = a.gt_index[o];
        if (st == 1 && claim[jm] != i) { st = 0; a.status[o] = 0; }      // an earlier position took the GT: duplicate FP
        if (a.lm_err) {
            double e = nan;
            if (st == 1) {
                const double* d = a.dets + (size_t)(f.r0 + f.kl[1 + i]) * dc + 5;
                const double* q = gt + (size_t)jm * a.gt_cols + 4;
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double dx = d[2 * c] - q[2 * c], dy = d[2 * c + 1] - q[2 * c + 1];
                    s += sqrt(dx * dx + dy * dy);
                }
                e = s / 4.0 / sqrt(gar[jm]);
            }
            a.lm_err[o] = e;
        }
        tp += st == 1; fp += st == 0; ign += st == -1;
    }
    if (tp) atomicAdd(&cnt[0], tp);
    if (fp) atomicAdd(&cnt[1], fp);
    if (ign) atomicAdd(&cnt[2], ign);
    __syncthreads();
    if (tid == 0) {
        int* t = a.tally + (size_t)b * 5;
        t[0] = cnt[0] + cnt[1] + cnt[2]; t[1] = cnt[0]; t[2] = cnt[1]; t[3] = cnt[2]; t[4] = cnt[3];
    }
}

static size_t match_lds_bytes(int max_gt) { return ((size_t)max_gt * (5 * 8 + 4 + 1) + 15) & ~(size_t)15; }

extern "C" int dbx_match_gt_batch(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                                  int32_t batch, int32_t slots, const double* gt, int32_t gt_cols, const int32_t* gt_counts,
                                  const uint8_t* gt_ignore, int32_t max_gt, double iou_thresh, int32_t* status, int32_t* gt_index,
                                  double* iou, double* lm_err, int32_t* tally, void* stream) {
    const int rc = det_rows_check("match_gt_batch", det_cols, det_rows, prefix, batch, slots, EVAL_MAX_SLOTS);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(gt_cols == 4 || gt_cols == 12, "match_gt_batch: gt_cols=%d must be 4 or 12", gt_cols);
    DBX_REQUIRE(max_gt >= 1 && max_gt <= 1024, "match_gt_batch: max_gt=%d must be 1..1024", max_gt);
    DBX_REQUIRE(!std::isnan(iou_thresh), "match_gt_batch: iou_thresh is NaN");
    DBX_REQUIRE(!lm_err || (det_cols == 13 && gt_cols == 12), "match_gt_batch: lm_err needs det_cols 13 and gt_cols 12, got %d and %d", det_cols,
                gt_cols);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(dets && keep && gt && gt_counts && status && gt_index && iou && tally, "match_gt_batch: null argument");
    MatchArgs a;
    a.dets = dets; a.keep = keep; a.prefix = prefix; a.gt = gt; a.gt_counts = gt_counts; a.gt_ignore = gt_ignore;
    a.status = status; a.gt_index = gt_index; a.iou = iou; a.lm_err = lm_err; a.tally = tally;
    a.det_rows = det_rows; a.iou_thresh = iou_thresh; a.det_cols = det_cols; a.slots = slots; a.gt_cols = gt_cols; a.max_gt = max_gt;
    hipLaunchKernelGGL(match_gt_batch_kernel, dim3((unsigned)batch), dim3(EVAL_MATCH_THREADS), match_lds_bytes(max_gt), (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

struct AppendArgs {
    const double* dets; const int* keep; const int* prefix;
    const int* status; const double* lm_err; const int* tally;
    dbx_eval_record* records; long long* state;
    long long det_rows, capacity;
    int det_cols, batch, slots;
};

// ONE workgroup walks the frames in order and each frame's list in chunks of its 1024 threads; a ballot and the waves' totals give every
// counted position its place behind the cursor, so the records land in frame order, then list order, whatever the scheduling.  The state
// is read by every thread before the first barrier and written by thread 0 behind the last one.
__global__ __launch_bounds__(EVAL_APPEND_THREADS) void eval_append_kernel(const AppendArgs a) {
    __shared__ int wsum[EVAL_APPEND_THREADS / 64];
    __shared__ unsigned long long sums[4];               // GT, TP, FP, ignored of the call
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long frame0 = a.state[2];
    long long cur = a.state[0];                          // uniform: every thread keeps the same running cursor
    if (tid < 4) sums[tid] = 0ull;
    __syncthreads();
    unsigned long long t[4] = {0ull, 0ull, 0ull, 0ull};
    for (int b = tid; b < a.batch; b += EVAL_APPEND_THREADS) {
        const int* q = a.tally + (size_t)b * 5;
        t[0] += (unsigned long long)(long long)q[4]; t[1] += (unsigned long long)(long long)q[1];
        t[2] += (unsigned long long)(long long)q[2]; t[3] += (unsigned long long)(long long)q[3];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (t[i]) atomicAdd(&sums[i], t[i]);
    const double nan = __builtin_nan("");
    for (int b = 0; b < a.batch; ++b) {
        const DetFrame f = det_frame(a.keep, a.prefix, b, a.slots, a.det_rows);
        for (int c0 = 0; c0 < f.k; c0 += EVAL_APPEND_THREADS) {
            const int i = c0 + tid;
            const size_t o = (size_t)b * a.slots + i;
            int st = -2, r = -1;
            if (i < f.k) { st = a.status[o]; r = f.kl[1 + i]; }
            const bool valid = st >= -1 && st <= 1 && r >= 0 && r < f.n;
            const unsigned long long m = __ballot(valid);
            if (lane == 0) wsum[wave] = __popcll(m);
            __syncthreads();
            int off = 0, total = 0;
#pragma unroll
            for (int w = 0; w < EVAL_APPEND_THREADS / 64; ++w) { off += w < wave ? wsum[w] : 0; total += wsum[w]; }
            if (valid) {
                const long long at = cur + off + __popcll(m & ((1ull << lane) - 1ull));
                if (at < a.capacity) {
                    dbx_eval_record rec;
                    rec.score = a.dets[(size_t)(f.r0 + r) * a.det_cols + 4];
                    rec.lm_err = a.lm_err ? a.lm_err[o] : nan;
                    rec.status = st;
                    rec.frame = (int)(frame0 + b);
                    a.records[at] = rec;
                }
            }
            cur += total;
            __syncthreads();                             // wsum is rewritten by the next chunk
        }
    }
    __syncthreads();
    if (tid == 0) {
        const long long kept = cur < a.capacity ? cur : a.capacity;
        a.state[0] = kept;
        a.state[1] += cur - kept;
        a.state[2] = frame0 + a.batch;
        a.state[3] += (long long)sums[0]; a.state[4] += (long long)sums[1]; a.state[5] += (long long)sums[2]; a.state[6] += (long long)sums[3];
    }
}

extern "C" int dbx_eval_append(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                               int32_t batch, int32_t slots, const int32_t* status, const double* lm_err, const int32_t* tally,
                               dbx_eval_record* records, int64_t capacity, int64_t* state, void* stream) {
    static_assert(sizeof(dbx_eval_record) == 24, "dbx_eval_record is 24 bytes");
    const int rc = det_rows_check("eval_append", det_cols, det_rows, prefix, batch, slots, EVAL_MAX_SLOTS);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(capacity >= 0, "eval_append: capacity=%lld is negative", (long long)capacity);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(dets && keep && status && tally && state && (records || capacity == 0), "eval_append: null argument");
    AppendArgs a;
    a.dets = dets; a.keep = keep; a.prefix = prefix; a.status = status; a.lm_err = lm_err; a.tally = tally;
    a.records = records; a.state = (long long*)state; a.det_rows = det_rows; a.capacity = capacity;
    a.det_cols = det_cols; a.batch = batch; a.slots = slots;
    hipLaunchKernelGGL(eval_append_kernel, dim3(1), dim3(EVAL_APPEND_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
