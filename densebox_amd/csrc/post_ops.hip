// SGD(momentum, weight decay) multi-tensor update and the inference tail: top-K decode + greedy NMS.
// Index bookkeeping must be bit-exact against NumPy/torch-CPU, so floating-point contraction is OFF in this
// file: `areas[i] + areas[j] - w*h` must round the product before the subtraction like NumPy does.
#pragma clang fp contract(off)
#include "common.hpp"
#include "nms_large.hpp"
#include "warp_px.hpp"

#include <cmath>
#include <cstring>
#include <vector>

// ---------------------------------------------------------------------------------------------- SGD (DenseBox.py:2001-2004)
// torch.optim.SGD, dampening 0, no Nesterov: g = grad + wd*p; buf = g (first step) | mu*buf + g; p -= lr*buf
// guard (round 6): dbx_grad_guard leaves step_id in guard[0] when any gradient element of the step is not finite (f16 training keeps its
// activation gradients in 16-bit frames and the reference loss is an un-normalised sum: an overflow there reaches every weight gradient
// behind it as inf / NaN); an update launched with that guard and the same step_id then returns without touching anything and counts
// the skipped step in guard[1].  guard == NULL: the plain update.
__global__ void sgd_kernel(float* const* __restrict__ ptrs, const long long* __restrict__ sizes, float lr, float mu, float wd,
                           int first, int* __restrict__ guard, int step_id) {
    if (guard && guard[0] == step_id) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(guard + 1, 1);
        return;
    }
    const int t = blockIdx.y;
    float* p = ptrs[3 * t];
    const float* g = ptrs[3 * t + 1];
    float* b = ptrs[3 * t + 2];
    const long long n = sizes[t];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        p[i] = dbx_sgd_update(p[i], g[i], b + i, lr, mu, wd, first);
    }
}
extern "C" int dbx_sgd_step_guarded(float* const* ptrs, const int64_t* sizes, int32_t count, int64_t max_size, float lr, float momentum,
                                    float weight_decay, int32_t first_step, int32_t* guard, int32_t step_id, void* stream) {
    DBX_REQUIRE(ptrs && sizes && count > 0, "sgd: empty parameter list");
    int bx = (int)((max_size + 255) / 256);
    bx = bx < 1 ? 1 : (bx > 512 ? 512 : bx);
    hipLaunchKernelGGL(sgd_kernel, dim3(bx, count), dim3(256), 0, (hipStream_t)stream, ptrs, (const long long*)sizes, lr, momentum,
                       weight_decay, first_step, guard, step_id);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
extern "C" int dbx_sgd_step(float* const* ptrs, const int64_t* sizes, int32_t count, int64_t max_size, float lr, float momentum,
                            float weight_decay, int32_t first_step, void* stream) {
    return dbx_sgd_step_guarded(ptrs, sizes, count, max_size, lr, momentum, weight_decay, first_step, nullptr, 0, stream);
}
// one pass over the step's flat gradient buffer (46.7 MB for DenseBoxLMLOC: ~12 us): |x| with the exponent field all ones = inf or NaN
__global__ __launch_bounds__(256) void grad_guard_kernel(const float* __restrict__ g, long long n, int* __restrict__ guard, int step_id) {
    const long long n4 = n >> 2;
    const u32x4* g4 = (const u32x4*)g;
    unsigned bad = 0u;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const u32x4 v = g4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) bad |= ((v[e] & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n & 3))
        bad |= ((__float_as_uint(g[(n4 << 2) + threadIdx.x]) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
    if (__any((int)bad) && (threadIdx.x & 63) == 0) atomicMax(guard, step_id);
}
extern "C" int dbx_grad_guard(const float* grads, int64_t n, int32_t* guard, int32_t step_id, void* stream) {
    DBX_REQUIRE(grads && guard && n >= 0 && step_id > 0 && ((size_t)grads % 16) == 0, "grad_guard: 16-byte aligned gradients, a guard word pair, step ids from 1");
    if (n == 0) return DBX_OK;
    long long blocks = (n / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(grad_guard_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, grads, (long long)n, guard, step_id);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------- top-K + decode
// (DET_THREADS, the workgroup width of the decode and the small NMS, is nms_large.hpp's)

__device__ __forceinline__ void block_argmax_g(const float* vals, int n, float* red_v, int* red_i, float& ov, int& oi) {
    const int tid = threadIdx.x;
    float bv = -INFINITY; int bi = 0x7fffffff;
    for (int i = tid; i < n; i += DET_THREADS) {
        const float v = vals[i];
        if (v > bv || bi == 0x7fffffff) { bv = v; bi = i; }        // lower index wins ties; first element seeds
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float v2 = __shfl_down(bv, off); const int i2 = __shfl_down(bi, off);
        if (i2 != 0x7fffffff && (bi == 0x7fffffff || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
    }
    if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DET_THREADS / 64; ++w) {
            const float v2 = red_v[w]; const int i2 = red_i[w];
            if (i2 != 0x7fffffff && (bi == 0x7fffffff || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
        }
        red_v[0] = bv; red_i[0] = bi;
    }
    __syncthreads();
    ov = red_v[0]; oi = red_i[0];
    __syncthreads();
}

// Block-wide maximum of one 64-bit composite per thread (0 = no candidate), for the top-K rounds: a wave reduction by shuffles, the 16
// wave maxima through red_c, every thread reads all of them.  One barrier inside; the caller puts one between two calls (red_c).
__device__ __forceinline__ unsigned long long block_max_comp(unsigned long long c, unsigned long long* red_c) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(c, off); c = o > c ? o : c; }
    if ((tid & 63) == 0) red_c[tid >> 6] = c;
    __syncthreads();
    c = red_c[0];
#pragma unroll
    for (int w = 1; w < DET_THREADS / 64; ++w) { const unsigned long long o = red_c[w]; c = o > c ? o : c; }
    return c;
}

// greedy NMS over dets[n][dc] (float64): keep list in `keep` (keep[0] = count).  order = score descending, ties by
// higher row index first (= numpy argsort(stable)[::-1]; DenseBox.py:3415).
#define NMS_LDS_MAX 1024
__device__ void nms_block(const double* dets, int n, int dc, double thresh, int* keep, int* order, unsigned char* supp,
                          unsigned long long* mask = nullptr) {
    const int tid = threadIdx.x, nt = blockDim.x;
    // NaN scores rank where NumPy's sort puts them: argsort leaves NaN last, so [::-1] has them FIRST, the higher row index first among
    // them.  (NaN compares false both ways: ranked by `>` and `==` alone, every NaN row and the best row shared rank 0 -- not a
    // permutation, and which of them landed in the slot was a race between their threads.)  Every slot still starts as a valid row.
    for (int i = tid; i < n; i += nt) order[i] = i;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const double si = dets[(size_t)i * dc + 4];
        const bool nan_i = si != si;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double sj = dets[(size_t)j * dc + 4];
            const bool nan_j = sj != sj;
            rank += nan_i ? (nan_j && j > i) : (nan_j || (sj > si) || (sj == si && j > i));
        }
        order[rank] = i;
        supp[i] = 0;
    }
    __syncthreads();
    if (n <= NMS_LDS_MAX) {
        // boxes in rank order, areas and suppression flags staged in LDS: a greedy round is one LDS pass + one barrier
        __shared__ double bx1[NMS_LDS_MAX], by1[NMS_LDS_MAX], bx2[NMS_LDS_MAX], by2[NMS_LDS_MAX], bar[NMS_LDS_MAX];
        __shared__ unsigned char sp[NMS_LDS_MAX];
        for (int q = tid; q < n; q += nt) {
            const double* d = dets + (size_t)order[q] * dc;
            bx1[q] = d[0]; by1[q] = d[1]; bx2[q] = d[2]; by2[q] = d[3];
            bar[q] = (d[2] - d[0] + 1) * (d[3] - d[1] + 1);
            sp[q] = 0;
        }
        __syncthreads();
        if (mask != nullptr && n > 64) {
            // Many boxes (K = 1000): the greedy loop above costs one barrier per surviving box (~0.6 ms).  Instead (1) every thread
            // fills one row of the suppression matrix -- bit q of row p (q > p, rank order): box p would suppress box q, with the
            // very same fp64 expression -- into `mask` (n x 16 words, global scratch), all pairs in parallel; (2) ONE wave walks the
            // rows in rank order with the removed-set in registers (lane w holds word w), rows fetched 32 at a time.
            const int nw = (n + 63) >> 6;
            for (int p_ = tid; p_ < n; p_ += nt) {
                const double x1 = bx1[p_], y1 = by1[p_], x2 = bx2[p_], y2 = by2[p_], ai = bar[p_];
                for (int w = 0; w < nw; ++w) {
                    unsigned long long bits = 0ull;
                    if (64 * w + 63 > p_) {
                        for (int b = 0; b < 64; ++b) {
                            const int q = 64 * w + b;
                            if (q <= p_ || q >= n) continue;
                            const double xx1 = fmax(x1, bx1[q]), yy1 = fmax(y1, by1[q]), xx2 = fmin(x2, bx2[q]), yy2 = fmin(y2, by2[q]);
                            const double ww = fmax(0.0, xx2 - xx1 + 1), hh = fmax(0.0, yy2 - yy1 + 1);
                            const double inter = ww * hh;
                            const double ovr = inter / (ai + bar[q] - inter);
                            if (!(ovr <= thresh)) bits |= 1ull << b;             // NaN is dropped, like np.where(ovr <= t)
                        }
                    }
                    mask[(size_t)p_ * 16 + w] = bits;
                }
            }
            __threadfence_block();
            __syncthreads();
            if (tid < 64) {
                const int lane = tid;
                unsigned long long removed = 0ull;                  // lanes >= nw carry nothing
                int cnt = 0;
                for (int p0 = 0; p0 < n; p0 += 32) {
                    unsigned long long rows[32];
#pragma unroll
                    for (int r = 0; r < 32; ++r) rows[r] = (lane < nw && p0 + r < n) ? mask[(size_t)(p0 + r) * 16 + lane] : 0ull;
#pragma unroll
                    for (int r = 0; r < 32; ++r) {
                        const int pos = p0 + r;
                        if (pos >= n) break;
                        const unsigned long long word = __shfl(removed, pos >> 6);
                        if (!((word >> (pos & 63)) & 1ull)) {          // (uniform) box `pos` survives
                            if (lane == 0) keep[1 + cnt] = order[pos];
                            ++cnt;
                            removed |= rows[r];
                        }
                    }
                }
                if (lane == 0) keep[0] = cnt;
            }
            return;
        }
        int cnt = 0;
        for (int pos = 0; pos < n; ++pos) {
            if (sp[pos]) continue;                              // uniform: sp[] only changes between barriers
            if (tid == 0) keep[1 + cnt] = order[pos];
            ++cnt;
            const double x1 = bx1[pos], y1 = by1[pos], x2 = bx2[pos], y2 = by2[pos], ai = bar[pos];
            for (int q = pos + 1 + tid; q < n; q += nt) {
                if (sp[q]) continue;
                const double xx1 = fmax(x1, bx1[q]), yy1 = fmax(y1, by1[q]), xx2 = fmin(x2, bx2[q]), yy2 = fmin(y2, by2[q]);
                const double w = fmax(0.0, xx2 - xx1 + 1), h = fmax(0.0, yy2 - yy1 + 1);
                const double inter = w * h;
                const double ovr = inter / (ai + bar[q] - inter);
                if (!(ovr <= thresh)) sp[q] = 1;                 // NaN is dropped, like np.where(ovr <= t)
            }
            __syncthreads();
        }
        if (tid == 0) keep[0] = cnt;
        return;
    }
    int cnt = 0;
    for (int pos = 0; pos < n; ++pos) {
        const int i = order[pos];
        if (supp[i]) continue;                                  // uniform: supp[] only changes between barriers
        if (tid == 0) keep[1 + cnt] = i;
        ++cnt;
        const double x1 = dets[(size_t)i * dc], y1 = dets[(size_t)i * dc + 1], x2 = dets[(size_t)i * dc + 2], y2 = dets[(size_t)i * dc + 3];
        const double ai = (x2 - x1 + 1) * (y2 - y1 + 1);
        for (int q = pos + 1 + tid; q < n; q += nt) {
            const int j = order[q];
            if (supp[j]) continue;
            const double u1 = dets[(size_t)j * dc], v1 = dets[(size_t)j * dc + 1], u2 = dets[(size_t)j * dc + 2], v2 = dets[(size_t)j * dc + 3];
            const double aj = (u2 - u1 + 1) * (v2 - v1 + 1);
            const double xx1 = fmax(x1, u1), yy1 = fmax(y1, v1), xx2 = fmin(x2, u2), yy2 = fmin(y2, v2);
            const double w = fmax(0.0, xx2 - xx1 + 1), h = fmax(0.0, yy2 - yy1 + 1);
            const double inter = w * h;
            const double ovr = inter / (ai + aj - inter);
            if (!(ovr <= thresh)) supp[j] = 1;                   // NaN is dropped, like np.where(ovr <= t)
        }
        __syncthreads();
    }
    if (tid == 0) keep[0] = cnt;
}

// image 0's maps, outputs and scratch slice; workgroup b reads [b][C][rows][cols] maps, writes dets[b], topk[b], keep[b] and works
// in the scratch slice `scratch_stride` bytes further on per image (a multiple of 256: the slices keep image 0's alignment)
struct DetArgs {
    const float* score; const float* loc; const float* lm_heat; const float* lm_loc;
    int rows, cols, K, dc; double thresh;
    double* dets; long long* topk; int* keep; unsigned* work; int* order; unsigned char* supp; unsigned long long* mask;
    long long scratch_stride;
};

// order-preserving key of a score for the radix select: larger float <-> larger key, -0 == +0, NaN below every number
__device__ __forceinline__ unsigned det_key(float v) {
    if (v != v) return 0u;
    if (v == 0.f) return 0x80000000u;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One decoded row d[dc] of pixel idx of an n = rows x cols map: the row writer of every decode kernel (top-K and threshold), so they
// cannot drift apart.  lm_loc: parse_DetLMLOC's eight offsets; else (dc == 13) lm_arg[4], parse_DetLM's shared heat-map arg-max.
__device__ __forceinline__ void det_write_row(double* d, int idx, const float* score, const float* loc, const float* lm_loc,
                                              const int* lm_arg, int n, int cols, int dc) {
    const float xi = (float)(idx % cols), yi = (float)(idx / cols);
    // fp32 subtraction (python int - fp32 tensor), then float()*4.0 in double (DenseBox.py:3334-3343)
    d[0] = (double)(xi - loc[idx]) * 4.0;
    d[1] = (double)(yi - loc[(size_t)n + idx]) * 4.0;
    d[2] = (double)(xi - loc[(size_t)2 * n + idx]) * 4.0;
    d[3] = (double)(yi - loc[(size_t)3 * n + idx]) * 4.0;
    d[4] = (double)score[idx];
    if (dc == 13) {
        if (lm_loc) {
            for (int c = 0; c < 8; ++c)
                d[5 + c] = (double)(((c & 1) ? yi : xi) - lm_loc[(size_t)c * n + idx]) * 4.0;   // :3183-3196
        } else {
            for (int j = 0; j < 4; ++j) {
                d[5 + 2 * j] = (double)(float)(lm_arg[j] % cols) * 4.0;
                d[6 + 2 * j] = (double)(float)(lm_arg[j] / cols) * 4.0;
            }
        }
    }
}

// Radix select of the K largest scores of score[0..n) (four 8-bit passes over det_key, LDS histogram `hist` [256]), then compaction of the
// keys above the K-th plus the lowest-index ties: exactly K (key << 32 | ~index) composites in cand[0..K), in no particular order.
// Every thread of a DET_THREADS-wide workgroup calls it; it returns behind a barrier.
__device__ __forceinline__ void det_radix_select(const float* score, int n, int K, unsigned* hist, unsigned long long* cand) {
    const int tid = threadIdx.x;
    __shared__ unsigned sel_prefix, sel_remaining, sel_ties, cand_n, tie_base[DET_THREADS / 64 + 1];
    if (tid == 0) { sel_prefix = 0; sel_remaining = (unsigned)K; }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = sel_prefix;
        for (int i = tid; i < n; i += DET_THREADS) {
            const unsigned k = det_key(score[i]);
            if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned rem = sel_remaining, b = 255;
            for (;; --b) { const unsigned c = hist[b]; if (c >= rem || b == 0) break; rem -= c; }
            sel_prefix = prefix | (b << shift); sel_remaining = rem; sel_ties = hist[b];
        }
        __syncthreads();
    }
    const unsigned T = sel_prefix, need = sel_remaining, ties = sel_ties;     // K-th key; how many of its `ties` copies are taken
    if (tid == 0) cand_n = 0;
    __syncthreads();
    for (int i = tid; i < n; i += DET_THREADS) {
        const unsigned k = det_key(score[i]);
        if (k > T || (k == T && ties == need)) {
            const unsigned slot = atomicAdd(&cand_n, 1u);
            cand[slot] = ((unsigned long long)k << 32) | (unsigned)(~(unsigned)i);
        }
    }
    __syncthreads();
    if (ties != need) {
        // more copies of the K-th score than places: the lowest indices win.  Thread t owns the contiguous index range
        // [t * seg, (t + 1) * seg): per-thread tie counts -> exclusive block scan -> the first `need` ties in index order.
        const int seg = (n + DET_THREADS - 1) / DET_THREADS, lo = tid * seg, hi = min(n, lo + seg);
        unsigned mine = 0;
        for (int i = lo; i < hi; ++i) mine += det_key(score[i]) == T;
        unsigned incl = mine;                                   // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(incl, off); if ((tid & 63) >= off) incl += o; }
        if ((tid & 63) == 63) tie_base[(tid >> 6) + 1] = incl;
        __syncthreads();
        if (tid == 0) { tie_base[0] = 0; for (int w = 1; w <= DET_THREADS / 64; ++w) tie_base[w] += tie_base[w - 1]; }
        __syncthreads();
        unsigned before = tie_base[tid >> 6] + incl - mine;
        const unsigned base_slot = cand_n;
        for (int i = lo; i < hi && before < need; ++i)
            if (det_key(score[i]) == T) { cand[base_slot + before] = ((unsigned long long)T << 32) | (unsigned)(~(unsigned)i); ++before; }
        __syncthreads();
    }
}

// detect_kernel's top-K: ONE order on every path -- the descending order of the (det_key << 32 | ~index) composites: larger score
// first, lower index on ties, -0 == +0, -inf above NaN, NaN below every number with the lower index first, no index twice -- and five
// paths chosen from (K, n = rows * cols):
//   1  register tournament                                  K <= 48 and n <= 16384
//   2  radix select + bitonic sort                          DET_SELECT_MIN_K <= K <= 1024, any n
//   3  rounds, working copy in LDS, bucket maxima in LDS    K > 1024 and n <= 16384
//   4  rounds, working copy in global scratch, buckets      (K <= 48 or K > 1024) and 16384 < n <= 262144 (4096 buckets of 64)
//   5  rounds, flat per-thread rescan of the global copy    (K <= 48 or K > 1024) and n > 262144
// tests/test_hip_topk_paths.py holds every path to NumPy's order on both sides of every switch.
// Radix select + sort from DET_SELECT_MIN_K on; below it the rounds over the two-level LDS structure are faster (same-box
// A/B at K = 10 on a 128 x 128 map: whole 512 x 512 detect() 0.486 ms with rounds, 0.506 ms with select + a 16-element sort).
#ifndef DET_SELECT_MIN_K
#define DET_SELECT_MIN_K 49
#endif
// one workgroup per image (blockIdx.x): the same top-K paths, tie order, NaN handling and NMS on every image of the batch
__global__ __launch_bounds__(DET_THREADS) void detect_kernel(const DetArgs a0) {
    DetArgs a = a0;
    {
        const size_t b = blockIdx.x, n = (size_t)a0.rows * a0.cols;
        a.score += b * n;
        a.loc += b * 4 * n;
        if (a.lm_heat) a.lm_heat += b * 4 * n;
        if (a.lm_loc) a.lm_loc += b * 8 * n;
        a.dets += b * a0.K * a0.dc;
        a.topk += b * a0.K;
        a.keep += b * (a0.K + 1);
        const size_t so = b * (size_t)a0.scratch_stride;
        a.work = (unsigned*)((char*)a0.work + so);
        a.order = (int*)((char*)a0.order + so);
        a.supp = a0.supp + so;
        if (a.mask) a.mask = (unsigned long long*)((char*)a0.mask + so);
    }
    __shared__ float red_v[DET_THREADS / 64];
    __shared__ int red_i[DET_THREADS / 64];
    __shared__ int lm_arg[4];
    const int tid = threadIdx.x, n = a.rows * a.cols;
    constexpr int BK = 64, NB_MAX = 4096;
    __shared__ unsigned long long bcomp[NB_MAX];                 // bucket maxima of the rounds; the candidates of the other two paths
    __shared__ unsigned det_hist[256];
    // landmark arg-max per heat-map channel (parse_DetLM, DenseBox.py:3284-3292): identical for every detection
    if (a.lm_heat && !a.lm_loc) {
        for (int j = 0; j < 4; ++j) {
            float v; int idx;
            block_argmax_g(a.lm_heat + (size_t)j * n, n, red_v, red_i, v, idx);
            if (tid == 0) lm_arg[j] = idx;
        }
        __syncthreads();
    }
    // ---- top-K indices into a.topk, in the reference's order: larger score first, lower index on ties
    const bool select = a.K >= DET_SELECT_MIN_K && a.K <= DET_THREADS;
    const bool tourney = !select && a.K <= 48 && n <= 16 * DET_THREADS;
    if (tourney) {
        // Small K on a map of <= 16384 scores (the 512 x 512 input's 128 x 128 map, K = 10): every lane keeps its 16 scores in registers
        // as (key << 32 | ~index) composites -- larger composite = larger score, lower index on ties, the select path's order -- each
        // wave extracts ITS top K by K rounds of a register maximum + a wave reduction (shuffles only, no workgroup barrier), the 16
        // waves leave their sorted lists in LDS and wave 0 merges the 16 K candidates the same way: ~6 us instead of K block-wide
        // rounds with their barriers (measured when a round had three: 30 us at K = 10).
        unsigned long long* wcand = bcomp;                                 // [16][48]
        const int lane = tid & 63, wv = tid >> 6;
        unsigned long long comp[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = tid + e * DET_THREADS;
            comp[e] = i < n ? ((unsigned long long)det_key(a.score[i]) << 32) | (unsigned)(~(unsigned)i) : 0ull;
        }
        auto wave_max = [&](unsigned long long v) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; }
            return v;
        };
        for (int r = 0; r < a.K; ++r) {
            unsigned long long best = comp[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) best = comp[e] > best ? comp[e] : best;
            best = wave_max(best);
#pragma unroll
            for (int e = 0; e < 16; ++e) comp[e] = comp[e] == best ? 0ull : comp[e];
            if (lane == 0) wcand[wv * 48 + r] = best;
        }
        __syncthreads();
        if (wv == 0) {
            const int tot = (DET_THREADS / 64) * a.K;                        // <= 768: 12 per lane
            unsigned long long c2[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const int f = lane + 64 * j;
                c2[j] = f < tot ? wcand[(f / a.K) * 48 + f % a.K] : 0ull;
            }
            for (int r = 0; r < a.K; ++r) {
                unsigned long long best = c2[0];
#pragma unroll
                for (int j = 1; j < 12; ++j) best = c2[j] > best ? c2[j] : best;
                best = wave_max(best);
#pragma unroll
                for (int j = 0; j < 12; ++j) c2[j] = c2[j] == best ? 0ull : c2[j];
                if (lane == 0) a.topk[r] = (long long)(~(unsigned)(best & 0xffffffffull));
            }
        }
        __syncthreads();
    } else if (select) {
        // K in (48, 1024] (round 3: K = 1000 at 1080p took 4.7 ms as 1000 arg-max rounds): radix select of the K-th largest key
        // (four 8-bit passes, LDS histogram), compaction of the keys above it plus the lowest-index ties, bitonic sort of <= 1024
        // (key, index) pairs in LDS -- ~0.1 ms, the same ranking bit for bit.
        unsigned long long* cand = bcomp;                        // [1024] (key << 32) | ~index: descending sort = reference order
        det_radix_select(a.score, n, a.K, det_hist, cand);
        int P2 = 2;                                               // sort size: the power of two >= K (K = 10: 16 elements, 10 exchange steps)
        while (P2 < a.K) P2 <<= 1;
        for (int i = a.K + tid; i < P2; i += DET_THREADS) cand[i] = 0ull;                // padding sorts last
        __syncthreads();
        // bitonic sort, descending, P2 <= 1024 elements: one element per thread
        for (int size = 2; size <= P2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const int partner = tid ^ stride;
                unsigned long long me = 0, ot = 0;
                if (tid < P2) { me = cand[tid]; ot = cand[partner]; }
                __syncthreads();
                const bool desc = (tid & size) == 0;                // this block sorts descending
                const bool keep_max = (tid < partner) == desc;
                if (tid < P2) cand[tid] = keep_max ? (me > ot ? me : ot) : (me < ot ? me : ot);
                __syncthreads();
            }
        }
        if (tid < a.K) a.topk[tid] = (long long)(~(unsigned)(cand[tid] & 0xffffffffull));
        __syncthreads();
    } else {
        // The retire-and-rescan rounds rank by the SAME (key << 32 | ~index) composites as the two paths above, so the order is theirs on
        // every input: larger score first, lower index on ties, -0 == +0, NaN below every number and the lower index first among NaN.
        // The working copy holds det_key + 1 per score (NaN = 1, +inf = 0xff800001: no overflow) and 0 for a retired one, which no
        // score can equal: a genuine -inf is emitted once and a retired element never again (composite 0 = nothing, below everything).
        // The copy lives in LDS when the map fits (<= 128 x 128, the 512 x 512 input: a round's store -> 64 reloads of the winner's
        // bucket is an LDS round trip instead of an L2 one), else in global scratch.
        constexpr int WORK_LDS = 16384;
        __shared__ unsigned work_lds[WORK_LDS];
        __shared__ unsigned long long red_c[DET_THREADS / 64];
        unsigned* const work = n <= WORK_LDS ? work_lds : a.work;
        for (int i = tid; i < n; i += DET_THREADS) work[i] = det_key(a.score[i]) + 1u;
        __syncthreads();
        // K rounds of maximum over a two-level structure: LDS holds the largest composite of every bucket of 64 consecutive scores;
        // a round reduces the bucket maxima (LDS only) and one wave re-scans the winner's bucket (64 loads in flight at once),
        // instead of every thread re-reading its share of the whole map from global memory: ~4 us per round instead of 24.
        // K <= n (checked at the ABI) and a round retires exactly one live score, so a round's maximum is never 0.
        const int nb = (n + BK - 1) / BK;
        const int lane = tid & 63, wv = tid >> 6;
        const bool two_level = nb <= NB_MAX;
        auto comp_of = [&](int i) {
            const unsigned w = work[i];
            return w ? ((unsigned long long)w << 32) | (unsigned)(~(unsigned)i) : 0ull;
        };
        auto scan_bucket = [&](int b) {                              // one wave: the largest composite of bucket b -> LDS
            const int i = b * BK + lane;
            unsigned long long c = i < n ? comp_of(i) : 0ull;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(c, off); c = o > c ? o : c; }
            if (lane == 0) bcomp[b] = c;
        };
        if (two_level) {
            for (int b = wv; b < nb; b += DET_THREADS / 64) scan_bucket(b);
            __syncthreads();
        }
        unsigned long long mine = 0ull;
        auto rescan = [&]() {                                        // fallback for huge maps: per-thread cached candidate
            mine = 0ull;
            for (int i = tid; i < n; i += DET_THREADS) { const unsigned long long c = comp_of(i); mine = c > mine ? c : mine; }
        };
        if (!two_level) rescan();
        for (int k = 0; k < a.K; ++k) {
            unsigned long long c = mine;
            if (two_level) {
                for (int b = tid; b < nb; b += DET_THREADS) { const unsigned long long o = bcomp[b]; c = o > c ? o : c; }
            }
            const int idx = (int)(~(unsigned)(block_max_comp(c, red_c) & 0xffffffffull));
            if (two_level) {
                if (wv == 0) {                                       // wave 0 retires the winner and refreshes its bucket
                    if (lane == 0) work[idx] = 0u;
                    __builtin_amdgcn_wave_barrier();
                    __threadfence_block();
                    scan_bucket(idx / BK);
                }
            } else if ((idx & (DET_THREADS - 1)) == tid) { work[idx] = 0u; rescan(); }
            if (tid == 0) a.topk[k] = idx;
            __syncthreads();                                         // bcomp / red_c: this round's reads before the next one's writes
        }
    }
    __threadfence_block();
    __syncthreads();
    // ---- decode: one thread per detection (the rows no longer sit as dependent global loads inside the selection rounds)
    for (int k = tid; k < a.K; k += DET_THREADS) {
        det_write_row(a.dets + (size_t)k * a.dc, (int)a.topk[k], a.score, a.loc, a.lm_loc, lm_arg, n, a.cols, a.dc);
    }
    __threadfence_block();
    __syncthreads();
    nms_block(a.dets, a.K, a.dc, a.thresh, a.keep, a.order, a.supp, a.mask);
}

extern "C" int64_t dbx_detect_scratch_bytes(int32_t rows, int32_t cols, int32_t K) {
    // scores copy, NMS order, suppression flags, + the 16-word-per-box suppression matrix when the boxes fit the LDS path
    return (int64_t)rows * cols * 4 + (int64_t)K * 4 + ((int64_t)K + 255) / 256 * 256 + (K <= NMS_LDS_MAX ? (int64_t)K * 128 : 0) + 256;
}

// one image's slice of the batched scratch: the single-image layout rounded up to 256 B
static int64_t detect_slice_bytes(int32_t rows, int32_t cols, int32_t K) {
    return (dbx_detect_scratch_bytes(rows, cols, K) + 255) / 256 * 256;
}

extern "C" int64_t dbx_detect_batch_scratch_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t K) {
    return (int64_t)batch * detect_slice_bytes(rows, cols, K);
}

static int detect_launch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc, int32_t batch, int32_t rows,
                         int32_t cols, int32_t K, double nms_thresh, double* dets, int32_t det_cols, int64_t* topk_idx, int32_t* keep,
                         void* scratch, void* stream) {
    DetArgs a;
    a.score = score; a.loc = loc; a.lm_heat = lm_heat; a.lm_loc = lm_loc;
    a.rows = rows; a.cols = cols; a.K = K; a.dc = det_cols; a.thresh = nms_thresh;
    a.dets = dets; a.topk = (long long*)topk_idx; a.keep = keep;
    char* s = (char*)scratch;
    a.work = (unsigned*)s; s += (size_t)rows * cols * 4;
    a.order = (int*)s; s += (size_t)K * 4;
    a.supp = (unsigned char*)s; s += ((size_t)K + 255) / 256 * 256;
    s = (char*)(((size_t)s + 7) & ~(size_t)7);                          // (inside the 256 spare bytes)
    a.mask = K <= NMS_LDS_MAX ? (unsigned long long*)s : nullptr;
    a.scratch_stride = detect_slice_bytes(rows, cols, K);
    hipLaunchKernelGGL(detect_kernel, dim3(batch), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_detect(const float* score, const float* loc, const float* lm_heat, const float* lm_loc, int32_t rows,
                          int32_t cols, int32_t K, double nms_thresh, double* dets, int32_t det_cols, int64_t* topk_idx,
                          int32_t* keep, void* scratch, void* stream) {
    DBX_REQUIRE(score && loc && dets && topk_idx && keep && scratch, "detect: null argument");
    DBX_REQUIRE(K > 0 && K <= rows * cols, "detect: K=%d out of range", K);
    DBX_REQUIRE(det_cols == 5 || (det_cols == 13 && (lm_heat || lm_loc)), "detect: det_cols must be 5, or 13 with landmark maps");
    return detect_launch(score, loc, lm_heat, lm_loc, 1, rows, cols, K, nms_thresh, dets, det_cols, topk_idx, keep, scratch, stream);
}

extern "C" int dbx_detect_batch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc, int32_t batch,
                                int32_t rows, int32_t cols, int32_t K, double nms_thresh, double* dets, int32_t det_cols,
                                int64_t* topk_idx, int32_t* keep, void* scratch, void* stream) {
    DBX_REQUIRE(score && loc && dets && topk_idx && keep && scratch, "detect_batch: null argument");
    DBX_REQUIRE(batch > 0, "detect_batch: batch=%d must be positive", batch);
    DBX_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols <= 0x7fffffff, "detect_batch: bad map size %d x %d", rows, cols);
    DBX_REQUIRE(K > 0 && K <= rows * cols, "detect_batch: K=%d out of range", K);
    DBX_REQUIRE(det_cols == 5 || (det_cols == 13 && (lm_heat || lm_loc)), "detect_batch: det_cols must be 5, or 13 with landmark maps");
    return detect_launch(score, loc, lm_heat, lm_loc, batch, rows, cols, K, nms_thresh, dets, det_cols, topk_idx, keep, scratch, stream);
}

__global__ __launch_bounds__(DET_THREADS) void nms_kernel(const double* dets, int n, int dc, double thresh, int* keep, int* order,
                                                          unsigned char* supp) {
    nms_block(dets, n, dc, thresh, keep, order, supp);
}
extern "C" int dbx_nms(const double* dets, int32_t n, int32_t det_cols, double nms_thresh, int32_t* keep, void* scratch,
                       void* stream) {
    DBX_REQUIRE(dets && keep && scratch && n > 0 && det_cols >= 5, "nms: bad arguments");
    int* order = (int*)scratch;
    unsigned char* supp = (unsigned char*)scratch + (size_t)n * 4;
    hipLaunchKernelGGL(nms_kernel, dim3(1), dim3(DET_THREADS), 0, (hipStream_t)stream, dets, n, det_cols, nms_thresh, keep, order, supp);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---- pyramid merge: the rows of every level of every frame of a chunk mapped back to the source frame + ONE greedy NMS per frame over
// their union, in one launch (dbx_merge_nms_batch).  Workgroup b owns frame b.  Stage 1 copies row r of level l to row l * K + r of
// out_dets[b] with x * scale - off_x / y * scale - off_y in float64 (contraction is off in this file: the product is rounded before
// the subtraction, NumPy's `d * scale - off` bit for bit; the score column is copied).  Stage 2, after a barrier, is nms_block on those
// n = levels * K rows -- the code dbx_nms runs, at the same workgroup width, so order, ties, the +1 pixel IoU and the NaN handling
// cannot drift apart.  The map stage uses no LDS; nms_block's static arrays are the kernel's whole LDS budget.
// workspace: [levels device pointers][levels * batch transforms] rounded to 256 B, then one slice per frame:
// order (4 n, to 256 B) | suppression flags (n, to 256 B) | the 16-word suppression rows (128 n, only when n <= NMS_LDS_MAX)
#define MERGE_MAX_ROWS 4096
static int64_t merge_head_bytes(int32_t levels, int32_t batch) {
    return ((int64_t)levels * 8 + (int64_t)levels * batch * (int64_t)sizeof(dbx_merge_xform) + 255) / 256 * 256;
}
static int64_t merge_slice_bytes(int64_t n) {
    return (n * 4 + 255) / 256 * 256 + (n + 255) / 256 * 256 + (n <= NMS_LDS_MAX ? (n * 128 + 255) / 256 * 256 : 0);
}
static_assert(sizeof(dbx_merge_xform) == 24, "dbx_merge_xform layout");

// one column of a level row in source-frame coordinates: x columns 0, 2, 5, 7, 9, 11, y columns 1, 3, 6, 8, 10, 12, the score copied
__device__ __forceinline__ double merge_map_col(double v, int col, const dbx_merge_xform& t) {
    if (col == 4) return v;
    const bool is_x = col < 4 ? !(col & 1) : (col & 1);
    return v * t.scale - (is_x ? t.off_x : t.off_y);
}

__global__ __launch_bounds__(DET_THREADS) void merge_nms_kernel(const double* const* __restrict__ level_dets,
                                                                const dbx_merge_xform* __restrict__ xform, int levels, int batch, int K,
                                                                int dc, double thresh, double* __restrict__ out_dets, int* out_keep,
                                                                unsigned char* slices, long long slice_bytes) {
    const size_t b = blockIdx.x;
    const int n = levels * K;                                   // <= MERGE_MAX_ROWS
    const long long ne = (long long)n * dc;
    double* const o = out_dets + b * (size_t)ne;
    for (long long e = threadIdx.x; e < ne; e += blockDim.x) {
        const int row = (int)(e / dc), col = (int)(e - (long long)row * dc);
        const int l = row / K, r = row - l * K;
        o[e] = merge_map_col(level_dets[l][(b * (size_t)K + (size_t)r) * (size_t)dc + (size_t)col], col, xform[(size_t)l * batch + b]);
    }
    __threadfence_block();
    __syncthreads();
    unsigned char* s = slices + b * (size_t)slice_bytes;
    int* order = (int*)s;
    unsigned char* supp = s + ((size_t)n * 4 + 255) / 256 * 256;
    unsigned long long* mask = n <= NMS_LDS_MAX ? (unsigned long long*)(supp + ((size_t)n + 255) / 256 * 256) : nullptr;
    nms_block(o, n, dc, thresh, out_keep + b * ((size_t)n + 1), order, supp, mask);
}

extern "C" int64_t dbx_merge_nms_batch_workspace_bytes(int32_t levels, int32_t batch, int32_t K) {
    if (levels < 1 || batch < 1 || K < 1 || (int64_t)levels * K > MERGE_MAX_ROWS) return -1;
    return merge_head_bytes(levels, batch) + (int64_t)batch * merge_slice_bytes((int64_t)levels * K);
}

extern "C" int dbx_merge_nms_batch(const double* const* level_dets, const dbx_merge_xform* xform, int32_t levels, int32_t batch, int32_t K,
                                   int32_t det_cols, double nms_thresh, double* out_dets, int32_t* out_keep, void* workspace,
                                   void* stream) {
    DBX_REQUIRE(levels >= 1, "merge_nms_batch: levels=%d must be positive", levels);
    DBX_REQUIRE(batch >= 1, "merge_nms_batch: batch=%d must be positive", batch);
    DBX_REQUIRE(K >= 1, "merge_nms_batch: K=%d must be positive", K);
    DBX_REQUIRE(det_cols == 5 || det_cols == 13, "merge_nms_batch: det_cols=%d must be 5 or 13", det_cols);
    DBX_REQUIRE((int64_t)levels * K <= MERGE_MAX_ROWS, "merge_nms_batch: levels * K = %lld rows per frame exceed %d (the rank pass is quadratic)",
                (long long)levels * K, MERGE_MAX_ROWS);
    DBX_REQUIRE(level_dets && xform && out_dets && out_keep && workspace, "merge_nms_batch: null argument");
    for (int l = 0; l < levels; ++l) DBX_REQUIRE(level_dets[l], "merge_nms_batch: level %d has a null row pointer", l);
    for (int64_t i = 0; i < (int64_t)levels * batch; ++i) {
        const dbx_merge_xform& t = xform[i];
        DBX_REQUIRE(std::isfinite(t.scale) && t.scale > 0.0, "merge_nms_batch: level %d frame %d has scale %g (finite and positive needed)",
                    (int)(i / batch), (int)(i % batch), t.scale);
        DBX_REQUIRE(std::isfinite(t.off_x) && std::isfinite(t.off_y), "merge_nms_batch: level %d frame %d has a non-finite offset",
                    (int)(i / batch), (int)(i % batch));
    }
    // device records: the level pointers, then the transforms.  Pageable host source: the copy has read the vector when it returns,
    // so it may go out of scope (and the caller's arrays be reused)
    const int64_t head = merge_head_bytes(levels, batch);
    std::vector<unsigned char> rec((size_t)head, 0);
    memcpy(rec.data(), level_dets, (size_t)levels * 8);
    memcpy(rec.data() + (size_t)levels * 8, xform, (size_t)levels * batch * sizeof(dbx_merge_xform));
    unsigned char* ws = (unsigned char*)workspace;
    DBX_HIP(hipMemcpyAsync(ws, rec.data(), (size_t)head, hipMemcpyHostToDevice, (hipStream_t)stream));
    hipLaunchKernelGGL(merge_nms_kernel, dim3(batch), dim3(DET_THREADS), 0, (hipStream_t)stream, (const double* const*)ws,
                       (const dbx_merge_xform*)(ws + (size_t)levels * 8), levels, batch, K, det_cols, nms_thresh, out_dets, out_keep,
                       ws + head, (long long)merge_slice_bytes((int64_t)levels * K));
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------- threshold decode + NMS for <= 4096 rows
// dbx_detect_thresh_batch: per image every pixel with score > t (strict: NaN never, +inf always, -0.0 > 0.0 is false) is a candidate row,
// at most `cap` of them (the best in the top-K order when more pass), and the reference's greedy NMS runs over all of them.  Three
// launches whose grids depend on (batch, cap) alone -- the counts stay on the device, so the sequence can be captured:
//   1. thresh_select_kernel, one workgroup per image: ONE pass over the map counts and compacts the (det_key << 32 | ~index) composites
//      into LDS (the radix select runs only when more than cap pass), a bitonic sort puts them into the reference's row order, the rows
//      go to the image's scratch slice through det_write_row, and the NMS order comes from the sort (runs of equal scores reversed:
//      nms_block ranks the HIGHER row index first on ties) -- no quadratic rank pass.  counts[b] = (n_b, pixels above t).
//   2. thresh_pack_mask_kernel, grid (cap / 64, batch): workgroup (rb, b) copies rows [64 rb, 64 rb + 64) of image b behind the rows of
//      the images before it (exclusive prefix of the counts) and fills those rows of the suppression matrix, every word at or right of
//      the diagonal, with nms_block's fp64 expression; workgroups past n_b leave at once.  Many CUs per image.
//   3. thresh_sweep_kernel, one wave per image: the greedy walk with the removed set in registers (lane w holds word w of 64).
// dbx_nms_large runs 2 (without the copy) and 3 on caller rows behind a sort of (score key, row index) pairs.
// nmsl_mask_rows, nmsl_sweep, nmsl_score_key and nmsl_sort_pairs live in nms_large.hpp: the tile stitch (tile_ops.hip) runs the same
// functions.
// one image's scratch slice: rows [cap][13] float64 | map indices [cap] int64 | NMS order [cap] int32 | matrix [cap][ceil(cap / 64)] words
struct ThrLayout { long long topk, order, mask, total; int nw; };
static __host__ __device__ inline ThrLayout thr_layout(int cap) {
    ThrLayout L;
    L.nw = (cap + 63) / 64;
    L.topk = thr_up256((long long)cap * 13 * 8);
    L.order = L.topk + thr_up256((long long)cap * 8);
    L.mask = L.order + thr_up256((long long)cap * 4);
    L.total = L.mask + thr_up256((long long)cap * L.nw * 8);
    return L;
}

struct ThrArgs {
    const float* score; const float* loc; const float* lm_heat; const float* lm_loc;
    int batch, rows, cols, dc, cap, keep_behind_rows;
    float t; double thresh;
    double* dets; long long* topk; int* keep; int* counts;        // counts: [batch][2] pairs, then the [batch + 1] exclusive prefix
    unsigned char* scratch;
};

// descending bitonic sort of a[0..P2) in LDS by the whole workgroup (a barrier in front is the caller's)
__device__ __forceinline__ void bitonic_desc_u64(unsigned long long* a, int P2) {
    for (int size = 2; size <= P2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P2 >> 1); t += blockDim.x) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const unsigned long long x = a[i], y = a[j];
                if (((i & size) == 0) ? x < y : x > y) { a[i] = y; a[j] = x; }
            }
            __syncthreads();
        }
}

// The select stage of image b = blockIdx.x, shared by dbx_detect_thresh_batch and dbx_thresh_rows_batch: threshold + compaction, the
// radix select past the cap, the sort, the rows (rows_fs [cap][dc]) and map indices (topk_fs [cap]) of the image and its count pair.
// ORDER: also the NMS order of the rows (order [cap]); without it `order` is not touched.
template <bool ORDER>
__device__ __forceinline__ void thresh_select_image(const ThrArgs& a, double* rows_fs, long long* topk_fs, int* order) {
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x, n = a.rows * a.cols, cap = a.cap;
    const float* score = a.score + b * (size_t)n;
    const float* loc = a.loc + b * 4 * (size_t)n;
    const float* lm_heat = a.lm_heat ? a.lm_heat + b * 4 * (size_t)n : nullptr;
    const float* lm_loc = a.lm_loc ? a.lm_loc + b * 8 * (size_t)n : nullptr;
    __shared__ float red_v[DET_THREADS / 64];
    __shared__ int red_i[DET_THREADS / 64];
    __shared__ int lm_arg[4];
    __shared__ unsigned long long cand[THR_MAX_DETS];
    __shared__ unsigned hist[256];
    __shared__ unsigned above;
    if (tid < 4) lm_arg[tid] = 0;
    if (tid == 0) above = 0;
    __syncthreads();
    if (lm_heat && !lm_loc) {
        for (int j = 0; j < 4; ++j) {
            float v; int idx;
            block_argmax_g(lm_heat + (size_t)j * n, n, red_v, red_i, v, idx);
            if (tid == 0) lm_arg[j] = idx;
        }
        __syncthreads();
    }
    // ---- threshold + compaction in one pass; slots past the cap are counted, not stored
    for (int i = tid; i < n; i += DET_THREADS) {
        const float v = score[i];
        if (v > a.t) {
            const unsigned slot = atomicAdd(&above, 1u);
            if (slot < (unsigned)cap) cand[slot] = ((unsigned long long)det_key(v) << 32) | (unsigned)(~(unsigned)i);
        }
    }
    __syncthreads();
    const unsigned total = above;
    const int nb = total < (unsigned)cap ? (int)total : cap;
    if (total > (unsigned)cap) det_radix_select(score, n, cap, hist, cand);          // the cap best of the map = the cap best candidates
    int P2 = 2;
    while (P2 < nb) P2 <<= 1;
    for (int i = nb + tid; i < P2; i += DET_THREADS) cand[i] = 0ull;                    // padding sorts last
    __syncthreads();
    bitonic_desc_u64(cand, P2);
    // ---- rows in the reference's order; NMS position of row r of a run [s, e) of equal scores: s + (e - 1 - r)
    for (int r = tid; r < nb; r += DET_THREADS) {
        const unsigned long long c = cand[r];
        const unsigned key = (unsigned)(c >> 32);
        const int idx = (int)(~(unsigned)(c & 0xffffffffull));
        det_write_row(rows_fs + (size_t)r * a.dc, idx, score, loc, lm_loc, lm_arg, n, a.cols, a.dc);
        topk_fs[r] = idx;
        if (ORDER) {
            int lo = 0, hi = r;                                     // first position whose key is <= key
            while (lo < hi) { const int m = (lo + hi) >> 1; if ((unsigned)(cand[m] >> 32) > key) lo = m + 1; else hi = m; }
            const int rs = lo;
            lo = r + 1; hi = nb;                                    // first position whose key is < key
            while (lo < hi) { const int m = (lo + hi) >> 1; if ((unsigned)(cand[m] >> 32) >= key) lo = m + 1; else hi = m; }
            order[rs + (lo - 1 - r)] = r;
        }
    }
    if (tid == 0) { a.counts[2 * b] = nb; a.counts[2 * b + 1] = (int)total; }
}

__global__ __launch_bounds__(DET_THREADS) void thresh_select_kernel(const ThrArgs a) {
    const ThrLayout L = thr_layout(a.cap);
    unsigned char* const s = a.scratch + blockIdx.x * (size_t)L.total;
    thresh_select_image<true>(a, (double*)s, (long long*)(s + L.topk), (int*)(s + L.order));
}

// dbx_thresh_rows_batch: the select stage alone, straight into the caller's [batch][cap] slots (a.dets, a.topk)
__global__ __launch_bounds__(DET_THREADS) void thresh_rows_kernel(const ThrArgs a) {
    const size_t r0 = blockIdx.x * (size_t)a.cap;
    thresh_select_image<false>(a, a.dets + r0 * a.dc, a.topk + r0, nullptr);
}

__global__ __launch_bounds__(NMSL_THREADS) void thresh_pack_mask_kernel(const ThrArgs a) {
    const int rb = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = a.counts[2 * b];
    if (rb > 0 && 64 * rb >= n) return;
    __shared__ int s_pre, s_tot;
    if (tid == 0) { s_pre = 0; s_tot = 0; }
    __syncthreads();
    int pre = 0, tot = 0;
    for (int j = tid; j < a.batch; j += NMSL_THREADS) { const int c = a.counts[2 * j]; tot += c; pre += j < b ? c : 0; }
    atomicAdd(&s_pre, pre); atomicAdd(&s_tot, tot);
    __syncthreads();
    pre = s_pre; tot = s_tot;
    int* const prefix = a.counts + 2 * (size_t)a.batch;
    if (rb == 0 && tid == 0) { prefix[b] = pre; if (b == a.batch - 1) prefix[a.batch] = tot; }
    if (64 * rb >= n) return;
    const ThrLayout L = thr_layout(a.cap);
    unsigned char* const s = a.scratch + (size_t)b * L.total;
    const double* rows_fs = (const double*)s;
    const long long* topk_fs = (const long long*)(s + L.topk);
    const int r0 = 64 * rb, nr = min(64, n - r0);
    double* const od = a.dets + ((size_t)pre + r0) * a.dc;
    for (int e = tid; e < nr * a.dc; e += NMSL_THREADS) od[e] = rows_fs[(size_t)r0 * a.dc + e];
    for (int r = tid; r < nr; r += NMSL_THREADS) a.topk[(size_t)pre + r0 + r] = topk_fs[r0 + r];
    nmsl_mask_rows(rows_fs, a.dc, (const int*)(s + L.order), n, a.thresh, (unsigned long long*)(s + L.mask), L.nw, rb);
}

__global__ __launch_bounds__(64) void thresh_sweep_kernel(const ThrArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int pre = 0, tot = 0;
    for (int j = lane; j < a.batch; j += 64) { const int c = a.counts[2 * j]; tot += c; pre += j < b ? c : 0; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { pre += __shfl_xor(pre, off); tot += __shfl_xor(tot, off); }
    // image b's keep list: n_b + 1 words behind those of the images before it; the lists start right behind the packed rows when asked
    int* const keep = (a.keep_behind_rows ? (int*)(a.dets + (size_t)tot * a.dc) : a.keep) + (size_t)pre + b;
    const ThrLayout L = thr_layout(a.cap);
    const unsigned char* s = a.scratch + (size_t)b * L.total;
    nmsl_sweep((const unsigned long long*)(s + L.mask), L.nw, (const int*)(s + L.order), a.counts[2 * b], keep);
}

extern "C" int64_t dbx_detect_thresh_batch_scratch_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t max_dets) {
    if (batch < 1 || rows < 1 || cols < 1 || max_dets < 1 || max_dets > THR_MAX_DETS) return -1;
    return (int64_t)batch * thr_layout(max_dets).total;
}

extern "C" int dbx_detect_thresh_batch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc, int32_t batch,
                                       int32_t rows, int32_t cols, float score_thresh, int32_t max_dets, double nms_thresh, double* dets,
                                       int32_t det_cols, int64_t* topk_idx, int32_t* keep, int32_t* counts, void* scratch, void* stream) {
    DBX_REQUIRE(score && loc && dets && topk_idx && keep && counts && scratch, "detect_thresh_batch: null argument");
    DBX_REQUIRE(batch > 0, "detect_thresh_batch: batch=%d must be positive", batch);
    DBX_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols <= 0x7fffffff, "detect_thresh_batch: bad map size %d x %d", rows, cols);
    DBX_REQUIRE(max_dets >= 1 && max_dets <= THR_MAX_DETS, "detect_thresh_batch: max_dets=%d must be 1..%d", max_dets, THR_MAX_DETS);
    DBX_REQUIRE(!std::isnan(score_thresh), "detect_thresh_batch: score_thresh is NaN");
    DBX_REQUIRE(!std::isnan(nms_thresh) && nms_thresh >= 0.0, "detect_thresh_batch: nms_thresh=%g must be a number >= 0", nms_thresh);
    DBX_REQUIRE(det_cols == 5 || (det_cols == 13 && (lm_heat || lm_loc)), "detect_thresh_batch: det_cols must be 5, or 13 with landmark maps");
    DBX_REQUIRE((int64_t)batch * max_dets <= 0x7fffffff / 16, "detect_thresh_batch: batch * max_dets = %lld rows do not fit the packed arena's int32 prefix",
                (long long)batch * max_dets);
    ThrArgs a;
    a.score = score; a.loc = loc; a.lm_heat = lm_heat; a.lm_loc = lm_loc;
    a.batch = batch; a.rows = rows; a.cols = cols; a.dc = det_cols; a.cap = max_dets;
    a.keep_behind_rows = (const void*)keep == (const void*)dets;
    a.t = score_thresh; a.thresh = nms_thresh;
    a.dets = dets; a.topk = (long long*)topk_idx; a.keep = keep; a.counts = counts; a.scratch = (unsigned char*)scratch;
    hipLaunchKernelGGL(thresh_select_kernel, dim3(batch), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(thresh_pack_mask_kernel, dim3((max_dets + 63) / 64, batch), dim3(NMSL_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(thresh_sweep_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---- dbx_thresh_rows_batch: launch 1 alone, for a caller that merges the rows of several runs before the NMS (the threshold pyramid).
// The kernel works in LDS and writes straight into the caller's slots; the scratch argument is kept in the contract (a non-null
// pointer of dbx_thresh_rows_batch_scratch_bytes) so that a later version may stage through global memory without an ABI change.
extern "C" int64_t dbx_thresh_rows_batch_scratch_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t max_dets) {
    if (batch < 1 || rows < 1 || cols < 1 || max_dets < 1 || max_dets > THR_MAX_DETS) return -1;
    return 256;
}

extern "C" int dbx_thresh_rows_batch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc, int32_t batch,
                                     int32_t rows, int32_t cols, float score_thresh, int32_t max_dets, double* dets, int32_t det_cols,
                                     int64_t* topk_idx, int32_t* counts, void* scratch, void* stream) {
    DBX_REQUIRE(score && loc && dets && topk_idx && counts && scratch, "thresh_rows_batch: null argument");
    DBX_REQUIRE(batch > 0, "thresh_rows_batch: batch=%d must be positive", batch);
    DBX_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols <= 0x7fffffff, "thresh_rows_batch: bad map size %d x %d", rows, cols);
    DBX_REQUIRE(max_dets >= 1 && max_dets <= THR_MAX_DETS, "thresh_rows_batch: max_dets=%d must be 1..%d", max_dets, THR_MAX_DETS);
    DBX_REQUIRE(!std::isnan(score_thresh), "thresh_rows_batch: score_thresh is NaN");
    DBX_REQUIRE(det_cols == 5 || (det_cols == 13 && (lm_heat || lm_loc)), "thresh_rows_batch: det_cols must be 5, or 13 with landmark maps");
    DBX_REQUIRE((int64_t)batch * max_dets <= 0x7fffffff / 16, "thresh_rows_batch: batch * max_dets = %lld rows do not fit an int32 row number",
                (long long)batch * max_dets);
    ThrArgs a;
    a.score = score; a.loc = loc; a.lm_heat = lm_heat; a.lm_loc = lm_loc;
    a.batch = batch; a.rows = rows; a.cols = cols; a.dc = det_cols; a.cap = max_dets;
    a.keep_behind_rows = 0;
    a.t = score_thresh; a.thresh = 0.0;
    a.dets = dets; a.topk = (long long*)topk_idx; a.keep = nullptr; a.counts = counts; a.scratch = (unsigned char*)scratch;
    hipLaunchKernelGGL(thresh_rows_kernel, dim3(batch), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---- dbx_nms_large: the same matrix + sweep on caller rows.  The order comes from a bitonic sort of (score key, row) pairs in LDS
// (48 KB): key = the float64 score's bits made order-preserving, -0 == +0, every NaN the largest; larger key first, the higher row first
// among equal keys -- nms_block's rank for every input.
__global__ __launch_bounds__(DET_THREADS) void nms_large_order_kernel(const double* dets, int n, int dc, int* order) {
    __shared__ unsigned long long key[THR_MAX_DETS];
    __shared__ int row[THR_MAX_DETS];
    int P2 = 2;
    while (P2 < n) P2 <<= 1;
    for (int i = threadIdx.x; i < P2; i += DET_THREADS) {
        key[i] = i < n ? nmsl_score_key(dets[(size_t)i * dc + 4]) : 0ull;      // padding: below -inf's key
        row[i] = i < n ? i : -1;
    }
    __syncthreads();
    nmsl_sort_pairs(key, row, P2);
    for (int i = threadIdx.x; i < n; i += DET_THREADS) order[i] = row[i];
}
__global__ __launch_bounds__(NMSL_THREADS) void nms_large_mask_kernel(const double* dets, int n, int dc, double thresh, const int* order,
                                                                      unsigned long long* mask) {
    nmsl_mask_rows(dets, dc, order, n, thresh, mask, (n + 63) >> 6, blockIdx.x);
}
__global__ __launch_bounds__(64) void nms_large_sweep_kernel(const unsigned long long* mask, const int* order, int n, int* keep) {
    nmsl_sweep(mask, (n + 63) >> 6, order, n, keep);
}

extern "C" int64_t dbx_nms_large_scratch_bytes(int32_t n) {
    if (n < 1 || n > THR_MAX_DETS) return -1;
    return thr_up256((long long)n * 4) + thr_up256((long long)n * ((n + 63) / 64) * 8);
}

extern "C" int dbx_nms_large(const double* dets, int32_t n, int32_t det_cols, double nms_thresh, int32_t* keep, void* scratch,
                             void* stream) {
    DBX_REQUIRE(dets && keep && scratch, "nms_large: null argument");
    DBX_REQUIRE(n >= 1 && n <= THR_MAX_DETS, "nms_large: n=%d must be 1..%d", n, THR_MAX_DETS);
    DBX_REQUIRE(det_cols >= 5, "nms_large: det_cols=%d must be at least 5", det_cols);
    DBX_REQUIRE(!std::isnan(nms_thresh) && nms_thresh >= 0.0, "nms_large: nms_thresh=%g must be a number >= 0", nms_thresh);
    int* order = (int*)scratch;
    unsigned long long* mask = (unsigned long long*)((unsigned char*)scratch + thr_up256((long long)n * 4));
    hipLaunchKernelGGL(nms_large_order_kernel, dim3(1), dim3(DET_THREADS), 0, (hipStream_t)stream, dets, n, det_cols, order);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_large_mask_kernel, dim3((n + 63) / 64), dim3(NMSL_THREADS), 0, (hipStream_t)stream, dets, n, det_cols, nms_thresh,
                       (const int*)order, mask);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_large_sweep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)mask, (const int*)order, n,
                       keep);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---- dbx_merge_nms_thresh_batch: dbx_merge_nms_batch over the variable row counts dbx_thresh_rows_batch leaves on the device.  Three
// launches whose grids depend on (levels, batch, max_dets) alone; the counts are read on the device and clamped to 0..max_dets there.
//   1. merge_thresh_pack_kernel, one workgroup per frame: its level counts and the unions of the frames before it give P[b]; the rows
//      go, mapped by merge_map_col, to rows P[b].. of out_dets level by level; the thread that copies a score also files the
//      (nmsl_score_key, union row) pair in LDS, and nmsl_sort_pairs gives the NMS order (dbx_nms_large's, 48 KB).
//   2. merge_thresh_mask_kernel, grid (ceil(levels * max_dets / 64), batch): nmsl_mask_rows on the frame's packed rows; workgroups
//      past m_b leave at once.
//   3. merge_thresh_sweep_kernel, one wave per frame: nmsl_sweep into the frame's packed keep list.
// workspace: [levels row pointers][levels count pointers][levels * batch transforms] to 256 B, then per frame
// order [levels * max_dets] int32 (to 256 B) | matrix [levels * max_dets][ceil(levels * max_dets / 64)] words
struct MergeThrArgs {
    const double* const* level_dets; const int* const* level_counts; const dbx_merge_xform* xform;
    int levels, batch, cap, dc, keep_behind_rows;
    double thresh;
    double* out_dets; int* out_keep; int* out_counts;
    unsigned char* slices;
};
struct MergeThrLayout { long long mask, total; int nw; };
static __host__ __device__ inline MergeThrLayout merge_thr_layout(int nmax) {
    MergeThrLayout L;
    L.nw = (nmax + 63) / 64;
    L.mask = thr_up256((long long)nmax * 4);
    L.total = L.mask + thr_up256((long long)nmax * L.nw * 8);
    return L;
}
static int64_t merge_thr_head_bytes(int32_t levels, int32_t batch) {
    return thr_up256((int64_t)levels * 16 + (int64_t)levels * batch * (int64_t)sizeof(dbx_merge_xform));
}
__device__ __forceinline__ int merge_thr_count(const MergeThrArgs& a, int l, int b) {      // n_(l,b), never trusted as it stands
    return min(max(a.level_counts[l][2 * b], 0), a.cap);
}

__global__ __launch_bounds__(DET_THREADS) void merge_thresh_pack_kernel(const MergeThrArgs a) {
    __shared__ unsigned long long key[THR_MAX_DETS];
    __shared__ int row[THR_MAX_DETS];
    __shared__ int s_pre, s_mine, s_tot;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s_pre = 0; s_mine = 0; s_tot = 0; }
    __syncthreads();
    int pre = 0, mine = 0, tot = 0;
    for (int i = tid; i < a.levels * a.batch; i += DET_THREADS) {
        const int l = i / a.batch, j = i - l * a.batch, c = merge_thr_count(a, l, j);
        tot += c; pre += j < b ? c : 0; mine += j == b ? c : 0;
    }
    atomicAdd(&s_pre, pre); atomicAdd(&s_mine, mine); atomicAdd(&s_tot, tot);
    __syncthreads();
    pre = s_pre; tot = s_tot;
    const int m = s_mine;                                            // <= levels * cap <= MERGE_MAX_ROWS
    int* const pairs = a.out_counts + (size_t)b * a.levels * 2;
    for (int l = tid; l < a.levels; l += DET_THREADS) { pairs[2 * l] = merge_thr_count(a, l, b); pairs[2 * l + 1] = a.level_counts[l][2 * b + 1]; }
    int* const prefix = a.out_counts + (size_t)a.batch * a.levels * 2;
    if (tid == 0) { prefix[b] = pre; if (b == a.batch - 1) prefix[a.batch] = tot; }
    if (m == 0) return;
    double* const o = a.out_dets + (size_t)pre * a.dc;
    int u0 = 0;                                                      // union row of the level's row 0
    for (int l = 0; l < a.levels; ++l) {
        const int nl = merge_thr_count(a, l, b);                     // (uniform)
        const double* src = a.level_dets[l] + (size_t)b * a.cap * a.dc;
        const dbx_merge_xform t = a.xform[(size_t)l * a.batch + b];
        for (int e = tid; e < nl * a.dc; e += DET_THREADS) {
            const int r = e / a.dc, col = e - r * a.dc;
            const double v = src[e];
            o[(size_t)u0 * a.dc + e] = merge_map_col(v, col, t);
            if (col == 4) { key[u0 + r] = nmsl_score_key(v); row[u0 + r] = u0 + r; }
        }
        u0 += nl;
    }
    int P2 = 2;
    while (P2 < m) P2 <<= 1;
    for (int i = m + tid; i < P2; i += DET_THREADS) { key[i] = 0ull; row[i] = -1; }      // padding: below -inf's key
    __syncthreads();
    nmsl_sort_pairs(key, row, P2);
    int* const order = (int*)(a.slices + (size_t)b * merge_thr_layout(a.levels * a.cap).total);
    for (int i = tid; i < m; i += DET_THREADS) order[i] = row[i];
}

__global__ __launch_bounds__(NMSL_THREADS) void merge_thresh_mask_kernel(const MergeThrArgs a) {
    const int rb = blockIdx.x, b = blockIdx.y;
    const int* const prefix = a.out_counts + (size_t)a.batch * a.levels * 2;
    const int pre = prefix[b], m = min(prefix[b + 1] - pre, a.levels * a.cap);
    if (64 * rb >= m) return;
    const MergeThrLayout L = merge_thr_layout(a.levels * a.cap);
    unsigned char* const s = a.slices + (size_t)b * L.total;
    nmsl_mask_rows(a.out_dets + (size_t)pre * a.dc, a.dc, (const int*)s, m, a.thresh, (unsigned long long*)(s + L.mask), L.nw, rb);
}

__global__ __launch_bounds__(64) void merge_thresh_sweep_kernel(const MergeThrArgs a) {
    const int b = blockIdx.x;
    const int* const prefix = a.out_counts + (size_t)a.batch * a.levels * 2;
    const int pre = prefix[b], m = min(prefix[b + 1] - pre, a.levels * a.cap), tot = prefix[a.batch];
    int* const keep = (a.keep_behind_rows ? (int*)(a.out_dets + (size_t)tot * a.dc) : a.out_keep) + (size_t)pre + b;
    const MergeThrLayout L = merge_thr_layout(a.levels * a.cap);
    const unsigned char* s = a.slices + (size_t)b * L.total;
    nmsl_sweep((const unsigned long long*)(s + L.mask), L.nw, (const int*)s, m, keep);
}

extern "C" int64_t dbx_merge_nms_thresh_batch_workspace_bytes(int32_t levels, int32_t batch, int32_t max_dets) {
    if (levels < 1 || batch < 1 || max_dets < 1 || max_dets > THR_MAX_DETS || (int64_t)levels * max_dets > MERGE_MAX_ROWS) return -1;
    return merge_thr_head_bytes(levels, batch) + (int64_t)batch * merge_thr_layout(levels * max_dets).total;
}

extern "C" int dbx_merge_nms_thresh_batch(const double* const* level_dets, const int32_t* const* level_counts, const dbx_merge_xform* xform,
                                          int32_t levels, int32_t batch, int32_t max_dets, int32_t det_cols, double nms_thresh,
                                          double* out_dets, int32_t* out_keep, int32_t* out_counts, void* workspace, void* stream) {
    DBX_REQUIRE(levels >= 1, "merge_nms_thresh_batch: levels=%d must be positive", levels);
    DBX_REQUIRE(batch >= 1, "merge_nms_thresh_batch: batch=%d must be positive", batch);
    DBX_REQUIRE(max_dets >= 1 && max_dets <= THR_MAX_DETS, "merge_nms_thresh_batch: max_dets=%d must be 1..%d", max_dets, THR_MAX_DETS);
    DBX_REQUIRE(det_cols == 5 || det_cols == 13, "merge_nms_thresh_batch: det_cols=%d must be 5 or 13", det_cols);
    DBX_REQUIRE((int64_t)levels * max_dets <= MERGE_MAX_ROWS, "merge_nms_thresh_batch: levels * max_dets = %lld rows per frame exceed %d",
                (long long)levels * max_dets, MERGE_MAX_ROWS);
    DBX_REQUIRE(!std::isnan(nms_thresh) && nms_thresh >= 0.0, "merge_nms_thresh_batch: nms_thresh=%g must be a number >= 0", nms_thresh);
    DBX_REQUIRE(level_dets && level_counts && xform && out_dets && out_keep && out_counts && workspace, "merge_nms_thresh_batch: null argument");
    DBX_REQUIRE((int64_t)batch * levels * max_dets <= 0x7fffffff / 16, "merge_nms_thresh_batch: batch * levels * max_dets = %lld rows do not fit the packed arena's int32 prefix",
                (long long)batch * levels * max_dets);
    for (int l = 0; l < levels; ++l)
        DBX_REQUIRE(level_dets[l] && level_counts[l], "merge_nms_thresh_batch: level %d has a null row or count pointer", l);
    for (int64_t i = 0; i < (int64_t)levels * batch; ++i) {
        const dbx_merge_xform& t = xform[i];
        DBX_REQUIRE(std::isfinite(t.scale) && t.scale > 0.0, "merge_nms_thresh_batch: level %d frame %d has scale %g (finite and positive needed)",
                    (int)(i / batch), (int)(i % batch), t.scale);
        DBX_REQUIRE(std::isfinite(t.off_x) && std::isfinite(t.off_y), "merge_nms_thresh_batch: level %d frame %d has a non-finite offset",
                    (int)(i / batch), (int)(i % batch));
    }
    // device records, as in dbx_merge_nms_batch (pageable source: the copy has read the vector when it returns)
    const int64_t head = merge_thr_head_bytes(levels, batch);
    std::vector<unsigned char> rec((size_t)head, 0);
    memcpy(rec.data(), level_dets, (size_t)levels * 8);
    memcpy(rec.data() + (size_t)levels * 8, level_counts, (size_t)levels * 8);
    memcpy(rec.data() + (size_t)levels * 16, xform, (size_t)levels * batch * sizeof(dbx_merge_xform));
    unsigned char* ws = (unsigned char*)workspace;
    DBX_HIP(hipMemcpyAsync(ws, rec.data(), (size_t)head, hipMemcpyHostToDevice, (hipStream_t)stream));
    MergeThrArgs a;
    a.level_dets = (const double* const*)ws; a.level_counts = (const int* const*)(ws + (size_t)levels * 8);
    a.xform = (const dbx_merge_xform*)(ws + (size_t)levels * 16);
    a.levels = levels; a.batch = batch; a.cap = max_dets; a.dc = det_cols;
    a.keep_behind_rows = (const void*)out_keep == (const void*)out_dets;
    a.thresh = nms_thresh;
    a.out_dets = out_dets; a.out_keep = out_keep; a.out_counts = out_counts; a.slices = ws + head;
    hipLaunchKernelGGL(merge_thresh_pack_kernel, dim3(batch), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_thresh_mask_kernel, dim3((levels * max_dets + 63) / 64, batch), dim3(NMSL_THREADS), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_thresh_sweep_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---------------------------------------------------------------------------------------------- plate rectification
// perspective_transform (DenseBox.py:3446-3481): homography from the four landmark corners to their axis-aligned bounding
// rectangle (cv2.getPerspectiveTransform) and a warp of the whole image to 1.5x its size (cv2.warpPerspective, default
// INTER_LINEAR, constant border 0).  OpenCV is not part of the reference tree (and not installed here), so both follow its
// PUBLISHED algorithm (imgwarp.cpp): 8x8 system in double solved by LU with partial pivoting; inverse map through the
// 3x3 inverse; source coordinates rounded to 1/32 pixel (INTER_BITS = 5); 8-bit bilinear weights in 15-bit fixed point,
// (sum + 2^14) >> 15.  Parity with OpenCV itself is unpinned; the GPU kernel is bit-exact against oracle/.
// perspective_solve, warp_px_u8 and warp_inverse live in warp_px.hpp: the patch warp (warp_aug_ops.hip) runs the same functions.
extern "C" int dbx_perspective_matrix(const float* src_xy, const float* dst_xy, double* m9) {
    DBX_REQUIRE(src_xy && dst_xy && m9, "perspective_matrix: null argument");
    double s[8], d[8];
    for (int i = 0; i < 8; ++i) { s[i] = src_xy[i]; d[i] = dst_xy[i]; }
    DBX_REQUIRE(perspective_solve(s, d, m9), "perspective_matrix: degenerate corner configuration");
    return DBX_OK;
}

struct WarpArgs { const unsigned char* src; unsigned char* dst; int sh, sw, c, dh, dw; double im[9]; };
__global__ void warp_perspective_u8_kernel(const WarpArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.dw || y >= a.dh) return;
    const unsigned int px = warp_px_u8(a.im, a.src, a.sh, a.sw, a.c, x, y);
    for (int ch = 0; ch < a.c; ++ch) a.dst[((size_t)y * a.dw + x) * a.c + ch] = (unsigned char)(px >> (8 * ch));
}

extern "C" int dbx_warp_perspective_u8(const uint8_t* src, int32_t sh, int32_t sw, int32_t c, const double* m9, uint8_t* dst,
                                       int32_t dh, int32_t dw, void* stream) {
    DBX_REQUIRE(src && dst && m9 && sh > 0 && sw > 0 && dh > 0 && dw > 0 && c >= 1 && c <= 4, "warp_perspective: bad arguments");
    WarpArgs a;
    DBX_REQUIRE(warp_inverse(m9, a.im), "warp_perspective: singular matrix");
    a.src = src; a.dst = dst; a.sh = sh; a.sw = sw; a.c = c; a.dh = dh; a.dw = dw;
    hipLaunchKernelGGL(warp_perspective_u8_kernel, dim3((dw + 255) / 256, dh), dim3(256), 0, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---- batched warp: every plate of a batch in one launch (dbx_warp_perspective_batch_u8)
// A job's output window [oh][ow][c] is one contiguous byte range, so the kernel walks it as a flat list of oh*ow pixels (wrapping from
// one window row to the next).  Each wave owns a segment of WARP_SEG consecutive pixels.  Pass 1: in each of WARP_PPT steps the 64
// lanes make 64 CONSECUTIVE pixels -- the neighbour gathers of a wave instruction cover a narrow span of the source, as in the
// single-image kernel -- and put their c bytes into the wave's slice of LDS.  Pass 2: each lane stores 16-byte words of the segment
// (64 consecutive words per wave instruction) when the job's output is 16-byte aligned, dwords when it is 4-byte aligned, bytes
// otherwise and for the job's last partial word.  Source and destination go through global-address-space pointers (global_load /
// global_store, not flat).  A tile is one workgroup's WARP_THREADS / 64 segments; tile0[j] is the first tile of job j (a prefix of
// the per-job tile counts), and each workgroup finds its job by a binary search of tile0.
#define WARP_THREADS 256
#define WARP_PPT 8
#define WARP_SEG (64 * WARP_PPT)
typedef const __attribute__((address_space(1))) unsigned char* warp_gsrc_t;
typedef __attribute__((address_space(1))) unsigned char* warp_gdst_t;
typedef __attribute__((address_space(1))) u32x4* warp_gdst4_t;
typedef __attribute__((address_space(1))) unsigned int* warp_gdst1_t;
struct WarpJobDev {                     // device record of one job (128 bytes)
    const unsigned char* src;
    unsigned char* dst;                 // dst + dst_off
    double im[9];                       // canvas -> source map
    long long npix;                     // oh * ow
    int sh, sw, x0, y0, ow, pad[3];
};
static_assert(sizeof(WarpJobDev) == 128, "WarpJobDev layout");

template <int C>
__global__ __launch_bounds__(WARP_THREADS) void warp_perspective_batch_u8_kernel(const WarpJobDev* __restrict__ jobs,
                                                                                  const int* __restrict__ tile0, int njobs) {
    __shared__ __attribute__((aligned(16))) unsigned char seg[WARP_THREADS / 64][WARP_SEG * C];
    const int t = blockIdx.x;
    int lo = 0, hi = njobs - 1;                        // the last job whose first tile is <= t (jobs without tiles never match)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const WarpJobDev* J = jobs + lo;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long npix = J->npix;
    const long long s0 = ((long long)(t - tile0[lo]) * (WARP_THREADS / 64) + wave) * WARP_SEG;   // first pixel of the wave's segment
    const int nseg = s0 >= npix ? 0 : (npix - s0 < WARP_SEG ? (int)(npix - s0) : WARP_SEG);       // its pixels (wave-uniform)
    unsigned char* L = seg[wave];
    if (nseg > 0) {
        double im[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) im[i] = J->im[i];
        const warp_gsrc_t src = (warp_gsrc_t)J->src;
        const int sh = J->sh, sw = J->sw, ow = J->ow, x0 = J->x0, y0 = J->y0;
        const long long p = s0 + lane;
        int y = (int)(p / ow), x = (int)(p - (long long)y * ow);
#pragma unroll
        for (int i = 0; i < WARP_PPT; ++i) {
            const int q = i * 64 + lane;
            if (q < nseg) {
                const unsigned int px = warp_px_u8(im, src, sh, sw, C, x0 + x, y0 + y);
                if (C == 4) {
                    reinterpret_cast<unsigned int*>(L)[q] = px;
                } else {
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) L[q * C + ch] = (unsigned char)(px >> (8 * ch));
                }
            }
            x += 64;                                   // the lane's next pixel is 64 further on
            if (x >= ow) { y += x / ow; x %= ow; }
        }
    }
    __syncthreads();
    if (nseg == 0) return;
    const warp_gdst_t d = (warp_gdst_t)(J->dst + s0 * C);
    const int nb = nseg * C;
    const size_t al = (size_t)d;
    for (int k = lane; 16 * k < nb; k += 64) {
        const int b0 = 16 * k;
        if (b0 + 16 <= nb && al % 16 == 0) {
            reinterpret_cast<warp_gdst4_t>(d)[k] = reinterpret_cast<const u32x4*>(L)[k];
        } else if (b0 + 16 <= nb && al % 4 == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) reinterpret_cast<warp_gdst1_t>(d)[4 * k + j] = reinterpret_cast<const unsigned int*>(L)[4 * k + j];
        } else {
            for (int j = b0; j < nb && j < b0 + 16; ++j) d[j] = L[j];
        }
    }
}

static int64_t warp_tile0_offset(int32_t njobs) { return (int64_t)njobs * (int64_t)sizeof(WarpJobDev); }

extern "C" int64_t dbx_warp_batch_workspace_bytes(int32_t njobs) {
    if (njobs < 0) return -1;
    return (warp_tile0_offset(njobs) + 4 * ((int64_t)njobs + 1) + 255) / 256 * 256;
}

extern "C" int dbx_warp_perspective_batch_u8(const dbx_warp_job* jobs, int32_t njobs, int32_t c, uint8_t* dst, void* workspace,
                                             void* stream) {
    DBX_REQUIRE(njobs >= 0, "warp_perspective_batch: njobs=%d is negative", njobs);
    DBX_REQUIRE(c >= 1 && c <= 4, "warp_perspective_batch: c=%d must be 1..4", c);
    if (njobs == 0) return DBX_OK;
    DBX_REQUIRE(jobs && dst && workspace, "warp_perspective_batch: null argument");
    std::vector<WarpJobDev> rec(njobs);
    std::vector<int> tile0(njobs + 1);
    constexpr long long tile = (long long)WARP_THREADS * WARP_PPT;        // pixels per workgroup
    long long tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const dbx_warp_job& g = jobs[j];
        DBX_REQUIRE(g.src, "warp_perspective_batch: job %d has a null source", j);
        DBX_REQUIRE(g.sh > 0 && g.sw > 0 && g.dh > 0 && g.dw > 0 && g.oh > 0 && g.ow > 0,
                    "warp_perspective_batch: job %d has a non-positive size (source %d x %d, canvas %d x %d, window %d x %d)", j, g.sh,
                    g.sw, g.dh, g.dw, g.oh, g.ow);
        DBX_REQUIRE(g.x0 >= 0 && g.y0 >= 0 && (int64_t)g.x0 + g.ow <= g.dw && (int64_t)g.y0 + g.oh <= g.dh,
                    "warp_perspective_batch: job %d window (%d, %d) + %d x %d lies outside its %d x %d canvas", j, g.x0, g.y0, g.ow, g.oh,
                    g.dw, g.dh);
        DBX_REQUIRE(g.dst_off >= 0, "warp_perspective_batch: job %d has a negative dst_off", j);
        WarpJobDev& r = rec[j];
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(g.m9[i]);
        DBX_REQUIRE(finite, "warp_perspective_batch: job %d has a non-finite matrix", j);
        DBX_REQUIRE(warp_inverse(g.m9, r.im), "warp_perspective_batch: job %d has a singular matrix", j);
        r.src = g.src; r.dst = dst + g.dst_off; r.npix = (long long)g.oh * g.ow;
        r.sh = g.sh; r.sw = g.sw; r.x0 = g.x0; r.y0 = g.y0; r.ow = g.ow; r.pad[0] = r.pad[1] = r.pad[2] = 0;
        tile0[j] = (int)tiles;
        tiles += (r.npix + tile - 1) / tile;
        // one workgroup per tile, and a grid holds at most 2^32 - 1 work-items per dimension
        DBX_REQUIRE(tiles <= 0xffffffffLL / WARP_THREADS, "warp_perspective_batch: more than %lld tiles of %lld pixels", 0xffffffffLL / WARP_THREADS,
                    tile);
    }
    tile0[njobs] = (int)tiles;
    // pageable host source: the copy has read both vectors when it returns, so they may go out of scope (and `jobs` be reused)
    unsigned char* ws = (unsigned char*)workspace;
    DBX_HIP(hipMemcpyAsync(ws, rec.data(), sizeof(WarpJobDev) * njobs, hipMemcpyHostToDevice, (hipStream_t)stream));
    DBX_HIP(hipMemcpyAsync(ws + warp_tile0_offset(njobs), tile0.data(), sizeof(int) * (njobs + 1), hipMemcpyHostToDevice,
                           (hipStream_t)stream));
    const WarpJobDev* dj = (const WarpJobDev*)ws;
    const int* dt = (const int*)(ws + warp_tile0_offset(njobs));
    const dim3 grid((unsigned)tiles), block(WARP_THREADS);
    switch (c) {
        case 1: hipLaunchKernelGGL(warp_perspective_batch_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
        case 2: hipLaunchKernelGGL(warp_perspective_batch_u8_kernel<2>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
        case 3: hipLaunchKernelGGL(warp_perspective_batch_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
        default: hipLaunchKernelGGL(warp_perspective_batch_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, dj, dt, njobs); break;
    }
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// ---- fixed-size plate crops, rectified on the device (dbx_plate_crops_batch)
// frames x slots crops of oh x ow pixels: a fixed grid, so the (frame, slot, tile) triple comes from blockIdx by division -- no prefix
// table, no search.  Every workgroup of a slot solves the slot's homography itself: all lanes run perspective_solve on the same values
// (the float32-rounded quad read from device memory -> the rectangle (0,0)..(ow-1,oh-1)), so there is no broadcast and no second
// launch; the copies of the solve run side by side on different SIMDs and cost no wall time over solving it once.  Then the batched
// warp's two passes, unchanged: 64 consecutive pixels per wave step into LDS, 16-byte / dword / byte stores by the slot's alignment.
// Slots that are not ok (and slots past the frame's count) store zeros through the same path, so the call writes every byte of dst.
struct PlateCropArgs {
    const dbx_crop_frame* frames;
    const double* quads;
    const int* sel;
    unsigned char* dst;
    int* ok;
    double* m9_out;
    long long row_stride, frame_stride, npix;
    int slots, ow, oh;
    unsigned int tiles;                  // workgroups per slot
};

__host__ __device__ static inline bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and inf

template <int C>
__global__ __launch_bounds__(WARP_THREADS) void plate_crops_batch_u8_kernel(const PlateCropArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char seg[WARP_THREADS / 64][WARP_SEG * C];
    const unsigned int t = blockIdx.x % a.tiles, slot = blockIdx.x / a.tiles;
    const int j = (int)(slot % (unsigned int)a.slots), b = (int)(slot / (unsigned int)a.slots);
    const int* S = a.sel ? a.sel + (size_t)b * (a.slots + 1) : nullptr;
    const int count = S ? (S[0] < 0 ? 0 : (S[0] > a.slots ? a.slots : S[0])) : a.slots;
    const dbx_crop_frame F = a.frames[b];
    double m[9], im[9];
    bool ok = j < count && F.src != nullptr && F.sh > 0 && F.sw > 0;
    if (ok) {
        const int r = S ? S[1 + j] : j;
        ok = r >= 0 && (!S || (long long)r * a.row_stride + 8 <= a.frame_stride);     // a row of `sel` must lie inside its frame's stride
        if (ok) {
            const double* q = a.quads + (long long)b * a.frame_stride + (long long)r * a.row_stride;
            double s[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s[i] = (double)(float)q[i];            // np.float32(src_pts), widened again
                ok = ok && finite_f64(s[i]);
            }
            const double W = (double)(float)(a.ow - 1), H = (double)(float)(a.oh - 1);
            const double d[8] = {0.0, 0.0, W, 0.0, W, H, 0.0, H};
            ok = ok && perspective_solve(s, d, m);
            if (ok) {
#pragma unroll
                for (int i = 0; i < 8; ++i) ok = ok && finite_f64(m[i]);
            }
            ok = ok && warp_inverse(m, im);
        }
    }
    if (t == 0 && threadIdx.x == 0) {
        a.ok[slot] = ok ? 1 : 0;
        if (ok && a.m9_out) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a.m9_out[(size_t)slot * 9 + i] = m[i];
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long npix = a.npix;
    const long long s0 = ((long long)t * (WARP_THREADS / 64) + wave) * WARP_SEG;                 // first pixel of the wave's segment
    const int nseg = s0 >= npix ? 0 : (npix - s0 < WARP_SEG ? (int)(npix - s0) : WARP_SEG);       // its pixels (wave-uniform)
    unsigned char* L = seg[wave];
    if (nseg > 0) {
        const warp_gsrc_t src = (warp_gsrc_t)F.src;
        const int ow = a.ow;
        const long long p = s0 + lane;
        int y = (int)(p / ow), x = (int)(p - (long long)y * ow);
#pragma unroll
        for (int i = 0; i < WARP_PPT; ++i) {
            const int q = i * 64 + lane;
            if (q < nseg) {
                const unsigned int px = ok ? warp_px_u8(im, src, F.sh, F.sw, C, x, y) : 0u;
                if (C == 4) {
                    reinterpret_cast<unsigned int*>(L)[q] = px;
                } else {
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) L[q * C + ch] = (unsigned char)(px >> (8 * ch));
                }
            }
            x += 64;                                   // the lane's next pixel is 64 further on
            if (x >= ow) { y += x / ow; x %= ow; }
        }
    }
    __syncthreads();
    if (nseg == 0) return;
    const warp_gdst_t d = (warp_gdst_t)(a.dst + ((size_t)slot * (size_t)npix + (size_t)s0) * C);
    const int nb = nseg * C;
    const size_t al = (size_t)d;
    for (int k = lane; 16 * k < nb; k += 64) {
        const int b0 = 16 * k;
        if (b0 + 16 <= nb && al % 16 == 0) {
            reinterpret_cast<warp_gdst4_t>(d)[k] = reinterpret_cast<const u32x4*>(L)[k];
        } else if (b0 + 16 <= nb && al % 4 == 0) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) reinterpret_cast<warp_gdst1_t>(d)[4 * k + jj] = reinterpret_cast<const unsigned int*>(L)[4 * k + jj];
        } else {
            for (int jj = b0; jj < nb && jj < b0 + 16; ++jj) d[jj] = L[jj];
        }
    }
}

extern "C" int dbx_plate_crops_batch(const dbx_crop_frame* frames, int32_t nframes, int32_t c, const double* quads, int64_t row_stride,
                                     int64_t frame_stride, const int32_t* sel, int32_t slots, int32_t ow, int32_t oh, uint8_t* dst,
                                     int32_t* ok, double* m9_out, void* stream) {
    DBX_REQUIRE(nframes >= 0, "plate_crops_batch: nframes=%d is negative", nframes);
    DBX_REQUIRE(c >= 1 && c <= 4, "plate_crops_batch: c=%d must be 1..4", c);
    DBX_REQUIRE(slots >= 1, "plate_crops_batch: slots=%d must be positive", slots);
    DBX_REQUIRE(ow >= 1 && oh >= 1, "plate_crops_batch: crop size %d x %d must be positive", ow, oh);
    DBX_REQUIRE(row_stride >= 8, "plate_crops_batch: row_stride=%lld holds no quad of 8 values", (long long)row_stride);
    DBX_REQUIRE(sel || frame_stride >= (int64_t)slots * row_stride, "plate_crops_batch: frame_stride=%lld is below slots * row_stride = %lld",
                (long long)frame_stride, (long long)slots * (long long)row_stride);
    if (nframes == 0) return DBX_OK;
    DBX_REQUIRE(frames && quads && dst && ok, "plate_crops_batch: null argument");
    constexpr long long tile = (long long)WARP_THREADS * WARP_PPT;        // pixels per workgroup
    PlateCropArgs a;
    a.npix = (long long)oh * ow;
    const long long tiles = (a.npix + tile - 1) / tile, nslots = (long long)nframes * slots;
    // one workgroup per tile, and a grid holds at most 2^32 - 1 work-items per dimension
    DBX_REQUIRE(tiles <= 0xffffffffLL / WARP_THREADS / nslots, "plate_crops_batch: %lld slots of %lld tiles exceed the %lld tiles of one grid", nslots,
                tiles, 0xffffffffLL / WARP_THREADS);
    a.frames = frames; a.quads = quads; a.sel = sel; a.dst = dst; a.ok = ok; a.m9_out = m9_out;
    a.row_stride = row_stride; a.frame_stride = frame_stride; a.slots = slots; a.ow = ow; a.oh = oh; a.tiles = (unsigned int)tiles;
    const dim3 grid((unsigned)(tiles * nslots)), block(WARP_THREADS);
    switch (c) {
        case 1: hipLaunchKernelGGL(plate_crops_batch_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(plate_crops_batch_u8_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(plate_crops_batch_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(plate_crops_batch_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
    }
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
