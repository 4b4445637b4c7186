// The pixel-centric tile walk of the kernels that paint on frames -- viz_ops.hip (dbx_draw_overlay_batch, 128 x 16 tiles) and
// redact_ops.hip (dbx_redact_batch, 64 x 16 tiles) -- once: one workgroup of 256 threads per TW x TH tile of a dbx_overlay_frame
// record collects in LDS the candidates that meet the tile (tile_collect) and copies the tile when none does (tile_copy_through); a
// tile with entries is resolved pixel by pixel by a loop of the kernel's own (shared as a skeleton over a lambda it cost the
// redaction's blur 0.8 %).  What a collected entry is is the caller's lambda; every function here is inlined into the kernel,
// so each `return` stays the kernel's own and workgroup-uniform, and every barrier stands outside the lambda.  The host half holds
// the checks and the launch set-up the two entry points share.
#pragma once
#include "common.hpp"

#define TILE_THREADS 256

__host__ __device__ static inline bool tile_usable(double v) { return fabs(v) < 1073741824.0; }    // false for NaN and the infinities
template <typename T> __host__ __device__ static inline T tile_min(T a, T b) { return b < a ? b : a; }
template <typename T> __host__ __device__ static inline T tile_max(T a, T b) { return b > a ? b : a; }

// n bytes from src to dst by lanes q of nq: 16-byte words where both addresses allow the same ones, else dwords, else bytes; the bytes in
// front of the first whole word and behind the last one go as bytes.
__device__ static inline void tile_copy(uint8_t* dst, const uint8_t* src, size_t n, int q, int nq) {
    const uintptr_t d = (uintptr_t)dst, s = (uintptr_t)src;
    const size_t word = ((d ^ s) & 15) == 0 ? 16 : (((d ^ s) & 3) == 0 ? 4 : 1);
    size_t head = (word - (d & (word - 1))) & (word - 1);
    if (head > n) head = n;
    const size_t body = (n - head) / word;
    for (size_t i = q; i < head; i += nq) dst[i] = src[i];
    if (word == 16) {
        u32x4* dw = (u32x4*)(dst + head);
        const u32x4* sw = (const u32x4*)(src + head);
        for (size_t i = q; i < body; i += nq) dw[i] = sw[i];
    } else if (word == 4) {
        unsigned* dw = (unsigned*)(dst + head);
        const unsigned* sw = (const unsigned*)(src + head);
        for (size_t i = q; i < body; i += nq) dw[i] = sw[i];
    }
    for (size_t i = head + (word > 1 ? body * word : 0) + q; i < n; i += nq) dst[i] = src[i];
}

// The workgroup's tile: frame blockIdx.y's record, the tile's origin and its size clipped to the frame.
struct FrameTile { dbx_overlay_frame fm; int x0, y0, rows, cols; };

// Opens tile blockIdx.x (of tiles_x per tile row) of frame blockIdx.y; false -- for the whole workgroup -- when the record is null or
// out of range or the tile lies outside the frame: the kernel returns.
template <int TW, int TH>
__device__ __forceinline__ bool tile_open(const dbx_overlay_frame* frames, int tiles_x, int max_h, int max_w, FrameTile& t) {
    t.fm = frames[blockIdx.y];
    t.x0 = (int)(blockIdx.x % tiles_x) * TW; t.y0 = (int)(blockIdx.x / tiles_x) * TH;
    // (one test without short cuts: the kernel's arguments are then loaded together, not one behind each branch)
    if ((!t.fm.src) | (!t.fm.dst) | (t.fm.h < 1) | (t.fm.w < 1) | (t.fm.h > max_h) | (t.fm.w > max_w) | (t.x0 >= t.fm.w) | (t.y0 >= t.fm.h)) return false;
    t.rows = min(TH, t.fm.h - t.y0); t.cols = min(TW, t.fm.w - t.x0);
    return true;
}

// Whether the rectangle xa..xb x ya..yb (inclusive) meets the tile.
template <typename T> __device__ __forceinline__ bool tile_meets(const FrameTile& t, T xa, T xb, T ya, T yb) {
    return xa < (T)t.x0 + t.cols && xb >= t.x0 && ya < (T)t.y0 + t.rows && yb >= t.y0;
}

// Candidates 0..total-1, 256 at a time: make(i, e) says whether candidate i meets the tile and, if so, leaves its entry in e; the
// entries are compacted into list by a ballot prefix, in candidate order.  Returns their number, the same in every thread.  Called by
// the whole workgroup; total is uniform.
template <typename Ent, typename Make> __device__ __forceinline__ int tile_collect(Ent* list, int total, Make make) {
    __shared__ int wsum[TILE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0;
    for (int c0 = 0; c0 < total; c0 += TILE_THREADS) {
        const int i = c0 + tid;
        Ent e;
        const bool hit = i < total && make(i, e);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < TILE_THREADS / 64; ++w) { off += w < wave ? wsum[w] : 0; sum += wsum[w]; }
        if (hit) list[cnt + off + __popcll(m & ((1ull << lane) - 1ull))] = e;
        cnt += sum;
        __syncthreads();                                           // wsum is rewritten by the next chunk; the list is read by the caller
    }
    return cnt;
}

// The tile that no candidate meets: copied row segment by row segment, TW / 4 lanes each (nothing to do in place).
template <int TW> __device__ __forceinline__ void tile_copy_through(const FrameTile& t, int c) {
    constexpr int NQ = TW / 4;
    const int tid = threadIdx.x;
    const size_t nb = (size_t)t.cols * c;
    for (int rr = tid / NQ; t.fm.dst != t.fm.src && rr < t.rows; rr += TILE_THREADS / NQ) {
        const size_t o = ((size_t)(t.y0 + rr) * t.fm.w + t.x0) * c;
        tile_copy(t.fm.dst + o, t.fm.src + o, nb, tid & (NQ - 1), NQ);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host's half
static int tile_dims_check(const char* fn, int32_t c, int32_t max_h, int32_t max_w) {
    DBX_REQUIRE(c >= 1 && c <= 4, "%s: c=%d must be 1..4", fn, c);
    DBX_REQUIRE(max_h >= 1 && max_w >= 1, "%s: max_h=%d and max_w=%d must be positive", fn, max_h, max_w);
    return DBX_OK;
}

// The grid of `batch` frames of at most max_h x max_w pixels in TW x TH tiles, and its tiles per tile row.
template <int TW, int TH> static int tile_grid(const char* fn, int32_t max_h, int32_t max_w, int32_t batch, dim3* grid, int* tiles_x) {
    const int64_t tx = ((int64_t)max_w + TW - 1) / TW, ty = ((int64_t)max_h + TH - 1) / TH;
    DBX_REQUIRE(tx * ty < (1 << 24) && batch <= 65535, "%s: %lld tiles x %d frames exceed one grid (2^24 - 1 tiles, 65535 frames)", fn,
                (long long)(tx * ty), batch);
    *grid = dim3((unsigned)(tx * ty), (unsigned)batch);
    *tiles_x = (int)tx;
    return DBX_OK;
}

// A launch of `lds` bytes of dynamic LDS: above the default limit, raises the kernel's to its worst case, once per device.
template <auto Kernel> static int tile_lds_limit(size_t lds, size_t worst) {
    static DbxDevOnce attr_once;
    int attr_dev = 0;
    if (lds > 32768 && attr_once.pending(&attr_dev)) {
        DBX_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)worst));
        attr_once.mark(attr_dev);
    }
    return DBX_OK;
}
