// What the training-patch stages share on the device -- patch_ops.hip (plan + cut), warp_aug_ops.hip (warp) and aug_ops.hip (augment)
// -- once: the constants of a stage that works a 16-row band of a 240 x 240 slot per workgroup, the label row's three outputs, the plan
// kernel and its host loop over a per-stage policy, the band kernels' prologue and store, the pixel entry points' common checks and the
// dispatch over the channel count.  The per-pixel loop stays in each kernel: the two produce differently shaped values.  Every function
// here is inlined into its kernel, so a `return` stays the kernel's own and workgroup-uniform.
//
// This header is compiled with fp contraction off (patch_ops.hip, warp_aug_ops.hip) and on (aug_ops.hip) and must give the same bits
// under both: it holds NO floating-point expression that contraction could change, that is, no multiply that feeds an add.  A division
// and a cast, as in patch_write_labels, are safe.
#pragma once
#include "common.hpp"

#define PATCH_THREADS 256
#define PATCH_SIDE DBX_PATCH_SIDE
#define PATCH_BAND 16
#define PATCH_BANDS (PATCH_SIDE / PATCH_BAND)
#define PATCH_MAX_N 4096

__host__ __device__ inline int patch_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// draw h as an integer in lo..hi, for any int lo <= hi
__host__ __device__ inline int patch_range(uint64_t h, int lo, int hi) {
    return (int)((int64_t)lo + (int64_t)((h >> 11) % (uint64_t)((int64_t)hi - (int64_t)lo + 1)));
}

// all twelve integers are zero: the slot is a negative
__host__ __device__ inline bool patch_row_negative(const int32_t* row) {
    bool negative = true;
    for (int k = 0; k < 12; ++k) negative = negative && row[k] == 0;
    return negative;
}

// slot s of the label outputs: the integer row, net.loss's float32 inputs (the integers / 4) and the label flag
__host__ __device__ inline void patch_write_labels(const int32_t* row, int s, int32_t* labels, float* bbox, float* vertices, float* label,
                                                   bool is_negative) {
    for (int k = 0; k < 12; ++k) labels[12 * s + k] = row[k];
    for (int k = 0; k < 4; ++k) bbox[4 * s + k] = (float)((double)row[k] / 4.0);
    for (int k = 0; k < 8; ++k) vertices[8 * s + k] = (float)((double)row[4 + k] / 4.0);
    label[s] = is_negative ? 0.0f : 1.0f;
}

// The plan of a stage that follows the cut.  Stage names io_t and cfg_t (the dbx_patch_*_io and _cfg structs) and has
//     static void slot(io, cfg, device_mode, seed, counter, s)
// which decides slot s -- from io.params_in[s], or in device mode from the hash of (seed, counter, s) -- and writes its rows.
// One workgroup, slot k * PATCH_THREADS + tid in pass k.
template <class Stage>
__global__ __launch_bounds__(PATCH_THREADS) void patch_stage_plan_kernel(typename Stage::io_t io, typename Stage::cfg_t cfg, int n) {
    const int tid = threadIdx.x;
    const bool device_mode = io.params_in == nullptr;
    const int64_t seed = device_mode ? io.state[0] : 0, counter = device_mode ? io.state[1] : 0;
    const int cnt = patch_clamp(*io.count, 0, n);
    for (int s = tid; s < cnt; s += PATCH_THREADS) Stage::slot(io, cfg, device_mode, seed, counter, s);
    __syncthreads();                                   // every thread has read the counter
    if (tid == 0 && device_mode) io.state[1] = counter + 1;
}

// the same slots on the host, for the *_params_host exports; io.count and io.state are not read
template <class Stage>
inline void patch_stage_plan_host(const typename Stage::io_t& io, const typename Stage::cfg_t& cfg, int64_t seed, int64_t counter, int count) {
    for (int s = 0; s < count; ++s) Stage::slot(io, cfg, io.params_in == nullptr, seed, counter, s);
}

// Workgroup t of a kernel with PARTS workgroups per slot: part t % PARTS of slot t / PARTS, and the count clamped to n.  The kernel
// returns when slot >= count, which is uniform over the workgroup.
struct PatchPart { int slot, part, count; };
template <int PARTS>
__device__ inline PatchPart patch_part(const int* count, int n) {
    const int cnt = *count;
    return {(int)(blockIdx.x / PARTS), (int)(blockIdx.x % PARTS), cnt < n ? cnt : n};
}

// A band kernel makes its NB bytes in out_sm (16-byte aligned, NB + 16 bytes) at the offset the band's destination gd has inside a
// 16-byte word: byte b of the band is out_sm[patch_band_shift(gd) + b].  After a barrier patch_band_store moves them: the band is ONE
// contiguous block of the output; its aligned 16-byte words, and at the two ends whole dwords, then bytes.
__device__ inline int patch_band_shift(const unsigned char* gd) { return (int)((size_t)gd & 15); }

template <int NB>
__device__ inline void patch_band_store(const unsigned char* out_sm, unsigned char* gd, int tid) {
    const int shift = patch_band_shift(gd), end = shift + NB;
    unsigned char* gw = gd - shift;                    // 16-byte aligned; byte b of the band is gw[shift + b] = out_sm[shift + b]
    for (int k = tid; 16 * k < end; k += PATCH_THREADS) {
        const int b0 = 16 * k;
        if (b0 >= shift && b0 + 16 <= end) {
            reinterpret_cast<uint4*>(gw)[k] = reinterpret_cast<const uint4*>(out_sm)[k];
        } else {
            for (int j = b0; j < b0 + 16; j += 4) {
                if (j >= shift && j + 4 <= end) {
                    reinterpret_cast<unsigned int*>(gw)[j >> 2] = reinterpret_cast<const unsigned int*>(out_sm)[j >> 2];
                } else {
                    for (int q = j < shift ? shift : j; q < j + 4 && q < end; ++q) gw[q] = out_sm[q];
                }
            }
        }
    }
}

// what the pixel entry points of the band stages check alike; `why`: what the stage reads that forbids working in place
static int patch_check_pixels(const char* who, const void* patches, const void* out, int c, long long n, const char* why) {
    DBX_REQUIRE(c >= 1 && c <= 4, "%s: c=%d must be 1..4", who, c);
    DBX_REQUIRE(patches && out, "%s: null argument", who);
    const uintptr_t a = (uintptr_t)patches, b = (uintptr_t)out, bytes = (uintptr_t)(n * PATCH_SIDE * PATCH_SIDE * c);
    DBX_REQUIRE((a >= b ? a - b : b - a) >= bytes, "%s: patches and out overlap (out of place only: %s)", who, why);
    return DBX_OK;
}

// the statement with C = c as a constant expression; c is 1..4 (checked by the caller)
#define PATCH_WITH_C(c, ...)                                 \
    switch (c) {                                             \
        case 1: { constexpr int C = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int C = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int C = 3; __VA_ARGS__; } break; \
        default: { constexpr int C = 4; __VA_ARGS__; } break; \
    }
