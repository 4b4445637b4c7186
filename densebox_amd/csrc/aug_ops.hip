// Training patch augmentation on the device (include/densebox_hip.h, "training patch augmentation"): ONE workgroup decides a parameter
// record and the labels per slot (dbx_patch_aug_plan); a workgroup per 16-row band of a slot makes the pixels (dbx_patch_augment).
// Integer arithmetic throughout; the per-pixel functions and the parameter derivation are __host__ __device__ and exported for the CPU
// suite (dbx_patch_aug_params_host, dbx_patch_augment_host).
#include "common.hpp"
#include "patch_hash.hpp"
#include "patch_stage.hpp"

static_assert(sizeof(dbx_patch_aug) == 64 && sizeof(dbx_patch_aug_cfg) == 112 && sizeof(dbx_patch_aug_io) == 72, "augmentation ABI layouts");
static_assert(offsetof(dbx_patch_aug, key_lo) == 32 && offsetof(dbx_patch_aug, gain) == 40 && offsetof(dbx_patch_aug_cfg, kind_w) == 32 &&
              offsetof(dbx_patch_aug_cfg, box_lo) == 44 && offsetof(dbx_patch_aug_cfg, G) == 100, "augmentation ABI layouts");

#define AUG_HALO 2
#define AUG_MAX_G 65536
#define AUG_Q_MAX 65535

__host__ __device__ inline int aug_u8(int v) { return patch_clamp(v, 0, 255); }

// what a kernel reads of a record
__host__ __device__ inline void aug_sanitize(dbx_patch_aug* a, int G) {
    a->flags &= 3;
    if (a->blur < 0 || a->blur > 3) a->blur = 0;
    if (a->blur == 3 && (a->box_len < 3 || a->box_len > 9 || !(a->box_len & 1))) a->blur = 0;
    a->sat = patch_clamp(a->sat, 0, AUG_Q_MAX);
    a->contrast = patch_clamp(a->contrast, 0, AUG_Q_MAX);
    a->brightness = patch_clamp(a->brightness, -255, 255);
    if (a->curve < 0 || a->curve >= G) a->curve = -1;
    a->noise_amp = patch_clamp(a->noise_amp, 0, AUG_Q_MAX);
    for (int k = 0; k < 3; ++k) { a->gain[k] = patch_clamp(a->gain[k], 0, AUG_Q_MAX); a->reserved[k] = 0; }
}

__host__ __device__ inline bool aug_identity(const dbx_patch_aug& a, int c) {
    return !(a.flags & 1) && a.blur == 0 && (c < 3 || a.sat == 256) && a.contrast == 256 && a.brightness == 0 && a.curve < 0 &&
           a.noise_amp == 0 && a.gain[0] == 256 && a.gain[1] == 256 && a.gain[2] == 256;
}

// the record of slot s in device mode: a fixed draw number per field
__host__ __device__ inline void aug_draw(const dbx_patch_aug_cfg& f, int64_t seed, int64_t counter, int s, dbx_patch_aug* a) {
    a->flags = patch_unit(patch_hash(seed, counter, s, 0)) < f.p_flip ? 1 : 0;
    const bool blur_on = patch_unit(patch_hash(seed, counter, s, 1)) < f.p_blur;
    const int w0 = f.kind_w[0], w1 = f.kind_w[1], wsum = w0 + w1 + f.kind_w[2];
    int kind = 0;
    if (wsum > 0) {
        const int w = (int)((patch_hash(seed, counter, s, 2) >> 11) % (uint64_t)wsum);
        kind = w < w0 ? 1 : (w < w0 + w1 ? 2 : 3);
    }
    a->blur = blur_on ? kind : 0;
    a->box_len = f.box_lo + 2 * (int)((patch_hash(seed, counter, s, 3) >> 11) % (uint64_t)((f.box_hi - f.box_lo) / 2 + 1));
    a->sat = patch_range(patch_hash(seed, counter, s, 4), f.sat_lo, f.sat_hi);
    a->contrast = patch_range(patch_hash(seed, counter, s, 5), f.contrast_lo, f.contrast_hi);
    a->brightness = patch_range(patch_hash(seed, counter, s, 6), f.brightness_lo, f.brightness_hi);
    const bool curve_on = patch_unit(patch_hash(seed, counter, s, 7)) < f.p_curve;
    a->curve = curve_on ? patch_range(patch_hash(seed, counter, s, 8), f.curve_lo, f.curve_hi) : -1;
    const bool noise_on = patch_unit(patch_hash(seed, counter, s, 9)) < f.p_noise;
    a->noise_amp = noise_on ? patch_range(patch_hash(seed, counter, s, 10), f.noise_lo, f.noise_hi) : 0;
    const uint64_t key = patch_hash(seed, counter, s, 11);
    a->key_lo = (int32_t)(uint32_t)key;
    a->key_hi = (int32_t)(uint32_t)(key >> 32);
    for (int k = 0; k < 3; ++k) {
        a->gain[k] = patch_range(patch_hash(seed, counter, s, 12 + k), f.gain_lo, f.gain_hi);
        a->reserved[k] = 0;
    }
}

// One slot of the plan: the sanitised record with the flip decided, and the label row that goes with it.
__host__ __device__ inline void aug_plan_slot(const dbx_patch_aug_cfg& f, const dbx_patch_aug* injected, int64_t seed, int64_t counter, int s,
                                              const int32_t* lin, dbx_patch_aug* a, int32_t* lout) {
    if (injected) *a = *injected;
    else aug_draw(f, seed, counter, s, a);
    aug_sanitize(a, f.G);
    a->flags &= 1;                                     // bit 1 is decided here
    for (int k = 0; k < 12; ++k) lout[k] = lin[k];
    if (!(a->flags & 1) || patch_row_negative(lin)) return;
    const int xs[6] = {lin[0], lin[2], lin[4], lin[6], lin[8], lin[10]};
    for (int k = 0; k < 6; ++k)
        if (xs[k] < 0 || xs[k] > PATCH_SIDE - 1) { a->flags = 2; return; }
    const int m = PATCH_SIDE - 1;
    lout[0] = m - lin[2]; lout[2] = m - lin[0];
    lout[4] = m - lin[6]; lout[5] = lin[7];            // lu' from ru
    lout[6] = m - lin[4]; lout[7] = lin[5];            // ru' from lu
    lout[8] = m - lin[10]; lout[9] = lin[11];          // rd' from ld
    lout[10] = m - lin[8]; lout[11] = lin[9];          // ld' from rd
}

// patch_stage.hpp's policy: the plan kernel and its host loop over aug_plan_slot
struct AugStage {
    typedef dbx_patch_aug_io io_t;
    typedef dbx_patch_aug_cfg cfg_t;
    __host__ __device__ static void slot(const io_t& io, const cfg_t& f, bool device_mode, int64_t seed, int64_t counter, int s) {
        dbx_patch_aug a;
        int32_t lab[12];
        aug_plan_slot(f, device_mode ? nullptr : io.params_in + s, seed, counter, s, io.labels_in + 12 * s, &a, lab);
        io.params[s] = a;
        patch_write_labels(lab, s, io.labels, io.bbox, io.vertices, io.label, patch_row_negative(lab));
    }
};

// entry v of colour channel k's tone table
__host__ __device__ inline int aug_tone(const dbx_patch_aug& a, int k, int v, const unsigned char* curves) {
    const int g = aug_u8((v * a.gain[k] + 128) >> 8);
    const int t = aug_u8((((g - 128) * a.contrast + 128) >> 8) + 128 + a.brightness);
    return a.curve >= 0 ? (int)curves[(size_t)a.curve * 256 + t] : t;
}

// binomial weight i of radius R: [1 2 1] or [1 4 6 4 1]
__host__ __device__ constexpr int aug_weight(int R, int i) { return R == 1 ? (i == 1 ? 2 : 1) : (i == 2 ? 6 : ((i == 1 || i == 3) ? 4 : 1)); }

// The taps are compile-time loops, so all of a pixel's LDS reads are issued before the first is waited for.  Rows first, then columns:
// the intermediates are exact integers, the one rounding comes last.
template <int C, int R, class Rows>
__host__ __device__ inline void aug_binomial(const Rows& rows, int sx, int y, int* v) {
    int cx[2 * R + 1], s[C];
#pragma unroll
    for (int i = 0; i <= 2 * R; ++i) cx[i] = patch_clamp(sx + i - R, 0, PATCH_SIDE - 1);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) s[ch] = 0;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) {
        int h[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) h[ch] = 0;
#pragma unroll
        for (int i = 0; i <= 2 * R; ++i) {
            int q[C];
            rows.template px<C>(y + j - R, cx[i], q);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) h[ch] += aug_weight(R, i) * q[ch];
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) s[ch] += aug_weight(R, j) * h[ch];
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[ch] = R == 1 ? (s[ch] + 8) >> 4 : (s[ch] + 128) >> 8;
}

template <int C, int L, class Rows>
__host__ __device__ inline void aug_box(const Rows& rows, int sx, int y, int* v) {
    int s[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) s[ch] = 0;
#pragma unroll
    for (int dx = -(L / 2); dx <= L / 2; ++dx) {
        int q[C];
        rows.template px<C>(y, patch_clamp(sx + dx, 0, PATCH_SIDE - 1), q);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) s[ch] += q[ch];
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[ch] = (2 * s[ch] + L) / (2 * L);      // a division by a constant
}

// steps 1 and 2: the C channels of pixel (x, y) of the mirrored, blurred image.  rows.px<C>(y, x, q) gives the channels of source
// pixel (x, y) for x in 0..239 and y in -2..241 (replicated outside 0..239).  `a` is sanitised.
template <int C, class Rows>
__host__ __device__ inline void aug_gather(const Rows& rows, const dbx_patch_aug& a, int x, int y, int* v) {
    const int sx = (a.flags & 1) ? PATCH_SIDE - 1 - x : x;   // the weights are symmetric: the taps around the mirrored column
    switch (a.blur) {
        case 1: aug_binomial<C, 1>(rows, sx, y, v); return;
        case 2: aug_binomial<C, 2>(rows, sx, y, v); return;
        case 3:
            switch (a.box_len) {
                case 3: aug_box<C, 3>(rows, sx, y, v); return;
                case 5: aug_box<C, 5>(rows, sx, y, v); return;
                case 7: aug_box<C, 7>(rows, sx, y, v); return;
                default: aug_box<C, 9>(rows, sx, y, v); return;
            }
        default: rows.template px<C>(y, sx, v);
    }
}

// steps 3 to 5 on the colour channels of output pixel number pix = y * 240 + x; tone = the 3 x 256 table
template <int C>
__host__ __device__ inline void aug_finish(const dbx_patch_aug& a, const unsigned char* tone, int pix, int* v) {
    constexpr int K = C < 3 ? C : 3;
    if (C >= 3) {
        const int Y = (v[0] + 2 * v[1] + v[2] + 2) >> 2;
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = aug_u8(Y + (((v[k] - Y) * a.sat + 128) >> 8));
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = tone[256 * k + v[k]];
    if (a.noise_amp > 0) {
        const uint64_t key = ((uint64_t)(uint32_t)a.key_hi << 32) | (uint64_t)(uint32_t)a.key_lo;
        const uint64_t h = patch_mix(key + 0x9E3779B97F4A7C15ull * ((uint64_t)pix + 1ull));
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = (int)((h >> (16 * k)) & 255u) + (int)((h >> (16 * k + 8)) & 255u) - 255;
            const int d = t * a.noise_amp;             // |d| <= 255 * 65535
            v[k] = aug_u8(v[k] + (d >= 0 ? (d + 128) >> 8 : -((-d + 128) >> 8)));
        }
    }
}

struct AugHostRows {
    const unsigned char* patch;
    template <int C>
    void px(int y, int x, int* v) const {
        const unsigned char* p = patch + ((size_t)patch_clamp(y, 0, PATCH_SIDE - 1) * PATCH_SIDE + x) * C;
        for (int ch = 0; ch < C; ++ch) v[ch] = p[ch];
    }
};
// The staged rows in LDS.  A pixel's c <= 4 bytes start at any byte: they are read as the two aligned dwords around them and shifted
// out, since byte reads of neighbouring channels get merged into 16-bit reads at odd addresses, which the LDS serves many times slower.
struct AugLdsRows {
    const unsigned char* sm;                           // 16-byte aligned; row r at r * stride + off
    int off, stride, y_first;
    template <int C>
    __device__ void px(int y, int x, int* v) const {
        const int o = (y - y_first) * stride + off + x * C;
        if (C == 1) { v[0] = sm[o]; return; }
        const unsigned int* w = reinterpret_cast<const unsigned int*>(sm + (o & ~3));
        const unsigned int q = (unsigned int)((((unsigned long long)w[1] << 32) | w[0]) >> (8 * (o & 3)));
#pragma unroll
        for (int ch = 0; ch < C; ++ch) v[ch] = (int)((q >> (8 * ch)) & 255u);
    }
};

template <int C>
static void aug_patch_host(const unsigned char* patch, dbx_patch_aug a, const unsigned char* curves, int G, unsigned char* out) {
    aug_sanitize(&a, G);
    unsigned char tone[3 * 256];
    for (int k = 0; k < 3; ++k)
        for (int v = 0; v < 256; ++v) tone[256 * k + v] = (unsigned char)aug_tone(a, k, v, curves);
    const AugHostRows rows = {patch};
    for (int y = 0; y < PATCH_SIDE; ++y)
        for (int x = 0; x < PATCH_SIDE; ++x) {
            int v[C];
            aug_gather<C>(rows, a, x, y, v);
            aug_finish<C>(a, tone, y * PATCH_SIDE + x, v);
            for (int ch = 0; ch < C; ++ch) out[((size_t)y * PATCH_SIDE + x) * C + ch] = (unsigned char)v[ch];
        }
}

// Workgroup t: band t % 15 (rows 16 * band .. + 15) of slot t / 15.
//   1. Stage: the band's rows and the blur's rows above and below (clamped: the replicated edge) into LDS as aligned 16-byte words,
//      each row at the offset its global address has inside such a word (a patch row is a multiple of 16 bytes, so the offset is one
//      for all rows).  A word that holds one byte of the patch lies in that byte's page, so the bytes around a row are safe to read.
//   2. The 3 x 256 tone table, one entry per thread and colour channel.
//   3. Pixels: thread p, p + 256, ... of the band's 3840; the bytes go to LDS at the offset the band's destination has inside a
//      16-byte word.  The identity record copies instead.
//   4. Stores: patch_band_store (patch_stage.hpp).
template <int C>
__global__ __launch_bounds__(PATCH_THREADS) void patch_augment_kernel(const unsigned char* __restrict__ src, const dbx_patch_aug* __restrict__ params,
                                                                    const int* __restrict__ count, const unsigned char* __restrict__ curves,
                                                                    int G, int n, unsigned char* __restrict__ dst) {
    constexpr int RB = PATCH_SIDE * C, RS = RB + 16, NR = PATCH_BAND + 2 * AUG_HALO, WPR = RB / 16 + 1, NB = PATCH_BAND * RB;
    __shared__ __attribute__((aligned(16))) unsigned char in_sm[NR * RS + 16];     // + 16: the dword pair of the last pixel ends past the last row
    __shared__ __attribute__((aligned(16))) unsigned char out_sm[NB + 16];
    __shared__ unsigned char tone[3 * 256];
    const int tid = threadIdx.x;
    const PatchPart wg = patch_part<PATCH_BANDS>(count, n);
    if (wg.slot >= wg.count) return;                   // uniform over the workgroup
    const int slot = wg.slot;
    dbx_patch_aug a = params[slot];
    aug_sanitize(&a, G);
    const bool copy = aug_identity(a, C);
    const int y0 = wg.part * PATCH_BAND;
    const unsigned char* ps = src + (size_t)slot * PATCH_SIDE * RB;
    const int soff = (int)((size_t)ps & 15);
    const int vr = a.blur == 1 ? 1 : (a.blur == 2 ? 2 : 0);
    const int w_end = (AUG_HALO + PATCH_BAND + vr) * WPR;
    for (int base = (AUG_HALO - vr) * WPR + tid; base < w_end; base += 4 * PATCH_THREADS) {
        uint4 buf[4];                                  // four loads in flight per thread
#pragma unroll
        for (int i = 0; i < 4; ++i) {                  // a word that is not wanted loads the row's first word instead and is not stored
            const int w = base + i * PATCH_THREADS < w_end ? base + i * PATCH_THREADS : w_end - 1;
            const int r = w / WPR, k = 16 * (w % WPR) < soff + RB ? w % WPR : 0;
            const int y = patch_clamp(y0 - AUG_HALO + r, 0, PATCH_SIDE - 1);
            buf[i] = reinterpret_cast<const uint4*>(ps + (size_t)y * RB - soff)[k];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int w = base + i * PATCH_THREADS, r = w / WPR, k = w % WPR;
            if (w < w_end && 16 * k < soff + RB) reinterpret_cast<uint4*>(in_sm + r * RS)[k] = buf[i];   // the last word only when the row reaches into it
        }
    }
    if (!copy) {
        constexpr int K = C < 3 ? C : 3;
#pragma unroll
        for (int k = 0; k < K; ++k) tone[256 * k + tid] = (unsigned char)aug_tone(a, k, tid, curves);
    }
    __syncthreads();
    unsigned char* gd = dst + ((size_t)slot * PATCH_SIDE + y0) * RB;
    const int shift = patch_band_shift(gd);
    const AugLdsRows rows = {in_sm, soff, RS, y0 - AUG_HALO};
    for (int p = tid; p < PATCH_BAND * PATCH_SIDE; p += PATCH_THREADS) {
        const int yy = p / PATCH_SIDE, x = p % PATCH_SIDE;
        int v[C];
        if (copy) {
            rows.template px<C>(y0 + yy, x, v);
        } else {
            aug_gather<C>(rows, a, x, y0 + yy, v);
            aug_finish<C>(a, tone, (y0 + yy) * PATCH_SIDE + x, v);
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out_sm[shift + p * C + ch] = (unsigned char)v[ch];
    }
    __syncthreads();
    patch_band_store<NB>(out_sm, gd, tid);
}

static int aug_check_cfg(const char* who, const dbx_patch_aug_cfg* f) {
    DBX_REQUIRE(f, "%s: null cfg", who);
    const double ps[4] = {f->p_flip, f->p_blur, f->p_curve, f->p_noise};
    const char* pn[4] = {"p_flip", "p_blur", "p_curve", "p_noise"};
    for (int k = 0; k < 4; ++k) DBX_REQUIRE(ps[k] >= 0.0 && ps[k] <= 1.0, "%s: %s=%g must lie in [0, 1]", who, pn[k], ps[k]);
    DBX_REQUIRE(f->G >= 0 && f->G <= AUG_MAX_G, "%s: G=%d must be 0..%d", who, f->G, AUG_MAX_G);
    long long wsum = 0;
    for (int k = 0; k < 3; ++k) {
        DBX_REQUIRE(f->kind_w[k] >= 0 && f->kind_w[k] <= (1 << 20), "%s: blur kind weight %d is %d, must be 0..2^20", who, k, f->kind_w[k]);
        wsum += f->kind_w[k];
    }
    DBX_REQUIRE(wsum > 0 || f->p_blur == 0.0, "%s: p_blur=%g but every blur kind weight is 0", who, f->p_blur);
    DBX_REQUIRE(f->box_lo >= 3 && f->box_hi <= 9 && (f->box_lo & 1) && (f->box_hi & 1) && f->box_lo <= f->box_hi,
                "%s: box length %d..%d must be odd, 3..9, lo <= hi", who, f->box_lo, f->box_hi);
    const int q[4][2] = {{f->sat_lo, f->sat_hi}, {f->contrast_lo, f->contrast_hi}, {f->gain_lo, f->gain_hi}, {f->noise_lo, f->noise_hi}};
    const char* qn[4] = {"saturation", "contrast", "gain", "noise amplitude"};
    for (int k = 0; k < 4; ++k)
        DBX_REQUIRE(q[k][0] >= 0 && q[k][1] <= AUG_Q_MAX && q[k][0] <= q[k][1], "%s: %s range %d..%d must lie in 0..%d, lo <= hi", who, qn[k],
                    q[k][0], q[k][1], AUG_Q_MAX);
    DBX_REQUIRE(f->brightness_lo >= -255 && f->brightness_hi <= 255 && f->brightness_lo <= f->brightness_hi,
                "%s: brightness range %d..%d must lie in -255..255, lo <= hi", who, f->brightness_lo, f->brightness_hi);
    DBX_REQUIRE(f->p_curve == 0.0 || (f->curve_lo >= 0 && f->curve_lo <= f->curve_hi && f->curve_hi < f->G),
                "%s: curve index range %d..%d leaves the bank of G=%d curves", who, f->curve_lo, f->curve_hi, f->G);
    return DBX_OK;
}

extern "C" int dbx_patch_aug_plan(const dbx_patch_aug_io* io, const dbx_patch_aug_cfg* cfg, int32_t n, void* stream) {
    DBX_REQUIRE(io, "patch_aug_plan: null io");
    if (int rc = aug_check_cfg("patch_aug_plan", cfg)) return rc;
    DBX_REQUIRE(n >= 1 && n <= PATCH_MAX_N, "patch_aug_plan: n=%d must be 1..%d", n, PATCH_MAX_N);
    DBX_REQUIRE(io->labels_in && io->count, "patch_aug_plan: null input");
    DBX_REQUIRE(io->params_in || io->state, "patch_aug_plan: null state in device mode");
    DBX_REQUIRE(io->params && io->labels && io->bbox && io->vertices && io->label, "patch_aug_plan: null output");
    hipLaunchKernelGGL(patch_stage_plan_kernel<AugStage>, dim3(1), dim3(PATCH_THREADS), 0, (hipStream_t)stream, *io, *cfg, n);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

static int aug_check_pixels(const char* who, const void* patches, const void* params, const void* curves, int G, int c, const void* out,
                            long long n) {
    DBX_REQUIRE(G >= 0 && G <= AUG_MAX_G, "%s: G=%d must be 0..%d", who, G, AUG_MAX_G);
    DBX_REQUIRE(params && (curves || G == 0), "%s: null argument", who);
    return patch_check_pixels(who, patches, out, c, n, "a blurred band reads its neighbours' rows");
}

extern "C" int dbx_patch_augment(const uint8_t* patches, const dbx_patch_aug* params, const int32_t* count, const uint8_t* curves, int32_t G,
                                 int32_t n, int32_t c, uint8_t* out, void* stream) {
    DBX_REQUIRE(n >= 1 && n <= PATCH_MAX_N, "patch_augment: n=%d must be 1..%d", n, PATCH_MAX_N);
    if (int rc = aug_check_pixels("patch_augment", patches, params, curves, G, c, out, n)) return rc;
    DBX_REQUIRE(count, "patch_augment: null count");
    const dim3 grid((unsigned)n * PATCH_BANDS), block(PATCH_THREADS);
    PATCH_WITH_C(c, hipLaunchKernelGGL(patch_augment_kernel<C>, grid, block, 0, (hipStream_t)stream, patches, params, count, curves, G, n, out));
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_patch_aug_params_host(const dbx_patch_aug_cfg* cfg, int64_t seed, int64_t counter, const dbx_patch_aug* params_in,
                                         const int32_t* labels_in, int32_t count, dbx_patch_aug* params, int32_t* labels, float* bbox,
                                         float* vertices, float* label) {
    if (int rc = aug_check_cfg("patch_aug_params_host", cfg)) return rc;
    DBX_REQUIRE(count >= 0 && count <= PATCH_MAX_N, "patch_aug_params_host: count=%d must be 0..%d", count, PATCH_MAX_N);
    DBX_REQUIRE(count == 0 || (labels_in && params && labels && bbox && vertices && label), "patch_aug_params_host: null argument");
    patch_stage_plan_host<AugStage>({labels_in, nullptr, params_in, nullptr, params, labels, bbox, vertices, label}, *cfg, seed, counter, count);
    return DBX_OK;
}

extern "C" int dbx_patch_augment_host(const uint8_t* patch, const dbx_patch_aug* rec, const uint8_t* curves, int32_t G, int32_t c,
                                      uint8_t* out) {
    if (int rc = aug_check_pixels("patch_augment_host", patch, rec, curves, G, c, out, 1)) return rc;
    PATCH_WITH_C(c, aug_patch_host<C>(patch, *rec, curves, G, out));
    return DBX_OK;
}
