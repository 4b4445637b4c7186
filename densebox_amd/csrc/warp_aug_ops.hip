// Training patch warp on the device (include/densebox_hip.h, "training patch warp"): ONE workgroup decides a record, the label row and
// the two 3 x 3 matrices per slot (dbx_patch_warp_plan); a workgroup per 16-row band of a slot makes the pixels (dbx_patch_warp).  The
// solve, the inverse and the pixel arithmetic are the rectification's (warp_px.hpp); fp contraction is off in the whole file, so the
// __host__ __device__ functions round alike on both sides and are exported for the CPU suite (dbx_patch_warp_params_host,
// dbx_patch_warp_host).
#pragma clang fp contract(off)
#include "common.hpp"
#include "patch_hash.hpp"
#include "patch_stage.hpp"
#include "warp_px.hpp"

static_assert(sizeof(dbx_patch_warp_rec) == 64 && sizeof(dbx_patch_warp_cfg) == 72 && sizeof(dbx_patch_warp_io) == 96, "warp ABI layouts");
static_assert(offsetof(dbx_patch_warp_rec, quad) == 16 && offsetof(dbx_patch_warp_rec, scale) == 48 && offsetof(dbx_patch_warp_cfg, rot_lo) == 8 &&
              offsetof(dbx_patch_warp_cfg, tx) == 40 && offsetof(dbx_patch_warp_cfg, R) == 64, "warp ABI layouts");

#define WARP_MAX_R 65536
#define WARP_QUAD_MAX (1 << 20)
#define WARP_HALF 1912                                 // 119.5 pixels in 1/16 pixel
#define WARP_FULL (16 * (PATCH_SIDE - 1))

__host__ __device__ inline bool warp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN

// what a kernel reads of a record
__host__ __device__ inline void warp_sanitize(dbx_patch_warp_rec* r) {
    r->flags &= 1;
    if (r->border < 0 || r->border > 1) r->border = 0;
    for (int k = 0; k < 8; ++k) r->quad[k] = patch_clamp(r->quad[k], -WARP_QUAD_MAX, WARP_QUAD_MAX);
    r->reserved = 0;
}

// the record of slot s in device mode: a fixed draw number per field
__host__ __device__ inline void warp_draw(const dbx_patch_warp_cfg& f, const int32_t* bank, int64_t seed, int64_t counter, int s,
                                          dbx_patch_warp_rec* r) {
    const bool on = patch_unit(patch_hash(seed, counter, s, 0)) < f.p_warp;
    r->flags = on ? 1 : 0;
    r->border = f.border;
    r->fill = f.fill;
    r->rot = patch_range(patch_hash(seed, counter, s, 1), f.rot_lo, f.rot_hi);
    r->scale = patch_range(patch_hash(seed, counter, s, 2), f.scale_lo, f.scale_hi);
    r->aspect = patch_range(patch_hash(seed, counter, s, 3), f.aspect_lo, f.aspect_hi);
    r->shear = patch_range(patch_hash(seed, counter, s, 4), f.shear_lo, f.shear_hi);
    r->reserved = 0;
    const int ident[8] = {0, 0, WARP_FULL, 0, WARP_FULL, WARP_FULL, 0, WARP_FULL};
    for (int k = 0; k < 8; ++k) r->quad[k] = ident[k];
    if (!on) return;                                   // the bank is not read
    const int64_t t[2] = {patch_range(patch_hash(seed, counter, s, 5), -f.tx, f.tx), patch_range(patch_hash(seed, counter, s, 6), -f.ty, f.ty)};
    const int64_t co = bank[2 * r->rot], si = bank[2 * r->rot + 1];
    const int64_t sc = r->scale, as = r->aspect, sh = r->shear;
    for (int k = 0; k < 4; ++k) {
        const int64_t px = (k == 1 || k == 2) ? WARP_HALF : -WARP_HALF, py = k >= 2 ? WARP_HALF : -WARP_HALF;
        int64_t u = (px * sc * as) >> 16;
        const int64_t v = (py * sc) >> 8;
        u += (sh * v) >> 8;
        const int64_t xy[2] = {(co * u - si * v + 32768) >> 16, (si * u + co * v + 32768) >> 16};
        for (int a = 0; a < 2; ++a) {
            const int64_t q = xy[a] + WARP_HALF + t[a] + patch_range(patch_hash(seed, counter, s, 7 + 2 * k + a), -f.jitter, f.jitter);
            r->quad[2 * k + a] = (int)(q < -WARP_QUAD_MAX ? -WARP_QUAD_MAX : (q > WARP_QUAD_MAX ? WARP_QUAD_MAX : q));
        }
    }
}

// vertex (vx, vy) through m: false where the label rule refuses it
__host__ __device__ inline bool warp_vertex(const double* m, int vx, int vy, int margin, int* ox, int* oy) {
    const double W = m[6] * vx + m[7] * vy + m[8];
    if (!warp_finite(W) || !(W > 0.0)) return false;
    const double fx = (m[0] * vx + m[1] * vy + m[2]) / W + 0.5, fy = (m[3] * vx + m[4] * vy + m[5]) / W + 0.5;
    if (!(fx > -1.0 && fx < (double)PATCH_SIDE && fy > -1.0 && fy < (double)PATCH_SIDE)) return false;   // also NaN; the casts below are defined
    const int x = (int)fx, y = (int)fy;
    if (x < margin || x > PATCH_SIDE - 1 - margin || y < margin || y > PATCH_SIDE - 1 - margin) return false;
    *ox = x; *oy = y;
    return true;
}

// One slot of the plan: the sanitised record with its refusal bits, the label row and the two matrices that go with it.
__host__ __device__ inline void warp_plan_slot(const dbx_patch_warp_cfg& f, const dbx_patch_warp_rec* injected, const int32_t* bank, int64_t seed,
                                               int64_t counter, int s, const int32_t* lin, dbx_patch_warp_rec* r, int32_t* lout, double* fwd,
                                               double* inv) {
    if (injected) *r = *injected;
    else warp_draw(f, bank, seed, counter, s, r);
    warp_sanitize(r);
    const bool negative = patch_row_negative(lin);
    for (int k = 0; k < 12; ++k) lout[k] = lin[k];
    for (int k = 0; k < 9; ++k) fwd[k] = inv[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (!(r->flags & 1)) return;
    const double e = (double)(PATCH_SIDE - 1);
    const double sq[8] = {0.0, 0.0, e, 0.0, e, e, 0.0, e};
    double d[8], m[9], im[9];
    for (int k = 0; k < 8; ++k) d[k] = (double)r->quad[k] / 16.0;
    bool ok = perspective_solve(sq, d, m);
    ok = ok && warp_inverse(m, im);
    if (ok)
        for (int k = 0; k < 9; ++k) ok = ok && warp_finite(m[k]) && warp_finite(im[k]);
    if (!ok) { r->flags = 4; return; }
    if (!negative) {
        int v[8];
        bool keep = true;
        for (int k = 0; k < 4; ++k) keep = keep && warp_vertex(m, lin[4 + 2 * k], lin[5 + 2 * k], f.margin, &v[2 * k], &v[2 * k + 1]);
        int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
        if (keep) {                                    // v = lu, ru, rd, ld
            bx0 = v[0] < v[6] ? v[0] : v[6]; bx1 = v[2] > v[4] ? v[2] : v[4];
            by0 = v[1] < v[3] ? v[1] : v[3]; by1 = v[7] > v[5] ? v[7] : v[5];
            keep = bx1 > bx0 && by1 > by0;
        }
        if (!keep) { r->flags = 2; return; }
        lout[0] = bx0; lout[1] = by0; lout[2] = bx1; lout[3] = by1;
        for (int k = 0; k < 8; ++k) lout[4 + k] = v[k];
    }
    for (int k = 0; k < 9; ++k) { fwd[k] = m[k]; inv[k] = im[k]; }
}

// patch_stage.hpp's policy: the plan kernel and its host loop over warp_plan_slot
struct WarpStage {
    typedef dbx_patch_warp_io io_t;
    typedef dbx_patch_warp_cfg cfg_t;
    __host__ __device__ static void slot(const io_t& io, const cfg_t& f, bool device_mode, int64_t seed, int64_t counter, int s) {
        dbx_patch_warp_rec r;
        int32_t lab[12];
        double fwd[9], inv[9];
        warp_plan_slot(f, device_mode ? nullptr : io.params_in + s, io.rot, seed, counter, s, io.labels_in + 12 * s, &r, lab, fwd, inv);
        io.params[s] = r;
        patch_write_labels(lab, s, io.labels, io.bbox, io.vertices, io.label, patch_row_negative(lab));
        for (int k = 0; k < 9; ++k) { io.fwd[9 * s + k] = fwd[k]; io.inv[9 * s + k] = inv[k]; }
    }
};

// the C channels of output pixel (x, y) of a slot, channel ch in byte ch; r is sanitised
template <int C>
__host__ __device__ inline unsigned int warp_pixel(const unsigned char* patch, const dbx_patch_warp_rec& r, const double* im, int x, int y) {
    if (!(r.flags & 1)) {
        unsigned int px = 0;
        for (int ch = 0; ch < C; ++ch) px |= (unsigned int)patch[((size_t)y * PATCH_SIDE + x) * C + ch] << (8 * ch);
        return px;
    }
    if (r.border) return warp_px_u8_border<1>(im, patch, PATCH_SIDE, PATCH_SIDE, C, x, y, 0u);
    return warp_px_u8_border<0>(im, patch, PATCH_SIDE, PATCH_SIDE, C, x, y, (unsigned int)r.fill);
}

template <int C>
static void warp_patch_host(const unsigned char* patch, dbx_patch_warp_rec r, const double* im, unsigned char* out) {
    warp_sanitize(&r);
    for (int y = 0; y < PATCH_SIDE; ++y)
        for (int x = 0; x < PATCH_SIDE; ++x) {
            const unsigned int px = warp_pixel<C>(patch, r, im, x, y);
            for (int ch = 0; ch < C; ++ch) out[((size_t)y * PATCH_SIDE + x) * C + ch] = (unsigned char)(px >> (8 * ch));
        }
}

// Workgroup t: band t % 15 (rows 16 * band .. + 15) of slot t / 15.
//   1. Pixels: thread p, p + 256, ... of the band's 3840, so the lanes of a wave make 64 CONSECUTIVE output pixels and their gathers
//      cover a narrow span of the source patch, which is read in place (a batch of patches is cache resident).  The bytes go to LDS at
//      the offset the band's destination has inside a 16-byte word.  A slot with bit 0 clear copies instead.
//   2. Stores: patch_band_store (patch_stage.hpp).
// Whatever inv holds, warp_px_u8_border reads inside the slot's 240 x 240 patch only.
template <int C>
__global__ __launch_bounds__(PATCH_THREADS) void patch_warp_kernel(const unsigned char* __restrict__ src, const dbx_patch_warp_rec* __restrict__ params,
                                                                  const double* __restrict__ inv, const int* __restrict__ count, int n,
                                                                  unsigned char* __restrict__ dst) {
    constexpr int RB = PATCH_SIDE * C, NB = PATCH_BAND * RB;
    __shared__ __attribute__((aligned(16))) unsigned char out_sm[NB + 16];
    const int tid = threadIdx.x;
    const PatchPart wg = patch_part<PATCH_BANDS>(count, n);
    if (wg.slot >= wg.count) return;                   // uniform over the workgroup
    const int slot = wg.slot;
    dbx_patch_warp_rec r = params[slot];
    warp_sanitize(&r);
    double im[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) im[k] = inv[9 * (size_t)slot + k];
    const int y0 = wg.part * PATCH_BAND;
    const unsigned char* ps = src + (size_t)slot * PATCH_SIDE * RB;
    unsigned char* gd = dst + ((size_t)slot * PATCH_SIDE + y0) * RB;
    const int shift = patch_band_shift(gd);
    for (int p = tid; p < PATCH_BAND * PATCH_SIDE; p += PATCH_THREADS) {
        const int yy = p / PATCH_SIDE, x = p % PATCH_SIDE;
        const unsigned int px = warp_pixel<C>(ps, r, im, x, y0 + yy);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out_sm[shift + p * C + ch] = (unsigned char)(px >> (8 * ch));
    }
    __syncthreads();
    patch_band_store<NB>(out_sm, gd, tid);
}

static int warp_check_cfg(const char* who, const dbx_patch_warp_cfg* f, bool device_mode, const void* bank) {
    DBX_REQUIRE(f, "%s: null cfg", who);
    DBX_REQUIRE(f->p_warp >= 0.0 && f->p_warp <= 1.0, "%s: p_warp=%g must lie in [0, 1]", who, f->p_warp);
    DBX_REQUIRE(f->R >= 0 && f->R <= WARP_MAX_R, "%s: R=%d must be 0..%d", who, f->R, WARP_MAX_R);
    DBX_REQUIRE(f->rot_lo <= f->rot_hi && f->rot_lo >= -WARP_QUAD_MAX && f->rot_hi <= WARP_QUAD_MAX,
                "%s: rot range %d..%d must lie in -2^20..2^20, lo <= hi", who, f->rot_lo, f->rot_hi);
    const int q[2][2] = {{f->scale_lo, f->scale_hi}, {f->aspect_lo, f->aspect_hi}};
    const char* qn[2] = {"scale", "aspect"};
    for (int k = 0; k < 2; ++k)
        DBX_REQUIRE(q[k][0] >= 1 && q[k][1] <= 65535 && q[k][0] <= q[k][1], "%s: %s range %d..%d must lie in 1..65535, lo <= hi", who, qn[k], q[k][0],
                    q[k][1]);
    DBX_REQUIRE(f->shear_lo >= -65535 && f->shear_hi <= 65535 && f->shear_lo <= f->shear_hi,
                "%s: shear range %d..%d must lie in -65535..65535, lo <= hi", who, f->shear_lo, f->shear_hi);
    const int t[3] = {f->tx, f->ty, f->jitter};
    const char* tn[3] = {"tx", "ty", "jitter"};
    for (int k = 0; k < 3; ++k) DBX_REQUIRE(t[k] >= 0 && t[k] <= 65536, "%s: %s=%d must be 0..2^16 (1/16 pixel)", who, tn[k], t[k]);
    DBX_REQUIRE(f->margin >= 0 && f->margin <= 119, "%s: margin=%d must be 0..119", who, f->margin);
    DBX_REQUIRE(f->border >= 0 && f->border <= 1, "%s: border=%d must be 0 (constant) or 1 (replicate)", who, f->border);
    DBX_REQUIRE(f->p_warp == 0.0 || (f->rot_lo >= 0 && f->rot_hi < f->R), "%s: rot index range %d..%d leaves the bank of R=%d rows", who, f->rot_lo,
                f->rot_hi, f->R);
    DBX_REQUIRE(!device_mode || f->p_warp == 0.0 || bank, "%s: null rot bank in device mode with p_warp > 0", who);
    return DBX_OK;
}

extern "C" int dbx_patch_warp_plan(const dbx_patch_warp_io* io, const dbx_patch_warp_cfg* cfg, int32_t n, void* stream) {
    DBX_REQUIRE(io, "patch_warp_plan: null io");
    if (int rc = warp_check_cfg("patch_warp_plan", cfg, io->params_in == nullptr, io->rot)) return rc;
    DBX_REQUIRE(n >= 1 && n <= PATCH_MAX_N, "patch_warp_plan: n=%d must be 1..%d", n, PATCH_MAX_N);
    DBX_REQUIRE(io->labels_in && io->count, "patch_warp_plan: null input");
    DBX_REQUIRE(io->params_in || io->state, "patch_warp_plan: null state in device mode");
    DBX_REQUIRE(io->params && io->labels && io->bbox && io->vertices && io->label && io->fwd && io->inv, "patch_warp_plan: null output");
    hipLaunchKernelGGL(patch_stage_plan_kernel<WarpStage>, dim3(1), dim3(PATCH_THREADS), 0, (hipStream_t)stream, *io, *cfg, n);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

static int warp_check_pixels(const char* who, const void* patches, const void* params, const void* inv, int c, const void* out, long long n) {
    DBX_REQUIRE(params && inv, "%s: null argument", who);
    return patch_check_pixels(who, patches, out, c, n, "a warped pixel reads anywhere in its patch");
}

extern "C" int dbx_patch_warp(const uint8_t* patches, const dbx_patch_warp_rec* params, const double* inv, const int32_t* count, int32_t n,
                              int32_t c, uint8_t* out, void* stream) {
    DBX_REQUIRE(n >= 1 && n <= PATCH_MAX_N, "patch_warp: n=%d must be 1..%d", n, PATCH_MAX_N);
    if (int rc = warp_check_pixels("patch_warp", patches, params, inv, c, out, n)) return rc;
    DBX_REQUIRE(count, "patch_warp: null count");
    const dim3 grid((unsigned)n * PATCH_BANDS), block(PATCH_THREADS);
    PATCH_WITH_C(c, hipLaunchKernelGGL(patch_warp_kernel<C>, grid, block, 0, (hipStream_t)stream, patches, params, inv, count, n, out));
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

extern "C" int dbx_patch_warp_params_host(const dbx_patch_warp_cfg* cfg, int64_t seed, int64_t counter, const dbx_patch_warp_rec* params_in,
                                          const int32_t* rot, const int32_t* labels_in, int32_t count, dbx_patch_warp_rec* params,
                                          int32_t* labels, float* bbox, float* vertices, float* label, double* fwd, double* inv) {
    if (int rc = warp_check_cfg("patch_warp_params_host", cfg, params_in == nullptr, rot)) return rc;
    DBX_REQUIRE(count >= 0 && count <= PATCH_MAX_N, "patch_warp_params_host: count=%d must be 0..%d", count, PATCH_MAX_N);
    DBX_REQUIRE(count == 0 || (labels_in && params && labels && bbox && vertices && label && fwd && inv), "patch_warp_params_host: null argument");
    patch_stage_plan_host<WarpStage>({labels_in, nullptr, params_in, nullptr, rot, params, labels, bbox, vertices, label, fwd, inv}, *cfg, seed, counter,
                                     count);
    return DBX_OK;
}

extern "C" int dbx_patch_warp_host(const uint8_t* patch, const dbx_patch_warp_rec* rec, const double* inv, int32_t c, uint8_t* out) {
    if (int rc = warp_check_pixels("patch_warp_host", patch, rec, inv, c, out, 1)) return rc;
    PATCH_WITH_C(c, warp_patch_host<C>(patch, *rec, inv, out));
    return DBX_OK;
}
