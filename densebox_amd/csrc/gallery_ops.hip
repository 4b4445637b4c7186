// Best-shot gallery behind the plate crops and the tracking update: per track slot the best crop the camera ever saw of the track,
// scored by an exact integer focus measure (dbx_crop_sharpness) or by the detection score, kept on the device (dbx_track_gallery_update)
// and moved into an arena, at the index dbx_track_append gives the track's record, when the track ends.  Every result is an integer or a
// copied word, so the NumPy restatement (tests/gallery_ref.py) gives the same bits whatever the scheduling.
#include "common.hpp"

#include <cmath>

#define GAL_THREADS 256
#define GAL_MAX_PIXELS 16384
#define GAL_MAX_SLOTS 1024
#define GAL_MAX_TRACKS 256
#define GAL_TAIL_BYTES 64            // LDS behind the luma plane: the waves' sums, the arena base, the two searches' results
#define GAL_NONE 0x7fffffff

// Dynamic LDS only (its base stays 16-byte aligned): the luma plane as 16-bit values, rounded up to 16 bytes, then GAL_TAIL_BYTES.
static size_t gal_lds_bytes(int oh, int ow) { return (((size_t)oh * ow * 2 + 15) & ~(size_t)15) + GAL_TAIL_BYTES; }

// The focus measure of one crop [oh][ow][c], by the whole workgroup of GAL_THREADS threads: every thread returns the sum.  luma holds
// oh * ow 16-bit words, wsum GAL_THREADS / 64 sums.  Barriers inside: every thread of the workgroup calls it, with the same arguments;
// luma and wsum may be rewritten behind one more barrier.
__device__ static long long gal_sharpness(const uint8_t* __restrict__ crop, int oh, int ow, int c, unsigned short* luma, long long* wsum) {
    const int tid = threadIdx.x, npix = oh * ow;
    if (oh < 3 || ow < 3) return 0;                                          // uniform
    // four pixels per step from whole dwords where the crop starts on one (3 dwords with c == 3, 1 with c == 1), bytes for the rest
    const int quads = ((uintptr_t)crop & 3) == 0 ? npix >> 2 : 0;
    for (int q = tid; q < quads; q += GAL_THREADS) {
        unsigned short y[4];
        if (c == 3) {
            const unsigned* w = (const unsigned*)(crop + (size_t)q * 12);
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
            y[0] = (unsigned short)((w0 & 255u) + 2u * ((w0 >> 8) & 255u) + ((w0 >> 16) & 255u));
            y[1] = (unsigned short)((w0 >> 24) + 2u * (w1 & 255u) + ((w1 >> 8) & 255u));
            y[2] = (unsigned short)(((w1 >> 16) & 255u) + 2u * (w1 >> 24) + (w2 & 255u));
            y[3] = (unsigned short)(((w2 >> 8) & 255u) + 2u * ((w2 >> 16) & 255u) + (w2 >> 24));
        } else {
            const unsigned w0 = *(const unsigned*)(crop + (size_t)q * 4);
            y[0] = (unsigned short)(4u * (w0 & 255u)); y[1] = (unsigned short)(4u * ((w0 >> 8) & 255u));
            y[2] = (unsigned short)(4u * ((w0 >> 16) & 255u)); y[3] = (unsigned short)(4u * (w0 >> 24));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) luma[q * 4 + k] = y[k];
    }
    for (int p = quads * 4 + tid; p < npix; p += GAL_THREADS) {
        const uint8_t* v = crop + (size_t)p * c;
        luma[p] = (unsigned short)(c == 3 ? v[0] + 2 * v[1] + v[2] : 4 * v[0]);
    }
    __syncthreads();
    const int iw = ow - 2, inner = (oh - 2) * iw;
    long long acc = 0;
    for (int p = tid; p < inner; p += GAL_THREADS) {
        const int y = p / iw, x = p - y * iw;
        const unsigned short* m = luma + (y + 1) * ow + x + 1;
        const int l = 4 * (int)m[0] - (int)m[-ow] - (int)m[ow] - (int)m[-1] - (int)m[1];          // |l| <= 4080: l * l fits 32 bits
        acc += (long long)(l * l);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    long long sum = 0;
#pragma unroll
    for (int w = 0; w < GAL_THREADS / 64; ++w) sum += wsum[w];
    return sum;
}

__global__ __launch_bounds__(GAL_THREADS) void crop_sharpness_kernel(const uint8_t* crops, long long n, int oh, int ow, int c,
                                                                     long long* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gal_sm[];
    unsigned short* luma = (unsigned short*)gal_sm;
    long long* wsum = (long long*)(gal_sm + (((size_t)oh * ow * 2 + 15) & ~(size_t)15));
    const size_t bytes = (size_t)oh * ow * c;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const long long s = gal_sharpness(crops + (size_t)i * bytes, oh, ow, c, luma, wsum);
        if (threadIdx.x == 0) out[i] = s;
        __syncthreads();                                                     // luma and wsum are rewritten by the next crop
    }
}

extern "C" int dbx_crop_sharpness(const uint8_t* crops, int64_t n, int32_t oh, int32_t ow, int32_t c, int64_t* out, void* stream) {
    const char* fn = "crop_sharpness";
    DBX_REQUIRE(n >= 0, "%s: n=%lld is negative", fn, (long long)n);
    DBX_REQUIRE(c == 1 || c == 3, "%s: c=%d must be 1 or 3", fn, c);
    DBX_REQUIRE(oh >= 1 && ow >= 1 && (int64_t)oh * ow <= GAL_MAX_PIXELS, "%s: a crop of %d x %d pixels is not 1..%d pixels", fn, ow, oh,
                GAL_MAX_PIXELS);
    DBX_REQUIRE(crops && out, "%s: null argument", fn);
    if (n == 0) return DBX_OK;
    const unsigned blocks = (unsigned)(n < (1 << 20) ? n : (1 << 20));
    hipLaunchKernelGGL(crop_sharpness_kernel, dim3(blocks), dim3(GAL_THREADS), gal_lds_bytes(oh, ow), (hipStream_t)stream, crops,
                       (long long)n, oh, ow, c, (long long*)out);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}

// n bytes from src to dst by the whole workgroup (src == nullptr: zeros): 16-byte words where both addresses allow the same ones, else
// dwords, else bytes; the bytes in front of the first whole word and behind the last one go as bytes.
__device__ static void gal_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    const int tid = threadIdx.x;
    const uintptr_t d = (uintptr_t)dst, s = src ? (uintptr_t)src : d;
    const size_t word = ((d ^ s) & 15) == 0 ? 16 : (((d ^ s) & 3) == 0 ? 4 : 1);
    size_t head = (word - (d & (word - 1))) & (word - 1);
    if (head > n) head = n;
    const size_t body = (n - head) / word;
    for (size_t i = tid; i < head; i += GAL_THREADS) dst[i] = src ? src[i] : (uint8_t)0;
    if (word == 16) {
        u32x4* dw = (u32x4*)(dst + head);
        const u32x4* sw = (const u32x4*)(src + head);
        for (size_t i = tid; i < body; i += GAL_THREADS) dw[i] = src ? sw[i] : (u32x4){0u, 0u, 0u, 0u};
    } else if (word == 4) {
        unsigned* dw = (unsigned*)(dst + head);
        const unsigned* sw = (const unsigned*)(src + head);
        for (size_t i = tid; i < body; i += GAL_THREADS) dw[i] = src ? sw[i] : 0u;
    }
    for (size_t i = head + (word > 1 ? body * word : 0) + tid; i < n; i += GAL_THREADS) dst[i] = src ? src[i] : (uint8_t)0;
}

struct GalleryArgs {
    const dbx_track* tracks; const int* headers; const int* track_slot; const uint8_t* crops; const int* ok;
    const dbx_track* retired; const int* tally; const long long* append_state;
    dbx_shot* shots; uint8_t* shot_crops; dbx_shot_record* arena; uint8_t* arena_crops; unsigned long long* gstate;
    long long capacity;
    double min_score;
    int batch, slots, stream0, max_tracks, oh, ow, c, policy, commit;
};

// One workgroup per (track slot t, frame b).  Everything a branch depends on is the same in every thread (words read by all of them, or
// LDS words behind a barrier), so the barriers inside the branches are reached by the whole workgroup or by none of it.  The slot's
// entry lives in registers (the same copy in every thread) and is written once, by thread 0, at the end; the slot's crop is written
// last as well, behind the barrier that ends the arena copy's reads of it.
__global__ __launch_bounds__(GAL_THREADS) void track_gallery_update_kernel(const GalleryArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gal_sm[];
    unsigned short* luma = (unsigned short*)gal_sm;
    unsigned char* tail = gal_sm + (((size_t)a.oh * a.ow * 2 + 15) & ~(size_t)15);
    long long* wsum = (long long*)tail;                                      // 32 bytes
    unsigned long long* base = (unsigned long long*)(tail + 32);             // the retired records of the frames in front of b
    int* found = (int*)(tail + 40);                                          // [0] the record's place in retired[b], [1] the list position
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, T = a.max_tracks;
    const size_t s = (size_t)(a.stream0 + b);
    const size_t bytes = (size_t)a.oh * a.ow * a.c;
    dbx_shot* gp = a.shots + s * T + t;
    const dbx_track* kp = a.tracks + s * T + t;
    const int gid0 = gp->id, kid = kp->id;
    if (gid0 < 0 && kid < 0) return;                                         // a free slot that stays free: most workgroups
    dbx_shot g = *gp;
    const double kscore = kp->score;
    const int f = a.headers[s * 4] - 1;
    uint8_t* mine = a.shot_crops + (s * T + t) * bytes;
    if (tid == 0) { *base = 0ull; found[0] = GAL_NONE; found[1] = GAL_NONE; }
    __syncthreads();

    const bool ended = gid0 >= 0 && kid != gid0;
    const bool adopt = kid >= 0 && (ended || gid0 != kid);                   // G.id is -1 behind step 1
    int outcome = -1;                                                        // the gstate word next to `ended`: 1 stored, 2 lost, 3 dropped
    if (ended) {
        const int c0 = a.tally[(size_t)b * 6 + 4];
        const int rb = c0 < 0 ? 0 : (c0 > T ? T : c0);
        if (tid < rb && a.retired[(size_t)b * T + tid].id == gid0) atomicMin(&found[0], tid);
        unsigned long long part = 0;
        for (int q = tid; q < b; q += GAL_THREADS) {
            const int cq = a.tally[(size_t)q * 6 + 4];
            part += (unsigned long long)(cq < 0 ? 0 : (cq > T ? T : cq));
        }
        if (part) atomicAdd(base, part);
        __syncthreads();
        const int n = found[0];
        const long long cursor = a.append_state[0];
        if (n == GAL_NONE) {
            outcome = 2;
        } else {
            const long long at = cursor + (long long)*base + n;
            if (cursor >= 0 && at < a.capacity) {
                outcome = 1;
                if (a.commit) {
                    gal_copy(a.arena_crops + (size_t)at * bytes, mine, bytes);
                    if (tid == 0) {
                        dbx_shot_record r;
                        r.stream = (int)s; r.slot = t; r.shot = g;
                        a.arena[at] = r;
                    }
                }
            } else {
                outcome = 3;
            }
        }
        g.id = -1;
    }
    if (adopt) {
        g.key = -INFINITY; g.score = NAN; g.sharpness = 0;
        g.id = kid; g.frame = -1; g.shots = 0; g.reserved = 0;
    }
    const uint8_t* take = nullptr;                                           // the crop that replaces the slot's
    if (kid >= 0) {
        for (int j = tid; j < a.slots; j += GAL_THREADS)
            if (a.track_slot[(size_t)b * a.slots + j] == t) atomicMin(&found[1], j);
        __syncthreads();
        const int j = found[1];
        if (j != GAL_NONE && a.ok[(size_t)b * a.slots + j] != 0 && kscore >= a.min_score) {
            const uint8_t* crop = a.crops + ((size_t)b * a.slots + j) * bytes;
            const long long sh = gal_sharpness(crop, a.oh, a.ow, a.c, luma, wsum);
            const double key = a.policy == 0 ? (double)sh : kscore;
            const bool first = g.shots == 0;
            g.shots += 1;
            if (first || key > g.key) {
                g.key = key; g.score = kscore; g.sharpness = sh; g.frame = f;
                take = crop;
            }
        }
    }
    if (!a.commit) return;
    __syncthreads();                                                         // the arena copy has read the slot's crop
    if (take) gal_copy(mine, take, bytes);
    else if (adopt) gal_copy(mine, nullptr, bytes);
    if (tid == 0) {
        *gp = g;
        if (ended) {
            atomicAdd(a.gstate, 1ull);
            atomicAdd(a.gstate + outcome, 1ull);
        }
    }
}

extern "C" int dbx_track_gallery_update(const dbx_track* tracks, const int32_t* headers, const int32_t* track_slot, const uint8_t* crops,
                                        const int32_t* ok, const dbx_track* retired, const int32_t* tally, const int64_t* append_state,
                                        dbx_shot* shots, uint8_t* shot_crops, dbx_shot_record* arena, uint8_t* arena_crops,
                                        int64_t* gstate, int32_t batch, int32_t slots, int32_t streams, int32_t stream0, int32_t max_tracks,
                                        int32_t oh, int32_t ow, int32_t c, int64_t capacity, int32_t policy, double min_score,
                                        int32_t commit, void* stream) {
    static_assert(sizeof(dbx_shot) == 40 && sizeof(dbx_shot_record) == 48, "dbx_shot is 40 bytes, dbx_shot_record 48");
    static_assert(32 + 8 + 2 * sizeof(int) <= GAL_TAIL_BYTES, "the words behind the luma plane");
    const char* fn = "track_gallery_update";
    DBX_REQUIRE(batch >= 0, "%s: batch=%d is negative", fn, batch);
    DBX_REQUIRE(stream0 >= 0 && streams >= 0 && (int64_t)stream0 + batch <= streams, "%s: streams %d..%lld are not all in 0..%d", fn, stream0,
                (long long)stream0 + batch - 1, streams - 1);
    DBX_REQUIRE(slots >= 1 && slots <= GAL_MAX_SLOTS, "%s: slots=%d must be 1..%d", fn, slots, GAL_MAX_SLOTS);
    DBX_REQUIRE(max_tracks >= 1 && max_tracks <= GAL_MAX_TRACKS, "%s: max_tracks=%d must be 1..%d", fn, max_tracks, GAL_MAX_TRACKS);
    DBX_REQUIRE(c == 1 || c == 3, "%s: c=%d must be 1 or 3", fn, c);
    DBX_REQUIRE(oh >= 1 && ow >= 1 && (int64_t)oh * ow <= GAL_MAX_PIXELS, "%s: a crop of %d x %d pixels is not 1..%d pixels", fn, ow, oh,
                GAL_MAX_PIXELS);
    DBX_REQUIRE(capacity >= 0, "%s: capacity=%lld is negative", fn, (long long)capacity);
    DBX_REQUIRE(policy == 0 || policy == 1, "%s: policy=%d must be 0 (sharpness) or 1 (score)", fn, policy);
    DBX_REQUIRE(!std::isnan(min_score), "%s: min_score must not be NaN", fn);
    if (batch == 0) return DBX_OK;
    DBX_REQUIRE(tracks && headers && track_slot && crops && ok && retired && tally && append_state && shots && shot_crops && gstate &&
                    ((arena && arena_crops) || capacity == 0), "%s: null argument", fn);
    DBX_REQUIRE(batch <= 65535, "%s: batch=%d exceeds one grid's 65535 frames", fn, batch);
    GalleryArgs a;
    a.tracks = tracks; a.headers = headers; a.track_slot = track_slot; a.crops = crops; a.ok = ok; a.retired = retired; a.tally = tally;
    a.append_state = (const long long*)append_state; a.shots = shots; a.shot_crops = shot_crops; a.arena = arena; a.arena_crops = arena_crops;
    a.gstate = (unsigned long long*)gstate; a.capacity = capacity; a.min_score = min_score;
    a.batch = batch; a.slots = slots; a.stream0 = stream0; a.max_tracks = max_tracks; a.oh = oh; a.ow = ow; a.c = c; a.policy = policy;
    a.commit = commit != 0;
    hipLaunchKernelGGL(track_gallery_update_kernel, dim3((unsigned)max_tracks, (unsigned)batch), dim3(GAL_THREADS), gal_lds_bytes(oh, ow),
                       (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
