// The counter-based hash of the training-patch kernels (patch_ops.hip, aug_ops.hip), for device and host alike.
//     mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
//     h = mix(mix(seed + 0x9E3779B97F4A7C15 * (counter + 1)) + 0xD1B54A32D192ED03 * (i + 1) + 0x8CB92BA72F3D8DD7 * (j + 1))
// k = h >> 11 is the 53-bit draw: a probability test is k * 2^-53 < p, an integer in a range of r values is k mod r.
#pragma once
#include <stdint.h>

__host__ __device__ inline uint64_t patch_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
__host__ __device__ inline uint64_t patch_hash(int64_t seed, int64_t counter, int i, int j) {
    const uint64_t a = patch_mix((uint64_t)seed + 0x9E3779B97F4A7C15ull * ((uint64_t)counter + 1ull));
    return patch_mix(a + 0xD1B54A32D192ED03ull * ((uint64_t)i + 1ull) + 0x8CB92BA72F3D8DD7ull * ((uint64_t)j + 1ull));
}
__host__ __device__ inline double patch_unit(uint64_t h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }     // k * 2^-53
