// bitrange_device.h -- the device pieces of ranged BITCOUNT / BITPOS that bitrange_kernels.hip and
// rangestream_kernels.hip share: one aligned 16-byte vector masked to a bit interval, its count and its first
// hit, and the per-wave walkers over an interval.
//
// Layout (bitset_kernels.hip): bit i = byte i>>3, mask 0x80 >> (i&7), the bytes read as little-endian
// words.  A byte-swapped word holds string position j (0..31) at bit 31 - j, so the first position of a
// word is a count of leading zeros, and the positions [a, b] are (~0u >> a) & (~0u << (31 - b)).
#pragma once
#include <hip/hip_runtime.h>

#include "rbx_kernels.h"

namespace rbx {

constexpr uint32_t kBlockBits = 32768;  // a directory block (launch_bits_directory): 4 KiB of the string
constexpr int kBlockLog2 = 15;

// string positions >= a / <= b of a byte-swapped word (a, b relative to the word's first position)
__device__ __forceinline__ uint32_t pos_from(int64_t a) { return a <= 0 ? ~0u : (a >= 32 ? 0u : ~0u >> (int)a); }
__device__ __forceinline__ uint32_t pos_to(int64_t b) { return b < 0 ? 0u : (b >= 31 ? ~0u : ~0u << (31 - (int)b)); }

// Vector v as loaded -> byte-swapped words holding a one at every position of [lo, hi] whose bit is the wanted
// one: FLIP = false the set bits (BITCOUNT, BITPOS 1), FLIP = true the clear ones (BITPOS 0: complementing and
// then clearing the positions out of range is OR-ing them in and looking for a zero).
template <bool FLIP> __device__ __forceinline__ uint4 vec_wanted(uint4 x, uint64_t v, uint64_t lo, uint64_t hi) {
    x = make_uint4(__builtin_bswap32(x.x), __builtin_bswap32(x.y), __builtin_bswap32(x.z), __builtin_bswap32(x.w));
    if (FLIP) x = make_uint4(~x.x, ~x.y, ~x.z, ~x.w);
    const int64_t a = (int64_t)lo - (int64_t)(v << 7), b = (int64_t)hi - (int64_t)(v << 7);
    x.x &= pos_from(a) & pos_to(b);
    x.y &= pos_from(a - 32) & pos_to(b - 32);
    x.z &= pos_from(a - 64) & pos_to(b - 64);
    x.w &= pos_from(a - 96) & pos_to(b - 96);
    return x;
}

__device__ __forceinline__ uint32_t popc4(const uint4 &x) { return __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w); }

// the first position (0..127) of a vec_wanted vector that holds a one; 128 = none
__device__ __forceinline__ uint32_t vec_first(const uint4 &x) {
    if (x.x) return (uint32_t)__builtin_clz(x.x);
    if (x.y) return 32u + (uint32_t)__builtin_clz(x.y);
    if (x.z) return 64u + (uint32_t)__builtin_clz(x.z);
    if (x.w) return 96u + (uint32_t)__builtin_clz(x.w);
    return 128u;
}

// the ones of [lo, hi], in every lane
__device__ __forceinline__ uint64_t wave_count(const uint4 *__restrict__ vecs, uint64_t lo, uint64_t hi, uint32_t lane) {
    const uint64_t v1 = hi >> 7;
    uint64_t c = 0;
    for (uint64_t v = (lo >> 7) + lane; v <= v1; v += 64) c += popc4(vec_wanted<false>(vecs[v], v, lo, hi));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    return c;
}

// the first position of [lo, hi] that holds the wanted bit, in every lane; kBitsNone = none
template <bool FLIP>
__device__ __forceinline__ uint64_t wave_find(const uint4 *__restrict__ vecs, uint64_t lo, uint64_t hi, uint32_t lane) {
    const uint64_t v1 = hi >> 7;
    for (uint64_t base = lo >> 7; base <= v1; base += 64) {
        const uint64_t v = base + lane;
        uint32_t f = 128u;
        if (v <= v1) f = vec_first(vec_wanted<FLIP>(vecs[v], v, lo, hi));
        const unsigned long long m = __ballot(f < 128u);
        if (m) {
            const int src = __ffsll(m) - 1;
            return ((base + (uint64_t)src) << 7) + (uint32_t)__shfl((int)f, src, 64);
        }
    }
    return kBitsNone;
}

// ---- what the kernels over many strings share (rangestream_kernels.hip, members_kernels.hip) ----
// the string of command (k, c) as the kernels read it: its length (clamped to the allocation, which the host
// keeps at or above it) and whether the key is missing
__device__ __forceinline__ uint64_t rs_len(const BitKey &k, bool *missing) {
    *missing = k.len == nullptr;
    return *missing ? 0 : min((uint64_t)*k.len, k.cap_bits >> 3);
}

// the tiles of an interval: its vectors cut into runs of tile_vecs, from the interval's first vector
__device__ __forceinline__ uint64_t rs_tiles(uint64_t lo, uint64_t hi, uint32_t tile_lg) {
    return (((hi >> 7) - (lo >> 7)) >> (tile_lg - 4)) + 1;
}

}  // namespace rbx
