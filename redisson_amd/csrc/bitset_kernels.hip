// bitset_kernels.hip -- RBitSet over the engine's bitmap strings (M/RedissonBitSet.java): BITOP,
// range fill, and batched SETBIT / GETBIT by raw index.  A bitmap is the Redis string's bytes
// (bit i = byte i>>3, mask 0x80 >> (i&7)), read as little-endian u32 words: word i>>5, bit
// (i^7)&31 (rbx_device.h bit_in_word).  Every kernel keeps the invariant the contains kernels
// rely on: the bytes from the string's length up to the allocation's end are zero.
// M/ = /root/reference/redisson/src/main/java/org/redisson/
#include <hip/hip_runtime.h>

#include "../../include/rbx.h"
#include "bitop_device.h"
#include "bloom_common.h"
#include "rbx_kernels.h"

namespace rbx {

// ---------------------------------------------------------------------------------
// BITOP ([redis-7.2] bitops.c bitopCommand, restated): dest := op(src_0 .. src_{n-1}) over
// max(len_s) bytes, a source reading as zero past its own end.  One pass for any n: lane l of a
// sweep owns the 16 bytes at one offset, reads them from every source and only then stores them,
// so dst may be any of the sources.  No pointer is __restrict__ for that reason.
//
// The sweep covers `span` bytes (a multiple of 16 within dst's allocation): the result, and
// whatever longer string dst held before, which is cleared -- as are the bytes of the last
// vector past out_len (NOT would otherwise turn them into ones).
// A source is read with a 16-byte load only where the whole vector lies inside its string;
// the vector holding its last bytes is assembled byte by byte, and nothing past len is touched.
// ---------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(256) void k_bitop(uint8_t *dst, unsigned long long *dst_len, const BitopSrc *srcs,
                                               uint32_t nsrc, uint64_t out_len, uint64_t span) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16;
    for (uint64_t o = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; o < span; o += stride) {
        uint4 r = make_uint4(0, 0, 0, 0);
        if (o < out_len) {
            r = bitop_load(srcs[0], o);
            if (OP == RBX_BITOP_NOT) r = make_uint4(~r.x, ~r.y, ~r.z, ~r.w);
            for (uint32_t s = 1; s < nsrc; ++s) {
                const uint4 v = bitop_load(srcs[s], o);
                if (OP == RBX_BITOP_AND) r = make_uint4(r.x & v.x, r.y & v.y, r.z & v.z, r.w & v.w);
                if (OP == RBX_BITOP_OR) r = make_uint4(r.x | v.x, r.y | v.y, r.z | v.z, r.w | v.w);
                if (OP == RBX_BITOP_XOR) r = make_uint4(r.x ^ v.x, r.y ^ v.y, r.z ^ v.z, r.w ^ v.w);
            }
            if (o + 16 > out_len) {  // the result's last vector: zero past out_len
                const int64_t n = (int64_t)(out_len - o);
                r.x &= low_bytes(n);
                r.y &= low_bytes(n - 4);
                r.z &= low_bytes(n - 8);
                r.w &= low_bytes(n - 12);
            }
        }
        *(uint4 *)(dst + o) = r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst_len = out_len;
}

void launch_bitop(int op, uint8_t *dst, unsigned long long *dst_len, const BitopSrc *d_srcs, uint32_t nsrc,
                  uint64_t out_len, uint64_t span, hipStream_t st) {
    const unsigned grid = grid_for(span / 16, kMaxGrid);
    switch (op) {
    case RBX_BITOP_AND:
        hipLaunchKernelGGL(k_bitop<RBX_BITOP_AND>, dim3(grid), dim3(256), 0, st, dst, dst_len, d_srcs, nsrc, out_len, span);
        break;
    case RBX_BITOP_OR:
        hipLaunchKernelGGL(k_bitop<RBX_BITOP_OR>, dim3(grid), dim3(256), 0, st, dst, dst_len, d_srcs, nsrc, out_len, span);
        break;
    case RBX_BITOP_XOR:
        hipLaunchKernelGGL(k_bitop<RBX_BITOP_XOR>, dim3(grid), dim3(256), 0, st, dst, dst_len, d_srcs, nsrc, out_len, span);
        break;
    default:
        hipLaunchKernelGGL(k_bitop<RBX_BITOP_NOT>, dim3(grid), dim3(256), 0, st, dst, dst_len, d_srcs, nsrc, out_len, span);
        break;
    }
}

// ---------------------------------------------------------------------------------
// set(from, to, value) / clear(from, to) (M/RedissonBitSet.java:442-454: one SETBIT per index):
// bits [from, to), from < to <= 8 * capacity.  Words wholly inside the range are stored (four at a
// time where a 16-byte vector lies inside it); the word holding `from` and the word holding `to`
// -- the same word for a short range -- are read, masked and written back by one lane.
// ---------------------------------------------------------------------------------
// the bits of a word at in-word indexes [0, b), b in 0..32 (MSB-first inside each byte)
__device__ __forceinline__ uint32_t bits_below(uint32_t b) {
    if (b >= 32) return ~0u;
    const uint32_t whole = b >> 3;
    return ((1u << (8 * whole)) - 1) | (((0xFF00u >> (b & 7)) & 0xFFu) << (8 * whole));
}

__global__ __launch_bounds__(256) void k_bits_fill(uint32_t *words, unsigned long long *len, uint64_t from, uint64_t to,
                                                   uint32_t value) {
    const uint64_t w_from = from >> 5, w_to = to >> 5;
    const uint64_t fw = (from + 31) >> 5;  // whole words [fw, w_to)
    const uint32_t fill = value ? ~0u : 0u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (fw >> 2) + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q * 4 < w_to; q += stride) {
        const uint64_t w = q * 4;
        if (w >= fw && w + 4 <= w_to) {
            *(uint4 *)(words + w) = make_uint4(fill, fill, fill, fill);
        } else {
            for (uint64_t j = w; j < w + 4; ++j)
                if (j >= fw && j < w_to) words[j] = fill;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool head = (from & 31) != 0;
        if (head) {
            const uint64_t end = to - (w_from << 5);  // in-word end of the range, capped at the word
            const uint32_t m = bits_below(end > 32 ? 32u : (uint32_t)end) & ~bits_below((uint32_t)(from & 31));
            words[w_from] = value ? (words[w_from] | m) : (words[w_from] & ~m);
        }
        if ((to & 31) != 0 && !(head && w_to == w_from)) {
            const uint32_t m = bits_below((uint32_t)(to & 31));
            words[w_to] = value ? (words[w_to] | m) : (words[w_to] & ~m);
        }
        atomicMax(len, (unsigned long long)(((to - 1) >> 3) + 1));  // SETBIT grows the string whatever the value
    }
}

void launch_bits_fill(uint32_t *words, unsigned long long *len, uint64_t from, uint64_t to, bool value, hipStream_t st) {
    const unsigned grid = grid_for((to - from) / 128 + 2, kMaxGrid);
    hipLaunchKernelGGL(k_bits_fill, dim3(grid), dim3(256), 0, st, words, len, from, to, value ? 1u : 0u);
}

// ---------------------------------------------------------------------------------
// n raw indexes: SETBIT (set(long[], boolean), M/RedissonBitSet.java:312-324) and GETBIT (:277-279).
// Every element of a scatter carries the same value, so duplicates and the order are immaterial.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bits_scatter(uint32_t *words, unsigned long long *len, uint64_t cap_bits,
                                                      const uint64_t *__restrict__ idx, uint64_t n, uint32_t value,
                                                      uint64_t new_len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t b = idx[i];
        if (b >= cap_bits) continue;  // the host sized the bitmap from the maximum: never taken
        if (value) atomicOr(words + (b >> 5), bit_in_word((uint32_t)b));
        else atomicAnd(words + (b >> 5), ~bit_in_word((uint32_t)b));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(len, (unsigned long long)new_len);
}

// out[i] = GETBIT idx[i]; 0 at or past 8 * capacity (and past the string's end: those bytes are zero)
__global__ __launch_bounds__(256) void k_bits_gather(const uint32_t *__restrict__ words, uint64_t cap_bits,
                                                     const uint64_t *__restrict__ idx, uint64_t n,
                                                     uint8_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t b = idx[i];
        out[i] = b < cap_bits ? (uint8_t)((words[b >> 5] & bit_in_word((uint32_t)b)) != 0) : (uint8_t)0;
    }
}

// *out = max(*out, max idx): the host's range check, growth and new length
__global__ __launch_bounds__(256) void k_bits_max(const uint64_t *__restrict__ idx, uint64_t n, unsigned long long *out) {
    __shared__ unsigned long long s_part[4];
    unsigned long long m = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = max(m, (unsigned long long)idx[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned long long)__shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out, max(max(s_part[0], s_part[1]), max(s_part[2], s_part[3])));
}

// SETBIT index value -> the old bit (M/RedissonBitSet.java:302-305), one lane
__global__ void k_bits_set_one(uint32_t *words, unsigned long long *len, uint64_t b, uint32_t value,
                               unsigned long long *old) {
    const uint32_t m = bit_in_word((uint32_t)b);
    const uint32_t w = value ? atomicOr(words + (b >> 5), m) : atomicAnd(words + (b >> 5), ~m);
    *old = (w & m) != 0;
    atomicMax(len, (unsigned long long)((b >> 3) + 1));
}

void launch_bits_scatter(uint32_t *words, unsigned long long *len, uint64_t cap_bits, const uint64_t *d_idx, uint64_t n,
                         bool value, uint64_t new_len, hipStream_t st) {
    hipLaunchKernelGGL(k_bits_scatter, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, words, len, cap_bits, d_idx, n,
                       value ? 1u : 0u, new_len);
}

void launch_bits_gather(const uint32_t *words, uint64_t cap_bits, const uint64_t *d_idx, uint64_t n, uint8_t *d_out,
                        hipStream_t st) {
    hipLaunchKernelGGL(k_bits_gather, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, words, cap_bits, d_idx, n, d_out);
}

void launch_bits_max(const uint64_t *d_idx, uint64_t n, unsigned long long *d_out, hipStream_t st) {
    hipLaunchKernelGGL(k_bits_max, dim3(grid_for(n, 512)), dim3(256), 0, st, d_idx, n, d_out);
}

void launch_bits_set_one(uint32_t *words, unsigned long long *len, uint64_t bit, bool value, unsigned long long *d_old,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_bits_set_one, dim3(1), dim3(1), 0, st, words, len, bit, value ? 1u : 0u, d_old);
}

}  // namespace rbx
