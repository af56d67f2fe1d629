// bitop_device.h -- what BITOP's kernels share (bitset_kernels.hip k_bitop, bitgroups_kernels.hip k_bg_sweep): a
// source's 16 bytes at an offset, read without touching anything at or past its length, and the byte mask of the
// result's last vector.
#pragma once
#include <hip/hip_runtime.h>

#include "rbx_device.h"
#include "rbx_kernels.h"

namespace rbx {

__device__ __forceinline__ uint4 bitop_load(const BitopSrc &s, uint64_t o) {
    if (o + 16 <= s.len) return ld_nt16(s.bytes + o);
    uint32_t w[4] = {0, 0, 0, 0};
    if (o < s.len) {
        const int n = (int)(s.len - o);  // 1..15
#pragma unroll
        for (int j = 0; j < 15; ++j)  // unrolled: w[] stays in registers
            if (j < n) w[j >> 2] |= (uint32_t)s.bytes[o + j] << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the low min(max(n, 0), 4) bytes of a word
__device__ __forceinline__ uint32_t low_bytes(int64_t n) {
    return n >= 4 ? ~0u : (n <= 0 ? 0u : (1u << (8 * (int)n)) - 1);
}

}  // namespace rbx
