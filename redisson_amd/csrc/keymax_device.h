// keymax_device.h -- the per-key maximum of the bit streams' summary passes (k_bs_summary of
// bitstream_kernels.hip, k_fs_summary of fieldstream_kernels.hip): keymax[canonical key] = the largest "end" (1 +
// the last bit written) among the key's writing commands that run, 0 = none.  It is an atomicMax kept rare: a
// lane holds its maximum back while its commands stay on one key, a load that already shows as much settles it
// without the atomic, and the lanes of a wave that end on one key send one.  (One atomicMax per SETBIT measured
// 191 ms for 2^24 SETBITs on ONE key, every one of them on the same word, against 2.2 ms on 4,096 keys.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rbx {

// keymax[key] = max(keymax[key], m); m = 0: nothing.  The word only rises during the pass, so a load that
// shows m or more settles it; the load goes past the L1, which other CUs' atomics do not refresh.
__device__ __forceinline__ void keymax_raise(unsigned long long *keymax, uint32_t key, unsigned long long m) {
    if (m == 0) return;
    if (__hip_atomic_load(keymax + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= m) return;
    atomicMax(keymax + key, m);
}

// what one lane holds back over its loop
struct KeymaxHeld {
    uint32_t key = ~0u;          // the key whose maximum this lane holds back
    unsigned long long end = 0;  // that maximum (0 = nothing held)
    // a writing command that runs, on canonical key `canon`, ending at `e` > 0
    __device__ __forceinline__ void take(unsigned long long *keymax, uint32_t canon, unsigned long long e) {
        if (canon != key) {
            keymax_raise(keymax, key, end);
            key = canon;
            end = 0;
        }
        end = max(end, e);
    }
    // after the loop, every lane of the workgroup together: one atomic per wave when its lanes all hold the
    // same key (a batch on few keys); a wave that holds nothing sends m = 0, which raises nothing
    __device__ __forceinline__ void flush(unsigned long long *keymax) const {
        uint32_t lo = end ? key : ~0u;
        unsigned long long m = end;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
            m = max(m, (unsigned long long)__shfl_xor(m, d, 64));
        }
        if (__all(!end || key == lo)) {
            if ((threadIdx.x & 63) == 0) keymax_raise(keymax, lo, m);
        } else {
            keymax_raise(keymax, key, end);
        }
    }
};

}  // namespace rbx
