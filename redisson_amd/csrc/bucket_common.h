// bucket_common.h -- helpers shared by the region-partitioned Bloom pipelines
// (contains_partitioned.hip, add_partitioned.hip), on top of bloom_common.h: the run stores, the
// partitioned contains' geometry, the LDS bucket scan and the phase timer.
#pragma once

#include "bk_entry.h"
#include "bloom_common.h"

namespace rbx {

// Stores of the partition passes' runs: non-temporal (plain stores, which keep the line in the XCD's
// L2, measured slower: DESIGN.md r02).
template <class T> __device__ __forceinline__ void run_store(T v, T *p) { __builtin_nontemporal_store(v, p); }

// Partitioned contains, one radix pass (contains_partitioned.hip).  Stage 1 buckets entries by
// 2^21-bit (256 KiB) bitmap region, at most 2048 of them; the probe holds one 2^20-bit (128 KiB)
// slice of a region in LDS, and the two workgroups of a cluster hold the two slices of one region.
// The region size, the stage-1 tile and grid and the entry's line (kBkLineEntries entries, copied
// as kBkLineWords u64) are bk_entry.h's.
constexpr uint32_t kBkCS = 2;                                                   // workgroups per cluster
constexpr uint32_t kBkSliceBits = kBkBucketBits - 1;                            // bits per slice
constexpr uint32_t kBkSliceWords = 1u << (kBkSliceBits - 5);
constexpr uint32_t kBkMaxBuckets = 1u << (32 - kBkBucketBits);                  // filters hold <= 2^32 bits

// exclusive scan of cnt[0..nb) (nb <= 64 * PER, PER consecutive buckets per lane) by wave 0 into
// start[] and pos[]
template <int PER>
__device__ __forceinline__ void bk_scan(const uint32_t *cnt, uint32_t nb, uint32_t *start, uint32_t *pos,
                                        uint32_t lane = threadIdx.x) {
    uint32_t v[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        v[j] = PER * lane + j < nb ? cnt[PER * lane + j] : 0u;
        s += v[j];
    }
    uint32_t x = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if ((int)lane >= off) x += y;
    }
    uint32_t ex = x - s;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (PER * lane + j < nb) start[PER * lane + j] = pos[PER * lane + j] = ex;
        ex += v[j];
    }
}

// Phase timer for A/B diagnostics (template-gated: the production instantiation carries none of
// it): s_memtime deltas of the block's wave 0 summed per phase, added by thread 0 to dst[0..N).
template <bool ON, int N = 8> struct PhaseStamps {
    uint64_t t = 0, acc[N] = {};
    __device__ __forceinline__ void start() {
        if constexpr (ON) t = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void mark(int i) {
        if constexpr (ON) {
            const uint64_t n = __builtin_amdgcn_s_memtime();
            acc[i] += n - t;
            t = n;
        }
    }
    __device__ __forceinline__ void flush(unsigned long long *dst) {
        if constexpr (ON) {
            if (threadIdx.x == 0)
                for (int i = 0; i < N; ++i) atomicAdd(dst + i, (unsigned long long)acc[i]);
        }
    }
};

}  // namespace rbx
