// bench_kernels.hip -- roofline probes on gfx950: the memory patterns of the Bloom kernels with the
// hashing removed (random gathers, region- and segment-local gathers, streaming reads and writes, the
// slice probe).  Reached only through api_bench.cpp (include/rbx_bench.h).
#include "bloom_common.h"

namespace rbx {

// ---------------------------------------------------------------------------------
// Random-gather roofline probe: the contains kernel's memory pattern with the hashing
// removed.  Each lane issues k independent 4-byte loads at pseudo-random word offsets
// of a `nwords`-word table (same MLP structure as k_bloom_contains), XOR-reduced to a
// sink so nothing is dead-code eliminated.
// ---------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void k_gather_probe(const uint32_t *__restrict__ tbl, uint64_t nwords,
                                                      uint64_t nkeys, uint64_t seed, uint32_t *__restrict__ sink) {
    uint32_t acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nkeys; i += stride) {
        uint64_t z = (seed + i) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z ^= z >> 27;
        uint32_t w[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t r = (uint32_t)(z >> (j & 1 ? 32 : 0)) ^ (uint32_t)(j * 0x9E3779B9u);
            z += 0x632BE59BD9B4E019ULL;
            w[j] = tbl[(uint64_t)r * nwords >> 32];
        }
#pragma unroll
        for (int j = 0; j < K; ++j) acc ^= w[j];
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;  // practically never taken; keeps the loads live
}

void launch_gather_probe(const uint32_t *tbl, uint64_t nwords, uint64_t nkeys, uint32_t k, uint32_t *sink,
                         hipStream_t st) {
    const unsigned grid = grid_for(nkeys, kMaxGrid);
    switch (k) {
    case 10: hipLaunchKernelGGL(k_gather_probe<10>, dim3(grid), dim3(256), 0, st, tbl, nwords, nkeys, 0x5EEDull, sink); break;
    default: hipLaunchKernelGGL(k_gather_probe<7>, dim3(grid), dim3(256), 0, st, tbl, nwords, nkeys, 0x5EEDull, sink); break;
    }
}
// ---------------------------------------------------------------------------------
// Region-local gather probe: the table is cut into regions of `region_words`; workgroup b
// works on regions b%8, b%8+8, ... in order (blocks b and b+8 share an XCD under the
// observed round-robin placement -- speed only), each lane doing k random loads inside the
// current region.  Measures the L2-resident gather rate a region-bucketed probe can reach.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_regions(const uint32_t *__restrict__ tbl, uint64_t nregions,
                                                        uint64_t region_words, uint64_t per_region,
                                                        uint32_t *__restrict__ sink) {
    const uint32_t xcd = blockIdx.x & 7, local = blockIdx.x >> 3, nlocal = gridDim.x >> 3;
    uint32_t acc = 0;
    for (uint64_t r = xcd; r < nregions; r += 8) {
        const uint32_t *base = tbl + r * region_words;
        for (uint64_t i = (uint64_t)local * blockDim.x + threadIdx.x; i < per_region; i += (uint64_t)nlocal * blockDim.x) {
            uint64_t z = (r * 0x9E3779B97F4A7C15ULL) ^ (i * 0xBF58476D1CE4E5B9ULL);
            z ^= z >> 31;
            z *= 0x94D049BB133111EBULL;
            uint32_t w[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                w[j] = base[(uint64_t)(uint32_t)(z >> (j & 1 ? 32 : 0) ^ (j * 0x9E3779B9u)) * region_words >> 32];
                z += 0x632BE59BD9B4E019ULL;
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) acc ^= w[j];
        }
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;
}

// Segment-local gather probe (the locality of a multi-tenant batch, BASELINE C3): key i belongs
// to segment i / keys_per_seg, segments are consecutive slices of seg_words words (wrapping over
// the table), and every key does K random 4-byte loads inside its own segment.
template <int K>
__global__ __launch_bounds__(256) void k_gather_segments(const uint32_t *__restrict__ tbl, uint64_t nwords,
                                                         uint64_t seg_words, uint64_t keys_per_seg, uint64_t nkeys,
                                                         uint32_t *__restrict__ sink) {
    uint32_t acc = 0;
    const uint64_t nseg_tbl = nwords / seg_words;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nkeys; i += stride) {
        const uint32_t *base = tbl + ((i / keys_per_seg) % nseg_tbl) * seg_words;
        uint64_t z = (i + 0x5EEDull) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z ^= z >> 27;
        uint32_t w[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t r = (uint32_t)(z >> (j & 1 ? 32 : 0)) ^ (uint32_t)(j * 0x9E3779B9u);
            z += 0x632BE59BD9B4E019ULL;
            w[j] = base[(uint64_t)r * seg_words >> 32];
        }
#pragma unroll
        for (int j = 0; j < K; ++j) acc ^= w[j];
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;
}

void launch_gather_segments(const uint32_t *tbl, uint64_t nwords, uint64_t seg_words, uint64_t keys_per_seg,
                            uint64_t nkeys, uint32_t *sink, hipStream_t st) {
    const unsigned grid = grid_for(nkeys, kMaxGrid);
    hipLaunchKernelGGL(k_gather_segments<4>, dim3(grid), dim3(256), 0, st, tbl, nwords, seg_words, keys_per_seg,
                       nkeys, sink);
}

// Streaming-read roofline probe: 16-byte loads of a whole buffer, 4 in flight per lane.
__global__ __launch_bounds__(256) void k_stream_read(const u32x4 *__restrict__ src, uint64_t n16,
                                                     uint32_t *__restrict__ sink) {
    uint32_t acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(src + i + u * stride);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    for (; i < n16; i += stride) {
        const u32x4 v = src[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;
}

void launch_stream_read(const void *buf, uint64_t bytes, uint32_t *sink, hipStream_t st) {
    hipLaunchKernelGGL(k_stream_read, dim3(4096), dim3(256), 0, st, (const u32x4 *)buf, bytes / 16, sink);
}

// Streaming-write roofline probe: 16-byte nontemporal stores over a whole buffer (whole 64-byte
// write requests, the form the partition passes' runs take).
__global__ __launch_bounds__(256) void k_stream_write(u32x4 *__restrict__ dst, uint64_t n16, uint32_t seed) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const uint32_t x = (uint32_t)i ^ seed;
        __builtin_nontemporal_store(u32x4{x, x + 1u, x + 2u, x + 3u}, dst + i);
    }
}

void launch_stream_write(void *buf, uint64_t bytes, hipStream_t st) {
    hipLaunchKernelGGL(k_stream_write, dim3(4096), dim3(256), 0, st, (u32x4 *)buf, bytes / 16, 0x9E3779B9u);
}

// Slice-probe roofline: the bitmap is cut into nbuckets slices of 2^slice_log2 bytes; bucket b's
// entries (8 bytes: word offset in the slice, payload) are streamed and each tests one word of
// slice b.  Workgroup w takes the buckets w % 8, w % 8 + 8, ... (blocks b and b + 8 share an XCD
// under the observed round-robin placement: speed only), so one XCD's workgroups gather inside
// one slice at a time and the slice can stay in that XCD's L2.
__global__ __launch_bounds__(256) void k_bench_slice_probe(const u32x2 *__restrict__ ent, uint64_t per_bucket,
                                                           uint32_t nbuckets, const uint32_t *__restrict__ bm,
                                                           uint32_t slice_words_log2, uint32_t *__restrict__ sink) {
    const uint32_t x = blockIdx.x & 7, local = blockIdx.x >> 3, nlocal = gridDim.x >> 3;
    uint32_t acc = 0;
    for (uint32_t b = x; b < nbuckets; b += 8) {
        const u32x2 *e = ent + (uint64_t)b * per_bucket;
        const uint32_t *slice = bm + ((uint64_t)b << slice_words_log2);
        const uint64_t step = (uint64_t)nlocal * 256;
        uint64_t i = (uint64_t)local * 256 + threadIdx.x;
        for (; i + 3 * step < per_bucket; i += 4 * step) {
            u32x2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(e + i + u * step);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc ^= slice[v[u].x & ((1u << slice_words_log2) - 1)] ^ v[u].y;
        }
        for (; i < per_bucket; i += step) {
            const u32x2 v = e[i];
            acc ^= slice[v.x & ((1u << slice_words_log2) - 1)] ^ v.y;
        }
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;
}

void launch_bench_slice_probe(const void *ent, uint64_t per_bucket, uint32_t nbuckets, const uint32_t *bm,
                              uint32_t slice_words_log2, unsigned grid, uint32_t *sink, hipStream_t st) {
    hipLaunchKernelGGL(k_bench_slice_probe, dim3(grid), dim3(256), 0, st, (const u32x2 *)ent, per_bucket, nbuckets, bm,
                       slice_words_log2, sink);
}

void launch_gather_regions(const uint32_t *tbl, uint64_t nwords, uint64_t region_words, uint64_t total_lanes,
                           uint32_t *sink, hipStream_t st, unsigned grid) {
    const uint64_t nregions = nwords / region_words;
    hipLaunchKernelGGL(k_gather_regions, dim3(grid), dim3(256), 0, st, tbl, nregions, region_words,
                       total_lanes / nregions, sink);
}

}  // namespace rbx
