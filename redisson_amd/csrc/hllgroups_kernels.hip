// hllgroups_kernels.hip -- many PFCOUNT unions and many PFMERGEs in one launch (rbx_hll_count_groups,
// rbx_hll_merge_groups): what RHyperLogLog.countWith / mergeWith (M/RedissonHyperLogLog.java:89-102) send one
// command each, and what a batch queues through RBatch.getHyperLogLog(name) (M/RedissonBatch.java:57-64).
// DESIGN section 11.8 has the rules; the phases of a merge call and the cache rule of a one-key count are
// api_hll.cpp's.
//
// A group is a list of register blocks (16384 bytes each, one byte per register), given as a CSR table in device
// memory: members[off[g] .. off[g + 1]).  Its union is the bytewise maximum.  The registers of a group are split
// over P workgroups (P a power of two, 1 .. 16): workgroup b owns the slice b % P of group b / P, 16384 / P
// registers, in 16-byte vectors: a lane takes one vector at a time and walks the group's members for it eight at a
// time, so that eight independent 16-byte loads are in flight before the first maximum is taken (P <= 4: 256 lanes,
// 4 / P vectors each, one after the other; P = 8, 16: 128 and 64 lanes, one vector each).
//   k_hg_union_count  counts the slice into a per-wave LDS histogram (as k_hll_count).  P = 1: the workgroup holds
//                     the whole histogram and finishes with the estimator.  P > 1: it adds its 64 bins into the
//                     group's zeroed global histogram, and k_hg_finish runs the estimator, one lane per group,
//                     in the next launch: stream order is the only ordering, no tickets and no fences.
//   k_hg_merge        the same walk, started from the destination's slice and stored back to it.  Inside one
//                     launch no destination is another group's member (the host's phases see to it), a
//                     destination among its own members is read and written by the same lane: plain loads and
//                     stores.
// M/ = redisson/src/main/java/org/redisson/ of the reference
#include <hip/hip_runtime.h>

#include "hll_device.h"
#include "rbx_kernels.h"

namespace rbx {

typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));

constexpr int kHgVectors = 16384 / 16;  // 16-byte vectors of one register block
constexpr int kHgUnroll = 8;             // members whose loads are in flight together, per lane

// the maximum of vector `vec` over the members [m0, m1), folded into acc
__device__ __forceinline__ void hg_walk(const uint8_t *const *__restrict__ members, uint32_t m0, uint32_t m1,
                                        uint32_t vec, u8x16 &acc) {
    uint32_t m = m0;
    for (; m + kHgUnroll <= m1; m += kHgUnroll) {
        u8x16 x[kHgUnroll];
#pragma unroll
        for (int u = 0; u < kHgUnroll; ++u) x[u] = ((const u8x16 *)members[m + u])[vec];
#pragma unroll
        for (int u = 0; u < kHgUnroll; ++u) acc = __builtin_elementwise_max(acc, x[u]);
    }
    for (; m < m1; ++m) acc = __builtin_elementwise_max(acc, ((const u8x16 *)members[m])[vec]);
}

// blockDim.x = min(256, kHgVectors >> lg_split): a lane takes the slice's vectors threadIdx.x, + blockDim.x, ..
__global__ __launch_bounds__(256) void k_hg_union_count(const uint8_t *const *__restrict__ members,
                                                        const uint32_t *__restrict__ off, int lg_split,
                                                        int *__restrict__ histo, unsigned long long *__restrict__ out) {
    __shared__ int h[4][64];
    const uint32_t g = blockIdx.x >> lg_split, slice = blockIdx.x & ((1u << lg_split) - 1u);
    const uint32_t per = (uint32_t)kHgVectors >> lg_split, m0 = off[g], m1 = off[g + 1];
    const int wid = threadIdx.x >> 6;
    (&h[0][0])[threadIdx.x] = 0;  // (a workgroup of fewer than 256 lanes uses fewer rows)
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < per; v += blockDim.x) {
        u8x16 acc = (u8x16)(0);
        hg_walk(members, m0, m1, slice * per + v, acc);
#pragma unroll
        for (int b = 0; b < 16; ++b) atomicAdd(&h[wid][acc[b] & 63u], 1);
    }
    __syncthreads();
    const int waves = blockDim.x >> 6;
    if (threadIdx.x < 64) {
        const int t = threadIdx.x;
        int s = 0;
        for (int w = 0; w < waves; ++w) s += h[w][t];
        if (lg_split == 0) {
            h[0][t] = s;
            histo[(size_t)g * 64 + t] = s;
        } else if (s) {
            atomicAdd(&histo[(size_t)g * 64 + t], s);
        }
    }
    if (lg_split != 0) return;
    __syncthreads();
    if (threadIdx.x == 0) out[g] = hll_estimate(h[0]);  // ~0: the hllTau path, the host evaluates it
}

__global__ __launch_bounds__(256) void k_hg_finish(const int *__restrict__ histo, uint32_t ngroups,
                                                   unsigned long long *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    out[g] = hll_estimate(histo + (size_t)g * 64);  // (read in place: a private copy would live in scratch)
}

__global__ __launch_bounds__(256) void k_hg_merge(uint8_t *const *__restrict__ dst,
                                                  const uint8_t *const *__restrict__ members,
                                                  const uint32_t *__restrict__ off, int lg_split) {
    const uint32_t g = blockIdx.x >> lg_split, slice = blockIdx.x & ((1u << lg_split) - 1u);
    const uint32_t per = (uint32_t)kHgVectors >> lg_split, m0 = off[g], m1 = off[g + 1];
    u8x16 *d = (u8x16 *)dst[g];
    for (uint32_t v = threadIdx.x; v < per; v += blockDim.x) {
        u8x16 acc = d[slice * per + v];
        hg_walk(members, m0, m1, slice * per + v, acc);
        d[slice * per + v] = acc;
    }
}

static int hg_lg(int split) {
    int lg = 0;
    while ((1 << lg) < split) ++lg;
    return lg;
}

static int hg_lanes(int lg) { return (kHgVectors >> lg) < 256 ? (kHgVectors >> lg) : 256; }

int launch_hllgroups_union_count(const uint8_t *const *d_members, const uint32_t *d_off, uint32_t ngroups, int split,
                                 int *d_histo, unsigned long long *d_out, hipStream_t st) {
    if (!ngroups) return 0;
    const int lg = hg_lg(split);
    if (lg) {
        hipError_t e = hipMemsetAsync(d_histo, 0, (size_t)ngroups * 64 * sizeof(int), st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_hg_union_count, dim3(ngroups << lg), dim3(hg_lanes(lg)), 0, st, d_members, d_off, lg, d_histo,
                       d_out);
    if (lg) hipLaunchKernelGGL(k_hg_finish, dim3((ngroups + 255) / 256), dim3(256), 0, st, d_histo, ngroups, d_out);
    return 0;
}

void launch_hllgroups_merge(uint8_t *const *d_dst, const uint8_t *const *d_members, const uint32_t *d_off,
                            uint32_t ngroups, int split, hipStream_t st) {
    if (!ngroups) return;
    const int lg = hg_lg(split);
    hipLaunchKernelGGL(k_hg_merge, dim3(ngroups << lg), dim3(hg_lanes(lg)), 0, st, d_dst, d_members, d_off, lg);
}

}  // namespace rbx
