// bitgroups_kernels.hip -- many BITOPs and many BITCOUNTs of a combination in one launch (rbx_bitset_op_groups):
// what RBitSet.and / or / xor / not and cardinality (M/RedissonBitSet.java:362-388, :462-464, :482-484) send one
// command each, and what a batch queues through RBatch.getBitSet(name) (M/RedissonBatch.java:182-184).  DESIGN
// section 11.9 has the rules; the phases of a call, the forwarded counts and every length are api_bitset_multi.cpp's.
//
// Groups span six orders of magnitude -- ten thousand strings of 128 bytes, or one of 512 MiB -- so a launch is a
// segmented sweep.  The host, which knows every length, cuts each group's span into tiles of T bytes (a power of
// two, 4 KiB .. 1 MiB) and numbers them through the launch: group g owns the tiles first[g] .. first[g + 1).  The
// grid is the tile total capped at kMaxGrid (and at the workgroups the device holds at once, when those are
// fewer); a workgroup strides over tile numbers, finds its tile's group by binary search over first[] (the tile
// number depends on blockIdx only, so the search is the same in every lane), keeps that group while its next tiles
// lie in it, and sweeps the tile as k_bitop sweeps a whole string: lane l owns the 16 bytes at one offset, reads them from
// every source and only then stores them, so the destination may be any of the sources and no pointer is
// __restrict__; a source's last partial vector is assembled bytewise and nothing at or past its length is touched;
// the result's last vector is masked; the span past out_len (what a longer previous destination held) is cleared.
// Below `full` -- the length every source of the group reaches, in whole vectors -- the sources are walked
// kBgDepth at a time with plain 16-byte loads, all of them issued before the first combine.
// A group with a count adds the popcount of its masked result: reduced over the workgroup, then one u64 atomicAdd
// per tile -- per run of tiles that a workgroup takes from one group -- onto the group's word, which the host
// zeroed in the same stream (integer adds: the order is immaterial).  A group without a destination stores
// nothing.  One lane of a group's first tile writes the destination's length word.  Inside one launch no
// destination is another group's source or destination (the host's phases see to it).
// M/ = redisson/src/main/java/org/redisson/ of the reference
#include <hip/hip_runtime.h>

#include "../../include/rbx.h"
#include "bitop_device.h"
#include "rbx_kernels.h"

namespace rbx {

constexpr int kBgDepth = 8;  // sources whose loads are in flight together, per lane

template <int OP> __device__ __forceinline__ uint4 bg_combine(const uint4 r, const uint4 v) {
    if (OP == RBX_BITOP_AND) return make_uint4(r.x & v.x, r.y & v.y, r.z & v.z, r.w & v.w);
    if (OP == RBX_BITOP_OR) return make_uint4(r.x | v.x, r.y | v.y, r.z | v.z, r.w | v.w);
    return make_uint4(r.x ^ v.x, r.y ^ v.y, r.z ^ v.z, r.w ^ v.w);
}

// the vector at offset o of the combination, o + 16 <= every source's length: whole-vector loads only
template <int OP> __device__ __forceinline__ uint4 bg_vector_full(const BitopSrc *s, uint32_t n, uint64_t o) {
    uint4 r = ld_nt16(s[0].bytes + o);
    if (OP == RBX_BITOP_NOT) return make_uint4(~r.x, ~r.y, ~r.z, ~r.w);
    uint32_t i = 1;
    for (; i + kBgDepth <= n; i += kBgDepth) {
        uint4 x[kBgDepth];
#pragma unroll
        for (int u = 0; u < kBgDepth; ++u) x[u] = ld_nt16(s[i + u].bytes + o);
#pragma unroll
        for (int u = 0; u < kBgDepth; ++u) r = bg_combine<OP>(r, x[u]);
    }
    for (; i < n; ++i) r = bg_combine<OP>(r, ld_nt16(s[i].bytes + o));
    return r;
}

// the same where some source ends inside or before the vector (bitop_load reads nothing at or past a length)
template <int OP> __device__ __forceinline__ uint4 bg_vector_edge(const BitopSrc *s, uint32_t n, uint64_t o) {
    uint4 r = bitop_load(s[0], o);
    if (OP == RBX_BITOP_NOT) return make_uint4(~r.x, ~r.y, ~r.z, ~r.w);
    for (uint32_t i = 1; i < n; ++i) r = bg_combine<OP>(r, bitop_load(s[i], o));
    return r;
}

// the bytes [base, end) of group G's span; returns this lane's share of the result's one bits when counted
template <int OP>
__device__ __forceinline__ uint32_t bg_tile(const BitGroup &G, const BitopSrc *s, uint64_t base, uint64_t end) {
    uint32_t ones = 0;
    for (uint64_t o = base + (uint64_t)threadIdx.x * 16; o < end; o += 256 * 16) {
        uint4 r = make_uint4(0, 0, 0, 0);
        if (o < G.out_len) {
            r = o + 16 <= G.full ? bg_vector_full<OP>(s, G.nsrc, o) : bg_vector_edge<OP>(s, G.nsrc, o);
            if (o + 16 > G.out_len) {  // the result's last vector: zero past out_len
                const int64_t n = (int64_t)(G.out_len - o);
                r.x &= low_bytes(n);
                r.y &= low_bytes(n - 4);
                r.z &= low_bytes(n - 8);
                r.w &= low_bytes(n - 12);
            }
        }
        if (G.dst) *(uint4 *)(G.dst + o) = r;
        if (G.count) ones += __popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w);
    }
    return ones;
}

// adds the workgroup's ones onto *count: reduced over the workgroup, one atomicAdd by one lane.  Every lane of the
// workgroup calls it (it holds barriers).
__device__ __forceinline__ void bg_flush(unsigned long long *count, uint32_t ones, uint32_t *s_part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ones += __shfl_down(ones, off, 64);
    __syncthreads();  // the previous flush's sum has been read
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ones;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (unsigned long long)s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (sum) atomicAdd(count, sum);
    }
}

__global__ __launch_bounds__(256) void k_bg_sweep(const BitGroup *groups, const uint64_t *first, uint32_t ngroups,
                                                  const BitopSrc *srcs, uint32_t tile_bytes) {
    __shared__ uint32_t s_part[4];
    const uint64_t tiles = first[ngroups];
    // the group of the workgroup's current tile and its tiles [g_first, g_next): a group of more tiles than the
    // grid has workgroups keeps a workgroup for several tiles in a row, which then neither searches nor loads the
    // record again, and adds its count once for all of them
    BitGroup G{};
    uint64_t g_first = 0, g_next = 0;
    uint32_t ones = 0;  // this lane's share of G's count so far (a workgroup sweeps far less than 2^32 bits per lane)
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // (t is the same in every lane of the workgroup)
        if (t >= g_next) {
            if (G.count) bg_flush(G.count, ones, s_part);
            ones = 0;
            uint32_t lo = 0, hi = ngroups;  // first[lo] <= t < first[hi]
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (first[mid] <= t) lo = mid;
                else hi = mid;
            }
            G = groups[lo];
            g_first = first[lo];
            g_next = first[lo + 1];
        }
        const BitopSrc *s = srcs + G.src_off;
        const uint64_t base = (t - g_first) * tile_bytes;
        const uint64_t end = base + tile_bytes < G.span ? base + tile_bytes : G.span;
        switch (G.op) {
        case RBX_BITOP_AND: ones += bg_tile<RBX_BITOP_AND>(G, s, base, end); break;
        case RBX_BITOP_OR: ones += bg_tile<RBX_BITOP_OR>(G, s, base, end); break;
        case RBX_BITOP_XOR: ones += bg_tile<RBX_BITOP_XOR>(G, s, base, end); break;
        default: ones += bg_tile<RBX_BITOP_NOT>(G, s, base, end); break;
        }
        if (t == g_first && threadIdx.x == 0 && G.dst_len) *G.dst_len = G.out_len;
    }
    if (G.count) bg_flush(G.count, ones, s_part);
}

// out[i] = *ptrs[i]: the length words of a call's keys, one lane each
__global__ __launch_bounds__(256) void k_bg_lens(const unsigned long long *const *__restrict__ ptrs, uint32_t n,
                                                 unsigned long long *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = *ptrs[i];
}

void launch_bitgroups_lens(const unsigned long long *const *d_ptrs, uint32_t n, unsigned long long *d_out,
                           hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(k_bg_lens, dim3((n + 255) / 256), dim3(256), 0, st, d_ptrs, n, d_out);
}

void launch_bitgroups_sweep(const BitGroup *d_groups, const uint64_t *d_first, uint32_t ngroups, uint64_t tiles,
                            const BitopSrc *d_srcs, uint32_t tile_bytes, hipStream_t st) {
    if (!ngroups || !tiles) return;
    // kMaxGrid, or fewer: no more workgroups than the device holds at once.  A workgroup that starts only when
    // another has finished would sweep its share of a large group alone, behind all the others.
    static const unsigned cap = [] {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bg_sweep, 256, 0) != hipSuccess || per_cu < 1 ||
            hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            return kMaxGrid;
        const unsigned resident = (unsigned)per_cu * (unsigned)cus;
        return resident < kMaxGrid ? resident : kMaxGrid;
    }();
    const unsigned grid = (unsigned)(tiles < cap ? tiles : cap);
    hipLaunchKernelGGL(k_bg_sweep, dim3(grid), dim3(256), 0, st, d_groups, d_first, ngroups, d_srcs, tile_bytes);
}

}  // namespace rbx
