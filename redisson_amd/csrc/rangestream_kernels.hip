// rangestream_kernels.hip -- BITCOUNT / BITPOS / STRLEN / RBitSet.length() over many strings in one call
// (rbx_bitset_range_stream).  Command i is (key[i], cmds[i]); range_cmd.h has its rules, the
// strings are reached through the BitKey table of the bit streams (rbx_kernels.h), and bitrange_device.h has the
// masked 16-byte vector.  The kernels only read the strings: an interval [lo, hi] is normalised (lo <= hi < 8 *
// length), its vectors lo>>7 .. hi>>7 lie inside the allocation (a multiple of 256 bytes), and what the last
// one holds past the length is zero.
//
//  1. k_rs_short<G>: a group of G lanes per command answers everything whose interval covers at most short_max
//     bytes, and lists the others with their tile numbers.
//  2. k_rs_tiles: the listed commands' tiles, flattened, swept by the whole grid.
//  3. k_rs_finish: one lane per listed POS command turns the published minimum into the reply.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitrange_device.h"
#include "bloom_common.h"
#include "rbx_kernels.h"

namespace rbx {

// (rs_len, the string of a table entry, and the two tiers' list, tiles and summary idioms: bitrange_device.h)
constexpr int kRsFlags = rs_flags_at(kRangeKinds), kRsLong = rs_long_at(kRangeKinds);

// ---------------------------------------------------------------------------------
// 1. One group of G lanes per command; the grid strides over the commands, and the trip count is the same in
// every lane of the grid, so the group reduction at the end of an iteration runs in uniform control flow.
// A lane's accumulator is a count for COUNT and the lowest position it found for POS; the groups of one wave
// may hold different commands, so the reduction picks per lane between sum and minimum.
// ---------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void k_rs_short(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                  const rbx_range_cmd *__restrict__ cmds, uint32_t n, uint32_t nkeys,
                                                  uint32_t short_max, uint32_t tile_lg, int64_t *__restrict__ replies,
                                                  uint8_t *__restrict__ status, unsigned long long *sum,
                                                  unsigned long long *__restrict__ longs) {
    constexpr uint32_t kGroups = 256 / G;  // per workgroup
    const uint32_t gl = threadIdx.x & (G - 1);
    const uint32_t ngroups = gridDim.x * kGroups;
    const uint32_t g0 = blockIdx.x * kGroups + threadIdx.x / G;
    // the lanes of this group inside the wave's ballot
    const unsigned long long gmask = (G == 64 ? ~0ULL : ((1ULL << (G & 63)) - 1)) << ((threadIdx.x & 63) & ~(G - 1));
    for (uint32_t base = 0; base < n; base += ngroups) {
        const uint64_t i = (uint64_t)base + g0;
        enum { kNone, kStore, kCount, kPos } what = kNone;
        uint64_t lo = 0, hi = 0;
        int64_t reply = 0;
        uint8_t st = 0;
        bool flip = false;
        rbx_range_cmd c = {};
        const uint4 *vecs = nullptr;
        if (i < n) {
            c = cmds[i];
            const uint32_t k = key[i];
            if (k >= nkeys || range_cmd_illegal(c)) {
                if (gl == 0) atomicOr(sum + kRsFlags, (unsigned long long)kRsIllegal);
            } else {
                const BitKey bk = tab[k];
                what = kStore;
                int f = range_cmd_fails(c);
                if (!f && (bk.flags & kBitKeyWrong)) f = kRangeWrongType;
                bool missing = true;
                uint64_t len = 0;
                if (!f) len = rs_len(bk, &missing);
                if (!f && c.op == RBX_RANGE_LENGTH) {
                    const uint8_t *s = (const uint8_t *)bk.words;
                    if (!bitset_length_rule(len, len ? s[0] : 0, len ? s[len - 1] : 0, &reply)) f = kRangeScript;
                } else if (!f && range_cmd_plan(c, len, missing, &lo, &hi, &reply)) {
                    vecs = (const uint4 *)bk.words;
                    flip = c.op == RBX_RANGE_POS && c.bit == 0;
                    if ((hi >> 3) - (lo >> 3) + 1 > short_max) {
                        // preset the reply the tiles add to or take the minimum of, and list the command
                        reply = c.op == RBX_RANGE_COUNT ? 0 : (int64_t)kBitsNone;
                        if (gl == 0) rs_list_claim(sum + kRsLong, longs, i, lo, hi, tile_lg);
                    } else {
                        what = c.op == RBX_RANGE_COUNT ? kCount : kPos;
                    }
                }
                if (f) {
                    reply = 0;
                    st = kRsFailedStatus;
                    if (gl == 0) rs_first_min(sum + (f - 1), i);
                }
            }
        }
        uint64_t acc = what == kPos ? kBitsNone : 0;
        const uint64_t v1 = hi >> 7;
        if (what == kCount) {
            for (uint64_t v = (lo >> 7) + gl; v <= v1; v += G) acc += popc4(vec_wanted<false>(vecs[v], v, lo, hi));
        } else if (what == kPos) {
            // front to back, G vectors per step; the step with a hit ends the group's walk (the bound and the
            // ballot's group bits are the same in every lane of the group)
            for (uint64_t vb = lo >> 7; vb <= v1; vb += G) {
                const uint64_t v = vb + gl;
                uint32_t f = 128u;
                if (v <= v1) {
                    const uint4 x = vecs[v];
                    f = vec_first(flip ? vec_wanted<true>(x, v, lo, hi) : vec_wanted<false>(x, v, lo, hi));
                }
                if (f < 128u) acc = (v << 7) + f;
                if (__ballot(f < 128u) & gmask) break;
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const uint64_t y = __shfl_xor((unsigned long long)acc, off, G);
            acc = what == kPos ? min(acc, y) : acc + y;
        }
        if (what == kCount) reply = (int64_t)acc;
        if (what == kPos) reply = range_cmd_pos_reply(c, acc, hi);
        if (what != kNone && gl == 0) {
            if (replies) replies[i] = reply;
            if (status) status[i] = st;
        }
    }
}

// ---------------------------------------------------------------------------------
// 2. The tiles of the listed commands, numbered across the list.  Workgroup w takes tiles w, w + grid, ...; it
// finds its command (rs_tile_of), works the command's interval out again from the command and the table, and
// sweeps the tile's vectors.  COUNT: a block reduction and one atomicAdd into the reply per tile.
// POS: the tile is skipped when a hit at or before its first bit is published, else scanned front to back,
// 256 vectors per step, and the first step with a hit publishes atomicMin(reply, position) and ends the tile's
// scan.  Exact by k_bits_pos's argument (bitrange_kernels.hip): a tile is scanned to its end or left only behind
// a published hit at or before its start, so every tile below the final minimum was scanned without a hit.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rs_tiles(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                  const rbx_range_cmd *__restrict__ cmds, uint32_t tile_lg,
                                                  const unsigned long long *__restrict__ longs, uint32_t nlong,
                                                  uint64_t ntiles, int64_t *replies) {
    __shared__ unsigned long long s_part[4];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile_vecs = 1ULL << (tile_lg - 4);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RsTile rt = rs_tile_of(longs, nlong, t);
        const uint64_t i = rt.i;
        const rbx_range_cmd c = cmds[i];
        const BitKey bk = tab[key[i]];
        bool missing;
        const uint64_t len = rs_len(bk, &missing);
        uint64_t lo, hi;
        int64_t fixed;
        if (!range_cmd_plan(c, len, missing, &lo, &hi, &fixed)) continue;  // (listed commands have an interval)
        const uint4 *vecs = (const uint4 *)bk.words;
        // cb <= v1: the tile is one of the command's (the list's invariant, bitrange_device.h)
        const uint64_t v1 = hi >> 7, cb = (lo >> 7) + rt.own * tile_vecs, ce = min(cb + tile_vecs - 1, v1);
        auto *result = (unsigned long long *)(replies + i);
        if (c.op == RBX_RANGE_COUNT) {
            uint64_t n1 = 0;
            for (uint64_t v = cb + threadIdx.x; v <= ce; v += 256) {
                uint4 x = ld_nt16(vecs + v);
                if (v == (lo >> 7) || v == v1) x = vec_wanted<false>(x, v, lo, hi);
                n1 += popc4(x);
            }
            block_sum4(n1, s_part, [&](unsigned long long sum) {
                if (sum) atomicAdd(result, sum);
            });
        } else {
            const bool flip = c.bit == 0;
            // (read past L1 for the early exit only; the answer rests on the atomicMin alone)
            if (__syncthreads_or(threadIdx.x == 0 &&
                                 __hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (cb << 7)))
                continue;
            bool leave = false;
            for (uint64_t s = cb; s <= ce && !leave; s += 256) {
                bool done = false;
                const uint64_t v = s + threadIdx.x;
                unsigned long long best = kBitsNone;
                if (v <= ce) {
                    const uint4 x = ld_nt16(vecs + v);
                    const uint32_t f = vec_first(flip ? vec_wanted<true>(x, v, lo, hi) : vec_wanted<false>(x, v, lo, hi));
                    if (f < 128u) best = (v << 7) + f;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) best = min(best, (unsigned long long)__shfl_down(best, off, 64));
                if (lane == 0 && best < kBitsNone) {
                    atomicMin(result, best);
                    done = true;
                }
                leave = __syncthreads_or(done);
            }
        }
    }
}

// 3. One lane per listed command: a POS command's published minimum becomes its reply.
__global__ __launch_bounds__(256) void k_rs_finish(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                   const rbx_range_cmd *__restrict__ cmds,
                                                   const unsigned long long *__restrict__ longs, uint32_t nlong,
                                                   int64_t *replies) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nlong; j += stride) {
        const uint64_t i = rs_entry_pos(longs[j]);
        const rbx_range_cmd c = cmds[i];
        if (c.op != RBX_RANGE_POS) continue;
        bool missing;
        const uint64_t len = rs_len(tab[key[i]], &missing);
        uint64_t lo, hi;
        int64_t fixed;
        if (!range_cmd_plan(c, len, missing, &lo, &hi, &fixed)) continue;
        replies[i] = range_cmd_pos_reply(c, (uint64_t)replies[i], hi);
    }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_rangestream_short(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_range_cmd *d_cmds,
                              uint32_t n, uint32_t nkeys, uint32_t short_max, uint32_t tile_bytes, int64_t *d_replies,
                              uint8_t *d_status, unsigned long long *d_sum, unsigned long long *d_long, hipStream_t st) {
    const uint32_t lg = log2_of(tile_bytes);
#define RS_SHORT(G)                                                                                                        \
    hipLaunchKernelGGL(k_rs_short<G>, dim3(grid_for((uint64_t)n * G, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, n, nkeys, short_max, lg, \
                       d_replies, d_status, d_sum, d_long)
    RBX_FOR_LANES(lanes, RS_SHORT);
#undef RS_SHORT
}

void launch_rangestream_tiles(const BitKey *d_tab, const uint32_t *d_key, const rbx_range_cmd *d_cmds,
                              uint32_t tile_bytes, const unsigned long long *d_long, uint32_t nlong, uint64_t ntiles,
                              int64_t *d_replies, hipStream_t st) {
    hipLaunchKernelGGL(k_rs_tiles, dim3((unsigned)std::min<uint64_t>(ntiles, kMaxGrid)), dim3(256), 0, st, d_tab, d_key,
                       d_cmds, log2_of(tile_bytes), d_long, nlong, ntiles, d_replies);
    hipLaunchKernelGGL(k_rs_finish, dim3(grid_for(nlong, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, d_long, nlong,
                       d_replies);
}

}  // namespace rbx
