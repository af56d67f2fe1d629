// bitrange_kernels.hip -- ranged BITCOUNT and BITPOS over the engine's bitmap strings (Spring Data's
// RedissonConnection.bitCount / bitPos; [redis-7.2] bitops.c bitcountCommand / bitposCommand, restated in
// DESIGN §11.2).  Every kernel works on a bit interval [lo, hi] that the reply rules of rbx_kernels.h have
// already normalised (lo <= hi < 8 * length), reads the aligned 16-byte vectors lo>>7 .. hi>>7 -- the last
// one may reach into the zero padding behind the length, never past the allocation, whose size is a
// multiple of 256 bytes -- masks the first and the last of them, and stores nothing to the bitmap.
//
// The vector masks and the per-wave walkers are bitrange_device.h's, shared with rangestream_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitrange_device.h"
#include "bloom_common.h"
#include "rbx_kernels.h"

namespace rbx {

// (kBlockBits / kBlockLog2, the directory's 4 KiB block: bitrange_device.h)

// ---------------------------------------------------------------------------------
// 1. BITCOUNT over one interval, the whole GPU: k_bitcount's grid-stride sweep over the vectors of the
// interval; the lanes holding the first and the last vector (the same lane for a short interval) mask theirs.
// *out += the count (the caller zeroes it).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bits_count_range(const uint4 *__restrict__ vecs, uint64_t lo, uint64_t hi,
                                                          unsigned long long *__restrict__ out) {
    const uint64_t v0 = lo >> 7, v1 = hi >> 7;
    uint64_t c = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = v0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= v1; v += stride) {
        uint4 x = ld_nt16(vecs + v);
        if (v == v0 || v == v1) x = vec_wanted<false>(x, v, lo, hi);
        c += popc4(x);
    }
    block_add_u64(c, out);
}

// ---------------------------------------------------------------------------------
// 2. BITPOS over one interval, with an early exit.  The vectors of the interval are cut into chunks of
// 2^lg vectors.  Workgroup w starts on chunk w; further chunks are claimed in ascending order with one
// returning atomicAdd on the ticket word: claim k (k = 0, 1, ...) is chunk gridDim.x + k, and no workgroup
// claims when the grid covers every chunk.  A chunk is scanned front to back, kPosLoads x 256 vectors per step;
// the first step with a hit publishes atomicMin(result, position) and ends the workgroup's scan.  Before each
// step a workgroup reads the result word and leaves once its chunk starts at or after it.
// Exact: every chunk below a claimed one belongs to some workgroup, and a chunk is scanned to its end or left
// only behind a published hit that lies at or before its start, so every chunk below the final minimum was
// scanned without a hit.  (The result is read past L1 for the early exit only; the answer rests on the
// atomicMin alone.)
//
// The state is three words on three 128-byte lines -- the minimum, the ticket, the count of workgroups that
// are done -- which the caller sets to all ones with one memset: the minimum then lies above kBitsNone, and
// the two counters wrap to 0 with their first increment.  The last workgroup to finish turns the minimum into
// the reply: *out = the position found, or none_reply.
// ---------------------------------------------------------------------------------
// vectors in flight per lane: 32 KiB per workgroup and step
constexpr int kPosLoads = 8;

template <bool FLIP>
__global__ __launch_bounds__(256) void k_bits_pos(const uint4 *__restrict__ vecs, uint64_t lo, uint64_t hi, uint32_t lg,
                                                  unsigned long long *state, int64_t none_reply, int64_t *out) {
    __shared__ uint32_t s_chunk;
    unsigned long long *result = state;
    uint32_t *ticket = (uint32_t *)(state + kBitsPosTicketAt), *finished = (uint32_t *)(state + kBitsPosDoneAt);
    const uint64_t v0 = lo >> 7, v1 = hi >> 7;
    const uint64_t nchunk = ((v1 - v0) >> lg) + 1;
    bool leave = false;
    for (uint64_t c = blockIdx.x; c < nchunk;) {
        const uint64_t cb = v0 + (c << lg), ce = min(cb + ((1ULL << lg) - 1), v1);
        for (uint64_t s = cb; s <= ce && !leave; s += 256 * kPosLoads) {
            // a hit at or before this chunk's first position: nothing here or later can be the answer
            bool done = threadIdx.x == 0 &&
                        __hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (cb << 7);
            uint4 x[kPosLoads];
#pragma unroll
            for (int u = 0; u < kPosLoads; ++u) {
                const uint64_t v = s + u * 256 + threadIdx.x;
                x[u] = v <= ce ? ld_nt16(vecs + v) : make_uint4(0, 0, 0, 0);
            }
            unsigned long long best = kBitsNone;
#pragma unroll
            for (int u = kPosLoads - 1; u >= 0; --u) {  // descending: the lowest vector's hit stays
                const uint64_t v = s + u * 256 + threadIdx.x;
                if (v <= ce) {
                    const uint32_t f = vec_first(vec_wanted<FLIP>(x[u], v, lo, hi));
                    if (f < 128u) best = (v << 7) + f;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) best = min(best, (unsigned long long)__shfl_down(best, off, 64));
            if ((threadIdx.x & 63) == 0 && best < kBitsNone) {
                atomicMin(result, best);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // performed before this workgroup counts itself done
                done = true;
            }
            leave = __syncthreads_or(done);
        }
        if (leave || nchunk <= gridDim.x) break;  // the second: every chunk had its workgroup from the start
        if (threadIdx.x == 0) s_chunk = gridDim.x + (atomicAdd(ticket, 1u) + 1u);
        __syncthreads();
        c = s_chunk;
        __syncthreads();
    }
    // Every path ends here, behind a barrier that follows this workgroup's last atomicMin, which its lane
    // has waited for.  The atomics are relaxed and of device scope: they are performed where every workgroup
    // sees them, and a fence, which on this part writes the L2 back, is not needed to order them.
    if (threadIdx.x == 0) {
        if (atomicAdd(finished, 1u) == gridDim.x - 2u) {  // all ones, 0, 1, ...: this is the last workgroup
            const unsigned long long r = __hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *out = r < kBitsNone ? (int64_t)r : none_reply;
        }
    }
}

// ---------------------------------------------------------------------------------
// 3. The block directory of a batch: dir[b] = the ones of the string's 4 KiB block b (k_bits_block_ones, one
// wave per block; the last block ends with the vector that holds the string's last byte, and what that
// vector holds past the length is zero), then the exclusive prefix sums P[b] in place and P[nblocks] = the
// string's ones (k_bits_block_scan, one workgroup, 8192 entries per pass).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bits_block_ones(const uint4 *__restrict__ vecs, uint64_t nvec, uint32_t nblocks,
                                                         unsigned long long *__restrict__ dir) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwave = gridDim.x * 4;
    for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < nblocks; b += nwave) {
        uint32_t c = 0;
        uint4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t v = (uint64_t)b * 256 + u * 64 + lane;
            x[u] = v < nvec ? ld_nt16(vecs + v) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) c += popc4(x[u]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0) dir[b] = c;
    }
}

__global__ __launch_bounds__(1024) void k_bits_block_scan(unsigned long long *dir, uint32_t nblocks) {
    __shared__ unsigned long long s_wave[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;  // the ones below this pass, the same in every thread
    for (uint32_t base = 0; base < nblocks; base += 8192) {
        const uint32_t i0 = base + threadIdx.x * 8;
        unsigned long long x[8], t = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = i0 + j < nblocks ? dir[i0 + j] : 0;
            t += x[j];
        }
        unsigned long long incl = t;  // inclusive scan of the wave's thread sums
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long y = __shfl_up(incl, off, 64);
            if (lane >= (uint32_t)off) incl += y;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long below = 0, total = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wave) below += s_wave[w];
            total += s_wave[w];
        }
        unsigned long long p = carry + below + incl - t;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (i0 + j < nblocks) dir[i0 + j] = p;
            p += x[j];
        }
        carry += total;
        __syncthreads();  // s_wave is rewritten by the next pass
    }
    if (threadIdx.x == 0) dir[nblocks] = carry;
}

// ---------------------------------------------------------------------------------
// 4. Batches: one wave per query.  The query prologue applies the command's reply rules (rbx_kernels.h)
// from the string's length, so out[i] is final.  DIR = false walks the interval 64 vectors (1 KiB) per step;
// DIR = true reads the whole blocks inside it from the directory P.
// ---------------------------------------------------------------------------------
template <bool DIR>
__global__ __launch_bounds__(256) void k_bits_count_ranges(const uint4 *__restrict__ vecs, uint64_t len,
                                                           const int64_t *__restrict__ starts,
                                                           const int64_t *__restrict__ ends, uint64_t n, int unit,
                                                           const unsigned long long *__restrict__ P,
                                                           unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwave = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nwave) {
        uint64_t lo, hi, c = 0;
        if (bits_count_interval(starts[i], ends[i], unit, len, &lo, &hi)) {
            // whole blocks [fb, lb) from the directory, what lies before and behind them from the string
            const uint64_t fb = (lo + kBlockBits - 1) >> kBlockLog2, lb = (hi + 1) >> kBlockLog2;
            if (DIR && fb < lb) {
                c = P[lb] - P[fb];
                if (lo < (fb << kBlockLog2)) c += wave_count(vecs, lo, (fb << kBlockLog2) - 1, lane);
                if ((lb << kBlockLog2) <= hi) c += wave_count(vecs, lb << kBlockLog2, hi, lane);
            } else {
                c = wave_count(vecs, lo, hi, lane);
            }
        }
        if (lane == 0) out[i] = c;
    }
}

// ends == nullptr: every query is "bit start" -- the end is the string's last byte and counts as not given
template <bool DIR, bool FLIP>
__global__ __launch_bounds__(256) void k_bits_pos_ranges(const uint4 *__restrict__ vecs, uint64_t len,
                                                         const int64_t *__restrict__ starts,
                                                         const int64_t *__restrict__ ends, uint64_t n, int unit,
                                                         const unsigned long long *__restrict__ P,
                                                         int64_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwave = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nwave) {
        uint64_t lo, hi;
        int64_t reply = -1;  // an empty interval
        if (bits_normalise(starts[i], ends ? ends[i] : (int64_t)len - 1, unit, len, &lo, &hi)) {
            uint64_t found;
            if (!DIR) {
                found = wave_find<FLIP>(vecs, lo, hi, lane);
            } else {
                // the rest of lo's block; then the first later block b with the wanted bit in blocks
                // b0 .. b -- ones: P[b+1] > P[b0], zeros: P[b+1] - P[b0] < (b+1-b0) * 32768, both monotone in
                // b -- and that block alone.  Only the last block of the interval can hold unwanted bits
                // alone (past hi, or past the string's end, which counts as zeros): it is masked by hi.
                const uint64_t b0 = (lo >> kBlockLog2) + 1, bh = hi >> kBlockLog2;
                found = wave_find<FLIP>(vecs, lo, min(hi, (b0 << kBlockLog2) - 1), lane);
                if (found >= kBitsNone && b0 <= bh) {
                    const unsigned long long base = P[b0];
                    uint64_t l = b0, r = bh + 1;  // the answer lies in [l, r]; r = bh + 1: no block has it
                    while (l < r) {
                        const uint64_t m = (l + r) >> 1;
                        const unsigned long long ones = P[m + 1] - base;
                        const bool has = FLIP ? ones < ((m + 1 - b0) << kBlockLog2) : ones > 0;
                        if (has) r = m;
                        else l = m + 1;
                    }
                    if (l <= bh) found = wave_find<FLIP>(vecs, l << kBlockLog2, min(hi, ((l + 1) << kBlockLog2) - 1), lane);
                }
            }
            reply = bits_pos_reply(found, FLIP ? 0 : 1, ends != nullptr, hi);
        }
        if (lane == 0) out[i] = reply;
    }
}

// The batch's work summary for the path choice, from the length word on the device: out3[0] = the string's
// length, out3[1] += the bytes of the clamped intervals, out3[2] = max(out3[2], the longest).
__global__ __launch_bounds__(256) void k_bits_ranges_summary(const int64_t *__restrict__ starts,
                                                             const int64_t *__restrict__ ends, uint64_t n, int unit,
                                                             int pos, const unsigned long long *__restrict__ d_len,
                                                             unsigned long long *out3) {
    __shared__ unsigned long long s_max[4];
    const uint64_t len = *d_len;
    unsigned long long sum = 0, mx = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t b = bits_interval_bytes(starts[i], ends ? ends[i] : (int64_t)len - 1, unit, len, pos != 0);
        sum += b;
        mx = max(mx, (unsigned long long)b);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned long long)__shfl_down(mx, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    block_add_u64(sum, out3 + 1);  // its barrier also publishes s_max
    if (threadIdx.x == 0) {
        atomicMax(out3 + 2, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
        if (blockIdx.x == 0) out3[0] = len;
    }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_bits_count_range(const uint32_t *words, uint64_t lo, uint64_t hi, unsigned long long *d_out, hipStream_t st) {
    const unsigned grid = grid_for((hi >> 7) - (lo >> 7) + 1, kMaxGrid);
    hipLaunchKernelGGL(k_bits_count_range, dim3(grid), dim3(256), 0, st, (const uint4 *)words, lo, hi, d_out);
}

void launch_bits_pos(const uint32_t *words, uint64_t lo, uint64_t hi, int bit, uint32_t chunk_bytes,
                     unsigned long long *d_state, int64_t none_reply, int64_t *d_out, hipStream_t st) {
    uint32_t lg = 0;
    while ((16u << lg) < chunk_bytes) ++lg;  // 16-byte vectors per chunk, log2
    const uint64_t nchunk = (((hi >> 7) - (lo >> 7)) >> lg) + 1;
    const unsigned grid = (unsigned)std::min<uint64_t>(nchunk, kMaxGrid);
    if (bit) hipLaunchKernelGGL(k_bits_pos<false>, dim3(grid), dim3(256), 0, st, (const uint4 *)words, lo, hi, lg, d_state, none_reply, d_out);
    else hipLaunchKernelGGL(k_bits_pos<true>, dim3(grid), dim3(256), 0, st, (const uint4 *)words, lo, hi, lg, d_state, none_reply, d_out);
}

void launch_bits_directory(const uint32_t *words, uint64_t len, unsigned long long *d_dir, hipStream_t st) {
    const uint32_t nblocks = (uint32_t)bits_dir_blocks(len);
    hipLaunchKernelGGL(k_bits_block_ones, dim3(std::min<uint32_t>((nblocks + 3) / 4, kMaxGrid)), dim3(256), 0, st,
                       (const uint4 *)words, (len + 15) >> 4, nblocks, d_dir);
    hipLaunchKernelGGL(k_bits_block_scan, dim3(1), dim3(1024), 0, st, d_dir, nblocks);
}

void launch_bits_scan(unsigned long long *d_counts, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_bits_block_scan, dim3(1), dim3(1024), 0, st, d_counts, n);
}

void launch_bits_ranges_summary(const int64_t *d_starts, const int64_t *d_ends, uint64_t n, int unit, bool pos,
                                const unsigned long long *d_len, unsigned long long *d_out3, hipStream_t st) {
    hipLaunchKernelGGL(k_bits_ranges_summary, dim3(grid_for(n, 512)), dim3(256), 0, st, d_starts, d_ends, n, unit,
                       pos ? 1 : 0, d_len, d_out3);
}

static unsigned grid_for_waves(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 3) / 4, kMaxGrid); }

void launch_bits_count_ranges(const uint32_t *words, uint64_t len, const int64_t *d_starts, const int64_t *d_ends,
                              uint64_t n, int unit, const unsigned long long *d_dir, uint64_t *d_out, hipStream_t st) {
    const uint4 *v = (const uint4 *)words;
    auto *out = (unsigned long long *)d_out;
    if (d_dir) hipLaunchKernelGGL(k_bits_count_ranges<true>, dim3(grid_for_waves(n)), dim3(256), 0, st, v, len, d_starts, d_ends, n, unit, d_dir, out);
    else hipLaunchKernelGGL(k_bits_count_ranges<false>, dim3(grid_for_waves(n)), dim3(256), 0, st, v, len, d_starts, d_ends, n, unit, d_dir, out);
}

void launch_bits_pos_ranges(const uint32_t *words, uint64_t len, int bit, const int64_t *d_starts, const int64_t *d_ends,
                            uint64_t n, int unit, const unsigned long long *d_dir, int64_t *d_out, hipStream_t st) {
    const uint4 *v = (const uint4 *)words;
    const dim3 grid(grid_for_waves(n));
    if (d_dir && bit) hipLaunchKernelGGL((k_bits_pos_ranges<true, false>), grid, dim3(256), 0, st, v, len, d_starts, d_ends, n, unit, d_dir, d_out);
    else if (d_dir) hipLaunchKernelGGL((k_bits_pos_ranges<true, true>), grid, dim3(256), 0, st, v, len, d_starts, d_ends, n, unit, d_dir, d_out);
    else if (bit) hipLaunchKernelGGL((k_bits_pos_ranges<false, false>), grid, dim3(256), 0, st, v, len, d_starts, d_ends, n, unit, d_dir, d_out);
    else hipLaunchKernelGGL((k_bits_pos_ranges<false, true>), grid, dim3(256), 0, st, v, len, d_starts, d_ends, n, unit, d_dir, d_out);
}

}  // namespace rbx
