// bitstream_kernels.hip -- an ordered stream of GETBIT / SETBIT commands over many bit strings in one
// call (rbx_bitset_stream): what RBatch.getBitSet(name) queues (M/RedissonBatch.java:182-184) and
// CommandBatchService executes in submission order (M/command/CommandBatchService.java:115-134,335).
// Command i is (key[i], op[i], index[i]) with op 0 = GETBIT, 1 = SETBIT index 0, 2 = SETBIT index 1; its
// reply is the bit (GETBIT) or the bit before (SETBIT), 0xFF for a command that failed alone (an index
// >= 2^32, a key of another type) and changed nothing.  DESIGN section 11.5 has the rules.
//
// The strings are reached through the key table, one BitKey per entry of `names`: the host creates and
// grows every written string between the summary pass and the execution kernels, so a SETBIT always
// lies inside its allocation; a GETBIT at or past the allocation reads 0 (the bytes from a string's
// length to its allocation's end are zero, bitset_kernels.hip).  Bit i of a string is word i >> 5,
// bit_in_word(i).
// M/ = redisson/src/main/java/org/redisson/ of the reference
#include <hip/hip_runtime.h>

#include "../../include/rbx.h"
#include "bloom_common.h"
#include "keymax_device.h"
#include "rbx_kernels.h"

namespace rbx {

typedef unsigned long long u64;

static constexpr uint8_t kFailedReply = 0xFF;
static constexpr u64 kOffsetLimit = 1ULL << 32;

__device__ __forceinline__ uint32_t key_bit(const BitKey &k, u64 idx) {
    return idx < k.cap_bits ? (uint32_t)((k.words[idx >> 5] & bit_in_word((uint32_t)idx)) != 0) : 0u;
}

// ---------------------------------------------------------------------------------
// 1. The summary pass, before anything is written.  A lane folds its commands into registers, a
// workgroup into one set of atomics on the summary words.  The per-key maximum (of index + 1: 0 = the
// key has no SETBIT that runs) goes through keymax_device.h, which keeps its atomicMax rare.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_summary(const uint32_t *__restrict__ ckey, const uint8_t *__restrict__ cop,
                                                    const uint64_t *__restrict__ cidx, uint64_t n, uint32_t nkeys,
                                                    const uint32_t *__restrict__ canon,
                                                    const uint8_t *__restrict__ wrong, u64 *sum, u64 *keymax) {
    __shared__ u64 s_oob[4], s_wrong[4], s_max[4];
    __shared__ uint32_t s_flags[4];
    u64 oob = ~0ULL, wr = ~0ULL, mx = 0;
    uint32_t flags = 0;
    KeymaxHeld held;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t k = ckey[i];
        const uint32_t op = cop[i];
        const u64 idx = cidx[i];
        if (k >= nkeys || op > 2) {
            flags |= kBsIllegal;
            continue;
        }
        flags |= op == 0 ? kBsHasGet : (op == 1 ? kBsHasSet0 : kBsHasSet1);
        if (idx >= kOffsetLimit) {  // the single call checks the offset first
            oob = min(oob, (u64)i);
        } else if (wrong[k]) {
            wr = min(wr, (u64)i);
        } else {
            mx = max(mx, idx);
            if (op) held.take(keymax, canon[k], idx + 1);
        }
    }
    held.flush(keymax);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        oob = min(oob, (u64)__shfl_down(oob, d, 64));
        wr = min(wr, (u64)__shfl_down(wr, d, 64));
        mx = max(mx, (u64)__shfl_down(mx, d, 64));
        flags |= (uint32_t)__shfl_down((int)flags, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_oob[threadIdx.x >> 6] = oob;
        s_wrong[threadIdx.x >> 6] = wr;
        s_max[threadIdx.x >> 6] = mx;
        s_flags[threadIdx.x >> 6] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        oob = min(min(s_oob[0], s_oob[1]), min(s_oob[2], s_oob[3]));
        wr = min(min(s_wrong[0], s_wrong[1]), min(s_wrong[2], s_wrong[3]));
        mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        flags = s_flags[0] | s_flags[1] | s_flags[2] | s_flags[3];
        if (oob != ~0ULL) atomicMin(sum + kBsFirstOob, oob);
        if (wr != ~0ULL) atomicMin(sum + kBsFirstWrong, wr);
        if (flags) atomicOr(sum + kBsFlags, (u64)flags);
        if (mx) atomicMax(sum + kBsMaxIndex, mx);
    }
}

// ---------------------------------------------------------------------------------
// 2. Gather: a batch without SETBITs.  One lane per command: its key's record, one word, one byte.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_gather(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                                                   const uint64_t *__restrict__ cidx, uint64_t n,
                                                   uint8_t *__restrict__ replies) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const BitKey k = tab[ckey[i]];
        const u64 idx = cidx[i];
        replies[i] = (idx >= kOffsetLimit || (k.flags & kBitKeyWrong)) ? kFailedReply : (uint8_t)key_bit(k, idx);
    }
}

// ---------------------------------------------------------------------------------
// 3. Scatter: SETBITs of one value and no replies, so the order is immaterial (k_bits_scatter).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_scatter(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                                                    const uint64_t *__restrict__ cidx, uint64_t n, uint32_t value) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const BitKey k = tab[ckey[i]];
        const u64 idx = cidx[i];
        if ((k.flags & kBitKeyWrong) || idx >= k.cap_bits) continue;  // a failed command (the host sized every other)
        if (value) atomicOr(k.words + (idx >> 5), bit_in_word((uint32_t)idx));
        else atomicAnd(k.words + (idx >> 5), ~bit_in_word((uint32_t)idx));
    }
}

// ---------------------------------------------------------------------------------
// 4. Grouped: commands on different (key, bit) cells are independent, those on one cell totally
// ordered.  k_bs_pairs emits (cell, position) with cell = canonical key id << index_bits | index, a
// failed command's cell carrying the bit above every cell (it sorts behind them and no run reads it);
// a stable sort by cell lists each cell's commands in array order; the lane at a run's head reads the
// bit once, walks the run writing the replies and stores the bit once if it changed.  A cell has one
// writer, but cells share words: the store is an atomicOr or atomicAnd.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_pairs(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                                                  const uint64_t *__restrict__ cidx, uint32_t n, uint32_t index_bits,
                                                  u64 failed_cell, u64 *__restrict__ cell, uint32_t *__restrict__ pos,
                                                  uint8_t *__restrict__ replies) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const BitKey k = tab[ckey[i]];
        const u64 idx = cidx[i];
        const bool failed = idx >= kOffsetLimit || (k.flags & kBitKeyWrong);
        cell[i] = failed ? failed_cell : (((u64)k.canon << index_bits) | idx);
        pos[i] = i;
        if (failed && replies) replies[i] = kFailedReply;
    }
}

__global__ __launch_bounds__(256) void k_bs_runs(const BitKey *__restrict__ tab, const uint8_t *__restrict__ cop,
                                                 const u64 *__restrict__ cell, const uint32_t *__restrict__ pos,
                                                 uint32_t n, uint32_t index_bits, u64 failed_cell,
                                                 uint8_t *__restrict__ replies) {
    const u64 index_mask = (1ULL << index_bits) - 1;  // index_bits <= 32
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 c = cell[i];
        if (c == failed_cell || (i > 0 && cell[i - 1] == c)) continue;  // failed, or not a run's head
        const BitKey k = tab[c >> index_bits];
        const u64 idx = c & index_mask;
        const uint32_t was = key_bit(k, idx);
        uint32_t cur = was;
        uint32_t j = i;
        do {
            const uint32_t p = pos[j];
            const uint32_t op = cop[p];
            if (replies) replies[p] = (uint8_t)cur;
            if (op) cur = op - 1;
            ++j;
        } while (j < n && cell[j] == c);
        if (cur != was && idx < k.cap_bits) {  // (the host sized the string for every SETBIT)
            if (cur) atomicOr(k.words + (idx >> 5), bit_in_word((uint32_t)idx));
            else atomicAnd(k.words + (idx >> 5), ~bit_in_word((uint32_t)idx));
        }
    }
}

// ---------------------------------------------------------------------------------
// 5. Serial: one lane runs the commands in array order (k_bitfield_serial's form).  Small batches, and
// the independent implementation the tests hold the other paths against.
// ---------------------------------------------------------------------------------
__global__ void k_bs_serial(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                            const uint8_t *__restrict__ cop, const uint64_t *__restrict__ cidx, uint64_t n,
                            uint8_t *__restrict__ replies) {
    for (uint64_t i = 0; i < n; ++i) {
        const BitKey k = tab[ckey[i]];
        const u64 idx = cidx[i];
        const uint32_t op = cop[i];
        uint8_t r = kFailedReply;
        if (idx < kOffsetLimit && !(k.flags & kBitKeyWrong)) {
            r = (uint8_t)key_bit(k, idx);
            if (op && idx < k.cap_bits) {
                uint32_t *w = k.words + (idx >> 5);
                const uint32_t m = bit_in_word((uint32_t)idx);
                *w = op == 2 ? (*w | m) : (*w & ~m);
            }
        }
        if (replies) replies[i] = r;
    }
}

// ---------------------------------------------------------------------------------
// 6. Lengths: SETBIT grows the string to (index >> 3) + 1 bytes whatever it writes.  keymax holds the
// largest in-range SETBIT index + 1 per canonical key (0 = none).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_lengths(const BitKey *__restrict__ tab, const u64 *__restrict__ keymax,
                                                    uint32_t nkeys) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nkeys; i += stride) {
        const BitKey k = tab[i];
        const u64 m = keymax[i];
        if (m && k.canon == i && k.len) atomicMax(k.len, (u64)(((m - 1) >> 3) + 1));
    }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_bitstream_summary(const uint32_t *d_key, const uint8_t *d_op, const uint64_t *d_idx, uint64_t n,
                              uint32_t nkeys, const uint32_t *d_canon, const uint8_t *d_wrong,
                              unsigned long long *d_sum, unsigned long long *d_keymax, hipStream_t st) {
    // 512 workgroups: each ends in up to four atomics on the same words (k_fields_check_signs measured this)
    hipLaunchKernelGGL(k_bs_summary, dim3(grid_for(n, 512)), dim3(256), 0, st, d_key, d_op, d_idx, n, nkeys, d_canon,
                       d_wrong, d_sum, d_keymax);
}

void launch_bitstream_gather(const BitKey *d_tab, const uint32_t *d_key, const uint64_t *d_idx, uint64_t n,
                             uint8_t *d_replies, hipStream_t st) {
    hipLaunchKernelGGL(k_bs_gather, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_idx, n, d_replies);
}

void launch_bitstream_scatter(const BitKey *d_tab, const uint32_t *d_key, const uint64_t *d_idx, uint64_t n, bool value,
                              hipStream_t st) {
    hipLaunchKernelGGL(k_bs_scatter, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_idx, n,
                       value ? 1u : 0u);
}

void launch_bitstream_serial(const BitKey *d_tab, const uint32_t *d_key, const uint8_t *d_op, const uint64_t *d_idx,
                             uint64_t n, uint8_t *d_replies, hipStream_t st) {
    hipLaunchKernelGGL(k_bs_serial, dim3(1), dim3(1), 0, st, d_tab, d_key, d_op, d_idx, n, d_replies);
}

void launch_bitstream_lengths(const BitKey *d_tab, const unsigned long long *d_keymax, uint32_t nkeys, hipStream_t st) {
    hipLaunchKernelGGL(k_bs_lengths, dim3(grid_for(nkeys, kMaxGrid)), dim3(256), 0, st, d_tab, d_keymax, nkeys);
}

int launch_bitstream_grouped(const BitKey *d_tab, const uint32_t *d_key, const uint8_t *d_op, const uint64_t *d_idx,
                             uint32_t n, uint8_t *d_replies, int index_bits, int key_bits, bool has_failed,
                             void *d_scratch, size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<u64> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, n, &b);
    if (e) return e;
    // the bit above every cell (index_bits + key_bits <= 63); the sort looks at it only when a command failed
    const u64 failed_cell = 1ULL << (index_bits + key_bits);
    const int cell_bits = index_bits + key_bits + (has_failed ? 1 : 0);
    hipLaunchKernelGGL(k_bs_pairs, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_idx, n,
                       (uint32_t)index_bits, failed_cell, b.cell_in, b.pos_in, d_replies);
    e = cell_sort(b, n, 0, cell_bits, st);  // over the cells' significant bits only
    if (e) return e;
    hipLaunchKernelGGL(k_bs_runs, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_op, b.cell_out, b.pos_out, n,
                       (uint32_t)index_bits, failed_cell, d_replies);
    return 0;
}

}  // namespace rbx
