// fieldstream_kernels.hip -- an ordered stream of single-sub-command BITFIELDs over many bit strings in one
// call (rbx_bitset_field_stream): what RBatch.getBitSet(name)'s typed-field methods queue
// (M/api/RBitSetAsync.java:36-206) and a Spring Data pipeline of one-sub-command bitField calls sends.
// Command i is `BITFIELD names[key[i]] [OVERFLOW m] GET|SET|INCRBY <i|u><size> <offset> [value]`, written as
// an rbx_field_cmd; its reply is what rbx_bitset_bitfield with that one sub-command returns, its status 0,
// 1 (nil: OVERFLOW FAIL) or 0xFF (the command failed alone and changed nothing).  DESIGN section 11.6 has
// the rules.
//
// The strings are reached through the key table of bitstream_kernels.hip, one BitKey per entry of `names`:
// the host creates and grows every written string between the summary pass and the execution kernels, so
// a SET / INCRBY always lies inside its allocation; a GET reads zero at or past it (field_device.h).
// M/ = redisson/src/main/java/org/redisson/ of the reference
#include <hip/hip_runtime.h>

#include "../../include/rbx.h"
#include "bloom_common.h"
#include "field_device.h"
#include "keymax_device.h"
#include "rbx_kernels.h"

namespace rbx {

typedef unsigned long long u64;

static constexpr uint8_t kFailedStatus = 0xFF;
static_assert(kFsBadType == kFieldCmdBadType && kFsBadOffset == kFieldCmdBadOffset, "one numbering of the failure kinds");

// 0 = the command runs, else its failure kind (kFsBadType, kFsBadOffset, kFsWrongType), checked in the
// order the single call applies them: the type, the offset limit, the key's type
__device__ __forceinline__ int fs_failure(const rbx_field_cmd &c, bool wrong) {
    const int f = field_cmd_check(c.is_signed, c.size, c.offset);
    return f ? f : (wrong ? kFsWrongType : 0);
}

// one command that runs, on its key's record: the status (1 = nil), the reply in *reply
__device__ __forceinline__ uint8_t fs_run(const BitKey &k, const rbx_field_cmd &c, int64_t *reply) {
    *reply = 0;
    if (c.op != RBX_FIELD_GET && c.offset + c.size > k.cap_bits) return 0;  // (the host sized the string: never taken)
    bool nil;
    *reply = field_apply_ov((u64 *)k.words, k.cap_bits >> 6, c.op, c.is_signed, c.size, c.overflow, c.offset, c.value,
                            &nil);
    return (uint8_t)nil;
}

// any one command: checked, run, answered
__device__ __forceinline__ void fs_exec(const BitKey &k, const rbx_field_cmd &c, uint64_t i,
                                        int64_t *__restrict__ replies, uint8_t *__restrict__ status) {
    int64_t r = 0;
    uint8_t s = kFailedStatus;
    if (!fs_failure(c, k.flags & kBitKeyWrong)) s = fs_run(k, c, &r);
    if (replies) replies[i] = r;
    if (status) status[i] = s;
}

// ---------------------------------------------------------------------------------
// 1. The summary pass, before anything is written (k_bs_summary's form).  A lane folds its commands into
// registers, a workgroup into one set of atomics on the summary words.  The per-key maximum (of offset +
// size over the SET / INCRBY that run: 0 = none) goes through keymax_device.h, as there.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fs_summary(const uint32_t *__restrict__ ckey,
                                                    const rbx_field_cmd *__restrict__ cmds, uint64_t n, uint32_t nkeys,
                                                    const uint32_t *__restrict__ canon,
                                                    const uint8_t *__restrict__ wrong, u64 *sum, u64 *keymax) {
    __shared__ u64 s_type[4], s_off[4], s_wrong[4], s_max[4], s_sizes[4];
    __shared__ uint32_t s_flags[4];
    u64 bad_type = ~0ULL, bad_off = ~0ULL, wr = ~0ULL, mx = 0, sizes = 0;
    uint32_t flags = 0;
    KeymaxHeld held;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t k = ckey[i];
        const rbx_field_cmd c = cmds[i];
        if (k >= nkeys || c.op > RBX_FIELD_INCRBY || c.overflow > RBX_OVERFLOW_FAIL || c.is_signed > 1) {
            flags |= kFsIllegal;
            continue;
        }
        const int f = fs_failure(c, wrong[k] != 0);
        if (f == kFsBadType) {
            bad_type = min(bad_type, (u64)i);
        } else if (f == kFsBadOffset) {
            bad_off = min(bad_off, (u64)i);
        } else if (f == kFsWrongType) {
            wr = min(wr, (u64)i);
        } else {
            const u64 end = c.offset + c.size;  // <= 2^32
            flags |= kFsHasGet << c.op;
            sizes |= 1ULL << (c.size - 1);
            mx = max(mx, (end - 1) >> 6);
            if ((c.offset >> 6) != ((end - 1) >> 6)) flags |= kFsStraddles;
            if ((uint32_t)c.offset % c.size != 0) flags |= kFsUnaligned;
            if (c.op != RBX_FIELD_GET) {
                flags |= kFsWrap << c.overflow;
                held.take(keymax, canon[k], end);
            }
        }
    }
    held.flush(keymax);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        bad_type = min(bad_type, (u64)__shfl_down(bad_type, d, 64));
        bad_off = min(bad_off, (u64)__shfl_down(bad_off, d, 64));
        wr = min(wr, (u64)__shfl_down(wr, d, 64));
        mx = max(mx, (u64)__shfl_down(mx, d, 64));
        sizes |= (u64)__shfl_down(sizes, d, 64);
        flags |= (uint32_t)__shfl_down((int)flags, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_type[threadIdx.x >> 6] = bad_type;
        s_off[threadIdx.x >> 6] = bad_off;
        s_wrong[threadIdx.x >> 6] = wr;
        s_max[threadIdx.x >> 6] = mx;
        s_sizes[threadIdx.x >> 6] = sizes;
        s_flags[threadIdx.x >> 6] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bad_type = min(min(s_type[0], s_type[1]), min(s_type[2], s_type[3]));
        bad_off = min(min(s_off[0], s_off[1]), min(s_off[2], s_off[3]));
        wr = min(min(s_wrong[0], s_wrong[1]), min(s_wrong[2], s_wrong[3]));
        mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        sizes = s_sizes[0] | s_sizes[1] | s_sizes[2] | s_sizes[3];
        flags = s_flags[0] | s_flags[1] | s_flags[2] | s_flags[3];
        if (bad_type != ~0ULL) atomicMin(sum + kFsFirstType, bad_type);
        if (bad_off != ~0ULL) atomicMin(sum + kFsFirstOffset, bad_off);
        if (wr != ~0ULL) atomicMin(sum + kFsFirstWrong, wr);
        if (flags) atomicOr(sum + kFsFlags, (u64)flags);
        if (sizes) atomicOr(sum + kFsSizes, sizes);
        if (mx) atomicMax(sum + kFsMaxWord, mx);
    }
}

// ---------------------------------------------------------------------------------
// 2. Gather: a batch without SET / INCRBY.  One lane per command: its key's record, then k_fields_get's body.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fs_gather(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                                                   const rbx_field_cmd *__restrict__ cmds, uint64_t n,
                                                   int64_t *__restrict__ replies, uint8_t *__restrict__ status) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        fs_exec(tab[ckey[i]], cmds[i], i, replies, status);  // every command that runs is a GET: nothing is written
}

// ---------------------------------------------------------------------------------
// 3. Atomic: every command that runs is an INCRBY under WRAP whose reply is not wanted, all of ONE size that
// divides 64, each at a multiple of it.  Such fields are equal or disjoint and lie inside one aligned
// word, and sums modulo 2^size commute, so the commands run in any order: one compare-and-swap loop per
// command (k_fields_incr_atomic behind a table record).  This does NOT extend to a batch of mixed sizes,
// aligned or not: a u8 lies inside a u16, and a carry out of the u8 is dropped when the u8 is incremented
// but enters the u16's upper byte when the u16 is -- u8 += 1 then u16 += 255 on 00ff gives 00ff, the other
// order 0100.  Such a batch goes to the word cells.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fs_incr_atomic(const BitKey *__restrict__ tab,
                                                        const uint32_t *__restrict__ ckey,
                                                        const rbx_field_cmd *__restrict__ cmds, uint64_t n,
                                                        uint8_t *__restrict__ status) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const BitKey k = tab[ckey[i]];
        const rbx_field_cmd c = cmds[i];
        const bool failed = fs_failure(c, k.flags & kBitKeyWrong) != 0;
        if (status) status[i] = failed ? kFailedStatus : 0;
        if (failed) continue;
        const u64 mask = field_mask(c.size);
        const u64 inc = (u64)c.value & mask;
        if (inc == 0 || c.offset + c.size > k.cap_bits) continue;  // (the host sized the string: the latter is never taken)
        const uint32_t shift = 64 - (uint32_t)(c.offset & 63) - c.size;
        u64 *p = (u64 *)k.words + (c.offset >> 6);
        u64 seen = *p, expect;
        do {
            expect = seen;
            const u64 be = __builtin_bswap64(expect);
            const u64 f = ((be >> shift) + inc) & mask;
            seen = atomicCAS(p, expect, __builtin_bswap64((be & ~(mask << shift)) | (f << shift)));
        } while (seen != expect);
    }
}

// ---------------------------------------------------------------------------------
// 4. Grouped.  k_fs_cells emits (cell, position); a failed command's cell carries the bit above every cell
// (it sorts behind them and no run reads it), as in k_bs_pairs.  A stable sort by cell lists each cell's
// commands in array order.
//   word cells  cell = canonical key id << word_bits | offset >> 6, for a batch whose every running command
//               lies inside one aligned 64-bit word: commands on different words are independent whatever
//               their sizes.  The lane at a run's head loads the byte-swapped word once, applies each command
//               to the register through field_rule, and stores the word once if it changed.  A word has
//               one writer, so the store is plain.
//   key cells   cell = canonical key id (word_bits = 0): fields that straddle words may partly overlap
//               fields of other words, so a key's commands are totally ordered; keys stay independent.  One
//               lane per key walks its commands with the non-atomic apply.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fs_cells(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                                                  const rbx_field_cmd *__restrict__ cmds, uint32_t n,
                                                  uint32_t word_bits, u64 failed_cell, u64 *__restrict__ cell,
                                                  uint32_t *__restrict__ pos, int64_t *__restrict__ replies,
                                                  uint8_t *__restrict__ status) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const BitKey k = tab[ckey[i]];
        const rbx_field_cmd c = cmds[i];
        const bool failed = fs_failure(c, k.flags & kBitKeyWrong) != 0;
        cell[i] = failed ? failed_cell : (((u64)k.canon << word_bits) | (word_bits ? c.offset >> 6 : 0ULL));
        pos[i] = i;
        if (failed) {
            if (replies) replies[i] = 0;
            if (status) status[i] = kFailedStatus;
        }
    }
}

__global__ __launch_bounds__(256) void k_fs_word_runs(const BitKey *__restrict__ tab,
                                                      const rbx_field_cmd *__restrict__ cmds,
                                                      const u64 *__restrict__ cell, const uint32_t *__restrict__ pos,
                                                      uint32_t n, uint32_t word_bits, u64 failed_cell,
                                                      int64_t *__restrict__ replies, uint8_t *__restrict__ status) {
    const u64 word_mask = (1ULL << word_bits) - 1;  // word_bits <= 26
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 cl = cell[i];
        if (cl == failed_cell || (i > 0 && cell[i - 1] == cl)) continue;  // failed, or not a run's head
        const BitKey k = tab[cl >> word_bits];
        const u64 q = cl & word_mask;
        const bool inside = q < (k.cap_bits >> 6);  // a word at or past the allocation is only read (as zero)
        u64 *p = (u64 *)k.words + q;
        const u64 was = inside ? __builtin_bswap64(*p) : 0ULL;
        u64 be = was;
        uint32_t j = i;
        do {
            const uint32_t at = pos[j];
            const rbx_field_cmd c = cmds[at];
            const u64 mask = field_mask(c.size);
            const uint32_t shift = 64 - (uint32_t)(c.offset & 63) - c.size;  // the field ends inside the word
            int64_t now, reply;
            const bool nil = field_rule(c.op, c.is_signed, c.size, c.overflow,
                                        field_extend((be >> shift) & mask, c.size, c.is_signed), c.value, &now, &reply);
            if (c.op != RBX_FIELD_GET && !nil) be = (be & ~(mask << shift)) | (((u64)now & mask) << shift);
            if (replies) replies[at] = reply;
            if (status) status[at] = (uint8_t)nil;
            ++j;
        } while (j < n && cell[j] == cl);
        if (be != was && inside) *p = __builtin_bswap64(be);
    }
}

__global__ __launch_bounds__(256) void k_fs_key_runs(const BitKey *__restrict__ tab,
                                                     const rbx_field_cmd *__restrict__ cmds,
                                                     const u64 *__restrict__ cell, const uint32_t *__restrict__ pos,
                                                     uint32_t n, u64 failed_cell, int64_t *__restrict__ replies,
                                                     uint8_t *__restrict__ status) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 cl = cell[i];
        if (cl == failed_cell || (i > 0 && cell[i - 1] == cl)) continue;
        const BitKey k = tab[cl];
        uint32_t j = i;
        do {
            const uint32_t at = pos[j];
            int64_t r;
            const uint8_t s = fs_run(k, cmds[at], &r);
            if (replies) replies[at] = r;
            if (status) status[at] = s;
            ++j;
        } while (j < n && cell[j] == cl);
    }
}

// ---------------------------------------------------------------------------------
// 5. Serial: one lane runs the commands in array order (k_bitfield_serial behind the key table).  Small
// batches, and the independent implementation the tests hold the other paths against.
// ---------------------------------------------------------------------------------
__global__ void k_fs_serial(const BitKey *__restrict__ tab, const uint32_t *__restrict__ ckey,
                            const rbx_field_cmd *__restrict__ cmds, uint64_t n, int64_t *__restrict__ replies,
                            uint8_t *__restrict__ status) {
    for (uint64_t i = 0; i < n; ++i) fs_exec(tab[ckey[i]], cmds[i], i, replies, status);
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_fieldstream_summary(const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n, uint32_t nkeys,
                                const uint32_t *d_canon, const uint8_t *d_wrong, unsigned long long *d_sum,
                                unsigned long long *d_keymax, hipStream_t st) {
    // 512 workgroups: each ends in up to six atomics on the same words (launch_bitstream_summary)
    hipLaunchKernelGGL(k_fs_summary, dim3(grid_for(n, 512)), dim3(256), 0, st, d_key, d_cmds, n, nkeys, d_canon, d_wrong,
                       d_sum, d_keymax);
}

void launch_fieldstream_gather(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n,
                               int64_t *d_replies, uint8_t *d_status, hipStream_t st) {
    hipLaunchKernelGGL(k_fs_gather, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, n, d_replies,
                       d_status);
}

void launch_fieldstream_incr_atomic(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n,
                                    uint8_t *d_status, hipStream_t st) {
    hipLaunchKernelGGL(k_fs_incr_atomic, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, n,
                       d_status);
}

void launch_fieldstream_serial(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n,
                               int64_t *d_replies, uint8_t *d_status, hipStream_t st) {
    hipLaunchKernelGGL(k_fs_serial, dim3(1), dim3(1), 0, st, d_tab, d_key, d_cmds, n, d_replies, d_status);
}

int launch_fieldstream_grouped(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint32_t n,
                               int64_t *d_replies, uint8_t *d_status, int word_bits, int key_bits, bool has_failed,
                               void *d_scratch, size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<u64> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, n, &b);
    if (e) return e;
    // the bit above every cell (word_bits + key_bits <= 57); the sort looks at it only when a command failed
    const u64 failed_cell = 1ULL << (word_bits + key_bits);
    const int cell_bits = word_bits + key_bits + (has_failed ? 1 : 0);
    hipLaunchKernelGGL(k_fs_cells, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, n,
                       (uint32_t)word_bits, failed_cell, b.cell_in, b.pos_in, d_replies, d_status);
    e = cell_sort(b, n, 0, cell_bits, st);  // over the cells' significant bits only
    if (e) return e;
    if (word_bits)
        hipLaunchKernelGGL(k_fs_word_runs, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_cmds, b.cell_out,
                           b.pos_out, n, (uint32_t)word_bits, failed_cell, d_replies, d_status);
    else
        hipLaunchKernelGGL(k_fs_key_runs, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_tab, d_cmds, b.cell_out,
                           b.pos_out, n, failed_cell, d_replies, d_status);
    return 0;
}

}  // namespace rbx
