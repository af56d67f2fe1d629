// bitfield_kernels.hip -- RBitSet's typed fields (M/RedissonBitSet.java:71-254): every call is one
// Redis `BITFIELD key [OVERFLOW WRAP|SAT|FAIL] GET|SET|INCRBY <i|u><size> <offset> [value]`
// ([redis-7.2] bitops.c bitfieldGeneric, restated in DESIGN sections 11 and 11.3).  A field is `size`
// bits of the string from bit `offset`, most significant bit first, at any alignment.  The overflow
// mode is a template parameter of the writing kernels: the WRAP instantiations are the modular
// arithmetic below, SAT and FAIL go through field_rule (field_rule.h).
//
// The bitmap is addressed here as aligned 64-bit words (field_device.h has the layout and the loads and
// stores); the kernels keep the bytes from the string's length to the allocation's end zero (they write
// only inside fields the host sized the string for).
// M/ = redisson/src/main/java/org/redisson/ of the reference
#include <hip/hip_runtime.h>

#include "../../include/rbx.h"
#include "bloom_common.h"
#include "field_device.h"  // field_load / field_store / field_apply_ov; field_rule.h
#include "rbx_kernels.h"

namespace rbx {

typedef unsigned long long u64;

// one sub-command on the field at `off`: the reply, the field updated in place
template <bool ATOMIC>
__device__ __forceinline__ int64_t field_apply(u64 *w, uint64_t cap_words, int op, uint32_t is_signed, uint32_t size,
                                               uint64_t off, int64_t value) {
    const u64 old = field_load(w, cap_words, off, size);
    if (op == RBX_FIELD_GET) return field_extend(old, size, is_signed);
    const u64 now = (op == RBX_FIELD_SET ? (u64)value : old + (u64)value) & field_mask(size);
    field_store<ATOMIC>(w, off, size, now);
    return field_extend(op == RBX_FIELD_SET ? old : now, size, is_signed);
}

// ---------------------------------------------------------------------------------
// 1. The batch's check: out[0] = max(out[0], max offset), out[1] |= (some offset % size != 0).
// The host adds `size` to the maximum (every sub-command has the same type) for the offset
// limit, the growth and the new length, and picks the path from the alignment word.
// ---------------------------------------------------------------------------------
// a lane's maximum and flags into out[0] (max) and out[1] (or), one pair of atomics per workgroup
__device__ __forceinline__ void check_reduce(u64 m, uint32_t flags, u64 *out) {
    __shared__ u64 s_max[4];
    __shared__ uint32_t s_flags[4];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m = max(m, (u64)__shfl_down(m, d, 64));
        flags |= (uint32_t)__shfl_down((int)flags, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_max[threadIdx.x >> 6] = m;
        s_flags[threadIdx.x >> 6] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(out, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
        const uint32_t f = s_flags[0] | s_flags[1] | s_flags[2] | s_flags[3];
        if (f) atomicOr(out + 1, (u64)f);
    }
}

__global__ __launch_bounds__(256) void k_fields_check(const uint64_t *__restrict__ offs, uint64_t n, uint32_t size,
                                                      u64 *out) {
    u64 m = 0;
    uint32_t mis = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 o = offs[i];
        m = max(m, o);
        mis |= (uint32_t)(o % size != 0);
    }
    check_reduce(m, mis, out);
}

// The check of a SAT INCRBY without replies also reads the increments: out[1] gets bit 1 = some increment
// is > 0 and bit 2 = some increment is < 0 (saturating sums commute only when every increment has one
// sign).  Twice the bytes of k_fields_check: VEC = each lane takes two elements of each array in one
// 16-byte load (both arrays 16-byte aligned), else one element as k_fields_check does.
// (The remainder is taken of the offset's low 32 bits, a shorter instruction sequence than the 64-bit one:
// an offset of 2^32 or more fails the batch on its maximum before the alignment flag is looked at.  The
// pass's time did not depend on it, nor on 16-byte loads; it fell from 92 to 68 us at 2^24 elements when the
// grid went back from 2048 to 512 workgroups, each of which ends in two atomics on the same two words.)
__device__ __forceinline__ uint32_t check_flags(u64 o, int64_t v, uint32_t size) {
    return (uint32_t)((uint32_t)o % size != 0) | (v > 0 ? 2u : 0u) | (v < 0 ? 4u : 0u);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_fields_check_signs(const uint64_t *__restrict__ offs,
                                                            const int64_t *__restrict__ vals, uint64_t n,
                                                            uint32_t size, u64 *out) {
    u64 m = 0;
    uint32_t flags = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const ulonglong2 *offs2 = (const ulonglong2 *)offs;
    const longlong2 *vals2 = (const longlong2 *)vals;
    if (VEC) {
        for (uint64_t i = first; i < n / 2; i += stride) {
            const ulonglong2 o = offs2[i];
            const longlong2 v = vals2[i];
            m = max(m, max((u64)o.x, (u64)o.y));
            flags |= check_flags(o.x, v.x, size) | check_flags(o.y, v.y, size);
        }
        if ((n & 1) && first == 0) {  // the odd element out
            m = max(m, (u64)offs[n - 1]);
            flags |= check_flags(offs[n - 1], vals[n - 1], size);
        }
    } else {
        for (uint64_t i = first; i < n; i += stride) {
            m = max(m, (u64)offs[i]);
            flags |= check_flags(offs[i], vals[i], size);
        }
    }
    check_reduce(m, flags, out);
}

// ---------------------------------------------------------------------------------
// 2. GET, one lane per element, any offsets.  Nothing at or past the allocation is read.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fields_get(const u64 *__restrict__ w, uint64_t cap_words,
                                                    const uint64_t *__restrict__ offs, uint64_t n, uint32_t size,
                                                    uint32_t is_signed, int64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = field_extend(field_load(w, cap_words, offs[i], size), size, is_signed);
}

// ---------------------------------------------------------------------------------
// 3. INCRBY without replies on aligned fields whose size divides 64: such a field lies inside one
// aligned word, and sums modulo 2^size commute, so the elements run in any order and duplicates
// need no grouping -- one compare-and-swap loop per element.  The addition is done on the
// byte-swapped word, in the field's own (big-endian) bit positions.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fields_incr_atomic(u64 *w, u64 *len, uint64_t cap_bits,
                                                            const uint64_t *__restrict__ offs,
                                                            const int64_t *__restrict__ incs, uint64_t n, uint32_t size,
                                                            uint64_t new_len) {
    const u64 mask = field_mask(size);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t off = offs[i];
        const u64 inc = (u64)incs[i] & mask;
        if (inc == 0 || off + size > cap_bits) continue;  // (the host sized the bitmap: the latter is never taken)
        const uint32_t shift = 64 - (uint32_t)(off & 63) - size;
        u64 *p = w + (off >> 6);
        u64 seen = *p, expect;
        do {
            expect = seen;
            const u64 be = __builtin_bswap64(expect);
            const u64 f = ((be >> shift) + inc) & mask;
            seen = atomicCAS(p, expect, __builtin_bswap64((be & ~(mask << shift)) | (f << shift)));
        } while (seen != expect);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(len, (u64)new_len);
}

// ---------------------------------------------------------------------------------
// 3b. The same under OVERFLOW SAT, for a batch whose increments all have one sign: then
// clamp(old + sum of the increments) is the result in every order, so the elements still run in
// any order.  (With mixed signs they do not: a u8 at 250 with +10, -10 ends at 245, with -10, +10
// at 250 -- the host sends such a batch to the grouped path.)  The sum is clamped in the field's type
// inside the loop.  A field only moves towards one bound during the kernel, so a field read at that
// bound is final and the element issues no atomic; a stale read of an earlier value costs one
// failed compare-and-swap.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fields_incr_sat(u64 *w, u64 *len, uint64_t cap_bits,
                                                         const uint64_t *__restrict__ offs,
                                                         const int64_t *__restrict__ incs, uint64_t n, uint32_t size,
                                                         uint32_t is_signed, uint64_t new_len) {
    const u64 mask = field_mask(size);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t off = offs[i];
        const int64_t inc = incs[i];
        if (inc == 0 || off + size > cap_bits) continue;  // (the host sized the bitmap: the latter is never taken)
        const uint32_t shift = 64 - (uint32_t)(off & 63) - size;
        u64 *p = w + (off >> 6);
        u64 seen = *p, expect;
        do {
            expect = seen;
            const u64 be = __builtin_bswap64(expect);
            const int64_t old = field_extend((be >> shift) & mask, size, is_signed);
            int64_t now, reply;
            field_rule(kFieldIncrBy, (int)is_signed, (int)size, kOverflowSat, old, inc, &now, &reply);
            if (now == old) break;  // at the bound it moves towards
            seen = atomicCAS(p, expect, __builtin_bswap64((be & ~(mask << shift)) | (((u64)now & mask) << shift)));
        } while (seen != expect);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(len, (u64)new_len);
}

// ---------------------------------------------------------------------------------
// 4. Every other aligned SET / INCRBY: the (slot, position) pairs arrive stably sorted by slot
// (slot = offset / size), so a run of equal slots lists one field's sub-commands in array order.
// The lane at a run's head reads the field once, walks the run writing each reply, and stores
// the final value once.  Fields are pairwise disjoint and each has one writer, but they share
// words: the store is atomicAnd + atomicOr.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fields_slots(const uint64_t *__restrict__ offs, uint32_t n, uint32_t size,
                                                      uint32_t *__restrict__ slot, uint32_t *__restrict__ pos) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        slot[i] = (uint32_t)(offs[i] / size);  // offsets are below 2^32
        pos[i] = i;
    }
}

// MODE != WRAP: each step of the walk is field_rule on the running value; a nil step (FAIL on
// overflow) sets nil[p] and leaves the running value as it is.
template <int MODE>
__global__ __launch_bounds__(256) void k_fields_runs(u64 *w, u64 *len, uint64_t cap_bits, int op, uint32_t is_signed,
                                                     uint32_t size, const uint32_t *__restrict__ slot,
                                                     const uint32_t *__restrict__ pos, uint32_t n,
                                                     const int64_t *__restrict__ values, int64_t *__restrict__ replies,
                                                     uint8_t *__restrict__ nil, uint64_t new_len) {
    const u64 mask = field_mask(size);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t s = slot[i];
        if (i > 0 && slot[i - 1] == s) continue;  // not a run's head
        const uint64_t off = (uint64_t)s * size;
        if (off + size > cap_bits) continue;  // (the host sized the bitmap: never taken)
        u64 cur = field_load(w, cap_bits >> 6, off, size);
        uint32_t j = i;
        do {
            const uint32_t p = pos[j];
            const u64 v = (u64)values[p];
            if (MODE != RBX_OVERFLOW_WRAP) {
                int64_t now, reply;
                const bool none = field_rule(op, (int)is_signed, (int)size, MODE, field_extend(cur, size, is_signed),
                                             (int64_t)v, &now, &reply);
                cur = (u64)now & mask;
                if (replies) replies[p] = reply;
                if (MODE == RBX_OVERFLOW_FAIL && nil) nil[p] = (uint8_t)none;
            } else if (op == RBX_FIELD_SET) {
                if (replies) replies[p] = field_extend(cur, size, is_signed);
                cur = v & mask;
            } else {
                cur = (cur + v) & mask;
                if (replies) replies[p] = field_extend(cur, size, is_signed);
            }
            ++j;
        } while (j < n && slot[j] == s);
        field_store<true>(w, off, size, cur);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(len, (u64)new_len);
}

// ---------------------------------------------------------------------------------
// 5. The exact path: one lane runs the sub-commands in array order.  Unaligned fields may partly
// overlap, so a sub-command's reply and result depend on every earlier one.  Also the single call.
// ---------------------------------------------------------------------------------
template <int MODE>
__global__ void k_fields_serial(u64 *w, u64 *len, uint64_t cap_bits, int op, uint32_t is_signed, uint32_t size,
                                const uint64_t *__restrict__ offs, const int64_t *__restrict__ values, uint64_t n,
                                int64_t *__restrict__ replies, uint8_t *__restrict__ nil, uint64_t new_len) {
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t off = offs[i];
        if (off + size > cap_bits) continue;  // (never taken)
        bool none = false;
        const int64_t r = MODE == RBX_OVERFLOW_WRAP
                              ? field_apply<false>(w, cap_bits >> 6, op, is_signed, size, off, values[i])
                              : field_apply_ov(w, cap_bits >> 6, op, is_signed, size, MODE, off, values[i], &none);
        if (replies) replies[i] = r;
        if (MODE == RBX_OVERFLOW_FAIL && nil) nil[i] = (uint8_t)none;
    }
    atomicMax(len, (u64)new_len);
}

// ---------------------------------------------------------------------------------
// 6. A list of sub-commands of any operations, types and modes (rbx_bitset_bitfield), one lane, in
// order: fields of different sizes may partly overlap, so the order is total.  GET reads bits at or
// past the allocation as zero (cap_bits = 0 with w = null: a missing key and nothing to write);
// the host sized the bitmap for every SET / INCRBY, failing ones included.
// ---------------------------------------------------------------------------------
__global__ void k_bitfield_serial(u64 *w, u64 *len, uint64_t cap_bits, const rbx_field_cmd *__restrict__ cmds,
                                  uint64_t n, int64_t *__restrict__ replies, uint8_t *__restrict__ nil,
                                  uint64_t new_len) {
    for (uint64_t i = 0; i < n; ++i) {
        const rbx_field_cmd c = cmds[i];
        bool none = false;
        int64_t r = 0;
        if (c.op == RBX_FIELD_GET)
            r = field_extend(field_load(w, cap_bits >> 6, c.offset, c.size), c.size, c.is_signed);
        else if (c.offset + c.size <= cap_bits)  // (always)
            r = field_apply_ov(w, cap_bits >> 6, c.op, c.is_signed, c.size, c.overflow, c.offset, c.value, &none);
        replies[i] = r;
        nil[i] = (uint8_t)none;
    }
    if (new_len) atomicMax(len, (u64)new_len);
}

__global__ void k_field_one(u64 *w, u64 *len, uint64_t cap_bits, int op, uint32_t is_signed, uint32_t size,
                            uint64_t off, int64_t value, int64_t *reply, uint64_t new_len) {
    if (off + size <= cap_bits) *reply = field_apply<false>(w, cap_bits >> 6, op, is_signed, size, off, value);
    atomicMax(len, (u64)new_len);
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_fields_check(const uint64_t *d_offs, const int64_t *d_vals, uint64_t n, int size,
                         unsigned long long *d_out2, hipStream_t st) {
    if (!d_vals) {
        hipLaunchKernelGGL(k_fields_check, dim3(grid_for(n, 512)), dim3(256), 0, st, d_offs, n, (uint32_t)size, d_out2);
        return;
    }
    // 16-byte loads need 16-byte addresses (every allocator gives them; a pointer into an array may not)
    const bool vec = (((uintptr_t)d_offs | (uintptr_t)d_vals) & 15) == 0;
    auto *check = vec ? k_fields_check_signs<true> : k_fields_check_signs<false>;
    hipLaunchKernelGGL(check, dim3(grid_for(vec ? (n + 1) / 2 : n, 512)), dim3(256), 0, st, d_offs, d_vals, n,
                       (uint32_t)size, d_out2);
}

void launch_fields_get(const uint32_t *words, uint64_t cap_bytes, const uint64_t *d_offs, uint64_t n, int size,
                       int is_signed, int64_t *d_out, hipStream_t st) {
    hipLaunchKernelGGL(k_fields_get, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, (const u64 *)words, cap_bytes / 8,
                       d_offs, n, (uint32_t)size, is_signed ? 1u : 0u, d_out);
}

void launch_fields_incr_atomic(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, const uint64_t *d_offs,
                               const int64_t *d_incs, uint64_t n, int size, uint64_t new_len, hipStream_t st) {
    hipLaunchKernelGGL(k_fields_incr_atomic, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, (u64 *)words, len,
                       cap_bytes * 8, d_offs, d_incs, n, (uint32_t)size, new_len);
}

void launch_fields_incr_sat(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, const uint64_t *d_offs,
                            const int64_t *d_incs, uint64_t n, int size, int is_signed, uint64_t new_len,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_fields_incr_sat, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, (u64 *)words, len,
                       cap_bytes * 8, d_offs, d_incs, n, (uint32_t)size, is_signed ? 1u : 0u, new_len);
}

int launch_fields_grouped(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, int op, int is_signed,
                          int size, int mode, const uint64_t *d_offs, const int64_t *d_values, uint32_t n,
                          int64_t *d_replies, uint8_t *d_nil, uint64_t new_len, int slot_bits, void *d_scratch,
                          size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<uint32_t> b;  // the cells are the slots
    int e = cell_sort_carve(d_scratch, scratch_bytes, n, &b);
    if (e) return e;
    hipLaunchKernelGGL(k_fields_slots, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, d_offs, n, (uint32_t)size,
                       b.cell_in, b.pos_in);
    e = cell_sort(b, n, 0, slot_bits, st);  // over the slot's significant bits only
    if (e) return e;
    auto *runs = mode == RBX_OVERFLOW_SAT    ? k_fields_runs<RBX_OVERFLOW_SAT>
                 : mode == RBX_OVERFLOW_FAIL ? k_fields_runs<RBX_OVERFLOW_FAIL>
                                             : k_fields_runs<RBX_OVERFLOW_WRAP>;
    hipLaunchKernelGGL(runs, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, (u64 *)words, len, cap_bytes * 8, op,
                       is_signed ? 1u : 0u, (uint32_t)size, b.cell_out, b.pos_out, n, d_values, d_replies, d_nil, new_len);
    return 0;
}

void launch_fields_serial(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, int op, int is_signed, int size,
                          int mode, const uint64_t *d_offs, const int64_t *d_values, uint64_t n, int64_t *d_replies,
                          uint8_t *d_nil, uint64_t new_len, hipStream_t st) {
    auto *serial = mode == RBX_OVERFLOW_SAT    ? k_fields_serial<RBX_OVERFLOW_SAT>
                   : mode == RBX_OVERFLOW_FAIL ? k_fields_serial<RBX_OVERFLOW_FAIL>
                                               : k_fields_serial<RBX_OVERFLOW_WRAP>;
    hipLaunchKernelGGL(serial, dim3(1), dim3(1), 0, st, (u64 *)words, len, cap_bytes * 8, op, is_signed ? 1u : 0u,
                       (uint32_t)size, d_offs, d_values, n, d_replies, d_nil, new_len);
}

void launch_bitfield_serial(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, const rbx_field_cmd *d_cmds,
                            uint64_t n, int64_t *d_replies, uint8_t *d_nil, uint64_t new_len, hipStream_t st) {
    hipLaunchKernelGGL(k_bitfield_serial, dim3(1), dim3(1), 0, st, (u64 *)words, len, cap_bytes * 8, d_cmds, n,
                       d_replies, d_nil, new_len);
}

void launch_field_one(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, int op, int is_signed, int size,
                      uint64_t offset, int64_t value, int64_t *d_reply, uint64_t new_len, hipStream_t st) {
    hipLaunchKernelGGL(k_field_one, dim3(1), dim3(1), 0, st, (u64 *)words, len, cap_bytes * 8, op, is_signed ? 1u : 0u,
                       (uint32_t)size, offset, value, d_reply, new_len);
}

}  // namespace rbx
