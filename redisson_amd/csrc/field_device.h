// field_device.h -- a BITFIELD field as the kernels address it (bitfield_kernels.hip, fieldstream_kernels.hip).
//
// The bitmap is addressed as aligned 64-bit words.  A word's bytes are the string's bytes in order, so the
// byte-swapped word holds string bit 64q + j at position 63 - j: a field is a run of adjacent bits of at
// most two byte-swapped words, and integer arithmetic on that run is arithmetic on the field.  The
// allocation is a multiple of 256 bytes, so an aligned word lies inside it or wholly past it.
// Device code only; include after <hip/hip_runtime.h> and field_rule.h.
#pragma once
#include <stdint.h>

#include "field_rule.h"

namespace rbx {

__device__ __forceinline__ unsigned long long field_mask(uint32_t size) {
    return size >= 64 ? ~0ULL : (1ULL << size) - 1;
}

// the reply form of a field's bits: sign-extended for i<size>, as they are for u<size>
__device__ __forceinline__ int64_t field_extend(unsigned long long v, uint32_t size, uint32_t is_signed) {
    if (is_signed && size < 64 && ((v >> (size - 1)) & 1)) v |= ~0ULL << size;
    return (int64_t)v;
}

// word q of the string in big-endian bit order; zero at or past the allocation
__device__ __forceinline__ unsigned long long ld_be(const unsigned long long *w, uint64_t q, uint64_t cap_words) {
    return q < cap_words ? __builtin_bswap64(w[q]) : 0ULL;
}

// the field's bits, zero-extended
__device__ __forceinline__ unsigned long long field_load(const unsigned long long *w, uint64_t cap_words, uint64_t off,
                                                         uint32_t size) {
    const uint64_t q = off >> 6;
    const uint32_t sh = (uint32_t)(off & 63);
    unsigned long long hi = ld_be(w, q, cap_words) << sh;
    if (sh + size > 64) hi |= ld_be(w, q + 1, cap_words) >> (64 - sh);  // sh >= 1 here
    return hi >> (64 - size);
}

// field := v (already below 2^size), the field inside the allocation.  ATOMIC: other lanes write
// other fields of the same words at the same time, so the bits go out as atomicAnd + atomicOr.
template <bool ATOMIC>
__device__ __forceinline__ void word_put(unsigned long long *p, unsigned long long m, unsigned long long bits) {
    if (ATOMIC) {
        atomicAnd(p, __builtin_bswap64(~m));
        atomicOr(p, __builtin_bswap64(bits));
    } else {
        *p = __builtin_bswap64((__builtin_bswap64(*p) & ~m) | bits);
    }
}

template <bool ATOMIC>
__device__ __forceinline__ void field_store(unsigned long long *w, uint64_t off, uint32_t size, unsigned long long v) {
    const uint64_t q = off >> 6;
    const uint32_t sh = (uint32_t)(off & 63);
    const unsigned long long m = field_mask(size) << (64 - size), top = v << (64 - size);  // the field at a word's top
    word_put<ATOMIC>(w + q, m >> sh, top >> sh);
    if (sh + size > 64) word_put<ATOMIC>(w + q + 1, m << (64 - sh), top << (64 - sh));
}

// one sub-command under an overflow mode (field_rule) on the field at `off`: the reply, the field updated
// in place; *nil = the reply is nil and the field untouched
__device__ __forceinline__ int64_t field_apply_ov(unsigned long long *w, uint64_t cap_words, int op, uint32_t is_signed,
                                                  uint32_t size, int mode, uint64_t off, int64_t value, bool *nil) {
    const int64_t old = field_extend(field_load(w, cap_words, off, size), size, is_signed);
    int64_t now, reply;
    *nil = field_rule(op, (int)is_signed, (int)size, mode, old, value, &now, &reply);
    if (op != kFieldGet && !*nil) field_store<false>(w, off, size, (unsigned long long)now & field_mask(size));
    return reply;
}

}  // namespace rbx
