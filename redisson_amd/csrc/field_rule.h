// field_rule.h -- what one BITFIELD sub-command does to one field under OVERFLOW WRAP / SAT / FAIL
// ([redis-7.2] bitops.c bitfieldGeneric, checkSignedBitfieldOverflow, checkUnsignedBitfieldOverflow,
// restated in DESIGN section 11.3), and the check of one sub-command's type and offset.  One function each for the
// kernels (bitfield_kernels.hip, fieldstream_kernels.hip), the host entry points (api_bitset.cpp) and the
// stand-alone sanitizer programs (tests/c/field_rule_test.cpp, tests/c/field_cmd_check_test.cpp): it
// includes <stdint.h> only and compiles without HIP.
#pragma once
#include <stdint.h>

#ifndef RBX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RBX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RBX_HD inline
#endif
#endif

namespace rbx {

// the values of RBX_FIELD_* and RBX_OVERFLOW_* (include/rbx.h), restated so this header stands alone
enum { kFieldGet = 0, kFieldSet = 1, kFieldIncrBy = 2 };
enum { kOverflowWrap = 0, kOverflowSat = 1, kOverflowFail = 2 };

// The checks Redis makes on one sub-command's type and offset, in the order rbx_bitset_bitfield applies
// them: the type first (u64, i65 and size 0 are "ERR Invalid bitfield type"), then the offset limit (the
// whole field lies below bit 2^32: "ERR bit offset is not an integer or out of range").  One rule for the
// single call, the field stream's summary pass and its execution kernels (fieldstream_kernels.hip) and
// the stand-alone program tests/c/field_cmd_check_test.cpp.
enum { kFieldCmdOk = 0, kFieldCmdBadType = 1, kFieldCmdBadOffset = 2 };
RBX_HD int field_cmd_check(int is_signed, int size, uint64_t offset) {
    if (size < 1 || size > (is_signed ? 64 : 63)) return kFieldCmdBadType;
    const uint64_t limit = 1ULL << 32;
    if (offset >= limit || offset + (uint64_t)size > limit) return kFieldCmdBadOffset;
    return kFieldCmdOk;
}

// the low `size` bits of v as a value of the type: sign-extended for i<size>, as they are for u<size>
RBX_HD int64_t field_typed(uint64_t v, int size, int is_signed) {
    if (size < 64) {
        v &= (1ULL << size) - 1;
        if (is_signed && ((v >> (size - 1)) & 1)) v |= ~0ULL << size;
    }
    return (int64_t)v;
}

// One sub-command on a field of type <i|u><size> (signed 1..64, unsigned 1..63) that holds `old`
// (a value of the type).  *now = the field after, *reply = the reply; returns true when the reply
// is nil (FAIL on overflow: *now = old, *reply = 0).  The sums are exact: no step overflows an
// int64_t, whatever old and value are.
RBX_HD bool field_rule(int op, int is_signed, int size, int mode, int64_t old, int64_t value, int64_t *now,
                       int64_t *reply) {
    if (op == kFieldGet) {
        *now = *reply = old;
        return false;
    }
    const int hbits = is_signed ? size - 1 : size;  // 0..63 value bits
    const int64_t hi = hbits == 0 ? 0 : (int64_t)(~0ULL >> (64 - hbits));
    const int64_t lo = is_signed ? -hi - 1 : 0;
    int over = 0;  // +1: the exact result lies above hi, -1: below lo
    uint64_t bits;  // the result modulo 2^size, in the low bits
    if (op == kFieldSet) {
        bits = (uint64_t)value;
        // an unsigned field takes the argument as a uint64_t: a negative one overflows upwards
        if (is_signed)
            over = value > hi ? 1 : (value < lo ? -1 : 0);
        else
            over = (uint64_t)value > (uint64_t)hi ? 1 : 0;
    } else {
        bits = (uint64_t)old + (uint64_t)value;
        int64_t sum;
        if (__builtin_add_overflow(old, value, &sum))
            over = value > 0 ? 1 : -1;
        else
            over = sum > hi ? 1 : (sum < lo ? -1 : 0);
    }
    int64_t t = field_typed(bits, size, is_signed);  // exact when over == 0, else WRAP's answer
    if (over != 0 && mode == kOverflowFail) {
        *now = old;
        *reply = 0;
        return true;
    }
    if (over != 0 && mode == kOverflowSat) t = over > 0 ? hi : lo;
    *now = t;
    *reply = op == kFieldSet ? old : t;
    return false;
}

}  // namespace rbx
