// range_cmd.h -- the read queries on one bit string as one rule set: the range rules of BITCOUNT / BITPOS
// ([redis-7.2] bitops.c bitcountCommand / bitposCommand, restated in DESIGN section 11.2), RBitSet.length()'s
// script over (length, first byte, last byte), and what one command of rbx_bitset_range_stream (DESIGN
// section 11.10) is from the command alone and from (command, length, missing).  One function each for the
// kernels (bitrange_kernels.hip, rangestream_kernels.hip), the host entry points (api_bitset_multi.cpp,
// keyspace.cpp) and the stand-alone sanitizer program tests/c/range_cmd_test.cpp: it includes <stdint.h>
// and the C ABI header only and compiles without HIP.  No step overflows an int64_t, whatever start and end are.
#pragma once
#include <stdint.h>

#include "../../include/rbx.h"

#ifndef RBX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RBX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RBX_HD inline
#endif
#endif

namespace rbx {

// ---- the range rules (unit: RBX_RANGE_BYTE or RBX_RANGE_BIT; a string has at most 2^29 bytes) ----
constexpr unsigned long long kBitsNone = 1ULL << 40;  // "no such bit": above every bit position
// Normalise(start, end) over a string of len bytes: the bit interval [*lo, *hi], or false = empty
RBX_HD bool bits_normalise(int64_t start, int64_t end, int unit, uint64_t len, uint64_t *lo, uint64_t *hi) {
    const int64_t t = (int64_t)(unit ? len * 8 : len);
    if (start < 0) start += t;
    if (end < 0) end += t;
    if (start < 0) start = 0;
    if (end < 0) end = 0;
    if (end > t - 1) end = t - 1;
    if (start > end) return false;
    *lo = unit ? (uint64_t)start : (uint64_t)start * 8;
    *hi = unit ? (uint64_t)end : (uint64_t)end * 8 + 7;
    return true;
}
// BITCOUNT's interval: "start < 0 && end < 0 && start > end" answers 0 before anything is normalised
RBX_HD bool bits_count_interval(int64_t start, int64_t end, int unit, uint64_t len, uint64_t *lo, uint64_t *hi) {
    if (start < 0 && end < 0 && start > end) return false;
    return bits_normalise(start, end, unit, len, lo, hi);
}
// BITPOS's reply over a non-empty interval ending at hi; found >= kBitsNone = no position holds the bit: -1,
// but hi + 1 for a clear bit when no end was given (the string counts as zero-padded on the right)
RBX_HD int64_t bits_pos_reply(uint64_t found, int bit, bool end_given, uint64_t hi) {
    if (found < kBitsNone) return (int64_t)found;
    return (bit || end_given) ? -1 : (int64_t)hi + 1;
}
// the bytes a query's clamped interval covers (0 = empty): the batch's work summary adds them up
RBX_HD uint64_t bits_interval_bytes(int64_t start, int64_t end, int unit, uint64_t len, bool pos) {
    uint64_t lo, hi;
    const bool any = pos ? bits_normalise(start, end, unit, len, &lo, &hi) : bits_count_interval(start, end, unit, len, &lo, &hi);
    return any ? (hi >> 3) - (lo >> 3) + 1 : 0;
}

// ---- RBitSet.length(): the script's rule (keyspace.cpp has the derivation) over the string's length and its
// first and last byte.  false = the script fails (GETBIT key -1).
RBX_HD bool bitset_length_rule(uint64_t len, uint8_t first, uint8_t last, int64_t *out) {
    if (len && last) {
        int low = 0;  // lowest set bit of the byte = the highest MSB-first index
        while (!((last >> low) & 1)) ++low;
        *out = (int64_t)((len - 1) * 8 + (uint64_t)(7 - low) + 1);
        return true;
    }
    if (len && (first & 0x80)) {
        *out = 1;
        return true;
    }
    *out = 0;
    return false;
}

// ---- one command of rbx_bitset_range_stream ----
// the caller's errors: the whole call is refused
RBX_HD bool range_cmd_illegal(const rbx_range_cmd &c) {
    return c.op > RBX_RANGE_LENGTH || c.unit > RBX_RANGE_BIT || c.nargs > 2 || (c.op == RBX_RANGE_COUNT && c.nargs == 1);
}

// Why a legal command fails alone, in the order the single calls look: BITPOS's bit, BITPOS's unit without an
// end; then the key's type, which the caller knows; then LENGTH's script, which depends on the data.
enum { kRangeOk = 0, kRangeBadBit = 1, kRangeSyntax = 2, kRangeWrongType = 3, kRangeScript = 4, kRangeKinds = 4 };
RBX_HD int range_cmd_fails(const rbx_range_cmd &c) {
    if (c.op != RBX_RANGE_POS) return kRangeOk;
    if (c.bit > 1) return kRangeBadBit;
    if (c.nargs < 2 && c.unit == RBX_RANGE_BIT) return kRangeSyntax;  // a unit needs an end
    return kRangeOk;
}

// A COUNT, POS or STRLEN command that does not fail, over a string of len bytes (missing: no such key, len = 0).
// true = the bits [*lo, *hi] are to be scanned (lo <= hi < 8 * len); false = *fixed is the reply.
RBX_HD bool range_cmd_plan(const rbx_range_cmd &c, uint64_t len, bool missing, uint64_t *lo, uint64_t *hi,
                           int64_t *fixed) {
    if (c.op == RBX_RANGE_STRLEN) {
        *fixed = (int64_t)len;
        return false;
    }
    if (c.op == RBX_RANGE_COUNT) {
        *fixed = 0;  // a missing key, an empty string, an empty range
        if (missing || len == 0) return false;
        if (c.nargs == 0) {
            *lo = 0;
            *hi = len * 8 - 1;
            return true;
        }
        return bits_count_interval(c.start, c.end, c.unit, len, lo, hi);
    }
    if (missing) {
        *fixed = c.bit ? -1 : 0;
        return false;
    }
    *fixed = -1;  // an empty range: every query on an existing empty string
    return bits_normalise(c.nargs >= 1 ? c.start : 0, c.nargs == 2 ? c.end : (int64_t)len - 1, c.unit, len, lo, hi);
}

// POS's reply from the first position found in the planned interval (>= kBitsNone: none)
RBX_HD int64_t range_cmd_pos_reply(const rbx_range_cmd &c, uint64_t found, uint64_t hi) {
    return bits_pos_reply(found, c.bit, c.nargs == 2, hi);
}

}  // namespace rbx
