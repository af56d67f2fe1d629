// byte_cmd.h -- the byte-level commands on one Redis string as one rule set: GETRANGE, SETRANGE, APPEND and GET
// ([redis-7.2, external] t_string.c getrangeCommand / setrangeCommand / appendCommand / getCommand, restated in
// DESIGN section 11.12), and what one command of rbx_string_stream is from (running length, missing, command).
// One function each for the kernels (bytestream_kernels.hip), the host entry points (api_bitset.cpp,
// api_bitset_multi.cpp), rbx_string_range_of and the stand-alone sanitizer program tests/c/byte_cmd_test.cpp: it
// includes <stdint.h> and the C ABI header only and compiles without HIP.  No step overflows an int64_t, whatever
// the arguments are.
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

// a string has at most 2^29 bytes: proto-max-bulk-len, and the engine's 2^32-bit cap
constexpr uint64_t kStrMax = 1ULL << 29;

// GETRANGE key start end over a string of len <= kStrMax bytes (a missing key: len 0): the bytes [*lo, *hi), or
// false = the empty reply.  start and end are any int64_t: a negative one has len added, which cannot overflow.
RBX_HD bool byte_getrange(int64_t start, int64_t end, uint64_t len, uint64_t *lo, uint64_t *hi) {
    const int64_t t = (int64_t)len;
    if (start < 0 && end < 0 && start > end) return false;
    if (start < 0) start += t;
    if (end < 0) end += t;
    if (start < 0) start = 0;
    if (end < 0) end = 0;
    if (end >= t) end = t - 1;
    if (t == 0 || start > end) return false;
    *lo = (uint64_t)start;
    *hi = (uint64_t)end + 1;
    return true;
}

// ---- one command of rbx_string_stream ----
// the caller's errors: the whole call is refused.  vals_len: the bytes of the call's value buffer.
RBX_HD bool byte_cmd_illegal(const rbx_string_cmd &c, uint64_t vals_len) {
    if (c.op > RBX_STR_GET) return true;
    if (c.op != RBX_STR_SETRANGE && c.op != RBX_STR_APPEND) return false;
    return c.val_off > vals_len || c.val_len > vals_len - c.val_off;
}

// Why a legal command fails alone, in the order the single calls look: SETRANGE's offset before the key is looked
// at; then the key's type; then the size, which depends on the running length.
enum { kByteOk = 0, kByteBadOffset = 1, kByteWrongType = 2, kByteTooBig = 3, kByteKinds = 3 };

struct ByteStep {
    int fails;         // kByte*; a failed command leaves the running state as it was
    int64_t reply;     // the new length of a write, the byte count of a read
    uint64_t at, cnt;  // the bytes moved: a read's [at, at + cnt) of the string, a write's value at [at, at + cnt)
    uint64_t len;      // the running length behind the command
    bool exists;       // the key exists behind the command
    bool writes;       // the command stores (or creates): its key is to be there with `len` bytes
    bool nil;          // GET on a missing key
};

// The run step on a key that holds a string or is missing: running_len bytes (0 when missing) before the command.
RBX_HD ByteStep byte_run_step(uint64_t running_len, bool missing, const rbx_string_cmd &c) {
    ByteStep s = {kByteOk, 0, 0, 0, running_len, !missing, false, false};
    const uint64_t v = c.val_len;
    if (c.op == RBX_STR_GETRANGE || c.op == RBX_STR_GET) {
        uint64_t lo, hi;
        const bool whole = c.op == RBX_STR_GET;
        s.nil = whole && missing;
        if (byte_getrange(whole ? 0 : c.a, whole ? -1 : c.b, running_len, &lo, &hi)) {
            s.at = lo;
            s.cnt = hi - lo;
            s.reply = (int64_t)s.cnt;
        }
        return s;
    }
    if (c.op == RBX_STR_SETRANGE) {
        if (c.a < 0) {
            s.fails = kByteBadOffset;
            return s;
        }
        s.reply = (int64_t)running_len;
        if (v == 0) return s;  // nothing is created, and there is no size check
        if ((uint64_t)c.a + v > kStrMax) {  // (at most 2^63 + 2^32: no wrap)
            s.fails = kByteTooBig;
            s.reply = 0;
            return s;
        }
        s.at = (uint64_t)c.a;
    } else {  // APPEND: a missing key is created holding the value, an empty one included
        if (running_len + v > kStrMax) {  // (a value above the limit cannot reach a missing key either)
            s.fails = kByteTooBig;
            return s;
        }
        s.at = running_len;
    }
    s.cnt = v;
    s.len = s.at + v > running_len ? s.at + v : running_len;
    s.reply = (int64_t)s.len;
    s.exists = s.writes = true;
    return s;
}

// The same on any key: wrong = the key holds another type.
RBX_HD ByteStep byte_key_step(uint64_t running_len, bool missing, bool wrong, const rbx_string_cmd &c) {
    if (wrong && !(c.op == RBX_STR_SETRANGE && c.a < 0)) {
        ByteStep s = {kByteWrongType, 0, 0, 0, running_len, !missing, false, false};
        return s;
    }
    return byte_run_step(running_len, missing, c);
}

constexpr uint8_t kByteStatusNil = 1, kByteStatusFailed = 0xFF;
RBX_HD uint8_t byte_step_status(const ByteStep &s) { return s.fails ? kByteStatusFailed : (s.nil ? kByteStatusNil : 0); }

}  // namespace rbx
