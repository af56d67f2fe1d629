// members_rule.h -- the rules of set-bit enumeration (rbx_bitset_members*) and of the java.util.BitSet exchange
// (rbx_bitset_as_words / rbx_bitset_set_words; M/RedissonBitSet.java:391-420 fromByteArrayReverse /
// toByteArrayReverse), DESIGN section 11.11.  One function each for the kernels (members_kernels.hip), the host
// entry points (api_bitset.cpp, api_bitset_multi.cpp) and the stand-alone sanitizer program tests/c/members_rule_test.cpp: like
// range_cmd.h, whose interval rule it takes, it includes <stdint.h> and the C ABI header only and compiles
// without HIP.  No step wraps a uint64_t, whatever skip, limit and cap are.
#pragma once
#include <stdint.h>

#include "range_cmd.h"

namespace rbx {

// ---- which bits ----
// the caller's errors of one command: the whole call is refused
RBX_HD bool members_cmd_illegal(int nargs, int unit) {
    return (nargs != 0 && nargs != 2) || (unit != RBX_RANGE_BYTE && unit != RBX_RANGE_BIT);
}
// The bit interval [*lo, *hi] whose ones a legal command enumerates over a string of len bytes (lo <= hi < 8 * len),
// or false = none (a missing key, an empty string, an empty range).  nargs 0: the whole string; nargs 2: BITCOUNT's
// interval, its "both negative and start > end" pre-check included.
RBX_HD bool members_interval(int nargs, int64_t start, int64_t end, int unit, uint64_t len, uint64_t *lo, uint64_t *hi) {
    if (len == 0) return false;
    if (nargs == 0) {
        *lo = 0;
        *hi = len * 8 - 1;
        return true;
    }
    return bits_count_interval(start, end, unit, len, lo, hi);
}
// The page of an interval that holds `total` ones: the ranks [*first, *first + *count) are written.  skip past
// the end gives an empty page at rank `total`; a + b is never formed for a, b near 2^64.
RBX_HD void members_page(uint64_t total, uint64_t skip, uint64_t limit, uint64_t cap, uint64_t *first, uint64_t *count) {
    const uint64_t f = skip < total ? skip : total, left = total - f, m = limit < cap ? limit : cap;
    *first = f;
    *count = m < left ? m : left;
}

// ---- one vector: the k-th one ----
// the position (0..31) of the k-th set bit of r counted from bit 0, k < popcount(r)
RBX_HD uint32_t word_select(uint32_t r, uint32_t k) {
    uint32_t pos = 0;
    for (uint32_t s = 16; s; s >>= 1) {  // the bit sought is the k-th set one of r's bits [pos, pos + 2 s)
        const uint32_t c = (uint32_t)__builtin_popcount((r >> pos) & ((1u << s) - 1u));
        if (k >= c) {
            k -= c;
            pos += s;
        }
    }
    return pos;
}
// reverses the bits of each byte of x
RBX_HD uint32_t rev_bytes(uint32_t x) {
    x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
}
// reverses all 32 bits (host and device alike; the device compiler turns it into its one instruction)
RBX_HD uint32_t rev_word(uint32_t x) {
    x = rev_bytes(x);
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
// The string position (0..127) of the k-th one, in string order, of a vector given as four byte-swapped words
// (bitrange_device.h: word j holds positions 32 j .. 32 j + 31, position p at bit 31 - p), k < their popcount.
RBX_HD uint32_t vec_select(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t k) {
    uint32_t base = 0, w = w0, c = (uint32_t)__builtin_popcount(w0);
    if (k >= c) {
        k -= c, base = 32, w = w1, c = (uint32_t)__builtin_popcount(w1);
        if (k >= c) {
            k -= c, base = 64, w = w2, c = (uint32_t)__builtin_popcount(w2);
            if (k >= c) k -= c, base = 96, w = w3;
        }
    }
    return base + word_select(rev_word(w), k);
}

// ---- java.util.BitSet's words <-> the string ----
// A BitSet is long[] words, bit j of word w = bit 64 w + j; the string holds bit i in byte i >> 3 under the mask
// 0x80 >> (i & 7).  So byte k of a word's little-endian image is string byte 8 w + k with its bits reversed, and a
// 32-bit little-endian load of the string maps to the word's half by rev_bytes, in both directions.
// asBitSet(): the words in use of a string whose last non-zero 64-bit word is word `last` (any = it has one)
RBX_HD uint64_t words_in_use(bool any, uint64_t last) { return any ? last + 1 : 0; }
// set(BitSet): Java's int length() is the highest set bit + 1 and overflows at bit 2^31 - 1
RBX_HD bool words_bit_illegal(uint64_t highest) { return highest >= 0x7FFFFFFFull; }
// set(BitSet): toByteArrayReverse's array is length() / 8 + 1 bytes -- one zero byte for the empty BitSet, two
// bytes for a highest bit of 7
RBX_HD uint64_t words_string_len(bool any, uint64_t highest) { return any ? (highest + 1) / 8 + 1 : 1; }
// the highest set bit of word w (non-zero) at index i
RBX_HD uint64_t words_highest(uint64_t i, uint64_t w) { return i * 64 + (63 - (uint64_t)__builtin_clzll(w)); }

}  // namespace rbx
