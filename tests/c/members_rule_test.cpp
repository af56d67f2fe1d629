// members_rule_test.cpp -- redisson_amd/csrc/members_rule.h as a stand-alone host program under ASan + UBSan
// (csrc/Makefile members_rule_asan; tests/test_members_rule_sanitized.py).  The header compiles without HIP; the
// interval, the page, the k-th one of a vector and the BitSet length rule equal bit-by-bit restatements at the boundary
// lengths with extreme start, end, skip, limit and cap, and no step wraps or overflows.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../redisson_amd/csrc/members_rule.h"

using namespace rbx;

static int g_fail = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            if (++g_fail < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                              \
    } while (0)

typedef unsigned __int128 u128;

// the interval from first principles, in 128-bit arithmetic
static bool ref_interval(int nargs, int64_t start, int64_t end, int unit, uint64_t len, uint64_t *lo, uint64_t *hi) {
    if (len == 0) return false;
    if (nargs == 0) {
        *lo = 0, *hi = len * 8 - 1;
        return true;
    }
    if (start < 0 && end < 0 && start > end) return false;
    const __int128 t = unit ? (__int128)len * 8 : (__int128)len;
    __int128 s = start, e = end;
    if (s < 0) s += t;
    if (e < 0) e += t;
    if (s < 0) s = 0;
    if (e < 0) e = 0;
    if (e > t - 1) e = t - 1;
    if (s > e) return false;
    *lo = (uint64_t)(unit ? s : s * 8);
    *hi = (uint64_t)(unit ? e : e * 8 + 7);
    return true;
}

static void test_intervals() {
    const uint64_t lens[] = {0, 1, 2, 15, 16, 17, 4095, 4096, 4097, (1ULL << 29) - 1, 1ULL << 29};
    const int64_t ext[] = {INT64_MIN, INT64_MIN + 1, -(1LL << 62), -(1LL << 32) - 1, -4097, -17, -9, -8, -2, -1, 0, 1, 7, 8,
                           9, 16, 4095, 4096, (1LL << 32) - 1, 1LL << 32, (1LL << 32) + 1, 1LL << 62, INT64_MAX - 1, INT64_MAX};
    for (uint64_t len : lens)
        for (int nargs : {0, 2})
            for (int unit : {0, 1})
                for (int64_t s : ext)
                    for (int64_t e : ext) {
                        uint64_t lo = 1, hi = 2, rlo = 3, rhi = 4;
                        const bool a = members_interval(nargs, s, e, unit, len, &lo, &hi);
                        const bool b = ref_interval(nargs, s, e, unit, len, &rlo, &rhi);
                        CHECK(a == b);
                        if (a && b) CHECK(lo == rlo && hi == rhi && lo <= hi && hi < len * 8);
                    }
    CHECK(!members_cmd_illegal(0, 0) && !members_cmd_illegal(2, 1) && !members_cmd_illegal(0, 1));
    CHECK(members_cmd_illegal(1, 0) && members_cmd_illegal(3, 0) && members_cmd_illegal(2, 2) && members_cmd_illegal(255, 0) &&
          members_cmd_illegal(0, 255) && members_cmd_illegal(-1, 0));
}

static void test_pages() {
    const uint64_t v[] = {0, 1, 2, 63, 64, 65, 32767, 32768, (1ULL << 32) - 1, 1ULL << 32, (1ULL << 63) - 1, 1ULL << 63,
                          UINT64_MAX - 1, UINT64_MAX};
    for (uint64_t total : v) {
        if (total > (1ULL << 32)) continue;  // a string has at most 2^32 bits
        for (uint64_t skip : v)
            for (uint64_t limit : v)
                for (uint64_t cap : v) {
                    uint64_t first = 7, count = 7;
                    members_page(total, skip, limit, cap, &first, &count);
                    const u128 lo = (u128)skip < total ? skip : total;
                    u128 hi = (u128)skip + (limit < cap ? limit : cap);  // skip + limit past 2^64 must not wrap
                    if (hi > total) hi = total;
                    if (hi < lo) hi = lo;
                    CHECK(first == (uint64_t)lo && count == (uint64_t)(hi - lo));
                    CHECK(first <= total && count <= total - first);
                }
    }
}

static void test_select() {
    // every word with up to three set bits, and random ones: the k-th set bit from bit 0, then a vector's k-th one in
    // string order (position p of word j at bit 31 - p)
    uint64_t x = 0x9E3779B97F4A7C15ull;
    std::vector<uint32_t> words = {1u, 0x80000000u, 0xFFFFFFFFu, 0x80000001u, 0x00010000u, 0x0000FFFFu, 0xFFFF0000u, 0x55555555u,
                                   0xAAAAAAAAu};
    for (int i = 0; i < 200; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        words.push_back((uint32_t)x);
        words.push_back((uint32_t)x & (uint32_t)(x >> 32));
    }
    for (uint32_t w : words) {
        uint32_t k = 0;
        for (uint32_t p = 0; p < 32; ++p)
            if ((w >> p) & 1) CHECK(word_select(w, k++) == p);
        uint32_t r = 0;
        for (int p = 0; p < 32; ++p) r |= ((w >> p) & 1u) << (31 - p);
        CHECK(rev_word(w) == r);
        uint32_t rb = 0;
        for (int p = 0; p < 32; ++p) rb |= ((w >> p) & 1u) << ((p & ~7) | (7 - (p & 7)));
        CHECK(rev_bytes(w) == rb);
    }
    for (size_t i = 0; i + 4 <= words.size(); ++i) {
        const uint32_t q[4] = {words[i], i % 3 ? words[i + 1] : 0u, i % 5 ? words[i + 2] : 0u, words[i + 3]};
        uint32_t k = 0;
        for (uint32_t p = 0; p < 128; ++p)
            if ((q[p >> 5] >> (31 - (p & 31))) & 1) CHECK(vec_select(q[0], q[1], q[2], q[3], k++) == p);
    }
}

static void test_words() {
    CHECK(words_in_use(false, 0) == 0 && words_in_use(true, 0) == 1 && words_in_use(true, (1ULL << 26) - 1) == 1ULL << 26);
    CHECK(words_string_len(false, 0) == 1);  // the empty BitSet stores one zero byte
    const uint64_t bits[] = {0, 6, 7, 8, 14, 15, 16, 62, 63, 64, 0x7FFFFFFDull, 0x7FFFFFFEull};
    for (uint64_t b : bits) {
        CHECK(words_string_len(true, b) == (b + 1) / 8 + 1);
        CHECK(!words_bit_illegal(b));
        CHECK(words_highest(b / 64, 1ULL << (b % 64)) == b);
        CHECK(words_highest(b / 64, (1ULL << (b % 64)) | 1ULL) == b);
    }
    CHECK(words_string_len(true, 7) == 2 && words_string_len(true, 6) == 1 && words_string_len(true, 0x7FFFFFFEull) == 1ULL << 28);
    CHECK(words_bit_illegal(0x7FFFFFFFull) && words_bit_illegal(1ULL << 32) && words_bit_illegal(UINT64_MAX));
    CHECK(words_highest((1ULL << 58) - 1, 1ULL << 63) == UINT64_MAX);
}

int main() {
    test_intervals();
    test_pages();
    test_select();
    test_words();
    if (g_fail) {
        printf("members_rule_test: %d FAILED\n", g_fail);
        return 1;
    }
    printf("members_rule_test: ok\n");
    return 0;
}
