// range_cmd_test.cpp -- redisson_amd/csrc/range_cmd.h as a stand-alone host program (no HIP), built with ASan +
// UBSan (Makefile target range_cmd_asan, tests/test_range_cmd_sanitized.py).  Every command the rule set can be
// given at the boundary lengths, with starts and ends around 0, around the string's ends and at the ends of
// int64_t, is run through the rule -- the caller-error test, the fails-alone test, the plan, a scan of the planned
// interval, the final reply -- and compared with a restatement that works bit by bit on wide integers: positions
// are __int128, so the restatement cannot overflow where the rule under test might.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../redisson_amd/csrc/range_cmd.h"

using namespace rbx;
typedef __int128 wide;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failed <= 20) {                       \
                std::printf("FAILED %s: ", #cond);        \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static int bit_at(const std::vector<uint8_t> &s, wide p) { return (s[(size_t)(p >> 3)] >> (7 - (int)(p & 7))) & 1; }

// the restatement: 0 = ran with *reply, else the failure kind; data: the string (empty with missing = no key)
static int restated(const std::vector<uint8_t> &s, bool missing, const rbx_range_cmd &c, int64_t *reply) {
    *reply = 0;
    if (c.op == RBX_RANGE_POS && c.bit > 1) return kRangeBadBit;
    if (c.op == RBX_RANGE_POS && c.nargs < 2 && c.unit == RBX_RANGE_BIT) return kRangeSyntax;
    const wide len = (wide)s.size();
    if (c.op == RBX_RANGE_STRLEN) return *reply = (int64_t)len, 0;
    if (c.op == RBX_RANGE_LENGTH) {
        // the script: the first set bit of the last byte, then downwards from the byte's end; else bit 0, else GETBIT -1
        if (len && s.back()) {
            for (int j = 7; j >= 0; --j)
                if ((s.back() >> (7 - j)) & 1) return *reply = (int64_t)((len - 1) * 8 + j + 1), 0;
        }
        if (len && (s[0] & 0x80)) return *reply = 1, 0;
        return kRangeScript;
    }
    const bool pos = c.op == RBX_RANGE_POS;
    if (missing) return *reply = pos && c.bit ? -1 : 0, 0;
    const bool end_given = c.nargs == 2;
    wide start = c.nargs >= 1 ? (wide)c.start : 0, end = end_given ? (wide)c.end : len - 1;
    const int unit = c.nargs == 2 ? c.unit : RBX_RANGE_BYTE;
    if (!pos && c.nargs == 0) start = 0, end = len - 1;
    if (!pos && c.nargs == 2 && start < 0 && end < 0 && start > end) return 0;
    const wide t = unit ? len * 8 : len;
    if (start < 0) start += t;
    if (end < 0) end += t;
    if (start < 0) start = 0;
    if (end < 0) end = 0;
    if (end > t - 1) end = t - 1;
    if (start > end) return *reply = pos ? -1 : 0, 0;
    const wide lo = unit ? start : start * 8, hi = unit ? end : end * 8 + 7;
    int64_t ones = 0;
    for (wide p = lo; p <= hi; ++p) {
        const int b = bit_at(s, p);
        ones += b;
        if (pos && b == c.bit) return *reply = (int64_t)p, 0;
    }
    if (pos) *reply = (c.bit || end_given) ? -1 : (int64_t)(hi + 1);
    else *reply = ones;
    return 0;
}

// the rule under test, driven as rbx_bitset_range_of and the kernels drive it
static int ruled(const std::vector<uint8_t> &s, bool missing, const rbx_range_cmd &c, int64_t *reply) {
    *reply = 0;
    if (const int kind = range_cmd_fails(c)) return kind;
    const uint64_t len = s.size();
    if (c.op == RBX_RANGE_LENGTH) return bitset_length_rule(len, len ? s[0] : 0, len ? s[len - 1] : 0, reply) ? 0 : kRangeScript;
    uint64_t lo = 0, hi = 0;
    if (!range_cmd_plan(c, len, missing, &lo, &hi, reply)) return 0;
    CHECK(lo <= hi && hi < len * 8, "interval [%llu, %llu] of %llu bytes", (unsigned long long)lo, (unsigned long long)hi,
          (unsigned long long)len);
    uint64_t ones = 0, found = kBitsNone;
    for (uint64_t p = lo; p <= hi && found == kBitsNone; ++p) {
        const int b = bit_at(s, p);
        ones += b;
        if (c.op == RBX_RANGE_POS && b == c.bit) found = p;
    }
    *reply = c.op == RBX_RANGE_POS ? range_cmd_pos_reply(c, found, hi) : (int64_t)ones;
    return 0;
}

int main() {
    static_assert(sizeof(rbx_range_cmd) == 24, "the ABI's record");
    const size_t lengths[] = {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097};
    uint64_t seed = 0x9E3779B97F4A7C15ULL, checked = 0;
    auto next = [&seed]() {
        seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
        return seed;
    };
    for (size_t len : lengths) {
        for (int pattern = 0; pattern < 4; ++pattern) {
            std::vector<uint8_t> s(len);
            for (auto &b : s) b = pattern == 0 ? 0 : pattern == 1 ? 0xFF : (uint8_t)next();
            if (pattern == 3 && len) s[0] |= 0x80, s[len - 1] = 0;  // length()'s odd path
            const int64_t T = (int64_t)len * 8;
            std::vector<int64_t> bounds = {INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, -(1LL << 40), 1LL << 40};
            for (int64_t d = -2; d <= 2; ++d)
                for (int64_t base : {(int64_t)0, (int64_t)len, -(int64_t)len, T, -T, T / 2})
                    bounds.push_back(base + d);
            for (int missing = 0; missing < (len ? 1 : 2); ++missing)
                for (uint8_t op = 0; op < 4; ++op)
                    for (uint8_t nargs = 0; nargs < 3; ++nargs)
                        for (uint8_t unit = 0; unit < 2; ++unit)
                            for (uint8_t bit : {0, 1, 2, 255})
                                for (int64_t start : bounds)
                                    for (int64_t end : bounds) {
                                        if (op != RBX_RANGE_POS && bit > 0) continue;
                                        if ((op >= RBX_RANGE_STRLEN || nargs == 0) && (start != bounds[0] || end != bounds[0])) continue;
                                        rbx_range_cmd c = {start, end, op, bit, nargs, unit, {0, 0, 0, 0}};
                                        const bool illegal = op == RBX_RANGE_COUNT && nargs == 1;
                                        CHECK(range_cmd_illegal(c) == illegal, "op %d nargs %d", op, nargs);
                                        if (illegal) continue;
                                        int64_t want, got;
                                        const int kw = restated(s, missing != 0, c, &want), kg = ruled(s, missing != 0, c, &got);
                                        CHECK(kw == kg && want == got,
                                              "len %zu pattern %d missing %d op %d bit %d nargs %d unit %d start %lld end %lld: "
                                              "kind %d reply %lld, restated kind %d reply %lld",
                                              len, pattern, missing, op, bit, nargs, unit, (long long)start, (long long)end, kg,
                                              (long long)got, kw, (long long)want);
                                        ++checked;
                                    }
        }
    }
    // the caller's errors
    for (int op = 0; op < 256; ++op)
        for (int unit = 0; unit < 4; ++unit)
            for (int nargs = 0; nargs < 5; ++nargs) {
                rbx_range_cmd c = {0, 0, (uint8_t)op, 1, (uint8_t)nargs, (uint8_t)unit, {0, 0, 0, 0}};
                CHECK(range_cmd_illegal(c) == (op > 3 || unit > 1 || nargs > 2 || (op == 0 && nargs == 1)), "op %d", op);
            }
    if (g_failed) {
        std::printf("range_cmd_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("range_cmd_test: ok (%llu commands)\n", (unsigned long long)checked);
    return 0;
}
