// byte_cmd_test.cpp -- redisson_amd/csrc/byte_cmd.h as a stand-alone host program (no HIP), built with ASan + UBSan
// (Makefile target byte_cmd_asan, tests/test_byte_cmd_sanitized.py).  Every sequence of up to 4 commands drawn from a
// small alphabet -- ranges and offsets around 0, around the string's ends, around the 2^29 limit and at the ends of
// int64_t -- runs from each of a few starting strings through byte_run_step, whose reads and writes are applied to an
// array, and is compared step by step with a plain restatement of the commands that works on an array of its own
// in __int128 arithmetic, so it cannot overflow where the rule under test might.  A string too long to keep (beyond
// 64 bytes: the ones near the limit) is followed by its length alone.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../redisson_amd/csrc/byte_cmd.h"

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

static const wide kMax = (wide)1 << 29;
static const size_t kKeep = 64;  // strings up to here are kept byte by byte

struct Str {
    bool exists = false;
    wide len = 0;
    bool kept = true;  // bytes holds the content
    std::vector<uint8_t> bytes;
    void resize(wide n) {
        len = n;
        if (kept && n <= (wide)kKeep) bytes.resize((size_t)n, 0);
        else kept = false, bytes.clear();
    }
};

static uint8_t value_byte(int step, wide j) { return (uint8_t)(0xA0 + 16 * step + (int)(j & 15)); }

// the restatement: 0 = ran, else the failure kind.  *reply as the stream's; read = the reply's bytes when kept.
static int restated(Str &s, const rbx_string_cmd &c, int step, int64_t *reply, bool *nil, std::vector<uint8_t> *read,
                    bool *read_known) {
    *reply = 0;
    *nil = false;
    read->clear();
    *read_known = true;
    const wide v = c.val_len;
    if (c.op == RBX_STR_GET || c.op == RBX_STR_GETRANGE) {
        if (c.op == RBX_STR_GET && !s.exists) return *nil = true, 0;
        wide start = c.op == RBX_STR_GET ? 0 : (wide)c.a, end = c.op == RBX_STR_GET ? -1 : (wide)c.b;
        if (start < 0 && end < 0 && start > end) return 0;
        if (start < 0) start += s.len;
        if (end < 0) end += s.len;
        if (start < 0) start = 0;
        if (end < 0) end = 0;
        if (end >= s.len) end = s.len - 1;
        if (start > end || s.len == 0) return 0;
        *reply = (int64_t)(end - start + 1);
        *read_known = s.kept;
        if (s.kept) read->assign(s.bytes.begin() + (size_t)start, s.bytes.begin() + (size_t)end + 1);
        return 0;
    }
    if (c.op == RBX_STR_SETRANGE) {
        if (c.a < 0) return kByteBadOffset;
        if (v == 0) return *reply = (int64_t)s.len, 0;
        const wide at = (wide)c.a;
        if (at + v > kMax) return kByteTooBig;
        if (at + v > s.len) s.resize(at + v);
        s.exists = true;
        if (s.kept)
            for (wide j = 0; j < v; ++j) s.bytes[(size_t)(at + j)] = value_byte(step, j);
        return *reply = (int64_t)s.len, 0;
    }
    if (s.len + v > kMax) return kByteTooBig;  // APPEND
    const wide at = s.len;
    s.resize(at + v);
    s.exists = true;
    if (s.kept)
        for (wide j = 0; j < v; ++j) s.bytes[(size_t)(at + j)] = value_byte(step, j);
    return *reply = (int64_t)s.len, 0;
}

static rbx_string_cmd cmd(int op, int64_t a, int64_t b, uint32_t v) {
    rbx_string_cmd c = {};
    c.op = (uint8_t)op;
    c.a = a;
    c.b = b;
    c.val_len = v;
    return c;
}

int main() {
    const int64_t mx = (int64_t)1 << 29;
    std::vector<rbx_string_cmd> alphabet;
    const int64_t ends[][2] = {{0, -1}, {-3, -2}, {1, 2}, {INT64_MIN, INT64_MAX}, {INT64_MAX, INT64_MIN}, {-1, -3},
                               {mx - 2, mx + 5}, {-2, INT64_MAX}};
    for (auto &e : ends) alphabet.push_back(cmd(RBX_STR_GETRANGE, e[0], e[1], 0));
    for (int64_t o : {(int64_t)-1, (int64_t)0, (int64_t)3, mx - 2, mx - 1, mx, INT64_MAX, INT64_MIN})
        for (uint32_t v : {0u, 1u, 2u}) alphabet.push_back(cmd(RBX_STR_SETRANGE, o, 0, v));
    for (uint32_t v : {0u, 1u, 3u, 0xFFFFFFFFu}) alphabet.push_back(cmd(RBX_STR_APPEND, INT64_MIN, INT64_MAX, v));
    alphabet.push_back(cmd(RBX_STR_GET, INT64_MAX, INT64_MIN, 0));
    const size_t A = alphabet.size();

    struct Start { bool exists; wide len; };
    const Start starts[] = {{false, 0}, {true, 0}, {true, 2}, {true, kMax - 1}, {true, kMax}};
    unsigned long long sequences = 0, steps = 0;
    for (const Start &st0 : starts) {
        for (int n = 1; n <= 4; ++n) {
            size_t total = 1;
            for (int i = 0; i < n; ++i) total *= A;
            for (size_t code = 0; code < total; ++code) {
                ++sequences;
                Str ref, eng;  // the restatement's string; the one byte_run_step's moves are applied to
                ref.exists = eng.exists = st0.exists;
                ref.resize(st0.len);
                eng.resize(st0.len);
                for (size_t j = 0; j < ref.bytes.size(); ++j) ref.bytes[j] = eng.bytes[j] = (uint8_t)(j + 1);
                size_t rest = code;
                for (int i = 0; i < n; ++i, rest /= A) {
                    ++steps;
                    const rbx_string_cmd &c = alphabet[rest % A];
                    int64_t want_reply;
                    bool want_nil, read_known;
                    std::vector<uint8_t> want_read;
                    const int want = restated(ref, c, i, &want_reply, &want_nil, &want_read, &read_known);
                    const ByteStep s = byte_run_step((uint64_t)eng.len, !eng.exists, c);
                    CHECK(s.fails == want, "op %d a %lld b %lld v %u: fails %d, want %d", c.op, (long long)c.a,
                          (long long)c.b, c.val_len, s.fails, want);
                    CHECK(s.reply == want_reply, "op %d a %lld b %lld v %u: reply %lld, want %lld", c.op, (long long)c.a,
                          (long long)c.b, c.val_len, (long long)s.reply, (long long)want_reply);
                    CHECK(s.nil == want_nil, "op %d: nil %d", c.op, (int)s.nil);
                    CHECK(byte_step_status(s) == (want ? 0xFF : want_nil ? 1 : 0), "op %d: status", c.op);
                    if (s.fails) {
                        CHECK(s.len == (uint64_t)eng.len && s.exists == eng.exists && !s.writes,
                              "a failed command moved the running state");
                    } else if (s.writes) {
                        CHECK(s.at + s.cnt <= s.len && s.len <= (uint64_t)kMax, "a write leaves the string");
                        eng.resize((wide)s.len);
                        eng.exists = true;
                        if (eng.kept)
                            for (uint64_t j = 0; j < s.cnt; ++j) eng.bytes[(size_t)(s.at + j)] = value_byte(i, (wide)j);
                    } else {
                        CHECK(s.len == (uint64_t)eng.len && s.exists == eng.exists, "a read moved the running state");
                        CHECK(s.at + s.cnt <= (uint64_t)eng.len, "a read leaves the string");
                        if (read_known && eng.kept) {
                            const std::vector<uint8_t> got(eng.bytes.begin() + (size_t)s.at,
                                                           eng.bytes.begin() + (size_t)(s.at + s.cnt));
                            CHECK(got == want_read, "op %d a %lld b %lld: the bytes read differ", c.op, (long long)c.a,
                                  (long long)c.b);
                        }
                    }
                    CHECK(eng.exists == ref.exists && eng.len == ref.len && eng.kept == ref.kept && eng.bytes == ref.bytes,
                          "the strings differ behind op %d a %lld v %u", c.op, (long long)c.a, c.val_len);
                }
            }
        }
    }
    // the caller's errors: the op, and a value slice against the value buffer, without a wrap
    rbx_string_cmd c = cmd(RBX_STR_APPEND, 0, 0, 4);
    c.val_off = 6;
    CHECK(!byte_cmd_illegal(c, 10) && byte_cmd_illegal(c, 9), "slice end");
    c.val_off = UINT64_MAX;
    CHECK(byte_cmd_illegal(c, UINT64_MAX - 1) && byte_cmd_illegal(c, UINT64_MAX), "slice wrap");
    c.val_len = 0;
    CHECK(!byte_cmd_illegal(c, UINT64_MAX) && byte_cmd_illegal(c, 5), "empty slice");
    c.op = RBX_STR_GET;
    CHECK(!byte_cmd_illegal(c, 0), "a read has no slice");
    c.op = RBX_STR_GET + 1;
    CHECK(byte_cmd_illegal(c, 0), "op");
    // the key's type comes behind SETRANGE's offset and ahead of everything else
    CHECK(byte_key_step(5, false, true, cmd(RBX_STR_SETRANGE, -1, 0, 1)).fails == kByteBadOffset, "offset first");
    CHECK(byte_key_step(5, false, true, cmd(RBX_STR_SETRANGE, mx, 0, 1)).fails == kByteWrongType, "type before size");
    CHECK(byte_key_step(5, false, true, cmd(RBX_STR_GET, 0, 0, 0)).fails == kByteWrongType, "GET");
    CHECK(byte_key_step(5, false, true, cmd(RBX_STR_APPEND, 0, 0, 0)).fails == kByteWrongType, "APPEND");

    if (g_failed) {
        std::printf("byte_cmd_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("byte_cmd_test: ok (%llu sequences, %llu steps)\n", sequences, steps);
    return 0;
}
