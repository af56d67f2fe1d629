// bit_groups_plan_test.cpp -- the host's planner for grouped BITOP / BITCOUNT calls (redisson_amd/csrc/
// bit_groups_plan.h: the phase rule and forwarding) at its hazards, built with -fsanitize=address,undefined
// (tests/test_bit_groups_plan_sanitized.py): the stamps are indexed by key ids up to nkeys - 1 and the CSR arrays by
// offsets the caller gives, so every case runs on exactly sized heap arrays.  No HIP.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../redisson_amd/csrc/bit_groups_plan.h"

enum : uint8_t { AND = 0, OR = 1, XOR = 2, NOT = 3 };
constexpr uint32_t NONE = rbx::kBitGroupNoDest, RUNS = rbx::kBitGroupRuns;

struct Group {
    uint8_t op;
    uint32_t dest;  // or NONE
    std::vector<uint32_t> srcs;
};

struct Plan {
    std::vector<uint32_t> end, fwd;
};

static long cases = 0;

static Plan plan(const std::vector<Group> &groups, uint32_t nkeys, const std::vector<uint8_t> &failed = {}) {
    // exactly sized heap copies: an index one past any of them is an ASan report
    const uint32_t n = (uint32_t)groups.size();
    std::unique_ptr<uint8_t[]> op(new uint8_t[n]);
    std::unique_ptr<uint32_t[]> dest(new uint32_t[n]);
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
    off[0] = 0;
    for (uint32_t g = 0; g < n; ++g) {
        op[g] = groups[g].op;
        dest[g] = groups[g].dest;
        off[g + 1] = off[g] + groups[g].srcs.size();
    }
    std::unique_ptr<uint32_t[]> src(new uint32_t[off[n]]);
    for (uint32_t g = 0; g < n; ++g)
        if (!groups[g].srcs.empty())
            memcpy(src.get() + off[g], groups[g].srcs.data(), groups[g].srcs.size() * sizeof(uint32_t));
    std::unique_ptr<uint8_t[]> fl(new uint8_t[n]);
    for (uint32_t g = 0; g < n; ++g) fl[g] = g < failed.size() ? failed[g] : 0;
    Plan p{{77, 77}, {5}};  // both cleared by the planner
    rbx::bit_groups_plan(op.get(), dest.get(), off.get(), src.get(), failed.empty() ? nullptr : fl.get(), n, nkeys, &p.end,
                         &p.fwd);
    return p;
}

static void show(const std::vector<uint32_t> &v) {
    for (uint32_t x : v) {
        if (x == RUNS) std::printf(" -");
        else std::printf(" %u", x);
    }
}

static bool expect(const char *what, const Plan &got, const std::vector<uint32_t> &end, const std::vector<uint32_t> &fwd) {
    ++cases;
    if (got.end == end && got.fwd == fwd) return true;
    std::printf("bit_groups_plan_test: %s: got end", what);
    show(got.end);
    std::printf(" fwd");
    show(got.fwd);
    std::printf(", want end");
    show(end);
    std::printf(" fwd");
    show(fwd);
    std::printf("\n");
    return false;
}

int main() {
    bool ok = true;
    enum { A = 0, B = 1, C = 2, D = 3 };
    ok &= expect("empty input", plan({}, 0), {}, {});
    ok &= expect("one group", plan({{AND, A, {B, C}}}, 3), {1}, {RUNS});
    ok &= expect("one reader", plan({{OR, NONE, {B}}}, 2), {1}, {RUNS});
    ok &= expect("read after write", plan({{OR, A, {B}}, {OR, C, {A}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("write after read", plan({{OR, A, {B}}, {OR, B, {C}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("write after write", plan({{OR, A, {B}}, {OR, A, {C}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("destination first among its sources", plan({{XOR, A, {A, B}}}, 2), {1}, {RUNS});
    ok &= expect("destination last among its sources", plan({{XOR, A, {B, A}}}, 2), {1}, {RUNS});
    ok &= expect("self-source, then independent", plan({{OR, A, {A, B}}, {OR, C, {B, D}}}, 4), {2}, {RUNS, RUNS});
    ok &= expect("self-source is still a write", plan({{NOT, A, {A}}, {OR, B, {A}}}, 2), {1, 2}, {RUNS, RUNS});
    ok &= expect("shared sources", plan({{AND, A, {C, D}}, {AND, B, {C, D}}, {AND, NONE, {C, D}}}, 4), {3},
                 {RUNS, RUNS, RUNS});
    // a group without a destination only reads
    ok &= expect("reader before a writer of its source", plan({{AND, NONE, {A, B}}, {OR, A, {C}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("reader after a writer of its source", plan({{OR, A, {C}}, {AND, NONE, {A, B}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("reader before a writer of another key", plan({{AND, NONE, {A, B}}, {OR, C, {A}}}, 3), {2}, {RUNS, RUNS});
    ok &= expect("two readers of one key", plan({{OR, NONE, {A}}, {OR, NONE, {A}}}, 1), {2}, {RUNS, RUNS});
    // forwarding
    ok &= expect("forwarded", plan({{AND, C, {A, B}}, {OR, NONE, {C}}}, 3), {2}, {RUNS, 0});
    ok &= expect("forwarded under AND and XOR", plan({{AND, C, {A, B}}, {AND, NONE, {C}}, {XOR, NONE, {C}}}, 3), {3},
                 {RUNS, 0, 0});
    ok &= expect("not forwarded for NOT", plan({{AND, C, {A, B}}, {NOT, NONE, {C}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("not forwarded for two entries", plan({{AND, C, {A, B}}, {OR, NONE, {C, C}}}, 3), {1, 2}, {RUNS, RUNS});
    ok &= expect("not forwarded with a destination", plan({{AND, C, {A, B}}, {OR, D, {C}}}, 4), {1, 2}, {RUNS, RUNS});
    ok &= expect("not forwarded from a failed writer", plan({{AND, C, {A, B}}, {OR, NONE, {C}}}, 3, {1, 0}), {2},
                 {RUNS, RUNS});
    ok &= expect("not forwarded from an earlier phase", plan({{OR, C, {A}}, {OR, A, {B}}, {OR, NONE, {C}}}, 3), {1, 3},
                 {RUNS, RUNS, RUNS});
    ok &= expect("forwarded from the last writer", plan({{OR, C, {A}}, {OR, C, {B}}, {OR, NONE, {C}}}, 3), {1, 3},
                 {RUNS, RUNS, 1});
    ok &= expect("a forwarded count stamps no read", plan({{OR, C, {A}}, {OR, NONE, {C}}, {OR, D, {B}}}, 4), {3},
                 {RUNS, 0, RUNS});
    ok &= expect("a failed forwarded candidate", plan({{OR, C, {A}}, {OR, NONE, {C}}}, 3, {0, 1}), {2}, {RUNS, RUNS});
    // a failed group between two dependent ones: it writes nothing and closes nothing, the hazard stays
    ok &= expect("failed between dependents", plan({{OR, A, {B}}, {OR, B, {A}}, {OR, C, {A}}}, 3, {0, 1, 0}), {2, 3},
                 {RUNS, RUNS, RUNS});
    ok &= expect("failed would have been the hazard", plan({{OR, A, {B}}, {OR, A, {C}}, {OR, D, {C}}}, 4, {0, 1, 0}), {3},
                 {RUNS, RUNS, RUNS});
    ok &= expect("failed ones only", plan({{OR, A, {B}}, {OR, NONE, {A}}}, 2, {1, 1}), {}, {RUNS, RUNS});
    ok &= expect("failed first", plan({{OR, A, {B}}, {OR, B, {C}}}, 3, {1, 0}), {2}, {RUNS, RUNS});
    ok &= expect("key ids at nkeys - 1", plan({{OR, 9, {8, 9}}, {OR, NONE, {9}}, {OR, 8, {9}}}, 10), {2, 3}, {RUNS, 0, RUNS});
    {
        // BITOP AND t_i a b; BITCOUNT t_i -- with distinct temporaries one phase, on one temporary a phase per pair
        std::vector<Group> apart, same;
        std::vector<uint32_t> fwd, each;
        for (uint32_t i = 0; i < 1000; ++i) {
            apart.push_back({AND, 2 + i, {A, B}});
            apart.push_back({OR, NONE, {2 + i}});
            same.push_back({AND, C, {A, B}});
            same.push_back({OR, NONE, {C}});
            fwd.push_back(RUNS);
            fwd.push_back(2 * i);
            each.push_back(i < 999 ? 2 * i + 2 : 2000);
        }
        ok &= expect("1,000 pairs on distinct temporaries", plan(apart, 1002), {2000}, fwd);
        ok &= expect("1,000 pairs on one temporary", plan(same, 3), each, fwd);
        std::vector<Group> chain;
        std::vector<uint32_t> ends, runs;
        for (uint32_t i = 0; i < 1000; ++i) {
            chain.push_back({OR, i + 1, {i, i + 1}});  // k1 <- k0 | k1, k2 <- k1 | k2, ...
            ends.push_back(i + 1);
            runs.push_back(RUNS);
        }
        ok &= expect("a chain of 1,000", plan(chain, 1001), ends, runs);
    }
    if (!ok) return 1;
    std::printf("bit_groups_plan_test: ok (%ld cases)\n", cases);
    return 0;
}
