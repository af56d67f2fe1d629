// hll_groups_plan_test.cpp -- the host's planner for grouped PFCOUNT / PFMERGE calls (redisson_amd/csrc/
// hll_groups_plan.h: the argument check and the phase rule) at its hazards, built with -fsanitize=address,undefined
// (tests/test_hll_groups_plan_sanitized.py): the stamps are indexed by key ids up to nkeys - 1 and the CSR arrays by
// offsets the caller gives, so every case runs on exactly sized heap arrays.  No HIP.
#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../../redisson_amd/csrc/hll_groups_plan.h"

using Merge = std::pair<uint32_t, std::vector<uint32_t>>;  // destination, sources

static long cases = 0;

static std::vector<uint32_t> plan(const std::vector<Merge> &merges, uint32_t nkeys, const std::vector<uint8_t> &failed = {}) {
    // exactly sized heap copies: an index one past any of them is an ASan report
    const uint32_t n = (uint32_t)merges.size();
    std::unique_ptr<uint32_t[]> dest(new uint32_t[n]);
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
    off[0] = 0;
    for (uint32_t g = 0; g < n; ++g) {
        dest[g] = merges[g].first;
        off[g + 1] = off[g] + merges[g].second.size();
    }
    std::unique_ptr<uint32_t[]> src(new uint32_t[off[n]]);
    for (uint32_t g = 0; g < n; ++g)
        if (!merges[g].second.empty())
            memcpy(src.get() + off[g], merges[g].second.data(), merges[g].second.size() * sizeof(uint32_t));
    std::unique_ptr<uint8_t[]> fl(new uint8_t[n]);
    for (uint32_t g = 0; g < n; ++g) fl[g] = g < failed.size() ? failed[g] : 0;
    std::vector<uint32_t> end{77, 77};  // cleared by the planner
    rbx::hll_groups_plan(dest.get(), off.get(), src.get(), failed.empty() ? nullptr : fl.get(), n, nkeys, &end);
    return end;
}

static bool expect(const char *what, const std::vector<uint32_t> &got, const std::vector<uint32_t> &want) {
    ++cases;
    if (got == want) return true;
    std::printf("hll_groups_plan_test: %s: got", what);
    for (uint32_t x : got) std::printf(" %u", x);
    std::printf(", want");
    for (uint32_t x : want) std::printf(" %u", x);
    std::printf("\n");
    return false;
}

static bool expect_check(const char *what, const char *got, bool want_error) {
    ++cases;
    if ((got != nullptr) == want_error) return true;
    std::printf("hll_groups_plan_test: check %s: %s\n", what, got ? got : "accepted");
    return false;
}

int main() {
    bool ok = true;
    enum { A = 0, B = 1, C = 2, D = 3 };
    ok &= expect("empty input", plan({}, 0), {});
    ok &= expect("one group", plan({{A, {B, C}}}, 3), {1});
    ok &= expect("one group without sources", plan({{A, {}}}, 1), {1});
    ok &= expect("read after write", plan({{A, {B}}, {C, {A}}}, 3), {1, 2});
    ok &= expect("write after read", plan({{A, {B}}, {B, {C}}}, 3), {1, 2});
    ok &= expect("write after write", plan({{A, {B}}, {A, {C}}}, 3), {1, 2});
    ok &= expect("self-source", plan({{A, {A, B}}}, 2), {1});
    ok &= expect("self-source, then independent", plan({{A, {A, B}}, {C, {B, D}}}, 4), {2});
    ok &= expect("self-source is still a write", plan({{A, {A}}, {B, {A}}}, 2), {1, 2});
    ok &= expect("shared sources", plan({{A, {C, D}}, {B, {C, D}}}, 4), {2});
    ok &= expect("three groups, hazard at the third", plan({{A, {B}}, {C, {D}}, {D, {B}}}, 4), {2, 3});
    // a failed group between two dependent ones: it writes nothing and closes nothing, the hazard stays
    ok &= expect("failed between dependents", plan({{A, {B}}, {B, {A}}, {C, {A}}}, 3, {0, 1, 0}), {2, 3});
    ok &= expect("failed would have been the hazard", plan({{A, {B}}, {A, {C}}, {D, {C}}}, 4, {0, 1, 0}), {3});
    ok &= expect("failed ones only", plan({{A, {B}}, {B, {A}}}, 2, {1, 1}), {});
    ok &= expect("failed first", plan({{A, {B}}, {B, {C}}}, 3, {1, 0}), {2});
    ok &= expect("key ids at nkeys - 1", plan({{9, {8, 9}}, {8, {9}}}, 10), {1, 2});
    {
        std::vector<Merge> chain, apart;
        std::vector<uint32_t> each;
        for (uint32_t i = 0; i < 1000; ++i) {
            chain.push_back({i + 1, {i}});          // k1 <- k0, k2 <- k1, ...
            apart.push_back({2 * i, {2 * i + 1}});  // distinct pairs
            each.push_back(i + 1);
        }
        ok &= expect("a chain of 1,000", plan(chain, 1001), each);
        ok &= expect("1,000 independent groups", plan(apart, 2000), {1000});
    }
    // the argument check
    {
        const uint64_t off[] = {0, 2, 2, 3};
        const uint32_t key[] = {0, 4, 3};
        ok &= expect_check("no groups", rbx::hll_groups_check(nullptr, nullptr, 0, 0, true), false);
        ok &= expect_check("merges", rbx::hll_groups_check(off, key, 3, 5, false), false);
        ok &= expect_check("a count without entries", rbx::hll_groups_check(off, key, 3, 5, true), true);
        ok &= expect_check("a key at nkeys", rbx::hll_groups_check(off, key, 3, 4, false), true);
        ok &= expect_check("NULL offsets", rbx::hll_groups_check(nullptr, key, 3, 5, false), true);
        ok &= expect_check("NULL keys", rbx::hll_groups_check(off, nullptr, 3, 5, false), true);
        const uint64_t none[] = {0, 0};
        ok &= expect_check("NULL keys without entries", rbx::hll_groups_check(none, nullptr, 1, 0, false), false);
        const uint64_t late[] = {1, 2}, back[] = {0, 2, 1}, huge[] = {0, 1ULL << 32};
        ok &= expect_check("offsets from 1", rbx::hll_groups_check(late, key, 1, 5, false), true);
        ok &= expect_check("descending offsets", rbx::hll_groups_check(back, key, 2, 5, false), true);
        ok &= expect_check("2^32 entries", rbx::hll_groups_check(huge, key, 1, 5, false), true);
    }
    if (!ok) return 1;
    std::printf("hll_groups_plan_test: ok (%ld cases)\n", cases);
    return 0;
}
