// hll_groups_plan.h -- the host's view of a grouped PFCOUNT / PFMERGE call (rbx_hll_count_groups,
// rbx_hll_merge_groups) before anything reaches the device: the caller's arrays checked, and the
// merges split into phases.  No HIP, no context: tests/c/hll_groups_plan_test.cpp runs it alone under sanitizers.
#pragma once
#include <cstdint>
#include <vector>

namespace rbx {

// The CSR arrays of a call: group g is the entries grp_key[grp_off[g] .. grp_off[g + 1]), each below nkeys.
// Returns what is wrong with them, or nullptr.  need_entries: every group holds an entry (PFCOUNT needs a key; a
// PFMERGE without sources is legal).
inline const char *hll_groups_check(const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups, uint32_t nkeys,
                                    bool need_entries) {
    if (ngroups == 0) return nullptr;
    if (!grp_off) return "NULL argument";
    if (ngroups >= (1u << 31)) return "a call takes fewer than 2^31 groups";
    if (grp_off[0] != 0) return "group offsets must start at 0";
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (grp_off[g + 1] < grp_off[g]) return "group offsets must be ascending";
        if (need_entries && grp_off[g + 1] == grp_off[g]) return "a group names no key";
    }
    const uint64_t total = grp_off[ngroups];
    if (total >= (1ULL << 32)) return "a call takes fewer than 2^32 entries";
    if (total && !grp_key) return "NULL argument";
    for (uint64_t i = 0; i < total; ++i)
        if (grp_key[i] >= nkeys) return "a group's key is not below nkeys";
    return nullptr;
}

// The phases of a merge call.  Group g merges the keys src[off[g] .. off[g + 1]) into the key dest[g]; all are key
// ids below nkeys, equal ids are one key (the caller passes canonical ids).  failed (nullable): the groups that
// fail alone; they write nothing and close nothing.  A phase is a maximal stretch of groups one launch can run:
// group g closes the phase before it when
//   - its destination is the destination of an earlier group of the phase (write after write),
//   - its destination is a source of an earlier group of the phase (write after read: that group must not see it),
//   - one of its sources is the destination of an earlier group of the phase (read after write);
// its own destination among its own sources counts for nothing.  On return end[p] is one past the last group of
// phase p: phase p is the groups [p ? end[p - 1] : 0, end[p]) that do not fail.  A stretch without a group that
// runs is no phase: no groups, or failed ones only, give none.
inline void hll_groups_plan(const uint32_t *dest, const uint64_t *off, const uint32_t *src, const uint8_t *failed,
                            uint32_t ngroups, uint32_t nkeys, std::vector<uint32_t> *end) {
    end->clear();
    // the phase (1-based) in which a key was last written, and last read by a group with another destination
    std::vector<uint32_t> written(nkeys, 0), read(nkeys, 0);
    uint32_t phase = 1;
    bool open = false;  // the current phase holds a group
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (failed && failed[g]) continue;
        const uint32_t d = dest[g];
        bool hazard = written[d] == phase || read[d] == phase;
        for (uint64_t i = off[g]; i < off[g + 1] && !hazard; ++i) hazard = src[i] != d && written[src[i]] == phase;
        if (hazard) {  // (only a phase that holds a group has stamped a key)
            end->push_back(g);
            ++phase;
        }
        open = true;
        written[d] = phase;
        for (uint64_t i = off[g]; i < off[g + 1]; ++i)
            if (src[i] != d) read[src[i]] = phase;
    }
    if (open) end->push_back(ngroups);
}

}  // namespace rbx
