// bit_groups_plan.h -- the host's view of a grouped BITOP / BITCOUNT call (rbx_bitset_op_groups) before
// anything reaches the device: the groups split into phases, and the counts that need no launch of their own
// forwarded.  No HIP, no context: tests/c/bit_groups_plan_test.cpp runs it alone under sanitizers.  The caller's CSR
// arrays are checked by hll_groups_plan.h's hll_groups_check, whose limits this call shares.
#pragma once
#include <cstdint>
#include <vector>

namespace rbx {

constexpr uint32_t kBitGroupNoDest = 0xFFFFFFFFu;  // RBX_BITGROUP_NO_DEST: the group stores its result nowhere
constexpr uint32_t kBitGroupRuns = 0xFFFFFFFFu;    // fwd[g]: the group is not forwarded
constexpr uint8_t kBitGroupNot = 3;                // RBX_BITOP_NOT

// The phases of a call.  Group g combines the keys src[off[g] .. off[g + 1]) under op[g] into the key dest[g], or
// into nothing when dest[g] is kBitGroupNoDest (it then only reads: a BITCOUNT of the combination); all are key ids
// below nkeys, equal ids are one key (the caller passes canonical ids).  failed (nullable): the groups that fail
// alone; they write nothing, close nothing and forward nothing.
//
// Forwarding.  A group without a destination, with exactly one source entry and an op other than NOT, asks for the
// length and the count of that key as it stands.  When the key is the destination of an earlier group f of the
// current phase that does not fail, those are f's own replies: fwd[g] = f (the last such group), the group raises
// no hazard, stamps nothing and never reaches the device.  Every other group has fwd[g] = kBitGroupRuns.
//
// A phase is a maximal stretch of groups one launch can run: a group that runs closes the phase before it when
//   - its destination is the destination of an earlier group of the phase (write after write),
//   - its destination is a source of an earlier group of the phase with another or no destination (write after
//     read: that group must not see it),
//   - one of its sources is the destination of an earlier group of the phase (read after write); a group without a
//     destination closes the phase by this rule alone;
// its own destination among its own sources counts for nothing.  So `BITOP AND t_i a b; BITCOUNT t_i` with distinct
// t_i, repeated N times, is one phase (every BITCOUNT is forwarded), and the same pipeline on one temporary t is N
// phases: each BITOP writes the key the one before it wrote.  On return end[p] is one past the last group of
// phase p: phase p is the groups [p ? end[p - 1] : 0, end[p]) that neither fail nor are forwarded.  A stretch
// without a group that runs is no phase: no groups, or failed ones only, give none.
inline void bit_groups_plan(const uint8_t *op, const uint32_t *dest, const uint64_t *off, const uint32_t *src,
                            const uint8_t *failed, uint32_t ngroups, uint32_t nkeys, std::vector<uint32_t> *end,
                            std::vector<uint32_t> *fwd) {
    end->clear();
    fwd->assign(ngroups, kBitGroupRuns);
    // the phase (1-based) in which a key was last written, and last read by a group with another destination; the
    // group that wrote it last
    std::vector<uint32_t> written(nkeys, 0), read(nkeys, 0), writer(nkeys, 0);
    uint32_t phase = 1;
    bool open = false;  // the current phase holds a group
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (failed && failed[g]) continue;
        const uint32_t d = dest[g];
        const bool writes = d != kBitGroupNoDest;
        if (!writes && off[g + 1] - off[g] == 1 && op[g] != kBitGroupNot && written[src[off[g]]] == phase) {
            (*fwd)[g] = writer[src[off[g]]];
            continue;
        }
        bool hazard = writes && (written[d] == phase || read[d] == phase);
        for (uint64_t i = off[g]; i < off[g + 1] && !hazard; ++i)
            hazard = (!writes || src[i] != d) && written[src[i]] == phase;
        if (hazard) {  // (only a phase that holds a group has stamped a key)
            end->push_back(g);
            ++phase;
        }
        open = true;
        if (writes) {
            written[d] = phase;
            writer[d] = g;
        }
        for (uint64_t i = off[g]; i < off[g + 1]; ++i)
            if (!writes || src[i] != d) read[src[i]] = phase;
    }
    if (open) end->push_back(ngroups);
}

}  // namespace rbx
