// field_cmd_check_test.cpp -- the per-command check of the BITFIELD stream (redisson_amd/csrc/field_rule.h
// field_cmd_check: the type first, then the offset limit) at its edges, built with
// -fsanitize=address,undefined (tests/test_field_cmd_check_sanitized.py): offset + size must not be computed
// in a way that overflows or shifts out of range at offsets up to 2^64 - 1.  No HIP.
#include <cstdio>
#include <initializer_list>

#include "../../redisson_amd/csrc/field_rule.h"

using rbx::field_cmd_check;
using rbx::kFieldCmdBadOffset;
using rbx::kFieldCmdBadType;
using rbx::kFieldCmdOk;

static long cases = 0;

static bool expect(int is_signed, int size, uint64_t offset, int want) {
    ++cases;
    const int got = field_cmd_check(is_signed, size, offset);
    if (got == want) return true;
    std::printf("field_cmd_check_test: %c%d at %llu: %d, want %d\n", is_signed ? 'i' : 'u', size,
                (unsigned long long)offset, got, want);
    return false;
}

// the restated rule: a type is u1..u63 or i1..i64; a legal field lies wholly below bit 2^32
static int restated(int is_signed, int size, unsigned __int128 offset) {
    if (size < 1 || (is_signed ? size > 64 : size > 63)) return kFieldCmdBadType;
    const unsigned __int128 limit = (unsigned __int128)1 << 32;
    return offset + (unsigned)size <= limit ? kFieldCmdOk : kFieldCmdBadOffset;
}

int main() {
    const uint64_t limit = 1ULL << 32;
    bool ok = true;
    // the type check's edges, at a legal offset and at offsets past the limit: the type is looked at first
    for (uint64_t off : {(uint64_t)0, limit, ~(uint64_t)0}) {
        ok &= expect(0, 63, off, off ? kFieldCmdBadOffset : kFieldCmdOk);
        ok &= expect(0, 64, off, kFieldCmdBadType);
        ok &= expect(1, 64, off, off ? kFieldCmdBadOffset : kFieldCmdOk);
        ok &= expect(1, 65, off, kFieldCmdBadType);
        ok &= expect(0, 0, off, kFieldCmdBadType);
        ok &= expect(1, 0, off, kFieldCmdBadType);
        ok &= expect(1, -1, off, kFieldCmdBadType);
        ok &= expect(0, 255, off, kFieldCmdBadType);
    }
    // the offset limit's edges for every legal type
    for (int is_signed = 0; is_signed <= 1; ++is_signed)
        for (int size = 1; size <= (is_signed ? 64 : 63); ++size) {
            ok &= expect(is_signed, size, limit - (uint64_t)size, kFieldCmdOk);
            ok &= expect(is_signed, size, limit - (uint64_t)size + 1, kFieldCmdBadOffset);
            ok &= expect(is_signed, size, limit - 1, size == 1 ? kFieldCmdOk : kFieldCmdBadOffset);
            ok &= expect(is_signed, size, limit, kFieldCmdBadOffset);
            ok &= expect(is_signed, size, ~0ULL, kFieldCmdBadOffset);
            ok &= expect(is_signed, size, ~0ULL - (uint64_t)size + 1, kFieldCmdBadOffset);  // offset + size wraps to 0
            ok &= expect(is_signed, size, 0, kFieldCmdOk);
        }
    // against the restatement over a grid of offsets around every power of two
    for (int is_signed = 0; is_signed <= 1; ++is_signed)
        for (int size = -1; size <= 66; ++size)
            for (int b = 0; b < 64; ++b)
                for (int d = -70; d <= 70; ++d) {
                    const uint64_t off = (1ULL << b) + (uint64_t)(int64_t)d;
                    ok &= expect(is_signed, size, off, restated(is_signed, size, off));
                }
    if (!ok) return 1;
    std::printf("field_cmd_check_test: ok (%ld cases)\n", cases);
    return 0;
}
