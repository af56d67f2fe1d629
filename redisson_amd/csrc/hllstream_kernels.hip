// hllstream_kernels.hip -- the grouped add run of the ordered PFADD / PFCOUNT stream over many HyperLogLogs
// in one call (rbx_hll_stream): what RBatch.getHyperLogLog(name) queues (M/RedissonBatch.java:57-64,
// M/api/RBatch.java:213-215) and CommandBatchService executes in submission order.  DESIGN section 11.7 has
// the rules; the phases, the rounds path (k_hll_pfadd, one launch per run of distinct keys) and the sparse
// strings (k_hll_sparse_replay) are api_hll.cpp's and hll_kernels.hip's.
//
// A chunk of an add run holds m elements of consecutive commands.  A PFADD replies "a register changed", and
// a register only rises, so the elements that matter to a register are walked in command order:
//   1. k_hs_pairs   one lane per element: its command (a search over the call's element offsets), its key
//                   record, its hash; emits cell = canon << 20 | register << 6 | count and the command's
//                   position in the chunk.  An element of a command that fails alone gets the one bit above
//                   every cell.
//   2. cell_sort    a stable radix sort of the pairs over bits [6, 20 + key bits [+ 1]): equal (key, register)
//                   stay in element order, which is command order, and the count rides in the unsorted low bits.
//   3. k_hs_runs    the lane at the head of a run of equal (key, register) reads the register byte once, walks
//                   the run, stores 1 into the changed word of every command whose count rises above what
//                   stands, and stores the byte once if it rose.  Each byte has one writer: no atomics.
// The launch count does not depend on how often keys repeat.  The worst case is one (key, register) hit by
// every element of the chunk: one lane walks them all (DESIGN 11.1 row d's shape; documented, not engineered
// around).
// M/ = redisson/src/main/java/org/redisson/ of the reference
#include <hip/hip_runtime.h>

#include "../../include/rbx.h"
#include "bloom_common.h"
#include "rbx_kernels.h"

namespace rbx {

typedef unsigned long long u64;

constexpr uint32_t kHsRegMask = 16383u, kHsCountMask = 63u;

template <int ELEN>
__global__ __launch_bounds__(256) void k_hs_pairs(KeysDev elems, uint64_t first, uint64_t elem0, uint32_t m,
                                                  const HllKey *__restrict__ tab,
                                                  const uint64_t *__restrict__ cmd_elem,
                                                  const uint32_t *__restrict__ cmd_key, uint64_t cmd0, uint32_t ncmds,
                                                  u64 failed_cell, u64 *__restrict__ cell, uint32_t *__restrict__ pos) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        // the last command of the chunk that starts at or before the element (the commands before it that start
        // there too are empty); the chunk's first command starts at elem0
        const uint64_t g = elem0 + j;
        uint32_t lo = 0, hi = ncmds - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (cmd_elem[cmd0 + mid] <= g) lo = mid;
            else hi = mid - 1;
        }
        const HllKey k = tab[cmd_key[cmd0 + lo]];
        u64 c = failed_cell;
        if (!(k.flags & kHllKeyFailed)) {
            const uint64_t h = elem_hash<ELEN>(elems, first + j);
            c = ((u64)k.canon << kHsKeyShift) | ((u64)(h & kHsRegMask) << kHsRegShift) | hll_count_of(h);
        }
        cell[j] = c;
        pos[j] = lo;
    }
}

__global__ __launch_bounds__(256) void k_hs_runs(const HllKey *__restrict__ tab, const u64 *__restrict__ cell,
                                                 const uint32_t *__restrict__ pos, uint32_t m, u64 failed_cell,
                                                 uint32_t *__restrict__ changed) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const u64 c = cell[i];
        const u64 run = c >> kHsRegShift;
        if (c >= failed_cell || (i > 0 && (cell[i - 1] >> kHsRegShift) == run)) continue;  // failed, or not a head
        uint8_t *reg = tab[c >> kHsKeyShift].regs + ((uint32_t)run & kHsRegMask);
        const uint32_t was = *reg;
        uint32_t cur = was;
        uint32_t j = i;
        u64 cj = c;
        do {
            const uint32_t cnt = (uint32_t)cj & kHsCountMask;
            if (cnt > cur) {
                cur = cnt;
                changed[pos[j]] = 1u;  // plain and idempotent, as k_hll_pfadd's
            }
            if (++j == m) break;
            cj = cell[j];
        } while ((cj >> kHsRegShift) == run);
        if (cur != was) *reg = (uint8_t)cur;
    }
}

__global__ __launch_bounds__(256) void k_hs_promoted(uint32_t *const *__restrict__ states, uint32_t n,
                                                     uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = states[i][0];
}

int launch_hllstream_grouped(const KeysDev &elems, int elen_fast, uint64_t first, uint64_t elem0, uint32_t m,
                             const HllKey *d_tab, const uint64_t *d_cmd_elem, const uint32_t *d_cmd_key, uint64_t cmd0,
                             uint32_t ncmds, uint32_t *d_changed, int key_bits, bool has_failed, void *d_scratch,
                             size_t scratch_bytes, hipStream_t st) {
    if (!m || !ncmds) return 0;
    CellSortBufs<u64> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, m, &b);
    if (e) return e;
    // the bit above every cell (20 + key_bits <= 52); the sort looks at it only when a command fails
    const u64 failed_cell = 1ULL << (kHsKeyShift + key_bits);
    with_klen<true>(elen_fast, [&](auto elen) {
        hipLaunchKernelGGL(k_hs_pairs<decltype(elen)::value>, dim3(grid_for(m, kMaxGrid)), dim3(256), 0, st, elems, first,
                           elem0, m, d_tab, d_cmd_elem, d_cmd_key, cmd0, ncmds, failed_cell, b.cell_in, b.pos_in);
    });
    e = cell_sort(b, m, kHsRegShift, hllstream_end_bit(key_bits, has_failed), st);  // the (key, register) bits only
    if (e) return e;
    hipLaunchKernelGGL(k_hs_runs, dim3(grid_for(m, kMaxGrid)), dim3(256), 0, st, d_tab, b.cell_out, b.pos_out, m,
                       failed_cell, d_changed + cmd0);
    return 0;
}

void launch_hllstream_promoted(uint32_t *const *d_states, uint32_t n, uint32_t *d_out, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(k_hs_promoted, dim3((n + 255) / 256), dim3(256), 0, st, d_states, n, d_out);
}

}  // namespace rbx
