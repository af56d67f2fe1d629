// cell_sort.hip -- the stable sort of (cell, position) pairs behind every grouped path: the ordered streams
// (bitstream_, fieldstream_, hllstream_kernels.hip: 8-byte cells) and the single-key BITFIELD batch
// (bitfield_kernels.hip: 4-byte slots).  The only translation unit that includes rocPRIM's radix sort, so
// librbx.so carries each instantiation's kernels once.  rbx_kernels.h has the contract.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "rbx_kernels.h"

namespace rbx {

template <class Cell>
int cell_sort_scratch_bytes(uint32_t n, int begin_bit, int end_bit, size_t *bytes) {
    size_t temp = 0;
    Cell *nil_cell = nullptr;
    uint32_t *nil_pos = nullptr;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, temp, nil_cell, nil_cell, nil_pos, nil_pos, (size_t)n,
                                                   (unsigned)begin_bit, (unsigned)end_bit, (hipStream_t) nullptr);
    if (e != hipSuccess) return (int)e;
    *bytes = 2 * cell_sort_array_bytes(n, sizeof(Cell)) + 2 * cell_sort_array_bytes(n, 4) + temp;
    return 0;
}

template <class Cell>
int cell_sort(const CellSortBufs<Cell> &b, uint32_t n, int begin_bit, int end_bit, hipStream_t st) {
    size_t temp = b.temp_bytes;
    return (int)rocprim::radix_sort_pairs(b.temp, temp, b.cell_in, b.cell_out, b.pos_in, b.pos_out, (size_t)n,
                                          (unsigned)begin_bit, (unsigned)end_bit, st);
}

template int cell_sort_scratch_bytes<uint32_t>(uint32_t, int, int, size_t *);
template int cell_sort_scratch_bytes<unsigned long long>(uint32_t, int, int, size_t *);
template int cell_sort<uint32_t>(const CellSortBufs<uint32_t> &, uint32_t, int, int, hipStream_t);
template int cell_sort<unsigned long long>(const CellSortBufs<unsigned long long> &, uint32_t, int, int, hipStream_t);

}  // namespace rbx
