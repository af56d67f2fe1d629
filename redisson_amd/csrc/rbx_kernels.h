// rbx_kernels.h -- shared device structs and kernel launchers (host <-> .hip files): the shared types
// first, then one section per .hip file with its argument structs, its launchers and its set_* knobs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/rbx.h"
#include "bk_entry.h"
#include "rbx_device.h"
#include "range_cmd.h"  // after rbx_device.h: it keeps an RBX_HD that is already defined
#include "byte_cmd.h"

namespace rbx {

constexpr unsigned kMaxGrid = 2048;  // grid-stride cap: 256 CUs x 8 blocks of 256 threads

// Diagnostic switches that make answers wrong (timing A/Bs: rbx_tune "stream_diag",
// "contains_partition_flags", "add_partition_diag") exist only in the profiling build
// librbx_diag.so (`make diag`: -DRBX_DIAG=1, used by tools/ through RBX_LIB_PATH).  In librbx.so
// kDiag is false: every kernel zeroes its diag argument on entry, so those branches are compiled
// out, and rbx_tune rejects the keys.
#ifndef RBX_DIAG
#define RBX_DIAG 0
#endif
constexpr bool kDiag = RBX_DIAG != 0;  // true only in the -DRBX_DIAG=1 profiling build

// Launcher dispatch from the runtime key length to the kernels' KLEN template argument:
// f(std::integral_constant<int, L>{}) with L = 16 / 32 / 64 for the fixed-length fast paths (and 8 with
// WITH8: the HyperLogLog elements), 0 for the any-length path.
template <bool WITH8 = false, class F> inline void with_klen(int klen_fast, F &&f) {
    if constexpr (WITH8)
        if (klen_fast == 8) return f(std::integral_constant<int, 8>{});
    if (klen_fast == 16) return f(std::integral_constant<int, 16>{});
    if (klen_fast == 32) return f(std::integral_constant<int, 32>{});
    if (klen_fast == 64) return f(std::integral_constant<int, 64>{});
    return f(std::integral_constant<int, 0>{});
}
// ... and from k to KMAX, the unrolled loops' bound: the smallest of 8 / 16 / 32 that holds k, up to
// TOP (16 or 32).  A k past TOP gets REST: 0, the any-k kernels, or TOP itself where the host bounds k.
template <int TOP, int REST = 0, class F> inline void with_kmax(uint32_t k, F &&f) {
    static_assert((TOP == 16 || TOP == 32) && (REST == 0 || REST == TOP), "ladder 8 / 16 [/ 32] / rest");
    if (k <= 8) return f(std::integral_constant<int, 8>{});
    if (k <= 16) return f(std::integral_constant<int, 16>{});
    if (TOP == 32 && k <= 32) return f(std::integral_constant<int, TOP>{});
    return f(std::integral_constant<int, REST>{});
}

struct KeysDev {
    const uint8_t *bytes;
    const uint64_t *offsets;  // nullable: fixed stride
    uint64_t stride;
    uint64_t n;
    uint64_t off_base;        // subtracted from offsets[] (a slice of a larger arena)
};

// One Bloom filter as the kernels see it (device-resident table for multi-tenant calls).
struct FilterDesc {
    uint32_t *bm;                   // bitmap words (Redis string bytes, MSB-first)
    unsigned long long *redis_len;  // device word: Redis string length in bytes
    ModParams mp;
    uint32_t k;
    uint32_t fid;  // identity in the first-setter table (unique per filter within a call)
};

// The per-filter fields a probing kernel reads, in one 32-byte line-aligned record (FilterDesc is 56
// bytes with the 64-bit modulus and the Redis-length pointer): the ordered stream's contains reads
// one per command of a random (Zipf) tenant.
struct alignas(32) ProbeDesc {
    const uint32_t *bm;
    ModC mc;
    uint32_t k;
    uint32_t fid;
};
static_assert(sizeof(ProbeDesc) == 32, "one half line");

struct alignas(16) HTEntry {
    unsigned long long tag;  // [63:56] epoch, [55:32] fid, [31:0] bit index
    unsigned long long idw;  // [63:32] 254 - epoch, [31:0] min key id
};

// ---- bloom_kernels.hip
// Contains, the table adds, the one-key kernels, the wide filters, BITCOUNT and the digest.
struct AddChunkArgs {
    KeysDev keys;
    uint64_t base, nchunk;
    const FilterDesc *filt;  // nullable: single filter
    const uint64_t *seg_off;
    uint32_t nseg;
    const uint32_t *tile_seg0;
    FilterDesc single;
    HTEntry *table;
    uint32_t log2cap, epoch;
    uint32_t *zmask;  // nchunk words (k <= 32) or nchunk*k bytes
    uint32_t kmax;
    uint8_t *out_new;
    unsigned long long *count;
    unsigned long long *seg_counts;
    bool narrow;  // single filter, k <= 32: 8-byte entries, table cleared per chunk
};

void launch_bloom_contains(const KeysDev &keys, int klen_fast, const uint32_t *bm, const ModParams &mp,
                           uint32_t k, uint8_t *out, unsigned long long *count, hipStream_t st);
// add(T) / contains(T): one key of one filter (k <= 16), one lane; an add needs no first-setter table
// (run_add, keys.n == 1).  done (nullable): seq is stored there last, at system scope (bloom_host_tiny)
void launch_bloom_one(bool add, const KeysDev &keys, int klen_fast, const FilterDesc &f, uint8_t *out,
                      unsigned long long *count, uint32_t *done, uint32_t seq, hipStream_t st);
// one store of seq into done (coherent host memory), after the stream's earlier work
void launch_done_word(uint32_t *done, uint32_t seq, hipStream_t st);
// tile_seg0[t] = segment holding key 256*t (precomputed once per multi-tenant batch)
void launch_tile_seg0(const uint64_t *seg_off, uint32_t nseg, uint64_t nkeys, uint32_t *tile_seg0, hipStream_t st);
void launch_bloom_contains_multi(const KeysDev &keys, int klen_fast, const FilterDesc *filt,
                                 const uint64_t *seg_off, uint32_t nseg, const uint32_t *tile_seg0, uint32_t kmax,
                                 uint8_t *out, unsigned long long *counts, hipStream_t st, bool slots);
void launch_bloom_add_chunk(const AddChunkArgs &a, int klen_fast, hipStream_t st);
// |size| > 2^32 filters (k_wide_*): add = first-setter claim + resolve over a 2^tlog2-entry table
// (all ~0 on entry); *oob = 1 when an index passes the Redis offset limit.  bm may be NULL for
// contains (a missing key).
void launch_bloom_wide(const KeysDev &keys, uint64_t m, uint32_t k, uint32_t *bm, unsigned long long *len,
                       unsigned long long *table, uint32_t tlog2, bool is_add, uint8_t *out,
                       unsigned long long *count, unsigned long long *oob, hipStream_t st);
void launch_bitcount(const uint8_t *bytes, uint64_t nbytes, unsigned long long *out, hipStream_t st);
// order-independent digest of a Redis string's bytes (replica comparison); *out += digest
void launch_digest(const uint8_t *bytes, uint64_t nbytes, unsigned long long *out, hipStream_t st);
void set_contains_stage1(int v);  // early-exit schedule of the staged contains; 5 = the slot kernel
int get_contains_stage1();
void set_contains_qgrid(int v);   // slot contains kernel grid (blocks)

// ---- contains_partitioned.hip
// One chunk of keys against one filter, one radix pass.  Stage 1 buckets pairs by 2^21-bit (256 KiB)
// bitmap region; the probe holds one 2^20-bit (128 KiB) slice of a region in LDS (bucket_common.h).
// The stage-1 tile (kBkTileKeys), grid and the 5-byte entry format are bk_entry.h's.
constexpr int kBkMissRangeBits = 19;   // probe misses are bucketed by 2^19-key range (64 KiB LDS bitmap)
struct PcArgs {
    KeysDev keys;
    uint64_t base, nchunk;
    const uint32_t *bm;
    ModParams mp;
    uint32_t k;
    uint32_t nb;            // regions (stage-1 buckets) = ceil(size / 2^21) <= 2048
    uint32_t grid1;         // stage-1 blocks G = min(tiles of the chunk, 256 or "contains_stage1_grid"); every block owns a
                            // segment per bucket, and nchunk <= G * 2^19 (a block-local key index fits 19 bits)
    uint64_t capS;          // entry capacity of one segment, a multiple of 12 (whole 64-byte lines)
    uint64_t nwords4;       // bitmap words rounded up to a multiple of 4
    unsigned long long *pairs;  // nb * G segments of capS / 12 lines of 12 entries (bk_entry.h): segment (b, blk) at line (blk*nb + b) * capS / 12
    uint32_t *segcnt;       // nb * G entry counts, all written by stage 1
    unsigned long long *alive;  // ceil(nchunk/64)
    unsigned long long *miss;   // ceil(nchunk/64), zeroed
    uint32_t *mrec;         // nmranges * capm: key ids of the probe's clear bits, by 2^19-key range
    uint32_t *mcnt;         // nmranges, zeroed
    uint64_t capm;
    uint32_t nmranges;      // ceil(nchunk / 2^kBkMissRangeBits) <= 256
    uint8_t *out;
    unsigned long long *count;
    uint32_t flags;  // diagnostics only (rbx_tune "contains_partition_flags"); 0 in normal operation
    unsigned long long *stamps;  // flags & 64: probe phase times (rbx_bench_add_stamps), else null
};
void launch_contains_partitioned_chunk(const PcArgs &a, int klen_fast, hipStream_t st);

// ---- add_partitioned.hip
// The partitioned single-filter add, one chunk of keys.  2^16-bit regions (8 KiB bitmap + two bitsets
// + a collision table = 32 KiB of LDS, two blocks per CU); at most 8 pairs per thread of the
// 1024-thread region block.
constexpr int kBaRegionBits = 16;
constexpr uint32_t kBaSub = 8;               // stage-1 sub-partitions per level-1 bucket
constexpr uint32_t kBaMaxRegionPairs = 8192;  // cap3 <= this
constexpr int kBaKeyRangeBits = 20;           // owner records are bucketed by 2^20-key range
struct BaArgs {
    KeysDev keys;
    uint64_t base, nchunk;
    FilterDesc f;                 // bm, redis_len, mp, k
    uint32_t ncoarse;             // level-1 buckets (<= 256, each kBaSub sub-partitions)
    uint32_t s1, s3;              // level-1 bucket = idx >> s1, region = idx >> s3 (s3 = kBaRegionBits)
    uint32_t f3;                  // fan-out bits of the rebucket (level 1 -> regions), <= 8
    uint32_t nregions;
    uint64_t cap1, cap3;
    unsigned long long *p1, *p3;  // level-1 and region pair arrays
    uint32_t *cnt1, *cnt3;        // zeroed per chunk
    uint32_t *new_bits;           // ceil(nchunk / 32) words, zeroed per chunk
    uint32_t *ctr;                // byte counter per key (nchunk rounded up to 32), all zero between calls
    uint32_t *recs, *rec_cnt;     // owner records: nranges x cap_rec key ids, counts (zeroed per chunk)
    uint64_t cap_rec;             // k x 2^20: a range's records never exceed it
    uint32_t nranges;             // 2^20-key ranges of the chunk
    uint32_t *overflow;           // zeroed; set when a pair does not fit (the chunk then reruns on the table path)
    uint32_t *mode;               // written by k_ba_mode: 1 non-owner counters, 2 owner records, 0 owner bits
    uint32_t record_policy;       // rbx_tune "add_records": 0 owner bits, 1 counters, 3 owner records, 2 from the sampled fill
    uint64_t nwords4;             // bitmap words rounded up to a multiple of 4
    uint8_t *out_new;
    unsigned long long *count;
    uint32_t diag;                // diagnostics only (rbx_tune "add_partition_diag"); 0 in normal operation
    unsigned long long *stamps;   // diagnostics only (add_partition_diag & 64): region-pass phase times, else null
};
void launch_add_partitioned_chunk(const BaArgs &a, int klen_fast, hipStream_t st);
void set_add_region_grid(int v);    // 256..65536 (default 2048)
void set_add_rec_lds_limit(int v);  // 0..7168 (tests)

// ---- stream_kernels.hip
// The ordered mixed contains/add stream and the multi-tenant add on the 8-byte table (one chunk of keys
// each).
struct StreamChunkArgs {
    KeysDev keys;
    uint64_t base, nchunk;
    const FilterDesc *filt;
    const ProbeDesc *pdesc;  // the same filters' probe fields (stream contains)
    const uint32_t *kf;   // per key: index into filt
    const uint8_t *op;    // per key: 0 contains, 1 add
    HTEntry *table;
    uint32_t log2cap, epoch;
    uint32_t *zmask;      // per add-list entry
    uint32_t kmax;
    uint8_t *out;         // per key: present (contains) / newly added (add)
    unsigned long long *counts;  // [0] present contains, [1] new adds
    uint32_t *adds;       // nchunk: compacted chunk-local positions of the adds
    uint32_t *nadds;      // 1, zeroed per chunk
    // r04 first-setter table of 8-byte entries (null: the 16-byte epoch-tagged `table` above).
    // entry = (fid << bb | bit) << pb | chunk position, EMPTY = ~0; one CAS claims a bit, and an
    // atomicMin keeps the first setter of a shared one.  Capacity 2^t8_log2(*nadds, kmax), from the
    // chunk's add count on the device; k_stream_walk commits it and restores every entry to EMPTY.
    unsigned long long *t8;
    uint32_t bb, pb;              // bits of the largest bitmap's bit index / of a chunk position
    uint32_t tkmax;               // sizes the table: 2^t8_log2(*nadds, tkmax), tkmax = kmax x table scale
    uint32_t *const *fid_bm;      // bitmap words per table id (fid)
    uint32_t *fslot;              // per add-list entry: the table slot of its first zero bit's claim (r05)
};
// entries of the 8-byte stream table for a chunk of nadds adds (load <= 8/9 even if every bit is 0)
__host__ __device__ inline uint32_t t8_log2(uint32_t nadds, uint32_t kmax) {
    const uint64_t need = (uint64_t)nadds * kmax;
    const uint64_t want = need + need / 8;
    uint32_t lg = 12;
    while ((1ULL << lg) < want) ++lg;
    return lg;
}

void launch_stream_chunk(const StreamChunkArgs &a, int klen_fast, hipStream_t st);

// state of the optimistic multi-tenant add's conflict table (k_maddx_*), reset per chunk
struct MaddxState {
    uint32_t count;     // entries inserted into C
    uint32_t overflow;  // C too full (or a probe run too long): the full table T decides the chunk
};
// One chunk of a multi-tenant add on the 8-byte first-setter table (r05, k_maddx_*):
// probe (claims) -> final (replies, per-segment counts) -> walk (OR owned bits, empty the table).
struct MaddChunkArgs {
    KeysDev keys;
    uint64_t base, nchunk;
    const FilterDesc *filt;
    const uint64_t *seg_off;
    uint32_t nseg;
    const uint32_t *tile_seg0;
    uint32_t kmax;
    unsigned long long *t8;   // 2^lg entries, EMPTY before and after the chunk
    uint32_t lg, bb, pb;
    uint32_t *const *fid_bm;  // bitmap words per filter id
    uint32_t *zmask, *fslot;  // per key of the chunk
    uint8_t *out_new;
    unsigned long long *seg_counts;
    // r05 optimistic SETBITs with conflict repair (k_maddx_*): non-null = that path, with the small
    // conflict table C of 2^lgC entries and its state word; t8 / lg then serve only an overflowed chunk
    unsigned long long *c8;
    uint32_t lgC;
    MaddxState *cst;
    // r05 per-segment path (k_madd_seg) in front: non-null = every k_maddx_* kernel returns unless *big
    // (a segment past segmax exists), and handles only the keys of such segments
    const uint32_t *big;
    uint64_t segmax;
};
void launch_madd8_chunk(const MaddChunkArgs &a, int klen_fast, hipStream_t st);
void set_stream_diag(int v);        // profiling build only (kDiag): bits 1 | 8, see stream_kernels.hip
void set_stream_final_grid(int v);  // k_stream_final8 blocks (32..2048)
void set_stream_qgrid(int v);       // slot stream-contains kernel grid (blocks)

// ---- segment_add.hip
// The per-segment multi-tenant add (k_madd_seg): one 256-thread workgroup per segment, every filter of
// the batch in one segment only (disjoint bitmaps), k <= 16; segments past segmax (<= kSegMaxKeys) keys
// set *big and are left to the k_maddx_* chunks.
constexpr uint32_t kSegMaxKeys = 16384;
struct MaddSegArgs {
    KeysDev keys;
    const FilterDesc *filt;
    const uint64_t *seg_off;
    uint32_t nseg, kmax;
    uint32_t grid;            // workgroups (grid-stride over the segments)
    uint64_t segmax;
    uint8_t *out_new;
    unsigned long long *seg_counts;
    uint32_t *big;            // zeroed before the launch
    // filt == nullptr: one filter passed by value and one segment, all of `keys` (seg_off unused; the
    // small single-filter adds of run_add and bloom_host_tiny, keys.n <= segmax)
    FilterDesc single;
};
void launch_madd_seg(const MaddSegArgs &a, int klen_fast, hipStream_t st);

// ---- bitset_kernels.hip
// RBitSet over bitmap strings.
struct BitopSrc {
    const uint8_t *bytes;  // a source string (null when the key is missing)
    uint64_t len;          // its Redis length: nothing at or past it is read
};
// BITOP: dst[0, out_len) := op (RBX_BITOP_* of rbx.h) over the nsrc sources of the device table
// d_srcs, dst[out_len, span) := 0, *dst_len := out_len.  span: a multiple of 16 within dst's
// allocation covering out_len and dst's previous length.  dst may be any of the sources.
void launch_bitop(int op, uint8_t *dst, unsigned long long *dst_len, const BitopSrc *d_srcs, uint32_t nsrc,
                  uint64_t out_len, uint64_t span, hipStream_t st);
// bits [from, to) := value, from < to <= 8 * capacity; *len = max(*len, bytes up to `to`)
void launch_bits_fill(uint32_t *words, unsigned long long *len, uint64_t from, uint64_t to, bool value, hipStream_t st);
// SETBIT d_idx[i] value for n indexes below cap_bits; *len = max(*len, new_len)
void launch_bits_scatter(uint32_t *words, unsigned long long *len, uint64_t cap_bits, const uint64_t *d_idx, uint64_t n,
                         bool value, uint64_t new_len, hipStream_t st);
// d_out[i] = GETBIT d_idx[i] (0 at or past cap_bits)
void launch_bits_gather(const uint32_t *words, uint64_t cap_bits, const uint64_t *d_idx, uint64_t n, uint8_t *d_out,
                        hipStream_t st);
// *d_out = max(*d_out, max of the n indexes)
void launch_bits_max(const uint64_t *d_idx, uint64_t n, unsigned long long *d_out, hipStream_t st);
// SETBIT bit value; *d_old = the bit before
void launch_bits_set_one(uint32_t *words, unsigned long long *len, uint64_t bit, bool value, unsigned long long *d_old,
                         hipStream_t st);
// ---- cell_sort.hip
// What every grouped path below shares.  Commands on different cells are independent, those on one cell totally
// ordered: a pairs kernel emits (cell, position), a stable radix sort by cell lists each cell's commands in array
// order, and a runs kernel gives each run of equal cells to the lane at its head.  The cell encodings and the
// runs kernels are each path's own; the sort and its scratch are here.  Cell: uint32_t (the single-key BITFIELD
// batch's slots) or unsigned long long (the streams' cells); positions are 32-bit, n <= 2^30.
// A caller's scratch: cell_in | cell_out | pos_in | pos_out, each rounded up to 256 bytes, then rocPRIM's
// temporary storage.
inline size_t cell_sort_array_bytes(uint32_t n, size_t elem) { return ((size_t)n * elem + 255) & ~(size_t)255; }
template <class Cell> struct CellSortBufs {
    Cell *cell_in, *cell_out;
    uint32_t *pos_in, *pos_out;
    void *temp;
    size_t temp_bytes;
};
// the scratch for n pairs sorted over the cells' bits [begin_bit, end_bit); 0 or a hipError_t
template <class Cell> int cell_sort_scratch_bytes(uint32_t n, int begin_bit, int end_bit, size_t *bytes);
// carves a scratch of at least that size; hipErrorInvalidValue when it cannot hold the four arrays
template <class Cell> int cell_sort_carve(void *d_scratch, size_t scratch_bytes, uint32_t n, CellSortBufs<Cell> *b) {
    const size_t cb = cell_sort_array_bytes(n, sizeof(Cell)), pb = cell_sort_array_bytes(n, 4);
    if (scratch_bytes < 2 * cb + 2 * pb) return (int)hipErrorInvalidValue;
    uint8_t *s = (uint8_t *)d_scratch;
    *b = CellSortBufs<Cell>{(Cell *)s, (Cell *)(s + cb), (uint32_t *)(s + 2 * cb), (uint32_t *)(s + 2 * cb + pb),
                            s + 2 * cb + 2 * pb, scratch_bytes - 2 * cb - 2 * pb};
    return 0;
}
// (cell_in, pos_in) -> (cell_out, pos_out), stable and stream-ordered, looking at bits [begin_bit, end_bit) only;
// 0 or a hipError_t
template <class Cell> int cell_sort(const CellSortBufs<Cell> &b, uint32_t n, int begin_bit, int end_bit, hipStream_t st);

// bitfield_kernels.hip -- BITFIELD GET / SET / INCRBY (RBX_FIELD_* of rbx.h) on fields of one type;
// `words` / cap_bytes: a bitmap's allocation, which already holds every field written
// d_out2[0] = max(d_out2[0], max offset), d_out2[1] |= 1 when an offset is no multiple of size; with
// d_vals (nullable; k_fields_check_signs) also |= 2 when a value is > 0 and |= 4 when one is < 0
void launch_fields_check(const uint64_t *d_offs, const int64_t *d_vals, uint64_t n, int size,
                         unsigned long long *d_out2, hipStream_t st);
// d_out[i] = GET at d_offs[i], any offsets (bits at or past the allocation read as zero)
void launch_fields_get(const uint32_t *words, uint64_t cap_bytes, const uint64_t *d_offs, uint64_t n, int size,
                       int is_signed, int64_t *d_out, hipStream_t st);
// INCRBY without replies; offsets multiples of size, size a divisor of 64; *len = max(*len, new_len)
void launch_fields_incr_atomic(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, const uint64_t *d_offs,
                               const int64_t *d_incs, uint64_t n, int size, uint64_t new_len, hipStream_t st);
// the same under OVERFLOW SAT; every increment has one sign (>= 0 or <= 0)
void launch_fields_incr_sat(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, const uint64_t *d_offs,
                            const int64_t *d_incs, uint64_t n, int size, int is_signed, uint64_t new_len,
                            hipStream_t st);
// SET / INCRBY in array order on offsets that are multiples of size, n <= 2^30: a stable sort by
// slot (slot_bits = the significant bits of the largest offset / size), then one lane per slot.
// d_replies nullable.  mode = RBX_OVERFLOW_*; under FAIL d_nil[i] (nullable) = reply i is nil.  The
// scratch: cell_sort_scratch_bytes<uint32_t>(n, 0, slot_bits).  Returns 0 or a hipError_t.
int launch_fields_grouped(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, int op, int is_signed,
                          int size, int mode, const uint64_t *d_offs, const int64_t *d_values, uint32_t n,
                          int64_t *d_replies, uint8_t *d_nil, uint64_t new_len, int slot_bits, void *d_scratch,
                          size_t scratch_bytes, hipStream_t st);
// SET / INCRBY in array order at any offsets, one lane (exact for partly overlapping fields)
void launch_fields_serial(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, int op, int is_signed, int size,
                          int mode, const uint64_t *d_offs, const int64_t *d_values, uint64_t n, int64_t *d_replies,
                          uint8_t *d_nil, uint64_t new_len, hipStream_t st);
// n sub-commands of any operations, types and modes in array order, one lane; d_replies and d_nil
// get one entry each.  words = null with cap_bytes = 0 and new_len = 0: a missing key under GETs only
void launch_bitfield_serial(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, const rbx_field_cmd *d_cmds,
                            uint64_t n, int64_t *d_replies, uint8_t *d_nil, uint64_t new_len, hipStream_t st);
// one SET / INCRBY; *d_reply = its reply
void launch_field_one(uint32_t *words, unsigned long long *len, uint64_t cap_bytes, int op, int is_signed, int size,
                      uint64_t offset, int64_t value, int64_t *d_reply, uint64_t new_len, hipStream_t st);

// ---- bitrange_kernels.hip
// Ranged BITCOUNT / BITPOS ([redis-7.2] bitops.c bitcountCommand / bitposCommand as DESIGN §11.2 restates
// them).  The reply rules are host and device code: single calls and the host-string forms apply them on the
// host, the batch kernels in their query prologue.  unit: RBX_RANGE_BYTE (0) or RBX_RANGE_BIT of rbx.h.
// (kBitsNone and the bits_* range rules: range_cmd.h, which compiles without HIP)
// the directory's 4 KiB blocks over a string of len bytes; the directory holds one more word than that
RBX_HD uint64_t bits_dir_blocks(uint64_t len) { return (len + 4095) >> 12; }
// Every interval below is normalised: lo <= hi < 8 * length.
// *d_out += the ones of [lo, hi] (the caller zeroes it)
void launch_bits_count_range(const uint32_t *words, uint64_t lo, uint64_t hi, unsigned long long *d_out, hipStream_t st);
// *d_out = the first position of [lo, hi] holding `bit`, or none_reply.  d_state: kBitsPosStateBytes of scratch
// that the caller has set to all ones (the running minimum, the chunk ticket, the count of finished
// workgroups); chunk_bytes: a power of two >= 4096
constexpr size_t kBitsPosTicketAt = 16, kBitsPosDoneAt = 32, kBitsPosStateBytes = 384;  // u64 indexes: 128 bytes apart
void launch_bits_pos(const uint32_t *words, uint64_t lo, uint64_t hi, int bit, uint32_t chunk_bytes,
                     unsigned long long *d_state, int64_t none_reply, int64_t *d_out, hipStream_t st);
// d_dir[b] = the ones below 4 KiB block b, b = 0 .. bits_dir_blocks(len) (len > 0)
void launch_bits_directory(const uint32_t *words, uint64_t len, unsigned long long *d_dir, hipStream_t st);
// the directory's scan alone: d_counts[0 .. n) := their exclusive prefix sums, d_counts[n] := their sum
void launch_bits_scan(unsigned long long *d_counts, uint32_t n, hipStream_t st);
// d_out3 (zeroed by the caller) = {*d_len, sum of bits_interval_bytes, their maximum}; d_ends nullable (pos)
void launch_bits_ranges_summary(const int64_t *d_starts, const int64_t *d_ends, uint64_t n, int unit, bool pos,
                                const unsigned long long *d_len, unsigned long long *d_out3, hipStream_t st);
// d_out[i] = BITCOUNT / BITPOS reply of query i over a string of len > 0 bytes, one wave per query; d_dir
// null = walk the interval, else the directory of launch_bits_directory.  pos: d_ends null = "bit start"
void launch_bits_count_ranges(const uint32_t *words, uint64_t len, const int64_t *d_starts, const int64_t *d_ends,
                              uint64_t n, int unit, const unsigned long long *d_dir, uint64_t *d_out, hipStream_t st);
void launch_bits_pos_ranges(const uint32_t *words, uint64_t len, int bit, const int64_t *d_starts, const int64_t *d_ends,
                            uint64_t n, int unit, const unsigned long long *d_dir, int64_t *d_out, hipStream_t st);

// ---- members_kernels.hip
// Set-bit enumeration and the java.util.BitSet exchange (rules: members_rule.h).
// [lo, hi] is normalised over a string of len > 0 bytes and d_dir is launch_bits_directory's over that string.
// d_state (kMembersStateWords u64) = {the ones below lo, the page's first rank, its end rank} for the expand
// kernel; d_counts = {written, total} with written = min(cap, total - min(skip, total)).
constexpr size_t kMembersStateWords = 3;
constexpr unsigned kMembersMaxGrid = 8192;  // the expand kernel's grid-stride cap: a block outside the page costs two loads
void launch_members_head(const uint32_t *words, uint64_t len, uint64_t lo, uint64_t hi, uint64_t skip, uint64_t cap,
                         const unsigned long long *d_dir, unsigned long long *d_state, unsigned long long *d_counts,
                         hipStream_t st);
// d_out[r - first] = the position of the interval's one of rank r, for the page's ranks [first, end) of d_state
void launch_members_expand(const uint32_t *words, uint64_t len, uint64_t lo, uint64_t hi, const unsigned long long *d_dir,
                           const unsigned long long *d_state, uint64_t *d_out, hipStream_t st);
// *d_nwords (zeroed by the caller) = BitSet's words in use of the string at `words` (its length: *d_len)
void launch_words_last(const uint32_t *words, uint64_t cap_bytes, const unsigned long long *d_len,
                       unsigned long long *d_nwords, hipStream_t st);
// d_out[0 .. min(cap_words, *d_nwords)) = those words, *d_nwords read on the device
void launch_words_export(const uint32_t *words, uint64_t cap_bytes, const unsigned long long *d_nwords, uint64_t cap_words,
                         uint64_t *d_out, hipStream_t st);
// *d_highest1 (zeroed by the caller) = 1 + the highest set bit of the n words, 0 = none
void launch_words_highest(const uint64_t *d_words, uint64_t n, unsigned long long *d_highest1, hipStream_t st);
// the string of `bytes` bytes of the n words into a zeroed allocation of at least that size; *d_len = bytes
void launch_words_import(const uint64_t *d_words, uint64_t n, uint64_t bytes, uint32_t *words, unsigned long long *d_len,
                         hipStream_t st);

// Many keys (rbx_bitset_members_stream): command i is (d_key[i], d_cmds[i]) over the BitKey table below, n <= 2^30
// commands per chunk, in the range stream's two tiers with its summary words (below): the one "first" word is the
// first command on a key of another type.
struct BitKey;
constexpr int kMsFirsts = 1;
// d_off[i] = command i's yield (0 for a listed long command, whose (first tile << kRsPosBits | position) goes to
// d_long, ascending); d_status[i] (nullable) = 0, or 0xFF on a key of another type
void launch_members_count(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds, uint32_t n,
                          uint32_t nkeys, uint32_t short_max, uint32_t tile_bytes, unsigned long long *d_off,
                          uint8_t *d_status, unsigned long long *d_sum, unsigned long long *d_long, hipStream_t st);
// d_tiles[t] = the ones of its command before flattened tile t (ntiles entries); d_off[i] = the yield of each listed command
void launch_members_tiles_count(const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds, uint32_t tile_bytes,
                                const unsigned long long *d_long, uint32_t nlong, uint64_t ntiles,
                                unsigned long long *d_tiles, unsigned long long *d_off, hipStream_t st);
// d_off[0 .. m1) += *d_carry
void launch_members_carry(unsigned long long *d_off, uint64_t m1, const unsigned long long *d_carry, hipStream_t st);
// the positions of the commands not listed / listed, from the final d_off (n + 1 entries): d_out[d_off[i] ..
// d_off[i + 1]) as far as below cap
void launch_members_expand_short(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds,
                                 uint32_t n, uint32_t short_max, const unsigned long long *d_off, uint64_t *d_out,
                                 uint64_t cap, hipStream_t st);
void launch_members_expand_tiles(const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds,
                                 uint32_t tile_bytes, const unsigned long long *d_long, uint32_t nlong, uint64_t ntiles,
                                 const unsigned long long *d_tiles, const unsigned long long *d_off, uint64_t *d_out,
                                 uint64_t cap, hipStream_t st);

// ---- bitstream_kernels.hip
// The ordered GETBIT / SETBIT stream over many strings (rbx_bitset_stream).  Commands are
// (key, op, index) with op 0 = GETBIT, 1 = SETBIT index 0, 2 = SETBIT index 1; a reply is the bit, the bit
// before, or 0xFF for a command that failed alone.
// One string of the batch as the kernels see it, one record per entry of `names` (a missing key that is
// only read: words = len = null, cap_bits = 0, and every bit reads 0).
struct alignas(32) BitKey {
    uint32_t *words;
    uint64_t cap_bits;        // 8 * the allocation's bytes: every SETBIT of the batch lies below it
    unsigned long long *len;  // device word: Redis string length in bytes
    uint32_t flags;           // kBitKeyWrong
    uint32_t canon;           // the first entry of `names` with this entry's bytes (its own index if none is earlier)
};
static_assert(sizeof(BitKey) == 32, "one half line");
constexpr uint32_t kBitKeyWrong = 1;  // the key holds another type: its commands fail
// the summary words (u64) and the bits of the flags word
enum { kBsFirstOob = 0, kBsFirstWrong = 1, kBsFlags = 2, kBsMaxIndex = 3, kBsSummaryWords = 4 };
constexpr uint32_t kBsIllegal = 1, kBsHasGet = 2, kBsHasSet0 = 4, kBsHasSet1 = 8;
// One pass before anything is written.  d_sum (the caller sets words 0 and 1 to ~0, 2 and 3 to 0):
// [kBsFirstOob] the first position whose index is >= 2^32, [kBsFirstWrong] the first position on a key
// with d_wrong set (and an index below 2^32), [kBsFlags] kBsIllegal = some key >= nkeys or op > 2, kBsHas*
// = the legal commands' operations, [kBsMaxIndex] the largest index of a command that does not fail.
// d_keymax (nkeys words, zeroed): per canonical key, 1 + its largest SETBIT index among those.
void launch_bitstream_summary(const uint32_t *d_key, const uint8_t *d_op, const uint64_t *d_idx, uint64_t n,
                              uint32_t nkeys, const uint32_t *d_canon, const uint8_t *d_wrong,
                              unsigned long long *d_sum, unsigned long long *d_keymax, hipStream_t st);
// a batch of GETBITs
void launch_bitstream_gather(const BitKey *d_tab, const uint32_t *d_key, const uint64_t *d_idx, uint64_t n,
                             uint8_t *d_replies, hipStream_t st);
// a batch of SETBITs of one value whose replies are not wanted
void launch_bitstream_scatter(const BitKey *d_tab, const uint32_t *d_key, const uint64_t *d_idx, uint64_t n, bool value,
                              hipStream_t st);
// any batch in array order, one lane; d_replies nullable
void launch_bitstream_serial(const BitKey *d_tab, const uint32_t *d_key, const uint8_t *d_op, const uint64_t *d_idx,
                             uint64_t n, uint8_t *d_replies, hipStream_t st);
// any batch of n <= 2^30 commands: a stable sort by cell = canon << index_bits | index, then one lane per
// cell.  index_bits: the significant bits of the largest index (1..32); key_bits: those of nkeys - 1 (<= 31);
// has_failed: some command of the batch fails.  The scratch: cell_sort_scratch_bytes<unsigned long long>(n, 0,
// index_bits + key_bits + has_failed).  Returns 0 or a hipError_t.
int launch_bitstream_grouped(const BitKey *d_tab, const uint32_t *d_key, const uint8_t *d_op, const uint64_t *d_idx,
                             uint32_t n, uint8_t *d_replies, int index_bits, int key_bits, bool has_failed,
                             void *d_scratch, size_t scratch_bytes, hipStream_t st);
// *len = max(*len, bytes up to the key's largest SETBIT) for every key with an entry in d_keymax
void launch_bitstream_lengths(const BitKey *d_tab, const unsigned long long *d_keymax, uint32_t nkeys, hipStream_t st);

// ---- rangestream_kernels.hip
// The read queries over many strings (rbx_bitset_range_stream): command i is (key[i], cmds[i]),
// the strings are reached through the BitKey table above, range_cmd.h has the rules.
// The summary words (u64) of one chunk of a two-tier read stream (this one and the members stream): nfirst "first
// position" minima (here one per failure kind, kRange* - 1; preset to ~0, the others to 0), the flags, and one
// word that hands out the long list's slots and the tile numbers together: long commands << kRsTileBits | tiles
constexpr int rs_flags_at(int nfirst) { return nfirst; }
constexpr int rs_long_at(int nfirst) { return nfirst + 1; }
constexpr int rs_summary_words(int nfirst) { return nfirst + 2; }
constexpr uint32_t kRsIllegal = 1;
constexpr int kRsTileBits = 33, kRsPosBits = 30;  // a chunk has <= 2^30 commands and fewer than 2^33 tiles
// the two streams' launchers: a tile's log2 (a power of two), the "lanes" knob to LAUNCH(G); grid: grid_for(n * G)
inline uint32_t log2_of(uint32_t pow2) { return (uint32_t)__builtin_ctz(pow2); }
#define RBX_FOR_LANES(lanes, LAUNCH)    \
    if ((lanes) == 4) LAUNCH(4);        \
    else if ((lanes) == 8) LAUNCH(8);   \
    else if ((lanes) == 32) LAUNCH(32); \
    else if ((lanes) == 64) LAUNCH(64); \
    else LAUNCH(16)
// One group of `lanes` lanes (4, 8, 16, 32 or 64) per command, n <= 2^30: every command whose interval covers
// at most short_max bytes is answered (d_replies, d_status nullable); a longer one presets its reply (0 for
// COUNT, kBitsNone for POS) and appends (first tile << kRsPosBits | position) to d_long (n entries), ascending.
void launch_rangestream_short(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_range_cmd *d_cmds,
                              uint32_t n, uint32_t nkeys, uint32_t short_max, uint32_t tile_bytes, int64_t *d_replies,
                              uint8_t *d_status, unsigned long long *d_sum, unsigned long long *d_long, hipStream_t st);
// the long commands' tiles (ntiles > 0 in all, nlong commands) swept by the whole grid, then one lane per long POS
// command turns the minimum into its reply
void launch_rangestream_tiles(const BitKey *d_tab, const uint32_t *d_key, const rbx_range_cmd *d_cmds,
                              uint32_t tile_bytes, const unsigned long long *d_long, uint32_t nlong, uint64_t ntiles,
                              int64_t *d_replies, hipStream_t st);

// ---- bytestream_kernels.hip
// GETRANGE / SETRANGE / APPEND / GET over many strings (rbx_string_stream): command i is (key[i],
// cmds[i]), the strings are reached through the BitKey table above, byte_cmd.h has the rules.
// A key's running state through the plan: its length, whether it exists now and whether a command that runs writes
// it (the host creates or grows it to `len`; the lengths kernel stores `len`); nlong is the serial plan's own.
struct ByteKeyState {
    unsigned long long len;
    uint32_t flags, nlong;
};
constexpr uint32_t kByExists = 1, kByWritten = 2;
// The summary words (u64) of one chunk: the first position per failure kind (kByte* - 1; preset to ~0, the others to
// 0), the flags (kRsIllegal), the chunk's long commands, their tiles, the most long commands on one key; then two
// words the rounds use: the round's list word (long commands << kRsTileBits | tiles) and the number of runs.
enum { kByFlags = kByteKinds, kByLongCmds, kByTiles, kByMostLong, kByList, kByHeads, kBySummaryWords };
// the single calls: cnt bytes from src to dst in tiles over the grid, then *d_len (nullable) = new_len
void launch_bytes_copy(uint8_t *dst, const uint8_t *src, uint64_t cnt, uint32_t tile_bytes, unsigned long long *d_len,
                       uint64_t new_len, hipStream_t st);
// d_state[i] = canonical key i's length and existence (nkeys entries)
void launch_bytestream_state_init(const BitKey *d_tab, uint32_t nkeys, ByteKeyState *d_state, hipStream_t st);
// The chunk's m <= 2^30 commands sorted by canonical key into the scratch (cell_sort_scratch_bytes<uint32_t>(m, 0,
// key_bits), key_bits = the significant bits of nkeys: a command that is the caller's error takes cell nkeys and
// sets kRsIllegal).  The three launchers below read the sorted pairs from the same scratch.  0 or a hipError_t.
int launch_bytestream_sort(const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds, uint32_t m,
                           uint32_t nkeys, uint64_t vals_len, int key_bits, unsigned long long *d_sum, void *d_scratch,
                           size_t scratch_bytes, hipStream_t st);
// One lane per key's run plans it from d_state: d_plan / d_yield (the bytes a read yields, for the scan) / d_replies /
// d_status (nullable) are the chunk's slices, i0 its first position in the call.  Nothing is written to a string.
int launch_bytestream_plan(const BitKey *d_tab, const rbx_string_cmd *d_cmds, uint32_t m, uint32_t nkeys, uint64_t i0,
                           uint32_t short_max, uint32_t tile_bytes, ByteKeyState *d_state, unsigned long long *d_plan,
                           unsigned long long *d_yield, int64_t *d_replies, uint8_t *d_status, unsigned long long *d_sum,
                           void *d_scratch, size_t scratch_bytes, hipStream_t st);
// the same for a whole call of few commands in array order, one lane, without the sort
void launch_bytestream_plan_serial(const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds, uint32_t m,
                                   uint32_t nkeys, uint64_t vals_len, uint32_t short_max, uint32_t tile_bytes,
                                   ByteKeyState *d_state, unsigned long long *d_plan, unsigned long long *d_yield,
                                   int64_t *d_replies, uint8_t *d_status, unsigned long long *d_sum, hipStream_t st);
// the runs of the sorted chunk: d_cur (m entries) gets each head's cursor, d_heads (m entries) the heads, *d_nheads
// (zeroed by the caller) their number
int launch_bytestream_heads(uint32_t m, uint32_t nkeys, uint32_t *d_cur, uint32_t *d_heads, unsigned long long *d_nheads,
                            void *d_scratch, size_t scratch_bytes, hipStream_t st);
// One round's walk: a group of `lanes` lanes per run executes its short commands from the cursor and lists its next
// long one in d_long (m entries) through *d_list (zeroed by the caller).  d_cmds / d_plan / d_off are the chunk's
// slices; d_off holds the final offsets into d_out.
int launch_bytestream_walk(int lanes, const BitKey *d_tab, const rbx_string_cmd *d_cmds, const uint8_t *d_vals,
                           const unsigned long long *d_plan, const unsigned long long *d_off, uint8_t *d_out, uint32_t m,
                           uint32_t *d_cur, const uint32_t *d_heads, const unsigned long long *d_nheads,
                           uint32_t tile_bytes, unsigned long long *d_list, unsigned long long *d_long, void *d_scratch,
                           size_t scratch_bytes, hipStream_t st);
// a whole call of few commands, none of them long, in array order by one group
void launch_bytestream_walk_serial(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds,
                                   const uint8_t *d_vals, const unsigned long long *d_plan, const unsigned long long *d_off,
                                   uint8_t *d_out, uint32_t m, hipStream_t st);
// the tiles of the commands the walk just listed, swept by the whole grid (the list word is read on the device)
void launch_bytestream_tiles(const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds, const uint8_t *d_vals,
                             const unsigned long long *d_plan, const unsigned long long *d_off, uint8_t *d_out,
                             uint32_t tile_bytes, const unsigned long long *d_list, const unsigned long long *d_long,
                             hipStream_t st);
// *len = the planned final length for every key a command that ran writes
void launch_bytestream_lengths(const BitKey *d_tab, const ByteKeyState *d_state, uint32_t nkeys, hipStream_t st);

// ---- fieldstream_kernels.hip
// The ordered stream of single-sub-command BITFIELDs over many strings (rbx_bitset_field_stream, DESIGN
// §11.6).  Command i is (key[i], cmds[i]); a reply is what rbx_bitset_bitfield with that one sub-command
// returns, a status 0, 1 (nil) or 0xFF (the command failed alone; its reply is 0).  The strings are reached
// through the BitKey table above.
// a command's failure kinds: field_rule.h's kFieldCmdBadType / kFieldCmdBadOffset, then the key's type
constexpr int kFsBadType = 1, kFsBadOffset = 2, kFsWrongType = 3;
// the summary words (u64) and the bits of the flags word
enum { kFsFirstType = 0, kFsFirstOffset = 1, kFsFirstWrong = 2, kFsFlags = 3, kFsSizes = 4, kFsMaxWord = 5,
       kFsSummaryWords = 6 };
constexpr uint32_t kFsIllegal = 1, kFsHasGet = 2, kFsHasSet = 4, kFsHasIncr = 8;  // kFsHasGet << op
constexpr uint32_t kFsWrap = 16, kFsSat = 32, kFsFail = 64;                         // kFsWrap << overflow
constexpr uint32_t kFsStraddles = 128, kFsUnaligned = 256;
// One pass before anything is written.  d_sum (the caller sets words 0..2 to ~0, the others to 0):
// [kFsFirst*] the first position of each failure kind, [kFsFlags] kFsIllegal = some key >= nkeys, op or
// overflow > 2 or is_signed > 1; and over the commands that run: kFsHas* their operations, kFsWrap / Sat /
// Fail the modes of their SETs and INCRBYs, kFsStraddles = some field crosses an aligned 64-bit word,
// kFsUnaligned = some offset is no multiple of its size; [kFsSizes] bit size - 1 per size that occurs;
// [kFsMaxWord] the largest 64-bit word index a field reaches.  d_keymax (nkeys words, zeroed): per canonical
// key the largest offset + size among its SETs and INCRBYs that run, which is what
// launch_bitstream_lengths takes (1 + the last bit written).
void launch_fieldstream_summary(const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n, uint32_t nkeys,
                                const uint32_t *d_canon, const uint8_t *d_wrong, unsigned long long *d_sum,
                                unsigned long long *d_keymax, hipStream_t st);
// d_replies and d_status are nullable everywhere below.
// a batch whose running commands are all GETs
void launch_fieldstream_gather(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n,
                               int64_t *d_replies, uint8_t *d_status, hipStream_t st);
// a batch whose running commands are all INCRBYs under WRAP of ONE size dividing 64 at multiples of it, the
// replies not wanted: any order
void launch_fieldstream_incr_atomic(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n,
                                    uint8_t *d_status, hipStream_t st);
// any batch in array order, one lane
void launch_fieldstream_serial(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint64_t n,
                               int64_t *d_replies, uint8_t *d_status, hipStream_t st);
// any batch of n <= 2^30 commands: a stable sort by cell, then one lane per cell.  word_bits > 0: cell = canon
// << word_bits | offset >> 6 (word_bits = the significant bits of [kFsMaxWord], at least 1; the batch must not
// have kFsStraddles); word_bits = 0: cell = canon.  key_bits: the significant bits of nkeys - 1, at least 1;
// has_failed: some command of the batch fails.  The scratch: cell_sort_scratch_bytes<unsigned long long>(n, 0,
// word_bits + key_bits + has_failed).  Returns 0 or a hipError_t.
int launch_fieldstream_grouped(const BitKey *d_tab, const uint32_t *d_key, const rbx_field_cmd *d_cmds, uint32_t n,
                               int64_t *d_replies, uint8_t *d_status, int word_bits, int key_bits, bool has_failed,
                               void *d_scratch, size_t scratch_bytes, hipStream_t st);

// ---- bench_kernels.hip
// Roofline probes (api_bench.cpp only).
// region-local gathers: 6 loads per lane inside XCD-assigned regions (partitioned-probe roofline)
void launch_gather_regions(const uint32_t *tbl, uint64_t nwords, uint64_t region_words, uint64_t total_lanes,
                           uint32_t *sink, hipStream_t st, unsigned grid);
// 4 random 4-byte gathers per key inside the key's segment (keys_per_seg consecutive keys share
// one seg_words slice): the request roofline of multi-tenant batches at their locality
void launch_gather_segments(const uint32_t *tbl, uint64_t nwords, uint64_t seg_words, uint64_t keys_per_seg,
                            uint64_t nkeys, uint32_t *sink, hipStream_t st);
// slice-probe roofline: per bucket b, stream 8-byte entries and test one word of bitmap slice b
void launch_bench_slice_probe(const void *ent, uint64_t per_bucket, uint32_t nbuckets, const uint32_t *bm,
                              uint32_t slice_words_log2, unsigned grid, uint32_t *sink, hipStream_t st);
// streaming 16-byte reads of a whole buffer: the HBM stream-read roofline probe
void launch_stream_read(const void *buf, uint64_t bytes, uint32_t *sink, hipStream_t st);
void launch_stream_write(void *buf, uint64_t bytes, hipStream_t st);
// random 4-byte gathers (k per key, nkeys keys) over an nwords-word table: roofline probe
void launch_gather_probe(const uint32_t *tbl, uint64_t nwords, uint64_t nkeys, uint32_t k, uint32_t *sink,
                         hipStream_t st);

// ---- hll_kernels.hip
// MurmurHash64A of element i (ELEN: the fixed 16-byte-aligned length of with_klen<true>, 0 = any)
template <int ELEN>
__device__ __forceinline__ uint64_t elem_hash(const KeysDev &e, uint64_t i) {
    if constexpr (ELEN > 0) {
        return murmur_fixed<ELEN>(e.bytes + i * (uint64_t)ELEN);
    } else {
        uint64_t a, len;
        if (e.offsets) {
            a = e.offsets[i];
            len = e.offsets[i + 1] - a;
            a -= e.off_base;
        } else {
            a = i * e.stride;
            len = e.stride;
        }
        return murmur_bytes(e.bytes + a, len);
    }
}

struct HllSeg {
    uint8_t *regs;      // 16384 u8 registers
    uint64_t begin;     // element range [begin, end)
    uint64_t end;
    uint32_t seg;       // command index (for the changed flag)
    uint32_t pad;
};
void launch_hll_pfadd(const KeysDev &elems, int elen_fast, const HllSeg *d_tiles, uint32_t ntiles,
                      uint32_t *d_changed, hipStream_t st);
// Per-HLL histogram + Redis estimator; out[i] = count, or ~0 when the hllTau branch
// (a register == 51) must be evaluated on the host with glibc pow.  histo: n*64 ints.
void launch_hll_count(uint8_t *const *d_regs, uint32_t n, int *d_histo, unsigned long long *d_out,
                      hipStream_t st);
// dst = max(dst, src_0..src_{n-1}) over 16384 registers
void launch_hll_merge(uint8_t *dst, uint8_t *const *d_srcs, uint32_t nsrc, hipStream_t st);
// raw registers -> scratch union: out = max over a set of HLLs (multi-key PFCOUNT)
void launch_hll_union(uint8_t *const *d_srcs, uint32_t nsrc, uint8_t *out, hipStream_t st);
// Redis sparse HLL strings kept as redis-server builds them ([redis-7.2] hyperloglog.c
// hllSparseSet, replayed in command order): one u16 per opcode -- ZERO and VAL opcodes are their
// byte, XZERO is (byte0 << 8 | byte1) -- so ZERO < 0x40 <= VAL < 0x100 <= XZERO.
struct HllReplay {
    uint16_t *ops;        // the HLL's opcode list (capacity >= max(its bytes, 3000): opcodes <= bytes)
    uint32_t *state;      // [0] promoted (sticky: the list is stale once set), [1] opcodes (0 = the
                          // createHLLObject string, one XZERO), [2] opcode bytes (after the header)
    const uint8_t *regs;  // merge mode (PFMERGE write-back): the max registers, ascending; else null
    uint64_t begin, end;  // PFADD mode: the command's elements, in order
    const uint8_t *final_regs;  // the registers after the update (PFADD: the key's, merged already)
    // PFADD mode, second form (the HLL stream: one key's elements across many commands): non-null = the
    // elements are list_base + list[begin .. end), in that order; null = the elements [begin, end) themselves
    const uint32_t *list;
    uint64_t list_base;
};
// one block per item; items whose HLL is already promoted return at once
void launch_hll_sparse_replay(const KeysDev &elems, int elen_fast, const HllReplay *items, uint32_t n,
                              uint64_t max_bytes, hipStream_t st);
// zero n pool slots: 16384 register bytes and 4 state words each (kHllStateWords)
void launch_hll_zero(uint8_t *const *d_regs, uint32_t *const *d_state, uint32_t n, hipStream_t st);
// buf[i*16384..] = regs[i] (pack) or regs[i] = max(regs[i], buf[i*16384..]) (unpack_max)
void launch_hll_pack(uint8_t *const *d_regs, uint32_t n, uint8_t *buf, bool unpack_max, hipStream_t st);

// ---- hllstream_kernels.hip
// The grouped add run of the ordered PFADD / PFCOUNT stream over many HLLs (rbx_hll_stream).
// One HLL of the call as the kernels see it, one record per entry of `names`.
struct alignas(16) HllKey {
    uint8_t *regs;   // 16384 u8 registers (null: the key holds another type)
    uint32_t flags;  // kHllKeyWrong | kHllKeyFailed
    uint32_t canon;  // the first entry of `names` with this entry's bytes (its own index if none is earlier)
};
static_assert(sizeof(HllKey) == 16, "four to a line");
constexpr uint32_t kHllKeyWrong = 1;   // the key holds another type
constexpr uint32_t kHllKeyFailed = 2;  // its commands fail alone: their elements touch nothing
constexpr int kHsRegShift = 6, kHsKeyShift = 20;  // cell = canon << 20 | register << 6 | count
// One chunk of an add run: the commands [cmd0, cmd0 + ncmds) of the call, whose elements are the m <= 2^30
// elements from elem0 on in the call's numbering (d_cmd_elem's) and from `first` on in `elems`.  d_cmd_elem
// and d_cmd_key are the call's arrays (a PFCOUNT or an empty PFADD of the range owns no element); d_changed
// has one word per command of the call and gets a 1 for each command that raises a register.  key_bits: the
// significant bits of nkeys - 1; has_failed: some key of the table has kHllKeyFailed.  The sort looks at the
// (key, register) bits only, so the scratch is cell_sort_scratch_bytes<unsigned long long>(m, kHsRegShift,
// hllstream_end_bit(key_bits, has_failed)).  Returns 0 or a hipError_t.
constexpr int hllstream_end_bit(int key_bits, bool has_failed) { return kHsKeyShift + key_bits + (has_failed ? 1 : 0); }
int launch_hllstream_grouped(const KeysDev &elems, int elen_fast, uint64_t first, uint64_t elem0, uint32_t m,
                             const HllKey *d_tab, const uint64_t *d_cmd_elem, const uint32_t *d_cmd_key, uint64_t cmd0,
                             uint32_t ncmds, uint32_t *d_changed, int key_bits, bool has_failed, void *d_scratch,
                             size_t scratch_bytes, hipStream_t st);
// d_out[i] = d_states[i][0], the sticky promotion word (HllReplay::state) of each sparse HLL of a run
void launch_hllstream_promoted(uint32_t *const *d_states, uint32_t n, uint32_t *d_out, hipStream_t st);

// ---- hllgroups_kernels.hip
// Many PFCOUNT unions / PFMERGEs in one launch (rbx_hll_count_groups, rbx_hll_merge_groups).  Group g
// is the register blocks d_members[d_off[g] .. d_off[g + 1]) (16384 bytes each; a group may be empty); `split` = the
// workgroups a group's registers are spread over, a power of two in 1 .. kHllGroupsMaxSplit, ngroups * split < 2^31.
constexpr int kHllGroupsMaxSplit = 16;
// d_out[g] = the cardinality of group g's union, or ~0 when it holds a register of 51 (launch_hll_count's rule);
// d_histo: ngroups * 64 ints, the unions' histograms.  Returns 0 or a hipError_t.
int launch_hllgroups_union_count(const uint8_t *const *d_members, const uint32_t *d_off, uint32_t ngroups, int split,
                                 int *d_histo, unsigned long long *d_out, hipStream_t st);
// d_dst[g] = max(d_dst[g], group g's members).  No d_dst[g] may be a member of another group or another group's
// destination; it may be a member of its own group.
void launch_hllgroups_merge(uint8_t *const *d_dst, const uint8_t *const *d_members, const uint32_t *d_off,
                            uint32_t ngroups, int split, hipStream_t st);

// ---- bitgroups_kernels.hip
// Many BITOPs / BITCOUNTs of a combination in one launch (rbx_bitset_op_groups).  One record per group;
// its sources are the nsrc entries of the launch's BitopSrc table from src_off on.
struct BitGroup {
    uint8_t *dst;                 // the destination's bytes, or null: the combination is stored nowhere
    unsigned long long *dst_len;  // its length word (null with dst), which takes out_len
    unsigned long long *count;    // takes the result's one bits, added onto a zeroed word; null: not counted
    uint64_t out_len;             // the result's length: the longest source's, > 0
    uint64_t span;                // the bytes swept: a multiple of 16 within dst's allocation covering out_len and
                                  // dst's previous length; without dst, out_len rounded up to 16
    uint64_t full;                // a multiple of 16 that every source's length reaches (0 when one is missing)
    uint32_t op;                  // RBX_BITOP_*
    uint32_t nsrc;                // >= 1; exactly 1 under RBX_BITOP_NOT
    uint32_t src_off;
    uint32_t pad;
};
constexpr uint32_t kBitGroupsMinTile = 4096, kBitGroupsMaxTile = 1u << 20;
// d_out[i] = *d_ptrs[i] for n length words
void launch_bitgroups_lens(const unsigned long long *const *d_ptrs, uint32_t n, unsigned long long *d_out, hipStream_t st);
// The groups' spans cut into tiles of tile_bytes (a power of two in kBitGroupsMinTile .. kBitGroupsMaxTile): group g
// owns the tiles d_first[g] .. d_first[g + 1), d_first[0] = 0, d_first[ngroups] = tiles, every group at least one.  No
// dst may be a source or the dst of another group; it may be a source of its own.
void launch_bitgroups_sweep(const BitGroup *d_groups, const uint64_t *d_first, uint32_t ngroups, uint64_t tiles,
                            const BitopSrc *d_srcs, uint32_t tile_bytes, hipStream_t st);

}  // namespace rbx
