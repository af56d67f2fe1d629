// tunables.h -- every host-side knob of rbx_tune (include/rbx_bench.h documents the keys); the kernels' own
// are behind the set_* functions of rbx_kernels.h.  One instance, g_tune, defined in rbx_api.cpp beside
// rbx_tune's table.  rbx_tune may run on another thread: a call that uses a knob twice reads it ONCE.
#pragma once
#include <atomic>
#include <cstdint>

namespace rbx {

struct Tunables {
    // ---- single-filter add (api_bloom.cpp) ----
    // "add_partition": the partitioned add for one large filter, 0 never, 1 whenever k <= 16, 2 (default)
    // by bitmap and batch size (use_add_partitioned has the thresholds and the measured crossovers)
    std::atomic<int> add_partition_mode{2};
    // "add_partition_diag" (profiling build only): 4 = the region kernel emits no records, 8 = it loads only
    // its first two regions' pairs, 16 = it only loads, 64 = phase stamps (rbx_bench_add_stamps)
    std::atomic<int> add_partition_diag{0};
    // "add_records": how the add's region kernel reports which keys are new (add_partitioned.hip k_ba_mode): 0
    // owner bits, 1 non-owner counters, 3 owner records, 2 (default) chosen from the sampled fill.  All exact.
    std::atomic<int> add_record_policy{2};
    // "add_single_seg_keys": adds of <= this many keys (k <= 16) run the per-segment kernel (run_add); 0 = off
    std::atomic<uint64_t> seg_single_keys{256};
    // "add_one_key": 1 = a 1-key add takes k_bloom_add_one
    std::atomic<int> add_one{1};

    // ---- single-filter contains (api_bloom.cpp) ----
    // "contains_partition": the partitioned contains for one large filter, 0 never, 1 whenever k in
    // [2, 16], 2 (default) when the bitmap is >= 256 MiB and the batch >= 4M keys (use_partitioned)
    std::atomic<int> partition_mode{2};
    // "contains_partition_flags" (profiling build only): 4 = stage 1 emits no pairs, 8 = the probe records
    // no misses, 16 = one atomicOr per clear bit, 32 = no bit-0 gather, 64 = phase stamps
    std::atomic<int> partition_flags{0};
    // "contains_stage1_grid": caps the partitioned contains' stage-1 grid (default 256, one block per CU).  A chunk
    // holds at most grid * 2^19 keys (bk_entry.h), so tests reach a block's 512th tile on a small batch
    std::atomic<uint32_t> stage1_grid{256};

    // "wide_subchunk": bloom_wide_op's keys per sub-chunk cap (0 = default 2^29 / k; tests split small batches)
    std::atomic<uint64_t> wide_subchunk{0};

    // ---- host staging tiers (api_staging.cpp) ----
    // "host_small_batches": 0 = every host batch on the pipelined path
    std::atomic<int> small_host{1};
    // "host_small_bytes": the small tier's byte limit (keys <= limit / 4)
    std::atomic<uint64_t> small_bytes{4 << 20};
    // "host_tiny_keys": the tiny tier's key limit; 0 = off
    std::atomic<uint64_t> tiny_keys{16384};
    // "host_tiny_spin": 1 (default) = a tiny call spins on its completion word (tiny_wait), 0 = stream sync
    std::atomic<int> tiny_spin{1};

    // ---- multi-tenant and stream (api_bloom_multi.cpp) ----
    // "contains_multi_slots": the per-lane slot kernel 0 never, 1 always, 2 (default) past kSlotsMinBytes
    std::atomic<int> multi_slots{2};
    // "stream_chunk": caps a chunk of the ordered stream and of the 8-byte multi-tenant add at n commands
    // (tests: many chunks on small batches); 0 = no cap
    std::atomic<uint64_t> stream_chunk{0};
    // "add_multi_table8": multi-tenant adds whenever (filter id, bit) fits 41 bits and k <= 32:
    // 2 (default) optimistic SETBITs with conflict repair (k_maddx_*, r05), 0 the r03 16-byte table path
    // (the fallback past 41 bits or k > 32; tests).  (1, the 8-byte first-setter table with the walk
    // commit, measured 74.5 vs 53.3 ms at C3 and was removed in r06.)
    std::atomic<int> add_multi_t8{2};
    // "add_multi_conflict_log2": entries of the conflict table C, log2 (default 17: 1 MiB, L2-
    // resident; tests use small ones to run the overflow path)
    std::atomic<uint32_t> maddx_lgc{17};
    // "add_multi_segment": 1 (default) a batch whose filters are all distinct runs its segments of
    // <= add_multi_segmax keys one workgroup each (k_madd_seg: LDS first setters, plain word stores, no
    // memory-side atomics), longer segments on the chunked path; 0 everything on the chunked path
    std::atomic<int> madd_seg{1};
    std::atomic<uint64_t> madd_segmax{16384};  // "add_multi_segmax"
    // "add_multi_seg_grid": the per-segment kernel's workgroups, grid-stride over the segments
    // (8192: C3 add 28.5 ms; 4096 28.9, 2048 29.9, 1024 31.1, 512 32.7; profiles/r06/r06d_*)
    std::atomic<uint32_t> madd_seg_grid{8192};
    // "stream_table8": 1 (default) the 8-byte first-setter table + walk commit (r04) when (fid, bit) fits
    // 41 bits, 0 the r03 16-byte epoch-tagged table (the fallback past 41 bits; tests)
    std::atomic<int> stream_table8{1};

    // ---- ranged BITCOUNT / BITPOS (api_bitset.cpp) ----
    // "bitrange_pos_chunk": bytes of a chunk of the single search (k_bits_pos), a power of two in 4 KiB..1 MiB
    std::atomic<uint32_t> bitrange_pos_chunk{256 << 10};
    // "bitrange_chain_max": a batch whose longest interval exceeds this many bytes takes the block directory
    // (the longest walk one wave makes alone on the direct path)
    std::atomic<uint64_t> bitrange_chain_max{128 << 10};
    // "bitrange_dir": batches of >= 2 queries through the block directory 0 never, 1 always, 2 (default) by
    // the read-bytes and chain-length rules (ranges_run)
    std::atomic<int> bitrange_dir{2};

    // ---- BITFIELD overflow modes (api_bitset.cpp) ----
    // "bitfield_sat_atomic": 1 (default) = an aligned SAT INCRBY without replies whose size divides 64 and whose
    // increments have one sign takes k_fields_incr_sat, 0 = the grouped path (tests run both on one input)
    std::atomic<int> bitfield_sat_atomic{1};

    // ---- the ordered GETBIT / SETBIT stream (api_bitset_multi.cpp) ----
    // "bitstream_path": 0 (default) = gather for a batch of GETBITs, scatter for SETBITs of one value without
    // replies, else serial up to bitstream_serial_max commands and grouped past it; 1 = always serial, 2 = always
    // grouped.  All exact.
    std::atomic<int> bitstream_path{0};
    // "bitstream_serial_max": the auto rule's largest batch for the one-lane walk
    std::atomic<uint64_t> bitstream_serial_max{64};
    // "bitstream_chunk": commands per chunk of the grouped path (36 bytes of sort scratch per command: 2^25
    // commands are 1.125 GiB)
    std::atomic<uint64_t> bitstream_chunk{1 << 25};

    // ---- the ordered BITFIELD stream (api_bitset_multi.cpp) ----
    // "fieldstream_path": 0 (default) = gather for a batch without SET / INCRBY, one compare-and-swap loop per
    // command for WRAP INCRBYs of one size dividing 64 at multiples of it without replies, else serial up to
    // fieldstream_serial_max commands, past it grouped by word when every command lies inside one aligned
    // 64-bit word and by key otherwise; 1 = always serial, 2 = always grouped by word (by key when a field
    // straddles words), 3 = always grouped by key.  All exact.
    std::atomic<int> fieldstream_path{0};
    // "fieldstream_serial_max": the auto rule's largest batch for the one-lane walk.  bitstream_serial_max's
    // value, taken over from DESIGN 11.5: the crossover is NOT measured for fields.
    std::atomic<uint64_t> fieldstream_serial_max{64};
    // "fieldstream_chunk": commands per chunk of the grouped paths (24 bytes of sort scratch per command plus
    // rocPRIM's own; positions inside a chunk are 32-bit)
    std::atomic<uint64_t> fieldstream_chunk{1 << 25};

    // ---- the ordered PFADD / PFCOUNT stream (api_hll.cpp) ----
    // "hllstream_path": how an add run (the PFADDs of one phase) reaches the registers: 0 (default) = by rounds
    // (pfadd_run: one k_hll_pfadd launch per maximal run of commands on distinct keys) when the run has few
    // rounds for its elements, else grouped (one sort by (key, register) per chunk, hllstream_kernels.hip);
    // 1 = always rounds, 2 = always grouped.  All exact.
    std::atomic<int> hllstream_path{0};
    // "hllstream_chunk": elements per chunk of the grouped path (36.125 bytes of sort scratch per element, what
    // cell_sort_scratch_bytes returns at 2^25: 24 of cells and positions, the rest rocPRIM's temporary
    // storage; 2^25 elements are 1.129 GiB); a command with more elements than this runs by rounds, alone
    std::atomic<uint64_t> hllstream_chunk{1 << 25};
    // "hllstream_elems_per_round": the auto rule takes the grouped path iff the run's rounds R exceed
    // max(1, elements / this): what one round costs, in elements of the grouped path.  Measured on 2^20
    // one-element PFADDs over 4,096 keys (DESIGN 11.7 row d): 10.2 us per round by rounds against 8.97 ns per
    // element grouped, call times with the host's share in both: 1137 elements per round.
    std::atomic<uint64_t> hllstream_elems_per_round{1137};

    // ---- grouped PFCOUNT unions and PFMERGEs (api_hll.cpp) ----
    // "hllgroups_split": the workgroups P one group's 16,384 registers are spread over: 0 (default) = auto, else
    // P, a power of two up to 16.  All exact.  Auto (hllgroups_auto_split) takes the smallest P with groups * P >=
    // kHllGroupsFillBlocks, capped at 16: a handful of groups still fills the device, and from kHllGroupsFillBlocks
    // groups on each runs in one workgroup, which finishes with the estimator in place (P > 1 costs a fill of the
    // histograms and the finish launch).  kHllGroupsFillBlocks is 256, one workgroup per CU.  Measured on unions of
    // 24 members (DESIGN 11.8 row c): at 1 and 16 groups P = 16 is fastest (0.043 / 0.044 ms against 0.051 / 0.054 ms
    // at P = 1); at 256, 4,096 and 10,000 groups all six settings lie within 4 % (0.088 - 0.092, 0.754 - 0.757 and
    // 1.777 - 1.795 ms), so from 256 on P = 1 is taken.
    std::atomic<int> hllgroups_split{0};

    // ---- grouped BITOPs and BITCOUNTs (api_bitset_multi.cpp) ----
    // "bitgroups_tile": the bytes T of a tile of the segmented sweep: 0 (default) = auto, else a power of two in
    // 4 KiB .. 1 MiB.  All exact.  Auto: bitgroups_auto_tile below.
    std::atomic<uint32_t> bitgroups_tile{0};

    // ---- the read queries over many keys (api_bitset_multi.cpp) ----
    // "rangestream_lanes": the lanes G of the group that answers one command, 4, 8, 16, 32 or 64.  All exact.
    // Measured (DESIGN 11.10 row d): on 20,000 strings of 46 bytes and of 1 KiB the five settings lie within 1 % (the
    // call is host-bound there); 16 is kept.
    std::atomic<int> rangestream_lanes{16};
    // "rangestream_short_max": the bytes of the longest interval a lane group walks alone, a power of two in
    // 64 .. 1 MiB; a longer one is cut into tiles for the whole device.  4096 is a guess: no measurement decides it (DESIGN 11.10
    // row e's strings lie on one side of every setting).
    std::atomic<uint32_t> rangestream_short_max{4096};
    // "rangestream_tile": the bytes of a tile of a long interval, a power of two in 4 KiB .. 1 MiB.  65536 is the
    // large-work optimum of bitgroups_auto_tile's table below, and measured here (DESIGN 11.10 row e): 4 KiB tiles cost
    // 17 %, 16 KiB 2 %, and 64 KiB .. 1 MiB lie within 0.3 %.
    std::atomic<uint32_t> rangestream_tile{65536};
    // "rangestream_chunk": commands per chunk, 1 .. 2^30 (8 bytes of long list per command of a chunk; each chunk
    // has its own summary and wait)
    std::atomic<uint64_t> rangestream_chunk{1 << 25};

    // ---- set-bit enumeration over many keys (api_bitset_multi.cpp) ----
    // The four knobs of rbx_bitset_members_stream mirror the range stream's.  All exact.
    // "members_lanes": the lanes G of the group that counts and expands one short command, 4, 8, 16, 32 or 64.
    // Measured (DESIGN 11.11 row f): on 20,000 strings of 46 bytes the five settings lie within 0.5 % (the call is
    // host-bound there); 16 is kept.
    std::atomic<int> members_lanes{16};
    // "members_short_max": the bytes of the longest interval a lane group walks alone, a power of two in 64 .. 1 MiB;
    // a longer one is cut into tiles for the whole device.  4096 is a guess: no measurement decides it (DESIGN 11.11
    // row f's strings lie on one side of every setting).
    std::atomic<uint32_t> members_short_max{4096};
    // "members_tile": the bytes of a tile of a long interval, a power of two in 4 KiB .. 1 MiB.  Measured (DESIGN 11.11
    // row f): 4 KiB tiles cost 29 %, 1 MiB tiles 10 % against 64 KiB.
    std::atomic<uint32_t> members_tile{65536};
    // "members_chunk": commands per chunk, 1 .. 2^30 (8 bytes of long list per command of a chunk; each chunk has its
    // own summary and wait, and the offsets carry across chunks on the device).  2^25 is the range stream's: not measured.
    std::atomic<uint64_t> members_chunk{1 << 25};

    // ---- GETRANGE / SETRANGE / APPEND / GET over many keys (api_bitset_multi.cpp) ----
    // The five knobs of rbx_string_stream.  All exact.  Every default is the range stream's (the serial one the bit
    // stream's), taken over.  Measured (DESIGN 11.12 row d): on 100,000 keys of 46 bytes the five lane widths
    // lie within 2 % (the call is host-bound there), so 16 is kept; the other four are NOT measured.
    // "bytestream_lanes": the lanes G of the group that executes one key's commands, 4, 8, 16, 32 or 64
    std::atomic<int> bytestream_lanes{16};
    // "bytestream_short_max": the bytes of the longest command a lane group moves alone, a power of two in 64 .. 1 MiB;
    // a longer one is cut into tiles for the whole device
    std::atomic<uint32_t> bytestream_short_max{4096};
    // "bytestream_tile": the bytes of a tile of a long command (and of a single call), a power of two in 4 KiB .. 1 MiB
    std::atomic<uint32_t> bytestream_tile{65536};
    // "bytestream_chunk": commands per chunk, 1 .. 2^30 (12 bytes of sort scratch plus 16 of cursor, run list and long
    // list per command of a chunk; each chunk has its own summary and wait)
    std::atomic<uint64_t> bytestream_chunk{1 << 25};
    // "bytestream_serial_max": the largest call that one lane group runs in array order without the sort (when none
    // of its commands is long)
    std::atomic<uint64_t> bytestream_serial_max{64};
};

constexpr uint32_t kHllGroupsFillBlocks = 256;
inline int hllgroups_auto_split(uint64_t groups) {
    int p = 1;
    while (p < 16 && groups * (uint64_t)p < kHllGroupsFillBlocks) p <<= 1;
    return p;
}

// The auto tile of a launch that sweeps `bytes` bytes in all: the largest power of two T in 4 KiB .. kBitGroupsAutoMaxTile
// with bytes / T >= kBitGroupsFillTiles, so that a launch of little work still spreads over the device (one 1 MiB group
// is 256 tiles of 4 KiB) and a launch of much work makes tiles of kBitGroupsAutoMaxTile.  Measured call times (DESIGN
// 11.9 row f; T = 4 / 16 / 64 / 256 KiB / 1 MiB): 1 AND of 2 x 1 MiB 0.051 / 0.053 / 0.063 / 0.114 / 0.253 ms and 16 of
// them 0.069 / 0.070 / 0.089 / 0.171 / 0.502 ms -- little work wants small tiles; 256 of them 0.417 / 0.298 / 0.264 /
// 0.298 / 0.631 ms and 10,000 counted ANDs of 2 x 128 KiB 1.944 / 1.144 / 0.856 / 0.838 / 0.876 ms -- much work wants
// 64 - 256 KiB, which lie within 13 % of each other either way, and 1 MiB is slowest wherever a group is about one
// tile.  One AND of 2 x 512 MiB runs 0.335 / 0.388 / 0.406 / 0.419 / 0.628 ms: a single huge group would rather have
// 4 KiB (a workgroup keeps its group across tiles, and neighbouring workgroups then read neighbouring bytes), which
// this rule, looking at the launch's bytes only, does not give it.
constexpr uint32_t kBitGroupsFillTiles = 2048;  // kMaxGrid: eight workgroups per CU
constexpr uint32_t kBitGroupsAutoMaxTile = 64 << 10;
inline uint32_t bitgroups_auto_tile(uint64_t bytes) {
    uint32_t t = 4096;
    while (t < kBitGroupsAutoMaxTile && bytes / (2 * (uint64_t)t) >= kBitGroupsFillTiles) t <<= 1;
    return t;
}

extern Tunables g_tune;

}  // namespace rbx
