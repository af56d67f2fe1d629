// rbx_ctx.h -- private to csrc/ (never included from include/), shared by the host translation units of
// librbx.so (rbx_api.cpp and the api_*.cpp files): the owning buffer types (DevBuf, PinBuf, CachedTable), the
// objects the keyspace holds, the context with its device state grouped by subsystem, and the call scope.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rbx.h"
#include "host_exec.h"
#include "keyspace.h"
#include "rbx_kernels.h"

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return rbx::fail(e_ == hipErrorOutOfMemory ? RBX_E_OOM : RBX_E_DEVICE,             \
                             std::string(#expr ": ") + hipGetErrorString(e_));                 \
    } while (0)

#define RBX_TRY(expr)             \
    do {                          \
        int r_ = (expr);          \
        if (r_ != RBX_OK) return r_; \
    } while (0)

// ---- buffers that own their allocation ----------------------------------------------------------------
// Neither copies nor moves: a buffer is freed once, by the destructor of the group it is a member of.
inline std::atomic<int64_t> g_live_buffers{0};  // allocations DevBuf / PinBuf hold now (rbx_selftest_live_buffers)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    size_t filled = 0;  // bytes from p that hold reserve_filled's byte: 0 until the fill has been queued
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && hipFree(p) == hipSuccess) --g_live_buffers;
        p = nullptr;
        cap = filled = 0;
    }
    int reserve(size_t n) {
        if (n <= cap) return RBX_OK;
        release();
        size_t want = std::max<size_t>(n, 4096);
        HIP_TRY(hipMalloc(&p, want));
        ++g_live_buffers;
        cap = want;
        return RBX_OK;
    }
    // reserve(n) for a buffer whose users rely on a fill they restore themselves (an EMPTY table, zeroed
    // counters): `byte` is queued on `st` only when the buffer grows or an earlier fill did not get queued,
    // over the whole capacity or (whole = false) over the n bytes asked for
    int reserve_filled(size_t n, int byte, hipStream_t st, bool whole = true) {
        if (n <= filled) return RBX_OK;
        filled = 0;
        RBX_TRY(reserve(n));
        const size_t m = whole ? cap : n;
        HIP_TRY(hipMemsetAsync(p, byte, m, st));
        filled = m;
        return RBX_OK;
    }
    void invalidate() { filled = 0; }  // a user left the content in an unknown state: the next call fills again
    template <class T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && !std::is_move_constructible_v<DevBuf>, "DevBuf owns");

struct PinBuf {  // pinned host memory (hipHostMalloc with the caller's flags)
    void *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    void release() {
        if (p && hipHostFree(p) == hipSuccess) --g_live_buffers;
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(size_t n, unsigned flags) {  // replaces the block
        release();
        const hipError_t e = hipHostMalloc(&p, n, flags);
        if (e != hipSuccess) p = nullptr;
        else ++g_live_buffers, cap = n;
        return e;
    }
    template <class T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible_v<PinBuf>, "PinBuf owns");

// A device table uploaded only when its content changes: the buffer and the host copy of what it holds.
template <class T> struct CachedTable {
    DevBuf buf;
    std::vector<T> host;    // content of buf while `valid`
    bool valid = false;
    bool uploaded = false;  // the last sync copied (its caller refreshes what it derives from the table)
    int err = RBX_OK;       // why the last sync returned null
    void invalidate() { valid = false; }
    // the device table holding `items`; not cacheable: uploaded now and not compared against next time
    const T *sync(const std::vector<T> &items, hipStream_t st, bool cacheable = true) {
        const size_t bytes = items.size() * sizeof(T);
        uploaded = !(cacheable && valid && host.size() == items.size() && memcmp(host.data(), items.data(), bytes) == 0);
        if (!uploaded) return buf.as<T>();
        valid = false;
        // pageable source: the runtime has staged it when the copy call returns; stream order keeps the
        // table's previous reader ahead of this overwrite
        if ((err = upload(items.data(), bytes, st)) != RBX_OK) return nullptr;
        if (cacheable) host = items;
        valid = cacheable;
        return buf.as<T>();
    }
    int upload(const T *src, size_t bytes, hipStream_t st) {
        RBX_TRY(buf.reserve(bytes));
        HIP_TRY(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
        return RBX_OK;
    }
};

// ---- device objects held by the keyspace (keyspace.h declares them opaque) -------------------------
// Small bitmaps (<= 64 MiB) come from 1 GiB slabs, exact-size free lists, so that
// 100k tenant filters do not cost 100k hipMalloc calls; large ones get their own buffer.
// Memory returned to a free list is reused only through new_bitmap / hll_alloc, whose zero
// fill runs on the calling stream after it waited for every earlier call of the context
// (CallScope): so a freed bitmap or HLL still read by an in-flight *_dev call on another
// stream is never overwritten early.
struct SlabPool {
    std::mutex mu;
    std::vector<void *> slabs;
    std::map<uint64_t, std::vector<void *>> free_by_size;
    uint8_t *cur = nullptr;
    uint64_t left = 0;
    static constexpr uint64_t kSlab = 1ull << 30, kMaxSmall = 64ull << 20;
    void *get(uint64_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        auto &fl = free_by_size[bytes];
        if (!fl.empty()) {
            void *p = fl.back();
            fl.pop_back();
            return p;
        }
        if (left < bytes) {
            void *s = nullptr;
            if (hipMalloc(&s, kSlab) != hipSuccess) return nullptr;
            slabs.push_back(s);
            cur = (uint8_t *)s;
            left = kSlab;
        }
        void *p = cur;
        cur += bytes;
        left -= bytes;
        return p;
    }
    void put(void *p, uint64_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        free_by_size[bytes].push_back(p);
    }
    ~SlabPool() {
        for (void *s : slabs) (void)hipFree(s);
    }
};

namespace rbx {
struct Bitmap {  // a Redis string used with SETBIT/GETBIT
    int device = 0;
    uint32_t *d_words = nullptr;
    uint64_t cap_bytes = 0;                 // allocated bytes (multiple of 256)
    unsigned long long *d_len = nullptr;    // device word: Redis string length (in the slab too)
    std::shared_ptr<SlabPool> pool;         // set when d_words/d_len came from the pool
    ~Bitmap() {
        if (pool) {
            pool->put(d_words, cap_bytes + 256);
            return;
        }
        if (d_words) (void)hipFree(d_words);
        if (d_len) (void)hipFree(d_len);
    }
};

struct HllState {  // a Redis HLL string, registers unpacked (1 byte each) on the device
    uint8_t *d_regs = nullptr;  // 16384 bytes inside a pool chunk
    // device state words (HllReplay::state): [0] promoted -- a PFADD / PFMERGE promoted the sparse
    // string to dense --, [1] opcodes in d_sp_ops (0 = the createHLLObject string), [2] its bytes
    uint32_t *d_promoted = nullptr;
    uint16_t *d_sp_ops = nullptr;  // the sparse string as Redis built it, one u16 per opcode
    uint16_t *d_slot_ops = nullptr;  // the pool slot's opcode list (kHllSlotOps entries)
    uint16_t *d_big_ops = nullptr;   // own allocation (16384 entries) for a SET string past the slot
    uint64_t card = 0;          // the header's 8 cached-cardinality bytes (LE); bit 63 = invalid
    bool dense = false;         // Redis encoding: created sparse, promoted to dense once (never back)
    struct ::rbx_ctx *owner = nullptr;
    ~HllState();
};
}  // namespace rbx

// Handles are bound to a NAME, like a Redisson object: a call re-resolves the keys whenever the
// keyspace changed since the handle's last call (gen), so delete / rename / expire / re-import
// behave as they do through the name-based entry points.  A handle holds a reference on its
// context, so closing it after rbx_shutdown is safe (every other call on it then fails).
struct rbx_bloom {
    rbx_ctx *ctx;
    std::string name;
    int64_t size;  // the config's size (Java long)
    uint32_t k;
    std::shared_ptr<rbx::Bitmap> bm;
    uint64_t gen = 0;
    uint64_t serial = 0;  // unique per handle (a freed handle's address can be reused)
};

struct rbx_hll {
    rbx_ctx *ctx;
    std::string name;
    std::shared_ptr<rbx::HllState> st;
    uint64_t gen = 0;
};

// ---- the context's device state, grouped by the subsystem that owns it ----------------------------------
// Each group holds its buffers and the host fields that say what they contain.  rbx_ctx keeps them in one
// DeviceState, which rbx_shutdown destroys as a whole: a buffer added to a group needs no other mention.

// First-setter table of add() (16-byte HTEntry, cleared once per 254 epochs) and of its narrow 8-byte layout.
struct FirstSetterTable {
    DevBuf table;
    uint32_t log2cap = 0;
    uint32_t epoch = 255;  // 255 = table needs (re)initialisation
    // capacity >= 2 * pairs per chunk, between 2^16 and 2^27 entries (2 GiB), and the chunk's epoch
    int ensure(uint64_t want_pairs, hipStream_t st) {
        uint32_t lg = 16;
        while (lg < 27 && (1ULL << lg) < 2 * want_pairs) ++lg;
        if (lg > log2cap) {
            RBX_TRY(table.reserve(sizeof(rbx::HTEntry) << lg));
            log2cap = lg;
            epoch = 255;
        }
        if (epoch >= 254) {
            HIP_TRY(hipMemsetAsync(table.p, 0xff, sizeof(rbx::HTEntry) << log2cap, st));
            epoch = 0;
        } else {
            epoch++;
        }
        return RBX_OK;
    }
    // 2^lg EMPTY 8-byte entries for one chunk; the wide layout must be re-initialised before reuse
    int use_narrow(uint32_t lg, hipStream_t st) {
        RBX_TRY(table.reserve(8ull << lg));
        HIP_TRY(hipMemsetAsync(table.p, 0xff, 8ull << lg, st));
        epoch = 255;
        return RBX_OK;
    }
};

// 8-byte first-setter table shared by the ordered stream and the multi-tenant add: every chunk's walk
// restores EMPTY, so it is filled only when it grows (or after a user failed midway: buf.invalidate()).
struct T8Table {
    DevBuf buf;
    int ensure(uint64_t entries, hipStream_t st) { return buf.reserve_filled(entries * 8, 0xff, st, false); }
};

// what upload_filters hands its callers: the device tables of a multi-tenant call and their extent
struct FilterView {
    const rbx::FilterDesc *filt = nullptr;  // per segment
    const rbx::ProbeDesc *probes = nullptr;  // per segment
    uint32_t *const *fid_bm = nullptr;      // bitmap words per table id (fid)
    uint32_t kmax = 1;
    uint64_t bytes = 0;    // of the distinct bitmaps
    uint32_t nfids = 0;    // distinct table ids
    uint64_t maxbits = 0;  // the largest of their bitmaps, in bits
};

// Per-segment descriptor tables of the multi-tenant calls (upload_filters), cached by content and by handle list.
struct FilterTable {
    CachedTable<rbx::FilterDesc> table;
    uint64_t generation = 0;  // ks.generation `table` was built under (a bitmap may have moved since)
    DevBuf probes, fids;      // ProbeDesc per entry of table; bitmap words per fid
    // all-zero words standing in for a missing bitmap in multi-tenant contains (GETBIT on a
    // missing key reads 0; the key is not created), grown on demand, never written by a kernel
    DevBuf zero_bm;
    // the handle list the tables were built from (fast path for repeated multi-tenant calls)
    std::vector<std::pair<const rbx_bloom *, uint64_t>> keys;
    uint64_t key_generation = ~0ULL;
    bool create = false;
    bool had_absent = false;  // an entry stands on zero_bm: never reused by a call that may write
    FilterView view;  // of the tables as they are
};

struct StreamScratch {  // ordered stream and chunked multi-tenant add
    DevBuf adds, nadds;  // add list, one add counter per chunk
    DevBuf fslot;        // per add, the slot of its first zero bit's claim
    DevBuf madd_c;       // multi-tenant add: conflict table C + its MaddxState (+ the `big` flag)
    uint64_t geom[4] = {0, 0, 0, 0};  // last stream call: bb, fbits, pb, chunk
};

struct PartitionedContainsScratch {
    DevBuf bits, cnt, pairs, mrec;
};

struct PartitionedAddScratch {
    DevBuf p1, p2, cnt, bits, recs;
    DevBuf ctr;     // per-key non-owner counters: k_ba_final zeroes what it read
    DevBuf stamps;  // diagnostics: region-pass phase times (rbx_bench_add_stamps), also the partitioned contains'
};

// Host-buffer calls: plain uploads, the copy-stream double buffer, the small and tiny tiers' pinned blocks.
struct Staging {
    DevBuf keys_bytes, keys_offs, out_bytes, seg_offs;
    // pipeline: uploads on copy_stream into two device slots while the previous slot's kernels run
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    DevBuf slot_bytes[2], slot_offs[2];
    uint64_t staging_bytes = 64ull << 20;
    // small host batches (bloom_host_small): a pinned copy of the keys, uploaded on the context stream with
    // the zeroed count word in one transfer; the count and flags come back into it
    PinBuf pin_small;
    uint64_t pin_small_limit = 0;  // the host_small_bytes the block was laid out for (its tail offset)
    PinBuf pin_word;  // pinned readback words (counts, the partitioned add's overflow flag)
    // tiny host batches (bloom_host_tiny): coherent pinned memory the kernel reads the keys from and
    // writes the flags into, no transfer on either side
    PinBuf pin_tiny;
    uint8_t *pin_tiny_dev = nullptr;  // its device address
    uint32_t tiny_seq = 0;            // the last completion word a one-key kernel stored into the block
    unsigned long long *words() const { return pin_word.as<unsigned long long>(); }
    uint8_t *tiny() const { return pin_tiny.as<uint8_t>(); }
    ~Staging() {
        for (hipEvent_t e : {ev_copied[0], ev_copied[1], ev_done[0], ev_done[1]})
            if (e) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

// The ordered PFADD / PFCOUNT stream (rbx_hll_stream): one call at a time holds these.
struct HllStreamScratch {
    DevBuf cmds;     // the call's element offsets (n + 1 u64), then its keys (n u32)
    DevBuf changed;  // one word per command, then the promotion words read back after an add run
    DevBuf sort;     // the grouped path's cells, positions and rocPRIM's temporary storage
    DevBuf lists;    // the sparse keys' element lists of a chunk (HllReplay::list)
    DevBuf ptrs;     // the sparse keys' state words of a run, for the promotion readback
    CachedTable<rbx::HllKey> keys;  // the key table
};

// Grouped PFCOUNT unions and PFMERGEs (rbx_hll_count_groups / rbx_hll_merge_groups): one call at a
// time holds these.
struct HllGroupsScratch {
    DevBuf table;  // one launch's offsets | destinations | member pointers, uploaded in one copy
    DevBuf histo;  // 64 bins per group
    DevBuf out;    // one count per group; a merge phase's promotion words
    DevBuf ptrs;   // the state words of a merge phase's keys, for the promotion readback
};

// HLL register pool (chunks of kHllPerChunk x 16 KiB) and PFADD's uploaded tables.
struct HllPool {
    struct Slot {
        uint8_t *regs;
        uint32_t *state;
        uint16_t *ops;
    };
    std::vector<uint8_t *> chunks;
    std::vector<Slot> avail;  // zeroed slots (registers, state words, sparse opcodes)
    std::vector<Slot> dirty;  // slots of deleted HLLs, zeroed together when `avail` runs out
    DevBuf zero_ptrs;         // their pointers for k_hll_zero
    CachedTable<rbx::HllSeg> tiles;      // k_hll_pfadd tile list (cached for single-round calls)
    CachedTable<rbx::HllReplay> replay;  // k_hll_sparse_replay items
    DevBuf pack;                         // contiguous registers for the RCCL merge
    HllStreamScratch strm;
    HllGroupsScratch grp;
    void free_chunks() {
        for (auto *p : chunks) (void)hipFree(p);
        chunks.clear();
        avail.clear();
        dirty.clear();
    }
    ~HllPool() { free_chunks(); }
};

struct BitsetScratch {
    DevBuf idx, bitop_srcs;             // uploaded indexes, the BITOP source table
    DevBuf fld_vals, fld_out, fld_sort;  // BITFIELD: uploaded values, replies, the grouped path's sort scratch
    DevBuf fld_nil, fld_cmds;            // BITFIELD: the nil mask, the uploaded sub-commands of a mixed list
    DevBuf rng_args, rng_out, rng_dir;   // ranged BITCOUNT / BITPOS batches: starts | ends, replies, the block directory
    DevBuf rng_pos;                      // the single search's running minimum and chunk ticket
    // the GETBIT / SETBIT stream: the host form's uploaded keys | ops, canonical ids | wrong-type flags, the
    // summary words | per-key maxima, the grouped path's sort scratch, and the key table
    DevBuf bst_cmds, bst_keys, bst_sum, bst_sort;
    CachedTable<rbx::BitKey> bst_table;
    // the BITFIELD stream shares bst_keys, bst_sum, bst_sort and bst_table (one call at a time holds them);
    // its host form uploads commands | keys here and answers through fld_out and fld_nil
    DevBuf fst_cmds;
    // grouped BITOPs / BITCOUNTs (rbx_bitset_op_groups): one phase's group records | first tiles |
    // sources in one upload, the length words' pointers and values of the call's keys, one count per group
    DevBuf grp_table, grp_lens, grp_counts;
    PinBuf grp_pin;  // where the lengths and then the counts come back to (a pageable target costs a staging copy)
    // the read queries over many keys (rbx_bitset_range_stream): the host form's uploaded commands |
    // keys, its replies and status, a chunk's summary words, and its long list (8 bytes per command of a chunk)
    DevBuf rs_cmds, rs_out, rs_status, rs_sum, rs_long;
    // set-bit enumeration and the BitSet exchange (rbx_bitset_members / _as_words / _set_words): the
    // page's state words | the host forms' counts, and the host forms' positions or words on the device (the
    // enumeration's directory is rng_dir)
    DevBuf mem_state, mem_buf;
    // the enumeration over many keys (rbx_bitset_members_stream) shares bst_table, rs_cmds (commands | keys), rs_out
    // (the host form's offsets), rs_status, rs_sum and rs_long with the range stream; its own: the tiles' counts
    DevBuf mem_tiles;
    // the byte commands (rbx_string_*).  The single calls: the host forms' bytes on the device.  The
    // stream shares bst_table and bst_sort (the sorted pairs); its own: the keys' running states, the plan words (8
    // bytes per command of the call), the summary words, a chunk's cursors | run list and its long list, the host
    // form's commands | keys, values, offsets, replies | status and read bytes, and where states and total come back to
    DevBuf by_bytes, by_state, by_plan, by_sum, by_runs, by_long, by_cmds, by_vals, by_off, by_replies, by_out;
    PinBuf by_pin;
};

// Buffers more than one subsystem uses; one call at a time holds them (CallScope orders the calls).
struct SharedScratch {
    DevBuf zmask;       // add(): table path, chunked multi-tenant add, stream -- per key zero-bit masks
    DevBuf misc;        // per-segment counts (multi_host), PFADD changed words, PFCOUNT results
    DevBuf counters;    // 64 bytes of count words: Bloom host calls, BITCOUNT, digest, stream, RBitSet
    DevBuf ptrs, histo;  // register pointers and histograms: PFCOUNT, PFMERGE, register packing
    DevBuf tile_segs;   // each 256-key tile's first segment: multi-tenant contains and add, the table path
    DevBuf wide_table;  // first-setter table of |size| > 2^32 adds (bloom_wide_op)
};

struct DeviceState {
    FirstSetterTable fst;
    T8Table t8;
    FilterTable filt;
    StreamScratch strm;
    PartitionedContainsScratch pc;
    PartitionedAddScratch pa;
    Staging stage;
    HllPool hll;
    BitsetScratch bits;
    SharedScratch shared;
};

struct rbx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    rbx::Keyspace ks;  // names -> objects, and the context lock (ks.mu)
    // references: the API (rbx_init .. rbx_shutdown) + every open handle + every live HLL
    // state; the context's memory is released with the last one
    std::atomic<int> refs{1};
    bool shut = false;  // rbx_shutdown ran: device resources are gone, calls fail

    // every device and pinned allocation of the context; gone after rbx_shutdown, so reached only behind
    // RBX_ENTER / set_device (which fail on `shut`) or an explicit check of `shut` under the lock
    std::optional<DeviceState> dev{std::in_place};

    std::shared_ptr<SlabPool> slab = std::make_shared<SlabPool>();

    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;

    // stream order of the scratch above across calls issued on different streams (CallScope)
    hipEvent_t ev_scratch = nullptr;
    hipStream_t scratch_stream = nullptr;

    // the asynchronous entry points' serial executor (host_exec.h): its thread starts with the
    // first *_async call.  exec_mu guards the pointer: rbx_shutdown takes the executor out under
    // it, so a submit either lands before (and runs) or is refused.
    std::mutex exec_mu;
    std::unique_ptr<rbx::SerialExecutor> exec = std::make_unique<rbx::SerialExecutor>();
};

struct rbx_future {
    std::shared_ptr<rbx::Future> f;
};


inline void ctx_release(rbx_ctx *c) {
    if (c->refs.fetch_sub(1) == 1) delete c;
}

namespace rbx {

inline int set_device(rbx_ctx *c) {
    if (c->shut) return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    HIP_TRY(hipSetDevice(c->device));
    return RBX_OK;
}

inline hipStream_t pick_stream(rbx_ctx *c, void *s) { return s ? (hipStream_t)s : c->stream; }

// Every call that enqueues work touching the context's scratch (first-setter table, pair
// buckets, staging, descriptor tables, counters) or fills newly allocated object memory runs on
// the device after the previous such call, also when the two were issued on different streams:
// the new stream waits on an event the previous user recorded.  (The host mutex orders the
// calls; this orders their kernels.)
// CallScope opens such a call in the one safe order: the context lock, then the shutdown check and
// hipSetDevice (nothing touches ev_scratch on a shut context), then that wait.  Its destructor records
// the event -- only if the constructor got that far -- and then drops the lock.  The caller picks the
// stream (pick_stream) first.  Scopes nest on one thread (the mutex is recursive: rbx_bloom_stream calls
// rbx_bloom_stream_dev, and the copies between contexts enter the destination, under their own).
// RBX_ENTER is an entry point's whole preamble.
struct CallScope {
    std::lock_guard<std::recursive_mutex> lock;
    rbx_ctx *const c;
    const hipStream_t st;
    const int rc;  // RBX_OK, or why the call cannot run
    CallScope(rbx_ctx *c_, hipStream_t st_) : lock(c_->ks.mu), c(c_), st(st_), rc(set_device(c_)) {
        if (rc == RBX_OK && c->ev_scratch && c->scratch_stream && c->scratch_stream != st)
            (void)hipStreamWaitEvent(st, c->ev_scratch, 0);
    }
    ~CallScope() {
        if (rc == RBX_OK && c->ev_scratch && hipEventRecord(c->ev_scratch, st) == hipSuccess) c->scratch_stream = st;
    }
};

#define RBX_ENTER(ctx, stream) rbx::CallScope scope_((ctx), (stream)); RBX_TRY(scope_.rc)

// ---- shared constants -----------------------------------------------------------------------------
static constexpr size_t kHllBytes = 16384;
static constexpr size_t kHllPerChunk = 4096;  // 192 MiB per pool chunk
static constexpr size_t kHllStateWords = 4;   // HllReplay::state, 16 bytes
// Opcode list capacity per pooled HLL.  A sparse string's opcodes never outnumber its bytes, and
// hllSparseSet promotes instead of growing a string past hll-sparse-max-bytes (3000), so a
// PFADD-built string fits 3072 entries (6 KiB per HLL instead of 32 KiB); a SET string
// longer than that (up to 16384 opcodes) moves to its own allocation (hll_ops_reserve), and
// from then on it can only shrink or promote.
static constexpr size_t kHllSlotOps = 3072;
static constexpr size_t kHllOpsBytes = kHllSlotOps * 2;
static constexpr size_t kHllMaxOps = 16384;

constexpr const char *kWrongTypeMsg = "WRONGTYPE Operation against a key holding the wrong kind of value";
// what RBitSet's single-key calls and their many-key forms both report (api_bitset.cpp, api_bitset_multi.cpp)
constexpr const char *kFieldTypeMsg =
    "ERR Invalid bitfield type. Use something like i16 u8. Note that u64 is not supported but i64 is.";
constexpr const char *kBitopNotMsg = "ERR BITOP NOT must be called with a single source key.";

// the small host tier's pinned block (api_staging.cpp): zeroed result area ahead of the keys (counts, changed words)
static constexpr uint64_t kSmallHead = 64 << 10;
// the tiny host tier's coherent block (api_staging.cpp)
static constexpr uint64_t kTinyBytes = 64 << 10;
// block: flags | segment offsets | key bytes | key offsets (every segment holds a key: nseg <= n)
// (regions 64-byte aligned: 16-byte keys at a 16-byte boundary take the kernels' fixed-length loads, fast_len)
static constexpr uint64_t kTinySegAt = kSegMaxKeys, kTinyKeysAt = kTinySegAt + (kSegMaxKeys + 8) * 8;
static constexpr uint64_t kTinyOffsAt = kTinyKeysAt + kTinyBytes;
// then the small tables a call would upload (PFADD's tile list and sparse-replay items: TinyArena)
static constexpr uint64_t kTinyArenaAt = kTinyOffsAt + (kSegMaxKeys + 8) * 8, kTinyArenaBytes = 64 << 10;
static_assert(kTinyKeysAt % 64 == 0 && kTinyOffsAt % 64 == 0 && kTinyArenaAt % 64 == 0, "aligned regions");
static constexpr uint64_t kTinyDoneAt = kTinyArenaAt + kTinyArenaBytes;  // one-key kernels' completion word
static constexpr size_t kTinyBlock = kTinyDoneAt + 64;

// ---- helpers that cross a file boundary (api_staging.h has the staging tiers') ----------------------
inline bool bad_name(const rbx_name &n) { return !n.bytes && n.len; }

// the significant bits of v: 0 for 0, 64 for a value with bit 63 set (a shift by 64 is undefined)
inline int significant_bits(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// The grouped paths' sort (rbx_kernels.h, cell_sort.hip): sort_failed turns what it or a launch_*_grouped
// returns into the call's error; cell_sort_reserve sizes `buf` for n pairs sorted over [begin_bit, end_bit).
inline int sort_failed(int e) {
    return e ? fail(RBX_E_DEVICE, std::string("radix sort: ") + hipGetErrorString((hipError_t)e)) : RBX_OK;
}
template <class Cell> int cell_sort_reserve(DevBuf &buf, uint32_t n, int begin_bit, int end_bit) {
    size_t bytes = 0;
    RBX_TRY(sort_failed(cell_sort_scratch_bytes<Cell>(n, begin_bit, end_bit, &bytes)));
    return buf.reserve(bytes);
}

std::string name_of(const rbx_name &n);
// The names of one multi-key stream call (rbx_bitset_stream, rbx_bitset_field_stream, rbx_hll_stream), resolved
// once, lookup only, under the context lock.  Equal names are one key, known by its first entry: canon[i] = the
// first entry with entry i's bytes (its canonical id).  wrong[i] = the key holds another type than `expect`, which
// fails its commands.  canon and wrong are the caller's arrays of nkeys entries, in whatever form it keeps them;
// found(i, entry) is called for each canonical key that exists with the expected type, while the entry is at
// hand.  Returns "some key is wrong".
template <class Found>
bool stream_names_resolve(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, KType expect, std::vector<std::string> *nm,
                          uint32_t *canon, uint8_t *wrong, Found found) {
    bool any_wrong = false;
    nm->resize(nkeys);
    std::unordered_map<std::string, uint32_t> first;
    first.reserve(nkeys);
    for (uint32_t i = 0; i < nkeys; ++i) {
        (*nm)[i] = name_of(names[i]);
        canon[i] = first.emplace((*nm)[i], i).first->second;
        if (canon[i] != i) {
            wrong[i] = wrong[canon[i]];
            continue;
        }
        const Entry *e = c->ks.find((*nm)[i]);
        wrong[i] = e && e->type != expect;
        if (wrong[i]) any_wrong = true;
        else if (e) found(i, *e);
    }
    return any_wrong;
}
// rbx_api.cpp
// NULL context, NULL names, a name of NULL bytes with a length
int stream_names_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys);
int new_bitmap(rbx_ctx *c, uint64_t size_bits, hipStream_t st, std::shared_ptr<Bitmap> *out);
int grow_bitmap(rbx_ctx *c, Bitmap &b, uint64_t size_bits, hipStream_t st);
uint64_t read_dev_u64(rbx_ctx *c, const unsigned long long *p, int *rc);
int check_offsets(int64_t size);
int names_of(const rbx_name *names, uint32_t n, std::vector<std::string> *out);
int cstr_names(const char *const *names, uint32_t n, std::vector<std::string> *out);
int bitmap_for(rbx_ctx *c, const std::string &name, uint64_t nbits, bool create, hipStream_t st,
               std::shared_ptr<Bitmap> *out);
uint64_t import_bits(rbx_ctx *c, const std::string &name, uint64_t len);
int bitmap_export(rbx_ctx *c, const std::string &name, uint8_t *out, uint64_t cap, uint64_t *redis_len);
int bitmap_import(rbx_ctx *c, const std::string &name, const uint8_t *bytes, uint64_t len);
int quiesce(rbx_ctx *c);
// api_bloom.cpp
int run_add(rbx_ctx *c, const KeysDev &keys, const FilterDesc *d_filt, const uint64_t *d_seg_off, uint32_t nseg,
            const FilterDesc &single, uint32_t kmax, uint8_t *d_out_new, unsigned long long *d_count,
            unsigned long long *d_seg_counts, hipStream_t st);
FilterDesc desc_of(const Bitmap &b, uint64_t size, uint32_t k, uint32_t fid);
KeysDev keys_dev(const rbx_keys *k);
int bloom_bind(rbx_ctx *c, rbx_bloom *b, bool create, hipStream_t st, bool *absent);
int bitcount_locked(rbx_ctx *c, const std::string &name, uint64_t *out);
// api_bitset.cpp
int bitset_find(rbx_ctx *c, const std::string &name, std::shared_ptr<Bitmap> *out);
int bitset_for_write(rbx_ctx *c, const std::string &name, uint64_t need_bytes, hipStream_t st, std::shared_ptr<Bitmap> *out);
int byte_cmd_failed(int kind);
// api_hll.cpp
int hll_add_multi(rbx_ctx *c, const std::vector<std::string> &names, const uint64_t *seg_offsets,
                  const rbx_keys *elements, uint8_t *out_changed);
int hll_count(rbx_ctx *c, const std::vector<std::string> &names, uint64_t *out);
int hll_merge(rbx_ctx *c, const std::string &dest, const std::vector<std::string> &srcs);
}  // namespace rbx
