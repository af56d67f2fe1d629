// rbx_ctx.h -- private to csrc/ (never included from include/): the context, its device objects and the
// call scope, shared by the host translation units of librbx.so (rbx_api.cpp and the api_*.cpp files).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
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

// ---- device buffers ---------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int reserve(size_t n) {
        if (n <= cap) return RBX_OK;
        if (p) {
            (void)hipFree(p);
            p = nullptr;
            cap = 0;
        }
        size_t want = std::max<size_t>(n, 4096);
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return RBX_OK;
    }
    template <class T> T *as() const { return (T *)p; }
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

struct rbx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    rbx::Keyspace ks;  // names -> objects, and the context lock (ks.mu)
    // references: the API (rbx_init .. rbx_shutdown) + every open handle + every live HLL
    // state; the context's memory is released with the last one
    std::atomic<int> refs{1};
    bool shut = false;  // rbx_shutdown ran: device resources are gone, calls fail

    // Every DevBuf below is freed by rbx_shutdown from a list of its own: add a new one there too.
    // first-setter table for add()
    DevBuf table;
    uint32_t log2cap = 0;
    uint32_t epoch = 255;  // 255 = table needs (re)initialisation
    DevBuf zmask;

    // staging for host-buffer calls
    DevBuf keys_bytes, keys_offs, out_bytes, seg_offs, counters, filt_table, ptrs, histo, misc, tile_segs, hll_tiles;
    DevBuf probe_table;  // ProbeDesc per entry of filt_table
    DevBuf pc_bits, pc_cnt, pc_pairs, pc_mrec;  // partitioned contains
    DevBuf pa_p1, pa_p2, pa_cnt, pa_bits, pa_ctr, pa_recs;  // partitioned add
    DevBuf pa_stamps;  // add_partition_diag & 64: region-pass phase times (rbx_bench_add_stamps)
    DevBuf st_adds, st_nadds;    // ordered stream: add list, one add counter per chunk
    DevBuf st_t8;                // ordered stream (r04): 8-byte first-setter table (EMPTY between chunks)
    DevBuf st_fslot;             // ordered stream (r05): per add, the slot of its first zero bit's claim
    DevBuf madd_c;               // multi-tenant add (r05): conflict table C + its MaddxState (+ the `big` flag)
    uint64_t madd_maxseg_hint = ~0ULL;  // set by the host-arena add_multi: its largest segment (keys)
    uint64_t st_t8_entries = 0;  // initialized size of st_t8
    uint64_t st_geom[4] = {0, 0, 0, 0};             // last stream call: bb, fbits, pb, chunk
    DevBuf fid_table;            // bitmap words per table id (fid) of the filters of filt_table
    uint32_t filt_nfids = 0;     // distinct table ids of filt_table
    uint64_t filt_maxbits = 0;   // the largest of their bitmaps, in bits
    // all-zero words standing in for a missing bitmap in multi-tenant contains (GETBIT on a
    // missing key reads 0; the key is not created), grown on demand, never written by a kernel
    DevBuf zero_bm;
    DevBuf hll_pack;                                // contiguous registers for the RCCL merge
    DevBuf wide_table;  // first-setter table of |size| > 2^32 adds (bloom_wide_op)
    DevBuf bits_idx, bitop_srcs;  // RBitSet: uploaded indexes, the BITOP source table
    DevBuf fld_vals, fld_out, fld_sort;  // BITFIELD: uploaded values, replies, the grouped path's sort scratch
    std::vector<rbx::HllSeg> tile_cache;  // content of hll_tiles (valid when tiles_valid)
    bool tiles_valid = false;
    std::vector<rbx::FilterDesc> filt_cache;  // content of filt_table
    uint64_t filt_generation = 0;
    // the handle list filt_table was built from (fast path for repeated multi-tenant calls)
    std::vector<std::pair<const rbx_bloom *, uint64_t>> filt_keys;
    uint64_t filt_key_generation = ~0ULL, filt_bytes = 0;
    bool filt_create = false;
    uint32_t filt_kmax = 1;

    std::shared_ptr<SlabPool> slab = std::make_shared<SlabPool>();

    // HLL register pool: chunks of kHllPerChunk x 16 KiB
    std::vector<uint8_t *> hll_chunks;
    struct HllSlot {
        uint8_t *regs;
        uint32_t *state;
        uint16_t *ops;
    };
    std::vector<HllSlot> hll_free;   // zeroed slots (registers, state words, sparse opcodes)
    std::vector<HllSlot> hll_dirty;  // slots of deleted HLLs, zeroed together when hll_free runs out
    DevBuf hll_zero_ptrs;            // their pointers for k_hll_zero
    DevBuf hll_checks;                     // k_hll_sparse_replay items (cached by content)
    std::vector<rbx::HllReplay> check_cache;

    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;

    // host-buffer pipeline: uploads on copy_stream into two device slots while the
    // previous slot's kernels run on the compute stream
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    DevBuf slot_bytes[2], slot_offs[2];
    uint64_t staging_bytes = 64ull << 20;
    // small host batches (bloom_host_small): a pinned copy of the keys, uploaded on `stream` with the
    // zeroed count word in one transfer; the count and flags come back into it
    void *pin_small = nullptr;
    size_t pin_small_cap = 0;
    uint64_t pin_small_limit = 0;  // the host_small_bytes the block was laid out for (its tail offset)
    unsigned long long *pin_word = nullptr;  // pinned readback words (counts, the partitioned add's overflow flag)
    // tiny host batches (bloom_host_tiny): coherent pinned memory the kernel reads the keys from and
    // writes the flags into, no transfer on either side
    uint8_t *pin_tiny = nullptr, *pin_tiny_dev = nullptr;
    uint32_t tiny_seq = 0;  // the last completion word a one-key kernel stored into the block

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
// stream (pick_stream) first.  Scopes nest on one thread (the mutex is recursive: multi_host calls the
// public *_multi_dev entry points under its own).  RBX_ENTER is an entry point's whole preamble.
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
// rbx_api.cpp
int new_bitmap(rbx_ctx *c, uint64_t size_bits, hipStream_t st, std::shared_ptr<Bitmap> *out);
int grow_bitmap(rbx_ctx *c, Bitmap &b, uint64_t size_bits, hipStream_t st);
uint64_t read_dev_u64(rbx_ctx *c, const unsigned long long *p, int *rc);
int check_offsets(int64_t size);
std::string name_of(const rbx_name &n);
int names_of(const rbx_name *names, uint32_t n, std::vector<std::string> *out);
int cstr_names(const char *const *names, uint32_t n, std::vector<std::string> *out);
int bitmap_for(rbx_ctx *c, const std::string &name, uint64_t nbits, bool create, hipStream_t st,
               std::shared_ptr<Bitmap> *out);
uint64_t import_bits(rbx_ctx *c, const std::string &name, uint64_t len);
int bitmap_export(rbx_ctx *c, const std::string &name, uint8_t *out, uint64_t cap, uint64_t *redis_len);
int bitmap_import(rbx_ctx *c, const std::string &name, const uint8_t *bytes, uint64_t len);
int quiesce(rbx_ctx *c);
// api_bloom.cpp
int ensure_table(rbx_ctx *c, uint64_t want_pairs, hipStream_t st);
int run_add(rbx_ctx *c, const KeysDev &keys, const FilterDesc *d_filt, const uint64_t *d_seg_off, uint32_t nseg,
            const FilterDesc &single, uint32_t kmax, uint8_t *d_out_new, unsigned long long *d_count,
            unsigned long long *d_seg_counts, hipStream_t st);
FilterDesc desc_of(const Bitmap &b, uint64_t size, uint32_t k, uint32_t fid);
KeysDev keys_dev(const rbx_keys *k);
int bloom_bind(rbx_ctx *c, rbx_bloom *b, bool create, hipStream_t st, bool *absent);
int bitcount_locked(rbx_ctx *c, const std::string &name, uint64_t *out);
// api_hll.cpp
int hll_add_multi(rbx_ctx *c, const std::vector<std::string> &names, const uint64_t *seg_offsets,
                  const rbx_keys *elements, uint8_t *out_changed);
int hll_count(rbx_ctx *c, const std::vector<std::string> &names, uint64_t *out);
int hll_merge(rbx_ctx *c, const std::string &dest, const std::vector<std::string> &srcs);
}  // namespace rbx
