// rbx_api.cpp -- librbx.so host side: context life cycle, bitmap allocation, key-level calls, the async
// forms, self tests and rbx_tune.  The subsystems are in the api_*.cpp files; rbx_ctx.h is what they share.
//
// The keyspace mirrors how Redisson lays the structures out in Redis:
//   name          -> bitmap string (Bloom) | HLL string
//   {name}:config -> Bloom config hash    (RedissonObject.suffixName, M/RedissonObject.java:77-82)
// so delete/exists/rename keep the reference's key-level semantics.
// M/ = /root/reference/redisson/src/main/java/org/redisson/
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rbx_ctx.h"
#include "tunables.h"

namespace rbx {

Tunables g_tune;

// A zeroed bitmap of size_bits bits; the fill runs on `st` inside the caller's CallScope.
int new_bitmap(rbx_ctx *c, uint64_t size_bits, hipStream_t st, std::shared_ptr<Bitmap> *out) {
    auto b = std::make_shared<Bitmap>();
    b->device = c->device;
    uint64_t bytes = ((size_bits + 7) / 8 + 255) & ~255ULL;
    if (bytes == 0) bytes = 256;
    if (bytes <= SlabPool::kMaxSmall) {  // words + a 256-byte tail holding the length word
        uint8_t *p = (uint8_t *)c->slab->get(bytes + 256);
        if (!p) return fail(RBX_E_OOM, "bitmap slab allocation failed");
        b->pool = c->slab;
        b->d_words = (uint32_t *)p;
        b->d_len = (unsigned long long *)(p + bytes);
    } else {
        HIP_TRY(hipMalloc(&b->d_words, bytes));
        HIP_TRY(hipMalloc(&b->d_len, sizeof(unsigned long long)));
    }
    if (b->pool) {  // the words and the length word's 256-byte tail: one fill
        HIP_TRY(hipMemsetAsync(b->d_words, 0, bytes + 256, st));
    } else {
        HIP_TRY(hipMemsetAsync(b->d_words, 0, bytes, st));
        HIP_TRY(hipMemsetAsync(b->d_len, 0, sizeof(unsigned long long), st));
    }
    b->cap_bytes = bytes;
    c->ks.generation++;
    *out = b;
    return RBX_OK;
}

int grow_bitmap(rbx_ctx *c, Bitmap &b, uint64_t size_bits, hipStream_t st) {
    uint64_t bytes = ((size_bits + 7) / 8 + 255) & ~255ULL;
    if (bytes <= b.cap_bytes) return RBX_OK;
    // always move to a dedicated allocation (words + length word)
    uint32_t *nw = nullptr;
    unsigned long long *nl = nullptr;
    HIP_TRY(hipMalloc(&nw, bytes));
    HIP_TRY(hipMalloc(&nl, sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(nw, 0, bytes, st));
    HIP_TRY(hipMemcpyAsync(nw, b.d_words, b.cap_bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(nl, b.d_len, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (b.pool) {
        b.pool->put(b.d_words, b.cap_bytes + 256);
        b.pool.reset();
    } else {
        HIP_TRY(hipFree(b.d_words));
        HIP_TRY(hipFree(b.d_len));
    }
    b.d_words = nw;
    b.d_len = nl;
    b.cap_bytes = bytes;
    c->ks.generation++;
    return RBX_OK;
}

uint64_t read_dev_u64(rbx_ctx *c, const unsigned long long *p, int *rc) {
    unsigned long long v = 0;
    // into a pinned word: a pageable destination costs the runtime a staging copy
    unsigned long long *w = c->dev->stage.words();
    hipError_t e = hipMemcpyAsync(w, p, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) v = *w;
    *rc = e == hipSuccess ? RBX_OK : fail(RBX_E_DEVICE, hipGetErrorString(e));
    return v;
}

// Redis bit offsets end at 2^32 - 1: a filter whose |size| exceeds 2^32 (only reachable through
// tryInit with a negative expectedInsertions, M/RedissonBloomFilter.java:270-276) gets the error
// SETBIT/GETBIT would reply with.
int check_offsets(int64_t size) {
    if (size_bits(size) > kEngineMaxSize) return fail(RBX_E_REDIS, "ERR bit offset is not an integer or out of range");
    return RBX_OK;
}

// Names arrive as NUL-terminated strings or, in the *_n forms, as (bytes, length) pairs that may
// hold any byte (Spring Data's byte[] keys, RedissonConnection.java:2203).
std::string name_of(const rbx_name &n) { return std::string((const char *)n.bytes, (size_t)n.len); }

static int read_config(rbx_ctx *c, const std::string &name, rbx_bloom_config *out) {
    BloomConfig cfg;
    RBX_TRY(ks_get_config(c->ks, name, &cfg));
    out->size = cfg.size;
    out->hash_iterations = cfg.k;
    out->expected_insertions = cfg.expected;
    out->false_probability = cfg.fpp;
    snprintf(out->false_probability_str, sizeof out->false_probability_str, "%s", cfg.fpp_str.c_str());
    return RBX_OK;
}

// bitmap key for add (created by the first SETBIT) / contains (may be absent).  size_bits_ =
// |size|; a new or grown bitmap is zero-filled on `st` (the caller holds a CallScope on it).
int bitmap_for(rbx_ctx *c, const std::string &name, uint64_t nbits, bool create, hipStream_t st,
               std::shared_ptr<Bitmap> *out) {
    Entry *e = c->ks.find(name);
    if (e) {
        if (e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
        RBX_TRY(grow_bitmap(c, *e->bm, nbits, st));
        *out = e->bm;
        return RBX_OK;
    }
    if (!create) {
        out->reset();
        return RBX_OK;
    }
    std::shared_ptr<Bitmap> b;
    RBX_TRY(new_bitmap(c, nbits, st, &b));
    c->ks.put(name, Entry{KType::Bitmap, nullptr, b, nullptr});
    *out = b;
    return RBX_OK;
}

// DEL / EXISTS over any keys (binary names)
int names_of(const rbx_name *names, uint32_t n, std::vector<std::string> *out) {
    if (n && !names) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL names");
    out->clear();
    for (uint32_t i = 0; i < n; ++i) {
        if (bad_name(names[i])) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL key name");
        out->push_back(name_of(names[i]));
    }
    return RBX_OK;
}

int stream_names_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys) {
    if (!c || (nkeys && !names)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    for (uint32_t i = 0; i < nkeys; ++i)
        if (bad_name(names[i])) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL key name");
    return RBX_OK;
}

int cstr_names(const char *const *names, uint32_t n, std::vector<std::string> *out) {
    if (n && !names) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL names");
    out->clear();
    for (uint32_t i = 0; i < n; ++i) {
        if (!names[i]) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL key name");
        out->emplace_back(names[i]);
    }
    return RBX_OK;
}

int bitmap_export(rbx_ctx *c, const std::string &name, uint8_t *out, uint64_t cap, uint64_t *redis_len) {
    RBX_ENTER(c, c->stream);
    Entry *e = c->ks.find(name);
    if (!e) {
        if (redis_len) *redis_len = 0;
        return RBX_OK;
    }
    if (e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    int rc;
    uint64_t len = read_dev_u64(c, e->bm->d_len, &rc);
    RBX_TRY(rc);
    if (redis_len) *redis_len = len;
    uint64_t n = std::min(cap, len);
    if (out && n) {
        HIP_TRY(hipMemcpyAsync(out, e->bm->d_words, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return RBX_OK;
}

// bits a bitmap imported under `name` must cover: the string, and the config's |size|
uint64_t import_bits(rbx_ctx *c, const std::string &name, uint64_t len) {
    uint64_t bits = len * 8;
    Entry *cfg = c->ks.find(config_name(name));
    if (cfg && cfg->type == KType::Config) bits = std::max<uint64_t>(bits, size_bits(cfg->cfg->size));
    return std::min<uint64_t>(bits, kEngineMaxSize);
}

int bitmap_import(rbx_ctx *c, const std::string &name, const uint8_t *bytes, uint64_t len) {
    if (len > (1ULL << 29)) return fail(RBX_E_ILLEGAL_ARGUMENT, "string exceeds the 512 MiB Redis limit");
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> b;
    RBX_TRY(new_bitmap(c, import_bits(c, name, len), c->stream, &b));
    if (len) HIP_TRY(hipMemcpyAsync(b->d_words, bytes, len, hipMemcpyHostToDevice, c->stream));
    unsigned long long L = len;
    HIP_TRY(hipMemcpyAsync(b->d_len, &L, 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ks.put(name, Entry{KType::Bitmap, nullptr, b, nullptr});
    return RBX_OK;
}

// ---- asynchronous forms (RHyperLogLogAsync, M/api/RHyperLogLogAsync.java:37-70) ---------------
// The call is queued on the context's serial executor (host_exec.h) and runs after every call
// queued before it; names, segment offsets and the rbx_keys descriptor are copied at submit time,
// key bytes and output buffers are read / written when the call runs (valid until completion).
static int submit_async(rbx_ctx *c, std::function<int()> fn, rbx_callback cb, void *user, rbx_future **out) {
    if (!c || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    // exec_mu is held through the submit, so rbx_shutdown cannot free the executor under it; the
    // queued call holds a context reference until it has run (the context outlives a shutdown
    // issued from a completion callback while calls are still queued).
    std::lock_guard<std::mutex> g(c->exec_mu);
    if (!c->exec) return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    c->refs.fetch_add(1);
    auto f = c->exec->submit(
        [c, fn = std::move(fn)]() {
            const int rc = fn();
            ctx_release(c);
            return rc;
        },
        cb, user);
    if (!f) {
        ctx_release(c);
        return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    }
    *out = new rbx_future{std::move(f)};
    return RBX_OK;
}

// ---- sizeInMemory (M/RedissonObject.java:124-130, Bloom: both keys, M/RedissonBloomFilter.java:234-238)
// Bytes the engine holds for each existing key: a bitmap's device allocation (+ its 256-byte
// length-word tail), an HLL's 16384 register bytes, a config hash's fields; plus the key name.
// Redis' MEMORY USAGE reports its own allocator's figures, which no engine reproduces.
static int memory_usage(rbx_ctx *c, const std::vector<std::string> &names, uint64_t *bytes) {
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    uint64_t total = 0;
    for (const auto &nm : names) {
        Entry *e = c->ks.find(nm);
        if (!e) continue;
        total += nm.size();
        if (e->type == KType::Bitmap) total += e->bm->cap_bytes + 256;
        else if (e->type == KType::Hll) total += kHllBytes;
        else total += sizeof(BloomConfig) + e->cfg->fpp_str.size();
    }
    *bytes = total;
    return RBX_OK;
}

// ---- replicas: digest and device-to-device copies between contexts ---------------------------
// Waits until every engine call issued on `c` so far has finished on the device (the scratch
// event chain orders them all, whatever stream each used), so its objects can be read elsewhere.
int quiesce(rbx_ctx *c) {
    if (c->ev_scratch && c->scratch_stream) HIP_TRY(hipEventSynchronize(c->ev_scratch));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

static uint64_t mix64_host(uint64_t x) {
    x ^= x >> 31;
    x *= 0x7fb5d329728ea185ULL;
    x ^= x >> 27;
    x *= 0x81dadef4bc2dd44dULL;
    x ^= x >> 33;
    return x;
}

// ---- rbx_tune: one row per key (include/rbx_bench.h documents them) --------------------------------
struct TuneRow {
    const char *key;
    enum Kind { kRange, kOneOf, kBits, kPow2, kPow2Or0 } kind;  // v = {lo, hi} | the n values | {mask of the bits} | {lo, hi}
    int v[7], n;
    bool diag;            // exists only in the profiling build (kDiag, librbx_diag.so)
    void (*store)(int);   // a field of g_tune, or a set_* function of rbx_kernels.h
    bool accepts(int x) const {
        if (kind == kRange) return x >= v[0] && x <= v[1];
        if (kind == kPow2) return x >= v[0] && x <= v[1] && (x & (x - 1)) == 0;
        if (kind == kPow2Or0) return x == 0 || (x >= v[0] && x <= v[1] && (x & (x - 1)) == 0);
        if (kind == kBits) return (x & ~v[0]) == 0;
        return std::find(v, v + n, x) != v + n;
    }
    std::string wants() const {  // the tail of the rejection message
        if (kind == kRange || kind == kPow2 || kind == kPow2Or0)
            return std::string(kind == kPow2 ? ": a power of two" : kind == kPow2Or0 ? ": 0 or a power of two" : "") +
                   " in [" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + "]";
        std::string s;
        if (kind == kOneOf)
            for (int i = 0; i < n; ++i) s += (i ? ", " : "") + std::to_string(v[i]);
        else
            for (int b = 1; b <= v[0]; b <<= 1)
                if (v[0] & b) s += (s.empty() ? "" : "|") + std::to_string(b);
        return kind == kOneOf ? " in {" + s + "}" : ": bits of " + s;
    }
};
#define RANGE(lo, hi) TuneRow::kRange, {lo, hi}, 2
#define ONE_OF(...) TuneRow::kOneOf, {__VA_ARGS__}, (int)std::initializer_list<int>{__VA_ARGS__}.size()
#define BITS(mask) TuneRow::kBits, {mask}, 1
#define POW2(lo, hi) TuneRow::kPow2, {lo, hi}, 2
#define POW2_OR_0(lo, hi) TuneRow::kPow2Or0, {lo, hi}, 2
#define FIELD(f) [](int x) { g_tune.f = (decltype(g_tune.f.load()))x; }
static constexpr int kSegMax = (int)kSegMaxKeys, kIntMax = 0x7fffffff;
static const TuneRow kTuneRows[] = {
    {"contains_partition", RANGE(0, 2), false, FIELD(partition_mode)},
    {"contains_stage1_grid", RANGE(1, 256), false, FIELD(stage1_grid)},
    // DIAGNOSTICS ONLY (tools/microbench.py pflags / padiag through RBX_LIB_PATH): they change answers
    {"contains_partition_flags", ONE_OF(0, 4, 8, 12, 16, 32, 64), true, FIELD(partition_flags)},
    {"add_partition_diag", BITS(4 | 8 | 16 | 64), true, FIELD(add_partition_diag)},
    {"stream_diag", BITS(1 | 8), true, set_stream_diag},
    {"add_records", RANGE(0, 3), false, FIELD(add_record_policy)},
    {"add_partition", RANGE(0, 2), false, FIELD(add_partition_mode)},
    {"contains_multi_slots", RANGE(0, 2), false, FIELD(multi_slots)},
    {"stream_table8", RANGE(0, 1), false, FIELD(stream_table8)},
    {"stream_chunk", RANGE(0, kIntMax), false, FIELD(stream_chunk)},    // 0: 2^26 / k commands
    {"wide_subchunk", RANGE(0, kIntMax), false, FIELD(wide_subchunk)},  // 0: 2^29 / k keys
    {"contains_qgrid", RANGE(256, 8192), false, set_contains_qgrid},
    {"stream_qgrid", RANGE(256, 8192), false, set_stream_qgrid},
    {"add_multi_table8", ONE_OF(0, 2), false, FIELD(add_multi_t8)},
    {"add_multi_segment", RANGE(0, 1), false, FIELD(madd_seg)},
    {"add_multi_segmax", RANGE(1, kSegMax), false, FIELD(madd_segmax)},
    {"add_multi_conflict_log2", RANGE(6, 24), false, FIELD(maddx_lgc)},
    {"add_region_grid", RANGE(256, 65536), false, set_add_region_grid},
    {"add_multi_seg_grid", RANGE(64, 65536), false, FIELD(madd_seg_grid)},
    {"stream_final_grid", RANGE(32, 2048), false, set_stream_final_grid},
    {"host_small_bytes", RANGE(4096, 64 << 20), false, FIELD(small_bytes)},
    {"host_tiny_spin", RANGE(0, 1), false, FIELD(tiny_spin)},
    {"add_one_key", RANGE(0, 1), false, FIELD(add_one)},
    {"add_single_seg_keys", RANGE(0, kSegMax), false, FIELD(seg_single_keys)},
    {"host_tiny_keys", RANGE(0, kSegMax), false, FIELD(tiny_keys)},
    {"host_small_batches", RANGE(0, 1), false, FIELD(small_host)},
    {"add_rec_lds_limit", RANGE(0, 7168), false, set_add_rec_lds_limit},
    {"contains_stage1", RANGE(0, 5), false, set_contains_stage1},  // early-exit width of contains (0 = off)
    {"bitrange_pos_chunk", POW2(4096, 1 << 20), false, FIELD(bitrange_pos_chunk)},
    {"bitrange_chain_max", RANGE(0, kIntMax), false, FIELD(bitrange_chain_max)},
    {"bitrange_dir", RANGE(0, 2), false, FIELD(bitrange_dir)},
    {"bitfield_sat_atomic", RANGE(0, 1), false, FIELD(bitfield_sat_atomic)},
    {"bitstream_path", RANGE(0, 2), false, FIELD(bitstream_path)},
    {"bitstream_serial_max", RANGE(0, kIntMax), false, FIELD(bitstream_serial_max)},
    {"bitstream_chunk", RANGE(1, 1 << 30), false, FIELD(bitstream_chunk)},  // positions in a chunk are 32-bit
    {"fieldstream_path", RANGE(0, 3), false, FIELD(fieldstream_path)},
    {"fieldstream_serial_max", RANGE(0, kIntMax), false, FIELD(fieldstream_serial_max)},
    {"fieldstream_chunk", RANGE(1, 1 << 30), false, FIELD(fieldstream_chunk)},  // positions in a chunk are 32-bit
    {"hllstream_path", RANGE(0, 2), false, FIELD(hllstream_path)},
    {"hllstream_chunk", RANGE(1, 1 << 30), false, FIELD(hllstream_chunk)},  // positions in a chunk are 32-bit
    {"hllstream_elems_per_round", RANGE(1, kIntMax), false, FIELD(hllstream_elems_per_round)},
    {"hllgroups_split", ONE_OF(0, 1, 2, 4, 8, 16), false, FIELD(hllgroups_split)},
    {"bitgroups_tile", POW2_OR_0(4096, 1 << 20), false, FIELD(bitgroups_tile)},
    {"rangestream_lanes", ONE_OF(4, 8, 16, 32, 64), false, FIELD(rangestream_lanes)},
    {"rangestream_short_max", POW2(64, 1 << 20), false, FIELD(rangestream_short_max)},
    {"rangestream_tile", POW2(4096, 1 << 20), false, FIELD(rangestream_tile)},
    {"rangestream_chunk", RANGE(1, 1 << 30), false, FIELD(rangestream_chunk)},  // positions in a chunk are 30-bit
    {"members_lanes", ONE_OF(4, 8, 16, 32, 64), false, FIELD(members_lanes)},
    {"members_short_max", POW2(64, 1 << 20), false, FIELD(members_short_max)},
    {"members_tile", POW2(4096, 1 << 20), false, FIELD(members_tile)},
    {"members_chunk", RANGE(1, 1 << 30), false, FIELD(members_chunk)},
    {"bytestream_lanes", ONE_OF(4, 8, 16, 32, 64), false, FIELD(bytestream_lanes)},
    {"bytestream_short_max", POW2(64, 1 << 20), false, FIELD(bytestream_short_max)},
    {"bytestream_tile", POW2(4096, 1 << 20), false, FIELD(bytestream_tile)},
    {"bytestream_chunk", RANGE(1, 1 << 30), false, FIELD(bytestream_chunk)},  // positions in a chunk are 30-bit
    {"bytestream_serial_max", RANGE(0, kIntMax), false, FIELD(bytestream_serial_max)},
};
#undef RANGE
#undef ONE_OF
#undef BITS
#undef POW2
#undef POW2_OR_0
#undef FIELD

}  // namespace rbx

using namespace rbx;

extern "C" {

int rbx_abi_version(void) { return RBX_ABI_VERSION; }

const char *rbx_last_error(void) { return last_error_message(); }

int rbx_device_count(int *out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (out) *out = n;
    return RBX_OK;
}

int rbx_init(int device, rbx_ctx **out) {
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(RBX_E_DEVICE, "no HIP device available");
    if (device < 0 || device >= n) return fail(RBX_E_ILLEGAL_ARGUMENT, "device index out of range");
    auto *c = new rbx_ctx();
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    Staging &sg = c->dev->stage;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&sg.copy_stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipEventCreateWithFlags(&sg.ev_copied[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sg.ev_done[i], hipEventDisableTiming);
        if (e == hipSuccess && i == 0) e = hipEventCreateWithFlags(&c->ev_scratch, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = sg.pin_word.alloc(64, hipHostMallocDefault);
    if (e != hipSuccess) {
        delete c;
        return fail(RBX_E_DEVICE, hipGetErrorString(e));
    }
    *out = c;
    return RBX_OK;
}

// Frees the device resources now; the context object itself lives until its last handle is
// closed (closing a handle after shutdown is safe, every other call on it fails).
int rbx_shutdown(rbx_ctx *c) {
    if (!c) return RBX_OK;
    // Queued asynchronous calls run to completion first (they take the context lock themselves):
    // the executor is taken out under exec_mu (later submits are refused), then destroyed, which
    // runs its queue and joins its thread.  From a completion callback (the executor's own
    // thread) it cannot join itself: it is detached, runs what is queued -- those calls fail with
    // RBX_E_ILLEGAL_STATE once the context is shut -- and frees itself.
    std::unique_ptr<SerialExecutor> ex;
    {
        std::lock_guard<std::mutex> g(c->exec_mu);
        ex = std::move(c->exec);
    }
    if (ex) {
        if (ex->on_executor_thread()) SerialExecutor::release_from_inside(ex.release());
        else ex.reset();
    }
    {
        std::lock_guard<std::recursive_mutex> g(c->ks.mu);
        if (c->shut) return fail(RBX_E_ILLEGAL_STATE, "the context has already been shut down");
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();  // work queued on caller streams may still use the memory
        if (c->comm) ncclCommDestroy(c->comm);
        c->comm = nullptr;
        c->shut = true;  // from here on released HLL blocks are not recycled
        c->ks.clear();
        c->dev->hll.free_chunks();
        c->slab.reset();  // bitmaps still held by open handles keep their slab alive
        c->dev.reset();   // every buffer, the staging events, the pinned blocks, the copy stream
        if (c->ev_scratch) (void)hipEventDestroy(c->ev_scratch);
        c->ev_scratch = nullptr;
        if (c->stream) (void)hipStreamDestroy(c->stream);
        c->stream = nullptr;
    }
    ctx_release(c);
    return RBX_OK;
}

int rbx_synchronize(rbx_ctx *c) {
    if (!c) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx is NULL");
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    RBX_TRY(set_device(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

void *rbx_stream(rbx_ctx *c) { return c && !c->shut ? (void *)c->stream : nullptr; }

// ---- CRC16 / slots (keyspace.cpp) ------------------------------------------------------------
uint16_t rbx_crc16(const uint8_t *bytes, size_t len) { return crc16(bytes, len); }
int rbx_calc_slot(const uint8_t *key, size_t len) { return calc_slot(key, len); }
int rbx_slot_to_gpu(int slot, int n_gpus) { return slot_to_gpu(slot, n_gpus); }

int rbx_bloom_optimal_config(int64_t n, double p, int64_t *size, uint32_t *k) {
    int64_t s;
    uint32_t kk;
    RBX_TRY(optimal_config(n, p, kRedissonMaxSize, &s, &kk));
    if (size) *size = s;
    if (k) *k = kk;
    return RBX_OK;
}

// ---- Bloom: config (keyspace.cpp) -----------------------------------------------------------------
int rbx_bloom_try_init_n(rbx_ctx *c, rbx_name name, int64_t expected, double fpp, int *created) {
    if (!c || (!name.bytes && name.len)) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return ks_bloom_try_init(c->ks, name_of(name), expected, fpp, created);
}

int rbx_bloom_try_init(rbx_ctx *c, const char *name, int64_t expected, double fpp, int *created) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return ks_bloom_try_init(c->ks, name, expected, fpp, created);
}

int rbx_bloom_init_raw(rbx_ctx *c, const char *name, uint64_t size, uint32_t k, int *created) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return ks_bloom_init_raw(c->ks, name, size, k, created);
}

int rbx_bloom_read_config(rbx_ctx *c, const char *name, rbx_bloom_config *out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return read_config(c, name, out);
}

int rbx_bloom_read_config_n(rbx_ctx *c, rbx_name name, rbx_bloom_config *out) {
    if (!c || (!name.bytes && name.len) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return read_config(c, name_of(name), out);
}

// delete / isExists / rename / renamenx (keyspace.cpp)
int rbx_bloom_delete(rbx_ctx *c, const char *name, int *deleted) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_bloom_delete(c->ks, name, deleted);
}

int rbx_bloom_is_exists(rbx_ctx *c, const char *name, int *exists) {
    if (!c || !name || !exists) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_bloom_is_exists(c->ks, name, exists);
}

int rbx_bloom_rename(rbx_ctx *c, const char *name, const char *new_name) {
    if (!c || !name || !new_name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_bloom_rename(c->ks, name, new_name);
}

int rbx_bloom_renamenx(rbx_ctx *c, const char *name, const char *new_name, int *renamed) {
    if (!c || !name || !new_name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_bloom_renamenx(c->ks, name, new_name, renamed);
}

int rbx_del_n(rbx_ctx *c, const rbx_name *names, uint32_t n, int *deleted) {
    if (!c) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(names, n, &v));
    return ks_del(c->ks, v, deleted);
}

int rbx_exists_n(rbx_ctx *c, const rbx_name *names, uint32_t n, int *count) {
    if (!c) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(names, n, &v));
    return ks_exists(c->ks, v, count);
}

int rbx_bloom_export(rbx_ctx *c, const char *name, uint8_t *out, uint64_t cap, uint64_t *redis_len) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bitmap_export(c, name, out, cap, redis_len);
}

int rbx_bloom_import(rbx_ctx *c, const char *name, const uint8_t *bytes, uint64_t len) {
    if (!c || !name || (len && !bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bitmap_import(c, name, bytes, len);
}

// SET name <len bytes from a device buffer> (device-resident snapshot restore)
int rbx_bloom_import_dev(rbx_ctx *c, const char *name, const uint8_t *d_bytes, uint64_t len, void *stream) {
    if (!c || !name || (len && !d_bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (len > (1ULL << 29)) return fail(RBX_E_ILLEGAL_ARGUMENT, "string exceeds the 512 MiB Redis limit");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    const uint64_t bits = import_bits(c, name, len);
    std::shared_ptr<Bitmap> b;
    Entry *e = c->ks.find(name);
    if (e && e->type == KType::Bitmap && e->bm->cap_bytes >= ((bits + 7) / 8)) {
        b = e->bm;  // reuse in place (open handles keep seeing it)
        HIP_TRY(hipMemsetAsync(b->d_words, 0, b->cap_bytes, st));
    } else {
        RBX_TRY(new_bitmap(c, bits, st, &b));
    }
    if (len) HIP_TRY(hipMemcpyAsync(b->d_words, d_bytes, len, hipMemcpyDeviceToDevice, st));
    static thread_local unsigned long long L;
    L = len;
    HIP_TRY(hipMemcpyAsync(b->d_len, &L, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->ks.put(name, Entry{KType::Bitmap, nullptr, b, nullptr});
    return RBX_OK;
}

int rbx_future_wait(rbx_future *f, int64_t timeout_ms, int *call_rc) {
    if (!f) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL future");
    if (!f->f->wait(timeout_ms)) return fail(RBX_E_TIMEOUT, "the call has not completed");
    std::lock_guard<std::mutex> g(f->f->mu);
    if (call_rc) *call_rc = f->f->rc;
    if (f->f->rc) fail(f->f->rc, f->f->msg);  // rbx_last_error() on this thread = the call's message
    return RBX_OK;
}

int rbx_future_done(rbx_future *f, int *done) {
    if (!f || !done) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> g(f->f->mu);
    *done = f->f->done;
    return RBX_OK;
}

int rbx_future_free(rbx_future *f) {
    delete f;  // the executor keeps its own reference until the call completes
    return RBX_OK;
}

int rbx_bloom_add_async(rbx_ctx *c, const char *name, uint64_t size, uint32_t k, const rbx_keys *keys,
                        uint8_t *out_new, uint64_t *out_count, rbx_callback cb, void *user, rbx_future **out) {
    if (!c || !name || !keys) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::string nm(name);
    rbx_keys kc = *keys;
    return submit_async(c, [=]() { return rbx_bloom_add(c, nm.c_str(), size, k, &kc, out_new, out_count); }, cb,
                        user, out);
}

int rbx_bloom_contains_async(rbx_ctx *c, const char *name, uint64_t size, uint32_t k, const rbx_keys *keys,
                             uint8_t *out_present, uint64_t *out_count, rbx_callback cb, void *user,
                             rbx_future **out) {
    if (!c || !name || !keys) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::string nm(name);
    rbx_keys kc = *keys;
    return submit_async(c, [=]() { return rbx_bloom_contains(c, nm.c_str(), size, k, &kc, out_present, out_count); },
                        cb, user, out);
}

// addAsync / addAllAsync (:71-81)
int rbx_hll_add_async(rbx_ctx *c, const char *name, const rbx_keys *elements, int *changed, rbx_callback cb,
                      void *user, rbx_future **out) {
    if (!c || !name || !elements) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::string nm(name);
    rbx_keys kc = *elements;
    return submit_async(c, [=]() { return rbx_hll_add(c, nm.c_str(), &kc, changed); }, cb, user, out);
}

int rbx_hll_add_multi_async(rbx_ctx *c, const char *const *names, uint32_t nseg, const uint64_t *seg_offsets,
                            const rbx_keys *elements, uint8_t *out_changed, rbx_callback cb, void *user,
                            rbx_future **out) {
    if (!c || !names || !seg_offsets || !elements) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, nseg, &v));
    std::vector<uint64_t> seg(seg_offsets, seg_offsets + nseg + 1);
    rbx_keys kc = *elements;
    return submit_async(c, [=]() { return hll_add_multi(c, v, seg.data(), &kc, out_changed); }, cb, user, out);
}

// countAsync / countWithAsync (:84-94)
int rbx_hll_count_async(rbx_ctx *c, const char *const *names, uint32_t n, uint64_t *result, rbx_callback cb,
                        void *user, rbx_future **out) {
    if (!c || !names || !result || n == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, n, &v));
    return submit_async(c, [=]() { return hll_count(c, v, result); }, cb, user, out);
}

// mergeWithAsync (:97-102)
int rbx_hll_merge_async(rbx_ctx *c, const char *dest, const char *const *srcs, uint32_t nsrc, rbx_callback cb,
                        void *user, rbx_future **out) {
    if (!c || !dest || (nsrc && !srcs)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(srcs, nsrc, &v));
    std::string d(dest);
    return submit_async(c, [=]() { return hll_merge(c, d, v); }, cb, user, out);
}

// ---- self test of the host-compiled device primitives (CPU tests call this) ------------
// Returns the number of mismatches of mod63 against '%' over `n` pseudo-random pairs.
uint64_t rbx_selftest_mod(uint64_t n, uint64_t seed) {
    uint64_t bad = 0, s = seed;
    auto next = [&]() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t d;
        uint64_t r = next();
        switch (r & 7) {
        case 0: d = 1 + (next() & 0xff); break;
        case 1: d = (1ULL << 32) - (next() & 0xff); break;
        case 2: d = (1ULL << (1 + (next() % 32))); break;
        case 3: d = (1ULL << 31) + (next() & 0xffff) - 0x8000; break;
        default: d = 1 + (next() % (1ULL << 32)); break;
        }
        if (d == 0 || d > (1ULL << 32)) d = 1;
        ModParams p = make_mod_params(d);
        for (int t = 0; t < 16; ++t) {
            uint64_t h = next() & 0x7fffffffffffffffULL;
            if (t == 0) h = 0x7fffffffffffffffULL;
            if (t == 1) h = d - 1;
            if (t == 2) h = d;
            if (mod63(h, p) != (uint32_t)(h % d)) ++bad;
        }
    }
    return bad;
}

// The index sequence every Bloom kernel walks (BloomSeq), on both of its modulus forms.
uint32_t rbx_selftest_bloom_indexes(uint64_t h1, uint64_t h2, uint32_t k, uint64_t size, uint32_t *out) {
    const ModParams mp = make_mod_params(size);
    const ModC mc = mod_compact(mp);
    BloomSeq a(h1, h2), b(h1, h2);
    uint32_t bad = 0;
    for (uint32_t j = 0; j < k; ++j) {
        out[j] = a.next(j, mp);
        bad += b.next(j, mc) != out[j];
    }
    return bad;
}

// HighwayHash128 / MurmurHash64A of the host-compiled device code (CPU cross-check).
void rbx_selftest_hash128(const uint8_t *data, uint64_t len, uint64_t out[2]) {
    HH s;
    hh_reset(s);
    uint64_t i = 0;
    for (; i + 32 <= len; i += 32) {
        uint32_t w[8];
        memcpy(w, data + i, 32);
        hh_packet(s, w);
    }
    uint32_t r = (uint32_t)(len & 31);
    if (r) {
        uint32_t t[8] = {0}, p[8];
        memcpy(t, data + i, r);
        for (int j = (int)r; j < 32; ++j) ((uint8_t *)t)[j] = 0xA5;  // garbage past the tail
        hh_tail_packet(t, r, p);
        hh_remainder_prologue(s, r);
        hh_packet(s, p);
    }
    hh_finalize128(s, out[0], out[1]);
}

// allocations the contexts' DevBuf / PinBuf objects hold in this process (0 once every context is shut down)
int64_t rbx_selftest_live_buffers(void) { return g_live_buffers.load(); }

int rbx_host_alloc(uint64_t bytes, void **out) {
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL out");
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return RBX_OK;
}

int rbx_host_free(void *p) {
    if (p) HIP_TRY(hipHostFree(p));
    return RBX_OK;
}

int rbx_set_staging(rbx_ctx *c, uint64_t bytes) {
    if (!c || bytes < 4096) return fail(RBX_E_ILLEGAL_ARGUMENT, "staging must be >= 4 KiB");
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    if (c->shut) return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    c->dev->stage.staging_bytes = bytes;
    return RBX_OK;
}

int rbx_memory_usage_n(rbx_ctx *c, const rbx_name *names, uint32_t n, uint64_t *bytes) {
    if (!c || !bytes) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(names, n, &v));
    return memory_usage(c, v, bytes);
}

int rbx_bloom_size_in_memory(rbx_ctx *c, const char *name, uint64_t *bytes) {
    if (!c || !name || !bytes) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return memory_usage(c, {std::string(name), config_name(name)}, bytes);
}

// ---- key timeouts (RedissonExpirable, M/RedissonExpirable.java:53-251; keyspace.cpp) ----------
int rbx_pexpire(rbx_ctx *c, const char *const *names, uint32_t n, int64_t when_ms, int absolute, int cond,
                int *result) {
    if (!c || (n && !names)) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, n, &v));
    return ks_pexpire(c->ks, v, when_ms, absolute, cond, result);
}

int rbx_pexpire_n(rbx_ctx *c, const rbx_name *names, uint32_t n, int64_t when_ms, int absolute, int cond,
                  int *result) {
    if (!c) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(names, n, &v));
    return ks_pexpire(c->ks, v, when_ms, absolute, cond, result);
}

int rbx_persist(rbx_ctx *c, const char *const *names, uint32_t n, int *result) {
    if (!c || (n && !names)) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, n, &v));
    return ks_persist(c->ks, v, result);
}

int rbx_pttl(rbx_ctx *c, const char *name, int64_t *out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_pttl(c->ks, name, out);
}

int rbx_pexpiretime(rbx_ctx *c, const char *name, int64_t *out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_pexpiretime(c->ks, name, out);
}

int rbx_bloom_digest_n(rbx_ctx *c, rbx_name name, uint64_t *out) {
    if (!c || (!name.bytes && name.len) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    Entry *e = c->ks.find(name_of(name));
    if (!e) {
        *out = 0;  // a missing key (GET = nil)
        return RBX_OK;
    }
    if (e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    int rc;
    const uint64_t len = read_dev_u64(c, e->bm->d_len, &rc);
    RBX_TRY(rc);
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 4;
    HIP_TRY(hipMemsetAsync(d, 0, 8, c->stream));
    if (len) launch_digest((const uint8_t *)e->bm->d_words, len, d, c->stream);
    HIP_TRY(hipGetLastError());
    const uint64_t v = read_dev_u64(c, d, &rc);
    RBX_TRY(rc);
    *out = v + mix64_host(len ^ 0xD1B54A32D192ED03ULL) + 1;  // never 0 for an existing key
    return RBX_OK;
}

int rbx_bloom_digest(rbx_ctx *c, const char *name, uint64_t *out) {
    if (!name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return rbx_bloom_digest_n(c, rbx_name{(const uint8_t *)name, strlen(name)}, out);
}

// Replica sync of one Bloom filter: dst's {name}:config := src's (all four fields) and dst's
// bitmap string := src's, copied device to device (hipMemcpyPeerAsync: xGMI between the GPUs of
// a node, a plain device copy on one GPU).  The replica's key timeouts are not copied.
int rbx_bloom_copy_to(rbx_ctx *src, rbx_ctx *dst, rbx_name name) {
    if (!src || !dst || (!name.bytes && name.len)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (src == dst) return fail(RBX_E_ILLEGAL_ARGUMENT, "source and destination are the same context");
    std::scoped_lock lk(src->ks.mu, dst->ks.mu);
    const std::string nm = name_of(name);
    RBX_TRY(set_device(src));
    if (dst->shut) return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    BloomConfig cfg;
    RBX_TRY(ks_get_config(src->ks, nm, &cfg));
    RBX_TRY(check_offsets(cfg.size));
    Entry *e = src->ks.find(nm);
    if (e && e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    std::shared_ptr<Bitmap> sb = e ? e->bm : nullptr;
    uint64_t len = 0;
    if (sb) {
        RBX_TRY(quiesce(src));
        int rc;
        len = read_dev_u64(src, sb->d_len, &rc);
        RBX_TRY(rc);
    }
    RBX_ENTER(dst, dst->stream);  // its lock is held already (recursive): the device and the scratch order
    dst->ks.put(config_name(nm), Entry{KType::Config, std::make_shared<BloomConfig>(cfg), nullptr, nullptr});
    dst->ks.generation++;
    if (!sb) {  // the source has no bitmap yet: neither has the replica
        dst->ks.erase(nm);
        return RBX_OK;
    }
    const uint64_t bits = std::max<uint64_t>(size_bits(cfg.size), len * 8);
    std::shared_ptr<Bitmap> b;
    Entry *de = dst->ks.find(nm);
    if (de && de->type == KType::Bitmap && de->bm->cap_bytes >= (bits + 7) / 8) {
        b = de->bm;  // in place: the replica's open handles keep seeing it
        HIP_TRY(hipMemsetAsync(b->d_words, 0, b->cap_bytes, dst->stream));
    } else {
        RBX_TRY(new_bitmap(dst, bits, dst->stream, &b));
    }
    if (len) HIP_TRY(hipMemcpyPeerAsync(b->d_words, dst->device, sb->d_words, src->device, len, dst->stream));
    static thread_local unsigned long long L;
    L = len;
    HIP_TRY(hipMemcpyAsync(b->d_len, &L, 8, hipMemcpyHostToDevice, dst->stream));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    dst->ks.put(nm, Entry{KType::Bitmap, nullptr, b, nullptr});
    dst->ks.generation++;
    return RBX_OK;
}

// Peer access between the GPUs of a node (best effort: copies work without it, staged).
int rbx_enable_peer_access(int device, int peer) {
    if (device == peer) return RBX_OK;
    int can = 0;
    HIP_TRY(hipDeviceCanAccessPeer(&can, device, peer));
    if (!can) return RBX_OK;
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(RBX_E_DEVICE, hipGetErrorString(e));
    (void)hipGetLastError();
    return RBX_OK;
}

// Tuning knobs (process-wide): one lookup in kTuneRows.
int rbx_tune(const char *key, int value) {
    if (!key) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL key");
    for (const TuneRow &r : kTuneRows) {
        if (strcmp(key, r.key) != 0) continue;
        // librbx.so rejects the diagnostics keys: no knob there changes an answer
        if (r.diag && !kDiag) return fail(RBX_E_ILLEGAL_ARGUMENT, std::string(key) + ": diagnostics exist only in librbx_diag.so");
        if (!r.accepts(value)) return fail(RBX_E_ILLEGAL_ARGUMENT, std::string(key) + r.wants());
        r.store(value);
        return RBX_OK;
    }
    return fail(RBX_E_ILLEGAL_ARGUMENT, std::string("unknown tuning key ") + key);
}

// Java BigDecimal.valueOf(d).toPlainString() as stored in the config hash.
int rbx_selftest_plain_string(double d, char *out, int cap) {
    std::string s = java_plain_string(d);
    if (!out || cap <= 0) return (int)s.size();
    snprintf(out, (size_t)cap, "%s", s.c_str());
    return (int)s.size();
}

}  // extern "C"
