/*
 * rbx.h -- C ABI of the MI355X-native batched sketch engine (librbx.so).
 *
 * Drop-in boundary for Redisson's probabilistic-structure hot path.  Every entry
 * point below replaces a reference interface; the citation is given per function.
 * Abbreviation: M/ = /root/reference/redisson/src/main/java/org/redisson/
 *
 * Conventions
 *  - Every function returns int: RBX_OK (0) or a negative error class that mirrors
 *    the exception the reference throws.  rbx_last_error() returns the message
 *    (thread-local; valid until the next call on the same thread).
 *  - The caller owns every host buffer; the library never retains one past return.
 *    Object handles (rbx_bloom, rbx_hll) are library-owned and reference-counted.
 *  - Keys/elements are codec OUTPUT bytes (RedissonObject.encode,
 *    M/RedissonObject.java:319-321).  The engine is codec-agnostic.
 *  - A context owns one GPU.  Calls on one context are serialized (a batch is the
 *    unit of serialization, matching the reference's pipeline order); calls from
 *    several threads are safe.  Handles keep their context's memory alive: closing a
 *    handle after rbx_shutdown is safe, any other call on it returns RBX_E_ILLEGAL_STATE.
 *  - *_dev variants take DEVICE pointers and a hipStream_t (as void*; NULL = the
 *    context's stream), enqueue work and return without synchronizing.  Counts are
 *    accumulated into device-resident unsigned long long words.  Per-call device scratch
 *    of a context is stream-ordered: use one stream per context for *_dev calls (or
 *    synchronize before switching streams).
 */
#ifndef RBX_H
#define RBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBX_ABI_VERSION 1

enum {
    RBX_OK = 0,
    RBX_E_ILLEGAL_ARGUMENT = -1, /* java.lang.IllegalArgumentException             */
    RBX_E_ILLEGAL_STATE = -2,    /* IllegalStateException "Bloom filter is not initialized!" */
    RBX_E_CONFIG_CHANGED = -3,   /* RedisException "Bloom filter config has been changed" */
    RBX_E_ARITHMETIC = -4,       /* ArithmeticException "/ by zero" (empty collection) */
    RBX_E_WRONGTYPE = -5,        /* RedisException WRONGTYPE / INVALIDOBJ            */
    RBX_E_DEVICE = -6,           /* HIP / RCCL runtime failure                       */
    RBX_E_OOM = -7,              /* device or host allocation failure                */
    RBX_E_NO_SUCH_KEY = -8,      /* RedisException "ERR no such key" (RENAME)        */
    RBX_E_REDIS = -9,            /* other RedisException replies, e.g. "ERR bit offset is not an
                                    integer or out of range": a filter with |size| > 2^32 (only from
                                    tryInit with a negative expectedInsertions,
                                    M/RedissonBloomFilter.java:262-277) whose batch reaches an index
                                    (hash % |size|) past the Redis offset limit 2^32 - 1.  As in the
                                    reference's pipelined batch, rbx_bloom_add[_n] has then set every
                                    in-range bit (and created the key only if one was set) and
                                    rbx_bloom_contains[_n] changed nothing; a batch with no such
                                    index gets the exact in-order replies.  Handles (rbx_bloom_open*,
                                    hence the *_dev / multi-tenant / stream calls) and replica
                                    copies of such a filter are refused up front with this code. */
    RBX_E_TIMEOUT = -10          /* rbx_future_wait: the call has not completed in time        */
};

typedef struct rbx_ctx rbx_ctx;
typedef struct rbx_bloom rbx_bloom;
typedef struct rbx_hll rbx_hll;
typedef struct rbx_future rbx_future;
typedef struct rbx_node rbx_node;
/* completion callback of an asynchronous call: rc = the call's return code (runs on the
 * context's executor thread; a JVM binds it as an FFM upcall completing a CompletableFuture) */
typedef void (*rbx_callback)(void *user, int rc);

/* A batch of n encoded keys.  Key i is bytes[offsets[i] .. offsets[i+1]) when
 * offsets != NULL (n+1 entries), else bytes[i*stride .. (i+1)*stride). */
typedef struct rbx_keys {
    const uint8_t *bytes;
    const uint64_t *offsets;
    uint64_t stride;
    uint64_t n;
} rbx_keys;

/* A key name of any bytes (Redis keys are binary-safe; Spring Data passes byte[] keys,
 * redisson-spring-data-32 RedissonConnection.java:2203).  The *_n entry points take these; the
 * others take NUL-terminated names. */
typedef struct rbx_name {
    const uint8_t *bytes;
    uint64_t len;
} rbx_name;

/* The {name}:config hash (M/RedissonBloomFilter.java:285-288). */
typedef struct rbx_bloom_config {
    int64_t size;                /* "size" (bits; Java long: tryInit with a negative
                                    expectedInsertions stores a negative size, :270-276) */
    uint32_t hash_iterations;    /* "hashIterations" (k)                    */
    int64_t expected_insertions; /* "expectedInsertions" (0 if raw-created) */
    double false_probability;    /* "falseProbability"                      */
    char false_probability_str[64]; /* BigDecimal.toPlainString form        */
} rbx_bloom_config;

/* ---- library / context ------------------------------------------------------- */
int rbx_abi_version(void);
const char *rbx_last_error(void);
int rbx_device_count(int *out);
/* Redisson.create(config) -- M/Redisson.java; one context per GPU. */
int rbx_init(int device, rbx_ctx **out);
/* RedissonClient.shutdown() */
int rbx_shutdown(rbx_ctx *ctx);
int rbx_synchronize(rbx_ctx *ctx);
/* The context's hipStream_t, as void*. */
void *rbx_stream(rbx_ctx *ctx);

/* Pinned (page-locked) host memory for key arenas: batches whose bytes live here are
 * uploaded by DMA at full PCIe rate (a JVM wraps it as a MemorySegment). */
int rbx_host_alloc(uint64_t bytes, void **out);
int rbx_host_free(void *p);
/* Host-buffer batches are uploaded in double-buffered chunks of this many key bytes while
 * the previous chunk computes (default 64 MiB). */
int rbx_set_staging(rbx_ctx *ctx, uint64_t bytes);

/* ---- sharding: M/connection/CRC16.java:51-57, M/cluster/ClusterConnectionManager.java:777-792 */
uint16_t rbx_crc16(const uint8_t *bytes, size_t len);
int rbx_calc_slot(const uint8_t *key, size_t len);
/* Slot range -> GPU of one node: slot * n_gpus / 16384. */
int rbx_slot_to_gpu(int slot, int n_gpus);

/* ---- Bloom sizing: RedissonBloomFilter.optimalNumOfBits/HashFunctions :79-88 ---- */
int rbx_bloom_optimal_config(int64_t expected_insertions, double false_probability,
                             int64_t *size_out, uint32_t *k_out);

/* ---- RBloomFilter (by name) -- M/api/RBloomFilter.java:27-113 ---------------------- */
/* tryInit(expectedInsertions, falseProbability)  M/RedissonBloomFilter.java:262-300 */
int rbx_bloom_try_init(rbx_ctx *ctx, const char *name, int64_t expected_insertions,
                       double false_probability, int *created);
/* Engine-level init with a raw (size, k) -- reaches m = 2^32, which tryInit caps at
 * getMaxSize() = 4,294,967,294 (:257-259). */
int rbx_bloom_init_raw(rbx_ctx *ctx, const char *name, uint64_t size, uint32_t k, int *created);
/* readConfig() HGETALL {name}:config  :240-255 (RBX_E_ILLEGAL_STATE if absent) */
int rbx_bloom_read_config(rbx_ctx *ctx, const char *name, rbx_bloom_config *out);
/* add(Collection) :104-137.  size/k are the caller's cached config (size = the Java long's
 * bits; 0 = read the config first, :106-108), checked like addConfigCheck :207-213.
 * out_new (nullable): 1 byte per key, 1 iff the key counts as newly added under the
 * reference's in-order SETBIT semantics. */
int rbx_bloom_add(rbx_ctx *ctx, const char *name, uint64_t size, uint32_t k,
                  const rbx_keys *keys, uint8_t *out_new, uint64_t *out_count);
/* contains(Collection) :153-186.  out_present (nullable): 1 byte per key. */
int rbx_bloom_contains(rbx_ctx *ctx, const char *name, uint64_t size, uint32_t k,
                       const rbx_keys *keys, uint8_t *out_present, uint64_t *out_count);
/* count() :215-227 (BITCOUNT + the host double formula) */
int rbx_bloom_count(rbx_ctx *ctx, const char *name, int64_t *out);
/* the same four with binary names */
int rbx_bloom_try_init_n(rbx_ctx *ctx, rbx_name name, int64_t expected_insertions, double false_probability,
                         int *created);
int rbx_bloom_read_config_n(rbx_ctx *ctx, rbx_name name, rbx_bloom_config *out);
int rbx_bloom_add_n(rbx_ctx *ctx, rbx_name name, uint64_t size, uint32_t k, const rbx_keys *keys,
                    uint8_t *out_new, uint64_t *out_count);
int rbx_bloom_contains_n(rbx_ctx *ctx, rbx_name name, uint64_t size, uint32_t k, const rbx_keys *keys,
                         uint8_t *out_present, uint64_t *out_count);
int rbx_bloom_count_n(rbx_ctx *ctx, rbx_name name, int64_t *out);
/* DEL k1..kn (*deleted = keys removed) and EXISTS k1..kn (*count = existing keys, repeats
 * counted) over keys of any type -- RObject.delete / isExists for any name */
int rbx_del_n(rbx_ctx *ctx, const rbx_name *names, uint32_t n, int *deleted);
/* sizeInMemory (M/RedissonObject.java:124-130): bytes the engine holds for the existing keys --
 * device allocation of a bitmap / HLL, config fields, key names (not Redis' allocator figures).
 * The Bloom form sums the bitmap and {name}:config (M/RedissonBloomFilter.java:234-238). */
int rbx_memory_usage_n(rbx_ctx *ctx, const rbx_name *names, uint32_t n, uint64_t *bytes);
int rbx_bloom_size_in_memory(rbx_ctx *ctx, const char *name, uint64_t *bytes);
int rbx_exists_n(rbx_ctx *ctx, const rbx_name *names, uint32_t n, int *count);
/* BITCOUNT name */
int rbx_bloom_bitcount(rbx_ctx *ctx, const char *name, uint64_t *out);
/* delete() :230-232 -- DEL name {name}:config; *deleted = number of keys removed */
int rbx_bloom_delete(rbx_ctx *ctx, const char *name, int *deleted);
/* isExists() :344-347 -- EXISTS name {name}:config > 0 */
int rbx_bloom_is_exists(rbx_ctx *ctx, const char *name, int *exists);
/* rename :349-364 and renamenx :366-385 */
int rbx_bloom_rename(rbx_ctx *ctx, const char *name, const char *new_name);
int rbx_bloom_renamenx(rbx_ctx *ctx, const char *name, const char *new_name, int *renamed);

/* ---- key timeouts: RExpirable (M/RedissonExpirable.java:53-251) ----------------------------
 * Keys are removed lazily once their timeout passes (Redis semantics); handles follow their name.
 * rbx_pexpire replaces expireAsync / expireAtAsync (:207-239): PEXPIRE (absolute = 0, when_ms
 * relative) or PEXPIREAT (absolute = 1, unix ms) on every key, *result = 1 iff any timeout was
 * set.  cond: 0 none, 1 NX, 2 XX, 3 GT, 4 LT (expireIfNotSet / expireIfSet / expireIfGreater /
 * expireIfLess).  RBloomFilter passes {name, "{name}:config"} (M/RedissonBloomFilter.java:303-310),
 * RHyperLogLog {name}. */
int rbx_pexpire(rbx_ctx *ctx, const char *const *names, uint32_t n, int64_t when_ms, int absolute, int cond,
                int *result);
int rbx_pexpire_n(rbx_ctx *ctx, const rbx_name *names, uint32_t n, int64_t when_ms, int absolute, int cond,
                  int *result);
/* clearExpireAsync (:241-251): PERSIST every key, *result = 1 iff any timeout was removed */
int rbx_persist(rbx_ctx *ctx, const char *const *names, uint32_t n, int *result);
/* remainTimeToLiveAsync (:193-195) = PTTL, getExpireTimeAsync (:203-205) = PEXPIRETIME of one key:
 * -2 when the key does not exist, -1 when it has no timeout */
int rbx_pttl(rbx_ctx *ctx, const char *name, int64_t *out);
int rbx_pexpiretime(rbx_ctx *ctx, const char *name, int64_t *out);
/* GET name: the Redis bitmap string (MSB-first, length = highest SETBIT byte + 1).
 * Writes min(cap, len) bytes; *redis_len = len. */
int rbx_bloom_export(rbx_ctx *ctx, const char *name, uint8_t *out, uint64_t cap, uint64_t *redis_len);
/* SET name <bytes>: replaces the bitmap string (warm start from Redis data). */
int rbx_bloom_import(rbx_ctx *ctx, const char *name, const uint8_t *bytes, uint64_t len);

/* SET name from a DEVICE buffer (device-resident snapshot restore); synchronous. */
int rbx_bloom_import_dev(rbx_ctx *ctx, const char *name, const uint8_t *d_bytes, uint64_t len, void *stream);

/* ---- RBitSet (by binary name) -- M/api/RBitSet.java, impl M/RedissonBitSet.java ---------------
 * The bit set of `name` is the Redis string under that key: the one a Bloom filter of the same
 * name keeps its bits in (createBitSet, M/RedissonBloomFilter.java:203-205), so these calls and the
 * rbx_bloom_* calls see each other's writes.  Bit i is byte i>>3, mask 0x80 >> (i&7); offsets end
 * at 2^32 - 1 (a larger one: RBX_E_REDIS "ERR bit offset is not an integer or out of range").  A
 * write grows the string like SETBIT -- whatever the value written -- and keeps the key's timeout;
 * a missing key reads as the empty string.  A key of another type gives RBX_E_WRONGTYPE.
 * clear() (:492-494) is DEL name: rbx_del_n. */
/* get(bitIndex) = GETBIT  :277-279 */
int rbx_bitset_get(rbx_ctx *ctx, rbx_name name, uint64_t index, int *bit);
/* set(bitIndex, value) / clear(bitIndex) = SETBIT, *old (nullable) = the bit before  :302-305 */
int rbx_bitset_set(rbx_ctx *ctx, rbx_name name, uint64_t index, int value, int *old);
/* set(long[] indexArray, value) = one BITFIELD of `set u1 index value` sub-commands, void  :312-324.
 * BITFIELD parses every sub-command before it runs any: an index past the offset limit fails the
 * call with nothing changed.  n = 0 sends nothing (no key is created). */
int rbx_bitset_set_indexes(rbx_ctx *ctx, rbx_name name, const uint64_t *indexes, uint64_t n, int value);
/* n GETBITs in one call, out[i] = bit indexes[i] (engine extension, like containsEach) */
int rbx_bitset_get_indexes(rbx_ctx *ctx, rbx_name name, const uint64_t *indexes, uint64_t n, uint8_t *out);
/* The same two over DEVICE index arrays, enqueued on `stream` (d_out: device bytes).  Exception to
 * the *_dev convention: each waits once on the stream for the maximum index (the offset check,
 * the string's growth and its new length are host decisions). */
int rbx_bitset_set_indexes_dev(rbx_ctx *ctx, rbx_name name, const uint64_t *d_indexes, uint64_t n, int value,
                               void *stream);
int rbx_bitset_get_indexes_dev(rbx_ctx *ctx, rbx_name name, const uint64_t *d_indexes, uint64_t n, uint8_t *d_out,
                               void *stream);
/* set(fromIndex, toIndex, value) / clear(fromIndex, toIndex): a batch of one SETBIT per index of
 * [from, to), in order  :442-454.  from >= to sends nothing.  to > 2^32 applies [from, 2^32) and
 * then returns RBX_E_REDIS (the pipelined-batch rule of RBX_E_REDIS above). */
int rbx_bitset_set_range(rbx_ctx *ctx, rbx_name name, uint64_t from, uint64_t to, int value);
/* An ordered stream of GETBIT / SETBIT commands over many keys in one call: what a batch queues through
 * RBatch.getBitSet(name) (M/RedissonBatch.java:182-184), executes in submission order
 * (M/command/CommandBatchService.java:115-134,335) and answers in that order (BatchResult.getResponses(),
 * M/api/BatchResult.java:41); Spring Data reaches the same shape with getBit / setBit between openPipeline()
 * and closePipeline() (redisson-spring-data-32 RedissonConnection.java:139-160, :629-636).
 *   Commands  command i is (cmd_key[i], cmd_op[i], cmd_index[i]): an entry of `names`, 0 = GETBIT /
 *             1 = SETBIT index 0 / 2 = SETBIT index 1, and the bit offset.  Two entries of `names` with equal
 *             bytes are the same key.
 *   Result    exactly that of n calls of rbx_bitset_get / rbx_bitset_set in array order: replies[i]
 *             (nullable array) is the bit for a GETBIT and the bit before for a SETBIT, and a GETBIT sees
 *             every earlier SETBIT of its key.  A SETBIT grows the string to (index >> 3) + 1 bytes
 *             whatever it writes, creates a missing key and keeps the key's timeout; a GETBIT creates and
 *             grows nothing (a missing key, or an index past the end, reads 0).
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above: a command whose index is >= 2^32
 *             (RBX_E_REDIS "ERR bit offset is not an integer or out of range") or whose key holds
 *             another type (RBX_E_WRONGTYPE: a {name}:config hash, an HLL) fails alone.  It changes
 *             nothing -- a key whose only SETBITs failed is not created -- and its reply is 0xFF;
 *             every other command takes effect and gets its exact reply.  The call returns the code of the
 *             first failing command in array order, its message in rbx_last_error().
 *   Caller    cmd_key[i] >= nkeys, cmd_op[i] > 2 or a NULL array with n > 0 is RBX_E_ILLEGAL_ARGUMENT with
 *             nothing changed and nothing created.  n = 0 sends nothing.
 * `names` is host memory in both forms.  The _dev form takes device command arrays and enqueues on
 * `stream` (NULL: the context's); like rbx_bitset_set_indexes_dev it is an exception to the *_dev
 * convention: it waits once on the stream, for the batch's summary (the keys to create or grow, the
 * failed commands and the return code are host decisions). */
int rbx_bitset_stream(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                      const uint8_t *cmd_op, const uint64_t *cmd_index, uint64_t n, uint8_t *replies);
int rbx_bitset_stream_dev(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                          const uint8_t *d_cmd_op, const uint64_t *d_cmd_index, uint64_t n, uint8_t *d_replies,
                          void *stream);
/* and / or / xor (:362-388) and not (:462-464) = BITOP op dest src_0 .. src_{nsrc-1} ([redis-7.2]
 * bitops.c bitopCommand): the result is as long as the longest source, a shorter source reads as
 * zero past its end and a missing one is the empty string.  dest may be any of the sources
 * (Redisson passes its own name as the first, :381-388).  *result_len (nullable) = the reply.  A
 * result of length 0 deletes dest; otherwise dest is overwritten and loses its timeout (setKey
 * without KEEPTTL).  NOT takes one source (else RBX_E_REDIS).  A {name}:config hash as dest or
 * source gives RBX_E_WRONGTYPE with dest untouched.  The first of two divergences from Redis (the
 * second is BITFIELD's offset limit, below): an HLL key is a string there and a legal BITOP
 * operand; here it is refused with RBX_E_WRONGTYPE. */
enum { RBX_BITOP_AND = 0, RBX_BITOP_OR = 1, RBX_BITOP_XOR = 2, RBX_BITOP_NOT = 3 };
int rbx_bitset_op(rbx_ctx *ctx, int op, rbx_name dest, const rbx_name *srcs, uint32_t nsrc, uint64_t *result_len);
/* cardinality() = BITCOUNT  :482-484;  size() = STRLEN * 8  :472-474 */
int rbx_bitset_cardinality(rbx_ctx *ctx, rbx_name name, uint64_t *out);
int rbx_bitset_size(rbx_ctx *ctx, rbx_name name, uint64_t *out);
/* length(): the Lua script of lengthAsync  :428-439 -- not java.util.BitSet.length().  It looks at
 * the string's LAST byte only (BITPOS key 1 -1): the highest set bit of that byte + 1.  When that
 * byte is zero, or the key is missing, its loop runs over bits 0 and -1: 1 if bit 0 is set, else
 * the script fails on GETBIT key -1 (RBX_E_REDIS). */
int rbx_bitset_length(rbx_ctx *ctx, rbx_name name, int64_t *out);
/* the same script over a host string (no context) */
int rbx_bitset_length_of(const uint8_t *bytes, uint64_t len, int64_t *out);
/* toByteArray() = GET  :327-334 and the SET of set(BitSet)  :457-459 once its bytes exist: rbx_bloom_export /
 * rbx_bloom_import with a binary name.  set(BitSet) itself, conversion included, is rbx_bitset_set_words below. */
int rbx_bitset_export_n(rbx_ctx *ctx, rbx_name name, uint8_t *out, uint64_t cap, uint64_t *redis_len);
int rbx_bitset_import_n(rbx_ctx *ctx, rbx_name name, const uint8_t *bytes, uint64_t len);
/* asBitSet()  :391-408 and set(BitSet)  :411-420, :457-459 -- the exchange with java.util.BitSet, whose long[]
 * words hold bit j of word w = bit 64 w + j (LSB first) where the string holds bit i in byte i >> 3 under the mask
 * 0x80 >> (i & 7): the conversion reverses the bits of every byte, on the device next to the data.
 *   as_words   asBitSet().toLongArray().  *nwords = BitSet's words in use: the highest set bit / 64 + 1, or 0 for
 *              no set bit, a missing key or an empty string.  min(cap_words, *nwords) words are written (as
 *              rbx_bloom_export does with bytes; `words` may be NULL with cap_words 0).  It reads only.
 *   set_words  set(BitSet.valueOf(words)): the stored string is toByteArrayReverse's, bs.length() / 8 + 1 bytes
 *              with bs.length() = the highest set bit + 1 -- the empty BitSet stores ONE ZERO BYTE, a highest bit of
 *              7 stores two bytes -- and it is stored exactly as rbx_bitset_import_n stores those bytes (the key is
 *              replaced whatever it held, its timeout goes, the allocation covers an existing {name}:config's
 *              |size|).  Trailing zero words are allowed.  A highest set bit >= 2^31 - 1 is
 *              RBX_E_ILLEGAL_ARGUMENT: Java's int length() overflows there and the reference throws.
 * The _dev forms take device arrays and enqueue on `stream`.  as_words_dev does not wait: its kernels take the
 * length from the device length word, and *d_nwords is a device word.  set_words_dev waits once, for the highest
 * set bit.  The host forms without a context (as rbx_bitset_count_of): rbx_bitset_as_words_of is as_words over a
 * host string; rbx_bitset_bytes_of_words writes min(cap, *len) bytes of set_words' string and its length. */
int rbx_bitset_as_words(rbx_ctx *ctx, rbx_name name, uint64_t *words, uint64_t cap_words, uint64_t *nwords);
int rbx_bitset_as_words_dev(rbx_ctx *ctx, rbx_name name, uint64_t *d_words, uint64_t cap_words, uint64_t *d_nwords,
                            void *stream);
int rbx_bitset_set_words(rbx_ctx *ctx, rbx_name name, const uint64_t *words, uint64_t nwords);
int rbx_bitset_set_words_dev(rbx_ctx *ctx, rbx_name name, const uint64_t *d_words, uint64_t nwords, void *stream);
int rbx_bitset_as_words_of(const uint8_t *bytes, uint64_t len, uint64_t *words, uint64_t cap_words, uint64_t *nwords);
int rbx_bitset_bytes_of_words(const uint64_t *words, uint64_t nwords, uint8_t *out, uint64_t cap, uint64_t *len);
/* ENGINE EXTENSION (no RBitSet method; the inverse of rbx_bitset_set_indexes): the positions of the set bits.
 *   Interval  nargs 0: the whole string.  nargs 2: the bit interval of BITCOUNT key start end unit, normalised
 *             exactly as rbx_bitset_count_range does, the "start < 0 && end < 0 && start > end" pre-check included.
 *   total     *total = the ones of the interval: what rbx_bitset_count_range (rbx_bitset_cardinality for nargs 0)
 *             answers.  A missing key and an empty string give 0.
 *   out       the absolute bit positions of the ones of rank skip .. min(total, skip + cap) - 1, ascending, as
 *             uint64_t like rbx_bitset_set_indexes' indexes; *written = their number.  A cap smaller than what is
 *             left is pagination, not an error; cap = 0 with a NULL out is a legal "count only" call.
 *   Errors    a key of another type (an HLL key too) is RBX_E_WRONGTYPE; an unknown unit, nargs other than 0 or 2
 *             and a NULL out with cap > 0 are RBX_E_ILLEGAL_ARGUMENT.  Nothing is created, grown or touched,
 *             timeouts included.
 *   Cost      one block directory over the string per call (4 KiB blocks, living for the call only), then only the
 *             blocks that hold a rank of the page are read again: a page costs the directory plus the page.
 * The _dev form writes d_counts[0] = written, d_counts[1] = total and waits once on `stream`, for the string's
 * length.  rbx_bitset_members_of is the same over a host string without a context (as rbx_bitset_count_of): the
 * command's skip is the first rank and min(limit, cap) the page. */
typedef struct {
    int64_t start, end;   /* BITCOUNT's arguments; ignored for nargs 0 */
    uint64_t skip, limit; /* the ones of rank skip .. skip + limit - 1; limit UINT64_MAX = all */
    uint8_t nargs, unit;  /* 0 or 2; RBX_RANGE_BYTE / RBX_RANGE_BIT */
    uint8_t pad[6];
} rbx_members_cmd; /* 40 bytes */
int rbx_bitset_members(rbx_ctx *ctx, rbx_name name, int nargs, int64_t start, int64_t end, int unit, uint64_t skip,
                       uint64_t cap, uint64_t *out, uint64_t *written, uint64_t *total);
int rbx_bitset_members_dev(rbx_ctx *ctx, rbx_name name, int nargs, int64_t start, int64_t end, int unit, uint64_t skip,
                           uint64_t cap, uint64_t *d_out, uint64_t *d_counts, void *stream);
int rbx_bitset_members_of(const uint8_t *bytes, uint64_t len, int missing, const rbx_members_cmd *cmd, uint64_t cap,
                          uint64_t *out, uint64_t *written, uint64_t *total);
/* ENGINE EXTENSION: the members of many keys in one call (the per-entity workload of rbx_bitset_range_stream: every
 * user's active days).  Command i runs on names[cmd_key[i]] and yields the ones of rank skip .. skip + limit - 1 of its
 * interval (limit UINT64_MAX = all).
 *   off      n + 1 words, the exclusive prefix sums of the commands' yields: always written in full and exact, whatever
 *            cap is.  *total = off[n].
 *   out      the first min(total, cap) positions of the concatenation; command i's slice is out[off[i] .. off[i + 1]).
 *            What lies past min(total, cap) stays untouched.  The caller compares total with cap and asks again if it
 *            was short; cap = 0 (out may be NULL) only counts.
 *   status   (nullable) status[i] = 0, or 0xFF for a command that fails alone: its key holds another type
 *            (RBX_E_WRONGTYPE; an HLL key and a {name}:config hash too).  Such a command yields nothing, the others
 *            run, and the call returns the code -- the rule of rbx_bitset_range_stream.
 *   Errors   the caller's own are RBX_E_ILLEGAL_ARGUMENT with the outputs unspecified: a key id not below nkeys, an
 *            unknown unit, nargs other than 0 or 2, NULL arrays with n > 0, a NULL out with cap > 0.  n = 0 sends
 *            nothing (off[0] = 0).  Two names with equal bytes are one key.  Nothing is created, grown or touched.
 *   Paths    two passes around one scan, in the two tiers of rbx_bitset_range_stream: a group of lanes counts and
 *            expands an interval of at most "members_short_max" bytes itself; a longer one is cut into tiles of
 *            "members_tile" bytes that the whole device counts and expands (rbx_tune; every setting is exact).
 * The _dev form takes device arrays (off[n] is the total) and waits once per chunk of "members_chunk" commands on
 * `stream`; the host form runs the counting pass twice, once to size the output.  Scope as rbx_bitset_range_stream:
 * no handle form; the node router and the Java shim do not carry it. */
int rbx_bitset_members_stream(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                              const rbx_members_cmd *cmds, uint64_t n, uint64_t cap, uint64_t *off, uint64_t *out,
                              uint8_t *status, uint64_t *total);
int rbx_bitset_members_stream_dev(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                                  const rbx_members_cmd *d_cmds, uint64_t n, uint64_t cap, uint64_t *d_off,
                                  uint64_t *d_out, uint8_t *d_status, void *stream);
/* rename(newName) = RENAME name newName, `name` alone (M/RedissonObject.java:151-153) */
int rbx_bitset_rename(rbx_ctx *ctx, rbx_name name, rbx_name new_name);
/* getSigned / setSigned / incrementAndGetSigned, the Unsigned three, and the Byte / Short / Integer /
 * Long forms (i8 / i16 / i32 / i64) -- M/RedissonBitSet.java:71-254: each is one
 * BITFIELD name GET|SET|INCRBY <i|u><size> <offset> [value] with the default OVERFLOW WRAP
 * ([redis-7.2] bitops.c bitfieldGeneric).  OVERFLOW SAT / FAIL and lists of mixed sub-commands:
 * rbx_bitset_fields_ov, rbx_bitset_bitfield and rbx_bitset_field_rule, after these entries.
 *   Layout  the field is `size` bits from bit `offset`, the bit at `offset` its most significant;
 *           `offset` is a plain bit offset, fields need not be aligned (an i64 at offset 2 covers 9 bytes).
 *   Types   is_signed: sizes 1..64, else 1..63.  A larger size is RBX_E_ILLEGAL_ARGUMENT ("Size can't
 *           be greater than 64 bits" / "... 63 bits", Redisson's own checks :72-73, :99-100); size < 1
 *           reaches Redis and is RBX_E_REDIS ("ERR Invalid bitfield type...").
 *   GET     bits at or past the string's end, and a missing key, read as zero; nothing is created
 *           or grown; the reply is sign-extended for i, zero-extended for u.
 *   SET     the reply is the old value; the field becomes value mod 2^size.
 *   INCRBY  the field becomes (old + value) mod 2^size -- signed fields wrap in two's complement, a
 *           negative increment on an unsigned field wraps too; the reply is the new value.
 *   Growth  SET and INCRBY (even by 0) create a missing key and grow the string to
 *           ((offset + size - 1) >> 3) + 1 bytes, in place when the allocation suffices; the
 *           key's timeout stays.
 *   Limit   offset >= 2^32 is RBX_E_REDIS "ERR bit offset is not an integer or out of range".
 *           DIVERGENCE (the second, beside BITOP on an HLL key above): so is offset + size > 2^32.
 *           Redis checks the start offset only; the engine's bitmaps end at 2^32 bits.
 *   Batch   rbx_bitset_fields is one BITFIELD with n sub-commands of one operation and type.  Every
 *           sub-command is checked before any runs (an illegal offset fails the call with nothing
 *           changed or created); then they take effect in array order, exactly as n single calls,
 *           and replies[i] is what single call i would have returned.  n = 0 sends nothing.
 *           `values` is ignored for GET (may be NULL); `replies` may be NULL for SET and INCRBY.
 *           rbx_bitset_set_indexes(idx, v) and a SET of unsigned size-1 fields at idx leave the
 *           same string.
 *   Paths   GET: one lane per field.  SET / INCRBY with every offset a multiple of size (fields then
 *           equal or disjoint): INCRBY without replies and size a divisor of 64 is one atomic
 *           compare-and-swap loop per element; every other case sorts (slot, position) by slot and
 *           gives each slot one lane that walks its sub-commands in order.  Any other SET / INCRBY
 *           batch runs on one lane, serially: partly overlapping fields make the order total.
 * The _dev form takes device arrays and enqueues on `stream`; like rbx_bitset_set_indexes_dev it
 * waits once on the stream, for the batch's check result (the largest offset, and whether every
 * offset is aligned). */
enum { RBX_FIELD_GET = 0, RBX_FIELD_SET = 1, RBX_FIELD_INCRBY = 2 };
int rbx_bitset_field(rbx_ctx *ctx, rbx_name name, int op, int is_signed, int size, uint64_t offset, int64_t value,
                     int64_t *reply);
int rbx_bitset_fields(rbx_ctx *ctx, rbx_name name, int op, int is_signed, int size, const uint64_t *offsets,
                      const int64_t *values, uint64_t n, int64_t *replies);
int rbx_bitset_fields_dev(rbx_ctx *ctx, rbx_name name, int op, int is_signed, int size, const uint64_t *d_offsets,
                          const int64_t *d_values, uint64_t n, int64_t *d_replies, void *stream);
/* GET over a host string, no context (as rbx_bitset_length_of) */
int rbx_bitset_field_of(const uint8_t *bytes, uint64_t len, int is_signed, int size, uint64_t offset, int64_t *out);
/* BITFIELD's OVERFLOW WRAP | SAT | FAIL, and the one bit command of Spring Data's RedissonConnection that the
 * entries above cannot express: bitField(key, subCommands) S:2241-2291 (S/ as below), one BITFIELD whose
 * sub-commands differ in operation, type and overflow mode.  Restated from [redis-7.2] bitops.c bitfieldGeneric /
 * checkSignedBitfieldOverflow / checkUnsignedBitfieldOverflow; parity is unpinned, as for the HLL strings.
 *   Range   a type <i|u><size> holds [lo, hi]: [0, 2^size - 1] unsigned, [-2^(size-1), 2^(size-1) - 1] signed.
 *   INCRBY  t = old + value, exactly.  In range: the field and the reply are t, in every mode.  Else WRAP keeps
 *           t mod 2^size (the entries above); SAT makes the field hi when t > hi and lo when t < lo, and replies
 *           that; FAIL writes nothing and the reply is nil.
 *   SET     t = value for a signed type; for an unsigned type t = value as an unsigned 64-bit number, so a
 *           negative value overflows UPWARDS (SAT stores hi).  In range the field becomes t; else as INCRBY.  The
 *           reply is the old value, or nil under FAIL on overflow.
 *   GET     ignores the mode.
 *   nil     n bytes; nil[i] = 1: reply i is nil, the field is untouched and replies[i] = 0.  Required
 *           (RBX_E_ILLEGAL_ARGUMENT) when a sub-command runs under FAIL and `replies` is given; otherwise
 *           nullable, and zero-filled when given.
 *   Growth  the string is sized before the first sub-command runs, for every SET and INCRBY, those that then
 *           fail included: INCRBY u8 0 300 under FAIL on a missing key leaves the one-byte string 00 and nil.
 *           GETs grow nothing.
 *   Checks  every sub-command's mode, type and offset is checked before any runs; a bad one fails the call with
 *           nothing changed or created.  An unknown mode is RBX_E_ILLEGAL_ARGUMENT; the offset limit is the one
 *           above (offset + size > 2^32 is RBX_E_REDIS); a key of another type is RBX_E_WRONGTYPE.
 * rbx_bitset_fields_ov / _dev are rbx_bitset_fields / _dev under one mode; with RBX_OVERFLOW_WRAP they answer
 * byte for byte as those (same type checks: Redisson's 63 / 64 limits, then Redis's).
 *   Paths   aligned SAT INCRBY without replies, size a divisor of 64, every increment of one sign (>= 0 or
 *           <= 0): one compare-and-swap loop per element with the sum clamped in the loop -- saturating sums
 *           commute under that condition and under no weaker one; an element whose field already sits at the
 *           bound issues no atomic.  Every other aligned SAT / FAIL batch: the grouped path, each slot's lane
 *           applying the rule in array order.  Unaligned: one lane, serially.  rbx_tune "bitfield_sat_atomic"
 *           0 never takes the atomic path; every setting answers the same.  The _dev form still waits once,
 *           for the check result (now also: whether increments of both signs occur).
 * rbx_bitset_bitfield takes a host array of sub-commands, each with the mode it runs under (Redis's
 * OVERFLOW governs the sub-commands that follow it; the caller resolves that).  Types here get Redis's check
 * only, as S:2241-2291 makes none: u64, i65 and size 0 are RBX_E_REDIS "ERR Invalid bitfield type...".
 * `replies` is required when a GET is present.  Sub-commands that all share operation, type and mode run as
 * rbx_bitset_fields_ov; any other list runs on one lane in array order (fields of different sizes may partly
 * overlap, so the order is total).  n = 0 sends nothing.  There is no _dev form.
 * rbx_bitset_field_rule is the rule itself on one value, no context (as rbx_bitset_field_of): old must lie in
 * the type's range; *now = the field after, *reply = the reply (0 when *nil = 1). */
enum { RBX_OVERFLOW_WRAP = 0, RBX_OVERFLOW_SAT = 1, RBX_OVERFLOW_FAIL = 2 };
int rbx_bitset_fields_ov(rbx_ctx *ctx, rbx_name name, int op, int is_signed, int size, int overflow,
                         const uint64_t *offsets, const int64_t *values, uint64_t n, int64_t *replies, uint8_t *nil);
int rbx_bitset_fields_ov_dev(rbx_ctx *ctx, rbx_name name, int op, int is_signed, int size, int overflow,
                             const uint64_t *d_offsets, const int64_t *d_values, uint64_t n, int64_t *d_replies,
                             uint8_t *d_nil, void *stream);
typedef struct {
    uint64_t offset; /* a plain bit offset ("#N" is N * size, resolved by the caller) */
    int64_t value;   /* SET's value, INCRBY's increment; ignored for GET */
    uint8_t op, is_signed, size, overflow; /* RBX_FIELD_*, 0 / 1, bits, RBX_OVERFLOW_* */
    uint8_t pad[4];
} rbx_field_cmd; /* 24 bytes */
int rbx_bitset_bitfield(rbx_ctx *ctx, rbx_name name, const rbx_field_cmd *cmds, uint64_t n, int64_t *replies,
                        uint8_t *nil);
int rbx_bitset_field_rule(int op, int is_signed, int size, int overflow, int64_t old, int64_t value, int64_t *now,
                          int64_t *reply, int *nil);
/* An ordered stream of single-sub-command BITFIELDs over many keys in one call: what a batch queues through the
 * typed-field methods of RBatch.getBitSet(name) (M/api/RBitSetAsync.java:36-206: get / set / incrementAndGet x
 * Signed, Unsigned, Byte, Short, Integer, Long) and what a Spring Data pipeline of one-sub-command bitField
 * calls sends -- a few packed counters per user, updated for many users at once.  rbx_bitset_stream's shape
 * with rbx_bitset_bitfield's commands.
 *   Commands  command i is BITFIELD names[cmd_key[i]] [OVERFLOW m] GET|SET|INCRBY <i|u><size> <offset> [value],
 *             written as cmds[i] (`pad` is ignored).  Two entries of `names` with equal bytes are the same key.
 *   Result    exactly that of n calls of rbx_bitset_bitfield(ctx, name, &cmds[i], 1, ...) in array order:
 *             replies[i] (nullable array) is what call i returns, and a command sees every earlier write of
 *             its key.  A SET / INCRBY grows the string to ((offset + size - 1) >> 3) + 1 bytes, also when it
 *             ends nil under FAIL, creates a missing key, works in place when the allocation suffices and
 *             keeps the key's timeout; a GET creates and grows nothing.
 *   status    (nullable array) status[i] = 0: the reply is valid; 1: nil (OVERFLOW FAIL), the field is
 *             untouched and replies[i] = 0; 0xFF: the command failed alone, replies[i] = 0.  Required
 *             (RBX_E_ILLEGAL_ARGUMENT) when `replies` is given and a SET / INCRBY that runs is under FAIL --
 *             rbx_bitset_fields_ov's rule for `nil`.
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above.  A command fails alone on Redis's type check
 *             (u64, i65, size 0: RBX_E_REDIS "ERR Invalid bitfield type..."), on the offset limit (offset >=
 *             2^32 or offset + size > 2^32: RBX_E_REDIS "ERR bit offset..."), or on a key of another type
 *             (RBX_E_WRONGTYPE), looked at in this order, which is the single call's.  It changes nothing -- a
 *             key whose only writes failed is not created -- and every other command takes effect with its
 *             exact reply.  The call returns the code of the first failing command in array order, its
 *             message in rbx_last_error().
 *   Caller    cmd_key[i] >= nkeys, an op or overflow mode above 2, is_signed above 1, or a NULL array with
 *             n > 0 is RBX_E_ILLEGAL_ARGUMENT with nothing changed and nothing created.  n = 0 sends nothing.
 *   Paths     one summary pass, one wait, then: a batch without SET / INCRBY is one gather; INCRBYs under WRAP
 *             of one size dividing 64, each at a multiple of it, replies not asked for, are one compare-and-
 *             swap loop per command (not so for mixed sizes: a u8 inside a u16 does not commute with it); any
 *             other batch of at most fieldstream_serial_max commands runs on one lane; a longer one is sorted
 *             by (key, aligned 64-bit word) when every field lies inside one such word -- every mix of the
 *             Byte / Short / Integer / Long methods at multiples of their sizes does -- with one lane per word,
 *             and by key otherwise, one lane per key.  One cell repeated n times runs on one lane: not
 *             bounded.  rbx_tune "fieldstream_path" forces a path; every setting answers the same.
 * `names` is host memory in both forms.  The _dev form takes device arrays and enqueues on `stream` (NULL: the
 * context's); like rbx_bitset_stream_dev it waits once on the stream, for the batch's summary. */
int rbx_bitset_field_stream(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                            const rbx_field_cmd *cmds, uint64_t n, int64_t *replies, uint8_t *status);
int rbx_bitset_field_stream_dev(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                                const rbx_field_cmd *d_cmds, uint64_t n, int64_t *d_replies, uint8_t *d_status,
                                void *stream);
/* BITCOUNT key start end [BYTE|BIT] and BITPOS key bit [start [end [BYTE|BIT]]] -- the two bit commands that
 * Spring Data's RedissonConnection (S/ = redisson-spring-data/redisson-spring-data-31/src/main/java/org/
 * redisson/spring/data/connection/RedissonConnection.java) sends beside the ones above: bitCount(key, begin,
 * end) S:638-646 and bitPos(key, bit, range) S:2337-2359 (getBit / setBit S:628-636, bitOp S:650-661 and
 * strLen S:663-666 are rbx_bitset_get / _set / _op / _size).  RBitSet itself has neither.  Restated from
 * [redis-7.2] bitops.c bitcountCommand / bitposCommand; parity is unpinned, as for the HLL strings.
 *   Range   start and end are signed; the unit is RBX_RANGE_BYTE or RBX_RANGE_BIT and T = the string's
 *           length in that unit.  A negative start or end counts from the end (+= T); then start is clamped to
 *           >= 0 and end to [0, T - 1]; start > end is the empty range.  Both ends are inclusive.
 *   COUNT   the ones of the range; 0 for an empty range and a missing key.  start < 0 && end < 0 && start >
 *           end is 0 before anything is normalised (-10 -20 on 3 bytes would otherwise count byte 0).
 *   POS     the first position of the range whose bit equals `bit`, as an absolute bit offset.  nargs says
 *           how much was given: 0 = BITPOS key bit, 1 = + start, 2 = + start end [unit]; the default start
 *           is 0, the default end the last byte.  An empty range is -1 (every query on an existing empty
 *           string); there is no pre-check (1 -10 -20 on 3 bytes searches byte 0).  Nothing found: -1 for
 *           bit 1 and for bit 0 with an end given, else 8 * length (the string counts as zero-padded on the
 *           right).  A missing key is -1 for bit 1 and 0 for bit 0.  A bit other than 0 / 1 is RBX_E_REDIS
 *           "ERR The bit argument must be 1 or 0."; RBX_RANGE_BIT with nargs < 2 is RBX_E_REDIS "ERR
 *           syntax error" (a unit needs an end).
 *   Errors  an unknown unit or nargs is RBX_E_ILLEGAL_ARGUMENT.  A key of another type is RBX_E_WRONGTYPE, an
 *           HLL key included (the divergence noted at rbx_bitset_op).  Neither command creates, grows or
 *           touches a key or its timeout.
 *   Batch   rbx_bitset_count_ranges / _pos_ranges are n commands on one key in one call (engine extension,
 *           like rbx_bitset_get_indexes): out[i] is what single call i returns.  pos takes one `bit` per batch;
 *           ends == NULL makes every query "bit start" (RBX_RANGE_BYTE only).  n = 0 sends nothing.
 *   Paths   one command: a grid-wide masked count, or a search over ascending chunks that stops at the first
 *           hit.  A batch: one wave per query, which walks its range or -- when the ranges together hold more
 *           bytes than the string plus 8 KiB per query, or one exceeds rbx_tune "bitrange_chain_max" -- reads
 *           whole 4 KiB blocks from a prefix-sum directory built for the call.  Every path answers the same.
 * The _dev forms take device arrays and enqueue on `stream`; like rbx_bitset_get_indexes_dev they wait once on
 * the stream, for the length word and the batch's work summary (the bytes its ranges cover, and the longest). */
enum { RBX_RANGE_BYTE = 0, RBX_RANGE_BIT = 1 };
int rbx_bitset_count_range(rbx_ctx *ctx, rbx_name name, int64_t start, int64_t end, int unit, uint64_t *out);
int rbx_bitset_pos(rbx_ctx *ctx, rbx_name name, int bit, int nargs, int64_t start, int64_t end, int unit, int64_t *out);
int rbx_bitset_count_ranges(rbx_ctx *ctx, rbx_name name, const int64_t *starts, const int64_t *ends, uint64_t n,
                            int unit, uint64_t *out);
int rbx_bitset_pos_ranges(rbx_ctx *ctx, rbx_name name, int bit, const int64_t *starts, const int64_t *ends, uint64_t n,
                          int unit, int64_t *out);
int rbx_bitset_count_ranges_dev(rbx_ctx *ctx, rbx_name name, const int64_t *d_starts, const int64_t *d_ends, uint64_t n,
                                int unit, uint64_t *d_out, void *stream);
int rbx_bitset_pos_ranges_dev(rbx_ctx *ctx, rbx_name name, int bit, const int64_t *d_starts, const int64_t *d_ends,
                              uint64_t n, int unit, int64_t *d_out, void *stream);
/* the same rules over a host string, no context (as rbx_bitset_field_of); missing != 0 (with len == 0) = a
 * missing key */
int rbx_bitset_count_of(const uint8_t *bytes, uint64_t len, int missing, int64_t start, int64_t end, int unit,
                        uint64_t *out);
int rbx_bitset_pos_of(const uint8_t *bytes, uint64_t len, int missing, int bit, int nargs, int64_t start, int64_t end,
                      int unit, int64_t *out);
/* Many BITOPs, and many BITCOUNTs of a combination, in one ordered call: what RBitSet.and / or / xor / not and
 * cardinality send one command at a time (M/RedissonBitSet.java:362-388, :462-464, :482-484), what a batch queues
 * through RBatch.getBitSet(name).andAsync / orAsync / xorAsync / notAsync / cardinalityAsync
 * (M/RedissonBatch.java:182-184), and Spring Data's bitOp (S:650-661) / bitCount(key) (S:638-641) between
 * openPipeline() and closePipeline(): the combinations bitmaps are kept for (users active on day i AND day j for
 * every pair of days, 24 hourly bitmaps ORed into each daily one, BITCOUNT of each of 10,000 feature bitmaps).
 *   Commands  group g is BITOP grp_op[g] names[grp_dest[g]] <names[grp_key[grp_off[g] .. grp_off[g + 1])]>
 *             (grp_off has ngroups + 1 entries and ascends from 0; at least one source).  With grp_dest[g] =
 *             RBX_BITGROUP_NO_DEST the combination is computed and counted but stored nowhere: a one-source OR
 *             is BITCOUNT of that key, a two-source AND the size of an intersection with no temporary key.  Two
 *             entries of `names` with equal bytes are one key.
 *   Result    exactly that of ngroups single calls in array order.  lens[g] is what rbx_bitset_op puts in
 *             *result_len, the longest source's length; counts[g] is the number of one bits of the result -- for
 *             a group with a destination what rbx_bitset_cardinality(dest) answers right after it.  lens, counts
 *             and status are nullable.  Everything rbx_bitset_op does to dest holds per group: it is created if
 *             missing, overwritten over max(result, previous length) with the bytes past its length left zero,
 *             deleted by a result of length 0, loses its timeout otherwise, and never shrinks below the |size|
 *             of an existing {name}:config.  dest may be among its own sources.  Later groups see earlier ones:
 *             a destination may be a later group's source or its destination again.  Groups without a
 *             destination change nothing.
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above: a group that names a key of another type (an HLL, a
 *             {name}:config hash) as destination or source fails alone, and so does RBX_BITOP_NOT with other
 *             than one source.  status[g] is 0xFF, lens[g] = counts[g] = 0, and it changes and creates nothing.
 *             Every other group runs (status 0) with its exact result.  The call returns the code of the first
 *             failing group in array order with its message in rbx_last_error(): RBX_E_REDIS with rbx_bitset_op's
 *             BITOP NOT message (checked first, as there), else RBX_E_WRONGTYPE.
 *   Caller    an op above RBX_BITOP_NOT, a group without a source, an entry >= nkeys, a destination >= nkeys
 *             other than RBX_BITGROUP_NO_DEST, offsets that do not ascend from 0, or a NULL grp_op / grp_dest /
 *             grp_off / grp_key with ngroups > 0 is RBX_E_ILLEGAL_ARGUMENT with nothing changed and nothing
 *             created.  ngroups = 0 sends nothing.  A call takes fewer than 2^31 groups and 2^32 entries.
 *   Cost      each distinct name is looked up once; the length words of all existing keys come back through one
 *             gather launch, one copy and one wait.  From there the host carries every length through the
 *             groups itself and splits them into phases -- a group closes the phase before it when its
 *             destination is a destination or a source of an earlier group of the phase, or one of its sources
 *             is such a destination -- and runs each phase as one table upload and one launch, a segmented sweep
 *             in tiles of rbx_tune "bitgroups_tile" bytes.  The counts come back in one copy behind the call's
 *             second and last wait.  Growing an EXISTING destination past its allocation costs one more wait
 *             each (the old bytes are copied over before the block is freed).  A BITCOUNT of a key that an
 *             earlier group of the same phase wrote is answered from that group's count and reaches no device:
 *             `BITOP AND t_i a b; BITCOUNT t_i` over distinct t_i is one phase, over one t a phase per pair.
 *             Failed groups, and groups whose sources are all missing or empty, are answered on the host
 *             (DESIGN 11.9).
 *   Scope     no handle form, no _dev form; the node router and the Java shim do not carry this call.  Ranged
 *             BITCOUNT is rbx_bitset_count_ranges' on one key and rbx_bitset_range_stream's over many.
 * All arrays are host memory: the host must know the keys to create the destinations. */
#define RBX_BITGROUP_NO_DEST 0xFFFFFFFFu
int rbx_bitset_op_groups(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint8_t *grp_op,
                         const uint32_t *grp_dest, const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups,
                         uint64_t *lens, uint64_t *counts, uint8_t *status);
/* The read queries over many keys in one call: ranged and whole-string BITCOUNT, BITPOS, STRLEN and
 * RBitSet.length()'s script, one command per entry, each on its own key -- the per-entity bitmap workload (one
 * short string per user, "active days in the last 30" = BITCOUNT user:i -30 -1 BIT for every user at once), what
 * RBatch.getBitSet(name).sizeAsync / lengthAsync / bitCountAsync / bitPosAsync queue and Spring Data's
 * bitCount(key, begin, end) / bitPos / strLen send between openPipeline() and closePipeline().
 *   Commands  command i runs on names[cmd_key[i]].  RBX_RANGE_COUNT with nargs 0 is BITCOUNT key
 *             (rbx_bitset_cardinality), with nargs 2 BITCOUNT key start end unit (rbx_bitset_count_range);
 *             RBX_RANGE_POS is rbx_bitset_pos(bit, nargs, start, end, unit); RBX_RANGE_STRLEN is the string's
 *             length in bytes (rbx_bitset_size is 8 times that); RBX_RANGE_LENGTH is rbx_bitset_length, the script
 *             of RBitSet.length(), which looks at the first and the last byte only.  start / end / bit / unit are
 *             ignored where the command or nargs does not use them.  Two entries of `names` with equal bytes are
 *             one key.
 *   Result    exactly that of n single calls: replies[i] is what call i returns, status[i] is 0 for a command that
 *             ran and 0xFF, with replies[i] = 0, for one that failed alone.  replies and status are nullable.  The
 *             commands only read: nothing is created, grown or touched, key timeouts included, and the order
 *             between commands is immaterial.  A missing key answers as the single calls do: COUNT 0, POS -1 for
 *             bit 1 and 0 for bit 0, STRLEN 0, LENGTH what rbx_bitset_length gives (the script fails).
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above: a command fails alone and every other command gets
 *             its exact reply.  A POS command fails when its bit is not 0 / 1 (RBX_E_REDIS "ERR The bit argument
 *             must be 1 or 0.") or its unit is RBX_RANGE_BIT with nargs < 2 (RBX_E_REDIS "ERR syntax error"); any
 *             command fails when its key holds another type (RBX_E_WRONGTYPE, HLL keys included) -- looked at in
 *             that order, as the single calls do; a LENGTH command fails when the script fails (RBX_E_REDIS, as
 *             rbx_bitset_length reports it), the one failure that depends on data.  The call returns the code of
 *             the first failing command in array order with its message in rbx_last_error().
 *   Caller    cmd_key[i] >= nkeys, an op above RBX_RANGE_LENGTH, a unit above RBX_RANGE_BIT, nargs above 2,
 *             RBX_RANGE_COUNT with nargs 1, or a NULL names / cmd_key / cmds with n > 0 is
 *             RBX_E_ILLEGAL_ARGUMENT; replies and status are then unspecified.  n = 0 sends nothing.
 *   Cost      each distinct name is looked up once.  One kernel gives every command a group of rbx_tune
 *             "rangestream_lanes" lanes, which answers it when its interval covers at most "rangestream_short_max"
 *             bytes; longer intervals are cut into tiles of "rangestream_tile" bytes that the whole device sweeps
 *             in a second launch, so no lane group walks a long string alone.  The _dev form waits once on the
 *             stream, for the call's summary (the caller's errors, the first failures, the number of long
 *             commands); the host form uploads the commands, makes at most two waits and copies replies and
 *             status back.  More than "rangestream_chunk" commands run as consecutive chunks, each with its own
 *             summary and wait.
 *   Scope     no handle form; the node router and the Java shim do not carry this call.
 * `names` is host memory in both forms; the _dev form takes device arrays and enqueues on `stream`. */
enum { RBX_RANGE_COUNT = 0, RBX_RANGE_POS = 1, RBX_RANGE_STRLEN = 2, RBX_RANGE_LENGTH = 3 };
typedef struct {
    int64_t start, end;           /* as rbx_bitset_count_range / rbx_bitset_pos; ignored where nargs says so */
    uint8_t op, bit, nargs, unit; /* RBX_RANGE_*, 0 / 1 (POS), 0 / 1 / 2, RBX_RANGE_BYTE / _BIT */
    uint8_t pad[4];
} rbx_range_cmd; /* 24 bytes */
int rbx_bitset_range_stream(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                            const rbx_range_cmd *cmds, uint64_t n, int64_t *replies, uint8_t *status);
int rbx_bitset_range_stream_dev(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                                const rbx_range_cmd *d_cmds, uint64_t n, int64_t *d_replies, uint8_t *d_status,
                                void *stream);
/* one command over a host string, no context (as rbx_bitset_count_of / _pos_of / _length_of); missing != 0 = a
 * missing key.  Returns what the single call returns, *reply = 0 when it fails. */
int rbx_bitset_range_of(const uint8_t *bytes, uint64_t len, int missing, const rbx_range_cmd *cmd, int64_t *reply);

/* ---- Redis string commands on the same keys -- S/RedissonConnection.java:487-627, M/RedissonBinaryStream.java -----
 * The byte-level commands on the strings the RBitSet section's calls reach by bits ([redis-7.2, external] t_string.c,
 * restated in DESIGN 11.12).  A string has at most 2^29 bytes (proto-max-bulk-len, and the engine's 2^32-bit cap).
 * A key of another type -- a {name}:config hash, an HLL -- gives RBX_E_WRONGTYPE; a write keeps the key's timeout,
 * and what lies between a string's length and its allocation's end stays zero behind every call.
 *   getrange  GETRANGE key start end  (getRange :617, RBinaryStream's reads :128, :145).  Negative start / end count
 *             from the end, both are clamped to the string and the reply is the bytes [start, end]; "start < 0 &&
 *             end < 0 && start > end" and a missing key reply empty bytes (never nil).  *len = the reply's length,
 *             min(cap, *len) bytes are written (as rbx_bloom_export; out may be NULL with cap 0).
 *   setrange  SETRANGE key offset value  (setRange :624, the channel's write :158).  offset < 0: RBX_E_REDIS "ERR
 *             offset is out of range", before the key is looked at.  n = 0: *new_len = the current length and nothing
 *             is created.  offset + n > 2^29: RBX_E_REDIS "ERR string exceeds maximum allowed size
 *             (proto-max-bulk-len)".  Otherwise the string becomes max(length, offset + n) bytes, zeros between the
 *             old length and offset, a missing key is created, and *new_len = the new length.
 *   append    APPEND key value  (append :610, the OutputStream's write :62).  A missing key is created holding the
 *             value (n = 0: the empty string rbx_bitset_import_n with length 0 creates); length + n > 2^29 is the
 *             size error above; *new_len = the new length.
 *   truncate  the script of RBinaryStream's channel, M/RedissonBinaryStream.java:181-190, step by step: STRLEN; if
 *             size >= length return; GETRANGE key 0 size-1; SET key that.  Its quirks are the contract: size 0 on a
 *             non-empty key is GETRANGE 0 -1, so the content stays and only the timeout goes (a negative size keeps
 *             the bytes [0, length + size - 1]); the SET drops the timeout and creates a missing key as the empty
 *             string when size < 0.
 * new_len is nullable.  The _dev forms take DEVICE byte buffers and enqueue on `stream` (NULL: the context's); like
 * rbx_bitset_set_indexes_dev they are exceptions to the *_dev convention: each waits once, for the string's length
 * (the range, the growth and the reply are host decisions; len / new_len are host words).  No form moves string bytes
 * through the host except the host forms' own upload or download of the caller's bytes. */
int rbx_string_getrange(rbx_ctx *ctx, rbx_name name, int64_t start, int64_t end, uint8_t *out, uint64_t cap, uint64_t *len);
int rbx_string_setrange(rbx_ctx *ctx, rbx_name name, int64_t offset, const uint8_t *bytes, uint64_t n, uint64_t *new_len);
int rbx_string_append(rbx_ctx *ctx, rbx_name name, const uint8_t *bytes, uint64_t n, uint64_t *new_len);
int rbx_string_truncate(rbx_ctx *ctx, rbx_name name, int64_t size);
int rbx_string_getrange_dev(rbx_ctx *ctx, rbx_name name, int64_t start, int64_t end, uint8_t *d_out, uint64_t cap,
                            uint64_t *len, void *stream);
int rbx_string_setrange_dev(rbx_ctx *ctx, rbx_name name, int64_t offset, const uint8_t *d_bytes, uint64_t n,
                            uint64_t *new_len, void *stream);
int rbx_string_append_dev(rbx_ctx *ctx, rbx_name name, const uint8_t *d_bytes, uint64_t n, uint64_t *new_len, void *stream);
/* An ordered stream of GETRANGE / SETRANGE / APPEND / GET commands over many keys in one call: what Spring Data sends
 * between openPipeline() and closePipeline() (get :487, mGet :499 as n GETs, append :610, getRange :617, setRange :624)
 * and the per-entity twin of rbx_bitset_range_stream ("append today's byte to every user's string").
 *   Commands  command i runs on names[cmd_key[i]].  GETRANGE: a = start, b = end.  SETRANGE: a = offset, the value is
 *             vals[val_off .. val_off + val_len).  APPEND: that value.  GET: the whole string.  Fields a command does
 *             not use are ignored.  Two entries of `names` with equal bytes are one key.
 *   Result    exactly that of n single calls in array order: a GETRANGE / GET sees every earlier SETRANGE / APPEND of
 *             its key, overlapping writes resolve in submission order, an APPEND lies at the running length the
 *             commands before it produced.  replies[i] = the new length for a write, the byte count for a read.  off
 *             = n + 1 words, the exclusive prefix sums of the reads' byte counts (a write counts 0): read i's bytes
 *             are out[off[i] .. off[i + 1]), and *total = off[n].
 *   Status    status[i] = 0 for a command that ran, 1 for the nil of GET on a missing key (rbx_string_getrange's
 *             empty reply is 0), 0xFF for a command that failed alone.  replies, status and total are nullable.
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above: the failures of the single calls (SETRANGE's offset, the
 *             key's type, the size -- which for an APPEND depends on the running length, data) fail the command
 *             alone; it changes nothing, its reply is 0 and it does not move the running length, and a key whose only
 *             writes failed is not created.  A GET on a key of another type fails like the others (Spring's mGet
 *             maps it to nil).  The call returns the first failing command's code in array order, its message in
 *             rbx_last_error().
 *   Caller    RBX_E_ILLEGAL_ARGUMENT with nothing changed and nothing created: cmd_key[i] >= nkeys, an op above
 *             RBX_STR_GET, a value slice that leaves vals[0 .. vals_len), NULL names / cmd_key / cmds / off with n > 0,
 *             NULL vals with vals_len > 0, NULL out with cap > 0 -- and total > cap.  The call plans every command
 *             before it writes any, so a call whose reads do not fit `out` is refused BEFORE any write, with off (and
 *             *total) filled in exactly: the caller sizes `out` from them and asks again.  Nothing is truncated (as
 *             rbx_bitset_members_stream does): a call that also writes cannot be repeated.  n = 0 sends nothing
 *             (off[0] = 0).
 *   Device    an allocation that fails while the written keys are created or grown (RBX_E_OOM, RBX_E_DEVICE) ends the
 *             call before any command ran: the keys it had created by then are removed again; a key it had already
 *             grown keeps its larger allocation, with its bytes and length as they were.
 *   Cost      each distinct name is looked up once.  A planning pass sorts the commands by key and walks each key's
 *             run with one lane, from the key's length word (one key holding the whole call is one lane: DESIGN
 *             11.12); the host then creates or grows every written key once, to its final length.  A group of
 *             rbx_tune "bytestream_lanes" lanes per key executes the key's commands in order; a command that moves
 *             more than "bytestream_short_max" bytes is cut into tiles of "bytestream_tile" bytes that the whole
 *             device sweeps between two walks -- one such command per key and round, so a call makes 1 + (the most
 *             long commands on one key) rounds of launches and no wait between them.  Up to "bytestream_serial_max"
 *             commands without a long one run as one lane group in array order.  One wait per chunk of
 *             "bytestream_chunk" commands; the last one also brings the total and the keys' final lengths.
 *   Scope     no handle form; the node router and the Java shim do not carry these calls.
 * `names` is host memory in both forms; the _dev form takes device arrays (d_off[n] is the total; total stays a host
 * word) and enqueues on `stream`. */
enum { RBX_STR_GETRANGE = 0, RBX_STR_SETRANGE = 1, RBX_STR_APPEND = 2, RBX_STR_GET = 3 };
typedef struct {
    int64_t a, b;     /* GETRANGE start, end; SETRANGE offset in a */
    uint64_t val_off; /* SETRANGE / APPEND: the value is vals[val_off .. val_off + val_len) */
    uint32_t val_len;
    uint8_t op; /* RBX_STR_* */
    uint8_t pad[3];
} rbx_string_cmd; /* 32 bytes */
int rbx_string_stream(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                      const rbx_string_cmd *cmds, uint64_t n, const uint8_t *vals, uint64_t vals_len, uint64_t cap,
                      uint64_t *off, uint8_t *out, int64_t *replies, uint8_t *status, uint64_t *total);
int rbx_string_stream_dev(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                          const rbx_string_cmd *d_cmds, uint64_t n, const uint8_t *d_vals, uint64_t vals_len,
                          uint64_t cap, uint64_t *d_off, uint8_t *d_out, int64_t *d_replies, uint8_t *d_status,
                          uint64_t *total, void *stream);
/* one command over a host string, no context (as rbx_bitset_range_of); missing != 0 = a missing key.  A read writes
 * min(cap, its byte count) bytes to out; a write stores nothing (the failure and the lengths follow from len alone:
 * bytes may be NULL for a write) and reports *new_len.  *reply as the stream's; a GET on a missing key is RBX_OK with
 * *reply = -1.  Returns what the single call returns. */
int rbx_string_range_of(const uint8_t *bytes, uint64_t len, int missing, const rbx_string_cmd *cmd, const uint8_t *vals,
                        uint8_t *out, uint64_t cap, int64_t *reply, uint64_t *new_len);

/* ---- replicas ("replicate the bitmap, split contains keys across GPUs") ---------
 * Redisson serves contains' GETBITs as reads that may go to a replica
 * (M/RedissonBitSet.java:277-279 readAsync, ReadMode.SLAVE M/config/BaseMasterSlaveServersConfig.java:60)
 * and SETBITs to the master.  These are the engine's replica primitives. */
/* Order-independent 64-bit digest of `GET name` (0 = missing key): equal replicas have equal
 * digests (compared over a collective instead of moving the bitmaps). */
int rbx_bloom_digest(rbx_ctx *ctx, const char *name, uint64_t *out);
int rbx_bloom_digest_n(rbx_ctx *ctx, rbx_name name, uint64_t *out);
/* Replica sync inside one process: dst's {name}:config and bitmap string := src's, copied
 * device to device (hipMemcpyPeerAsync over xGMI between GPUs).  Key timeouts are not copied. */
int rbx_bloom_copy_to(rbx_ctx *src, rbx_ctx *dst, rbx_name name);
/* dst_name on dst := src_name on src (HLL registers, encoding, cached cardinality), device to
 * device; a missing source deletes dst_name.  PFCOUNT / PFMERGE inputs from another GPU. */
int rbx_hll_copy_to(rbx_ctx *src, rbx_name src_name, rbx_ctx *dst, rbx_name dst_name);
/* Enables peer access from `device` to `peer` where the hardware allows (best effort). */
int rbx_enable_peer_access(int device, int peer);

/* ---- Bloom handles and the device-resident batch path ------------------------------ */
int rbx_bloom_open(rbx_ctx *ctx, const char *name, rbx_bloom **out);
int rbx_bloom_open_n(rbx_ctx *ctx, rbx_name name, rbx_bloom **out);
int rbx_bloom_close(rbx_bloom *b);
int rbx_bloom_handle_config(const rbx_bloom *b, uint64_t *size, uint32_t *k);
/* contains over device-resident keys; *d_count += present keys (device word). */
int rbx_bloom_contains_dev(rbx_ctx *ctx, rbx_bloom *b, const rbx_keys *d_keys,
                           uint8_t *d_out_present, unsigned long long *d_count, void *stream);
/* add over device-resident keys; *d_count += newly added keys (device word).
 * Exception to the *_dev convention: a large batch on a large filter (the region-partitioned add,
 * bitmap >= 8 MiB and >= max(2^17, bits / 2^12) keys) waits on the stream once per chunk of up to
 * ~55M keys, for the chunk's bucket-overflow flag -- an adversarial batch (one key repeated ~1e5
 * times) reruns that chunk on the first-setter table path before the next chunk starts. */
int rbx_bloom_add_dev(rbx_ctx *ctx, rbx_bloom *b, const rbx_keys *d_keys, uint8_t *d_out_new,
                      unsigned long long *d_count, void *stream);
/* Multi-tenant batch: segment s = keys [seg_offsets[s], seg_offsets[s+1]) tested
 * against filters[s] -- one Redisson contains(Collection) per segment.
 * Device pointers: d_seg_offsets (nseg+1 u64), d_counts (nseg u64, accumulated). */
int rbx_bloom_contains_multi_dev(rbx_ctx *ctx, rbx_bloom *const *filters, uint32_t nseg,
                                 const uint64_t *d_seg_offsets, const rbx_keys *d_keys,
                                 uint8_t *d_out_present, unsigned long long *d_counts, void *stream);
/* add() per segment, segments applied in order (same semantics as nseg calls).  Enqueued on `stream`;
 * when every filter of the batch is distinct and the batch holds more than 16,384 keys, the call waits
 * for its per-segment kernel (one flag read back) to learn whether a segment that long needs the
 * chunked path (M/RedissonBloomFilter.java:104-137). */
int rbx_bloom_add_multi_dev(rbx_ctx *ctx, rbx_bloom *const *filters, uint32_t nseg,
                            const uint64_t *d_seg_offsets, const rbx_keys *d_keys,
                            uint8_t *d_out_new, unsigned long long *d_counts, void *stream);
/* Host-buffer multi-tenant forms (synchronous). */
int rbx_bloom_contains_multi(rbx_ctx *ctx, rbx_bloom *const *filters, uint32_t nseg,
                             const uint64_t *seg_offsets, const rbx_keys *keys,
                             uint8_t *out_present, uint64_t *out_counts);
int rbx_bloom_add_multi(rbx_ctx *ctx, rbx_bloom *const *filters, uint32_t nseg,
                        const uint64_t *seg_offsets, const rbx_keys *keys, uint8_t *out_new,
                        uint64_t *out_counts);

/* Ordered mixed stream (BASELINE C5): key i is one contains(T) (key_op[i] = 0) or add(T)
 * (key_op[i] = 1) on filters[key_filter[i]], executed in key order -- an add is visible to
 * every later contains of the same filter, exactly as the commands would run one after
 * another (M/RedissonBloomFilter.java:99-102, :198-201).  out (nullable): per key, present /
 * newly added.  counts[0] = present contains, counts[1] = newly added.  k <= 32.
 * A filter without a bitmap string: the host form creates it only if one of its commands adds to it (GETBIT on a
 * missing key creates nothing); the _dev form, whose ops are device memory, creates it for every filter it names,
 * empty if no add reaches it.  A call that is refused (k > 32, a changed config, another type) creates none. */
int rbx_bloom_stream_dev(rbx_ctx *ctx, rbx_bloom *const *filters, uint32_t nfilters, const uint32_t *d_key_filter,
                         const uint8_t *d_key_op, const rbx_keys *d_keys, uint8_t *d_out,
                         unsigned long long *d_counts, void *stream);
int rbx_bloom_stream(rbx_ctx *ctx, rbx_bloom *const *filters, uint32_t nfilters, const uint32_t *key_filter,
                     const uint8_t *key_op, const rbx_keys *keys, uint8_t *out, uint64_t *counts);

/* ---- RHyperLogLog (by name) -- M/api/RHyperLogLog.java:27-68 -------------------- */
/* add / addAll -> PFADD name e1..en   M/RedissonHyperLogLog.java:71-81.
 * *changed = 1 iff the key was created or any register changed. */
int rbx_hll_add(rbx_ctx *ctx, const char *name, const rbx_keys *elements, int *changed);
/* A batch of PFADD commands: segment s adds elements [seg_offsets[s], seg_offsets[s+1])
 * to names[s]; out_changed[s] is the reply of command s (commands apply in order).  A name that holds a key
 * of another type fails the whole call with RBX_E_WRONGTYPE before any command runs or any key is created. */
int rbx_hll_add_multi(rbx_ctx *ctx, const char *const *names, uint32_t nseg,
                      const uint64_t *seg_offsets, const rbx_keys *elements, uint8_t *out_changed);
/* count / countWith -> PFCOUNT k1..kn (union when n > 1)  :84-94 */
int rbx_hll_count(rbx_ctx *ctx, const char *const *names, uint32_t n, uint64_t *out);
/* n independent single-key PFCOUNTs in one batch (one GPU pass). */
int rbx_hll_count_each(rbx_ctx *ctx, const char *const *names, uint32_t n, uint64_t *out);
/* mergeWith -> PFMERGE dest src1..srcn (dest's registers included)  :97-102 */
int rbx_hll_merge(rbx_ctx *ctx, const char *dest, const char *const *srcs, uint32_t nsrc);
/* GET name: Redis dense HLL string (16-byte "HYLL" header + 12288 bytes).  *len = 0 if absent. */
int rbx_hll_export(rbx_ctx *ctx, const char *name, uint8_t *out, uint64_t cap, uint64_t *len);
/* GET name in a chosen encoding ([redis-7.2] hyperloglog.c):
 *   RBX_HLL_DENSE      the dense string (as rbx_hll_export);
 *   RBX_HLL_SPARSE     ZERO / XZERO / VAL opcodes: a key Redis holds sparse exports its string
 *                      (below); a dense key the fewest-bytes opcodes of its registers
 *                      (ILLEGAL_ARGUMENT if a register > 32);
 *   RBX_HLL_AS_STORED  what GET returns in Redis: PFADD creates sparse strings and applies each
 *                      element in order through hllSparseSet, promoting to dense (one way) at the
 *                      first element that stores a value > 32 or grows the string past
 *                      hll-sparse-max-bytes (3000); SET keeps the imported string; PFMERGE's
 *                      destination is dense iff it or any source is, else its string takes the
 *                      maxima register by register (pfmergeCommand).
 * *len receives the full length; at most cap bytes are copied. */
enum { RBX_HLL_DENSE = 0, RBX_HLL_SPARSE = 1, RBX_HLL_AS_STORED = 2 };
int rbx_hll_export_enc(rbx_ctx *ctx, const char *name, int encoding, uint8_t *out, uint64_t cap, uint64_t *len);
/* SET name <Redis HLL string> (dense or sparse encoding) */
int rbx_hll_import(rbx_ctx *ctx, const char *name, const uint8_t *bytes, uint64_t len);
int rbx_hll_delete(rbx_ctx *ctx, const char *name, int *deleted);
int rbx_hll_exists(rbx_ctx *ctx, const char *name, int *exists);
/* binary-name forms (Spring Data pfAdd/pfCount/pfMerge with byte[] keys,
 * redisson-spring-data-32 RedissonConnection.java:2200-2226) */
int rbx_hll_add_multi_n(rbx_ctx *ctx, const rbx_name *names, uint32_t nseg, const uint64_t *seg_offsets,
                        const rbx_keys *elements, uint8_t *out_changed);
int rbx_hll_count_n(rbx_ctx *ctx, const rbx_name *names, uint32_t n, uint64_t *out);
int rbx_hll_merge_n(rbx_ctx *ctx, rbx_name dest, const rbx_name *srcs, uint32_t nsrc);
int rbx_hll_export_enc_n(rbx_ctx *ctx, rbx_name name, int encoding, uint8_t *out, uint64_t cap, uint64_t *len);
int rbx_hll_import_n(rbx_ctx *ctx, rbx_name name, const uint8_t *bytes, uint64_t len);
/* An ordered stream of PFADD / single-key PFCOUNT commands over many keys in one call: what a batch queues
 * through RBatch.getHyperLogLog(name) (M/RedissonBatch.java:57-64, M/api/RBatch.java:213-215: addAsync,
 * addAllAsync, countAsync), executes in submission order and answers in that order; Spring Data reaches the
 * same shape with pfAdd / pfCount between openPipeline() and closePipeline().
 *   Commands  command i is (names[cmd_key[i]], cmd_op[i]).  A PFADD carries the elements [cmd_elem[i],
 *             cmd_elem[i + 1]) of `elements` (cmd_elem has n + 1 entries; the range may be empty); a PFCOUNT
 *             names one key and its range is empty.  Two entries of `names` with equal bytes are one key.
 *   Result    exactly that of n single calls in array order -- rbx_hll_add_multi_n with one segment for a PFADD,
 *             rbx_hll_count_n with one key for a PFCOUNT.  replies[i] (nullable array) is 1 for a PFADD iff the
 *             key was created or a register changed, and the cardinality for a PFCOUNT.  A PFADD sees every
 *             earlier PFADD of its key; the first PFADD that runs on a missing key creates it and replies 1,
 *             also without elements.  The header's cached cardinality is PFCOUNT's and PFADD's: a PFCOUNT
 *             returns a valid cache as it stands and stores a recount; a PFADD sets the invalid bit only when
 *             a register changed, and the low 63 bits stay.  A sparse string takes its key's elements through
 *             hllSparseSet in command order across all of that key's commands (promotion is sticky, at the
 *             first value above 32 or at growth past hll-sparse-max-bytes).  Timeouts are kept.
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above: a command whose key holds another type (a bit
 *             string, a {name}:config hash) fails alone.  status[i] (nullable array) is 0xFF and its reply 0;
 *             it changes and creates nothing.  Every other command runs (status 0) with its exact reply.  The
 *             call returns RBX_E_WRONGTYPE, the code of the first failing command in array order, with the
 *             HLL wrong-type message in rbx_last_error().
 *   Caller    cmd_key[i] >= nkeys, cmd_op[i] > 1, offsets that do not ascend or do not span [0, elements->n],
 *             a PFCOUNT with elements, or a NULL array with n > 0 is RBX_E_ILLEGAL_ARGUMENT with nothing
 *             changed and nothing created.  n = 0 sends nothing.
 *   Cost      the host splits the stream into phases: a phase is a maximal stretch in which no PFCOUNT names a
 *             key that an earlier PFADD of the stretch names.  A phase's PFCOUNTs run first, as one pass over
 *             the state before it, then its PFADDs as one add run, whose launch count does not depend on how
 *             often keys repeat.  Adds followed by counts are two phases; add, count, add, count
 *             on one key is one phase per pair -- a PFCOUNT is a 16,384-register scan either way.
 *   Scope     multi-key PFCOUNT and PFMERGE are not part of a stream: many of them travel through
 *             rbx_hll_count_groups / rbx_hll_merge_groups below.  The node router and the Java shim do not
 *             carry this call.  There is no point-in-time PFCOUNT from inside one launch: a count that must
 *             see an earlier add of its key closes the phase.
 * The command arrays, `names`, `replies` and `status` are host memory in both forms: the host must know the
 * commands to create the keys (as rbx_hll_add_multi_dev's h_seg_offsets).  The _dev form takes `elements` in
 * device memory and enqueues on `stream` (NULL: the context's); like the two bit streams it is an exception to
 * the *_dev convention: it waits on the stream, once per add run and count pass and at its end. */
enum { RBX_HLL_PFADD = 0, RBX_HLL_PFCOUNT = 1 };
int rbx_hll_stream(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key, const uint8_t *cmd_op,
                   const uint64_t *cmd_elem, uint64_t n, const rbx_keys *elements, uint64_t *replies, uint8_t *status);
int rbx_hll_stream_dev(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                       const uint8_t *cmd_op, const uint64_t *cmd_elem, uint64_t n, const rbx_keys *d_elements,
                       uint64_t *replies, uint8_t *status, void *stream);
/* Many multi-key PFCOUNTs, and many PFMERGEs, in one call each: what RHyperLogLog.countWith / mergeWith send one
 * command at a time (M/RedissonHyperLogLog.java:89-102), what a batch queues through
 * RBatch.getHyperLogLog(name).countWithAsync / mergeWithAsync (M/RedissonBatch.java:57-64), and Spring Data's
 * pfCount(k1, k2, ..) / pfMerge between openPipeline() and closePipeline(): the roll-ups that sketches exist for
 * (daily uniques from 24 hourly HLLs, one window per group).
 *   Commands  group g names the keys names[grp_key[grp_off[g] .. grp_off[g + 1])] (grp_off has ngroups + 1 entries
 *             and ascends from 0).  rbx_hll_count_groups: PFCOUNT of those keys, at least one.
 *             rbx_hll_merge_groups: PFMERGE names[grp_dest[g]] <those keys>; no source is legal.  Two entries of
 *             `names` with equal bytes are one key.
 *   Result    exactly that of ngroups single calls in array order -- rbx_hll_count_n into out[g], rbx_hll_merge_n.
 *             A count of one entry is the single-key PFCOUNT with the header cache: a valid cache is returned as
 *             it stands, otherwise the recount is stored.  A count of two or more entries -- counted as Redis
 *             counts argc, so [a, a] is one -- is the count of the register maxima and touches no header.  A
 *             missing key is empty; counts do not affect each other.  A merge includes the destination's own
 *             registers, creates a missing destination (sparse, one XZERO) first, leaves it dense iff it or any
 *             existing source is dense, else writes the maxima back through hllSparseSet in ascending register
 *             order (which may promote: a value above 32, growth past hll-sparse-max-bytes), and sets the cached
 *             cardinality's invalid bit always, also without sources; the low 63 bits and the timeout stay.
 *             Later merges see earlier ones: a destination may be a later group's source, a source a later
 *             group's destination, one key the destination twice; a source equal to its destination changes
 *             nothing.
 *   Failures  the pipelined-batch rule of RBX_E_REDIS above: a group that names a key of another type (a bit
 *             string, a {name}:config hash) anywhere fails alone.  status[g] (nullable array) is 0xFF, out[g] is 0,
 *             and it changes, stores and creates nothing.  Every other group runs (status 0) with its exact
 *             result.  The call returns RBX_E_WRONGTYPE, the code of the first failing group in array order, with
 *             the HLL wrong-type message in rbx_last_error().
 *   Caller    a count group without entries, an entry or destination >= nkeys, offsets that do not ascend from 0,
 *             or a NULL array with ngroups > 0 is RBX_E_ILLEGAL_ARGUMENT with nothing changed and nothing created.
 *             ngroups = 0 sends nothing.  A call takes fewer than 2^31 groups and 2^32 entries.
 *   Cost      each distinct name is looked up once.  Counts: one table upload, one launch that reads every
 *             member's 16 KiB once and ends in the estimator (plus a fill and a one-lane-per-group finish launch
 *             when few groups are spread over several workgroups each, rbx_tune "hllgroups_split"), one copy
 *             back, one wait; one-key counts with a valid cache never reach the device; a union that holds a
 *             register of 51 is finished on the host.  Merges: the host splits the groups into phases -- a group
 *             closes the phase before it when its destination is a destination or a source of an earlier group of
 *             the phase, or one of its sources is such a destination -- and runs each phase as one merge launch,
 *             one write-back launch for the destinations that stay sparse, and at most one wait (for the sparse
 *             keys' promotion words).  Independent merges are one phase; a chain of dependent ones is a phase
 *             each.
 *   Scope     the node router and the Java shim do not carry these calls.  No handle or device-pointer forms.
 *             PFADD and single-key PFCOUNT streams stay rbx_hll_stream's.
 * All arrays are host memory: the host must know the keys to create the destinations. */
int rbx_hll_count_groups(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint64_t *grp_off,
                         const uint32_t *grp_key, uint32_t ngroups, uint64_t *out, uint8_t *status);
int rbx_hll_merge_groups(rbx_ctx *ctx, const rbx_name *names, uint32_t nkeys, const uint32_t *grp_dest,
                         const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups, uint8_t *status);

/* ---- HLL handles and the device-resident path ------------------------------------- */
/* Opens (creating an empty HLL if absent and create != 0). */
int rbx_hll_open(rbx_ctx *ctx, const char *name, int create, rbx_hll **out);
int rbx_hll_open_n(rbx_ctx *ctx, rbx_name name, int create, rbx_hll **out);
int rbx_hll_close(rbx_hll *h);
/* Device address of the 16384 u8 registers (raw, one byte per register). */
int rbx_hll_registers_dev(rbx_hll *h, void **d_regs);
/* PFADD batch over device-resident elements; d_changed[s] |= 1 when command s
 * changed a register.  Each handle may appear at most once per call. */
int rbx_hll_add_multi_dev(rbx_ctx *ctx, rbx_hll *const *hlls, uint32_t nseg,
                          const uint64_t *d_seg_offsets, const uint64_t *h_seg_offsets,
                          const rbx_keys *d_elements, uint32_t *d_changed, void *stream);
/* Single-key PFCOUNT of each handle into host out[i] (synchronous). */
int rbx_hll_count_each_handles(rbx_ctx *ctx, rbx_hll *const *hlls, uint32_t n, uint64_t *out);

/* Register exchange of an element-partitioned HLL set (any transport): pack copies the
 * registers of hlls[i] to d_buf[i*16384 .. (i+1)*16384) in the caller's order; unpack_max
 * merges them back (register = max(register, buffer byte), PFMERGE semantics) and invalidates
 * the cached cardinalities.  Both enqueue on `stream` (NULL = the context's) and return. */
int rbx_hll_pack_registers(rbx_ctx *ctx, rbx_hll *const *hlls, uint32_t n, void *d_buf, void *stream);
int rbx_hll_unpack_max_registers(rbx_ctx *ctx, rbx_hll *const *hlls, uint32_t n, const void *d_buf, void *stream);

/* ---- multi-GPU (RCCL over xGMI) ------------------------------------------------------ */
/* 128-byte ncclUniqueId, created on rank 0 and broadcast by the caller. */
int rbx_rccl_unique_id(uint8_t out[128]);
int rbx_rccl_init(rbx_ctx *ctx, const uint8_t id[128], int nranks, int rank);
/* The communicator as RCCL reports it (ncclCommCount / ncclCommUserRank). */
int rbx_rccl_info(rbx_ctx *ctx, int *nranks, int *rank);
/* In-place uint8 MAX all-reduce of the registers of hlls[0..n) across ranks: pack (in the
 * given order) -> ONE ncclAllReduce(ncclUint8, ncclMax) of n x 16384 bytes -> unpack_max, so
 * every rank issues the same collective whatever its register pool layout.  Every rank passes
 * the same names in the same order. */
int rbx_hll_allreduce_max(rbx_ctx *ctx, rbx_hll *const *hlls, uint32_t n);

/* ---- asynchronous calls: the RFuture surface of RHyperLogLogAsync ---------------------------
 * M/api/RHyperLogLogAsync.java:37-70 (addAsync, addAllAsync, countAsync, countWithAsync,
 * mergeWithAsync; RBloomFilter has no async API in the reference -- the Bloom forms are an
 * engine extension).  Each *_async call is queued on the context's serial executor and runs after
 * every call queued before it on that context; it returns at once with a future.  Names, segment
 * offsets and the rbx_keys descriptor are copied at submit time; key bytes and result buffers
 * must stay valid until the future completes.  `cb` (nullable) runs when the call completes. */
int rbx_future_wait(rbx_future *f, int64_t timeout_ms, int *call_rc); /* RBX_E_TIMEOUT if not done;
                                                                         timeout_ms < 0 waits for ever */
int rbx_future_done(rbx_future *f, int *done);
int rbx_future_free(rbx_future *f);  /* may be called before completion (the result is dropped) */
int rbx_bloom_add_async(rbx_ctx *ctx, const char *name, uint64_t size, uint32_t k, const rbx_keys *keys,
                        uint8_t *out_new, uint64_t *out_count, rbx_callback cb, void *user, rbx_future **out);
int rbx_bloom_contains_async(rbx_ctx *ctx, const char *name, uint64_t size, uint32_t k, const rbx_keys *keys,
                             uint8_t *out_present, uint64_t *out_count, rbx_callback cb, void *user,
                             rbx_future **out);
int rbx_hll_add_async(rbx_ctx *ctx, const char *name, const rbx_keys *elements, int *changed, rbx_callback cb,
                      void *user, rbx_future **out);
int rbx_hll_add_multi_async(rbx_ctx *ctx, const char *const *names, uint32_t nseg, const uint64_t *seg_offsets,
                            const rbx_keys *elements, uint8_t *out_changed, rbx_callback cb, void *user,
                            rbx_future **out);
int rbx_hll_count_async(rbx_ctx *ctx, const char *const *names, uint32_t n, uint64_t *result, rbx_callback cb,
                        void *user, rbx_future **out);
int rbx_hll_merge_async(rbx_ctx *ctx, const char *dest, const char *const *srcs, uint32_t nsrc, rbx_callback cb,
                        void *user, rbx_future **out);

/* ---- one process over the GPUs of a node -----------------------------------------------------
 * A node holds one context per GPU and routes every name by Redis Cluster slot, the way the
 * reference's client groups a batch per node (M/command/CommandBatchService.java:569-604,
 * M/cluster/ClusterConnectionManager.java:777-830): GPU = calc_slot(name) * n_gpus / 16384, so a
 * filter's bitmap `name` and its `{name}:config` live on one GPU.  devices: the HIP device of
 * each of the n_gpus contexts (NULL = 0..n_gpus-1; a device may repeat, e.g. to rehearse a node
 * on one GPU).  Multi-tenant batches are scattered by slot into per-GPU batches, run
 * concurrently (one host thread per GPU, each GPU its own context and stream) and gathered back
 * in segment order.  Calls on one node from several threads are safe. */
int rbx_node_init(int n_gpus, const int *devices, rbx_node **out);
int rbx_node_shutdown(rbx_node *node);
int rbx_node_size(const rbx_node *node, int *n_gpus);
int rbx_node_gpu_of(const rbx_node *node, rbx_name name, int *gpu);
int rbx_node_ctx(rbx_node *node, int gpu, rbx_ctx **out); /* the GPU's context (device-path calls) */
int rbx_node_bloom_try_init(rbx_node *node, rbx_name name, int64_t expected_insertions, double false_probability,
                            int *created);
int rbx_node_bloom_read_config(rbx_node *node, rbx_name name, rbx_bloom_config *out);
int rbx_node_bloom_add(rbx_node *node, rbx_name name, uint64_t size, uint32_t k, const rbx_keys *keys,
                       uint8_t *out_new, uint64_t *out_count);
int rbx_node_bloom_contains(rbx_node *node, rbx_name name, uint64_t size, uint32_t k, const rbx_keys *keys,
                            uint8_t *out_present, uint64_t *out_count);
int rbx_node_bloom_count(rbx_node *node, rbx_name name, int64_t *out);
int rbx_node_del(rbx_node *node, const rbx_name *names, uint32_t n, int *deleted);
/* Replicated filter (SURVEY 8e, C2 "replicas only"): on != 0 copies the filter (config hash +
 * bitmap) from its home GPU to every other GPU, device to device, then routes every add of it
 * to all replicas (the home GPU's reply is returned) and spreads its contains over them (one
 * key range per replica; multi-tenant segments round-robin) -- Redisson's reads-from-replicas
 * (GETBIT via readAsync, M/RedissonBitSet.java:277-279; ReadMode.SLAVE,
 * M/config/BaseMasterSlaveServersConfig.java:60).  on == 0 drops the copies.  DEL of the
 * filter's keys deletes every copy; deleting its config ends the replication. */
int rbx_node_bloom_replicate(rbx_node *node, rbx_name name, int on);
int rbx_node_bloom_is_replicated(rbx_node *node, rbx_name name, int *replicated);
/* segment s = keys [seg_offsets[s], seg_offsets[s+1]) of names[s] (host buffers; a segment must
 * be non-empty, as contains/add(Collection) of an empty collection throw); out_* nullable. */
int rbx_node_bloom_contains_multi(rbx_node *node, const rbx_name *names, uint32_t nseg, const uint64_t *seg_offsets,
                                  const rbx_keys *keys, uint8_t *out_present, uint64_t *out_counts);
int rbx_node_bloom_add_multi(rbx_node *node, const rbx_name *names, uint32_t nseg, const uint64_t *seg_offsets,
                             const rbx_keys *keys, uint8_t *out_new, uint64_t *out_counts);
/* PFADD commands routed per name (commands on one name keep their order) */
int rbx_node_hll_add_multi(rbx_node *node, const rbx_name *names, uint32_t nseg, const uint64_t *seg_offsets,
                           const rbx_keys *elements, uint8_t *out_changed);
/* PFCOUNT / PFMERGE over names that may live on different GPUs: every HLL held by another GPU is
 * peer-copied device to device (rbx_hll_copy_to: registers, encoding, cached cardinality and the
 * sparse string, over xGMI on a multi-GPU node) into a temporary key on the GPU of the first name
 * (PFCOUNT) or of the destination (PFMERGE), which is deleted after the call -- no host staging.
 * M/RedissonHyperLogLog.java:89-102 (countWith / mergeWith). */
int rbx_node_hll_count(rbx_node *node, const rbx_name *names, uint32_t n, uint64_t *out);
int rbx_node_hll_merge(rbx_node *node, rbx_name dest, const rbx_name *srcs, uint32_t nsrc);

#ifdef __cplusplus
}
#endif
#endif /* RBX_H */
