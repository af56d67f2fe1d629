// api_bitset_multi.cpp -- RBitSet's calls over many keys: the ordered GETBIT / SETBIT and BITFIELD streams, grouped
// BITOPs / BITCOUNTs, and the two read streams in two tiers.  api_bitset.cpp has the single key.
#include <cstring>

#include "bit_groups_plan.h"
#include "hll_groups_plan.h"  // hll_groups_check: the grouped calls share their limits
#include "rbx_ctx.h"
#include "tunables.h"

#include "members_rule.h"  // after rbx_device.h, whose RBX_HD it then uses

namespace rbx {

// ---- the ordered GETBIT / SETBIT stream over many keys (RBatch.getBitSet, M/RedissonBatch.java:182-184) ----
// The keys of one stream call, its names resolved once, lookup only (stream_names_resolve has the rules)
struct StreamKeys {
    uint32_t nkeys = 0;
    std::vector<std::string> nm;
    std::vector<uint8_t> kinfo;  // canonical ids | wrong-type flags, as the summary kernels read them
    uint32_t *canon() { return (uint32_t *)kinfo.data(); }
    uint8_t *wrong() { return kinfo.data() + (size_t)nkeys * 4; }
    StreamKeys(rbx_ctx *c, const rbx_name *names, uint32_t n) : nkeys(n), kinfo((size_t)n * 5, 0) {
        stream_names_resolve(c, names, n, KType::Bitmap, &nm, canon(), wrong(), [](uint32_t, const Entry &) {});
    }
};

// Creates or grows every string the batch writes -- keymax[i] = 1 + the last bit a command that runs writes
// on canonical key i, 0 = none; a null keymax: nothing is written -- then uploads the table over the final
// allocations.  *writes = some key is written (its length word is to be raised).
static int stream_keys_table(rbx_ctx *c, StreamKeys &sk, const unsigned long long *keymax, hipStream_t st,
                             const BitKey **d_tab, bool *writes) {
    const uint32_t *canon = sk.canon();
    const uint8_t *wrong = sk.wrong();
    std::vector<BitKey> tab(sk.nkeys);
    *writes = false;
    for (uint32_t i = 0; i < sk.nkeys; ++i) {
        BitKey &k = tab[i];
        if (canon[i] != i) {
            k = tab[canon[i]];
            continue;
        }
        k = BitKey{nullptr, 0, nullptr, wrong[i] ? kBitKeyWrong : 0u, i};
        if (wrong[i]) continue;
        std::shared_ptr<Bitmap> bm;
        const uint64_t mx1 = keymax ? keymax[i] : 0;
        if (mx1) {
            RBX_TRY(bitset_for_write(c, sk.nm[i], ((mx1 - 1) >> 3) + 1, st, &bm));
            *writes = true;
        } else {
            RBX_TRY(bitset_find(c, sk.nm[i], &bm));
        }
        if (bm) k = BitKey{bm->d_words, bm->cap_bytes * 8, bm->d_len, 0u, i};
    }
    *d_tab = c->dev->bits.bst_table.sync(tab, st);
    return *d_tab ? RBX_OK : c->dev->bits.bst_table.err;
}

// what both bit streams check before anything runs; arrays: every per-command array is there
static int stream_args_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, uint64_t n, bool arrays) {
    if (n && !arrays) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(stream_names_check(c, names, nkeys));
    // a cell is (key id, index) in 64 bits, one of them the failed commands'
    if (nkeys > (1u << 31)) return fail(RBX_E_ILLEGAL_ARGUMENT, "a batch takes at most 2^31 keys");
    return RBX_OK;
}

// The summary pass of both bit streams, before anything is written: the resolved keys' canonical ids | wrong-type
// flags uploaded to bst_keys, the `words` summary words set (the first `ones` of them, the "first position"
// minima, to ~0; the others and the nkeys per-key maxima behind them to 0), the stream's summary kernel through
// launch(d_canon, d_wrong, d_sum, d_keymax), and the one wait for what the batch needs.  *sum = the summary words
// | the per-key maxima; they stay in bst_sum for launch_bitstream_lengths.
template <class Launch>
static int stream_summary(rbx_ctx *c, const StreamKeys &sk, size_t words, size_t ones, hipStream_t st, Launch launch,
                          std::vector<unsigned long long> *sum) {
    const uint32_t nkeys = sk.nkeys;
    if (nkeys == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "a command's key is not below nkeys");
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.bst_keys.reserve(sk.kinfo.size()));
    HIP_TRY(hipMemcpyAsync(b.bst_keys.p, sk.kinfo.data(), sk.kinfo.size(), hipMemcpyHostToDevice, st));
    const size_t sum_bytes = (words + (size_t)nkeys) * 8;
    RBX_TRY(b.bst_sum.reserve(sum_bytes));
    auto *d_sum = b.bst_sum.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(d_sum, 0xFF, ones * 8, st));
    HIP_TRY(hipMemsetAsync(d_sum + ones, 0, sum_bytes - ones * 8, st));
    launch(b.bst_keys.as<uint32_t>(), b.bst_keys.as<uint8_t>() + (size_t)nkeys * 4, d_sum, d_sum + words);
    HIP_TRY(hipGetLastError());
    sum->resize(words + (size_t)nkeys);
    HIP_TRY(hipMemcpyAsync(sum->data(), d_sum, sum_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the one wait
    return RBX_OK;
}

// A batch of n > 0 commands over device arrays inside the caller's scope on `st`; d_replies nullable.
// *failed = RBX_OK, or the code of the first command in array order that failed alone (the caller
// reports it once the replies are where they belong).  Three steps: the summary pass, the host's decisions
// (create or grow every written key, build the key table, pick the path), the execution kernels and the lengths.
static int stream_run(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_key, const uint8_t *d_op,
                      const uint64_t *d_idx, uint64_t n, uint8_t *d_replies, hipStream_t st, int *failed) {
    *failed = RBX_OK;
    BitsetScratch &b = c->dev->bits;
    StreamKeys sk(c, names, nkeys);
    std::vector<unsigned long long> sum;
    RBX_TRY(stream_summary(c, sk, kBsSummaryWords, kBsFlags, st,
                           [&](const uint32_t *d_canon, const uint8_t *d_wrong, unsigned long long *d_sum,
                               unsigned long long *d_keymax) {
                               launch_bitstream_summary(d_key, d_op, d_idx, n, nkeys, d_canon, d_wrong, d_sum, d_keymax, st);
                           },
                           &sum));
    const unsigned long long *d_keymax = b.bst_sum.as<unsigned long long>() + kBsSummaryWords;
    const uint64_t first_oob = sum[kBsFirstOob], first_wrong = sum[kBsFirstWrong];
    const uint32_t flags = (uint32_t)sum[kBsFlags];
    if (flags & kBsIllegal) return fail(RBX_E_ILLEGAL_ARGUMENT, "a command's key is not below nkeys, or its op not 0, 1 or 2");
    const bool has_failed = (first_oob & first_wrong) != ~0ULL;
    const bool gets = flags & kBsHasGet, sets = flags & (kBsHasSet0 | kBsHasSet1);
    const bool one_value = (flags & (kBsHasSet0 | kBsHasSet1)) != (kBsHasSet0 | kBsHasSet1);

    // the strings the batch writes (keymax: 1 + the key's largest SETBIT index that runs), then the table
    const BitKey *d_tab;
    bool writes;
    RBX_TRY(stream_keys_table(c, sk, sum.data() + kBsSummaryWords, st, &d_tab, &writes));

    const int path = g_tune.bitstream_path;
    if (path == 0 && !sets) {
        if (d_replies) launch_bitstream_gather(d_tab, d_key, d_idx, n, d_replies, st);
    } else if (path == 0 && !gets && one_value && !d_replies) {
        launch_bitstream_scatter(d_tab, d_key, d_idx, n, (flags & kBsHasSet1) != 0, st);
    } else if (path == 1 || (path == 0 && n <= g_tune.bitstream_serial_max)) {
        launch_bitstream_serial(d_tab, d_key, d_op, d_idx, n, d_replies, st);
    } else {
        // consecutive chunks in order; a cell that spans two of them is read again by the second
        const uint64_t chunk = g_tune.bitstream_chunk;
        const int index_bits = std::max(1, significant_bits(sum[kBsMaxIndex]));
        const int key_bits = significant_bits((uint64_t)nkeys - 1);
        RBX_TRY(cell_sort_reserve<unsigned long long>(b.bst_sort, (uint32_t)std::min(n, chunk), 0,
                                                      index_bits + key_bits + (has_failed ? 1 : 0)));
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            const uint32_t m = (uint32_t)std::min(chunk, n - i0);
            RBX_TRY(sort_failed(launch_bitstream_grouped(d_tab, d_key + i0, d_op + i0, d_idx + i0, m,
                                                         d_replies ? d_replies + i0 : nullptr, index_bits, key_bits,
                                                         has_failed, b.bst_sort.p, b.bst_sort.cap, st)));
        }
    }
    if (writes) launch_bitstream_lengths(d_tab, d_keymax, nkeys, st);
    HIP_TRY(hipGetLastError());
    if (has_failed) *failed = first_oob < first_wrong ? RBX_E_REDIS : RBX_E_WRONGTYPE;
    return RBX_OK;
}

static int stream_failed(int code) {
    if (code == RBX_OK) return RBX_OK;
    return fail(code, code == RBX_E_REDIS ? kBitOffsetMsg : kWrongTypeMsg);
}

// ---- the ordered BITFIELD stream over many keys (RBatch.getBitSet's typed fields, M/api/RBitSetAsync.java:36-206) ----
enum { kFsPathNone = 0, kFsPathSerial = 1, kFsPathWords = 2, kFsPathKeys = 3, kFsPathGather = 4, kFsPathAtomic = 5 };
static std::atomic<int> g_fieldstream_last_path{kFsPathNone};  // rbx_bench_fieldstream_last_path shows it

// A batch of n > 0 commands over device arrays inside the caller's scope on `st`; d_replies and d_status
// nullable.  *failed = 0, or the failure kind (kFs*) of the first command in array order that failed alone.
// stream_run's steps: the summary pass, the host's decisions (the caller's errors, every written key created
// or grown, the key table, the path), one execution path, the lengths.
static int field_stream_run(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_key,
                            const rbx_field_cmd *d_cmds, uint64_t n, int64_t *d_replies, uint8_t *d_status,
                            hipStream_t st, int *failed) {
    *failed = 0;
    BitsetScratch &b = c->dev->bits;
    StreamKeys sk(c, names, nkeys);
    std::vector<unsigned long long> sum;
    RBX_TRY(stream_summary(c, sk, kFsSummaryWords, kFsFlags, st,
                           [&](const uint32_t *d_canon, const uint8_t *d_wrong, unsigned long long *d_sum,
                               unsigned long long *d_keymax) {
                               launch_fieldstream_summary(d_key, d_cmds, n, nkeys, d_canon, d_wrong, d_sum, d_keymax, st);
                           },
                           &sum));
    const unsigned long long *d_keymax = b.bst_sum.as<unsigned long long>() + kFsSummaryWords;
    const uint32_t flags = (uint32_t)sum[kFsFlags];
    if (flags & kFsIllegal)
        return fail(RBX_E_ILLEGAL_ARGUMENT,
                    "a command's key is not below nkeys, or its op, overflow mode or is_signed is unknown");
    if ((flags & kFsFail) && d_replies && !d_status)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "OVERFLOW FAIL with replies needs status");
    const uint64_t first[3] = {sum[kFsFirstType], sum[kFsFirstOffset], sum[kFsFirstWrong]};
    const uint64_t first_failed = std::min(first[0], std::min(first[1], first[2]));
    const bool has_failed = first_failed != ~0ULL;

    const BitKey *d_tab;
    bool writes;
    RBX_TRY(stream_keys_table(c, sk, sum.data() + kFsSummaryWords, st, &d_tab, &writes));

    const bool sets = flags & (kFsHasSet | kFsHasIncr), straddles = flags & kFsStraddles;
    const uint64_t sizes = sum[kFsSizes];
    const int one_size = sizes && !(sizes & (sizes - 1)) ? significant_bits(sizes) : 0;  // 0: several sizes occur
    // sums modulo 2^size commute, and equal-or-disjoint fields keep them apart: not so for mixed sizes
    // (fieldstream_kernels.hip section 3)
    const bool commutes = (flags & (kFsHasGet | kFsHasSet | kFsHasIncr)) == kFsHasIncr && !(flags & (kFsSat | kFsFail)) &&
                          !d_replies && one_size && 64 % one_size == 0 && !(flags & kFsUnaligned);
    const int tuned = g_tune.fieldstream_path;
    int path;
    if (tuned == 0)
        path = !sets ? kFsPathGather
               : commutes ? kFsPathAtomic
               : n <= g_tune.fieldstream_serial_max ? kFsPathSerial
               : straddles ? kFsPathKeys : kFsPathWords;
    else
        path = tuned == 2 && straddles ? kFsPathKeys : tuned;
    g_fieldstream_last_path = path;
    if (path == kFsPathGather) {
        if (d_replies || d_status) launch_fieldstream_gather(d_tab, d_key, d_cmds, n, d_replies, d_status, st);
    } else if (path == kFsPathAtomic) {
        launch_fieldstream_incr_atomic(d_tab, d_key, d_cmds, n, d_status, st);
    } else if (path == kFsPathSerial) {
        launch_fieldstream_serial(d_tab, d_key, d_cmds, n, d_replies, d_status, st);
    } else {
        // consecutive chunks in order; a cell that spans two of them is read again by the second
        const uint64_t chunk = g_tune.fieldstream_chunk;
        const int word_bits = path == kFsPathWords ? std::max(1, significant_bits(sum[kFsMaxWord])) : 0;
        const int key_bits = std::max(1, significant_bits((uint64_t)nkeys - 1));
        RBX_TRY(cell_sort_reserve<unsigned long long>(b.bst_sort, (uint32_t)std::min(n, chunk), 0,
                                                      word_bits + key_bits + (has_failed ? 1 : 0)));
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            const uint32_t m = (uint32_t)std::min(chunk, n - i0);
            RBX_TRY(sort_failed(launch_fieldstream_grouped(d_tab, d_key + i0, d_cmds + i0, m,
                                                           d_replies ? d_replies + i0 : nullptr,
                                                           d_status ? d_status + i0 : nullptr, word_bits, key_bits,
                                                           has_failed, b.bst_sort.p, b.bst_sort.cap, st)));
        }
    }
    if (writes) launch_bitstream_lengths(d_tab, d_keymax, nkeys, st);
    HIP_TRY(hipGetLastError());
    if (has_failed) *failed = first_failed == first[0] ? kFsBadType : (first_failed == first[1] ? kFsBadOffset : kFsWrongType);
    return RBX_OK;
}

static int field_stream_failed(int kind) {
    if (kind == 0) return RBX_OK;
    if (kind == kFsWrongType) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    return fail(RBX_E_REDIS, kind == kFsBadType ? kFieldTypeMsg : kBitOffsetMsg);
}

// ---- many BITOPs / BITCOUNTs of a combination in one call (rbx_bitset_op_groups) ----
static std::atomic<uint32_t> g_bitgroups_last[4];  // rbx_bench_bitgroups_last shows them
static int last_show(const std::atomic<uint32_t> *last, uint32_t *out) {  // what every rbx_bench_*_last does
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    for (int i = 0; i < 4; ++i) out[i] = last[i];
    return RBX_OK;
}
enum { kBgPhases = 0, kBgLaunches = 1, kBgTile = 2, kBgDeviceGroups = 3 };

// The keys of one grouped call, each distinct name resolved once (stream_names_resolve has the rules), with what
// the host carries through the groups: per canonical id the bitmap (null = missing) and its Redis length.  A
// bitmap the call deletes or replaces stays referenced in `retired` to the call's final wait: a launch of an
// earlier phase may still read it.
struct BgKeys {
    std::vector<std::string> nm;
    std::vector<uint32_t> canon;
    std::vector<uint8_t> wrong;
    std::vector<std::shared_ptr<Bitmap>> bm;
    std::vector<uint64_t> len;
    std::vector<std::shared_ptr<Bitmap>> retired;
};

// One phase, the groups [p0, p1) that are not skipped (failed or forwarded): no destination is another group's
// source or destination (bit_groups_plan), so one launch runs them all.  Every length is the host's: L[g] and the
// keys' lengths are carried forward here, destinations are created, grown and deleted, and only the groups with a
// result of some length and something to store or count reach the device.
static int bg_phase(rbx_ctx *c, BgKeys &K, const uint8_t *grp_op, const uint32_t *grp_dest, const uint64_t *grp_off,
                    const uint32_t *grp_key, const uint8_t *skip, uint32_t p0, uint32_t p1, uint64_t *L,
                    unsigned long long *d_counts, hipStream_t st, uint32_t *stats) {
    stats[kBgPhases]++;
    std::vector<BitGroup> recs;
    std::vector<BitopSrc> srcs;
    std::vector<const Bitmap *> src_bm, rec_dst;  // whose pointers the table takes once every allocation is final
    uint64_t total = 0;
    for (uint32_t g = p0; g < p1; ++g) {
        if (skip[g]) continue;
        uint64_t out_len = 0, full = ~0ULL;
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
            const uint32_t k = K.canon[grp_key[i]];
            out_len = std::max(out_len, K.len[k]);
            full = std::min<uint64_t>(full, K.bm[k] ? K.len[k] : 0);
        }
        L[g] = out_len;
        const bool writes = grp_dest[g] != RBX_BITGROUP_NO_DEST;
        const uint32_t d = writes ? K.canon[grp_dest[g]] : 0;
        if (out_len == 0) {  // the empty result: DEL dest; the count is 0
            if (writes) {
                c->ks.erase(K.nm[d]);
                if (K.bm[d]) K.retired.push_back(std::move(K.bm[d]));
                K.bm[d].reset();
                K.len[d] = 0;
            }
            continue;
        }
        if (!writes && !d_counts) continue;  // nothing to store and nothing to count
        BitGroup r{};
        r.count = d_counts ? d_counts + g : nullptr;
        r.out_len = out_len;
        r.full = full & ~15ULL;
        r.op = grp_op[g];
        r.nsrc = (uint32_t)(grp_off[g + 1] - grp_off[g]);
        r.src_off = (uint32_t)srcs.size();
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {  // (the lengths before dest takes its new one)
            const uint32_t k = K.canon[grp_key[i]];
            srcs.push_back(BitopSrc{nullptr, K.len[k]});
            src_bm.push_back(K.bm[k].get());
        }
        r.span = (out_len + 15) & ~15ULL;
        if (writes) {
            uint64_t prev = K.len[d];
            std::shared_ptr<Bitmap> now;
            RBX_TRY(bitset_for_write(c, K.nm[d], out_len, st, &now));
            if (now != K.bm[d]) {  // created (or the key's timeout passed since the names were resolved)
                if (K.bm[d]) K.retired.push_back(std::move(K.bm[d]));
                K.bm[d] = now;
                prev = 0;
            }
            // the sweep also clears what a longer previous dest held past the result
            r.span = std::min<uint64_t>((std::max(out_len, prev) + 15) & ~15ULL, now->cap_bytes);
            K.len[d] = out_len;
            if (Entry *e = c->ks.find(K.nm[d])) e->expire_at = -1;  // setKey without KEEPTTL
        }
        rec_dst.push_back(writes ? K.bm[d].get() : nullptr);
        total += r.span;
        recs.push_back(r);
    }
    if (recs.empty()) return RBX_OK;
    // the table after every dest has its final allocation: a source that is its dest moved with it
    for (size_t j = 0; j < srcs.size(); ++j) srcs[j].bytes = src_bm[j] ? (const uint8_t *)src_bm[j]->d_words : nullptr;
    const uint32_t tuned = g_tune.bitgroups_tile;
    const uint32_t tile = tuned ? tuned : bitgroups_auto_tile(total);
    const size_t n = recs.size();
    std::vector<uint64_t> first(n + 1, 0);
    for (size_t j = 0; j < n; ++j) {
        if (rec_dst[j]) {
            recs[j].dst = (uint8_t *)rec_dst[j]->d_words;
            recs[j].dst_len = rec_dst[j]->d_len;
        }
        first[j + 1] = first[j] + (recs[j].span + tile - 1) / tile;
    }
    // records | first tiles | sources, in one upload (a pageable source is staged by the runtime before the call
    // returns; stream order keeps the previous phase's launch ahead of this overwrite)
    const size_t rec_bytes = n * sizeof(BitGroup), first_bytes = (n + 1) * 8, src_bytes = srcs.size() * sizeof(BitopSrc);
    std::vector<uint8_t> blob(rec_bytes + first_bytes + src_bytes);
    memcpy(blob.data(), recs.data(), rec_bytes);
    memcpy(blob.data() + rec_bytes, first.data(), first_bytes);
    memcpy(blob.data() + rec_bytes + first_bytes, srcs.data(), src_bytes);
    DevBuf &tab = c->dev->bits.grp_table;
    RBX_TRY(tab.reserve(blob.size()));
    HIP_TRY(hipMemcpyAsync(tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    uint8_t *p = tab.as<uint8_t>();
    launch_bitgroups_sweep((const BitGroup *)p, (const uint64_t *)(p + rec_bytes), (uint32_t)n, first[n],
                           (const BitopSrc *)(p + rec_bytes + first_bytes), tile, st);
    HIP_TRY(hipGetLastError());
    stats[kBgLaunches]++;
    stats[kBgTile] = tile;
    stats[kBgDeviceGroups] += (uint32_t)n;
    return RBX_OK;
}

// at least n pinned bytes
static int bg_pin(PinBuf &pin, size_t n) {
    if (pin.cap >= n) return RBX_OK;
    HIP_TRY(pin.alloc(std::max<size_t>(n, 4096), hipHostMallocDefault));
    return RBX_OK;
}

static int bitset_op_groups(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint8_t *grp_op,
                            const uint32_t *grp_dest, const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups,
                            uint64_t *lens, uint64_t *counts, uint8_t *status) {
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    BitsetScratch &b = c->dev->bits;
    BgKeys K;
    K.canon.resize(nkeys);
    K.wrong.assign(nkeys, 0);
    K.bm.resize(nkeys);
    K.len.assign(nkeys, 0);
    stream_names_resolve(c, names, nkeys, KType::Bitmap, &K.nm, K.canon.data(), K.wrong.data(),
                         [&](uint32_t i, const Entry &e) { K.bm[i] = e.bm; });
    // the length words of the existing keys: one gather, one copy back, the call's first wait
    std::vector<const unsigned long long *> ptrs;
    std::vector<uint32_t> at;
    for (uint32_t i = 0; i < nkeys; ++i)
        if (K.bm[i]) {
            ptrs.push_back(K.bm[i]->d_len);
            at.push_back(i);
        }
    if (!ptrs.empty()) {
        const size_t n = ptrs.size();
        RBX_TRY(b.grp_lens.reserve(n * 16));  // pointers | values
        auto *d_out = b.grp_lens.as<unsigned long long>() + n;
        HIP_TRY(hipMemcpyAsync(b.grp_lens.p, ptrs.data(), n * 8, hipMemcpyHostToDevice, st));
        launch_bitgroups_lens(b.grp_lens.as<const unsigned long long *>(), (uint32_t)n, d_out, st);
        HIP_TRY(hipGetLastError());
        RBX_TRY(bg_pin(b.grp_pin, n * 8));
        const unsigned long long *got = b.grp_pin.as<unsigned long long>();
        HIP_TRY(hipMemcpyAsync(b.grp_pin.p, d_out, n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t j = 0; j < n; ++j) K.len[at[j]] = got[j];
    }
    // the groups that fail alone, and the canonical ids the planner reads
    std::vector<uint8_t> failed(ngroups, 0), skip(ngroups, 0);
    std::vector<uint32_t> cdest(ngroups), csrc(grp_off[ngroups]);
    int first_code = RBX_OK;
    for (uint32_t g = 0; g < ngroups; ++g) {
        const bool writes = grp_dest[g] != RBX_BITGROUP_NO_DEST;
        bool wrong = writes && K.wrong[grp_dest[g]] != 0;
        cdest[g] = writes ? K.canon[grp_dest[g]] : kBitGroupNoDest;
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
            wrong = wrong || K.wrong[grp_key[i]] != 0;
            csrc[i] = K.canon[grp_key[i]];
        }
        // (the single call checks NOT's source count before any key's type)
        const bool bad_not = grp_op[g] == RBX_BITOP_NOT && grp_off[g + 1] - grp_off[g] != 1;
        failed[g] = bad_not || wrong;
        if (failed[g] && first_code == RBX_OK) first_code = bad_not ? RBX_E_REDIS : RBX_E_WRONGTYPE;
        if (status) status[g] = failed[g] ? 0xFF : 0;
    }
    std::vector<uint32_t> end, fwd;
    bit_groups_plan(grp_op, cdest.data(), grp_off, csrc.data(), failed.data(), ngroups, nkeys, &end, &fwd);
    for (uint32_t g = 0; g < ngroups; ++g) skip[g] = failed[g] || fwd[g] != kBitGroupRuns;
    unsigned long long *d_counts = nullptr;
    if (counts) {
        RBX_TRY(b.grp_counts.reserve((size_t)ngroups * 8));
        RBX_TRY(bg_pin(b.grp_pin, (size_t)ngroups * 8));
        d_counts = b.grp_counts.as<unsigned long long>();
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)ngroups * 8, st));
    }
    // the largest table a phase can upload, once: growing the buffer between phases would wait for the device
    RBX_TRY(b.grp_table.reserve((size_t)ngroups * (sizeof(BitGroup) + 8) + 8 + (size_t)grp_off[ngroups] * sizeof(BitopSrc)));
    uint32_t stats[4] = {0, 0, 0, 0};
    std::vector<uint64_t> L(ngroups, 0);
    uint32_t p0 = 0;
    for (uint32_t p1 : end) {
        RBX_TRY(bg_phase(c, K, grp_op, grp_dest, grp_off, grp_key, skip.data(), p0, p1, L.data(), d_counts, st, stats));
        p0 = p1;
    }
    if (counts) HIP_TRY(hipMemcpyAsync(b.grp_pin.p, d_counts, (size_t)ngroups * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the call's second wait; K.retired may go
    if (counts) memcpy(counts, b.grp_pin.p, (size_t)ngroups * 8);
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (!failed[g] && fwd[g] != kBitGroupRuns) {  // answered from its writer, an earlier group
            L[g] = L[fwd[g]];
            if (counts) counts[g] = counts[fwd[g]];
        }
        if (lens) lens[g] = L[g];
    }
    for (int i = 0; i < 4; ++i) g_bitgroups_last[i] = stats[i];
    if (first_code == RBX_E_REDIS) return fail(RBX_E_REDIS, kBitopNotMsg);
    if (first_code != RBX_OK) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    return RBX_OK;
}

// ---- the read streams in two tiers: what the range stream and the members stream share ----
enum { kRsShortDone = 0, kRsLongCmds = 1, kRsTiles = 2, kRsWaits = 3 };  // what rbx_bench_*_last show of a call
static std::atomic<uint32_t> g_rangestream_last[4], g_members_last[4];

// One call of a read stream: read_stream_open, then per chunk read_chunk_begin with the stream's group kernel, the
// caller's own copies, read_chunk_end with the chunk's one wait, and the stream's tier-2 work over the listed commands.
struct ReadStream {
    const int nfirst;               // the summary's "first position" words (rbx_kernels.h rs_summary_words)
    const char *const illegal_msg;  // what a command that is the caller's error reports
    const BitKey *d_tab = nullptr;
    unsigned long long *d_sum = nullptr, *d_long = nullptr;
    uint64_t chunk = 0, stats[4] = {0, 0, 0, 0};  // commands per chunk; what rbx_bench_*_last will show
    // the chunk just ended: its first positions (pinned, nfirst words, ~0 = none), listed commands and tiles
    const unsigned long long *firsts = nullptr;
    uint32_t nlong = 0;  // (a chunk has <= 2^30 commands)
    uint64_t tiles = 0;
};

// the names resolved once, the key table built without writes, the chunk capped, the list and summary reserved
static int read_stream_open(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, uint64_t n, uint64_t tuned_chunk,
                            uint32_t tile, hipStream_t st, ReadStream *rs) {
    if (nkeys == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, rs->illegal_msg);
    const int nfirst = rs->nfirst;
    BitsetScratch &b = c->dev->bits;
    StreamKeys sk(c, names, nkeys);
    bool writes;
    RBX_TRY(stream_keys_table(c, sk, nullptr, st, &rs->d_tab, &writes));
    uint64_t max_bytes = 0;
    for (const BitKey &k : b.bst_table.host) max_bytes = std::max(max_bytes, k.cap_bits >> 3);
    // one summary word hands out a chunk's list slots and tile numbers: its tiles stay below 2^kRsTileBits
    rs->chunk = std::min<uint64_t>(tuned_chunk, ((1ULL << kRsTileBits) - 1) / (max_bytes / tile + 2));
    RBX_TRY(b.rs_long.reserve(std::min(n, rs->chunk) * 8));
    RBX_TRY(b.rs_sum.reserve(rs_summary_words(nfirst) * 8));
    rs->d_sum = b.rs_sum.as<unsigned long long>();
    rs->d_long = b.rs_long.as<unsigned long long>();
    return RBX_OK;
}

// the summary words preset, the group kernel through launch(), and the summary's copy to the pinned words
template <class Launch> static int read_chunk_begin(rbx_ctx *c, const ReadStream &rs, hipStream_t st, Launch launch) {
    HIP_TRY(hipMemsetAsync(rs.d_sum, 0xFF, rs.nfirst * 8, st));
    HIP_TRY(hipMemsetAsync(rs.d_sum + rs.nfirst, 0, (rs_summary_words(rs.nfirst) - rs.nfirst) * 8, st));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->dev->stage.words(), rs.d_sum, rs_summary_words(rs.nfirst) * 8, hipMemcpyDeviceToHost, st));
    return RBX_OK;
}

// the chunk's one wait, and what its m commands' summary says
static int read_chunk_end(rbx_ctx *c, ReadStream &rs, uint32_t m, hipStream_t st) {
    HIP_TRY(hipStreamSynchronize(st));
    ++rs.stats[kRsWaits];
    const unsigned long long *w = c->dev->stage.words();
    if (w[rs_flags_at(rs.nfirst)] & kRsIllegal) return fail(RBX_E_ILLEGAL_ARGUMENT, rs.illegal_msg);
    rs.firsts = w;
    rs.nlong = (uint32_t)(w[rs_long_at(rs.nfirst)] >> kRsTileBits);
    rs.tiles = w[rs_long_at(rs.nfirst)] & ((1ULL << kRsTileBits) - 1);
    rs.stats[kRsShortDone] += m - rs.nlong;
    rs.stats[kRsLongCmds] += rs.nlong;
    rs.stats[kRsTiles] += rs.tiles;
    return RBX_OK;
}

static void read_stream_publish(std::atomic<uint32_t> *last, const ReadStream &rs) {  // what last_show shows
    for (int i = 0; i < 4; ++i) last[i] = (uint32_t)std::min<uint64_t>(rs.stats[i], 0xFFFFFFFFu);
}

// ---- BITCOUNT / BITPOS / STRLEN / length() over many keys (rbx_bitset_range_stream) ----
static const char *const kRangeIllegalMsg =
    "a command's key is not below nkeys, its op, unit or nargs is unknown, or a BITCOUNT has a start without an end";

// what a command that failed alone reports (range_cmd.h kRange*), as the single calls do
static int range_cmd_failed(int kind) {
    if (kind == kRangeOk) return RBX_OK;
    if (kind == kRangeWrongType) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    return fail(RBX_E_REDIS, kind == kRangeBadBit   ? "ERR The bit argument must be 1 or 0."
                             : kind == kRangeSyntax ? "ERR syntax error"
                                                    : kBitOffsetMsg);
}

// A batch of n > 0 commands over device arrays inside the caller's scope on `st`; d_replies and d_status
// nullable.  *failed = the failure kind of the first command in array order that failed alone.  Per chunk the
// group kernel, the one wait, and -- when it listed long commands -- the tiles.  replies / status: the host form's
// targets (null for _dev), copied behind the group kernel and again behind the tiles, with a second wait.
static int range_stream_run(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_key,
                            const rbx_range_cmd *d_cmds, uint64_t n, int64_t *d_replies, uint8_t *d_status,
                            int64_t *replies, uint8_t *status, hipStream_t st, int *failed) {
    *failed = kRangeOk;
    const uint32_t tile = g_tune.rangestream_tile, short_max = g_tune.rangestream_short_max;
    const int lanes = g_tune.rangestream_lanes;
    ReadStream rs{kRangeKinds, kRangeIllegalMsg};
    RBX_TRY(read_stream_open(c, names, nkeys, n, g_tune.rangestream_chunk, tile, st, &rs));
    for (uint64_t i0 = 0; i0 < n; i0 += rs.chunk) {
        const uint32_t m = (uint32_t)std::min(rs.chunk, n - i0);
        int64_t *d_r = d_replies ? d_replies + i0 : nullptr;
        uint8_t *d_s = d_status ? d_status + i0 : nullptr;
        RBX_TRY(read_chunk_begin(c, rs, st, [&] {
            launch_rangestream_short(lanes, rs.d_tab, d_key + i0, d_cmds + i0, m, nkeys, short_max, tile, d_r, d_s, rs.d_sum,
                                     rs.d_long, st);
        }));
        if (replies) HIP_TRY(hipMemcpyAsync(replies + i0, d_r, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        if (status) HIP_TRY(hipMemcpyAsync(status + i0, d_s, m, hipMemcpyDeviceToHost, st));
        RBX_TRY(read_chunk_end(c, rs, m, st));
        if (*failed == kRangeOk) {
            uint64_t first = ~0ULL;
            for (int k = 0; k < kRangeKinds; ++k)
                if (rs.firsts[k] < first) first = rs.firsts[k], *failed = k + 1;
        }
        if (rs.nlong == 0 || !d_r) continue;  // (without replies a long command has nothing left to answer)
        launch_rangestream_tiles(rs.d_tab, d_key + i0, d_cmds + i0, tile, rs.d_long, rs.nlong, rs.tiles, d_r, st);
        HIP_TRY(hipGetLastError());
        if (replies) {
            HIP_TRY(hipMemcpyAsync(replies + i0, d_r, (size_t)m * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            ++rs.stats[kRsWaits];
        }
    }
    read_stream_publish(g_rangestream_last, rs);
    return RBX_OK;
}

static int range_stream_args_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, uint64_t n, bool arrays) {
    if (n && !arrays) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return stream_names_check(c, names, nkeys);
}

// ---- the enumeration over many keys (rbx_bitset_members_stream) ----
static const char *const kMembersIllegalMsg = "a command's key is not below nkeys, its nargs is not 0 or 2, or its unit is unknown";

// A batch of n > 0 commands over device arrays inside the caller's scope on `st`: d_off (n + 1 words) always in
// full, d_out (nullable with cap 0: count only) as far as below cap, d_status nullable.  *failed = some command ran
// on a key of another type.  Per chunk the count kernel with its one wait for the summary, the tiles of the listed
// commands, the scan of the chunk's yields in place (k_bits_block_scan) plus the carry -- the chunk before's total,
// kept on the device -- and the two expand kernels.
static int members_stream_run(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_key,
                              const rbx_members_cmd *d_cmds, uint64_t n, uint64_t cap, uint64_t *d_off, uint64_t *d_out,
                              uint8_t *d_status, hipStream_t st, bool *failed) {
    *failed = false;
    const uint32_t tile = g_tune.members_tile, short_max = g_tune.members_short_max;
    const int lanes = g_tune.members_lanes;
    ReadStream rs{kMsFirsts, kMembersIllegalMsg};
    RBX_TRY(read_stream_open(c, names, nkeys, n, g_tune.members_chunk, tile, st, &rs));
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.mem_state.reserve(64));
    auto *d_carry = b.mem_state.as<unsigned long long>() + 3, *off = (unsigned long long *)d_off;
    HIP_TRY(hipMemsetAsync(d_carry, 0, 8, st));
    for (uint64_t i0 = 0; i0 < n; i0 += rs.chunk) {
        const uint32_t m = (uint32_t)std::min(rs.chunk, n - i0);
        RBX_TRY(read_chunk_begin(c, rs, st, [&] {
            launch_members_count(lanes, rs.d_tab, d_key + i0, d_cmds + i0, m, nkeys, short_max, tile, off + i0,
                                 d_status ? d_status + i0 : nullptr, rs.d_sum, rs.d_long, st);
        }));
        RBX_TRY(read_chunk_end(c, rs, m, st));
        if (rs.firsts[0] != ~0ULL) *failed = true;
        if (rs.nlong) {
            RBX_TRY(b.mem_tiles.reserve(rs.tiles * 8));
            launch_members_tiles_count(rs.d_tab, d_key + i0, d_cmds + i0, tile, rs.d_long, rs.nlong, rs.tiles,
                                       b.mem_tiles.as<unsigned long long>(), off + i0, st);
        }
        launch_bits_scan(off + i0, m, st);  // off[i0 + m] = the chunk's total
        launch_members_carry(off + i0, (uint64_t)m + 1, d_carry, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(d_carry, off + i0 + m, 8, hipMemcpyDeviceToDevice, st));  // the next chunk overwrites that word
        if (d_out && cap) {
            launch_members_expand_short(lanes, rs.d_tab, d_key + i0, d_cmds + i0, m, short_max, off + i0, d_out, cap, st);
            if (rs.nlong)
                launch_members_expand_tiles(rs.d_tab, d_key + i0, d_cmds + i0, tile, rs.d_long, rs.nlong, rs.tiles,
                                            b.mem_tiles.as<unsigned long long>(), off + i0, d_out, cap, st);
            HIP_TRY(hipGetLastError());
        }
    }
    read_stream_publish(g_members_last, rs);
    return RBX_OK;
}


static int members_stream_args_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, uint64_t n, uint64_t cap,
                                     const void *key, const void *cmds, const void *off, const void *out) {
    if ((n && (!key || !cmds)) || !off || (cap && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n > (1ULL << 32)) return fail(RBX_E_ILLEGAL_ARGUMENT, "a batch takes at most 2^32 commands");
    return stream_names_check(c, names, nkeys);
}

// ---- GETRANGE / SETRANGE / APPEND / GET over many keys (rbx_string_stream) ----
enum { kBlShortDone = 0, kBlLongCmds = 1, kBlTiles = 2, kBlRounds = 3 };  // what rbx_bench_bytestream_last shows
static std::atomic<uint32_t> g_bytestream_last[4];
static const char *const kStringIllegalMsg =
    "a command's key is not below nkeys, its op is unknown, or its value leaves the value buffer";

// The key table over the strings as the plan left them: every canonical key a command that ran writes is created or
// grown to its planned final length, the others are looked up.  When a creation or a growth fails (memory), the keys
// this call created so far are removed again: the call ran nothing, and leaves no empty string behind.
static int string_keys_table(rbx_ctx *c, StreamKeys &sk, const ByteKeyState *state, hipStream_t st, const BitKey **d_tab) {
    const uint32_t *canon = sk.canon();
    const uint8_t *wrong = sk.wrong();
    std::vector<BitKey> tab(sk.nkeys);
    std::vector<uint32_t> created;
    int rc = RBX_OK;
    for (uint32_t i = 0; i < sk.nkeys && rc == RBX_OK; ++i) {
        BitKey &k = tab[i];
        if (canon[i] != i) {
            k = tab[canon[i]];
            continue;
        }
        k = BitKey{nullptr, 0, nullptr, wrong[i] ? kBitKeyWrong : 0u, i};
        if (wrong[i]) continue;
        std::shared_ptr<Bitmap> bm;
        if (state[i].flags & kByWritten) {
            const bool was_missing = c->ks.find(sk.nm[i]) == nullptr;
            rc = bitset_for_write(c, sk.nm[i], state[i].len, st, &bm);
            if (rc == RBX_OK && was_missing) created.push_back(i);
        } else {
            rc = bitset_find(c, sk.nm[i], &bm);
        }
        if (rc == RBX_OK && bm) k = BitKey{bm->d_words, bm->cap_bytes * 8, bm->d_len, 0u, i};
    }
    if (rc != RBX_OK) {
        for (uint32_t i : created) c->ks.erase(sk.nm[i]);
        return rc;
    }
    *d_tab = c->dev->bits.bst_table.sync(tab, st);
    return *d_tab ? RBX_OK : c->dev->bits.bst_table.err;
}

// A batch of n > 0 commands over device arrays inside the caller's scope on `st`; d_replies and d_status nullable.
// d_off (n + 1 words) is always written in full.  The reads go to d_out, or -- the host form, which cannot size its
// buffer before the plan -- to out_buf, reserved for the total.  *failed = the failure kind of the first command in
// array order that failed alone; *total_out = off[n]; *over = the reads exceed cap and nothing ran.  Three steps:
// the plan of every chunk (one wait each; nothing is written), the host's decisions (the caller's errors, total
// against cap, every written key created or grown once, the table), then per chunk the rounds, and the lengths.
static int string_stream_run(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_key,
                             const rbx_string_cmd *d_cmds, uint64_t n, const uint8_t *d_vals, uint64_t vals_len, uint64_t cap,
                             unsigned long long *d_off, uint8_t *d_out, DevBuf *out_buf, int64_t *d_replies,
                             uint8_t *d_status, hipStream_t st, int *failed, uint64_t *total_out, bool *over) {
    *failed = kByteOk;
    *over = false;
    if (nkeys == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, kStringIllegalMsg);
    const uint32_t tile = g_tune.bytestream_tile, short_max = g_tune.bytestream_short_max;
    const int lanes = g_tune.bytestream_lanes;
    // one list word hands out a round's list slots and tile numbers: its tiles stay below 2^kRsTileBits
    const uint64_t chunk = std::min<uint64_t>(g_tune.bytestream_chunk, ((1ULL << kRsTileBits) - 1) / (kStrMax / tile + 2));
    const bool tiny = n <= g_tune.bytestream_serial_max && n <= chunk;
    const uint32_t cmax = (uint32_t)std::min(n, chunk);
    const int key_bits = significant_bits(nkeys);  // cell nkeys: a command that is the caller's error
    BitsetScratch &b = c->dev->bits;
    StreamKeys sk(c, names, nkeys);
    const BitKey *d_tab;
    bool writes;
    RBX_TRY(stream_keys_table(c, sk, nullptr, st, &d_tab, &writes));
    RBX_TRY(b.by_state.reserve((size_t)nkeys * sizeof(ByteKeyState)));
    RBX_TRY(b.by_plan.reserve(n * 8));
    RBX_TRY(b.by_sum.reserve((kBySummaryWords + 1) * 8));  // and the offsets' carry
    RBX_TRY(b.by_runs.reserve((size_t)cmax * 8));  // cursors | heads
    RBX_TRY(b.by_long.reserve((size_t)cmax * 8));
    if (!tiny) RBX_TRY(cell_sort_reserve<uint32_t>(b.bst_sort, cmax, 0, key_bits));
    const size_t pin_bytes = (size_t)nkeys * sizeof(ByteKeyState) + (kBySummaryWords + 1) * 8;
    RBX_TRY(bg_pin(b.by_pin, pin_bytes));
    auto *d_state = b.by_state.as<ByteKeyState>();
    auto *d_plan = b.by_plan.as<unsigned long long>(), *d_sum = b.by_sum.as<unsigned long long>();
    auto *h_sum = b.by_pin.as<unsigned long long>();  // summary words | total | states
    auto *h_state = (ByteKeyState *)(h_sum + kBySummaryWords + 1);
    auto *d_carry = d_sum + kBySummaryWords;  // the yield of the chunks before: the next plan overwrites d_off[i0]
    HIP_TRY(hipMemsetAsync(d_carry, 0, 8, st));
    launch_bytestream_state_init(d_tab, nkeys, d_state, st);

    // 1. the plan, chunk by chunk; the running states and the offsets carry across the chunks on the device
    std::vector<uint32_t> rounds;
    uint64_t first[kByteKinds] = {~0ULL, ~0ULL, ~0ULL}, stats[4] = {0, 0, 0, 0};
    bool illegal = false;
    for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - i0);
        HIP_TRY(hipMemsetAsync(d_sum, 0xFF, kByteKinds * 8, st));
        HIP_TRY(hipMemsetAsync(d_sum + kByteKinds, 0, (kBySummaryWords - kByteKinds) * 8, st));
        int64_t *d_r = d_replies ? d_replies + i0 : nullptr;
        uint8_t *d_s = d_status ? d_status + i0 : nullptr;
        if (tiny) {
            launch_bytestream_plan_serial(d_tab, d_key, d_cmds, m, nkeys, vals_len, short_max, tile, d_state, d_plan, d_off,
                                          d_r, d_s, d_sum, st);
        } else {
            RBX_TRY(sort_failed(launch_bytestream_sort(d_tab, d_key + i0, d_cmds + i0, m, nkeys, vals_len, key_bits, d_sum,
                                                       b.bst_sort.p, b.bst_sort.cap, st)));
            RBX_TRY(sort_failed(launch_bytestream_plan(d_tab, d_cmds + i0, m, nkeys, i0, short_max, tile, d_state,
                                                       d_plan + i0, d_off + i0, d_r, d_s, d_sum, b.bst_sort.p,
                                                       b.bst_sort.cap, st)));
        }
        launch_bits_scan(d_off + i0, m, st);  // d_off[i0 + m] = the chunk's yield
        if (i0) launch_members_carry(d_off + i0, (uint64_t)m + 1, d_carry, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(d_carry, d_off + i0 + m, 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(h_sum, d_sum, kBySummaryWords * 8, hipMemcpyDeviceToHost, st));
        if (i0 + m == n) {  // the last chunk's wait also brings the total and the keys' final states
            HIP_TRY(hipMemcpyAsync(h_sum + kBySummaryWords, d_off + n, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_state, d_state, (size_t)nkeys * sizeof(ByteKeyState), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));  // the chunk's one wait
        illegal = illegal || (h_sum[kByFlags] & kRsIllegal);
        for (int k = 0; k < kByteKinds; ++k) first[k] = std::min<uint64_t>(first[k], h_sum[k]);
        rounds.push_back(1 + (uint32_t)h_sum[kByMostLong]);
        stats[kBlLongCmds] += h_sum[kByLongCmds];
        stats[kBlTiles] += h_sum[kByTiles];
    }
    // 2. the host's decisions
    if (illegal) return fail(RBX_E_ILLEGAL_ARGUMENT, kStringIllegalMsg);
    const uint64_t total = h_sum[kBySummaryWords];
    *total_out = total;
    if (total > cap) {
        *over = true;
        return fail(RBX_E_ILLEGAL_ARGUMENT, "the reads yield more bytes than cap: off and total are exact, nothing ran");
    }
    if (out_buf && total) {
        RBX_TRY(out_buf->reserve(total));
        d_out = out_buf->as<uint8_t>();
    }
    std::vector<ByteKeyState> state(h_state, h_state + nkeys);  // (bitset_for_write may wait: the pinned words are reused)
    RBX_TRY(string_keys_table(c, sk, state.data(), st, &d_tab));
    // 3. the rounds of every chunk, then the lengths
    auto *d_cur = b.by_runs.as<uint32_t>(), *d_heads = d_cur + cmax;
    auto *d_long = b.by_long.as<unsigned long long>();
    if (tiny && stats[kBlLongCmds] == 0) {
        launch_bytestream_walk_serial(lanes, d_tab, d_key, d_cmds, d_vals, d_plan, d_off, d_out, (uint32_t)n, st);
        stats[kBlRounds] = 1;
    } else {
        RBX_TRY(cell_sort_reserve<uint32_t>(b.bst_sort, cmax, 0, key_bits));
        size_t ci = 0;
        for (uint64_t i0 = 0; i0 < n; i0 += chunk, ++ci) {
            const uint32_t m = (uint32_t)std::min(chunk, n - i0);
            if (tiny || n > chunk)  // the scratch holds another chunk's pairs, or none
                RBX_TRY(sort_failed(launch_bytestream_sort(d_tab, d_key + i0, d_cmds + i0, m, nkeys, vals_len, key_bits, d_sum,
                                                           b.bst_sort.p, b.bst_sort.cap, st)));
            HIP_TRY(hipMemsetAsync(d_sum + kByHeads, 0, 8, st));
            RBX_TRY(sort_failed(launch_bytestream_heads(m, nkeys, d_cur, d_heads, d_sum + kByHeads, b.bst_sort.p,
                                                        b.bst_sort.cap, st)));
            for (uint32_t r = 0; r < rounds[ci]; ++r) {
                HIP_TRY(hipMemsetAsync(d_sum + kByList, 0, 8, st));
                RBX_TRY(sort_failed(launch_bytestream_walk(lanes, d_tab, d_cmds + i0, d_vals, d_plan + i0, d_off + i0, d_out, m,
                                                           d_cur, d_heads, d_sum + kByHeads, tile, d_sum + kByList, d_long,
                                                           b.bst_sort.p, b.bst_sort.cap, st)));
                if (r + 1 < rounds[ci])  // (the last round walks what lies behind every key's last long command)
                    launch_bytestream_tiles(d_tab, d_key + i0, d_cmds + i0, d_vals, d_plan + i0, d_off + i0, d_out, tile,
                                            d_sum + kByList, d_long, st);
            }
            stats[kBlRounds] += rounds[ci];
        }
    }
    launch_bytestream_lengths(d_tab, d_state, nkeys, st);
    HIP_TRY(hipGetLastError());
    stats[kBlShortDone] = n - stats[kBlLongCmds];
    for (int i = 0; i < 4; ++i) g_bytestream_last[i] = (uint32_t)std::min<uint64_t>(stats[i], 0xFFFFFFFFu);
    uint64_t at = ~0ULL;
    for (int k = 0; k < kByteKinds; ++k)
        if (first[k] < at) at = first[k], *failed = k + 1;
    return RBX_OK;
}

static int string_stream_args_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, uint64_t n, const void *key,
                                    const void *cmds, const void *vals, uint64_t vals_len, const void *off, const void *out,
                                    uint64_t cap) {
    if ((n && (!key || !cmds)) || !off || (vals_len && !vals) || (cap && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n > (1ULL << 32)) return fail(RBX_E_ILLEGAL_ARGUMENT, "a batch takes at most 2^32 commands");
    return stream_names_check(c, names, nkeys);
}

}  // namespace rbx

using namespace rbx;

extern "C" {

int rbx_bench_fieldstream_last_path(void) { return g_fieldstream_last_path; }

int rbx_bitset_stream_dev(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                          const uint8_t *d_cmd_op, const uint64_t *d_cmd_index, uint64_t n, uint8_t *d_replies,
                          void *stream) {
    RBX_TRY(stream_args_check(c, names, nkeys, n, d_cmd_key && d_cmd_op && d_cmd_index));
    if (n == 0) return RBX_OK;  // no command is sent
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    int failed;
    RBX_TRY(stream_run(c, names, nkeys, d_cmd_key, d_cmd_op, d_cmd_index, n, d_replies, st, &failed));
    return stream_failed(failed);
}

int rbx_bitset_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key, const uint8_t *cmd_op,
                      const uint64_t *cmd_index, uint64_t n, uint8_t *replies) {
    RBX_TRY(stream_args_check(c, names, nkeys, n, cmd_key && cmd_op && cmd_index));
    if (n == 0) return RBX_OK;
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.bst_cmds.reserve(n * 5));  // keys | ops
    RBX_TRY(b.idx.reserve(n * 8));
    if (replies) RBX_TRY(c->dev->stage.out_bytes.reserve(n));
    uint32_t *d_key = b.bst_cmds.as<uint32_t>();
    uint8_t *d_op = b.bst_cmds.as<uint8_t>() + n * 4, *d_replies = replies ? c->dev->stage.out_bytes.as<uint8_t>() : nullptr;
    HIP_TRY(hipMemcpyAsync(d_key, cmd_key, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_op, cmd_op, n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.idx.p, cmd_index, n * 8, hipMemcpyHostToDevice, st));
    int failed;
    RBX_TRY(stream_run(c, names, nkeys, d_key, d_op, b.idx.as<uint64_t>(), n, d_replies, st, &failed));
    if (replies) HIP_TRY(hipMemcpyAsync(replies, d_replies, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return stream_failed(failed);
}

int rbx_bitset_field_stream_dev(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                                const rbx_field_cmd *d_cmds, uint64_t n, int64_t *d_replies, uint8_t *d_status,
                                void *stream) {
    RBX_TRY(stream_args_check(c, names, nkeys, n, d_cmd_key && d_cmds));
    if (n == 0) return RBX_OK;  // no command is sent
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    int failed;
    RBX_TRY(field_stream_run(c, names, nkeys, d_cmd_key, d_cmds, n, d_replies, d_status, st, &failed));
    return field_stream_failed(failed);
}

int rbx_bitset_field_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                            const rbx_field_cmd *cmds, uint64_t n, int64_t *replies, uint8_t *status) {
    RBX_TRY(stream_args_check(c, names, nkeys, n, cmd_key && cmds));
    if (n == 0) return RBX_OK;
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.fst_cmds.reserve(n * (sizeof(rbx_field_cmd) + 4)));  // commands | keys
    if (replies) RBX_TRY(b.fld_out.reserve(n * 8));
    if (status) RBX_TRY(b.fld_nil.reserve(n));
    rbx_field_cmd *d_cmds = b.fst_cmds.as<rbx_field_cmd>();
    uint32_t *d_key = (uint32_t *)(d_cmds + n);
    int64_t *d_replies = replies ? b.fld_out.as<int64_t>() : nullptr;
    uint8_t *d_status = status ? b.fld_nil.as<uint8_t>() : nullptr;
    HIP_TRY(hipMemcpyAsync(d_cmds, cmds, n * sizeof(rbx_field_cmd), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_key, cmd_key, n * 4, hipMemcpyHostToDevice, st));
    int failed;
    RBX_TRY(field_stream_run(c, names, nkeys, d_key, d_cmds, n, d_replies, d_status, st, &failed));
    if (replies) HIP_TRY(hipMemcpyAsync(replies, d_replies, n * 8, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return field_stream_failed(failed);
}

int rbx_bitset_op_groups(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint8_t *grp_op, const uint32_t *grp_dest,
                         const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups, uint64_t *lens,
                         uint64_t *counts, uint8_t *status) {
    RBX_TRY(stream_names_check(c, names, nkeys));
    if (const char *what = hll_groups_check(grp_off, grp_key, ngroups, nkeys, true))
        return fail(RBX_E_ILLEGAL_ARGUMENT, what);
    if (ngroups == 0) return RBX_OK;  // no command is sent
    if (!grp_op || !grp_dest) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (grp_op[g] > RBX_BITOP_NOT) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown BITOP operation");
        if (grp_dest[g] >= nkeys && grp_dest[g] != RBX_BITGROUP_NO_DEST)
            return fail(RBX_E_ILLEGAL_ARGUMENT, "a group's destination is not below nkeys");
    }
    return bitset_op_groups(c, names, nkeys, grp_op, grp_dest, grp_off, grp_key, ngroups, lens, counts, status);
}

int rbx_bench_bitgroups_last(uint32_t out[4]) { return last_show(g_bitgroups_last, out); }

int rbx_bitset_range_stream_dev(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                                const rbx_range_cmd *d_cmds, uint64_t n, int64_t *d_replies, uint8_t *d_status,
                                void *stream) {
    RBX_TRY(range_stream_args_check(c, names, nkeys, n, d_cmd_key && d_cmds));
    if (n == 0) return RBX_OK;  // no command is sent
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    int failed;
    RBX_TRY(range_stream_run(c, names, nkeys, d_cmd_key, d_cmds, n, d_replies, d_status, nullptr, nullptr, st, &failed));
    return range_cmd_failed(failed);
}

int rbx_bitset_range_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                            const rbx_range_cmd *cmds, uint64_t n, int64_t *replies, uint8_t *status) {
    RBX_TRY(range_stream_args_check(c, names, nkeys, n, cmd_key && cmds));
    if (n == 0) return RBX_OK;
    for (uint64_t i = 0; i < n; ++i)  // the caller's errors, before any device work
        if (cmd_key[i] >= nkeys || range_cmd_illegal(cmds[i])) return fail(RBX_E_ILLEGAL_ARGUMENT, kRangeIllegalMsg);
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.rs_cmds.reserve(n * (sizeof(rbx_range_cmd) + 4)));  // commands | keys
    if (replies) RBX_TRY(b.rs_out.reserve(n * 8));
    if (status) RBX_TRY(b.rs_status.reserve(n));
    rbx_range_cmd *d_cmds = b.rs_cmds.as<rbx_range_cmd>();
    uint32_t *d_key = (uint32_t *)(d_cmds + n);
    HIP_TRY(hipMemcpyAsync(d_cmds, cmds, n * sizeof(rbx_range_cmd), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_key, cmd_key, n * 4, hipMemcpyHostToDevice, st));
    int failed;
    RBX_TRY(range_stream_run(c, names, nkeys, d_key, d_cmds, n, replies ? b.rs_out.as<int64_t>() : nullptr,
                             status ? b.rs_status.as<uint8_t>() : nullptr, replies, status, st, &failed));
    return range_cmd_failed(failed);
}

int rbx_bitset_range_of(const uint8_t *bytes, uint64_t len, int missing, const rbx_range_cmd *cmd, int64_t *reply) {
    if ((len && !bytes) || !cmd || !reply) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (range_cmd_illegal(*cmd)) return fail(RBX_E_ILLEGAL_ARGUMENT, kRangeIllegalMsg);
    *reply = 0;
    if (const int kind = range_cmd_fails(*cmd)) return range_cmd_failed(kind);
    if (missing) len = 0;
    if (cmd->op == RBX_RANGE_LENGTH)
        return bitset_length_rule(len, len ? bytes[0] : 0, len ? bytes[len - 1] : 0, reply) ? RBX_OK : range_cmd_failed(kRangeScript);
    uint64_t lo, hi;
    if (!range_cmd_plan(*cmd, len, missing != 0, &lo, &hi, reply)) return RBX_OK;
    const bool pos = cmd->op == RBX_RANGE_POS;
    uint64_t ones = 0, found = kBitsNone;
    for (uint64_t p = lo; p <= hi && found == kBitsNone; ++p) {
        const int bit = (bytes[p >> 3] >> (7 - (p & 7))) & 1;
        ones += bit;
        if (pos && bit == cmd->bit) found = p;
    }
    *reply = pos ? range_cmd_pos_reply(*cmd, found, hi) : (int64_t)ones;
    return RBX_OK;
}

int rbx_bench_rangestream_last(uint32_t out[4]) { return last_show(g_rangestream_last, out); }

int rbx_bitset_members_stream_dev(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                                  const rbx_members_cmd *d_cmds, uint64_t n, uint64_t cap, uint64_t *d_off, uint64_t *d_out,
                                  uint8_t *d_status, void *stream) {
    RBX_TRY(members_stream_args_check(c, names, nkeys, n, cap, d_cmd_key, d_cmds, d_off, d_out));
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    if (n == 0) {  // no command is sent
        HIP_TRY(hipMemsetAsync(d_off, 0, 8, st));
        return RBX_OK;
    }
    bool failed;
    RBX_TRY(members_stream_run(c, names, nkeys, d_cmd_key, d_cmds, n, cap, d_off, d_out, d_status, st, &failed));
    return failed ? fail(RBX_E_WRONGTYPE, kWrongTypeMsg) : RBX_OK;
}

int rbx_bitset_members_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                              const rbx_members_cmd *cmds, uint64_t n, uint64_t cap, uint64_t *off, uint64_t *out,
                              uint8_t *status, uint64_t *total) {
    if (!total) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(members_stream_args_check(c, names, nkeys, n, cap, cmd_key, cmds, off, out));
    *total = off[0] = 0;
    if (n == 0) return RBX_OK;
    for (uint64_t i = 0; i < n; ++i)  // the caller's errors, before any device work
        if (cmd_key[i] >= nkeys || members_cmd_illegal(cmds[i].nargs, cmds[i].unit))
            return fail(RBX_E_ILLEGAL_ARGUMENT, kMembersIllegalMsg);
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.rs_cmds.reserve(n * (sizeof(rbx_members_cmd) + 4)));  // commands | keys
    RBX_TRY(b.rs_out.reserve((n + 1) * 8));
    if (status) RBX_TRY(b.rs_status.reserve(n));
    rbx_members_cmd *d_cmds = b.rs_cmds.as<rbx_members_cmd>();
    uint32_t *d_key = (uint32_t *)(d_cmds + n);
    uint64_t *d_off = b.rs_out.as<uint64_t>();
    uint8_t *d_status = status ? b.rs_status.as<uint8_t>() : nullptr;
    HIP_TRY(hipMemcpyAsync(d_cmds, cmds, n * sizeof(rbx_members_cmd), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_key, cmd_key, n * 4, hipMemcpyHostToDevice, st));
    // The output's size is known only with the offsets: a counting run, then -- when there is anything to write --
    // the same run again with the positions' buffer.  (The device form, whose caller owns the buffer, runs once.)
    bool failed;
    RBX_TRY(members_stream_run(c, names, nkeys, d_key, d_cmds, n, 0, d_off, nullptr, d_status, st, &failed));
    HIP_TRY(hipMemcpyAsync(off, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *total = off[n];
    const uint64_t wr = std::min(*total, cap);
    if (wr) {
        RBX_TRY(b.mem_buf.reserve(wr * 8));
        RBX_TRY(members_stream_run(c, names, nkeys, d_key, d_cmds, n, wr, d_off, b.mem_buf.as<uint64_t>(), nullptr, st, &failed));
        HIP_TRY(hipMemcpyAsync(out, b.mem_buf.p, wr * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return failed ? fail(RBX_E_WRONGTYPE, kWrongTypeMsg) : RBX_OK;
}

int rbx_bench_members_last(uint32_t out[4]) { return last_show(g_members_last, out); }

int rbx_string_stream_dev(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *d_cmd_key,
                          const rbx_string_cmd *d_cmds, uint64_t n, const uint8_t *d_vals, uint64_t vals_len, uint64_t cap,
                          uint64_t *d_off, uint8_t *d_out, int64_t *d_replies, uint8_t *d_status, uint64_t *total,
                          void *stream) {
    RBX_TRY(string_stream_args_check(c, names, nkeys, n, d_cmd_key, d_cmds, d_vals, vals_len, d_off, d_out, cap));
    if (total) *total = 0;
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    if (n == 0) {  // no command is sent
        HIP_TRY(hipMemsetAsync(d_off, 0, 8, st));
        return RBX_OK;
    }
    int failed;
    uint64_t tot = 0;
    bool over;
    const int rc = string_stream_run(c, names, nkeys, d_cmd_key, d_cmds, n, d_vals, vals_len, cap, (unsigned long long *)d_off,
                                     d_out, nullptr, d_replies, d_status, st, &failed, &tot, &over);
    if (total) *total = tot;
    RBX_TRY(rc);
    return byte_cmd_failed(failed);
}

int rbx_string_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key, const rbx_string_cmd *cmds,
                      uint64_t n, const uint8_t *vals, uint64_t vals_len, uint64_t cap, uint64_t *off, uint8_t *out,
                      int64_t *replies, uint8_t *status, uint64_t *total) {
    RBX_TRY(string_stream_args_check(c, names, nkeys, n, cmd_key, cmds, vals, vals_len, off, out, cap));
    if (total) *total = 0;
    off[0] = 0;
    if (n == 0) return RBX_OK;
    for (uint64_t i = 0; i < n; ++i)  // the caller's errors, before any device work
        if (cmd_key[i] >= nkeys || byte_cmd_illegal(cmds[i], vals_len)) return fail(RBX_E_ILLEGAL_ARGUMENT, kStringIllegalMsg);
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.by_cmds.reserve(n * (sizeof(rbx_string_cmd) + 4)));  // commands | keys
    RBX_TRY(b.by_vals.reserve(vals_len));
    RBX_TRY(b.by_off.reserve((n + 1) * 8));
    RBX_TRY(b.by_replies.reserve(n * 9));  // replies | status
    rbx_string_cmd *d_cmds = b.by_cmds.as<rbx_string_cmd>();
    uint32_t *d_key = (uint32_t *)(d_cmds + n);
    auto *d_off = b.by_off.as<unsigned long long>();
    int64_t *d_replies = b.by_replies.as<int64_t>();
    uint8_t *d_status = (uint8_t *)(d_replies + n);
    HIP_TRY(hipMemcpyAsync(d_cmds, cmds, n * sizeof(rbx_string_cmd), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_key, cmd_key, n * 4, hipMemcpyHostToDevice, st));
    if (vals_len) HIP_TRY(hipMemcpyAsync(b.by_vals.p, vals, vals_len, hipMemcpyHostToDevice, st));
    int failed;
    uint64_t tot = 0;
    bool over;
    const int rc = string_stream_run(c, names, nkeys, d_key, d_cmds, n, b.by_vals.as<uint8_t>(), vals_len, cap, d_off, nullptr,
                                     &b.by_out, replies ? d_replies : nullptr, status ? d_status : nullptr, st, &failed, &tot,
                                     &over);
    if (total) *total = tot;
    if (rc != RBX_OK && !over) return rc;
    HIP_TRY(hipMemcpyAsync(off, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (rc == RBX_OK) {
        if (tot) HIP_TRY(hipMemcpyAsync(out, b.by_out.p, tot, hipMemcpyDeviceToHost, st));
        if (replies) HIP_TRY(hipMemcpyAsync(replies, d_replies, n * 8, hipMemcpyDeviceToHost, st));
        if (status) HIP_TRY(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return rc != RBX_OK ? rc : byte_cmd_failed(failed);
}

int rbx_bench_bytestream_last(uint32_t out[4]) { return last_show(g_bytestream_last, out); }

}  // extern "C"
