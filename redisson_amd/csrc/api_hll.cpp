// api_hll.cpp -- HyperLogLog: the register pool, PFADD / PFCOUNT / PFMERGE with Redis' sparse and dense
// encodings, export / import, handles, register packing, the RCCL merge, copies between contexts.
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "api_staging.h"
#include "hll_groups_plan.h"
#include "tunables.h"

namespace rbx {

rbx::HllState::~HllState() {
    if (d_regs && owner) {
        {
            std::lock_guard<std::recursive_mutex> g(owner->ks.mu);
            if (!owner->shut) owner->dev->hll.dirty.push_back({d_regs, d_promoted, d_slot_ops});
        }
        if (d_big_ops) (void)hipFree(d_big_ops);  // its own allocation: released also after a shutdown
        ctx_release(owner);
    }
}

// room for `nops` opcodes in h's list (the caller then overwrites the list)
static int hll_ops_reserve(HllState *h, uint64_t nops) {
    if (nops <= kHllSlotOps || h->d_big_ops) {
        if (nops > kHllMaxOps) return fail(RBX_E_WRONGTYPE, "a sparse HLL string holds at most 16384 opcodes");
        if (h->d_big_ops) h->d_sp_ops = h->d_big_ops;
        return RBX_OK;
    }
    if (nops > kHllMaxOps) return fail(RBX_E_WRONGTYPE, "a sparse HLL string holds at most 16384 opcodes");
    HIP_TRY(hipMalloc(&h->d_big_ops, kHllMaxOps * 2));
    h->d_sp_ops = h->d_big_ops;
    return RBX_OK;
}

// A fresh zeroed HLL register block; the fill runs on `st` (see SlabPool).
static int hll_alloc(rbx_ctx *c, hipStream_t st, std::shared_ptr<HllState> *out) {
    HllPool &hp = c->dev->hll;
    if (hp.avail.empty() && !hp.dirty.empty()) {
        // the deleted HLLs' slots, zeroed in one launch on the caller's stream (creating 10k HLLs
        // cost 20k small fills, ~10 ms of enqueueing, when each slot was zeroed on its own)
        const size_t n = hp.dirty.size();
        std::vector<void *> ptrs(2 * n);
        for (size_t i = 0; i < n; ++i) {
            ptrs[i] = hp.dirty[i].regs;
            ptrs[n + i] = hp.dirty[i].state;
        }
        RBX_TRY(hp.zero_ptrs.reserve(ptrs.size() * sizeof(void *)));
        HIP_TRY(hipMemcpyAsync(hp.zero_ptrs.p, ptrs.data(), ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, st));
        uint8_t *const *d_regs = hp.zero_ptrs.as<uint8_t *>();
        launch_hll_zero(d_regs, (uint32_t *const *)(d_regs + n), (uint32_t)n, st);
        HIP_TRY(hipGetLastError());
        // handed out last-deleted first, as before
        hp.avail.insert(hp.avail.end(), hp.dirty.begin(), hp.dirty.end());
        hp.dirty.clear();
    }
    if (hp.avail.empty()) {
        // registers of kHllPerChunk HLLs, then their state words, then their sparse opcode lists
        uint8_t *chunk = nullptr;
        HIP_TRY(hipMalloc(&chunk, (kHllBytes + kHllStateWords * 4 + kHllOpsBytes) * kHllPerChunk));
        hp.chunks.push_back(chunk);
        uint32_t *words = (uint32_t *)(chunk + kHllBytes * kHllPerChunk);
        uint16_t *ops = (uint16_t *)(words + kHllStateWords * kHllPerChunk);
        // registers and state words of the whole chunk zeroed at once: creating 10k HLLs cost
        // 20k small fills (~10 ms of enqueueing) when each slot was zeroed on its own
        HIP_TRY(hipMemsetAsync(chunk, 0, (kHllBytes + kHllStateWords * 4) * kHllPerChunk, st));
        // hand out in reverse so that successive allocations are ascending
        for (size_t i = kHllPerChunk; i-- > 0;)
            hp.avail.push_back({chunk + i * kHllBytes, words + i * kHllStateWords, ops + i * (kHllOpsBytes / 2)});
    }
    auto h = std::make_shared<HllState>();
    const auto slot = hp.avail.back();
    h->d_regs = slot.regs;
    h->d_promoted = slot.state;
    h->d_sp_ops = h->d_slot_ops = slot.ops;
    hp.avail.pop_back();
    h->owner = c;
    c->refs.fetch_add(1);
    // every slot in hll_free is zero: registers 0, state 0 (not promoted, the createHLLObject
    // sparse string: one XZERO)
    *out = h;
    return RBX_OK;
}

// ---- HyperLogLog ------------------------------------------------------------------------------
static constexpr uint64_t kTileElems = 65536;  // elements per PFADD workgroup
constexpr uint64_t kHllSparseMaxBytes = 3000;  // redis.conf hll-sparse-max-bytes (default)

static const char *kHllWrongType = "WRONGTYPE Key is not a valid HyperLogLog string value.";

// The HLL under `name`; with create, PFADD's createHLLObject (registers zero-filled on `st`).
static int hll_get(rbx_ctx *c, const std::string &name, bool create, hipStream_t st, std::shared_ptr<HllState> *out,
                   bool *created) {
    if (created) *created = false;
    Entry *e = c->ks.find(name);
    if (e) {
        if (e->type != KType::Hll) return fail(RBX_E_WRONGTYPE, kHllWrongType);
        *out = e->hll;
        return RBX_OK;
    }
    if (!create) {
        out->reset();
        return RBX_OK;
    }
    std::shared_ptr<HllState> h;
    RBX_TRY(hll_alloc(c, st, &h));
    h->card = 0;  // createHLLObject: cached cardinality 0, valid
    c->ks.put(name, Entry{KType::Hll, nullptr, nullptr, h});
    c->ks.generation++;
    *out = h;
    if (created) *created = true;
    return RBX_OK;
}

// HLL handles follow the name too; PFADD on a missing key creates it (createHLLObject), PFCOUNT
// reads it as empty (h->st = null) without creating it
static int hll_bind(rbx_ctx *c, rbx_hll *h, bool create, hipStream_t st) {
    c->ks.sweep();
    if (h->ctx != c) return fail(RBX_E_ILLEGAL_ARGUMENT, "the handle belongs to another context");
    if (h->gen == c->ks.generation && h->st) return RBX_OK;
    std::shared_ptr<HllState> s;
    RBX_TRY(hll_get(c, h->name, create, st, &s, nullptr));
    h->st = s;
    if (s) h->gen = c->ks.generation;
    return RBX_OK;
}

// Redis keeps a PFADD-created HLL sparse until an update would store a value > 32 or grow the
// string past hll-sparse-max-bytes, then promotes it to dense for good ([redis-7.2]
// hyperloglog.c hllSparseSet), and the sparse bytes depend on the order of the updates.
// k_hll_sparse_replay applies each command's updates, in order, to the sparse HLLs' strings on
// the device (the registers are updated by the PFADD / merge kernels as for dense keys) and sets
// the sticky promotion word at the first promotion.  `items` = one per sparse HLL of a round.
static int replay_sparse(rbx_ctx *c, std::vector<HllReplay> &items, const KeysDev &dk, int fl, hipStream_t st,
                         TinyArena *ta = nullptr) {
    if (items.empty()) return RBX_OK;
    if (const void *d = ta ? ta->put(items.data(), items.size() * sizeof(HllReplay)) : nullptr) {  // tiny call
        launch_hll_sparse_replay(dk, fl, (const HllReplay *)d, (uint32_t)items.size(), kHllSparseMaxBytes, st);
        HIP_TRY(hipGetLastError());
        return RBX_OK;
    }
    CachedTable<HllReplay> &tab = c->dev->hll.replay;  // cached by content
    const HllReplay *d_items = tab.sync(items, st);
    if (!d_items) return tab.err;
    launch_hll_sparse_replay(dk, fl, d_items, (uint32_t)items.size(), kHllSparseMaxBytes, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

// PFMERGE-style write-back (ascending registers) of the sparse HLLs among hl; their registers
// already hold the merged maxima
static int replay_merge(rbx_ctx *c, const std::vector<HllState *> &hl, hipStream_t st) {
    std::vector<HllReplay> items;
    std::unordered_map<HllState *, int> seen;
    for (HllState *h : hl)
        if (h && !h->dense && !seen.count(h)) {
            seen[h] = 1;
            items.push_back(HllReplay{h->d_sp_ops, h->d_promoted, h->d_regs, 0, 0, h->d_regs, nullptr, 0});
        }
    return replay_sparse(c, items, KeysDev{}, 0, st);
}

// host view of the promotion word (the caller holds a CallScope on c->stream)
static int resolve_dense(rbx_ctx *c, HllState *h) {
    if (h->dense) return RBX_OK;
    uint32_t w = 0;
    HIP_TRY(hipMemcpyAsync(&w, h->d_promoted, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (w) h->dense = true;
    return RBX_OK;
}

// PFADD batch: device elements, commands in order.  Commands naming the same HLL are
// split into successive launches so each reply sees the previous commands' effect.  Command s adds the
// elements [h_beg[s], h_end[s]) and reports under d_changed[seg_id ? seg_id[s] : s].
static int pfadd_run(rbx_ctx *c, const std::vector<HllState *> &hl, const uint64_t *h_beg, const uint64_t *h_end,
                     const uint32_t *seg_id, const KeysDev &dk, uint32_t *d_changed, hipStream_t st,
                     TinyArena *ta = nullptr) {
    const uint32_t nseg = (uint32_t)hl.size();
    std::vector<HllSeg> tiles;
    uint32_t s0 = 0;
    const int fl = fast_len_hll(dk);
    while (s0 < nseg) {
        // a round: maximal run of commands with distinct HLLs
        std::unordered_map<HllState *, int> seen;
        uint32_t s1 = s0;
        while (s1 < nseg && !seen.count(hl[s1])) seen[hl[s1++]] = 1;
        tiles.clear();
        for (uint32_t s = s0; s < s1; ++s) {
            for (uint64_t b = h_beg[s]; b < h_end[s]; b += kTileElems)
                tiles.push_back(HllSeg{hl[s]->d_regs, b, std::min(h_end[s], b + kTileElems), seg_id ? seg_id[s] : s, 0});
        }
        if (!tiles.empty()) {
            // a tiny call's tile list is read from the coherent block (each round its own copy)
            const HllSeg *d_tiles = ta ? (const HllSeg *)ta->put(tiles.data(), tiles.size() * sizeof(HllSeg)) : nullptr;
            if (!d_tiles) {
                // the tile table is cached by content (a steady PFADD pipeline re-sends the same one), for
                // single-round calls; stream order keeps the previous round's kernel ahead of an overwrite
                CachedTable<HllSeg> &tab = c->dev->hll.tiles;
                d_tiles = tab.sync(tiles, st, s0 == 0 && s1 == nseg);
                if (!d_tiles) return tab.err;
            }
            launch_hll_pfadd(dk, fl, d_tiles, (uint32_t)tiles.size(), d_changed, st);
            HIP_TRY(hipGetLastError());
            std::vector<HllReplay> items;  // the round's HLLs are distinct
            for (uint32_t s = s0; s < s1; ++s)
                if (!hl[s]->dense && h_end[s] > h_beg[s])
                    items.push_back(HllReplay{hl[s]->d_sp_ops, hl[s]->d_promoted, nullptr, h_beg[s], h_end[s],
                                              hl[s]->d_regs, nullptr, 0});
            RBX_TRY(replay_sparse(c, items, dk, fl, st, ta));
        }
        s0 = s1;
    }
    return RBX_OK;
}

int hll_add_multi(rbx_ctx *c, const std::vector<std::string> &names, const uint64_t *seg_offsets,
                  const rbx_keys *elements, uint8_t *out_changed) {
    const uint32_t nseg = (uint32_t)names.size();
    RBX_TRY(validate_keys(elements));
    if (nseg == 0) return RBX_OK;
    if (seg_offsets[0] != 0 || seg_offsets[nseg] != elements->n)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "segment offsets must span [0, n]");
    for (uint32_t s = 0; s < nseg; ++s)
        if (seg_offsets[s + 1] < seg_offsets[s]) return fail(RBX_E_ILLEGAL_ARGUMENT, "segment offsets must be ascending");
    RBX_ENTER(c, c->stream);
    Staging &sg = c->dev->stage;
    std::vector<HllState *> hl(nseg);
    std::vector<std::shared_ptr<HllState>> keep(nseg);
    std::vector<uint8_t> created(nseg, 0);
    // type-check every name first, as hll_merge does its sources: the call has one return code, so a key of
    // another type fails it before any missing key is created (the keys named before it were left behind empty)
    std::vector<uint32_t> missing;
    for (uint32_t s = 0; s < nseg; ++s) {
        const Entry *e = c->ks.find(names[s]);
        if (!e) missing.push_back(s);
        else if (e->type != KType::Hll) return fail(RBX_E_WRONGTYPE, kHllWrongType);
        else keep[s] = e->hll;
    }
    for (uint32_t s : missing) {  // (a missing name given twice: the second finds the key the first created)
        bool cr;
        RBX_TRY(hll_get(c, names[s], true, c->stream, &keep[s], &cr));
        created[s] = cr;
    }
    for (uint32_t s = 0; s < nseg; ++s) hl[s] = keep[s].get();
    std::vector<uint32_t> ch(nseg);  // each tier's changed words end up here
    auto reply = [&]() {
        for (uint32_t s = 0; s < nseg; ++s) {
            if (ch[s]) hl[s]->card |= 1ULL << 63;  // HLL_INVALIDATE_CACHE
            if (out_changed) out_changed[s] = ch[s] || created[s];
        }
        return RBX_OK;
    };
    if (nseg <= kSegMaxKeys && bloom_tiny_fits(c, elements)) {
        // elements, changed words, tile list and replay items in coherent pinned memory (bloom_host_tiny)
        auto *ch_h = (uint32_t *)(sg.tiny() + kTinySegAt);
        memset(ch_h, 0, (size_t)nseg * 4);
        const KeysDev dk = tiny_stage(c, elements);
        TinyArena ta{sg.tiny() + kTinyArenaAt, sg.pin_tiny_dev + kTinyArenaAt, kTinyArenaBytes, 0};
        RBX_TRY(tiny_done(c, pfadd_run(c, hl, seg_offsets, seg_offsets + 1, nullptr, dk,
                                       (uint32_t *)(sg.pin_tiny_dev + kTinySegAt), c->stream, &ta),
                          g_tune.tiny_spin));
        memcpy(ch.data(), ch_h, (size_t)nseg * 4);
        return reply();
    }
    if (nseg <= kSmallHead / 4 && bloom_small_fits(c, elements)) {
        // one transfer for the elements and the zeroed changed words, one readback (bloom_host_small)
        SmallStage sm;
        RBX_TRY(small_stage(c, elements, nseg * 4, &sm));
        const int rc = pfadd_run(c, hl, seg_offsets, seg_offsets + 1, nullptr, sm.dk, (uint32_t *)sm.dp, c->stream);
        (void)hipEventRecord(sg.ev_done[0], c->stream);
        if (rc != RBX_OK) return small_fail(c, rc);
        HIP_TRY(hipMemcpyAsync(sm.hp, sm.dp, nseg * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        memcpy(ch.data(), sm.hp, nseg * 4);
        return reply();
    }
    RBX_TRY(c->dev->shared.misc.reserve(nseg * 4));
    auto *d_changed = c->dev->shared.misc.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_changed, 0, nseg * 4, c->stream));
    auto span_bytes = [&](uint64_t e0, uint64_t e1) {
        return elements->offsets ? elements->offsets[e1] - elements->offsets[e0] : (e1 - e0) * elements->stride;
    };
    const uint64_t budget = 256ull << 20;
    for (uint32_t s0 = 0; s0 < nseg;) {
        // commands [s0, s1) whose elements fit one staging upload (at least one command)
        uint32_t s1 = s0 + 1;
        while (s1 < nseg && span_bytes(seg_offsets[s0], seg_offsets[s1 + 1]) <= budget) ++s1;
        const uint64_t e0 = seg_offsets[s0], e1 = seg_offsets[s1];
        KeysDev dk{};
        if (e1 > e0) RBX_TRY(upload_keys(c, elements, e0, e1, &dk));
        std::vector<uint64_t> reb(s1 - s0 + 1);
        for (uint32_t s = s0; s <= s1; ++s) reb[s - s0] = seg_offsets[s] - e0;
        std::vector<HllState *> grp(hl.begin() + s0, hl.begin() + s1);
        RBX_TRY(pfadd_run(c, grp, reb.data(), reb.data() + 1, nullptr, dk, d_changed + s0, c->stream));
        s0 = s1;
    }
    HIP_TRY(hipMemcpyAsync(ch.data(), d_changed, nseg * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return reply();
}

// glibc-side hllTau fallback and the full estimator from a histogram (redis hllCount)
static double hll_tau_host(double x) {
    if (x == 0. || x == 1.) return 0.;
    double zPrime;
    double y = 1.0;
    double z = 1 - x;
    do {
        x = std::sqrt(x);
        zPrime = z;
        y *= 0.5;
        z -= std::pow(1 - x, 2) * y;
    } while (zPrime != z);
    return z / 3;
}

static double hll_sigma_host(double x) {
    if (x == 1.) return INFINITY;
    double zPrime;
    double y = 1;
    double z = x;
    do {
        x *= x;
        zPrime = z;
        z += x * y;
        y += y;
    } while (zPrime != z);
    return z;
}

static uint64_t hll_count_from_histo(const int *reghisto) {
    double m = 16384;
    double z = m * hll_tau_host((m - reghisto[51]) / (double)m);
    for (int j = 50; j >= 1; --j) {
        z += reghisto[j];
        z *= 0.5;
    }
    z += m * hll_sigma_host(reghisto[0] / (double)m);
    double E = (double)llroundl(0.721347520444481703680 * m * m / z);
    return (uint64_t)E;
}

// Computes counts for raw register arrays (device pointers) -> host out, on `st` (waited for).
static int count_regs(rbx_ctx *c, const std::vector<uint8_t *> &regs, uint64_t *out, hipStream_t st) {
    uint32_t n = (uint32_t)regs.size();
    if (!n) return RBX_OK;
    SharedScratch &sh = c->dev->shared;
    RBX_TRY(sh.ptrs.reserve(n * sizeof(uint8_t *)));
    RBX_TRY(sh.histo.reserve((size_t)n * 64 * sizeof(int)));
    RBX_TRY(sh.misc.reserve(n * 8));
    HIP_TRY(hipMemcpyAsync(sh.ptrs.p, regs.data(), n * sizeof(uint8_t *), hipMemcpyHostToDevice, st));
    launch_hll_count(sh.ptrs.as<uint8_t *>(), n, sh.histo.as<int>(), sh.misc.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> res(n);
    HIP_TRY(hipMemcpyAsync(res.data(), sh.misc.p, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> h;
    for (uint32_t i = 0; i < n; ++i) {
        if (res[i] == ~0ULL) {  // tau branch: histogram to host, glibc pow
            if (h.empty()) {
                h.resize((size_t)n * 64);
                HIP_TRY(hipMemcpy(h.data(), sh.histo.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
            }
            res[i] = hll_count_from_histo(&h[(size_t)i * 64]);
        }
        out[i] = res[i];
    }
    return RBX_OK;
}

// single-key PFCOUNT with the header cache (valid cache -> cached value; else compute+store)
static int pfcount_each(rbx_ctx *c, const std::vector<HllState *> &hl, uint64_t *out, hipStream_t st) {
    std::vector<uint8_t *> regs;
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < hl.size(); ++i) {
        if (!hl[i]) {
            out[i] = 0;
            continue;
        }
        if (!(hl[i]->card >> 63)) {
            out[i] = hl[i]->card;
            continue;
        }
        regs.push_back(hl[i]->d_regs);
        idx.push_back(i);
    }
    std::vector<uint64_t> r(regs.size());
    RBX_TRY(count_regs(c, regs, r.data(), st));
    for (size_t j = 0; j < idx.size(); ++j) {
        out[idx[j]] = r[j];
        hl[idx[j]]->card = r[j];  // store the (valid) cached cardinality
    }
    return RBX_OK;
}

static int hll_count_each(rbx_ctx *c, const std::vector<std::string> &names, uint64_t *out) {
    RBX_ENTER(c, c->stream);
    const uint32_t n = (uint32_t)names.size();
    std::vector<HllState *> hl(n);
    std::vector<std::shared_ptr<HllState>> keep(n);
    for (uint32_t i = 0; i < n; ++i) {
        RBX_TRY(hll_get(c, names[i], false, c->stream, &keep[i], nullptr));
        hl[i] = keep[i].get();
    }
    return pfcount_each(c, hl, out, c->stream);
}

// ---- the ordered PFADD / PFCOUNT stream over many keys (RBatch.getHyperLogLog, M/RedissonBatch.java:57-64) ----
// DESIGN 11.7.  The commands are host arrays, so the host walks them: it finds the commands that fail alone,
// creates the keys, splits the stream into phases and picks each add run's path.
static std::atomic<uint32_t> g_hllstream_last[4];  // rbx_bench_hllstream_last shows them
enum { kHsPhases = 0, kHsRoundsRuns = 1, kHsGroupedRuns = 2, kHsChunks = 3 };

// The keys of one stream call (stream_names_resolve has the rules)
struct HsKeys {
    std::vector<uint32_t> canon;
    std::vector<uint8_t> wrong;                  // per entry of names
    std::vector<std::shared_ptr<HllState>> hll;  // per canonical id; null = missing
    std::vector<uint64_t> stamp, round;          // per canonical id: the phase of its last PFADD, its last round
    std::vector<uint32_t> slot;                  // per canonical id: its place among a chunk's sparse keys + 1
    bool any_wrong = false;
};

static int hll_stream_check(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key,
                            const uint8_t *cmd_op, const uint64_t *cmd_elem, uint64_t n, const rbx_keys *elements) {
    if (n && (!cmd_key || !cmd_op || !cmd_elem || !elements)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(stream_names_check(c, names, nkeys));
    if (n == 0) return RBX_OK;
    RBX_TRY(validate_keys(elements));
    if (n >= (1ULL << 32)) return fail(RBX_E_ILLEGAL_ARGUMENT, "a batch takes fewer than 2^32 commands");
    if (cmd_elem[0] != 0 || cmd_elem[n] != elements->n)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "element offsets must span [0, elements->n]");
    for (uint64_t i = 0; i < n; ++i) {
        if (cmd_key[i] >= nkeys) return fail(RBX_E_ILLEGAL_ARGUMENT, "a command's key is not below nkeys");
        if (cmd_op[i] > RBX_HLL_PFCOUNT) return fail(RBX_E_ILLEGAL_ARGUMENT, "a command's op is not RBX_HLL_PFADD or RBX_HLL_PFCOUNT");
        if (cmd_elem[i + 1] < cmd_elem[i]) return fail(RBX_E_ILLEGAL_ARGUMENT, "element offsets must be ascending");
        if (cmd_op[i] == RBX_HLL_PFCOUNT && cmd_elem[i + 1] != cmd_elem[i])
            return fail(RBX_E_ILLEGAL_ARGUMENT, "a PFCOUNT carries no elements");
    }
    return RBX_OK;
}

// What one call carries through its phases.  Element g of the call is element g - elem_base of `dk`.
struct HsCall {
    rbx_ctx *c;
    hipStream_t st;
    HsKeys keys;
    const uint32_t *cmd_key;
    const uint8_t *cmd_op;
    const uint64_t *cmd_elem;
    const HllKey *d_tab;
    const uint64_t *d_cmd_elem;
    const uint32_t *d_cmd_key;
    uint32_t *d_changed;
    uint32_t nkeys;
    uint64_t n;
    std::vector<uint8_t> created;  // per command: this PFADD created its key
    uint64_t *replies;
    KeysDev dk;
    uint64_t elem_base;
    uint64_t phase = 0, rounds = 0;
    uint32_t stats[4] = {0, 0, 0, 0};
    HllState *hll_of(uint64_t i) const { return keys.hll[keys.canon[cmd_key[i]]].get(); }
    bool failed(uint64_t i) const { return keys.wrong[cmd_key[i]] != 0; }
    bool adds(uint64_t i) const { return cmd_op[i] == RBX_HLL_PFADD && !failed(i); }
};

// the commands [a, b) by rounds: the PFADDs that run and carry elements, through pfadd_run
static int hs_rounds(HsCall &h, uint64_t a, uint64_t b) {
    std::vector<HllState *> hl;
    std::vector<uint64_t> beg, end;
    std::vector<uint32_t> id;
    for (uint64_t i = a; i < b; ++i)
        if (h.adds(i) && h.cmd_elem[i + 1] > h.cmd_elem[i]) {
            hl.push_back(h.hll_of(i));
            beg.push_back(h.cmd_elem[i] - h.elem_base);
            end.push_back(h.cmd_elem[i + 1] - h.elem_base);
            id.push_back((uint32_t)i);
        }
    if (hl.empty()) return RBX_OK;
    return pfadd_run(h.c, hl, beg.data(), end.data(), id.data(), h.dk, h.d_changed, h.st);
}

// One grouped chunk: the commands [a, b), m = cmd_elem[b] - cmd_elem[a] elements in 1 .. hllstream_chunk.
// Registers first (pairs, sort, runs); then, the registers final, one replay launch for the chunk's sparse
// keys, each over its own elements in command order across all of its commands.
static int hs_grouped_chunk(HsCall &h, uint64_t a, uint64_t b, int key_bits) {
    rbx_ctx *c = h.c;
    HllStreamScratch &ss = c->dev->hll.strm;
    const uint64_t e0 = h.cmd_elem[a], first = e0 - h.elem_base;
    const uint32_t m = (uint32_t)(h.cmd_elem[b] - e0);
    const int fl = fast_len_hll(h.dk);
    RBX_TRY(cell_sort_reserve<unsigned long long>(ss.sort, m, kHsRegShift, hllstream_end_bit(key_bits, h.keys.any_wrong)));
    RBX_TRY(sort_failed(launch_hllstream_grouped(h.dk, fl, first, e0, m, h.d_tab, h.d_cmd_elem, h.d_cmd_key, a,
                                                 (uint32_t)(b - a), h.d_changed, key_bits, h.keys.any_wrong, ss.sort.p,
                                                 ss.sort.cap, h.st)));
    HIP_TRY(hipGetLastError());
    // the sparse keys' element lists: count, place, fill
    std::vector<uint32_t> skeys;   // canonical ids of the chunk's sparse keys, in order of first appearance
    std::vector<uint64_t> count;   // their elements
    for (uint64_t i = a; i < b; ++i) {
        if (!h.adds(i) || h.cmd_elem[i + 1] == h.cmd_elem[i] || h.hll_of(i)->dense) continue;
        const uint32_t k = h.keys.canon[h.cmd_key[i]];
        if (!h.keys.slot[k]) {
            skeys.push_back(k);
            count.push_back(0);
            h.keys.slot[k] = (uint32_t)skeys.size();
        }
        count[h.keys.slot[k] - 1] += h.cmd_elem[i + 1] - h.cmd_elem[i];
    }
    if (skeys.empty()) return RBX_OK;
    std::vector<uint64_t> at(skeys.size() + 1, 0);
    for (size_t j = 0; j < skeys.size(); ++j) at[j + 1] = at[j] + count[j];
    std::vector<uint32_t> list(at.back());
    std::vector<uint64_t> fill(at.begin(), at.end() - 1);
    for (uint64_t i = a; i < b; ++i) {
        if (!h.adds(i) || h.cmd_elem[i + 1] == h.cmd_elem[i]) continue;
        const uint32_t sl = h.keys.slot[h.keys.canon[h.cmd_key[i]]];
        if (!sl) continue;
        uint64_t &w = fill[sl - 1];
        for (uint64_t g = h.cmd_elem[i]; g < h.cmd_elem[i + 1]; ++g) list[w++] = (uint32_t)(g - e0);
    }
    RBX_TRY(ss.lists.reserve(list.size() * 4));
    HIP_TRY(hipMemcpyAsync(ss.lists.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, h.st));
    std::vector<HllReplay> items;
    for (size_t j = 0; j < skeys.size(); ++j) {
        HllState *s = h.keys.hll[skeys[j]].get();
        h.keys.slot[skeys[j]] = 0;
        items.push_back(HllReplay{s->d_sp_ops, s->d_promoted, nullptr, at[j], at[j + 1], s->d_regs,
                                  ss.lists.as<uint32_t>(), first});
    }
    return replay_sparse(c, items, h.dk, fl, h.st);
}

// One phase, the commands [p0, p1): its PFCOUNTs as one pass over the state before it, then its PFADDs as one
// add run, then the run's one readback (the changed words and the sparse keys' promotion words).
static int hs_phase(HsCall &h, uint64_t p0, uint64_t p1) {
    rbx_ctx *c = h.c;
    HllStreamScratch &ss = c->dev->hll.strm;
    h.stats[kHsPhases]++;
    std::vector<HllState *> hl;
    std::vector<uint64_t> at;
    uint64_t nadd = 0, elems = 0, runs = 1;
    h.rounds++;
    for (uint64_t i = p0; i < p1; ++i) {
        if (h.failed(i)) continue;
        if (h.cmd_op[i] == RBX_HLL_PFCOUNT) {
            hl.push_back(h.hll_of(i));
            at.push_back(i);
        } else if (h.cmd_elem[i + 1] > h.cmd_elem[i]) {
            // the greedy rule of pfadd_run: a command on a key of the current round opens the next one
            uint64_t &r = h.keys.round[h.keys.canon[h.cmd_key[i]]];
            if (r == h.rounds) {
                h.rounds++;
                runs++;
            }
            r = h.rounds;
            nadd++;
            elems += h.cmd_elem[i + 1] - h.cmd_elem[i];
        }
    }
    if (!hl.empty()) {
        std::vector<uint64_t> out(hl.size());
        RBX_TRY(pfcount_each(c, hl, out.data(), h.st));
        if (h.replies)
            for (size_t j = 0; j < at.size(); ++j) h.replies[at[j]] = out[j];
    }
    std::vector<uint32_t> ch;
    if (nadd) {
        const int tuned = g_tune.hllstream_path;
        const uint64_t per_round = g_tune.hllstream_elems_per_round, chunk = g_tune.hllstream_chunk;
        const bool grouped = tuned == 2 || (tuned == 0 && runs > std::max<uint64_t>(1, elems / per_round));
        if (!grouped) {
            h.stats[kHsRoundsRuns]++;
            RBX_TRY(hs_rounds(h, p0, p1));
        } else {
            h.stats[kHsGroupedRuns]++;
            const int key_bits = significant_bits(h.nkeys - 1);
            for (uint64_t a = p0; a < p1;) {
                // the commands [a, b) whose elements fit one chunk; a command that does not goes by rounds, alone
                uint64_t b = a;
                while (b < p1 && h.cmd_elem[b + 1] - h.cmd_elem[a] <= chunk) ++b;
                if (b == a) {
                    RBX_TRY(hs_rounds(h, a, a + 1));
                    b = a + 1;
                } else if (h.cmd_elem[b] > h.cmd_elem[a]) {
                    h.stats[kHsChunks]++;
                    RBX_TRY(hs_grouped_chunk(h, a, b, key_bits));
                }
                a = b;
            }
        }
        // the sparse keys of the run: the host learns their promotions here, so that a key promoted by this run
        // costs the next one no element list and no replay block
        std::vector<uint32_t *> states;
        std::vector<HllState *> sparse;
        for (uint64_t i = p0; i < p1; ++i) {
            if (!h.adds(i) || h.cmd_elem[i + 1] == h.cmd_elem[i]) continue;
            const uint32_t k = h.keys.canon[h.cmd_key[i]];
            HllState *s = h.keys.hll[k].get();
            if (s->dense || h.keys.slot[k]) continue;
            h.keys.slot[k] = 1;
            states.push_back(s->d_promoted);
            sparse.push_back(s);
        }
        for (uint64_t i = p0; i < p1; ++i) h.keys.slot[h.keys.canon[h.cmd_key[i]]] = 0;
        std::vector<uint32_t> promoted(states.size());
        uint32_t *d_promoted = h.d_changed + h.n;
        if (!states.empty()) {
            RBX_TRY(ss.ptrs.reserve(states.size() * sizeof(uint32_t *)));
            HIP_TRY(hipMemcpyAsync(ss.ptrs.p, states.data(), states.size() * sizeof(uint32_t *), hipMemcpyHostToDevice, h.st));
            launch_hllstream_promoted(ss.ptrs.as<uint32_t *>(), (uint32_t)states.size(), d_promoted, h.st);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(promoted.data(), d_promoted, states.size() * 4, hipMemcpyDeviceToHost, h.st));
        }
        ch.resize(p1 - p0);
        HIP_TRY(hipMemcpyAsync(ch.data(), h.d_changed + p0, (p1 - p0) * 4, hipMemcpyDeviceToHost, h.st));
        HIP_TRY(hipStreamSynchronize(h.st));
        for (size_t j = 0; j < sparse.size(); ++j)
            if (promoted[j]) sparse[j]->dense = true;
    }
    for (uint64_t i = p0; i < p1; ++i) {
        if (!h.adds(i)) continue;
        const bool changed = !ch.empty() && ch[i - p0];
        if (changed) h.hll_of(i)->card |= 1ULL << 63;  // HLL_INVALIDATE_CACHE
        if (h.replies) h.replies[i] = changed || h.created[i];
    }
    return RBX_OK;
}

// the commands [g0, g1) over the elements of h.dk: a phase is a maximal stretch in which no PFCOUNT names a key
// that an earlier PFADD of the stretch names
static int hs_phases(HsCall &h, uint64_t g0, uint64_t g1) {
    for (uint64_t p0 = g0; p0 < g1;) {
        h.phase++;
        uint64_t p1 = p0;
        for (; p1 < g1; ++p1) {
            if (h.failed(p1)) continue;
            uint64_t &s = h.keys.stamp[h.keys.canon[h.cmd_key[p1]]];
            if (h.cmd_op[p1] == RBX_HLL_PFADD) s = h.phase;
            else if (s == h.phase) break;
        }
        RBX_TRY(hs_phase(h, p0, p1));
        p0 = p1;
    }
    return RBX_OK;
}

// rbx_hll_stream[_dev] behind the argument checks, n > 0.  dev: `elements` is device memory (else it is uploaded
// in groups of whole commands, as hll_add_multi uploads its segments).
static int hll_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key, const uint8_t *cmd_op,
                      const uint64_t *cmd_elem, uint64_t n, const rbx_keys *elements, uint64_t *replies, uint8_t *status,
                      bool dev, hipStream_t st) {
    RBX_ENTER(c, st);
    HsCall h{};
    h.c = c;
    h.st = st;
    h.cmd_key = cmd_key;
    h.cmd_op = cmd_op;
    h.cmd_elem = cmd_elem;
    h.nkeys = nkeys;
    h.n = n;
    h.replies = replies;
    HsKeys &K = h.keys;
    K.canon.resize(nkeys);
    K.wrong.assign(nkeys, 0);
    K.hll.resize(nkeys);
    K.stamp.assign(nkeys, 0);
    K.round.assign(nkeys, 0);
    K.slot.assign(nkeys, 0);
    std::vector<std::string> nm;
    K.any_wrong = stream_names_resolve(c, names, nkeys, KType::Hll, &nm, K.canon.data(), K.wrong.data(),
                                       [&](uint32_t i, const Entry &e) { K.hll[i] = e.hll; });
    // the commands that fail alone, and the keys the others create: the first PFADD that runs on a missing key
    uint64_t first_failed = ~0ULL;
    h.created.assign(n, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (replies) replies[i] = 0;
        if (status) status[i] = h.failed(i) ? 0xFF : 0;
        if (h.failed(i)) {
            first_failed = std::min(first_failed, i);
            continue;
        }
        const uint32_t k = K.canon[cmd_key[i]];
        if (cmd_op[i] == RBX_HLL_PFADD && !K.hll[k]) {
            bool cr;
            RBX_TRY(hll_get(c, nm[k], true, st, &K.hll[k], &cr));
            h.created[i] = cr;
        }
    }
    HllStreamScratch &ss = c->dev->hll.strm;
    std::vector<HllKey> tab(nkeys);
    for (uint32_t i = 0; i < nkeys; ++i) {
        const uint32_t k = K.canon[i];
        tab[i] = HllKey{K.hll[k] ? K.hll[k]->d_regs : nullptr, K.wrong[i] ? (kHllKeyWrong | kHllKeyFailed) : 0u, k};
    }
    h.d_tab = ss.keys.sync(tab, st);
    if (!h.d_tab) return ss.keys.err;
    // the call's element offsets and keys, and one zeroed changed word per command (+ the promotion words)
    RBX_TRY(ss.cmds.reserve((n + 1) * 8 + n * 4));
    RBX_TRY(ss.changed.reserve((n + nkeys) * 4));
    h.d_cmd_elem = ss.cmds.as<uint64_t>();
    h.d_cmd_key = (const uint32_t *)(h.d_cmd_elem + n + 1);
    h.d_changed = ss.changed.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync((void *)h.d_cmd_elem, cmd_elem, (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync((void *)h.d_cmd_key, cmd_key, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h.d_changed, 0, n * 4, st));
    if (dev) {
        h.dk = keys_dev(elements);
        h.elem_base = 0;
        RBX_TRY(hs_phases(h, 0, n));
    } else {
        auto span_bytes = [&](uint64_t e0, uint64_t e1) {
            return elements->offsets ? elements->offsets[e1] - elements->offsets[e0] : (e1 - e0) * elements->stride;
        };
        const uint64_t budget = 256ull << 20;
        for (uint64_t g0 = 0; g0 < n;) {
            // commands [g0, g1) whose elements fit one staging upload (at least one command)
            uint64_t g1 = g0 + 1;
            while (g1 < n && span_bytes(cmd_elem[g0], cmd_elem[g1 + 1]) <= budget) ++g1;
            h.dk = KeysDev{};
            h.elem_base = cmd_elem[g0];
            if (cmd_elem[g1] > cmd_elem[g0]) RBX_TRY(upload_keys(c, elements, cmd_elem[g0], cmd_elem[g1], &h.dk));
            RBX_TRY(hs_phases(h, g0, g1));
            g0 = g1;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) g_hllstream_last[i] = h.stats[i];
    if (first_failed != ~0ULL) return fail(RBX_E_WRONGTYPE, kHllWrongType);
    return RBX_OK;
}

// PFCOUNT k1..kn: one key = the cached single-key count; several = count of the union
int hll_count(rbx_ctx *c, const std::vector<std::string> &names, uint64_t *out) {
    if (names.size() == 1) return hll_count_each(c, names, out);
    RBX_ENTER(c, c->stream);
    std::vector<std::shared_ptr<HllState>> keep;
    std::vector<uint8_t *> srcs;
    for (const auto &nm : names) {
        std::shared_ptr<HllState> h;
        RBX_TRY(hll_get(c, nm, false, c->stream, &h, nullptr));
        if (h) {
            srcs.push_back(h->d_regs);
            keep.push_back(h);
        }
    }
    if (srcs.empty()) {
        *out = 0;
        return RBX_OK;
    }
    DevBuf &ptrs = c->dev->shared.ptrs, &merged = c->dev->stage.out_bytes;
    RBX_TRY(ptrs.reserve(srcs.size() * sizeof(uint8_t *)));
    RBX_TRY(merged.reserve(kHllBytes));
    HIP_TRY(hipMemcpyAsync(ptrs.p, srcs.data(), srcs.size() * sizeof(uint8_t *), hipMemcpyHostToDevice, c->stream));
    launch_hll_union(ptrs.as<uint8_t *>(), (uint32_t)srcs.size(), merged.as<uint8_t>(), c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<uint8_t *> u{merged.as<uint8_t>()};
    return count_regs(c, u, out, c->stream);
}

// PFMERGE dest src1..srcn (dest's own registers included)
int hll_merge(rbx_ctx *c, const std::string &dest, const std::vector<std::string> &srcs) {
    RBX_ENTER(c, c->stream);
    std::vector<std::shared_ptr<HllState>> keep;
    std::vector<uint8_t *> sp;
    for (const auto &s : srcs) {  // type-check every source first (isHLLObjectOrReply)
        std::shared_ptr<HllState> h;
        RBX_TRY(hll_get(c, s, false, c->stream, &h, nullptr));
        if (h) {
            sp.push_back(h->d_regs);
            keep.push_back(h);
        }
    }
    std::shared_ptr<HllState> d;
    RBX_TRY(hll_get(c, dest, true, c->stream, &d, nullptr));
    RBX_TRY(resolve_dense(c, d.get()));
    for (auto &h : keep) {
        RBX_TRY(resolve_dense(c, h.get()));
        d->dense = d->dense || h->dense;  // pfmergeCommand: use_dense if any input is
    }
    if (!sp.empty()) {
        DevBuf &ptrs = c->dev->shared.ptrs;
        RBX_TRY(ptrs.reserve(sp.size() * sizeof(uint8_t *)));
        HIP_TRY(hipMemcpyAsync(ptrs.p, sp.data(), sp.size() * sizeof(uint8_t *), hipMemcpyHostToDevice, c->stream));
        launch_hll_merge(d->d_regs, ptrs.as<uint8_t *>(), (uint32_t)sp.size(), c->stream);
        HIP_TRY(hipGetLastError());
        RBX_TRY(replay_merge(c, {d.get()}, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    d->card |= 1ULL << 63;  // HLL_INVALIDATE_CACHE
    return RBX_OK;
}

// ---- many PFCOUNT unions / PFMERGEs in one call (rbx_hll_count_groups, rbx_hll_merge_groups) ----
static std::atomic<uint32_t> g_hllgroups_last[4];  // rbx_bench_hllgroups_last shows them
enum { kHgPhases = 0, kHgLaunches = 1, kHgSplit = 2, kHgDeviceGroups = 3 };

// The keys of one grouped call, each distinct name resolved once (stream_names_resolve has the rules), and the
// groups that fail alone: those that name a key of another type.
struct HgKeys {
    std::vector<std::string> nm;
    std::vector<uint32_t> canon;
    std::vector<uint8_t> wrong;                  // per entry of names
    std::vector<std::shared_ptr<HllState>> hll;  // per canonical id; null = missing
    HllState *of(uint32_t key) const { return hll[canon[key]].get(); }
};

static void hg_resolve(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, HgKeys *K) {
    K->canon.resize(nkeys);
    K->wrong.assign(nkeys, 0);
    K->hll.resize(nkeys);
    stream_names_resolve(c, names, nkeys, KType::Hll, &K->nm, K->canon.data(), K->wrong.data(),
                         [&](uint32_t i, const Entry &e) { K->hll[i] = e.hll; });
}

static int hg_split(uint64_t groups) {
    const int tuned = g_tune.hllgroups_split;
    int p = tuned ? tuned : hllgroups_auto_split(groups);
    while (p > 1 && groups * (uint64_t)p >= (1ULL << 31)) p >>= 1;  // the grid
    return p;
}

// One launch's table -- offsets (n + 1 u32, padded to 8 bytes) | destinations (a merge's) | member pointers --
// in one upload.  off.size() == n + 1; dst is empty for a count.
struct HgTable {
    const uint32_t *d_off;
    uint8_t *const *d_dst;
    const uint8_t *const *d_members;
};
static int hg_upload(rbx_ctx *c, const std::vector<uint32_t> &off, const std::vector<uint8_t *> &dst,
                     const std::vector<const uint8_t *> &members, hipStream_t st, HgTable *t) {
    const size_t off_bytes = (off.size() * 4 + 7) & ~(size_t)7;
    const size_t bytes = off_bytes + (dst.size() + members.size()) * sizeof(void *);
    std::vector<uint8_t> blob(bytes);
    memcpy(blob.data(), off.data(), off.size() * 4);
    if (!dst.empty()) memcpy(blob.data() + off_bytes, dst.data(), dst.size() * sizeof(void *));
    if (!members.empty())
        memcpy(blob.data() + off_bytes + dst.size() * sizeof(void *), members.data(), members.size() * sizeof(void *));
    DevBuf &tab = c->dev->hll.grp.table;
    RBX_TRY(tab.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(tab.p, blob.data(), bytes, hipMemcpyHostToDevice, st));
    uint8_t *p = tab.as<uint8_t>();
    t->d_off = (const uint32_t *)p;
    t->d_dst = (uint8_t *const *)(p + off_bytes);
    t->d_members = (const uint8_t *const *)(p + off_bytes + dst.size() * sizeof(void *));
    return RBX_OK;
}

static int hll_count_groups(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint64_t *grp_off,
                            const uint32_t *grp_key, uint32_t ngroups, uint64_t *out, uint8_t *status) {
    RBX_ENTER(c, c->stream);
    hipStream_t st = c->stream;
    HgKeys K;
    hg_resolve(c, names, nkeys, &K);
    uint32_t stats[4] = {0, 0, 0, 0};
    // the groups that reach the device: unions of existing keys, and one-key counts whose cache is invalid
    std::vector<uint32_t> off{0}, at;
    std::vector<const uint8_t *> members;
    std::vector<HllState *> store;  // per device group: the key whose header takes the recount, or null
    bool any_failed = false;
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint64_t a = grp_off[g], b = grp_off[g + 1];
        bool failed = false;
        for (uint64_t i = a; i < b && !failed; ++i) failed = K.wrong[grp_key[i]] != 0;
        out[g] = 0;
        if (status) status[g] = failed ? 0xFF : 0;
        if (failed) {
            any_failed = true;
            continue;
        }
        HllState *single = nullptr;
        if (b - a == 1) {  // PFCOUNT key: the header cache
            single = K.of(grp_key[a]);
            if (!single) continue;
            if (!(single->card >> 63)) {
                out[g] = single->card;
                continue;
            }
            members.push_back(single->d_regs);
        } else {
            for (uint64_t i = a; i < b; ++i)
                if (HllState *h = K.of(grp_key[i])) members.push_back(h->d_regs);
            if (members.size() == off.back()) continue;  // every key is missing: 0
        }
        off.push_back((uint32_t)members.size());
        at.push_back(g);
        store.push_back(single);
    }
    const uint32_t n = (uint32_t)at.size();
    if (n) {
        HllGroupsScratch &gs = c->dev->hll.grp;
        HgTable t;
        RBX_TRY(hg_upload(c, off, {}, members, st, &t));
        RBX_TRY(gs.histo.reserve((size_t)n * 64 * sizeof(int)));
        RBX_TRY(gs.out.reserve((size_t)n * 8));
        const int split = hg_split(n);
        const int e = launch_hllgroups_union_count(t.d_members, t.d_off, n, split, gs.histo.as<int>(),
                                                   gs.out.as<unsigned long long>(), st);
        if (e) return fail(RBX_E_DEVICE, hipGetErrorString((hipError_t)e));
        HIP_TRY(hipGetLastError());
        stats[kHgLaunches] = 1;
        stats[kHgSplit] = (uint32_t)split;
        stats[kHgDeviceGroups] = n;
        std::vector<unsigned long long> res(n);
        HIP_TRY(hipMemcpyAsync(res.data(), gs.out.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<int> h;
        for (uint32_t j = 0; j < n; ++j) {
            if (res[j] == ~0ULL) {  // tau branch: histogram to host, glibc pow (count_regs)
                if (h.empty()) {
                    h.resize((size_t)n * 64);
                    HIP_TRY(hipMemcpy(h.data(), gs.histo.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
                }
                res[j] = hll_count_from_histo(&h[(size_t)j * 64]);
            }
            out[at[j]] = res[j];
            if (store[j]) store[j]->card = res[j];  // the (valid) cached cardinality; a union stores nothing
        }
    }
    for (int i = 0; i < 4; ++i) g_hllgroups_last[i] = stats[i];
    if (any_failed) return fail(RBX_E_WRONGTYPE, kHllWrongType);
    return RBX_OK;
}

// One phase of a merge call, the groups [p0, p1) that do not fail: no destination is another group's source or
// destination (hll_groups_plan), so one launch runs them all.
static int hg_merge_phase(rbx_ctx *c, HgKeys &K, const uint32_t *grp_dest, const uint64_t *grp_off,
                          const uint32_t *grp_key, const uint8_t *failed, uint32_t p0, uint32_t p1, hipStream_t st,
                          uint32_t *stats) {
    HllGroupsScratch &gs = c->dev->hll.grp;
    stats[kHgPhases]++;
    std::vector<uint32_t> groups;
    for (uint32_t g = p0; g < p1; ++g)
        if (!failed[g]) groups.push_back(g);
    // the missing destinations (createHLLObject: sparse, one XZERO)
    for (uint32_t g : groups) {
        const uint32_t k = K.canon[grp_dest[g]];
        if (!K.hll[k]) RBX_TRY(hll_get(c, K.nm[k], true, st, &K.hll[k], nullptr));
    }
    // the promotion words of the phase's keys that the host does not know to be dense, in one copy
    std::vector<HllState *> sparse;
    std::vector<uint32_t *> states;
    std::unordered_map<HllState *, int> seen;
    auto note = [&](HllState *h) {
        if (h && !h->dense && seen.emplace(h, 1).second) {
            sparse.push_back(h);
            states.push_back(h->d_promoted);
        }
    };
    std::vector<uint32_t> off{0};
    std::vector<uint8_t *> dst;
    std::vector<const uint8_t *> members;
    std::vector<uint32_t> launched;  // the groups with an existing source
    for (uint32_t g : groups) {
        HllState *d = K.of(grp_dest[g]);
        note(d);
        const size_t before = members.size();
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i)
            if (HllState *h = K.of(grp_key[i])) {
                note(h);
                members.push_back(h->d_regs);
            }
        if (members.size() == before) continue;  // nothing to merge in: the destination stands as it is
        dst.push_back(d->d_regs);
        off.push_back((uint32_t)members.size());
        launched.push_back(g);
    }
    std::vector<uint32_t> promoted(states.size());
    if (!states.empty()) {
        RBX_TRY(gs.ptrs.reserve(states.size() * sizeof(uint32_t *)));
        RBX_TRY(gs.out.reserve(states.size() * 4));
        HIP_TRY(hipMemcpyAsync(gs.ptrs.p, states.data(), states.size() * sizeof(uint32_t *), hipMemcpyHostToDevice, st));
        launch_hllstream_promoted(gs.ptrs.as<uint32_t *>(), (uint32_t)states.size(), gs.out.as<uint32_t>(), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(promoted.data(), gs.out.p, states.size() * 4, hipMemcpyDeviceToHost, st));
    }
    if (!launched.empty()) {
        HgTable t;
        RBX_TRY(hg_upload(c, off, dst, members, st, &t));
        const int split = hg_split(launched.size());
        launch_hllgroups_merge(t.d_dst, t.d_members, t.d_off, (uint32_t)launched.size(), split, st);
        HIP_TRY(hipGetLastError());
        stats[kHgLaunches]++;
        stats[kHgSplit] = (uint32_t)split;
        stats[kHgDeviceGroups] += (uint32_t)launched.size();
    }
    if (!states.empty()) {
        HIP_TRY(hipStreamSynchronize(st));  // the phase's one wait
        for (size_t j = 0; j < sparse.size(); ++j)
            if (promoted[j]) sparse[j]->dense = true;
    }
    // pfmergeCommand: use_dense if the destination or any existing source is; else the string takes the maxima
    std::vector<HllState *> back;
    for (uint32_t g : groups) {
        HllState *d = K.of(grp_dest[g]);
        bool had_source = false;
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i)
            if (HllState *h = K.of(grp_key[i])) {
                had_source = true;
                d->dense = d->dense || h->dense;
            }
        if (had_source && !d->dense) back.push_back(d);
        d->card |= 1ULL << 63;  // HLL_INVALIDATE_CACHE: always, also without sources
    }
    return replay_merge(c, back, st);
}

static int hll_merge_groups(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *grp_dest,
                            const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups, uint8_t *status) {
    RBX_ENTER(c, c->stream);
    hipStream_t st = c->stream;
    HgKeys K;
    hg_resolve(c, names, nkeys, &K);
    uint32_t stats[4] = {0, 0, 0, 0};
    std::vector<uint8_t> failed(ngroups, 0);
    std::vector<uint32_t> cdest(ngroups), csrc(grp_off[ngroups]);
    bool any_failed = false;
    for (uint32_t g = 0; g < ngroups; ++g) {
        bool f = K.wrong[grp_dest[g]] != 0;
        cdest[g] = K.canon[grp_dest[g]];
        for (uint64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
            f = f || K.wrong[grp_key[i]] != 0;
            csrc[i] = K.canon[grp_key[i]];
        }
        failed[g] = f;
        any_failed = any_failed || f;
        if (status) status[g] = f ? 0xFF : 0;
    }
    std::vector<uint32_t> end;
    hll_groups_plan(cdest.data(), grp_off, csrc.data(), failed.data(), ngroups, nkeys, &end);
    uint32_t p0 = 0;
    for (uint32_t p1 : end) {
        RBX_TRY(hg_merge_phase(c, K, grp_dest, grp_off, grp_key, failed.data(), p0, p1, st, stats));
        p0 = p1;
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) g_hllgroups_last[i] = stats[i];
    if (any_failed) return fail(RBX_E_WRONGTYPE, kHllWrongType);
    return RBX_OK;
}

// Redis HLL strings: 16-byte header ("HYLL", encoding, 3 unused, 8 cached-cardinality bytes)
// + dense registers (HLL_DENSE_SET_REGISTER layout, 6 bits each, LSB-first) or sparse opcodes.
constexpr uint64_t kHllDenseLen = 16 + 12288;

static void hll_header(uint8_t *s, int sparse, uint64_t card) {
    memcpy(s, "HYLL", 4);
    s[4] = (uint8_t)sparse;  // HLL_DENSE 0 / HLL_SPARSE 1
    s[5] = s[6] = s[7] = 0;
    for (int i = 0; i < 8; ++i) s[8 + i] = (uint8_t)(card >> (8 * i));
}

static void hll_encode_dense(const uint8_t *regs, uint8_t *p) {
    memset(p, 0, 12288);
    for (unsigned long r = 0; r < 16384; ++r) {
        const unsigned long byte = r * 6 / 8, fb = r * 6 & 7, fb8 = 8 - fb, v = regs[r];
        p[byte] |= (uint8_t)(v << fb);
        if (byte + 1 < 12288) p[byte + 1] |= (uint8_t)(v >> fb8);
    }
}

// Sparse opcodes with the fewest bytes: zero runs as ZERO (<= 64) or XZERO (65..16384), equal
// values as VAL runs of <= 4 (value 1..32).  Returns false when a register exceeds 32 (the
// sparse format cannot hold it).  Used for RBX_HLL_SPARSE exports of keys Redis holds dense
// (a sparse key exports the string it was built as, see hll_sparse_string).
static bool hll_encode_sparse(const uint8_t *regs, std::vector<uint8_t> &out) {
    out.clear();
    for (uint32_t i = 0; i < 16384;) {
        const uint8_t v = regs[i];
        uint32_t j = i + 1;
        while (j < 16384 && regs[j] == v) ++j;
        uint32_t run = j - i;
        if (v == 0) {
            if (run > 64) {
                out.push_back((uint8_t)(0x40 | ((run - 1) >> 8)));
                out.push_back((uint8_t)((run - 1) & 0xff));
            } else {
                out.push_back((uint8_t)(run - 1));
            }
        } else {
            if (v > 32) return false;
            for (; run; run -= std::min<uint32_t>(run, 4))
                out.push_back((uint8_t)(0x80 | ((v - 1) << 2) | (std::min<uint32_t>(run, 4) - 1)));
        }
        i = j;
    }
    return true;
}

// The sparse string of a key Redis holds sparse, as it was built (k_hll_sparse_replay's list):
// an XZERO opcode is two bytes, ZERO / VAL one.  The caller holds a CallScope on c->stream.
static int hll_sparse_string(rbx_ctx *c, HllState *h, std::vector<uint8_t> &out) {
    uint32_t st[kHllStateWords];
    HIP_TRY(hipMemcpyAsync(st, h->d_promoted, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out.clear();
    if (st[1] == 0) {  // createHLLObject
        out = {0x7f, 0xff};
        return RBX_OK;
    }
    std::vector<uint16_t> ops(st[1]);
    HIP_TRY(hipMemcpy(ops.data(), h->d_sp_ops, ops.size() * 2, hipMemcpyDeviceToHost));
    for (uint16_t op : ops) {
        if (op >= 0x100) out.push_back((uint8_t)(op >> 8));
        out.push_back((uint8_t)op);
    }
    if (out.size() != st[2]) return fail(RBX_E_DEVICE, "sparse HLL string length mismatch");
    return RBX_OK;
}

static int hll_export_enc(rbx_ctx *c, const std::string &name, int encoding, uint8_t *out, uint64_t cap,
                          uint64_t *len) {
    if (encoding < RBX_HLL_DENSE || encoding > RBX_HLL_AS_STORED)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "encoding must be RBX_HLL_DENSE, RBX_HLL_SPARSE or RBX_HLL_AS_STORED");
    RBX_ENTER(c, c->stream);
    std::shared_ptr<HllState> h;
    RBX_TRY(hll_get(c, name, false, c->stream, &h, nullptr));
    if (!h) {
        if (len) *len = 0;
        return RBX_OK;
    }
    if (encoding != RBX_HLL_DENSE) RBX_TRY(resolve_dense(c, h.get()));
    std::vector<uint8_t> s;
    bool sparse = false;
    if (encoding != RBX_HLL_DENSE && !h->dense) {
        std::vector<uint8_t> ops;
        RBX_TRY(hll_sparse_string(c, h.get(), ops));
        s.resize(16 + ops.size());
        memcpy(s.data() + 16, ops.data(), ops.size());
        sparse = true;
    } else {
        std::vector<uint8_t> regs(kHllBytes);
        HIP_TRY(hipMemcpyAsync(regs.data(), h->d_regs, kHllBytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (encoding == RBX_HLL_SPARSE) {
            std::vector<uint8_t> ops;
            if (!hll_encode_sparse(regs.data(), ops))
                return fail(RBX_E_ILLEGAL_ARGUMENT, "a register exceeds 32: not representable in the sparse encoding");
            s.resize(16 + ops.size());
            memcpy(s.data() + 16, ops.data(), ops.size());
            sparse = true;
        } else {
            s.resize(kHllDenseLen);
            hll_encode_dense(regs.data(), s.data() + 16);
        }
    }
    hll_header(s.data(), sparse, h->card);
    if (len) *len = s.size();
    if (out) memcpy(out, s.data(), std::min<uint64_t>(cap, s.size()));
    return RBX_OK;
}

// accepts the Redis dense and sparse encodings (isHLLObjectOrReply validation)
static int hll_import(rbx_ctx *c, const std::string &name, const uint8_t *bytes, uint64_t len) {
    if (len < 16 || memcmp(bytes, "HYLL", 4) != 0 || bytes[4] > 1) return fail(RBX_E_WRONGTYPE, kHllWrongType);
    std::vector<uint8_t> regs(kHllBytes, 0);
    std::vector<uint16_t> ops;  // sparse: the opcodes as stored (SET keeps the string)
    if (bytes[4] == 0) {
        if (len != kHllDenseLen) return fail(RBX_E_WRONGTYPE, kHllWrongType);
        const uint8_t *p = bytes + 16;
        for (unsigned long r = 0; r < 16384; ++r) {
            unsigned long byte = r * 6 / 8, fb = r * 6 & 7, fb8 = 8 - fb;
            unsigned long b0 = p[byte], b1 = byte + 1 < 12288 ? p[byte + 1] : 0;
            regs[r] = (uint8_t)(((b0 >> fb) | (b1 << fb8)) & 63);
        }
    } else {
        const uint8_t *p = bytes + 16, *end = bytes + len;
        uint64_t idx = 0;
        while (p < end) {
            uint8_t b = *p;
            uint64_t run;
            if ((b & 0xc0) == 0) {  // ZERO
                run = (b & 0x3f) + 1;
                ops.push_back(b);
                p++;
            } else if ((b & 0xc0) == 0x40) {  // XZERO
                if (p + 1 >= end) return fail(RBX_E_WRONGTYPE, kHllWrongType);
                run = (((uint64_t)(b & 0x3f) << 8) | p[1]) + 1;
                ops.push_back((uint16_t)(b << 8 | p[1]));
                p += 2;
            } else {  // VAL
                ops.push_back(b);
                run = (b & 3) + 1;
                uint8_t v = ((b >> 2) & 0x1f) + 1;
                if (idx + run > 16384) return fail(RBX_E_WRONGTYPE, kHllWrongType);
                for (uint64_t j = 0; j < run; ++j) regs[idx + j] = v;
                p++;
            }
            idx += run;
            if (idx > 16384) return fail(RBX_E_WRONGTYPE, kHllWrongType);
        }
        if (idx != 16384) return fail(RBX_E_WRONGTYPE, kHllWrongType);
    }
    RBX_ENTER(c, c->stream);
    Entry *ex = c->ks.find(name);
    std::shared_ptr<HllState> h;
    if (ex && ex->type == KType::Hll) {
        h = ex->hll;
        ex->expire_at = -1;  // SET discards the timeout
    } else {
        c->ks.generation++;
        RBX_TRY(hll_alloc(c, c->stream, &h));
        c->ks.put(name, Entry{KType::Hll, nullptr, nullptr, h});
    }
    uint64_t card = 0;
    for (int i = 0; i < 8; ++i) card |= (uint64_t)bytes[8 + i] << (8 * i);
    h->card = card;
    h->dense = bytes[4] == 0;  // SET keeps the string's encoding
    RBX_TRY(hll_ops_reserve(h.get(), ops.size()));
    // state: not promoted, the stored opcodes (a sparse string covers 16384 registers: >= 1)
    const uint32_t st[kHllStateWords] = {0u, (uint32_t)ops.size(), (uint32_t)(len - 16), 0u};
    HIP_TRY(hipMemcpyAsync(h->d_promoted, st, sizeof(st), hipMemcpyHostToDevice, c->stream));
    if (!ops.empty())
        HIP_TRY(hipMemcpyAsync(h->d_sp_ops, ops.data(), ops.size() * 2, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(h->d_regs, regs.data(), kHllBytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

static int hll_open(rbx_ctx *c, const std::string &name, int create, rbx_hll **out) {
    RBX_ENTER(c, c->stream);
    std::shared_ptr<HllState> h;
    RBX_TRY(hll_get(c, name, create != 0, c->stream, &h, nullptr));
    if (!h) return fail(RBX_E_NO_SUCH_KEY, "ERR no such key");
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = new rbx_hll{c, name, h, c->ks.generation};
    c->refs.fetch_add(1);
    return RBX_OK;
}

// ---- register packing (the exchange step of an element-partitioned HLL set) ------------------
// hlls[i]'s 16384 registers <-> d_buf[i*16384, (i+1)*16384), on `st` (both enqueue only).
static int hll_handles_regs(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n, hipStream_t st,
                            std::vector<uint8_t *> *regs) {
    regs->resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!hlls[i]) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL hll handle");
        RBX_TRY(hll_bind(c, hlls[i], true, st));
        (*regs)[i] = hlls[i]->st->d_regs;
    }
    return RBX_OK;
}

static int hll_pack_locked(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n, uint8_t *d_buf, bool unpack_max,
                           hipStream_t st) {
    std::vector<uint8_t *> regs;
    RBX_TRY(hll_handles_regs(c, hlls, n, st, &regs));
    if (!n) return RBX_OK;
    DevBuf &ptrs = c->dev->shared.ptrs;
    RBX_TRY(ptrs.reserve(n * sizeof(uint8_t *)));
    HIP_TRY(hipMemcpyAsync(ptrs.p, regs.data(), n * sizeof(uint8_t *), hipMemcpyHostToDevice, st));
    launch_hll_pack(ptrs.as<uint8_t *>(), n, d_buf, unpack_max, st);
    HIP_TRY(hipGetLastError());
    if (unpack_max) {
        // the exchange merges the other ranks' registers in: a sparse HLL's string takes them
        // as PFMERGE's write-back would (ascending registers, promotion by the same rules)
        std::vector<HllState *> hs(n);
        for (uint32_t i = 0; i < n; ++i) {
            hlls[i]->st->card |= 1ULL << 63;  // HLL_INVALIDATE_CACHE
            hs[i] = hlls[i]->st.get();
        }
        RBX_TRY(replay_merge(c, hs, st));
    }
    // `regs` is a pageable host vector: the runtime has staged it when hipMemcpyAsync returns
    return RBX_OK;
}

static int hll_pack(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n, uint8_t *d_buf, bool unpack_max, void *stream) {
    if (!c || (n && (!hlls || !d_buf))) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    return hll_pack_locked(c, hlls, n, d_buf, unpack_max, st);
}

}  // namespace rbx

using namespace rbx;

extern "C" {

int rbx_hll_add_multi(rbx_ctx *c, const char *const *names, uint32_t nseg, const uint64_t *seg_offsets,
                      const rbx_keys *elements, uint8_t *out_changed) {
    if (!c || !names || !seg_offsets) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, nseg, &v));
    return hll_add_multi(c, v, seg_offsets, elements, out_changed);
}

int rbx_hll_add_multi_n(rbx_ctx *c, const rbx_name *names, uint32_t nseg, const uint64_t *seg_offsets,
                        const rbx_keys *elements, uint8_t *out_changed) {
    if (!c || !names || !seg_offsets) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(names, nseg, &v));
    return hll_add_multi(c, v, seg_offsets, elements, out_changed);
}

int rbx_hll_add(rbx_ctx *c, const char *name, const rbx_keys *elements, int *changed) {
    if (!c || !name || !elements) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    uint64_t seg[2] = {0, elements->n};
    uint8_t ch = 0;
    RBX_TRY(hll_add_multi(c, {std::string(name)}, seg, elements, &ch));
    if (changed) *changed = ch;
    return RBX_OK;
}

int rbx_hll_count_each(rbx_ctx *c, const char *const *names, uint32_t n, uint64_t *out) {
    if (!c || (n && (!names || !out))) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, n, &v));
    return hll_count_each(c, v, out);
}

int rbx_hll_count(rbx_ctx *c, const char *const *names, uint32_t n, uint64_t *out) {
    if (!c || !names || !out || n == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(names, n, &v));
    return hll_count(c, v, out);
}

int rbx_hll_count_n(rbx_ctx *c, const rbx_name *names, uint32_t n, uint64_t *out) {
    if (!c || !names || !out || n == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(names, n, &v));
    return hll_count(c, v, out);
}

int rbx_hll_merge(rbx_ctx *c, const char *dest, const char *const *srcs, uint32_t nsrc) {
    if (!c || !dest || (nsrc && !srcs)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(cstr_names(srcs, nsrc, &v));
    return hll_merge(c, dest, v);
}

int rbx_hll_merge_n(rbx_ctx *c, rbx_name dest, const rbx_name *srcs, uint32_t nsrc) {
    if (!c || (!dest.bytes && dest.len) || (nsrc && !srcs)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::vector<std::string> v;
    RBX_TRY(names_of(srcs, nsrc, &v));
    return hll_merge(c, name_of(dest), v);
}

int rbx_hll_export_enc(rbx_ctx *c, const char *name, int encoding, uint8_t *out, uint64_t cap, uint64_t *len) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_export_enc(c, name, encoding, out, cap, len);
}

int rbx_hll_export_enc_n(rbx_ctx *c, rbx_name name, int encoding, uint8_t *out, uint64_t cap, uint64_t *len) {
    if (!c || (!name.bytes && name.len)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_export_enc(c, name_of(name), encoding, out, cap, len);
}

int rbx_hll_export(rbx_ctx *c, const char *name, uint8_t *out, uint64_t cap, uint64_t *len) {
    return rbx_hll_export_enc(c, name, RBX_HLL_DENSE, out, cap, len);
}

int rbx_hll_import(rbx_ctx *c, const char *name, const uint8_t *bytes, uint64_t len) {
    if (!c || !name || !bytes) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_import(c, name, bytes, len);
}

int rbx_hll_import_n(rbx_ctx *c, rbx_name name, const uint8_t *bytes, uint64_t len) {
    if (!c || (!name.bytes && name.len) || !bytes) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_import(c, name_of(name), bytes, len);
}

int rbx_hll_delete(rbx_ctx *c, const char *name, int *deleted) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_del(c->ks, {std::string(name)}, deleted);
}

int rbx_hll_exists(rbx_ctx *c, const char *name, int *exists) {
    if (!c || !name || !exists) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return ks_exists(c->ks, {std::string(name)}, exists);
}

int rbx_hll_open(rbx_ctx *c, const char *name, int create, rbx_hll **out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_open(c, name, create, out);
}

int rbx_hll_open_n(rbx_ctx *c, rbx_name name, int create, rbx_hll **out) {
    if (!c || (!name.bytes && name.len) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_open(c, name_of(name), create, out);
}

int rbx_hll_close(rbx_hll *h) {
    if (!h) return RBX_OK;
    rbx_ctx *c = h->ctx;
    {
        std::lock_guard<std::recursive_mutex> g(c->ks.mu);
        delete h;
    }
    ctx_release(c);
    return RBX_OK;
}

int rbx_hll_registers_dev(rbx_hll *h, void **d_regs) {
    if (!h || !d_regs) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    rbx_ctx *c = h->ctx;
    RBX_ENTER(c, c->stream);
    RBX_TRY(hll_bind(c, h, true, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // a re-created HLL's zero fill lands first
    *d_regs = h->st->d_regs;
    return RBX_OK;
}

int rbx_hll_add_multi_dev(rbx_ctx *c, rbx_hll *const *hlls, uint32_t nseg, const uint64_t *d_seg_offsets,
                          const uint64_t *h_seg_offsets, const rbx_keys *d_elements, uint32_t *d_changed,
                          void *stream) {
    (void)d_seg_offsets;
    if (!c || !hlls || !h_seg_offsets || !d_changed) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(validate_keys(d_elements));
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    std::vector<HllState *> hl(nseg);
    for (uint32_t s = 0; s < nseg; ++s) {
        if (!hlls[s]) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL hll handle");
        RBX_TRY(hll_bind(c, hlls[s], true, st));
        hl[s] = hlls[s]->st.get();
        hl[s]->card |= 1ULL << 63;  // conservatively invalidate (the flags are device-side)
    }
    return pfadd_run(c, hl, h_seg_offsets, h_seg_offsets + 1, nullptr, keys_dev(d_elements), d_changed, st);
}

int rbx_hll_count_each_handles(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n, uint64_t *out) {
    if (!c || (n && (!hlls || !out))) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    std::vector<HllState *> hl(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (hlls[i]) RBX_TRY(hll_bind(c, hlls[i], false, c->stream));
        hl[i] = hlls[i] ? hlls[i]->st.get() : nullptr;
    }
    return pfcount_each(c, hl, out, c->stream);
}

int rbx_hll_pack_registers(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n, void *d_buf, void *stream) {
    return hll_pack(c, hlls, n, (uint8_t *)d_buf, false, stream);
}

int rbx_hll_unpack_max_registers(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n, const void *d_buf, void *stream) {
    return hll_pack(c, hlls, n, (uint8_t *)d_buf, true, stream);
}

int rbx_hll_stream(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key, const uint8_t *cmd_op,
                   const uint64_t *cmd_elem, uint64_t n, const rbx_keys *elements, uint64_t *replies, uint8_t *status) {
    RBX_TRY(hll_stream_check(c, names, nkeys, cmd_key, cmd_op, cmd_elem, n, elements));
    if (n == 0) return RBX_OK;  // no command is sent
    return hll_stream(c, names, nkeys, cmd_key, cmd_op, cmd_elem, n, elements, replies, status, false, c->stream);
}

int rbx_hll_stream_dev(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *cmd_key, const uint8_t *cmd_op,
                       const uint64_t *cmd_elem, uint64_t n, const rbx_keys *d_elements, uint64_t *replies,
                       uint8_t *status, void *stream) {
    RBX_TRY(hll_stream_check(c, names, nkeys, cmd_key, cmd_op, cmd_elem, n, d_elements));
    if (n == 0) return RBX_OK;
    return hll_stream(c, names, nkeys, cmd_key, cmd_op, cmd_elem, n, d_elements, replies, status, true,
                      pick_stream(c, stream));
}

int rbx_bench_hllstream_last(uint32_t out[4]) {
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    for (int i = 0; i < 4; ++i) out[i] = g_hllstream_last[i];
    return RBX_OK;
}

static int hll_groups_args(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint64_t *grp_off,
                           const uint32_t *grp_key, uint32_t ngroups, bool need_entries) {
    RBX_TRY(stream_names_check(c, names, nkeys));
    if (const char *what = hll_groups_check(grp_off, grp_key, ngroups, nkeys, need_entries))
        return fail(RBX_E_ILLEGAL_ARGUMENT, what);
    return RBX_OK;
}

int rbx_hll_count_groups(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint64_t *grp_off,
                         const uint32_t *grp_key, uint32_t ngroups, uint64_t *out, uint8_t *status) {
    RBX_TRY(hll_groups_args(c, names, nkeys, grp_off, grp_key, ngroups, true));
    if (ngroups == 0) return RBX_OK;  // no command is sent
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return hll_count_groups(c, names, nkeys, grp_off, grp_key, ngroups, out, status);
}

int rbx_hll_merge_groups(rbx_ctx *c, const rbx_name *names, uint32_t nkeys, const uint32_t *grp_dest,
                         const uint64_t *grp_off, const uint32_t *grp_key, uint32_t ngroups, uint8_t *status) {
    RBX_TRY(hll_groups_args(c, names, nkeys, grp_off, grp_key, ngroups, false));
    if (ngroups == 0) return RBX_OK;
    if (!grp_dest) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    for (uint32_t g = 0; g < ngroups; ++g)
        if (grp_dest[g] >= nkeys) return fail(RBX_E_ILLEGAL_ARGUMENT, "a group's destination is not below nkeys");
    return hll_merge_groups(c, names, nkeys, grp_dest, grp_off, grp_key, ngroups, status);
}

int rbx_bench_hllgroups_last(uint32_t out[4]) {
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    for (int i = 0; i < 4; ++i) out[i] = g_hllgroups_last[i];
    return RBX_OK;
}

// ---- RCCL -----------------------------------------------------------------------------------
int rbx_rccl_unique_id(uint8_t out[128]) {
    if (!out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(RBX_E_DEVICE, ncclGetErrorString(r));
    memcpy(out, id.internal, 128);
    return RBX_OK;
}

int rbx_rccl_init(rbx_ctx *c, const uint8_t id[128], int nranks, int rank) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    RBX_TRY(set_device(c));
    if (c->comm) return fail(RBX_E_ILLEGAL_STATE, "rbx_rccl_init has already been called");
    ncclUniqueId u;
    memcpy(u.internal, id, 128);
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, u, rank);
    if (r != ncclSuccess) return fail(RBX_E_DEVICE, ncclGetErrorString(r));
    c->nranks = nranks;
    c->rank = rank;
    return RBX_OK;
}

// the communicator as RCCL sees it (ncclCommCount / ncclCommUserRank)
int rbx_rccl_info(rbx_ctx *c, int *nranks, int *rank) {
    if (!c) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    if (!c->comm) return fail(RBX_E_ILLEGAL_STATE, "rbx_rccl_init has not been called");
    int n = 0, r = 0;
    ncclResult_t e = ncclCommCount(c->comm, &n);
    if (e == ncclSuccess) e = ncclCommUserRank(c->comm, &r);
    if (e != ncclSuccess) return fail(RBX_E_DEVICE, ncclGetErrorString(e));
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    return RBX_OK;
}

// Every rank issues exactly ONE ncclAllReduce of n x 16384 bytes whatever its register pool
// layout: the registers are packed in the caller's (name) order into one contiguous buffer,
// max-reduced in place, and max-merged back.  (Coalescing "adjacent" pool blocks would make the
// number and sizes of the collectives depend on each rank's allocation history, and RCCL would
// pair mismatched calls.)  The pack/unpack kernels move 2 x 2 x n x 16 KiB of HBM (~0.1 ms for
// the 163.84 MB of C4), next to the all-reduce itself.
int rbx_hll_allreduce_max(rbx_ctx *c, rbx_hll *const *hlls, uint32_t n) {
    if (!c || (n && !hlls)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    if (!c->comm) return fail(RBX_E_ILLEGAL_STATE, "rbx_rccl_init has not been called");
    const size_t bytes = (size_t)n * kHllBytes;
    RBX_TRY(c->dev->hll.pack.reserve(std::max<size_t>(bytes, 16)));
    uint8_t *buf = c->dev->hll.pack.as<uint8_t>();
    RBX_TRY(hll_pack_locked(c, hlls, n, buf, false, c->stream));
    ncclResult_t r = ncclAllReduce(buf, buf, bytes, ncclUint8, ncclMax, c->comm, c->stream);
    if (r != ncclSuccess) return fail(RBX_E_DEVICE, ncclGetErrorString(r));
    return hll_pack_locked(c, hlls, n, buf, true, c->stream);
}

// PFMERGE's input from another GPU: dst_name on dst := src_name on src (registers, encoding,
// cached cardinality and promotion word), device to device.  A missing source deletes dst_name.
int rbx_hll_copy_to(rbx_ctx *src, rbx_name src_name, rbx_ctx *dst, rbx_name dst_name) {
    if (!src || !dst || (!src_name.bytes && src_name.len) || (!dst_name.bytes && dst_name.len))
        return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    const std::string sn = name_of(src_name), dn = name_of(dst_name);
    if (src == dst && sn == dn) return RBX_OK;
    std::unique_lock<std::recursive_mutex> l1(src->ks.mu, std::defer_lock), l2(dst->ks.mu, std::defer_lock);
    if (src == dst) l1.lock();
    else std::lock(l1, l2);
    RBX_TRY(set_device(src));
    if (dst->shut) return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    Entry *e = src->ks.find(sn);
    if (e && e->type != KType::Hll) return fail(RBX_E_WRONGTYPE, kHllWrongType);
    if (!e) {
        dst->ks.erase(dn);
        return RBX_OK;
    }
    std::shared_ptr<HllState> sh = e->hll;
    RBX_TRY(quiesce(src));
    RBX_ENTER(dst, dst->stream);  // its lock is held already (recursive): the device and the scratch order
    Entry *de = dst->ks.find(dn);
    if (de && de->type != KType::Hll) {
        dst->ks.erase(dn);
        de = nullptr;
    }
    std::shared_ptr<HllState> h;
    if (de) {
        h = de->hll;
        de->expire_at = -1;  // SET semantics
    } else {
        RBX_TRY(hll_alloc(dst, dst->stream, &h));
        dst->ks.put(dn, Entry{KType::Hll, nullptr, nullptr, h});
        dst->ks.generation++;
    }
    h->card = sh->card;
    h->dense = sh->dense;
    // the source's opcode count (its state word [1]) sizes the copy and the destination's list
    uint32_t sst[kHllStateWords];
    HIP_TRY(hipSetDevice(src->device));
    HIP_TRY(hipMemcpy(sst, sh->d_promoted, sizeof(sst), hipMemcpyDeviceToHost));
    HIP_TRY(hipSetDevice(dst->device));
    RBX_TRY(hll_ops_reserve(h.get(), sst[1]));
    HIP_TRY(hipMemcpyPeerAsync(h->d_regs, dst->device, sh->d_regs, src->device, kHllBytes, dst->stream));
    HIP_TRY(hipMemcpyPeerAsync(h->d_promoted, dst->device, sh->d_promoted, src->device, kHllStateWords * 4, dst->stream));
    if (sst[1])
        HIP_TRY(hipMemcpyPeerAsync(h->d_sp_ops, dst->device, sh->d_sp_ops, src->device, (size_t)sst[1] * 2, dst->stream));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    return RBX_OK;
}

}  // extern "C"
