// api_bloom.cpp -- single-filter Bloom: add() (first-setter table or partitioned), contains() (direct or
// partitioned), host-buffer calls through the staging tiers, BITCOUNT / count(), handles and the _dev path.
#include <cmath>
#include <cstring>

#include "api_staging.h"
#include "bucket_common.h"
#include "tunables.h"

namespace rbx {

static std::atomic<uint64_t> g_handle_serial{1};  // rbx_bloom::serial

// add(): `int c` -- add(Collection) counts in a Java int, contains(Collection) in a long
static uint64_t reply_count(bool is_add, uint64_t cnt) { return is_add ? (uint64_t)(int64_t)(int32_t)cnt : cnt; }

// =====================================================================================
// add(): chunked probe/commit over the first-setter table
// =====================================================================================
static int run_add_table(rbx_ctx *c, const KeysDev &keys, const FilterDesc *d_filt, const uint64_t *d_seg_off,
                         uint32_t nseg, const FilterDesc &single, uint32_t kmax, uint8_t *d_out_new,
                         unsigned long long *d_count, unsigned long long *d_seg_counts, hipStream_t st) {
    if (keys.n == 0) return RBX_OK;
    const uint64_t k = std::max<uint32_t>(kmax, 1);
    const bool narrow = d_filt == nullptr && kmax <= 32;
    // chunk so that pairs per chunk <= 2^26 (table <= 2^27 entries at load <= 1/2)
    uint64_t chunk = std::min<uint64_t>(keys.n, (1ULL << 26) / k);
    chunk = std::max<uint64_t>(chunk, 1);
    const size_t zbytes = kmax <= 32 ? chunk * 4 : chunk * (size_t)kmax;
    FirstSetterTable &fst = c->dev->fst;
    RBX_TRY(c->dev->shared.zmask.reserve(zbytes));
    const int fl = fast_len(keys);
    for (uint64_t base = 0; base < keys.n; base += chunk) {
        const uint64_t nch = std::min<uint64_t>(chunk, keys.n - base);
        AddChunkArgs a{};
        if (narrow) {
            uint32_t lg = 16;
            while (lg < 27 && (1ULL << lg) < 2 * nch * k) ++lg;
            RBX_TRY(fst.use_narrow(lg, st));
            a.log2cap = lg;
        } else {
            RBX_TRY(fst.ensure(nch * k, st));
            a.log2cap = fst.log2cap;
            a.epoch = fst.epoch;
        }
        a.keys = keys;
        a.base = base;
        a.nchunk = nch;
        a.filt = d_filt;
        a.seg_off = d_seg_off;
        a.nseg = nseg;
        a.tile_seg0 = c->dev->shared.tile_segs.as<uint32_t>();
        a.single = single;
        a.table = fst.table.as<HTEntry>();
        a.zmask = c->dev->shared.zmask.as<uint32_t>();
        a.kmax = kmax;
        a.out_new = d_out_new;
        a.count = d_count;
        a.seg_counts = d_seg_counts;
        a.narrow = narrow;
        launch_bloom_add_chunk(a, fl, st);
        HIP_TRY(hipGetLastError());
    }
    return RBX_OK;
}

// Partitioned add (add_partitioned.hip) for one large filter.  Mode: 0 never, 1 whenever
// k <= 16, 2 (default) when the bitmap is >= 8 MiB and the batch has >= max(2^17, size / 2^12)
// keys.  The region pass reads and writes every touched region of the bitmap, so its floor
// grows with the bitmap (0.7 ms at 512 MiB) while the table path's cost grows with the batch
// (0.7 us per 1K keys): crossovers ~150K keys at 12-32 MiB, ~1M at 512 MiB
// (tools/microbench.py addsweep, profiles/r02/r02h_addsweep_table_vs_partitioned.jsonl).
static bool use_add_partitioned(uint64_t size, uint32_t k, uint64_t n) {
    if (k < 1 || k > 16 || size > (1ULL << 32) || size < (1ULL << 15)) return false;
    if (g_tune.add_partition_mode == 0) return false;
    if (g_tune.add_partition_mode == 1) return true;
    return size >= (1ULL << 26) && n >= std::max<uint64_t>(1ULL << 17, size >> 12);
}

// the 16 phase-time words of the profiling build's stamp diagnostics (rbx_bench_add_stamps), zeroed once
static int phase_stamps(rbx_ctx *c, hipStream_t st, unsigned long long **out) {
    RBX_TRY(c->dev->pa.stamps.reserve_filled(16 * 8, 0, st, false));
    *out = c->dev->pa.stamps.as<unsigned long long>();
    return RBX_OK;
}

static KeysDev keys_slice(const KeysDev &k, uint64_t i0, uint64_t n) {
    KeysDev s = k;
    s.n = n;
    if (k.offsets) s.offsets = k.offsets + i0;  // offsets stay absolute (off_base unchanged)
    else s.bytes = k.bytes + i0 * k.stride;
    return s;
}

static int run_add_partitioned(rbx_ctx *c, const KeysDev &keys, const FilterDesc &f, uint8_t *d_out_new,
                               unsigned long long *d_count, hipStream_t st) {
    const uint32_t k = f.k;
    const uint64_t size = f.mp.size;
    const uint32_t nregions = (uint32_t)((size + (1ULL << kBaRegionBits) - 1) >> kBaRegionBits);
    uint32_t L = 0;
    while ((1ULL << L) < nregions) ++L;
    // two radix passes: stage 1 into 2^(L - f3) <= 256 buckets, one rebucket of fan-out 2^f3 <= 256
    const uint32_t f3 = std::min<uint32_t>(8, L);
    const uint32_t s3 = kBaRegionBits, s1 = s3 + f3;
    const uint32_t ncoarse = (uint32_t)((size + (1ULL << s1) - 1) >> s1);  // <= 256 for size <= 2^32
    // chunk: key ids < 2^26 and the expected pairs per region (x 1.3 slack) within the block's registers
    const double per_region = (double)k * (double)(1ULL << kBaRegionBits) / (double)size;  // pairs per key
    uint64_t chunk = (uint64_t)((kBaMaxRegionPairs - 512) / 1.3 / per_region);
    chunk = std::min<uint64_t>(chunk, 1ULL << 26);
    const uint64_t nch = (keys.n + chunk - 1) / chunk;
    chunk = (keys.n + nch - 1) / nch;
    const double pairs = (double)chunk * k;
    auto cap_of = [&](uint32_t shift, double slack, uint64_t add, uint64_t round) {
        const double frac = std::min(1.0, (double)(1ULL << shift) / (double)size);
        uint64_t cap = (uint64_t)(pairs * frac * slack) + add;
        return (cap + round - 1) / round * round;
    };
    PartitionedAddScratch &pa = c->dev->pa;
    const uint64_t cap1 = cap_of(s1, 1.15 / kBaSub, 8192, 8192);
    const uint64_t cap3 = std::min<uint64_t>(kBaMaxRegionPairs, cap_of(s3, 1.3, 256, 64));
    RBX_TRY(pa.p1.reserve((uint64_t)ncoarse * kBaSub * cap1 * 8));
    RBX_TRY(pa.p2.reserve((uint64_t)nregions * cap3 * 8));
    const uint32_t nranges = (uint32_t)((chunk + (1ULL << kBaKeyRangeBits) - 1) >> kBaKeyRangeBits);
    const uint64_t cap_rec = (uint64_t)k << kBaKeyRangeBits;  // a range's owner records <= 2^20 keys x k
    RBX_TRY(pa.recs.reserve((uint64_t)nranges * cap_rec * 4));
    const uint64_t ncnt = (uint64_t)ncoarse * kBaSub + nregions + nranges + 2;
    RBX_TRY(pa.cnt.reserve(ncnt * 4));
    const uint64_t nbw = (uint64_t)nranges << (kBaKeyRangeBits - 5);  // whole ranges (the records kernel's images)
    RBX_TRY(pa.bits.reserve(nbw * 4));
    // per-key non-owner counters (one byte per key; k_ba_final zeroes what it read): zeroed once
    // when (re)allocated
    RBX_TRY(pa.ctr.reserve_filled(nbw * 32, 0, st));
    const int fl = fast_len(keys);
    for (uint64_t base = 0; base < keys.n; base += chunk) {
        BaArgs a{};
        a.keys = keys;
        a.base = base;
        a.nchunk = std::min<uint64_t>(chunk, keys.n - base);
        a.f = f;
        a.ncoarse = ncoarse;
        a.s1 = s1;
        a.s3 = s3;
        a.f3 = f3;
        a.nregions = nregions;
        a.cap1 = cap1;
        a.cap3 = cap3;
        a.p1 = pa.p1.as<unsigned long long>();
        a.p3 = pa.p2.as<unsigned long long>();
        a.cnt1 = pa.cnt.as<uint32_t>();
        a.cnt3 = a.cnt1 + (uint64_t)ncoarse * kBaSub;
        a.rec_cnt = a.cnt3 + nregions;
        a.overflow = a.rec_cnt + nranges;
        a.mode = a.overflow + 1;
        a.recs = pa.recs.as<uint32_t>();
        a.cap_rec = cap_rec;
        a.nranges = (uint32_t)((a.nchunk + (1ULL << kBaKeyRangeBits) - 1) >> kBaKeyRangeBits);
        a.record_policy = (uint32_t)g_tune.add_record_policy;
        a.new_bits = pa.bits.as<uint32_t>();
        a.ctr = pa.ctr.as<uint32_t>();
        a.nwords4 = (size + 127) / 128 * 4;
        a.out_new = d_out_new;
        a.count = d_count;
        a.diag = (uint32_t)g_tune.add_partition_diag;
        if (a.diag & 64) RBX_TRY(phase_stamps(c, st, &a.stamps));
        // the counters (but the mode word) and new_bits are zeroed by k_ba_mode, the chunk's first kernel
        launch_add_partitioned_chunk(a, fl, st);
        HIP_TRY(hipGetLastError());
        unsigned long long *w = c->dev->stage.words();  // pinned: no staging copy
        HIP_TRY(hipMemcpyAsync(w, a.overflow, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t ovf;
        memcpy(&ovf, w, 4);
        if (ovf) {
            // a bucket overflowed before any bitmap word changed: this chunk on the table path
            const KeysDev sub = keys_slice(keys, base, a.nchunk);
            RBX_TRY(run_add_table(c, sub, nullptr, nullptr, 0, f, k, d_out_new ? d_out_new + base : nullptr, d_count,
                                  nullptr, st));
        }
    }
    return RBX_OK;
}

// Small single-filter adds (<= add_single_seg_keys keys, k <= 16): the per-segment kernel on one segment --
// one workgroup, the batch's first setters in LDS (§3.9) -- instead of the table path's memset, probe and
// commit: one launch.  Its plain word stores need the bitmap to itself, which the context's call order
// gives (every call waits for the previous one's stream, CallScope).
static void launch_seg_single(const KeysDev &keys, const FilterDesc &f, uint8_t *d_out_new,
                              unsigned long long *d_count, hipStream_t st) {
    MaddSegArgs a{};
    a.keys = keys;
    a.single = f;
    a.kmax = f.k;
    a.segmax = kSegMaxKeys;  // >= keys.n: the `big` flag stays unused
    a.out_new = d_out_new;
    a.seg_counts = d_count;
    launch_madd_seg(a, fast_len(keys), st);
}

int run_add(rbx_ctx *c, const KeysDev &keys, const FilterDesc *d_filt, const uint64_t *d_seg_off, uint32_t nseg,
            const FilterDesc &single, uint32_t kmax, uint8_t *d_out_new, unsigned long long *d_count,
            unsigned long long *d_seg_counts, hipStream_t st) {
    if (keys.n == 0) return RBX_OK;
    if (d_filt == nullptr && keys.n == 1 && single.k <= 16 && g_tune.add_one) {
        launch_bloom_one(true, keys, fast_len(keys), single, d_out_new, d_count, nullptr, 0, st);
        HIP_TRY(hipGetLastError());
        return RBX_OK;
    }
    if (d_filt == nullptr && single.k <= 16 && keys.n <= g_tune.seg_single_keys) {
        launch_seg_single(keys, single, d_out_new, d_count, st);
        HIP_TRY(hipGetLastError());
        return RBX_OK;
    }
    if (d_filt == nullptr && use_add_partitioned(single.mp.size, single.k, keys.n))
        return run_add_partitioned(c, keys, single, d_out_new, d_count, st);
    return run_add_table(c, keys, d_filt, d_seg_off, nseg, single, kmax, d_out_new, d_count, d_seg_counts, st);
}

// Partitioned contains (contains_partitioned.hip) for one large filter.  Mode: 0 never,
// 1 whenever k in [2, 16], 2 (default) when the bitmap is >= 256 MiB and the batch >= 4M keys.
// Below 256 MiB the direct kernel measured faster (its early exit costs ~1 gather per absent
// key, and smaller bitmaps gather partly from L2/MALL); DESIGN.md §3.6 has the size sweep.
static bool use_partitioned(uint64_t size, uint32_t k, uint64_t n) {
    if (k < 2 || k > 16 || size > (1ULL << 32)) return false;
    if (g_tune.partition_mode == 0) return false;
    if (g_tune.partition_mode == 1) return true;
    return size >= (1ULL << 31) && n >= (1ULL << 22);
}

static int run_contains_partitioned(rbx_ctx *c, const KeysDev &keys, const FilterDesc &f, uint8_t *d_out,
                                    unsigned long long *d_count, hipStream_t st) {
    const uint32_t k = f.k;
    const uint64_t size = f.mp.size;
    const uint32_t nb = (uint32_t)((size + (1ULL << kBkBucketBits) - 1) >> kBkBucketBits);
    // Chunk rule (bk_entry.h): at most grid * 2^19 keys, so a block-local key index fits an entry's 19 bits
    // (2^27 at the default grid: key ids fit 27 bits), and a chunk's entries stay <= 2^30.  A smaller
    // grid ("contains_stage1_grid", tests) splits the batch into more chunks.
    const uint32_t gcap = std::min<uint32_t>(std::max<uint32_t>(g_tune.stage1_grid, 1u), kBkMaxGrid1);
    const uint64_t chunk = bk_chunk_keys(keys.n, gcap, k);
    const uint64_t ngroups = (chunk + 63) / 64;
    // Segment capacity in entries, whole 64-byte lines of 12: bk_seg_cap has the Poisson bound.
    const uint64_t g0 = bk_grid(chunk, gcap);
    const uint64_t capS = bk_seg_cap(chunk, (uint32_t)g0, k, size);
    PartitionedContainsScratch &pc = c->dev->pc;
    RBX_TRY(pc.bits.reserve(ngroups * 16));
    const uint32_t nmranges = (uint32_t)((chunk + (1ULL << kBkMissRangeBits) - 1) >> kBkMissRangeBits);
    // miss records: sized for 2 per key (C2-like batches hold ~0.2); beyond that the probe falls
    // back to a direct atomicOr per clear bit, so the answer never depends on the capacity
    const uint64_t capm = 2ULL << kBkMissRangeBits;
    RBX_TRY(pc.mrec.reserve((uint64_t)nmranges * capm * 4));
    RBX_TRY(pc.cnt.reserve((256 + (uint64_t)nb * g0) * 4));  // mcnt, segment counts
    RBX_TRY(pc.pairs.reserve(bk_seg_line(0, (uint32_t)g0, nb, capS) * kBkLineBytes));  // nb * g0 segments, in lines
    const int fl = fast_len(keys);
    for (uint64_t base = 0; base < keys.n; base += chunk) {
        PcArgs a{};
        a.keys = keys;
        a.base = base;
        a.nchunk = std::min<uint64_t>(chunk, keys.n - base);
        a.bm = f.bm;
        a.mp = f.mp;
        a.k = k;
        a.nb = nb;
        a.grid1 = bk_grid(a.nchunk, gcap);  // <= g0, and nchunk <= grid1 * 2^19
        a.capS = capS;
        a.nwords4 = (size + 127) / 128 * 4;
        a.alive = pc.bits.as<unsigned long long>();
        a.miss = a.alive + ngroups;
        a.mcnt = pc.cnt.as<uint32_t>();
        a.segcnt = a.mcnt + 256;
        a.pairs = pc.pairs.as<unsigned long long>();
        a.mrec = pc.mrec.as<uint32_t>();
        a.capm = capm;
        a.nmranges = (uint32_t)((a.nchunk + (1ULL << kBkMissRangeBits) - 1) >> kBkMissRangeBits);
        a.out = d_out;
        a.count = d_count;
        a.flags = (uint32_t)g_tune.partition_flags;
        if (a.flags & 64) RBX_TRY(phase_stamps(c, st, &a.stamps));
        HIP_TRY(hipMemsetAsync(a.miss, 0, ngroups * 8, st));
        HIP_TRY(hipMemsetAsync(a.mcnt, 0, 256 * 4, st));
        launch_contains_partitioned_chunk(a, fl, st);
        HIP_TRY(hipGetLastError());
    }
    return RBX_OK;
}

// contains over device keys for one filter: direct (staged early exit) or partitioned
static int run_contains(rbx_ctx *c, const KeysDev &keys, const FilterDesc &f, uint8_t *d_out,
                        unsigned long long *d_count, hipStream_t st) {
    if (use_partitioned(f.mp.size, f.k, keys.n)) return run_contains_partitioned(c, keys, f, d_out, d_count, st);
    launch_bloom_contains(keys, fast_len(keys), f.bm, f.mp, f.k, d_out, d_count, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

FilterDesc desc_of(const Bitmap &b, uint64_t size, uint32_t k, uint32_t fid) {
    FilterDesc f{};
    f.bm = b.d_words;
    f.redis_len = b.d_len;
    f.mp = make_mod_params(size);
    f.k = k;
    f.fid = fid;
    return f;
}

// add / contains of a filter whose |size| exceeds 2^32 bits (tryInit with a negative
// expectedInsertions, M/RedissonBloomFilter.java:262-277), with the reference's semantics: indexes
// are taken mod |size| in 64 bits; a SETBIT / GETBIT past the Redis offset limit is an error reply
// that leaves the key alone while every other command of the batch runs; the call then fails with
// RBX_E_REDIS (RedisException) -- an add has set every in-range bit.  Without such an index the
// replies are the in-order ones.  Chunks run in key order (each sees the previous chunks' bits).
static int bloom_wide_op(rbx_ctx *c, const rbx_keys *keys, uint64_t m, uint32_t k, Bitmap *bm, uint8_t *out_flags,
                         uint64_t *out_count, bool is_add) {
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d_count = c->dev->shared.counters.as<unsigned long long>();
    auto *d_oob = d_count + 4;
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_oob, 0, 8, c->stream));
    uint8_t *d_out;
    RBX_TRY(out_flags_dev(c, out_flags, keys->n, &d_out));
    HIP_TRY(hipStreamSynchronize(c->stream));
    RBX_TRY(pipelined_host_batches(c, keys, c->stream, [&](const KeysDev &dk, uint64_t i0) -> int {
        // Sub-chunks of <= 2^29 / k keys, run in key order (each sees the previous one's bits), so
        // the first-setter table (>= 2x the sub-chunk's bit indexes) stays <= 2^30 entries (8 GiB)
        // and its 32-bit slot mask well-defined however short the keys (a staging
        // chunk of empty keys is unbounded in count).
        uint64_t sub = std::max<uint64_t>(1, (1ULL << 29) / k);
        if (g_tune.wide_subchunk) sub = std::min<uint64_t>(sub, g_tune.wide_subchunk);
        for (uint64_t j0 = 0; j0 < dk.n; j0 += sub) {
            KeysDev sk = dk;
            sk.n = std::min<uint64_t>(sub, dk.n - j0);
            if (dk.offsets) sk.offsets = dk.offsets + j0;
            else sk.bytes = dk.bytes + j0 * dk.stride;
            uint32_t tl = 10;  // table >= 2x the sub-chunk's bit indexes
            while ((1ULL << tl) < 2 * sk.n * k) ++tl;
            if (tl > 30) return fail(RBX_E_ILLEGAL_ARGUMENT, "wide-filter table past 2^30 entries");
            unsigned long long *table = nullptr;
            if (is_add) {
                RBX_TRY(c->dev->shared.wide_table.reserve(8ULL << tl));
                table = c->dev->shared.wide_table.as<unsigned long long>();
                HIP_TRY(hipMemsetAsync(table, 0xff, 8ULL << tl, c->stream));
            }
            launch_bloom_wide(sk, m, k, bm ? bm->d_words : nullptr, bm ? bm->d_len : nullptr, table, tl, is_add,
                              d_out ? d_out + i0 + j0 : nullptr, d_count, d_oob, c->stream);
            HIP_TRY(hipGetLastError());
        }
        return RBX_OK;
    }));
    int rc;
    const uint64_t oob = read_dev_u64(c, d_oob, &rc);
    RBX_TRY(rc);
    if (oob) return fail(RBX_E_REDIS, "ERR bit offset is not an integer or out of range");
    if (out_flags) HIP_TRY(hipMemcpyAsync(out_flags, d_out, keys->n, hipMemcpyDeviceToHost, c->stream));
    const uint64_t cnt = read_dev_u64(c, d_count, &rc);
    RBX_TRY(rc);
    if (out_count) *out_count = reply_count(is_add, cnt);
    return RBX_OK;
}

static int bloom_host_small(rbx_ctx *c, const FilterDesc &f, uint32_t k, const rbx_keys *keys, uint8_t *out_flags,
                            uint64_t *out_count, bool is_add) {
    SmallStage s;
    RBX_TRY(small_stage(c, keys, 8, &s));
    const uint64_t n = keys->n;
    uint8_t *d_out;
    RBX_TRY(out_flags_dev(c, out_flags, n, &d_out));
    auto *d_count = (unsigned long long *)s.dp;
    const int rc = is_add ? run_add(c, s.dk, nullptr, nullptr, 0, f, k, d_out, d_count, nullptr, c->stream)
                          : run_contains(c, s.dk, f, d_out, d_count, c->stream);
    (void)hipEventRecord(c->dev->stage.ev_done[0], c->stream);  // slot 0 read by what was queued, whatever rc
    if (rc != RBX_OK) return small_fail(c, rc);
    // the readback lands in the pinned block: its upload precedes it on the stream
    HIP_TRY(hipMemcpyAsync(s.hp, s.dp, 8, hipMemcpyDeviceToHost, c->stream));
    if (out_flags) HIP_TRY(hipMemcpyAsync(s.tail_h, d_out, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out_flags) memcpy(out_flags, s.tail_h, n);
    uint64_t cnt;
    memcpy(&cnt, s.hp, 8);
    if (out_count) *out_count = reply_count(is_add, cnt);
    return RBX_OK;
}

static int tiny_one(rbx_ctx *c, const FilterDesc &f, const KeysDev &dk, bool is_add) {
    const uint32_t seq = tiny_next_seq(c);
    uint8_t *blk = c->dev->stage.pin_tiny_dev;
    launch_bloom_one(is_add, dk, fast_len(dk), f, blk, nullptr, (uint32_t *)(blk + kTinyDoneAt), seq, c->stream);
    return tiny_wait(c, RBX_OK, seq, true);
}

static int bloom_host_tiny(rbx_ctx *c, const FilterDesc &f, uint32_t k, const rbx_keys *keys, uint8_t *out_flags,
                           uint64_t *out_count, bool is_add) {
    const KeysDev dk = tiny_stage(c, keys);
    uint8_t *d_flags = c->dev->stage.pin_tiny_dev;
    const bool spin = g_tune.tiny_spin;  // once per call
    if (keys->n == 1 && f.k <= 16 && spin && (!is_add || g_tune.add_one)) {
        RBX_TRY(tiny_one(c, f, dk, is_add));
        const uint8_t v = c->dev->stage.tiny()[0];
        if (out_flags) out_flags[0] = v;
        if (out_count) *out_count = v;
        return RBX_OK;
    }
    RBX_TRY(tiny_done(c, is_add ? run_add(c, dk, nullptr, nullptr, 0, f, k, d_flags, nullptr, nullptr, c->stream)
                                  : run_contains(c, dk, f, d_flags, nullptr, c->stream), spin));
    const uint8_t *fl = c->dev->stage.tiny();
    uint64_t cnt = 0;
    for (uint64_t i = 0; i < keys->n; ++i) cnt += fl[i];
    if (out_flags) memcpy(out_flags, fl, keys->n);
    if (out_count) *out_count = reply_count(is_add, cnt);
    return RBX_OK;
}

static int bloom_host_op(rbx_ctx *c, const std::string &name, int64_t size, uint32_t k, const rbx_keys *keys,
                         uint8_t *out_flags, uint64_t *out_count, bool is_add) {
    RBX_TRY(validate_keys(keys));
    RBX_ENTER(c, c->stream);
    // add()/contains() first read the config if the caller has none cached (:106-108)
    if (size == 0) {
        BloomConfig cfg;
        RBX_TRY(ks_get_config(c->ks, name, &cfg));
        size = cfg.size;
        k = cfg.k;
    }
    RBX_TRY(ks_config_check(c->ks, name, size, k));
    if (keys->n == 0) return fail(RBX_E_ARITHMETIC, "/ by zero");
    std::shared_ptr<Bitmap> bm;
    if (size_bits(size) > kEngineMaxSize) {  // indexes may pass the Redis offset limit (bloom_wide_op)
        const bool existed = c->ks.find(name) != nullptr;
        RBX_TRY(bitmap_for(c, name, kEngineMaxSize, is_add, c->stream, &bm));
        const int rc = bloom_wide_op(c, keys, size_bits(size), k, bm.get(), out_flags, out_count, is_add);
        if (bm && !existed) {  // only valid SETBITs create the key: a batch of error replies leaves none
            int r2;
            const uint64_t len = read_dev_u64(c, bm->d_len, &r2);
            if (r2 == RBX_OK && len == 0) c->ks.erase(name);
        }
        return rc;
    }
    RBX_TRY(bitmap_for(c, name, size_bits(size), is_add, c->stream, &bm));
    if (!bm) {  // GETBIT on a missing key: every bit is 0
        if (out_flags) memset(out_flags, 0, keys->n);
        if (out_count) *out_count = 0;
        return RBX_OK;
    }
    FilterDesc f = desc_of(*bm, size_bits(size), k, 0);
    if (bloom_tiny_fits(c, keys)) return bloom_host_tiny(c, f, k, keys, out_flags, out_count, is_add);
    if (bloom_small_fits(c, keys)) return bloom_host_small(c, f, k, keys, out_flags, out_count, is_add);
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d_count = c->dev->shared.counters.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, c->stream));
    uint8_t *d_out;
    RBX_TRY(out_flags_dev(c, out_flags, keys->n, &d_out));
    HIP_TRY(hipStreamSynchronize(c->stream));  // slots may still be read by an earlier call's stream
    RBX_TRY(pipelined_host_batches(c, keys, c->stream, [&](const KeysDev &dk, uint64_t i0) -> int {
        uint8_t *o = d_out ? d_out + i0 : nullptr;
        if (is_add) return run_add(c, dk, nullptr, nullptr, 0, f, k, o, d_count, nullptr, c->stream);
        return run_contains(c, dk, f, o, d_count, c->stream);
    }));
    if (out_flags) HIP_TRY(hipMemcpyAsync(out_flags, d_out, keys->n, hipMemcpyDeviceToHost, c->stream));
    int rc;
    uint64_t cnt = read_dev_u64(c, d_count, &rc);
    RBX_TRY(rc);
    if (out_count) *out_count = reply_count(is_add, cnt);
    return RBX_OK;
}

int bitcount_locked(rbx_ctx *c, const std::string &name, uint64_t *out) {
    Entry *e = c->ks.find(name);
    if (!e) {
        *out = 0;
        return RBX_OK;
    }
    if (e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    int rc;
    uint64_t len = read_dev_u64(c, e->bm->d_len, &rc);
    RBX_TRY(rc);
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 1;
    HIP_TRY(hipMemsetAsync(d, 0, 8, c->stream));
    if (len) launch_bitcount((const uint8_t *)e->bm->d_words, len, d, c->stream);
    HIP_TRY(hipGetLastError());
    *out = read_dev_u64(c, d, &rc);
    return rc;
}

// count() :215-227 (the size is the config's Java long, negative sizes included)
static int bloom_count(rbx_ctx *c, const std::string &name, int64_t *out) {
    RBX_ENTER(c, c->stream);
    BloomConfig cfg;
    RBX_TRY(ks_get_config(c->ks, name, &cfg));
    uint64_t bits;
    RBX_TRY(bitcount_locked(c, name, &bits));
    const double v = (double)(int64_t)(0 - (uint64_t)cfg.size) / ((double)cfg.k) *
                     std::log(1 - (double)bits / ((double)cfg.size));
    *out = java_math_round(v);
    return RBX_OK;
}

// ---- Bloom: handles / device path ---------------------------------------------------------
static int bloom_open(rbx_ctx *c, const std::string &name, rbx_bloom **out) {
    RBX_ENTER(c, c->stream);
    BloomConfig cfg;
    RBX_TRY(ks_get_config(c->ks, name, &cfg));
    RBX_TRY(check_offsets(cfg.size));
    // Opening a handle is RedissonBloomFilter's constructor + readConfig: it creates no bitmap
    // key (the first SETBIT does), so EXISTS / DEL / sizeInMemory see what the reference sees.
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitmap_for(c, name, size_bits(cfg.size), false, c->stream, &bm));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // gen 0 (never current: generations start at 1) makes the first call bind a missing bitmap
    *out = new rbx_bloom{c, name, cfg.size, cfg.k, bm, bm ? c->ks.generation : 0, g_handle_serial++};
    c->refs.fetch_add(1);
    return RBX_OK;
}

KeysDev keys_dev(const rbx_keys *k) { return KeysDev{k->bytes, k->offsets, k->stride, k->n}; }

// Re-resolves a Bloom handle's keys if the keyspace changed since its last call: the config
// must still hold the handle's (size, k) (addConfigCheck, M/RedissonBloomFilter.java:207-213) and
// the handle follows whatever bitmap the name holds now; *absent: no bitmap (GETBIT reads 0s).
// A bitmap created here is zero-filled on `st`.
int bloom_bind(rbx_ctx *c, rbx_bloom *b, bool create, hipStream_t st, bool *absent) {
    c->ks.sweep();
    *absent = false;
    if (b->ctx != c) return fail(RBX_E_ILLEGAL_ARGUMENT, "the handle belongs to another context");
    if (b->gen == c->ks.generation) return RBX_OK;
    RBX_TRY(ks_config_check(c->ks, b->name, b->size, b->k));
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitmap_for(c, b->name, size_bits(b->size), create, st, &bm));
    if (!bm) {
        *absent = true;
        b->bm.reset();  // a deleted bitmap's memory is not held by the handle
        return RBX_OK;  // (gen stays stale: the next call binds again)
    }
    b->bm = bm;
    b->gen = c->ks.generation;
    return RBX_OK;
}

}  // namespace rbx

using namespace rbx;

extern "C" {

int rbx_bloom_add(rbx_ctx *c, const char *name, uint64_t size, uint32_t k, const rbx_keys *keys,
                  uint8_t *out_new, uint64_t *out_count) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return bloom_host_op(c, name, (int64_t)size, k, keys, out_new, out_count, true);
}

int rbx_bloom_contains(rbx_ctx *c, const char *name, uint64_t size, uint32_t k, const rbx_keys *keys,
                       uint8_t *out_present, uint64_t *out_count) {
    if (!c || !name) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return bloom_host_op(c, name, (int64_t)size, k, keys, out_present, out_count, false);
}

int rbx_bloom_add_n(rbx_ctx *c, rbx_name name, uint64_t size, uint32_t k, const rbx_keys *keys, uint8_t *out_new,
                    uint64_t *out_count) {
    if (!c || (!name.bytes && name.len)) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return bloom_host_op(c, name_of(name), (int64_t)size, k, keys, out_new, out_count, true);
}

int rbx_bloom_contains_n(rbx_ctx *c, rbx_name name, uint64_t size, uint32_t k, const rbx_keys *keys,
                         uint8_t *out_present, uint64_t *out_count) {
    if (!c || (!name.bytes && name.len)) return fail(RBX_E_ILLEGAL_ARGUMENT, "ctx/name is NULL");
    return bloom_host_op(c, name_of(name), (int64_t)size, k, keys, out_present, out_count, false);
}

int rbx_bloom_bitcount(rbx_ctx *c, const char *name, uint64_t *out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    return bitcount_locked(c, name, out);
}

int rbx_bloom_count(rbx_ctx *c, const char *name, int64_t *out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bloom_count(c, name, out);
}

int rbx_bloom_count_n(rbx_ctx *c, rbx_name name, int64_t *out) {
    if (!c || (!name.bytes && name.len) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bloom_count(c, name_of(name), out);
}

int rbx_bloom_open(rbx_ctx *c, const char *name, rbx_bloom **out) {
    if (!c || !name || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bloom_open(c, name, out);
}

int rbx_bloom_open_n(rbx_ctx *c, rbx_name name, rbx_bloom **out) {
    if (!c || (!name.bytes && name.len) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bloom_open(c, name_of(name), out);
}

int rbx_bloom_close(rbx_bloom *b) {
    if (!b) return RBX_OK;
    rbx_ctx *c = b->ctx;
    {
        std::lock_guard<std::recursive_mutex> g(c->ks.mu);
        delete b;
    }
    ctx_release(c);
    return RBX_OK;
}

int rbx_bloom_handle_config(const rbx_bloom *b, uint64_t *size, uint32_t *k) {
    if (!b) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL handle");
    if (size) *size = (uint64_t)b->size;
    if (k) *k = b->k;
    return RBX_OK;
}

int rbx_bloom_contains_dev(rbx_ctx *c, rbx_bloom *b, const rbx_keys *d_keys, uint8_t *d_out,
                           unsigned long long *d_count, void *stream) {
    if (!c || !b) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(validate_keys(d_keys));
    if (d_keys->n == 0) return fail(RBX_E_ARITHMETIC, "/ by zero");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    bool absent;
    RBX_TRY(bloom_bind(c, b, false, st, &absent));
    if (absent) {  // GETBIT on a missing key: every bit is 0 (the count is unchanged)
        if (d_out) HIP_TRY(hipMemsetAsync(d_out, 0, d_keys->n, st));
        return RBX_OK;
    }
    KeysDev k = keys_dev(d_keys);
    FilterDesc f = desc_of(*b->bm, size_bits(b->size), b->k, 0);
    return run_contains(c, k, f, d_out, d_count, st);
}

int rbx_bloom_add_dev(rbx_ctx *c, rbx_bloom *b, const rbx_keys *d_keys, uint8_t *d_out_new,
                      unsigned long long *d_count, void *stream) {
    if (!c || !b) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(validate_keys(d_keys));
    if (d_keys->n == 0) return fail(RBX_E_ARITHMETIC, "/ by zero");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    bool absent;
    RBX_TRY(bloom_bind(c, b, true, st, &absent));
    KeysDev k = keys_dev(d_keys);
    FilterDesc f = desc_of(*b->bm, size_bits(b->size), b->k, 0);
    return run_add(c, k, nullptr, nullptr, 0, f, b->k, d_out_new, d_count, nullptr, st);
}

}  // extern "C"
