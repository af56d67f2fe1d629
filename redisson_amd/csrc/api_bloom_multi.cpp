// api_bloom_multi.cpp -- Bloom over many filters in one call: the multi-tenant contains / add (device
// and host arenas) and the ordered mixed stream.
#include <cstring>
#include <unordered_map>

#include "api_staging.h"
#include "tunables.h"

namespace rbx {

// Multi-tenant contains takes the per-lane slot kernel (one gather per key per round trip) when
// the distinct bitmaps of a call exceed this many bytes (past the caches, the request count
// binds); below it the staged kernel (fewer instructions per key) is faster.  rbx_tune
// "contains_multi_slots": 0 never, 1 always, 2 by this threshold (default).
constexpr uint64_t kSlotsMinBytes = 64ULL << 20;

// The tables derived from the descriptors `v` just uploaded: a ProbeDesc per segment, the bitmap words per
// table id (the stream's table walk finds a bit's bitmap by its fid), and the view's extent.
static int upload_derived(FilterTable &ft, const std::vector<FilterDesc> &v, hipStream_t st) {
    std::vector<ProbeDesc> pd(v.size());
    for (size_t s = 0; s < v.size(); ++s) pd[s] = ProbeDesc{v[s].bm, mod_compact(v[s].mp), v[s].k, v[s].fid};
    RBX_TRY(ft.probes.reserve(pd.size() * sizeof(ProbeDesc)));
    // pageable source: the runtime has staged it when the call returns
    HIP_TRY(hipMemcpyAsync(ft.probes.p, pd.data(), pd.size() * sizeof(ProbeDesc), hipMemcpyHostToDevice, st));
    uint32_t nf = 0;
    uint64_t maxbits = 1;
    for (size_t s = 0; s < v.size(); ++s) {
        nf = std::max(nf, v[s].fid + 1);
        maxbits = std::max<uint64_t>(maxbits, v[s].mp.size);
    }
    std::vector<uint32_t *> fb(std::max<uint32_t>(nf, 1), nullptr);
    for (size_t s = 0; s < v.size(); ++s) fb[v[s].fid] = v[s].bm;
    RBX_TRY(ft.fids.reserve(fb.size() * sizeof(uint32_t *)));
    HIP_TRY(hipMemcpyAsync(ft.fids.p, fb.data(), fb.size() * sizeof(uint32_t *), hipMemcpyHostToDevice, st));
    ft.view.probes = ft.probes.as<ProbeDesc>();
    ft.view.fid_bm = ft.fids.as<uint32_t *>();
    ft.view.nfids = nf;
    ft.view.maxbits = maxbits;
    return RBX_OK;
}

// Uploads the per-segment descriptor tables (cached by content + bitmap generation); *out: their view.
// create: a missing bitmap is created (add, stream); otherwise (contains) it reads as all zero
// through zero_bm and stays missing.  writes (nullable, with create): per filter, whether the call can set a
// bit in it -- the host stream knows; a filter it only reads stays missing like a contains'.
// kcap: the largest k the caller runs (the stream's 32), checked per handle before it is bound.
static int upload_filters(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, hipStream_t st, bool create,
                          FilterView *out, const uint8_t *writes = nullptr, uint32_t kcap = ~0u) {
    c->ks.sweep();
    FilterTable &ft = c->dev->filt;
    // same handles as the previous call and no keyspace change since: the tables are current
    // (100k tenants: ~5 ms of host work per call otherwise, more than the kernel takes)
    if (ft.key_generation == c->ks.generation && ft.keys.size() == nseg && ft.create == create &&
        !(create && ft.had_absent)) {
        bool same = true;
        for (uint32_t s = 0; s < nseg && same; ++s)
            same = filters[s] && ft.keys[s].first == filters[s] && ft.keys[s].second == filters[s]->serial;
        if (same) {
            *out = ft.view;
            return RBX_OK;
        }
    }
    ft.key_generation = ~0ULL;  // until the tables below are complete
    std::vector<FilterDesc> v(nseg);
    std::unordered_map<const Bitmap *, uint32_t> fid;
    uint32_t km = 1;
    uint64_t bytes = 0;
    std::vector<uint32_t> absent_segs;
    uint64_t zero_bytes = 0;
    // A call that fails at a later handle must leave no key behind: the strings this loop creates for the
    // handles before it are still empty (no kernel has run), so they go again with the error.
    std::vector<rbx_bloom *> created;
    auto undo = [&](int rc) {
        for (rbx_bloom *b : created) {
            Entry *e = c->ks.find(b->name);
            if (e && e->type == KType::Bitmap && e->bm == b->bm) c->ks.erase(b->name);
            b->bm.reset();
            b->gen = 0;
        }
        return rc;
    };
    for (uint32_t s = 0; s < nseg; ++s) {
        rbx_bloom *b = filters[s];
        if (!b) return undo(fail(RBX_E_ILLEGAL_ARGUMENT, "NULL filter handle"));
        if (b->k > kcap) return undo(fail(RBX_E_ILLEGAL_ARGUMENT, "stream batches support k <= 32"));
        if (b->gen != c->ks.generation) {
            const bool mk = create && (!writes || writes[s]);
            const bool had = !mk || c->ks.find(b->name) != nullptr;
            bool absent;
            const int rc = bloom_bind(c, b, mk, st, &absent);
            if (rc != RBX_OK) return undo(rc);
            if (!had && b->bm) created.push_back(b);
        }
        {
            const int rc = check_offsets(b->size);
            if (rc != RBX_OK) return undo(rc);
        }
        km = std::max(km, b->k);
        if (!b->bm) {  // contains on a missing key: every GETBIT reads 0
            absent_segs.push_back(s);
            zero_bytes = std::max<uint64_t>(zero_bytes, (size_bits(b->size) + 7) / 8);
            continue;
        }
        auto it = fid.find(b->bm.get());
        uint32_t id = it == fid.end() ? (uint32_t)fid.size() : it->second;
        if (it == fid.end()) {
            fid[b->bm.get()] = id;
            bytes += (size_bits(b->size) + 7) / 8;
        }
        if (id >= (1u << 24)) return undo(fail(RBX_E_ILLEGAL_ARGUMENT, "more than 2^24 distinct filters in one call"));
        v[s] = desc_of(*b->bm, size_bits(b->size), b->k, id);
    }
    if (!absent_segs.empty()) {
        // zero words for the largest missing bitmap + a zero Redis-length word (never written)
        const uint64_t need = ((zero_bytes + 255) & ~255ULL) + 256;
        RBX_TRY(ft.zero_bm.reserve_filled(need, 0, st));
        const uint32_t zid = (uint32_t)fid.size();
        for (uint32_t s : absent_segs) {
            rbx_bloom *b = filters[s];
            FilterDesc f{};
            f.bm = ft.zero_bm.as<uint32_t>();
            f.redis_len = (unsigned long long *)((uint8_t *)ft.zero_bm.p + need - 256);
            f.mp = make_mod_params(size_bits(b->size));
            f.k = b->k;
            f.fid = zid;
            v[s] = f;
        }
    }
    if (ft.generation != c->ks.generation) ft.table.invalidate();
    ft.view.filt = ft.table.sync(v, st);
    if (!ft.view.filt) return ft.table.err;
    if (ft.table.uploaded) {
        const int rc = upload_derived(ft, v, st);
        if (rc != RBX_OK) ft.table.invalidate();  // the next call uploads all three again
        RBX_TRY(rc);
        ft.generation = c->ks.generation;
    }
    ft.keys.resize(nseg);
    for (uint32_t s = 0; s < nseg; ++s) ft.keys[s] = {filters[s], filters[s]->serial};
    ft.key_generation = c->ks.generation;
    ft.create = create;
    ft.had_absent = !absent_segs.empty();
    ft.view.kmax = km;
    ft.view.bytes = bytes;
    *out = ft.view;
    return RBX_OK;
}

// bits of a bit index (bb) and of a table id (fbits) of the view's filters: the 8-byte first-setter entries
// hold both next to a chunk position
static void id_bits(const FilterView &v, uint32_t *bb, uint32_t *fbits) {
    *bb = 1, *fbits = 0;
    while ((1ULL << *bb) < v.maxbits) ++*bb;
    while ((1ULL << *fbits) < v.nfids) ++*fbits;
}

// d_tile_seg0 (nullable): each 256-key tile's first segment, already in device-visible memory (the tiny host
// path computes it on the host); else k_tile_seg0 finds it
static int contains_multi_run(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, const uint64_t *d_seg_offsets,
                              const rbx_keys *d_keys, uint8_t *d_out, unsigned long long *d_counts, hipStream_t st,
                              const uint32_t *d_tile_seg0) {
    FilterView fv;
    RBX_TRY(upload_filters(c, filters, nseg, st, false, &fv));
    if (d_keys->n == 0) return RBX_OK;
    KeysDev k = keys_dev(d_keys);
    if (!d_tile_seg0) {
        DevBuf &tile_segs = c->dev->shared.tile_segs;
        RBX_TRY(tile_segs.reserve(((d_keys->n + 255) / 256) * 4));
        launch_tile_seg0(d_seg_offsets, nseg, d_keys->n, tile_segs.as<uint32_t>(), st);
        d_tile_seg0 = tile_segs.as<uint32_t>();
    }
    const bool slots = g_tune.multi_slots == 1 || (g_tune.multi_slots == 2 && fv.bytes >= kSlotsMinBytes);
    launch_bloom_contains_multi(k, fast_len(k), fv.filt, d_seg_offsets, nseg, d_tile_seg0, fv.kmax, d_out, d_counts,
                                st, slots);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

// The 8-byte table (T8Table) is cleared only when it grows: every chunk's walk restores EMPTY.  A launch
// failing inside a chunk loop breaks that, so the guard then marks it as not filled and the next
// call clears it again.
struct ResetOnError {
    DevBuf &t8;
    bool ok = false;
    ~ResetOnError() {
        if (!ok) t8.invalidate();
    }
};

// Multi-tenant add by optimistic SETBITs with conflict repair (k_maddx_*): chunks of <= min(2^pb - 1,
// 2^27 / k) keys in key order (a chunk's bits are set before the next gathers).  The 8-byte table (an
// overflowed chunk's first setters) and its EMPTY state are shared with the ordered stream (T8Table).
static int run_add_multi8(rbx_ctx *c, const KeysDev &keys, const uint64_t *d_seg_off, uint32_t nseg,
                          const FilterView &fv, uint32_t bb, uint32_t pb, uint8_t *d_out_new,
                          unsigned long long *d_seg_counts, hipStream_t st, uint64_t lgc,
                          const uint32_t *big = nullptr, uint64_t segmax = 0) {
    const uint32_t kmax = fv.kmax;
    const uint64_t k = std::max<uint32_t>(kmax, 1);
    const uint64_t cap = std::min<uint64_t>((1ULL << std::min<uint32_t>(pb, 40)) - 1, (1ULL << 27) / k);
    uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(keys.n, cap));
    const uint64_t chunk_cap = g_tune.stream_chunk;  // the knob, once per call
    if (chunk_cap) chunk = std::min<uint64_t>(chunk, chunk_cap);
    const uint32_t lgmax = t8_log2((uint32_t)chunk, (uint32_t)k);
    const uint64_t entries = 1ULL << lgmax;
    DeviceState &dv = *c->dev;
    RBX_TRY(dv.t8.ensure(entries, st));
    RBX_TRY(dv.shared.zmask.reserve(chunk * 4));
    RBX_TRY(dv.strm.madd_c.reserve((8ULL << lgc) + 64));
    ResetOnError guard{dv.t8.buf};
    const int fl = fast_len(keys);
    for (uint64_t base = 0; base < keys.n; base += chunk) {
        MaddChunkArgs a{};
        a.keys = keys;
        a.base = base;
        a.nchunk = std::min<uint64_t>(chunk, keys.n - base);
        a.filt = fv.filt;
        a.seg_off = d_seg_off;
        a.nseg = nseg;
        a.tile_seg0 = dv.shared.tile_segs.as<uint32_t>();
        a.kmax = kmax;
        a.t8 = dv.t8.buf.as<unsigned long long>();
        a.lg = t8_log2((uint32_t)a.nchunk, (uint32_t)k);
        a.bb = bb;
        a.pb = pb;
        a.fid_bm = fv.fid_bm;
        a.zmask = dv.shared.zmask.as<uint32_t>();
        a.out_new = d_out_new;
        a.seg_counts = d_seg_counts;
        a.c8 = dv.strm.madd_c.as<unsigned long long>();
        a.lgC = (uint32_t)lgc;
        a.cst = (MaddxState *)(a.c8 + (1ULL << lgc));
        a.big = big;
        a.segmax = segmax;
        launch_madd8_chunk(a, fl, st);
        HIP_TRY(hipGetLastError());
    }
    guard.ok = true;
    return RBX_OK;
}

// Multi-tenant add over device keys, inside the caller's scope.  maxseg_hint: the largest segment in keys when
// the caller knows it from the host (multi_host), else ~0.
static int add_multi_run(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, const uint64_t *d_seg_offsets,
                         const rbx_keys *d_keys, uint8_t *d_out_new, unsigned long long *d_counts, hipStream_t st,
                         uint64_t maxseg_hint) {
    FilterView fv;
    RBX_TRY(upload_filters(c, filters, nseg, st, true, &fv));
    if (d_keys->n == 0) return RBX_OK;
    const uint32_t kmax = fv.kmax;
    KeysDev k = keys_dev(d_keys);
    // the chunked and table paths find each tile's first segment in tile_seg0 (the per-segment kernel does not)
    auto tiles = [&]() -> int {
        DevBuf &tile_segs = c->dev->shared.tile_segs;
        RBX_TRY(tile_segs.reserve(((d_keys->n + 255) / 256) * 4));
        launch_tile_seg0(d_seg_offsets, nseg, d_keys->n, tile_segs.as<uint32_t>(), st);
        return RBX_OK;
    };
    uint32_t bb, fbits;
    id_bits(fv, &bb, &fbits);
    // the knobs, once per call (rbx_tune may run on another thread)
    const int mode = g_tune.add_multi_t8;
    const uint64_t lgc = g_tune.maddx_lgc, segmax = g_tune.madd_segmax;
    if (mode == 2 && g_tune.madd_seg && kmax <= 16 && fv.nfids == nseg && bb + fbits <= 41) {
        // every filter in one segment only: k_madd_seg, one workgroup per segment; the chunked path
        // then handles only segments past segmax
        DevBuf &madd_c = c->dev->strm.madd_c;
        RBX_TRY(madd_c.reserve((8ULL << lgc) + 64));
        uint32_t *big = (uint32_t *)(madd_c.as<unsigned long long>() + (1ULL << lgc)) + 4;
        // no segment past segmax (known from the host, or the batch is that short): the flag is never
        // raised nor read, so it needs no zeroing launch
        const bool may_big = !(maxseg_hint <= segmax || d_keys->n <= segmax);
        if (may_big) HIP_TRY(hipMemsetAsync(big, 0, 4, st));
        MaddSegArgs a{};
        a.keys = k;
        a.filt = fv.filt;
        a.seg_off = d_seg_offsets;
        a.nseg = nseg;
        a.kmax = kmax;
        a.grid = g_tune.madd_seg_grid;
        a.segmax = segmax;
        a.out_new = d_out_new;
        a.seg_counts = d_counts;
        a.big = big;
        launch_madd_seg(a, fast_len(k), st);
        HIP_TRY(hipGetLastError());
        if (!may_big) return RBX_OK;  // no long segment
        // device offsets: read the flag (one sync) rather than launch the chunked path's kernels for
        // nothing -- 60 empty launches per C3 call in r05
        unsigned long long *w = c->dev->stage.words();  // pinned: no staging copy
        HIP_TRY(hipMemcpyAsync(w, big, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t has_big;
        memcpy(&has_big, w, 4);
        if (!has_big) return RBX_OK;
        RBX_TRY(tiles());
        return run_add_multi8(c, k, d_seg_offsets, nseg, fv, bb, 64 - bb - fbits, d_out_new, d_counts, st, lgc, big,
                              segmax);
    }
    RBX_TRY(tiles());
    if (mode && kmax <= 32 && bb + fbits <= 41)
        return run_add_multi8(c, k, d_seg_offsets, nseg, fv, bb, 64 - bb - fbits, d_out_new, d_counts, st, lgc);
    FilterDesc dummy{};
    return run_add(c, k, fv.filt, d_seg_offsets, nseg, dummy, kmax, d_out_new, nullptr, d_counts, st);
}

static int multi_host(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, const uint64_t *seg_offsets,
                      const rbx_keys *keys, uint8_t *out_flags, uint64_t *out_counts, bool is_add) {
    if (!c || !filters || !seg_offsets || nseg == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    RBX_TRY(validate_keys(keys));
    if (seg_offsets[0] != 0 || seg_offsets[nseg] != keys->n)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "segment offsets must span [0, n]");
    for (uint32_t s = 0; s < nseg; ++s) {
        if (seg_offsets[s + 1] < seg_offsets[s]) return fail(RBX_E_ILLEGAL_ARGUMENT, "segment offsets must be ascending");
        if (seg_offsets[s + 1] == seg_offsets[s]) return fail(RBX_E_ARITHMETIC, "/ by zero");
    }
    RBX_ENTER(c, c->stream);
    Staging &sg = c->dev->stage;
    uint64_t mx = 0;  // the largest segment: the per-segment add then skips the chunked path's launches
    for (uint32_t q = 0; q < nseg; ++q) mx = std::max<uint64_t>(mx, seg_offsets[q + 1] - seg_offsets[q]);
    // every tier's launches, over its staged keys, under this call's scope (the tiny contains brings each
    // tile's first segment)
    auto run = [&](const KeysDev &dk, const uint64_t *d_seg, uint8_t *d_out, unsigned long long *d_counts,
                   const uint32_t *d_tile_seg0 = nullptr) -> int {
        // rbx_keys has no off_base: shift the base so that bytes + offsets[i] is key i (never read below)
        rbx_keys kd{dk.bytes - dk.off_base, dk.offsets, dk.stride, dk.n};
        if (is_add) return add_multi_run(c, filters, nseg, d_seg, &kd, d_out, d_counts, c->stream, mx);
        return contains_multi_run(c, filters, nseg, d_seg, &kd, d_out, d_counts, c->stream, d_tile_seg0);
    };
    if (bloom_tiny_fits(c, keys)) {
        // keys, segment offsets and flags in coherent pinned memory (bloom_host_tiny); the per-segment counts
        // are the flags' sums (every segment holds a key, so nseg <= n fits the block)
        const KeysDev dk = tiny_stage(c, keys);
        memcpy(sg.tiny() + kTinySegAt, seg_offsets, (uint64_t)(nseg + 1) * 8);
        const auto *d_seg = (const uint64_t *)(sg.pin_tiny_dev + kTinySegAt);
        const uint32_t *d_tile_seg0 = nullptr;
        if (!is_add) {
            // each 256-key tile's first segment from the host (no k_tile_seg0 launch)
            std::vector<uint32_t> ts((keys->n + 255) / 256);
            for (uint32_t q = 0, t = 0; t < ts.size(); ++t) {
                while (seg_offsets[q + 1] <= (uint64_t)t * 256) ++q;
                ts[t] = q;
            }
            TinyArena ta{sg.tiny() + kTinyArenaAt, sg.pin_tiny_dev + kTinyArenaAt, kTinyArenaBytes, 0};
            d_tile_seg0 = (const uint32_t *)ta.put(ts.data(), ts.size() * 4);  // <= 64 entries: it fits
        }
        RBX_TRY(tiny_done(c, run(dk, d_seg, sg.pin_tiny_dev, nullptr, d_tile_seg0), g_tune.tiny_spin));
        const uint8_t *fl = sg.tiny();
        if (out_counts)
            for (uint32_t q = 0; q < nseg; ++q) {
                uint64_t t = 0;
                for (uint64_t i = seg_offsets[q]; i < seg_offsets[q + 1]; ++i) t += fl[i];
                out_counts[q] = t;
            }
        if (out_flags) memcpy(out_flags, fl, keys->n);
        return RBX_OK;
    }
    if ((uint64_t)nseg * 16 + 8 <= kSmallHead && bloom_small_fits(c, keys)) {
        // one transfer: the zeroed per-segment counts, the segment offsets, the keys (bloom_host_small)
        SmallStage sm;
        const uint64_t so_at = (uint64_t)nseg * 8;
        RBX_TRY(small_stage(c, keys, so_at + (uint64_t)(nseg + 1) * 8, &sm, seg_offsets, so_at, (uint64_t)(nseg + 1) * 8));
        auto *d_counts = (unsigned long long *)sm.dp;
        const auto *d_seg = (const uint64_t *)(sm.dp + so_at);
        uint8_t *d_out;
        RBX_TRY(out_flags_dev(c, out_flags, keys->n, &d_out));
        const int rc = run(sm.dk, d_seg, d_out, d_counts);
        (void)hipEventRecord(sg.ev_done[0], c->stream);
        if (rc != RBX_OK) return small_fail(c, rc);
        HIP_TRY(hipMemcpyAsync(sm.hp, sm.dp, (size_t)nseg * 8, hipMemcpyDeviceToHost, c->stream));
        if (out_flags) HIP_TRY(hipMemcpyAsync(sm.tail_h, d_out, keys->n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (out_flags) memcpy(out_flags, sm.tail_h, keys->n);
        if (out_counts) memcpy(out_counts, sm.hp, (size_t)nseg * 8);
        return RBX_OK;
    }
    KeysDev dk;
    RBX_TRY(upload_keys(c, keys, 0, keys->n, &dk));
    RBX_TRY(sg.seg_offs.reserve((nseg + 1) * 8));
    HIP_TRY(hipMemcpyAsync(sg.seg_offs.p, seg_offsets, (nseg + 1) * 8, hipMemcpyHostToDevice, c->stream));
    RBX_TRY(c->dev->shared.misc.reserve(nseg * 8));
    auto *d_counts = c->dev->shared.misc.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(d_counts, 0, nseg * 8, c->stream));
    uint8_t *d_out;
    RBX_TRY(out_flags_dev(c, out_flags, keys->n, &d_out));
    RBX_TRY(run(dk, sg.seg_offs.as<uint64_t>(), d_out, d_counts));
    if (out_flags) HIP_TRY(hipMemcpyAsync(out_flags, d_out, keys->n, hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned long long> cnt(nseg);
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_counts, nseg * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out_counts)
        for (uint32_t s = 0; s < nseg; ++s) out_counts[s] = cnt[s];
    return RBX_OK;
}

}  // namespace rbx

using namespace rbx;

extern "C" {

int rbx_bloom_contains_multi_dev(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg,
                                 const uint64_t *d_seg_offsets, const rbx_keys *d_keys, uint8_t *d_out,
                                 unsigned long long *d_counts, void *stream) {
    if (!c || !filters || !d_seg_offsets || nseg == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    RBX_TRY(validate_keys(d_keys));
    RBX_ENTER(c, pick_stream(c, stream));
    return contains_multi_run(c, filters, nseg, d_seg_offsets, d_keys, d_out, d_counts, pick_stream(c, stream), nullptr);
}

int rbx_bloom_add_multi_dev(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, const uint64_t *d_seg_offsets,
                            const rbx_keys *d_keys, uint8_t *d_out_new, unsigned long long *d_counts,
                            void *stream) {
    if (!c || !filters || !d_seg_offsets || nseg == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    RBX_TRY(validate_keys(d_keys));
    RBX_ENTER(c, pick_stream(c, stream));
    return add_multi_run(c, filters, nseg, d_seg_offsets, d_keys, d_out_new, d_counts, pick_stream(c, stream), ~0ULL);
}

// Ordered mixed stream (C5): see rbx.h.  Chunks of <= 2^26 pairs run probe -> contains -> commit
// (tunables.h: stream_table8, stream_chunk).
static int stream_run(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nfilters, const uint32_t *d_key_filter,
                      const uint8_t *d_key_op, const rbx_keys *d_keys, uint8_t *d_out, unsigned long long *d_counts,
                      void *stream, const uint8_t *writes) {
    if (!c || !filters || nfilters == 0 || !d_key_filter || !d_key_op)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL/empty argument");
    RBX_TRY(validate_keys(d_keys));
    RBX_ENTER(c, pick_stream(c, stream));
    hipStream_t st = pick_stream(c, stream);
    FilterView fv;
    RBX_TRY(upload_filters(c, filters, nfilters, st, true, &fv, writes, 32));
    const uint32_t kmax = fv.kmax;
    if (kmax > 32) return fail(RBX_E_ILLEGAL_ARGUMENT, "stream batches support k <= 32");  // a table add_multi built
    if (d_keys->n == 0) return RBX_OK;
    KeysDev keys = keys_dev(d_keys);
    const uint64_t k = std::max<uint32_t>(kmax, 1);
    // r04: 8-byte first-setter entries when (fid, bit) leaves >= 23 bits for a chunk position
    uint32_t bb, fbits;
    id_bits(fv, &bb, &fbits);
    const bool t8 = g_tune.stream_table8 && bb + fbits <= 41;
    const uint32_t pb = 64 - bb - fbits;
    // Chunks: <= 2^26 (add, bit) pairs for the 16-byte table; with 8-byte entries as many commands
    // as a position field holds, <= 2^27 pairs (a worst-case table of <= 1-2 GiB): C5 8.4M commands
    // per chunk instead of 6.7M.  What that bought (fresh C5, 16.2 vs 17.0 ms) is the table's load:
    // 838K adds size it at 2^24 entries (~27% used) where 671K gave 2^23 (~43%); 6.7M-command chunks
    // on a 2^24 table run as fast (16.34 / 16.41 vs 16.60 / 16.54 ms, r04l_c5_chunk_vs_table_load),
    // larger tables again slower (r04s_c5_table_scale).  Smaller chunks: 3.4M / 1.7M 18.5 / 20.3 ms.
    const uint64_t cap8 = std::min<uint64_t>((1ULL << std::min<uint32_t>(pb, 40)) - 1, (1ULL << 27) / k);
    uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(keys.n, t8 ? cap8 : (1ULL << 26) / k));
    // chunk bases on 128-command boundaries keep the replies' range images line-aligned
    if (chunk < keys.n && chunk > 128) chunk &= ~127ULL;
    if (g_tune.stream_chunk) chunk = std::min<uint64_t>(chunk, g_tune.stream_chunk);
    DeviceState &dv = *c->dev;
    StreamScratch &ss = dv.strm;
    ss.geom[0] = bb;
    ss.geom[1] = fbits;
    ss.geom[2] = t8 ? pb : 0;
    ss.geom[3] = chunk;
    RBX_TRY(dv.shared.zmask.reserve(chunk * 4));
    RBX_TRY(ss.adds.reserve(chunk * 4));
    if (t8) RBX_TRY(ss.fslot.reserve(chunk * 4));
    // one add counter per chunk (zeroed once per call: one fill, not one per chunk)
    const uint64_t nchunks = (keys.n + chunk - 1) / chunk;
    RBX_TRY(ss.nadds.reserve(nchunks * 4));
    HIP_TRY(hipMemsetAsync(ss.nadds.p, 0, nchunks * 4, st));
    const int fl = fast_len(keys);
    if (t8) RBX_TRY(dv.t8.ensure(1ULL << t8_log2((uint32_t)chunk, (uint32_t)k), st));
    ResetOnError guard{dv.t8.buf};
    for (uint64_t base = 0; base < keys.n; base += chunk) {
        const uint64_t nch = std::min<uint64_t>(chunk, keys.n - base);
        if (!t8) RBX_TRY(dv.fst.ensure(nch * k, st));
        StreamChunkArgs s{};
        if (t8) {
            s.t8 = dv.t8.buf.as<unsigned long long>();
            s.bb = bb;
            s.pb = pb;
            s.fid_bm = fv.fid_bm;
            s.tkmax = kmax;
            s.fslot = ss.fslot.as<uint32_t>();
        }
        s.adds = ss.adds.as<uint32_t>();
        s.nadds = ss.nadds.as<uint32_t>() + base / chunk;
        s.keys = keys;
        s.base = base;
        s.nchunk = nch;
        s.filt = fv.filt;
        s.pdesc = fv.probes;
        s.kf = d_key_filter;
        s.op = d_key_op;
        s.table = dv.fst.table.as<HTEntry>();
        s.log2cap = dv.fst.log2cap;
        s.epoch = dv.fst.epoch;
        s.zmask = dv.shared.zmask.as<uint32_t>();
        s.kmax = kmax;
        s.out = d_out;
        s.counts = d_counts;
        launch_stream_chunk(s, fl, st);
        HIP_TRY(hipGetLastError());
    }
    guard.ok = true;
    return RBX_OK;
}

// The device form cannot know which filters its commands write before it binds them: every filter without a
// string gets one (empty if no add reaches it).  The host form below reads the ops and binds for writing only
// the filters an add names.
int rbx_bloom_stream_dev(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nfilters, const uint32_t *d_key_filter,
                         const uint8_t *d_key_op, const rbx_keys *d_keys, uint8_t *d_out,
                         unsigned long long *d_counts, void *stream) {
    return stream_run(c, filters, nfilters, d_key_filter, d_key_op, d_keys, d_out, d_counts, stream, nullptr);
}

int rbx_bloom_stream(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nfilters, const uint32_t *key_filter,
                     const uint8_t *key_op, const rbx_keys *keys, uint8_t *out, uint64_t *counts) {
    if (!c || !filters || nfilters == 0 || !key_filter || !key_op) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(validate_keys(keys));
    std::vector<uint8_t> writes(nfilters, 0);
    for (uint64_t i = 0; i < keys->n; ++i) {
        if (key_filter[i] >= nfilters) return fail(RBX_E_ILLEGAL_ARGUMENT, "key_filter index out of range");
        if (key_op[i]) writes[key_filter[i]] = 1;
    }
    RBX_ENTER(c, c->stream);
    KeysDev dk;
    RBX_TRY(upload_keys(c, keys, 0, keys->n, &dk));
    const uint64_t n = keys->n;
    DevBuf &seg_offs = c->dev->stage.seg_offs;
    RBX_TRY(seg_offs.reserve(n * 4 + n + 64));
    auto *d_kf = seg_offs.as<uint32_t>();
    auto *d_op = (uint8_t *)(d_kf + n);
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_kf, key_filter, n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_op, key_op, n, hipMemcpyHostToDevice, c->stream));
    }
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d_cnt = c->dev->shared.counters.as<unsigned long long>() + 2;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 16, c->stream));
    uint8_t *d_out;
    RBX_TRY(out_flags_dev(c, out, n, &d_out));
    // the *_dev ABI has no off_base: shift the base so that bytes + offsets[i] is key i (never read below)
    rbx_keys kd{dk.bytes - dk.off_base, dk.offsets, dk.stride, dk.n};
    RBX_TRY(stream_run(c, filters, nfilters, d_kf, d_op, &kd, d_out, d_cnt, c->stream, writes.data()));
    if (out && n) HIP_TRY(hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, c->stream));
    unsigned long long cnt[2];
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (counts) {
        counts[0] = cnt[0];
        counts[1] = cnt[1];
    }
    return RBX_OK;
}

int rbx_bloom_contains_multi(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, const uint64_t *seg_offsets,
                             const rbx_keys *keys, uint8_t *out_present, uint64_t *out_counts) {
    return multi_host(c, filters, nseg, seg_offsets, keys, out_present, out_counts, false);
}

int rbx_bloom_add_multi(rbx_ctx *c, rbx_bloom *const *filters, uint32_t nseg, const uint64_t *seg_offsets,
                        const rbx_keys *keys, uint8_t *out_new, uint64_t *out_counts) {
    return multi_host(c, filters, nseg, seg_offsets, keys, out_new, out_counts, true);
}

}  // extern "C"
