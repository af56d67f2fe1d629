// api_bitset.cpp -- RBitSet over one bitmap key (M/RedissonBitSet.java): single and batched SETBIT /
// GETBIT, range fill, BITOP, cardinality / size / length, the typed fields of BITFIELD, the ranged
// BITCOUNT / BITPOS that Spring Data reaches the same strings with, set-bit enumeration and the BitSet
// exchange.  The calls over many keys: api_bitset_multi.cpp.
// S/ = redisson-spring-data/redisson-spring-data-31/src/main/java/org/redisson/spring/data/connection/
#include <cstring>

#include "rbx_ctx.h"
#include "tunables.h"

#include "field_rule.h"  // after rbx_device.h, whose RBX_HD it then uses
#include "members_rule.h"

namespace rbx {

static constexpr uint64_t kMaxBitOffset = kEngineMaxSize;  // offsets end at 2^32 - 1

// the bitmap under `name`; null for a missing key (the empty string)
int bitset_find(rbx_ctx *c, const std::string &name, std::shared_ptr<Bitmap> *out) {
    out->reset();
    Entry *e = c->ks.find(name);
    if (!e) return RBX_OK;
    if (e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    *out = e->bm;
    return RBX_OK;
}

// The bitmap a write reaching byte need_bytes - 1 goes to.  The key's own allocation when it
// suffices: the write is then in place and open rbx_bloom handles keep seeing the key.  Otherwise it
// grows geometrically (at most 2^32 bits, never below the |size| of an existing {name}:config),
// which rebinds the entry and bumps the keyspace generation (grow_bitmap); a missing key is created.
int bitset_for_write(rbx_ctx *c, const std::string &name, uint64_t need_bytes, hipStream_t st,
                     std::shared_ptr<Bitmap> *out) {
    Entry *e = c->ks.find(name);
    if (e && e->type != KType::Bitmap) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    if (e && e->bm->cap_bytes >= need_bytes) {
        *out = e->bm;
        return RBX_OK;
    }
    uint64_t bits = import_bits(c, name, need_bytes);
    if (e) {
        bits = std::min<uint64_t>(std::max<uint64_t>(bits, e->bm->cap_bytes * 16), kEngineMaxSize);
        RBX_TRY(grow_bitmap(c, *e->bm, bits, st));
        *out = e->bm;
        return RBX_OK;
    }
    RBX_TRY(new_bitmap(c, bits, st, out));
    c->ks.put(name, Entry{KType::Bitmap, nullptr, *out, nullptr});
    return RBX_OK;
}

// Redis lengths of bitmaps (null = missing key: 0), eight per trip through the pinned words
static int bitset_lens(rbx_ctx *c, const std::vector<Bitmap *> &bms, hipStream_t st, std::vector<uint64_t> *lens) {
    lens->assign(bms.size(), 0);
    for (size_t i0 = 0; i0 < bms.size(); i0 += 8) {
        const size_t m = std::min<size_t>(8, bms.size() - i0);
        for (size_t j = 0; j < m; ++j)
            if (bms[i0 + j]) HIP_TRY(hipMemcpyAsync(c->dev->stage.words() + j, bms[i0 + j]->d_len, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t j = 0; j < m; ++j)
            if (bms[i0 + j]) (*lens)[i0 + j] = c->dev->stage.words()[j];
    }
    return RBX_OK;
}

// the bitmap under `name` (null for a missing key) and its Redis length, inside the caller's scope
static int bitset_len(rbx_ctx *c, rbx_name name, std::shared_ptr<Bitmap> *bm, uint64_t *len) {
    RBX_TRY(bitset_find(c, name_of(name), bm));
    std::vector<uint64_t> lens;
    RBX_TRY(bitset_lens(c, {bm->get()}, c->stream, &lens));
    *len = lens[0];
    return RBX_OK;
}

static uint64_t max_index(const uint64_t *idx, uint64_t n) {
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; ++i) m = std::max(m, idx[i]);
    return m;
}

// the maximum of n device indexes (one wait on `st`), which must be a Redis bit offset
static int max_index_dev(rbx_ctx *c, const uint64_t *d_idx, uint64_t n, hipStream_t st, uint64_t *out) {
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 1;
    HIP_TRY(hipMemsetAsync(d, 0, 8, st));
    launch_bits_max(d_idx, n, d, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->dev->stage.words(), d, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = *c->dev->stage.words();
    return *out >= kMaxBitOffset ? fail(RBX_E_REDIS, kBitOffsetMsg) : RBX_OK;
}

// SETBIT of n device indexes whose maximum is mx
static int bitset_scatter(rbx_ctx *c, const std::string &name, const uint64_t *d_idx, uint64_t n, uint64_t mx, int value,
                          hipStream_t st) {
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_for_write(c, name, (mx >> 3) + 1, st, &bm));
    launch_bits_scatter(bm->d_words, bm->d_len, bm->cap_bytes * 8, d_idx, n, value != 0, (mx >> 3) + 1, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

// GETBIT of n device indexes into device bytes
static int bitset_gather(rbx_ctx *c, const std::string &name, const uint64_t *d_idx, uint64_t n, uint8_t *d_out,
                         hipStream_t st) {
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_find(c, name, &bm));
    if (!bm) {
        HIP_TRY(hipMemsetAsync(d_out, 0, n, st));
        return RBX_OK;
    }
    launch_bits_gather(bm->d_words, bm->cap_bytes * 8, d_idx, n, d_out, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

// ---- RBitSet's typed fields: BITFIELD GET / SET / INCRBY (M/RedissonBitSet.java:71-254) -------
// the type's checks: Redisson's own (:72-73, :99-100), then the one Redis makes
static int field_type_check(int op, int is_signed, int size) {
    if (op < RBX_FIELD_GET || op > RBX_FIELD_INCRBY) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown BITFIELD operation");
    if (is_signed && size > 64) return fail(RBX_E_ILLEGAL_ARGUMENT, "Size can't be greater than 64 bits");
    if (!is_signed && size > 63) return fail(RBX_E_ILLEGAL_ARGUMENT, "Size can't be greater than 63 bits");
    if (size < 1) return fail(RBX_E_REDIS, kFieldTypeMsg);
    return RBX_OK;
}

// the offset limit for fields of `size` bits whose largest offset is mx: the whole field lies below bit 2^32
static int field_range_check(uint64_t mx, int size) {
    if (mx >= kMaxBitOffset || mx + (uint64_t)size > kMaxBitOffset) return fail(RBX_E_REDIS, kBitOffsetMsg);
    return RBX_OK;
}

// GET on a host string: the field's bits from the bytes below len, zero past them
static int64_t field_of_bytes(const uint8_t *bytes, uint64_t len, int is_signed, int size, uint64_t offset) {
    uint64_t v = 0;
    for (int j = 0; j < size; ++j) {
        const uint64_t b = offset + (uint64_t)j;
        const uint64_t bit = (b >> 3) < len ? (bytes[b >> 3] >> (7 - (b & 7))) & 1 : 0;
        v = (v << 1) | bit;
    }
    if (is_signed && size < 64 && ((v >> (size - 1)) & 1)) v |= ~0ULL << size;
    return (int64_t)v;
}

static int overflow_check(int mode) {
    if (mode < RBX_OVERFLOW_WRAP || mode > RBX_OVERFLOW_FAIL)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown OVERFLOW mode");
    return RBX_OK;
}

// A checked batch over device arrays: mx = the largest offset, aligned = every offset is a multiple
// of size, one_sign = no two values of opposite signs (looked at for a SAT INCRBY without replies
// only).  GET gathers; an unaligned SET / INCRBY runs serially (partly overlapping fields make
// the order total); an aligned INCRBY without replies whose size divides 64 is one atomic loop per
// element under WRAP, and under SAT when the increments have one sign (saturating sums commute then
// and only then; FAIL never commutes); every other aligned batch is sorted by slot and walked run by
// run.  d_nil (nullable) is zeroed here and set by the FAIL kernels.
static int fields_run(rbx_ctx *c, const std::string &name, int op, int is_signed, int size, int mode,
                      const uint64_t *d_offs, const int64_t *d_values, uint64_t n, int64_t *d_replies, uint8_t *d_nil,
                      uint64_t mx, bool aligned, bool one_sign, hipStream_t st) {
    std::shared_ptr<Bitmap> bm;
    if (d_nil) HIP_TRY(hipMemsetAsync(d_nil, 0, n, st));
    if (op == RBX_FIELD_GET) {
        RBX_TRY(bitset_find(c, name, &bm));
        if (!bm) {
            HIP_TRY(hipMemsetAsync(d_replies, 0, n * 8, st));
            return RBX_OK;
        }
        launch_fields_get(bm->d_words, bm->cap_bytes, d_offs, n, size, is_signed, d_replies, st);
        HIP_TRY(hipGetLastError());
        return RBX_OK;
    }
    const uint64_t need = ((mx + size - 1) >> 3) + 1;
    RBX_TRY(bitset_for_write(c, name, need, st, &bm));
    const bool commutes = op == RBX_FIELD_INCRBY && !d_replies && 64 % size == 0;
    if (!aligned) {
        launch_fields_serial(bm->d_words, bm->d_len, bm->cap_bytes, op, is_signed, size, mode, d_offs, d_values, n,
                             d_replies, d_nil, need, st);
    } else if (commutes && mode == RBX_OVERFLOW_WRAP) {
        launch_fields_incr_atomic(bm->d_words, bm->d_len, bm->cap_bytes, d_offs, d_values, n, size, need, st);
    } else if (commutes && mode == RBX_OVERFLOW_SAT && one_sign && g_tune.bitfield_sat_atomic != 0) {
        launch_fields_incr_sat(bm->d_words, bm->d_len, bm->cap_bytes, d_offs, d_values, n, size, is_signed, need, st);
    } else {
        // consecutive chunks of at most 2^30 elements, in order (positions are 32-bit inside a chunk)
        const uint64_t kChunk = 1ULL << 30;
        const int slot_bits = std::min(32, std::max(1, significant_bits(mx / (uint64_t)size)));
        DevBuf &sort = c->dev->bits.fld_sort;
        RBX_TRY(cell_sort_reserve<uint32_t>(sort, (uint32_t)std::min(n, kChunk), 0, slot_bits));
        for (uint64_t i0 = 0; i0 < n; i0 += kChunk) {
            const uint32_t m = (uint32_t)std::min(kChunk, n - i0);
            RBX_TRY(sort_failed(launch_fields_grouped(bm->d_words, bm->d_len, bm->cap_bytes, op, is_signed, size, mode,
                                                      d_offs + i0, d_values + i0, m, d_replies ? d_replies + i0 : nullptr,
                                                      d_nil ? d_nil + i0 : nullptr, need, slot_bits, sort.p, sort.cap, st)));
        }
    }
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

static int fields_args_check(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, const void *offs,
                             const void *values, uint64_t n, const void *replies) {
    if (!c || bad_name(name)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(field_type_check(op, is_signed, size));
    if (n && (!offs || (op != RBX_FIELD_GET && !values) || (op == RBX_FIELD_GET && !replies)))
        return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return RBX_OK;
}

// nil's own rule: required under FAIL when replies are asked for (a nil reply has no other form)
static int nil_args_check(int op, int mode, uint64_t n, const void *replies, const void *nil) {
    RBX_TRY(overflow_check(mode));
    if (n && op != RBX_FIELD_GET && mode == RBX_OVERFLOW_FAIL && replies && !nil)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "OVERFLOW FAIL with replies needs nil");
    return RBX_OK;
}

// the host form of a batch whose arguments are checked: scan, upload, run, read back
static int fields_host(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, int mode, const uint64_t *offsets,
                       const int64_t *values, uint64_t n, int64_t *replies, uint8_t *nil) {
    if (n == 0) return RBX_OK;  // no command is sent
    uint64_t mx = 0;
    bool aligned = true;
    for (uint64_t i = 0; i < n; ++i) {
        mx = std::max(mx, offsets[i]);
        aligned &= offsets[i] % (uint64_t)size == 0;
    }
    RBX_TRY(field_range_check(mx, size));
    bool pos = false, neg = false;
    if (op == RBX_FIELD_INCRBY && mode == RBX_OVERFLOW_SAT && !replies)
        for (uint64_t i = 0; i < n; ++i) {
            pos |= values[i] > 0;
            neg |= values[i] < 0;
        }
    RBX_ENTER(c, c->stream);
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.idx.reserve(n * 8));
    HIP_TRY(hipMemcpyAsync(b.idx.p, offsets, n * 8, hipMemcpyHostToDevice, c->stream));
    if (op != RBX_FIELD_GET) {
        RBX_TRY(b.fld_vals.reserve(n * 8));
        HIP_TRY(hipMemcpyAsync(b.fld_vals.p, values, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (replies) RBX_TRY(b.fld_out.reserve(n * 8));
    if (nil) RBX_TRY(b.fld_nil.reserve(n));
    RBX_TRY(fields_run(c, name_of(name), op, is_signed, size, mode, b.idx.as<uint64_t>(), b.fld_vals.as<int64_t>(), n,
                       replies ? b.fld_out.as<int64_t>() : nullptr, nil ? b.fld_nil.as<uint8_t>() : nullptr, mx, aligned,
                       !(pos && neg), c->stream));
    if (replies) HIP_TRY(hipMemcpyAsync(replies, b.fld_out.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (nil) HIP_TRY(hipMemcpyAsync(nil, b.fld_nil.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

// the device form: one wait on the stream, for the batch's check result -- the largest offset, whether
// every offset is aligned and, for a SAT INCRBY without replies, whether increments of both signs occur
static int fields_dev(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, int mode, const uint64_t *d_offsets,
                      const int64_t *d_values, uint64_t n, int64_t *d_replies, uint8_t *d_nil, void *stream) {
    if (n == 0) return RBX_OK;
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 1;
    HIP_TRY(hipMemsetAsync(d, 0, 16, st));
    const bool signs = op == RBX_FIELD_INCRBY && mode == RBX_OVERFLOW_SAT && !d_replies;
    launch_fields_check(d_offsets, signs ? d_values : nullptr, n, size, d, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->dev->stage.words(), d, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t mx = c->dev->stage.words()[0], flags = c->dev->stage.words()[1];
    RBX_TRY(field_range_check(mx, size));
    return fields_run(c, name_of(name), op, is_signed, size, mode, d_offsets, d_values, n, d_replies, d_nil, mx,
                      (flags & 1) == 0, (flags & 6) != 6, st);
}

// ---- ranged BITCOUNT / BITPOS (S/RedissonConnection.java:638-646, :2337-2359; rules: rbx_kernels.h) ----
static int range_unit_check(int unit) {
    if (unit != RBX_RANGE_BYTE && unit != RBX_RANGE_BIT) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown range unit");
    return RBX_OK;
}

// BITPOS's own checks; nargs < 0 = a batch without ends ("bit start")
static int pos_args_check(int bit, int nargs, int unit) {
    if (nargs > 2) return fail(RBX_E_ILLEGAL_ARGUMENT, "nargs is 0, 1 or 2");
    RBX_TRY(range_unit_check(unit));
    if (bit != 0 && bit != 1) return fail(RBX_E_REDIS, "ERR The bit argument must be 1 or 0.");
    if (nargs < 2 && unit == RBX_RANGE_BIT) return fail(RBX_E_REDIS, "ERR syntax error");  // a unit needs an end
    return RBX_OK;
}

// A query over a string of len bytes: its interval, or false with the reply no kernel is needed for.
static bool range_interval(bool pos, int64_t start, int64_t end, bool end_given, int unit, uint64_t len, uint64_t *lo,
                           uint64_t *hi, int64_t *fixed) {
    *fixed = pos ? -1 : 0;  // the empty range
    if (!pos) return bits_count_interval(start, end, unit, len, lo, hi);
    return bits_normalise(start, end_given ? end : (int64_t)len - 1, unit, len, lo, hi);
}

// n replies that are all 0 or all -1: a missing key, an existing empty string
static int range_fill(void *out, uint64_t n, int64_t value, bool dev, hipStream_t st) {
    if (dev) HIP_TRY(hipMemsetAsync(out, value ? 0xFF : 0, n * 8, st));
    else memset(out, value ? 0xFF : 0, n * 8);
    return RBX_OK;
}
static int64_t missing_reply(bool pos, int bit) { return pos && bit ? -1 : 0; }

// one query over the normalised [lo, hi], its reply to the device word d_out: the grid-wide count, or the
// chunked search
static int range_one(rbx_ctx *c, const Bitmap &bm, bool pos, int bit, bool end_given, uint64_t lo, uint64_t hi,
                     void *d_out, hipStream_t st) {
    if (!pos) {
        HIP_TRY(hipMemsetAsync(d_out, 0, 8, st));
        launch_bits_count_range(bm.d_words, lo, hi, (unsigned long long *)d_out, st);
    } else {
        RBX_TRY(c->dev->bits.rng_pos.reserve(kBitsPosStateBytes));
        HIP_TRY(hipMemsetAsync(c->dev->bits.rng_pos.p, 0xFF, kBitsPosStateBytes, st));
        launch_bits_pos(bm.d_words, lo, hi, bit, g_tune.bitrange_pos_chunk, c->dev->bits.rng_pos.as<unsigned long long>(),
                        bits_pos_reply(kBitsNone, bit, end_given, hi), (int64_t *)d_out, st);
    }
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

// The batch path under the knobs as they stand: true = the block directory.  rbx_bench_bitrange_path shows it.
static bool ranges_take_directory(uint64_t len, uint64_t n, uint64_t total, uint64_t longest) {
    const int mode = g_tune.bitrange_dir;
    return mode == 1 || (mode == 2 && (total > len + n * 8192 || longest > g_tune.bitrange_chain_max));
}

// n >= 2 queries over a string of len > 0 bytes.  total / longest: the bytes the clamped intervals cover
// together, and the longest of them.  The walk reads `total` bytes, the directory path len to build the
// directory and then at most 8 KiB per query: it is taken when that is less, and when one wave would walk more
// than bitrange_chain_max bytes alone.  The directory lives for this call only: any write would invalidate it.
static int ranges_run(rbx_ctx *c, const Bitmap &bm, uint64_t len, bool pos, int bit, const int64_t *d_starts,
                      const int64_t *d_ends, uint64_t n, int unit, void *d_out, uint64_t total, uint64_t longest,
                      hipStream_t st) {
    const bool dir = ranges_take_directory(len, n, total, longest);
    unsigned long long *d_dir = nullptr;
    if (dir) {
        RBX_TRY(c->dev->bits.rng_dir.reserve((bits_dir_blocks(len) + 1) * 8));
        d_dir = c->dev->bits.rng_dir.as<unsigned long long>();
        launch_bits_directory(bm.d_words, len, d_dir, st);
    }
    if (pos) launch_bits_pos_ranges(bm.d_words, len, bit, d_starts, d_ends, n, unit, d_dir, (int64_t *)d_out, st);
    else launch_bits_count_ranges(bm.d_words, len, d_starts, d_ends, n, unit, d_dir, (uint64_t *)d_out, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

static int ranges_args_check(rbx_ctx *c, rbx_name name, bool pos, int bit, const void *starts, const void *ends,
                             uint64_t n, int unit, const void *out) {
    if (!c || bad_name(name) || (n && (!starts || !out || (!pos && !ends)))) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return pos ? pos_args_check(bit, ends ? 2 : -1, unit) : range_unit_check(unit);
}

// a batch over host arrays, n >= 2 (one query goes through the single entry points)
static int ranges_host(rbx_ctx *c, rbx_name name, bool pos, int bit, const int64_t *starts, const int64_t *ends,
                       uint64_t n, int unit, void *out) {
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    std::shared_ptr<Bitmap> bm;
    uint64_t len;
    RBX_TRY(bitset_len(c, name, &bm, &len));
    if (!bm) return range_fill(out, n, missing_reply(pos, bit), false, st);
    if (len == 0) return range_fill(out, n, pos ? -1 : 0, false, st);
    uint64_t total = 0, longest = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b = bits_interval_bytes(starts[i], ends ? ends[i] : (int64_t)len - 1, unit, len, pos);
        total += b;
        longest = std::max(longest, b);
    }
    BitsetScratch &bs = c->dev->bits;
    RBX_TRY(bs.rng_args.reserve(n * 16));
    RBX_TRY(bs.rng_out.reserve(n * 8));
    int64_t *d_starts = bs.rng_args.as<int64_t>(), *d_ends = ends ? d_starts + n : nullptr;
    HIP_TRY(hipMemcpyAsync(d_starts, starts, n * 8, hipMemcpyHostToDevice, st));
    if (ends) HIP_TRY(hipMemcpyAsync(d_ends, ends, n * 8, hipMemcpyHostToDevice, st));
    RBX_TRY(ranges_run(c, *bm, len, pos, bit, d_starts, d_ends, n, unit, bs.rng_out.p, total, longest, st));
    HIP_TRY(hipMemcpyAsync(out, bs.rng_out.p, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBX_OK;
}

// a batch over device arrays: one wait, for the length word, the work summary and -- n = 1 -- the query itself
static int ranges_dev(rbx_ctx *c, rbx_name name, bool pos, int bit, const int64_t *d_starts, const int64_t *d_ends,
                      uint64_t n, int unit, void *d_out, hipStream_t st) {
    RBX_ENTER(c, st);
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_find(c, name_of(name), &bm));
    if (!bm) return range_fill(d_out, n, missing_reply(pos, bit), true, st);
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 4;  // count words 4 .. 6
    unsigned long long *w = c->dev->stage.words();
    HIP_TRY(hipMemsetAsync(d, 0, 24, st));
    launch_bits_ranges_summary(d_starts, d_ends, n, unit, pos, bm->d_len, d, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w, d, 24, hipMemcpyDeviceToHost, st));
    if (n == 1) {
        HIP_TRY(hipMemcpyAsync(w + 3, d_starts, 8, hipMemcpyDeviceToHost, st));
        if (d_ends) HIP_TRY(hipMemcpyAsync(w + 4, d_ends, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t len = w[0], total = w[1], longest = w[2];
    if (len == 0) return range_fill(d_out, n, pos ? -1 : 0, true, st);
    if (n > 1) return ranges_run(c, *bm, len, pos, bit, d_starts, d_ends, n, unit, d_out, total, longest, st);
    uint64_t lo, hi;
    int64_t fixed;
    if (!range_interval(pos, (int64_t)w[3], (int64_t)w[4], d_ends != nullptr, unit, len, &lo, &hi, &fixed))
        return range_fill(d_out, 1, fixed, true, st);
    return range_one(c, *bm, pos, bit, d_ends != nullptr, lo, hi, d_out, st);
}

// one command on the context's stream: its reply in *out
static int range_single(rbx_ctx *c, rbx_name name, bool pos, int bit, int64_t start, int64_t end, bool end_given,
                        int unit, int64_t *out) {
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    uint64_t len, lo, hi;
    RBX_TRY(bitset_len(c, name, &bm, &len));
    *out = missing_reply(pos, bit);
    if (!bm) return RBX_OK;
    if (!range_interval(pos, start, end, end_given, unit, len, &lo, &hi, out)) return RBX_OK;
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 1;
    RBX_TRY(range_one(c, *bm, pos, bit, end_given, lo, hi, d, c->stream));
    int rc;
    *out = (int64_t)read_dev_u64(c, d, &rc);
    return rc;
}

// the two commands over a host string
static int range_of(const uint8_t *bytes, uint64_t len, int missing, bool pos, int bit, int64_t start, int64_t end,
                    bool end_given, int unit, int64_t *out) {
    if (missing) len = 0;
    uint64_t lo, hi;
    *out = missing_reply(pos, bit);
    if (missing || !range_interval(pos, start, end, end_given, unit, len, &lo, &hi, out)) return RBX_OK;
    uint64_t ones = 0, found = kBitsNone;
    for (uint64_t p = lo; p <= hi && found == kBitsNone; ++p) {
        const int b = (bytes[p >> 3] >> (7 - (p & 7))) & 1;
        ones += b;
        if (pos && b == bit) found = p;
    }
    *out = pos ? bits_pos_reply(found, bit, end_given, hi) : (int64_t)ones;
    return RBX_OK;
}

// ---- set-bit enumeration and the java.util.BitSet exchange (rules: members_rule.h) ----
static int members_args_check(rbx_ctx *c, rbx_name name, int nargs, int unit, uint64_t cap, const void *out,
                              const void *counts, const void *counts2) {
    if (!c || bad_name(name) || !counts || !counts2 || (cap && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (members_cmd_illegal(nargs, unit)) return fail(RBX_E_ILLEGAL_ARGUMENT, "nargs is 0 or 2, the unit BYTE or BIT");
    return RBX_OK;
}

// The key of one enumeration and its interval, inside the caller's scope on `st`, with the call's one wait for
// the length word.  *any = false: a missing key, an empty string or an empty interval, total = 0.
static int members_plan(rbx_ctx *c, rbx_name name, int nargs, int64_t start, int64_t end, int unit, hipStream_t st,
                        std::shared_ptr<Bitmap> *bm, uint64_t *len, uint64_t *lo, uint64_t *hi, bool *any) {
    *any = false;
    RBX_TRY(bitset_find(c, name_of(name), bm));
    if (!*bm) return RBX_OK;
    std::vector<uint64_t> lens;
    RBX_TRY(bitset_lens(c, {bm->get()}, st, &lens));
    *len = lens[0];
    *any = members_interval(nargs, start, end, unit, *len, lo, hi);
    return RBX_OK;
}

// The directory of the string (for this call only: any write would invalidate it), the page's state and counts,
// and -- d_out given -- the page itself.  The state words stay in mem_state for a later members_expand.
static int members_page_run(rbx_ctx *c, const Bitmap &bm, uint64_t len, uint64_t lo, uint64_t hi, uint64_t skip,
                            uint64_t cap, uint64_t *d_out, unsigned long long *d_counts, hipStream_t st) {
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.rng_dir.reserve((bits_dir_blocks(len) + 1) * 8));
    RBX_TRY(b.mem_state.reserve(64));
    auto *d_dir = b.rng_dir.as<unsigned long long>();
    launch_bits_directory(bm.d_words, len, d_dir, st);
    launch_members_head(bm.d_words, len, lo, hi, skip, cap, d_dir, b.mem_state.as<unsigned long long>(), d_counts, st);
    if (d_out) launch_members_expand(bm.d_words, len, lo, hi, d_dir, b.mem_state.as<unsigned long long>(), d_out, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

// set(BitSet) of n device words inside the caller's scope on `st`: one wait, for the highest set bit; then the key
// is replaced as bitmap_import replaces it
static int words_store(rbx_ctx *c, rbx_name name, const uint64_t *d_words, uint64_t n, hipStream_t st) {
    unsigned long long h1 = 0;
    if (n) {
        RBX_TRY(c->dev->bits.mem_state.reserve(64));
        auto *d_h = c->dev->bits.mem_state.as<unsigned long long>() + 7;
        HIP_TRY(hipMemsetAsync(d_h, 0, 8, st));
        launch_words_highest(d_words, n, d_h, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->dev->stage.words(), d_h, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h1 = *c->dev->stage.words();
    }
    if (h1 && words_bit_illegal(h1 - 1))
        return fail(RBX_E_ILLEGAL_ARGUMENT, "the highest set bit must be below 2^31 - 1 (java.util.BitSet.length() is an int)");
    const uint64_t bytes = words_string_len(h1 != 0, h1 ? h1 - 1 : 0);
    const std::string nm = name_of(name);
    std::shared_ptr<Bitmap> b;
    RBX_TRY(new_bitmap(c, import_bits(c, nm, bytes), st, &b));
    launch_words_import(d_words, n, bytes, b->d_words, b->d_len, st);
    HIP_TRY(hipGetLastError());
    c->ks.put(nm, Entry{KType::Bitmap, nullptr, b, nullptr});
    return RBX_OK;
}

// ---- the byte commands on one key (rbx_string_*; byte_cmd.h has the rules) ----
// what a command that failed alone reports (byte_cmd.h kByte*), single or in a stream
int byte_cmd_failed(int kind) {
    if (kind == kByteOk) return RBX_OK;
    if (kind == kByteWrongType) return fail(RBX_E_WRONGTYPE, kWrongTypeMsg);
    return fail(RBX_E_REDIS, kind == kByteBadOffset ? "ERR offset is out of range"
                                                    : "ERR string exceeds maximum allowed size (proto-max-bulk-len)");
}

// the string under `name` for a byte command inside the caller's scope: its bitmap (null: missing) and its length,
// read with the one wait on `st`
static int string_len(rbx_ctx *c, const std::string &nm, hipStream_t st, std::shared_ptr<Bitmap> *bm, uint64_t *len) {
    RBX_TRY(bitset_find(c, nm, bm));
    std::vector<uint64_t> lens;
    RBX_TRY(bitset_lens(c, {bm->get()}, st, &lens));
    *len = *bm ? std::min(lens[0], (*bm)->cap_bytes) : 0;
    return RBX_OK;
}

// the host forms' scratch is kept between calls up to this size; a larger one is given back behind the call's wait
static constexpr size_t kByteScratchKeep = 64u << 20;
static void string_scratch_trim(rbx_ctx *c) {
    if (c->dev->bits.by_bytes.cap > kByteScratchKeep) c->dev->bits.by_bytes.release();
}

// GETRANGE into device bytes (d_out) or, through the scratch, into host bytes (out)
static int string_getrange(rbx_ctx *c, rbx_name name, int64_t start, int64_t end, uint8_t *d_out, uint8_t *out, uint64_t cap,
                           uint64_t *len, hipStream_t st) {
    std::shared_ptr<Bitmap> bm;
    uint64_t L, lo = 0, hi = 0;
    RBX_TRY(string_len(c, name_of(name), st, &bm, &L));
    const uint64_t cnt = byte_getrange(start, end, L, &lo, &hi) ? hi - lo : 0;
    if (len) *len = cnt;
    const uint64_t wr = std::min(cap, cnt);
    if (wr == 0) return RBX_OK;
    if (out) {
        RBX_TRY(c->dev->bits.by_bytes.reserve(wr));
        d_out = c->dev->bits.by_bytes.as<uint8_t>();
    }
    launch_bytes_copy(d_out, (const uint8_t *)bm->d_words + lo, wr, g_tune.bytestream_tile, nullptr, 0, st);
    HIP_TRY(hipGetLastError());
    if (out) {
        HIP_TRY(hipMemcpyAsync(out, d_out, wr, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        string_scratch_trim(c);
    }
    return RBX_OK;
}

// SETRANGE / APPEND of n bytes from the device (d_bytes) or, through the scratch, from the host (bytes)
static int string_write(rbx_ctx *c, rbx_name name, int op, int64_t offset, const uint8_t *d_bytes, const uint8_t *bytes,
                        uint64_t n, uint64_t *new_len, hipStream_t st) {
    rbx_string_cmd cmd = {};
    cmd.op = (uint8_t)op;
    cmd.a = offset;
    cmd.val_len = (uint32_t)std::min<uint64_t>(n, kStrMax + 1);  // (a value above the limit fails at any offset)
    if (byte_key_step(0, true, false, cmd).fails == kByteBadOffset) return byte_cmd_failed(kByteBadOffset);
    const std::string nm = name_of(name);
    std::shared_ptr<Bitmap> bm;
    uint64_t L;
    RBX_TRY(string_len(c, nm, st, &bm, &L));
    const ByteStep s = byte_run_step(L, !bm, cmd);
    if (s.fails) return byte_cmd_failed(s.fails);
    if (new_len) *new_len = (uint64_t)s.reply;
    if (!s.writes) return RBX_OK;
    RBX_TRY(bitset_for_write(c, nm, s.len, st, &bm));
    if (bytes && s.cnt) {
        RBX_TRY(c->dev->bits.by_bytes.reserve(s.cnt));
        HIP_TRY(hipMemcpyAsync(c->dev->bits.by_bytes.p, bytes, s.cnt, hipMemcpyHostToDevice, st));
        d_bytes = c->dev->bits.by_bytes.as<uint8_t>();
    }
    launch_bytes_copy((uint8_t *)bm->d_words + s.at, d_bytes, s.cnt, g_tune.bytestream_tile, bm->d_len, s.len, st);
    HIP_TRY(hipGetLastError());
    if (bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        string_scratch_trim(c);
    }
    return RBX_OK;
}

}  // namespace rbx

using namespace rbx;

extern "C" int rbx_bench_bitrange_path(uint64_t len, uint64_t n, uint64_t total, uint64_t longest) {
    return ranges_take_directory(len, n, total, longest) ? 1 : 0;
}

extern "C" {

int rbx_bitset_get(rbx_ctx *c, rbx_name name, uint64_t index, int *bit) {
    if (!c || bad_name(name) || !bit) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (index >= kMaxBitOffset) return fail(RBX_E_REDIS, kBitOffsetMsg);
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_find(c, name_of(name), &bm));
    *bit = 0;
    if (!bm || (index >> 3) >= bm->cap_bytes) return RBX_OK;
    // one byte of the string (zero past its length) into a pinned word
    uint8_t *pin = (uint8_t *)c->dev->stage.words();
    HIP_TRY(hipMemcpyAsync(pin, (const uint8_t *)bm->d_words + (index >> 3), 1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *bit = (pin[0] >> (7 - (index & 7))) & 1;
    return RBX_OK;
}

int rbx_bitset_set(rbx_ctx *c, rbx_name name, uint64_t index, int value, int *old) {
    if (!c || bad_name(name)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (index >= kMaxBitOffset) return fail(RBX_E_REDIS, kBitOffsetMsg);
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_for_write(c, name_of(name), (index >> 3) + 1, c->stream, &bm));
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 1;
    launch_bits_set_one(bm->d_words, bm->d_len, index, value != 0, d, c->stream);
    HIP_TRY(hipGetLastError());
    int rc;
    const uint64_t was = read_dev_u64(c, d, &rc);
    if (old) *old = (int)was;
    return rc;
}

int rbx_bitset_set_indexes(rbx_ctx *c, rbx_name name, const uint64_t *indexes, uint64_t n, int value) {
    if (!c || bad_name(name) || (n && !indexes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n == 0) return RBX_OK;  // no command is sent
    const uint64_t mx = max_index(indexes, n);
    if (mx >= kMaxBitOffset) return fail(RBX_E_REDIS, kBitOffsetMsg);
    RBX_ENTER(c, c->stream);
    RBX_TRY(c->dev->bits.idx.reserve(n * 8));
    HIP_TRY(hipMemcpyAsync(c->dev->bits.idx.p, indexes, n * 8, hipMemcpyHostToDevice, c->stream));
    RBX_TRY(bitset_scatter(c, name_of(name), c->dev->bits.idx.as<uint64_t>(), n, mx, value, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

int rbx_bitset_get_indexes(rbx_ctx *c, rbx_name name, const uint64_t *indexes, uint64_t n, uint8_t *out) {
    if (!c || bad_name(name) || (n && (!indexes || !out))) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n == 0) return RBX_OK;
    if (max_index(indexes, n) >= kMaxBitOffset) return fail(RBX_E_REDIS, kBitOffsetMsg);
    RBX_ENTER(c, c->stream);
    RBX_TRY(c->dev->bits.idx.reserve(n * 8));
    RBX_TRY(c->dev->stage.out_bytes.reserve(n));
    HIP_TRY(hipMemcpyAsync(c->dev->bits.idx.p, indexes, n * 8, hipMemcpyHostToDevice, c->stream));
    RBX_TRY(bitset_gather(c, name_of(name), c->dev->bits.idx.as<uint64_t>(), n, c->dev->stage.out_bytes.as<uint8_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->dev->stage.out_bytes.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

int rbx_bitset_set_indexes_dev(rbx_ctx *c, rbx_name name, const uint64_t *d_indexes, uint64_t n, int value,
                               void *stream) {
    if (!c || bad_name(name) || (n && !d_indexes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n == 0) return RBX_OK;
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    uint64_t mx;
    RBX_TRY(max_index_dev(c, d_indexes, n, st, &mx));
    return bitset_scatter(c, name_of(name), d_indexes, n, mx, value, st);
}

int rbx_bitset_get_indexes_dev(rbx_ctx *c, rbx_name name, const uint64_t *d_indexes, uint64_t n, uint8_t *d_out,
                               void *stream) {
    if (!c || bad_name(name) || (n && (!d_indexes || !d_out))) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n == 0) return RBX_OK;
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    uint64_t mx;
    RBX_TRY(max_index_dev(c, d_indexes, n, st, &mx));
    return bitset_gather(c, name_of(name), d_indexes, n, d_out, st);
}

int rbx_bitset_set_range(rbx_ctx *c, rbx_name name, uint64_t from, uint64_t to, int value) {
    if (!c || bad_name(name)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (from >= to) return RBX_OK;  // an empty batch: no command is sent
    if (from >= kMaxBitOffset) return fail(RBX_E_REDIS, kBitOffsetMsg);
    // the batch's SETBITs below the limit run, the others fail: apply [from, 2^32), then report
    const bool past = to > kMaxBitOffset;
    if (past) to = kMaxBitOffset;
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_for_write(c, name_of(name), ((to - 1) >> 3) + 1, c->stream, &bm));
    launch_bits_fill(bm->d_words, bm->d_len, from, to, value != 0, c->stream);
    HIP_TRY(hipGetLastError());
    return past ? fail(RBX_E_REDIS, kBitOffsetMsg) : RBX_OK;
}

int rbx_bitset_op(rbx_ctx *c, int op, rbx_name dest, const rbx_name *srcs, uint32_t nsrc, uint64_t *result_len) {
    if (!c || bad_name(dest)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (op < RBX_BITOP_AND || op > RBX_BITOP_NOT) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown BITOP operation");
    if (nsrc == 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "BITOP needs a source key");
    if (op == RBX_BITOP_NOT && nsrc != 1)
        return fail(RBX_E_REDIS, kBitopNotMsg);
    std::vector<std::string> sn;
    RBX_TRY(names_of(srcs, nsrc, &sn));
    const std::string dn = name_of(dest);
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    // every operand's type first: a wrong one leaves dest untouched
    std::shared_ptr<Bitmap> db;
    RBX_TRY(bitset_find(c, dn, &db));
    std::vector<std::shared_ptr<Bitmap>> sb(nsrc);
    std::vector<Bitmap *> bms(nsrc + 1);
    for (uint32_t i = 0; i < nsrc; ++i) {
        RBX_TRY(bitset_find(c, sn[i], &sb[i]));
        bms[i] = sb[i].get();
    }
    bms[nsrc] = db.get();
    std::vector<uint64_t> lens;
    RBX_TRY(bitset_lens(c, bms, st, &lens));
    const uint64_t out_len = *std::max_element(lens.begin(), lens.begin() + nsrc);
    if (result_len) *result_len = out_len;
    if (out_len == 0) {  // the empty result: DEL dest
        c->ks.erase(dn);
        return RBX_OK;
    }
    RBX_TRY(bitset_for_write(c, dn, out_len, st, &db));
    // the table after dest has its final allocation: a source that is dest moved with it
    std::vector<BitopSrc> tab(nsrc);
    for (uint32_t i = 0; i < nsrc; ++i) tab[i] = BitopSrc{sb[i] ? (const uint8_t *)sb[i]->d_words : nullptr, lens[i]};
    RBX_TRY(c->dev->bits.bitop_srcs.reserve(nsrc * sizeof(BitopSrc)));
    // (a pageable source is staged by the runtime before the call returns)
    HIP_TRY(hipMemcpyAsync(c->dev->bits.bitop_srcs.p, tab.data(), nsrc * sizeof(BitopSrc), hipMemcpyHostToDevice, st));
    // the sweep also clears what a longer previous dest held past the result
    const uint64_t span = (std::max(out_len, lens[nsrc]) + 15) & ~15ULL;
    launch_bitop(op, (uint8_t *)db->d_words, db->d_len, c->dev->bits.bitop_srcs.as<BitopSrc>(), nsrc, out_len, span, st);
    HIP_TRY(hipGetLastError());
    if (Entry *e = c->ks.find(dn)) e->expire_at = -1;  // setKey without KEEPTTL
    return RBX_OK;
}

int rbx_bitset_cardinality(rbx_ctx *c, rbx_name name, uint64_t *out) {
    if (!c || bad_name(name) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    return bitcount_locked(c, name_of(name), out);
}

int rbx_bitset_size(rbx_ctx *c, rbx_name name, uint64_t *out) {
    if (!c || bad_name(name) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    uint64_t len;
    RBX_TRY(bitset_len(c, name, &bm, &len));
    *out = len * 8;
    return RBX_OK;
}

int rbx_bitset_length(rbx_ctx *c, rbx_name name, int64_t *out) {
    if (!c || bad_name(name) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    uint64_t len;
    RBX_TRY(bitset_len(c, name, &bm, &len));
    uint8_t *pin = (uint8_t *)c->dev->stage.words();
    pin[0] = pin[1] = 0;
    if (len) {  // the script reads the first and the last byte only
        const uint8_t *s = (const uint8_t *)bm->d_words;
        HIP_TRY(hipMemcpyAsync(pin, s, 1, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(pin + 1, s + len - 1, 1, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return bitset_length(len, pin[0], pin[1], out);
}

int rbx_bitset_length_of(const uint8_t *bytes, uint64_t len, int64_t *out) { return bitset_length_of(bytes, len, out); }

int rbx_bitset_export_n(rbx_ctx *c, rbx_name name, uint8_t *out, uint64_t cap, uint64_t *redis_len) {
    if (!c || bad_name(name)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bitmap_export(c, name_of(name), out, cap, redis_len);
}

int rbx_bitset_import_n(rbx_ctx *c, rbx_name name, const uint8_t *bytes, uint64_t len) {
    if (!c || bad_name(name) || (len && !bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    return bitmap_import(c, name_of(name), bytes, len);
}

int rbx_bitset_as_words_dev(rbx_ctx *c, rbx_name name, uint64_t *d_words, uint64_t cap_words, uint64_t *d_nwords,
                            void *stream) {
    if (!c || bad_name(name) || !d_nwords || (cap_words && !d_words)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_find(c, name_of(name), &bm));
    HIP_TRY(hipMemsetAsync(d_nwords, 0, 8, st));
    if (!bm) return RBX_OK;
    launch_words_last(bm->d_words, bm->cap_bytes, bm->d_len, (unsigned long long *)d_nwords, st);
    launch_words_export(bm->d_words, bm->cap_bytes, (const unsigned long long *)d_nwords, cap_words, d_words, st);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bitset_as_words(rbx_ctx *c, rbx_name name, uint64_t *words, uint64_t cap_words, uint64_t *nwords) {
    if (!c || bad_name(name) || !nwords || (cap_words && !words)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    std::shared_ptr<Bitmap> bm;
    RBX_TRY(bitset_find(c, name_of(name), &bm));
    *nwords = 0;
    if (!bm) return RBX_OK;
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.mem_state.reserve(64));
    auto *d_n = b.mem_state.as<unsigned long long>() + 6;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, st));
    launch_words_last(bm->d_words, bm->cap_bytes, bm->d_len, d_n, st);
    HIP_TRY(hipGetLastError());
    int rc;
    *nwords = read_dev_u64(c, d_n, &rc);
    RBX_TRY(rc);
    const uint64_t m = std::min(cap_words, *nwords);
    if (m == 0) return RBX_OK;
    RBX_TRY(b.mem_buf.reserve(m * 8));
    launch_words_export(bm->d_words, bm->cap_bytes, d_n, m, b.mem_buf.as<uint64_t>(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(words, b.mem_buf.p, m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBX_OK;
}

int rbx_bitset_set_words_dev(rbx_ctx *c, rbx_name name, const uint64_t *d_words, uint64_t nwords, void *stream) {
    if (!c || bad_name(name) || (nwords && !d_words)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    return words_store(c, name, d_words, nwords, st);
}

int rbx_bitset_set_words(rbx_ctx *c, rbx_name name, const uint64_t *words, uint64_t nwords) {
    if (!c || bad_name(name) || (nwords && !words)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    while (nwords && words[nwords - 1] == 0) --nwords;  // trailing zero words are not uploaded
    if (nwords > (1ULL << 25)) return fail(RBX_E_ILLEGAL_ARGUMENT, "the highest set bit must be below 2^31 - 1 (java.util.BitSet.length() is an int)");
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    RBX_TRY(c->dev->bits.mem_buf.reserve(nwords * 8));
    if (nwords) HIP_TRY(hipMemcpyAsync(c->dev->bits.mem_buf.p, words, nwords * 8, hipMemcpyHostToDevice, st));
    RBX_TRY(words_store(c, name, c->dev->bits.mem_buf.as<uint64_t>(), nwords, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBX_OK;
}

int rbx_bitset_as_words_of(const uint8_t *bytes, uint64_t len, uint64_t *words, uint64_t cap_words, uint64_t *nwords) {
    if ((len && !bytes) || !nwords || (cap_words && !words)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    uint64_t last = len;  // the bytes up to the last non-zero one
    while (last && bytes[last - 1] == 0) --last;
    *nwords = words_in_use(last != 0, last ? (last - 1) / 8 : 0);
    const uint64_t m = std::min(cap_words, *nwords);
    for (uint64_t w = 0; w < m; ++w) {
        uint64_t v = 0;
        for (uint64_t k = 0; k < 8 && 8 * w + k < last; ++k) v |= (uint64_t)(rev_bytes(bytes[8 * w + k]) & 0xFFu) << (8 * k);
        words[w] = v;
    }
    return RBX_OK;
}

int rbx_bitset_bytes_of_words(const uint64_t *words, uint64_t nwords, uint8_t *out, uint64_t cap, uint64_t *len) {
    if ((nwords && !words) || !len || (cap && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    while (nwords && words[nwords - 1] == 0) --nwords;
    const uint64_t highest = nwords ? words_highest(nwords - 1, words[nwords - 1]) : 0;
    if (nwords && words_bit_illegal(highest))
        return fail(RBX_E_ILLEGAL_ARGUMENT, "the highest set bit must be below 2^31 - 1 (java.util.BitSet.length() is an int)");
    *len = words_string_len(nwords != 0, highest);
    const uint64_t m = std::min(cap, *len);
    for (uint64_t i = 0; i < m; ++i)
        out[i] = i / 8 < nwords ? (uint8_t)rev_bytes((uint32_t)(words[i / 8] >> (8 * (i % 8))) & 0xFFu) : 0;
    return RBX_OK;
}

int rbx_bitset_members_dev(rbx_ctx *c, rbx_name name, int nargs, int64_t start, int64_t end, int unit, uint64_t skip,
                           uint64_t cap, uint64_t *d_out, uint64_t *d_counts, void *stream) {
    RBX_TRY(members_args_check(c, name, nargs, unit, cap, d_out, d_counts, d_counts));
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    std::shared_ptr<Bitmap> bm;
    uint64_t len, lo, hi;
    bool any;
    RBX_TRY(members_plan(c, name, nargs, start, end, unit, st, &bm, &len, &lo, &hi, &any));
    if (!any) {
        HIP_TRY(hipMemsetAsync(d_counts, 0, 16, st));
        return RBX_OK;
    }
    return members_page_run(c, *bm, len, lo, hi, skip, cap, cap ? d_out : nullptr, (unsigned long long *)d_counts, st);
}

int rbx_bitset_members(rbx_ctx *c, rbx_name name, int nargs, int64_t start, int64_t end, int unit, uint64_t skip,
                       uint64_t cap, uint64_t *out, uint64_t *written, uint64_t *total) {
    RBX_TRY(members_args_check(c, name, nargs, unit, cap, out, written, total));
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    std::shared_ptr<Bitmap> bm;
    uint64_t len, lo, hi;
    bool any;
    RBX_TRY(members_plan(c, name, nargs, start, end, unit, st, &bm, &len, &lo, &hi, &any));
    *written = *total = 0;
    if (!any) return RBX_OK;
    BitsetScratch &b = c->dev->bits;
    RBX_TRY(b.mem_state.reserve(64));
    auto *d_counts = b.mem_state.as<unsigned long long>() + 4;  // behind the state words
    RBX_TRY(members_page_run(c, *bm, len, lo, hi, skip, cap, nullptr, d_counts, st));
    unsigned long long *w = c->dev->stage.words();
    HIP_TRY(hipMemcpyAsync(w, d_counts, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *written = w[0];
    *total = w[1];
    if (*written == 0) return RBX_OK;
    RBX_TRY(b.mem_buf.reserve(*written * 8));  // the page's size is known only now
    launch_members_expand(bm->d_words, len, lo, hi, b.rng_dir.as<unsigned long long>(), b.mem_state.as<unsigned long long>(),
                          b.mem_buf.as<uint64_t>(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, b.mem_buf.p, *written * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBX_OK;
}

int rbx_bitset_members_of(const uint8_t *bytes, uint64_t len, int missing, const rbx_members_cmd *cmd, uint64_t cap,
                          uint64_t *out, uint64_t *written, uint64_t *total) {
    if ((len && !bytes) || !cmd || !written || !total || (cap && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (members_cmd_illegal(cmd->nargs, cmd->unit)) return fail(RBX_E_ILLEGAL_ARGUMENT, "nargs is 0 or 2, the unit BYTE or BIT");
    *written = *total = 0;
    uint64_t lo, hi;
    if (!members_interval(cmd->nargs, cmd->start, cmd->end, cmd->unit, missing ? 0 : len, &lo, &hi)) return RBX_OK;
    uint64_t ones = 0;
    for (uint64_t p = lo; p <= hi; ++p) ones += (bytes[p >> 3] >> (7 - (p & 7))) & 1;
    uint64_t first, count, rank = 0;
    members_page(ones, cmd->skip, cmd->limit, cap, &first, &count);
    for (uint64_t p = lo; p <= hi && rank < first + count; ++p) {
        if (!((bytes[p >> 3] >> (7 - (p & 7))) & 1)) continue;
        if (rank >= first) out[rank - first] = p;
        ++rank;
    }
    *written = count;
    *total = ones;
    return RBX_OK;
}

int rbx_bitset_rename(rbx_ctx *c, rbx_name name, rbx_name new_name) {
    if (!c || bad_name(name) || bad_name(new_name)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    return c->ks.rename(name_of(name), name_of(new_name));
}

int rbx_bitset_field_of(const uint8_t *bytes, uint64_t len, int is_signed, int size, uint64_t offset, int64_t *out) {
    if ((len && !bytes) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(field_type_check(RBX_FIELD_GET, is_signed, size));
    RBX_TRY(field_range_check(offset, size));
    *out = field_of_bytes(bytes, len, is_signed, size, offset);
    return RBX_OK;
}

int rbx_bitset_count_range(rbx_ctx *c, rbx_name name, int64_t start, int64_t end, int unit, uint64_t *out) {
    if (!c || bad_name(name) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(range_unit_check(unit));
    return range_single(c, name, false, 0, start, end, true, unit, (int64_t *)out);
}

int rbx_bitset_pos(rbx_ctx *c, rbx_name name, int bit, int nargs, int64_t start, int64_t end, int unit, int64_t *out) {
    if (!c || bad_name(name) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (nargs < 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "nargs is 0, 1 or 2");
    RBX_TRY(pos_args_check(bit, nargs, unit));
    return range_single(c, name, true, bit, nargs >= 1 ? start : 0, end, nargs == 2, unit, out);
}

int rbx_bitset_count_ranges(rbx_ctx *c, rbx_name name, const int64_t *starts, const int64_t *ends, uint64_t n, int unit,
                            uint64_t *out) {
    RBX_TRY(ranges_args_check(c, name, false, 0, starts, ends, n, unit, out));
    if (n == 0) return RBX_OK;  // no command is sent
    if (n == 1) return rbx_bitset_count_range(c, name, starts[0], ends[0], unit, out);
    return ranges_host(c, name, false, 0, starts, ends, n, unit, out);
}

int rbx_bitset_pos_ranges(rbx_ctx *c, rbx_name name, int bit, const int64_t *starts, const int64_t *ends, uint64_t n,
                          int unit, int64_t *out) {
    RBX_TRY(ranges_args_check(c, name, true, bit, starts, ends, n, unit, out));
    if (n == 0) return RBX_OK;
    if (n == 1) return rbx_bitset_pos(c, name, bit, ends ? 2 : 1, starts[0], ends ? ends[0] : 0, unit, out);
    return ranges_host(c, name, true, bit, starts, ends, n, unit, out);
}

int rbx_bitset_count_ranges_dev(rbx_ctx *c, rbx_name name, const int64_t *d_starts, const int64_t *d_ends, uint64_t n,
                                int unit, uint64_t *d_out, void *stream) {
    RBX_TRY(ranges_args_check(c, name, false, 0, d_starts, d_ends, n, unit, d_out));
    if (n == 0) return RBX_OK;
    return ranges_dev(c, name, false, 0, d_starts, d_ends, n, unit, d_out, pick_stream(c, stream));
}

int rbx_bitset_pos_ranges_dev(rbx_ctx *c, rbx_name name, int bit, const int64_t *d_starts, const int64_t *d_ends,
                              uint64_t n, int unit, int64_t *d_out, void *stream) {
    RBX_TRY(ranges_args_check(c, name, true, bit, d_starts, d_ends, n, unit, d_out));
    if (n == 0) return RBX_OK;
    return ranges_dev(c, name, true, bit, d_starts, d_ends, n, unit, d_out, pick_stream(c, stream));
}

int rbx_bitset_count_of(const uint8_t *bytes, uint64_t len, int missing, int64_t start, int64_t end, int unit,
                        uint64_t *out) {
    if ((len && !bytes) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(range_unit_check(unit));
    return range_of(bytes, len, missing, false, 0, start, end, true, unit, (int64_t *)out);
}

int rbx_bitset_pos_of(const uint8_t *bytes, uint64_t len, int missing, int bit, int nargs, int64_t start, int64_t end,
                      int unit, int64_t *out) {
    if ((len && !bytes) || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (nargs < 0) return fail(RBX_E_ILLEGAL_ARGUMENT, "nargs is 0, 1 or 2");
    RBX_TRY(pos_args_check(bit, nargs, unit));
    return range_of(bytes, len, missing, true, bit, nargs >= 1 ? start : 0, end, nargs == 2, unit, out);
}

int rbx_bitset_field(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, uint64_t offset, int64_t value,
                     int64_t *reply) {
    if (!c || bad_name(name) || (op == RBX_FIELD_GET && !reply)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_TRY(field_type_check(op, is_signed, size));
    RBX_TRY(field_range_check(offset, size));
    RBX_ENTER(c, c->stream);
    std::shared_ptr<Bitmap> bm;
    if (op == RBX_FIELD_GET) {
        RBX_TRY(bitset_find(c, name_of(name), &bm));
        // the field's covering bytes inside the allocation (zero past the string's length), at most 9
        uint8_t *pin = (uint8_t *)c->dev->stage.words();
        const uint64_t first = offset >> 3, last = (offset + size - 1) >> 3;
        uint64_t nb = 0;
        if (bm && first < bm->cap_bytes) {
            nb = std::min<uint64_t>(last + 1, bm->cap_bytes) - first;
            HIP_TRY(hipMemcpyAsync(pin, (const uint8_t *)bm->d_words + first, nb, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        *reply = field_of_bytes(pin, nb, is_signed, size, offset & 7);
        return RBX_OK;
    }
    const uint64_t need = ((offset + size - 1) >> 3) + 1;
    RBX_TRY(bitset_for_write(c, name_of(name), need, c->stream, &bm));
    RBX_TRY(c->dev->shared.counters.reserve(64));
    auto *d = c->dev->shared.counters.as<unsigned long long>() + 1;
    launch_field_one(bm->d_words, bm->d_len, bm->cap_bytes, op, is_signed, size, offset, value, (int64_t *)d, need,
                     c->stream);
    HIP_TRY(hipGetLastError());
    int rc;
    const uint64_t r = read_dev_u64(c, d, &rc);
    if (reply) *reply = (int64_t)r;
    return rc;
}

int rbx_bitset_fields(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, const uint64_t *offsets,
                      const int64_t *values, uint64_t n, int64_t *replies) {
    RBX_TRY(fields_args_check(c, name, op, is_signed, size, offsets, values, n, replies));
    return fields_host(c, name, op, is_signed, size, RBX_OVERFLOW_WRAP, offsets, values, n, replies, nullptr);
}

int rbx_bitset_fields_dev(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, const uint64_t *d_offsets,
                          const int64_t *d_values, uint64_t n, int64_t *d_replies, void *stream) {
    RBX_TRY(fields_args_check(c, name, op, is_signed, size, d_offsets, d_values, n, d_replies));
    return fields_dev(c, name, op, is_signed, size, RBX_OVERFLOW_WRAP, d_offsets, d_values, n, d_replies, nullptr,
                      stream);
}

int rbx_bitset_fields_ov(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, int overflow,
                         const uint64_t *offsets, const int64_t *values, uint64_t n, int64_t *replies, uint8_t *nil) {
    RBX_TRY(fields_args_check(c, name, op, is_signed, size, offsets, values, n, replies));
    RBX_TRY(nil_args_check(op, overflow, n, replies, nil));
    return fields_host(c, name, op, is_signed, size, overflow, offsets, values, n, replies, nil);
}

int rbx_bitset_fields_ov_dev(rbx_ctx *c, rbx_name name, int op, int is_signed, int size, int overflow,
                             const uint64_t *d_offsets, const int64_t *d_values, uint64_t n, int64_t *d_replies,
                             uint8_t *d_nil, void *stream) {
    RBX_TRY(fields_args_check(c, name, op, is_signed, size, d_offsets, d_values, n, d_replies));
    RBX_TRY(nil_args_check(op, overflow, n, d_replies, d_nil));
    return fields_dev(c, name, op, is_signed, size, overflow, d_offsets, d_values, n, d_replies, d_nil, stream);
}

int rbx_bitset_bitfield(rbx_ctx *c, rbx_name name, const rbx_field_cmd *cmds, uint64_t n, int64_t *replies,
                        uint8_t *nil) {
    if (!c || bad_name(name) || (n && !cmds)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (n == 0) return RBX_OK;  // no command is sent
    // every sub-command's checks before any effect; the growth is that of the writes, failing ones included
    bool same = true, writes = false, gets = false, fails = false;
    uint64_t need = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const rbx_field_cmd &k = cmds[i];
        if (k.op > RBX_FIELD_INCRBY) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown BITFIELD operation");
        RBX_TRY(overflow_check(k.overflow));
        if (k.is_signed > 1) return fail(RBX_E_ILLEGAL_ARGUMENT, "is_signed is 0 or 1");
        const int bad = field_cmd_check(k.is_signed, k.size, k.offset);  // the type, then the offset limit
        if (bad) return fail(RBX_E_REDIS, bad == kFieldCmdBadType ? kFieldTypeMsg : kBitOffsetMsg);
        same &= k.op == cmds[0].op && k.is_signed == cmds[0].is_signed && k.size == cmds[0].size &&
                (k.op == RBX_FIELD_GET || k.overflow == cmds[0].overflow);
        if (k.op == RBX_FIELD_GET) {
            gets = true;
        } else {
            writes = true;
            fails |= k.overflow == RBX_OVERFLOW_FAIL;
            need = std::max<uint64_t>(need, ((k.offset + k.size - 1) >> 3) + 1);
        }
    }
    if (gets && !replies) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (fails && replies && !nil) return fail(RBX_E_ILLEGAL_ARGUMENT, "OVERFLOW FAIL with replies needs nil");
    if (same) {  // one operation, type and mode: the batch paths
        std::vector<uint64_t> offs(n);
        std::vector<int64_t> vals(n);
        for (uint64_t i = 0; i < n; ++i) {
            offs[i] = cmds[i].offset;
            vals[i] = cmds[i].value;
        }
        return fields_host(c, name, cmds[0].op, cmds[0].is_signed, cmds[0].size, cmds[0].overflow, offs.data(),
                           vals.data(), n, replies, nil);
    }
    RBX_ENTER(c, c->stream);
    BitsetScratch &b = c->dev->bits;
    std::shared_ptr<Bitmap> bm;
    if (writes)
        RBX_TRY(bitset_for_write(c, name_of(name), need, c->stream, &bm));
    else
        RBX_TRY(bitset_find(c, name_of(name), &bm));
    RBX_TRY(b.fld_cmds.reserve(n * sizeof(rbx_field_cmd)));
    RBX_TRY(b.fld_out.reserve(n * 8));
    RBX_TRY(b.fld_nil.reserve(n));
    HIP_TRY(hipMemcpyAsync(b.fld_cmds.p, cmds, n * sizeof(rbx_field_cmd), hipMemcpyHostToDevice, c->stream));
    launch_bitfield_serial(bm ? bm->d_words : nullptr, bm ? bm->d_len : nullptr, bm ? bm->cap_bytes : 0,
                           b.fld_cmds.as<rbx_field_cmd>(), n, b.fld_out.as<int64_t>(), b.fld_nil.as<uint8_t>(), need,
                           c->stream);
    HIP_TRY(hipGetLastError());
    if (replies) HIP_TRY(hipMemcpyAsync(replies, b.fld_out.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (nil) HIP_TRY(hipMemcpyAsync(nil, b.fld_nil.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

int rbx_bitset_field_rule(int op, int is_signed, int size, int overflow, int64_t old, int64_t value, int64_t *now,
                          int64_t *reply, int *nil) {
    if (!now || !reply || !nil) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (op < RBX_FIELD_GET || op > RBX_FIELD_INCRBY) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown BITFIELD operation");
    RBX_TRY(overflow_check(overflow));
    if (size < 1 || size > (is_signed ? 64 : 63)) return fail(RBX_E_REDIS, kFieldTypeMsg);
    if (field_typed((uint64_t)old, size, is_signed) != old)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "old is outside the type's range");
    *nil = field_rule(op, is_signed ? 1 : 0, size, overflow, old, value, now, reply) ? 1 : 0;
    return RBX_OK;
}

int rbx_string_getrange(rbx_ctx *c, rbx_name name, int64_t start, int64_t end, uint8_t *out, uint64_t cap, uint64_t *len) {
    if (!c || bad_name(name) || (cap && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    return string_getrange(c, name, start, end, nullptr, out, out ? cap : 0, len, c->stream);
}

int rbx_string_getrange_dev(rbx_ctx *c, rbx_name name, int64_t start, int64_t end, uint8_t *d_out, uint64_t cap,
                            uint64_t *len, void *stream) {
    if (!c || bad_name(name) || (cap && !d_out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    return string_getrange(c, name, start, end, d_out, nullptr, cap, len, st);
}

int rbx_string_setrange(rbx_ctx *c, rbx_name name, int64_t offset, const uint8_t *bytes, uint64_t n, uint64_t *new_len) {
    if (!c || bad_name(name) || (n && !bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    return string_write(c, name, RBX_STR_SETRANGE, offset, nullptr, n ? bytes : nullptr, n, new_len, c->stream);
}

int rbx_string_setrange_dev(rbx_ctx *c, rbx_name name, int64_t offset, const uint8_t *d_bytes, uint64_t n,
                            uint64_t *new_len, void *stream) {
    if (!c || bad_name(name) || (n && !d_bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    return string_write(c, name, RBX_STR_SETRANGE, offset, d_bytes, nullptr, n, new_len, st);
}

int rbx_string_append(rbx_ctx *c, rbx_name name, const uint8_t *bytes, uint64_t n, uint64_t *new_len) {
    if (!c || bad_name(name) || (n && !bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    RBX_ENTER(c, c->stream);
    return string_write(c, name, RBX_STR_APPEND, 0, nullptr, n ? bytes : nullptr, n, new_len, c->stream);
}

int rbx_string_append_dev(rbx_ctx *c, rbx_name name, const uint8_t *d_bytes, uint64_t n, uint64_t *new_len, void *stream) {
    if (!c || bad_name(name) || (n && !d_bytes)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = pick_stream(c, stream);
    RBX_ENTER(c, st);
    return string_write(c, name, RBX_STR_APPEND, 0, d_bytes, nullptr, n, new_len, st);
}

// M/RedissonBinaryStream.java:181-190: STRLEN; if size >= len return; GETRANGE key 0 size-1; SET key that.  The
// GETRANGE starts at 0, so what it keeps is a prefix: the SET is the string cut in place, what it cuts off cleared.
int rbx_string_truncate(rbx_ctx *c, rbx_name name, int64_t size) {
    if (!c || bad_name(name)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    hipStream_t st = c->stream;
    RBX_ENTER(c, st);
    const std::string nm = name_of(name);
    std::shared_ptr<Bitmap> bm;
    uint64_t L, lo = 0, hi = 0;
    RBX_TRY(string_len(c, nm, st, &bm, &L));
    if (size >= (int64_t)L) return RBX_OK;
    if (!bm) return bitmap_import(c, nm, nullptr, 0);  // a negative size on a missing key: SET key ""
    // (size - 1 for the smallest size is clamped; every end below -L gives the empty reply alike)
    const uint64_t keep = byte_getrange(0, size > INT64_MIN ? size - 1 : INT64_MIN, L, &lo, &hi) ? hi : 0;
    if (keep < L) HIP_TRY(hipMemsetAsync((uint8_t *)bm->d_words + keep, 0, L - keep, st));
    launch_bytes_copy(nullptr, nullptr, 0, g_tune.bytestream_tile, bm->d_len, keep, st);
    HIP_TRY(hipGetLastError());
    if (Entry *e = c->ks.find(nm)) e->expire_at = -1;  // SET without KEEPTTL
    HIP_TRY(hipStreamSynchronize(st));
    return RBX_OK;
}

int rbx_string_range_of(const uint8_t *bytes, uint64_t len, int missing, const rbx_string_cmd *cmd, const uint8_t *vals,
                        uint8_t *out, uint64_t cap, int64_t *reply, uint64_t *new_len) {
    (void)vals;  // a write stores nothing here
    if (!cmd || !reply) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    if (cmd->op > RBX_STR_GET) return fail(RBX_E_ILLEGAL_ARGUMENT, "unknown string command");
    if (len > kStrMax) return fail(RBX_E_ILLEGAL_ARGUMENT, "string exceeds the 512 MiB Redis limit");
    if (missing) len = 0;
    *reply = 0;
    if (new_len) *new_len = len;
    const ByteStep s = byte_run_step(len, missing != 0, *cmd);
    if (s.fails) return byte_cmd_failed(s.fails);
    if (new_len) *new_len = s.len;
    *reply = s.nil ? -1 : s.reply;
    if (!s.writes && s.cnt) {
        const uint64_t wr = std::min(cap, s.cnt);
        if (!bytes || (wr && !out)) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
        memcpy(out, bytes + s.at, wr);
    }
    return RBX_OK;
}

}  // extern "C"
