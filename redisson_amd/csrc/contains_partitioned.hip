// contains_partitioned.hip -- RBloomFilter.contains(Collection) for one large filter
// (M/RedissonBloomFilter.java:153-186) with the bitmap probed from LDS instead of HBM.
//
// Why: a uniformly random 4-byte gather that misses L2 costs one fabric request (measured
// ~55 G requests/s chip-wide, flat from 64 MiB to 1 GiB working sets), the same request rate a
// 128-byte streaming read gets.  A 100M-key batch issues ~4e8 such gathers into a 512 MiB bitmap
// (4.2M cache lines), i.e. ~100 requests per line.  Routing the probes through one streaming
// radix pass turns almost all of them into 5-byte entries of whole-line streaming requests (twelve
// to a 64-byte line: a 21-bit offset inside the region and a 19-bit key index local to the stage-1
// block that wrote the segment, bk_entry.h), and the bitmap itself is read once, a 128 KiB slice at
// a time, into LDS.
//
//   K1 stage1 : hash every key, test bit 0 with one random gather (a key is absent at its first
//               0 bit, and on a lightly filled filter most absent keys fail here); `alive` bit per
//               key; the survivors' k-1 remaining bits become (bit offset, key index) entries, bucketed
//               by 256 KiB bitmap region (<= 2048 buckets) through one 64-byte line buffer per
//               bucket in LDS; a full buffer is stored as one whole line into the segment that
//               this block owns for the bucket (no global reservations).
//   K4 probe  : a cluster of two workgroups per region, each holding one 128 KiB slice (half) of it
//               in LDS.  Both workgroups stream all of the region's segments and test the entries
//               that fall into their slice; a clear bit (only keys that survived stage 1 by chance)
//               rebuilds the chunk's key id and records it, bucketed by 2^19-key range.  The workgroups of a cluster share
//               blockIdx % 8 and are adjacent in dispatch order, so they tend to share an XCD and
//               one of the two reads of a segment is served by its L2.  They never communicate:
//               placement changes only the speed.
//   K5 misses : records -> LDS image of the range's miss words -> OR-ed into `miss`.
//   K6 final  : present = alive AND NOT miss; count (+ per-key bytes).
// Measured bound (rocprof PMC, C2): every kernel runs at ~50 G memory requests/s at the L2->EA
// interface (a read moves 128 B, a write 64 B, an atomic is one request), the same rate the
// direct kernel's random gathers get; fewer requests per key is the only lever.
// Segments have a fixed capacity sized for "every key survives"; an entry that does not fit (only
// for adversarial batches, e.g. one key repeated 1e8 times) is probed directly from HBM where it
// overflows, so the answer is exact in every case.  The answer per key is the AND of its k bits,
// exactly as the direct kernel (bloom_kernels.hip) computes it.
#include "bucket_common.h"

namespace rbx {

// The entries [s0, fill) at stride `step` of bucket b's line buffer (at most kBkLineEntries real ones), whose
// segment is full: decode them (bk_entry.h) and test their bits in HBM
__device__ __forceinline__ void bk_direct(const unsigned long long *line, uint32_t b, uint32_t s0, uint32_t step,
                                          uint32_t fill, uint32_t G, const uint32_t *__restrict__ bm,
                                          unsigned long long *__restrict__ miss) {
    const uint32_t *words = (const uint32_t *)line;
    const uint8_t *his = (const uint8_t *)line + kBkLineHiByte;
    for (uint32_t s = s0; s < fill; s += step) {
        const uint32_t w = words[s];
        const uint32_t idx = (b << kBkBucketBits) | bk_off(w), key = bk_key(bk_q_of(w, his[s]), blockIdx.x, G);
        if ((bm[idx >> 5] & bit_in_word(idx)) == 0u) atomicOr(&miss[key >> 6], 1ULL << (key & 63));
    }
}

// entry (off, q) into slot s < kBkLineEntries of a line buffer: one u32 and one u8 LDS store
__device__ __forceinline__ void bk_place(unsigned long long *line, uint32_t s, uint32_t off, uint32_t q) {
    ((uint32_t *)line)[s] = bk_word(off, q);
    ((uint8_t *)line)[kBkLineHiByte + s] = bk_hi(q);
}

// K1 -----------------------------------------------------------------------------------
// Tile = NT * PER keys; a persistent grid of G <= 256 blocks strides over the tiles.  Hash, test
// bit 0 (one random gather per key), then each of the survivors' k-1 remaining bits takes a slot
// of its bucket's line buffer (one LDS atomic) and is placed there as a 5-byte entry (bk_entry.h:
// twelve to a line; the key is the block-local q = tile iteration * 1024 + thread).  An entry whose
// slot is past the line stays in its registers until a flush round has stored the line: a round
// stores every full line (eight lanes per bucket copy its eight u64, one 64-byte store; the copy does
// not interpret entries), then the pending entries move down by one line.  One round per tile is the
// common case; many entries of one bucket in one tile (a repeated key) take more.  A partial line
// costs a full write request, and this way only a block's last line per bucket is partial; it is
// stored whole (the byte plane sits at the line's end), its stale tail is never read as entries: the
// count says how many are real.  Block blk owns segment (b, blk) of every bucket b, so nothing is
// reserved globally and every block writes its nb counts at its end (segcnt needs no clearing).
constexpr uint32_t kBkNoSlot = 0xffffffffu;

template <int KLEN, int KMAX, int NT, int PER>
__global__ __launch_bounds__(NT) void k_bk_stage1(KeysDev keys, uint64_t base, uint64_t nchunk,
                                                   const uint32_t *__restrict__ bm, ModParams mp, uint32_t k,
                                                   uint32_t nb, uint64_t capS,
                                                   unsigned long long *__restrict__ pairs, uint32_t *__restrict__ segcnt,
                                                   unsigned long long *__restrict__ alive,
                                                   unsigned long long *__restrict__ miss, uint32_t flags) {
    if (!kDiag) flags = 0;  // wrong-answer diagnostics exist in the profiling build only (rbx_kernels.h)
    constexpr int TILE = NT * PER, NP = PER * (KMAX - 1);
    static_assert(TILE == (int)kBkTileKeys, "q = tile iteration * kBkTileKeys + the key's place in the tile");
    constexpr uint32_t LE = kBkLineEntries, LW = kBkLineWords;
    // 2048 line buffers are 128 KiB, 152 KiB with the counters and lists: one block per CU
    __shared__ __attribute__((aligned(16))) unsigned long long s_buf[kBkMaxBuckets * LW];
    __shared__ uint32_t s_fill[kBkMaxBuckets];  // entries in the bucket's line buffer (and pending past it)
    __shared__ uint32_t s_out[kBkMaxBuckets];   // entries of the bucket this block has stored
    // the buckets that hold a full line, for this flush round and the next: the pair that takes a
    // line's last slot lists its bucket, so a round visits full lines only, not all nb buckets
    __shared__ uint16_t s_list[2][kBkMaxBuckets];
    __shared__ uint32_t s_nlist[2];
    const uint64_t ntiles = (nchunk + TILE - 1) / TILE;
    const uint32_t lane = threadIdx.x & 63, lane8 = threadIdx.x & (LW - 1);
    // Segment (bucket b, stage-1 block blk) of nb buckets starts at line (blk * nb + b) * capS / 12.
    // Block-major: a block's nb segments are adjacent, so its line stores stay inside nb * capS entries
    // (C2: 23 MB) and the probe reads a region's segments at that stride (bucket-major, a region's
    // segments adjacent, measured slower: DESIGN.md §3.6 r07).
    const uint32_t G = gridDim.x;
    const uint64_t capW = capS / LE * LW;  // a segment in u64
    unsigned long long *seg0 = pairs + bk_seg_line(0, blockIdx.x, nb, capS) * LW;
    for (uint32_t b = threadIdx.x; b < nb; b += NT) s_fill[b] = s_out[b] = 0;
    if (threadIdx.x < 2) s_nlist[threadIdx.x] = 0;
    uint32_t cur = 0;  // the list the pairs' slots are filling
    // Software-pipelined over tiles: tile t+1's hash and bit-0 gather are issued once tile t's
    // pairs have their slots, so the gather has the flush rounds to land.
    uint64_t h1[PER], h2[PER];
    uint32_t w[PER], m[PER];
    auto hash_tile = [&](uint64_t tl) {
        const uint64_t tt0 = tl * TILE + threadIdx.x;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const uint64_t t = tt0 + q * NT;
            h1[q] = h2[q] = 0;
            // Generic key length: the hash's reset words, hoisted out of the tile loop, took 32 of a
            // 1024-thread block's 128 VGPRs per thread and made k > 8 spill; a zero the compiler
            // cannot see through keeps them literals (hh128_bytes).
            uint64_t zero = 0;
            if constexpr (KLEN == 0) {
                uint32_t z = 0;
                asm volatile("" : "+v"(z));
                zero = ((uint64_t)z << 32) | z;
            }
            if (t < nchunk) hash_key<KLEN>(keys, base + t, h1[q], h2[q], zero);
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const uint64_t t = tt0 + q * NT;
            w[q] = 0;
            m[q] = 0;
            if (t < nchunk) {
                const uint32_t idx = BloomSeq::index_of(h1[q], mp);
                m[q] = bit_in_word(idx);
                // diagnostics (flags 32, wrong answers): no bit-0 gather; ~54% of keys survive
                if (flags & 32) w[q] = (uint32_t)(h2[q] >> 40) % 100u < 54u ? m[q] : 0u;
                else w[q] = bm[idx >> 5];
            }
        }
    };
    if ((uint64_t)blockIdx.x < ntiles) hash_tile(blockIdx.x);
    __syncthreads();
    uint32_t q0 = threadIdx.x;  // bk_q(tile iteration, thread): the host's chunk rule keeps it below 2^19
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += G, q0 += TILE) {
        const uint64_t t0 = tile * TILE + threadIdx.x;
        uint32_t idx[NP], slot[NP];  // slot: kBkNoSlot = no pair, or the pair is in its line buffer
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const uint64_t t = t0 + q * NT;
            const bool surv = (w[q] & m[q]) != 0u;
            const uint64_t mask = __ballot(surv);
            if (lane == 0 && t < nchunk) alive[t >> 6] = mask;  // t is 64-aligned for lane 0
            BloomSeq seq(h1[q], h2[q]);
            seq.advance(0);
#pragma unroll
            for (int j = 1; j < KMAX; ++j) {
                const int p = q * (KMAX - 1) + j - 1;
                slot[p] = kBkNoSlot;
                idx[p] = 0;
                if (surv && !(flags & 4) && (uint32_t)j < k) {
                    idx[p] = seq.index(mp);
                    const uint32_t b = idx[p] >> kBkBucketBits;
                    const uint32_t s = atomicAdd(&s_fill[b], 1u);
                    if (s < LE) bk_place(s_buf + b * LW, s, idx[p] & kBkOffMask, q0 + q * NT);
                    else slot[p] = s;
                    // fill was below a line at the tile's start: one entry per bucket and tile gets this slot
                    if (s == LE - 1) s_list[cur][atomicAdd(&s_nlist[cur], 1u)] = (uint16_t)b;
                }
                seq.advance(j);
            }
        }
        if (tile + G < ntiles) hash_tile(tile + G);  // the next tile (see above)
        __syncthreads();
        for (;;) {
            // store the listed buckets' full lines: eight lanes per bucket, a wave instruction stores
            // eight whole 64-byte lines; a bucket that still holds a full line goes on the next list
            const uint32_t nfull = s_nlist[cur];
            bool more = false;
            for (uint32_t i = threadIdx.x / LW; i < nfull; i += NT / LW) {
                const uint32_t b = s_list[cur][i];
                const uint32_t fill = s_fill[b], out = s_out[b];  // fill >= LE; out is a multiple of LE
                const unsigned long long e = s_buf[b * LW + lane8];
                const bool fits = (uint64_t)out + LE <= capS;
                if (fits) run_store(e, seg0 + b * capW + out / LE * LW + lane8);
                else bk_direct(s_buf + b * LW, b, lane8, LW, LE, G, bm, miss);
                if (lane8 == 0) {  // the eight lanes of a bucket are in one wave: their reads came first
                    s_fill[b] = fill - LE;
                    if (fits) s_out[b] = out + LE;
                    if (fill - LE >= LE) {
                        s_list[cur ^ 1][atomicAdd(&s_nlist[cur ^ 1], 1u)] = (uint16_t)b;
                        more = true;
                    }
                }
            }
            // (not read from s_nlist[cur ^ 1]: after the last round the next tile's pairs list there)
            const int again = __syncthreads_or(more);
            // the stored lines' slots are free: pending entries move down by one line
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (slot[p] != kBkNoSlot) {
                    slot[p] -= LE;
                    if (slot[p] < LE) {
                        bk_place(s_buf + (idx[p] >> kBkBucketBits) * LW, slot[p], idx[p] & kBkOffMask,
                                 q0 + (p / (KMAX - 1)) * NT);
                        slot[p] = kBkNoSlot;
                    }
                }
            }
            // this round's list is done (every thread read its length before the barrier above); it is
            // empty again before anything is listed on it: that is a round or a tile later, behind a barrier
            if (threadIdx.x == 0) s_nlist[cur] = 0;
            cur ^= 1;
            // no bucket holds a full line: every pending pair has just been placed (its slot was
            // below its bucket's fill), and the next tile's barrier orders these writes
            if (!again) break;
            __syncthreads();
        }
    }
    __syncthreads();
    // the block's partial lines and its nb segment counts.  A partial line is stored whole, all eight u64 (its
    // byte plane is at its end); the exact count says which of its entries are real, the rest is stale LDS
    for (uint32_t b = threadIdx.x / LW; b < nb; b += NT / LW) {
        const uint32_t fill = s_fill[b], out = s_out[b];  // fill < LE
        const bool fits = (uint64_t)out + LE <= capS;
        if (fill) {
            if (fits) run_store(s_buf[b * LW + lane8], seg0 + b * capW + out / LE * LW + lane8);
            else bk_direct(s_buf + b * LW, b, lane8, LW, fill, G, bm, miss);
        }
        if (lane8 == 0) segcnt[(uint64_t)b * G + blockIdx.x] = out + (fits ? fill : 0u);
    }
}

// K4 -----------------------------------------------------------------------------------
// A clear bit means the key is absent.  Its key id goes to an LDS record list (one LDS atomic);
// at the end of the region the list is bucketed by 2^19-key range and written as runs, one
// reservation per (slice, range), for K5 to turn into miss bits.  A scattered 64-bit
// atomicOr per clear bit (~21M per 1e8 C2 keys: keys that passed bit 0 by chance, ~5.5 clear
// bits each) cost one memory request each; the runs cost ~1 per 27 records.
// records per slice held in LDS (C2: ~5.1k per 128 KiB slice); beyond: direct atomicOr
constexpr uint32_t kBkMissBuf = 6400;

__device__ __forceinline__ void bk_miss_direct(uint32_t key, unsigned long long *miss) {
    atomicOr(&miss[key >> 6], 1ULL << (key & 63));
}

// One entry against the slice in LDS; entries of the region's other slice are skipped.  The test needs the
// entry's word alone; on a clear bit the key id is rebuilt from the word, the entry's high byte (bits sh .. sh + 7
// of hi4), the segment's stage-1 block and the stage-1 grid (bk_entry.h).
__device__ __forceinline__ void bk_test(const uint32_t *s_bm, uint32_t slice, uint32_t w, uint32_t hi4, uint32_t sh,
                                        uint32_t blk, uint32_t G, unsigned long long *miss, uint32_t *s_mrec,
                                        uint32_t *s_mn, uint32_t flags) {
    const uint32_t idx = bk_off(w);
    if (((idx >> kBkSliceBits) & (kBkCS - 1)) != slice) return;
    const uint32_t off = idx & ((1u << kBkSliceBits) - 1);
    if ((s_bm[off >> 5] & bit_in_word(off)) == 0u) {  // slices are word-aligned: off's low bits = idx's
        const uint32_t key = bk_key(bk_q_of(w, (hi4 >> sh) & 0xffu), blk, G);
        if (flags & 8) {
            miss[0] = 0;  // diagnostics: one fixed store instead of the miss
        } else if (flags & 16) {
            bk_miss_direct(key, miss);  // diagnostics: the direct atomic per clear bit (A/B)
        } else {
            const uint32_t slot = atomicAdd(s_mn, 1u);
            if (slot < kBkMissBuf) s_mrec[slot] = key;
            else bk_miss_direct(key, miss);
        }
    }
}

// Block bid: x = bid % 8, j = bid / 8; slice = j % 2, cluster = (j / 2) * 8 + x: 128 clusters in a
// grid of 256.  A cluster walks regions cluster, cluster + nclusters, ...  Wave v of a workgroup reads
// segments v, v + 16, ... of the region's <= 256 (16 per wave): a lane loads 16 B at a time,
// lane-linear over the segment, so four consecutive lanes hold one line: lanes 0-2 of the quad four
// entry words each, lane 3 the byte plane.  All four lanes test three entries: lanes 0-2 their first
// three words, with their high bytes from lane 3 (three quad-broadcast DPP moves); lane 3 the fourth
// word of lanes 0, 1 and 2 (three more), whose high bytes it holds.  The moves stand outside any branch.
// (Lanes 0-2 testing four words each left a quarter of the lanes of every LDS gather idle: 0.86 ms against
// 0.76; the parent's 8-byte pairs: 0.71.  The probe's time follows the tests a wave issues, not the bytes
// it loads: DESIGN.md 3.6 r09 has the variants.)  kBkProbeU loads per segment are in flight (16 lines
// each), and the next segment's loads are issued before the current one's entries are tested.  Plain loads,
// not nontemporal ones: the sibling workgroup needs the lines to stay in L2.
constexpr uint32_t kBkProbeU = 4;  // 768 entries (64 lines) per segment in one round (C2: ~620); 5 and 6 spill

// lane L of the caller's quad's value of v
template <int L> __device__ __forceinline__ uint32_t bk_quad(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, L * 0x55 /* quad_perm [L,L,L,L] */, 0xf, 0xf, true);
}

template <bool STAMP>
__global__ __launch_bounds__(1024) void k_bk_probe(const unsigned long long *__restrict__ pairs,
                                                   const uint32_t *__restrict__ segcnt, uint32_t G, uint64_t capS,
                                                   uint32_t nb, const uint32_t *__restrict__ bm, uint64_t nwords4,
                                                   unsigned long long *__restrict__ miss, uint32_t *__restrict__ mrec,
                                                   uint32_t *__restrict__ mcnt, uint64_t capm, uint32_t nmranges,
                                                   uint32_t flags, unsigned long long *__restrict__ stamps) {
    if (!kDiag) flags = 0;  // wrong-answer diagnostics exist in the profiling build only (rbx_kernels.h)
    PhaseStamps<STAMP, 4> ps;
    ps.start();
    __shared__ __attribute__((aligned(16))) uint32_t s_bm[kBkSliceWords];
    // the bucketed image of the miss records reuses the slice's LDS once its probes are done
    __shared__ uint32_t s_mrec[kBkMissBuf];
    uint32_t *s_mimg = s_bm;
    __shared__ uint32_t s_mc[256], s_mst[256], s_mpos[256], s_mgb[256], s_mn;
    constexpr uint32_t NT = 1024, NW = NT / 64, U = kBkProbeU;
    static_assert(kBkMaxGrid1 <= NW * 64, "a wave holds the counts of its segments one per lane");
    static_assert(kBkMissBuf <= kBkSliceWords, "the record image fits the slice's LDS");
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x % 8, j = blockIdx.x / 8;
    const uint32_t slice = j % kBkCS, cluster = (j / kBkCS) * 8 + x, nclusters = gridDim.x / kBkCS;
    const uint32_t nsw = wave < G ? (G - wave + NW - 1) / NW : 0u;  // this wave's segments: wave + NW * i
    for (uint32_t r = cluster; r < nb; r += nclusters) {
        if (threadIdx.x == 0) s_mn = 0;  // ordered before the probes by the barrier below
        // slice bitmap (nwords4 = bitmap words rounded up to 4; the allocation covers them); a
        // slice past the bitmap's end (the last region of a size that is no multiple) holds no pair
        const uint64_t w0 = (uint64_t)r * (kBkSliceWords * kBkCS) + (uint64_t)slice * kBkSliceWords;
        const uint32_t nv = w0 < nwords4 ? (uint32_t)min<uint64_t>(kBkSliceWords, nwords4 - w0) / 4 : 0u;
        const u32x4 *srcv = (const u32x4 *)(bm + w0);
        // the slice goes straight to LDS (global_load_lds, 16 B per lane, lane-linear): no VGPRs held for it
#pragma unroll
        for (uint32_t i = 0; i < kBkSliceWords / 4 / NT; ++i) {
            const uint32_t q = i * NT + threadIdx.x;
            if (q < nv)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcv + q),
                                                 (__attribute__((address_space(3))) void *)((u32x4 *)s_bm + i * NT + wave * 64),
                                                 16, 0, 0);
        }
        // lane i holds the count of this wave's i-th segment
        const uint32_t *rcnt = segcnt + (uint64_t)r * G;
        uint32_t cntv = 0;
        if (lane < nsw) cntv = (uint32_t)min<uint64_t>(rcnt[wave + NW * lane], capS);
        // capS is a multiple of 12 entries: a segment is whole 64-byte lines, four 16-byte loads each.  n
        // entries are ceil(n / 12) lines; the last one's tail past n is stale and is not tested
        auto seg = [&](uint32_t i) {
            return (const u32x4 *)(pairs + bk_seg_line(r, wave + NW * i, nb, capS) * kBkLineWords);
        };
        auto load = [&](u32x4 (&v)[U], const u32x4 *src, uint32_t n, uint32_t q0) {
            const uint32_t nq = (n + kBkLineEntries - 1) / kBkLineEntries * 4;
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t q = q0 + u * 64 + lane;
                if (q < nq) v[u] = src[q];
            }
        };
        auto test = [&](const u32x4 (&v)[U], uint32_t n, uint32_t q0, uint32_t blk) {
            const uint32_t sub = lane & 3;
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                // the quad's lane 3 holds the line's byte plane: .x entries 0-3, .y 4-7, .z 8-11
                const uint32_t h0 = bk_quad<3>(v[u].x), h1 = bk_quad<3>(v[u].y), h2 = bk_quad<3>(v[u].z);
                const uint32_t w3 = bk_quad<0>(v[u].w), w7 = bk_quad<1>(v[u].w), w11 = bk_quad<2>(v[u].w);
                const bool last = sub == 3;  // lane 3 tests entries 3, 7, 11; lane s < 3 entries 4s, 4s + 1, 4s + 2
                const uint32_t hi4 = sub == 0 ? h0 : sub == 1 ? h1 : h2;
                const uint32_t e0 = (q0 + u * 64 + lane) / 4 * kBkLineEntries + (last ? 3 : sub * 4), de = last ? 4 : 1;
                const uint32_t wa = last ? w3 : v[u].x, wb = last ? w7 : v[u].y, wc = last ? w11 : v[u].z;
                const uint32_t ha = last ? h0 : hi4, hb = last ? h1 : hi4, hc = last ? h2 : hi4;
                const uint32_t sa = last ? 24 : 0, sb = last ? 24 : 8, sc = last ? 24 : 16;
                if (e0 < n) {
                    bk_test(s_bm, slice, wa, ha, sa, blk, G, miss, s_mrec, &s_mn, flags);
                    if (e0 + de < n) bk_test(s_bm, slice, wb, hb, sb, blk, G, miss, s_mrec, &s_mn, flags);
                    if (e0 + 2 * de < n) bk_test(s_bm, slice, wc, hc, sc, blk, G, miss, s_mrec, &s_mn, flags);
                }
            }
        };
        u32x4 cur[U], nxt[U];
        uint32_t ncur = 0, nnxt = 0;
        if (nsw) {
            ncur = __builtin_amdgcn_readlane(cntv, 0);
            load(cur, seg(0), ncur, 0);
        }
        __syncthreads();  // waits for the bitmap DMA (and the first pair loads)
        ps.mark(0);
        for (uint32_t i = 0; i < nsw; ++i) {
            if (i + 1 < nsw) {
                nnxt = __builtin_amdgcn_readlane(cntv, i + 1);
                load(nxt, seg(i + 1), nnxt, 0);
            }
            test(cur, ncur, 0, wave + NW * i);
            for (uint32_t q0 = U * 64; q0 / 4 * kBkLineEntries < ncur; q0 += U * 64) {  // a segment longer than one round
                load(cur, seg(i), ncur, q0);
                test(cur, ncur, q0, wave + NW * i);
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) cur[u] = nxt[u];
            ncur = nnxt;
        }
        __syncthreads();
        ps.mark(1);
        const uint32_t nm = min(s_mn, kBkMissBuf);
        if (nm) {  // uniform: bucket the slice's miss records by key range
            if (threadIdx.x < 256) s_mc[threadIdx.x] = 0;
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < nm; i += NT) atomicAdd(&s_mc[s_mrec[i] >> kBkMissRangeBits], 1u);
            __syncthreads();
            if (threadIdx.x < 64) bk_scan<4>(s_mc, nmranges, s_mst, s_mpos);
            else if (threadIdx.x >= 256 && threadIdx.x - 256 < nmranges) {
                const uint32_t q = threadIdx.x - 256;
                s_mgb[q] = s_mc[q] ? atomicAdd(&mcnt[q], s_mc[q]) : 0u;
            }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < nm; i += NT) {
                const uint32_t key = s_mrec[i];
                s_mimg[atomicAdd(&s_mpos[key >> kBkMissRangeBits], 1u)] = key;
            }
            __syncthreads();
            for (uint32_t q = wave; q < nmranges; q += NT / 64) {
                const uint32_t cq = s_mc[q], st = s_mst[q];
                const uint64_t gb = s_mgb[q];
                for (uint32_t t = lane; t < cq; t += 64) {
                    const uint32_t key = s_mimg[st + t];
                    if (gb + t < capm) run_store(key, mrec + (uint64_t)q * capm + gb + t);
                    else bk_miss_direct(key, miss);
                }
            }
        }
        __syncthreads();  // s_bm / s_mrec / s_mn reuse
        ps.mark(2);
    }
    ps.flush(stamps);
}

// K5 -----------------------------------------------------------------------------------
// Miss records -> miss bits.  Item = (key range q, slice of kBkMissSlice records): the slice's
// key ids set bits of a 64 KiB LDS image of the range's miss words, whose nonzero words are
// OR-ed into `miss` (consecutive words: one 64-B atomic request per 16 words).  Many small
// items, not one block per range: one block walking a range's ~1e5 records was latency-bound
// at ~0.5e9 records/s (0.23 ms at C2).
constexpr uint32_t kBkMissSlice = 32768;

__global__ __launch_bounds__(1024) void k_bk_misses(const uint32_t *__restrict__ mrec,
                                                    const uint32_t *__restrict__ mcnt, uint64_t capm,
                                                    uint32_t nmranges, unsigned long long *__restrict__ miss) {
    constexpr uint32_t NT = 1024, W = 1u << (kBkMissRangeBits - 5), PER = kBkMissSlice / NT;
    constexpr uint32_t KM = (1u << kBkMissRangeBits) - 1;
    __shared__ uint32_t s_m[W];  // 64 KiB
    const uint32_t nslices = (uint32_t)((capm + kBkMissSlice - 1) / kBkMissSlice);
    for (uint32_t item = blockIdx.x; item < nmranges * nslices; item += gridDim.x) {
        const uint32_t q = item % nmranges, sl = item / nmranges;
        const uint64_t n = min<uint64_t>(mcnt[q], capm), start = (uint64_t)sl * kBkMissSlice;
        if (start >= n) continue;  // uniform
        const uint32_t m = (uint32_t)min<uint64_t>(kBkMissSlice, n - start);
        const uint32_t *src = mrec + (uint64_t)q * capm + start;
        uint32_t kk[PER];
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) {
            const uint32_t i = u * NT + threadIdx.x;
            kk[u] = i < m ? __builtin_nontemporal_load(src + i) : 0xffffffffu;
        }
        for (uint32_t w = threadIdx.x; w < W; w += NT) s_m[w] = 0u;
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u)
            if (kk[u] != 0xffffffffu) atomicOr(&s_m[(kk[u] & KM) >> 5], 1u << (kk[u] & 31));
        __syncthreads();
        uint32_t *dst = (uint32_t *)miss + ((uint64_t)q << (kBkMissRangeBits - 5));  // u64 words as LE u32 pairs
        for (uint32_t w = threadIdx.x; w < W; w += NT) {
            const uint32_t v = s_m[w];
            if (v) atomicOr(&dst[w], v);
        }
        __syncthreads();  // s_m reuse
    }
}

// K6 -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bk_final(const unsigned long long *__restrict__ alive,
                                                  const unsigned long long *__restrict__ miss, uint64_t nchunk,
                                                  uint64_t base, uint8_t *__restrict__ out,
                                                  unsigned long long *__restrict__ count) {
    __shared__ unsigned long long s_part[4];
    unsigned long long c = 0;
    const uint64_t ngroups = (nchunk + 63) >> 6;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long pres = alive[g] & ~miss[g];
        const uint64_t rem = nchunk - (g << 6);
        if (rem < 64) pres &= (1ULL << rem) - 1;
        c += __popcll(pres);
    }
    if (out) {  // one byte per key, coalesced
        for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nchunk; t += (uint64_t)gridDim.x * blockDim.x)
            out[base + t] = (uint8_t)(((alive[t >> 6] & ~miss[t >> 6]) >> (t & 63)) & 1ULL);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (t && count) atomicAdd(count, t);
    }
}

// k_bk_final's blocks: each adds its count to ONE counter, and same-address atomics serialise at the
// kernel's end, so 512 blocks (grid-stride) rather than 2048 (r05, cf. k_stream_final8)
static unsigned grid_for_pc(uint64_t n) {
    uint64_t g = ((n + 63) / 64 + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 512 ? 512 : g));
}

// launcher -------------------------------------------------------------------------------
// Shapes: stage 1 at 1024 threads with one key per thread (1024-key tiles, kBkTileKeys), 152 KiB
// of LDS, one block per CU; the probe at 1024 threads, one workgroup per CU (a 128 KiB slice + the
// miss buffers), in whole groups of 8 clusters.  The A/Bs (region size, tile size, segment layout)
// are in DESIGN.md §3.6 r07 and r08, the entry format's in r09.
template <int KLEN, int KMAX>
static void bk_chunk(const PcArgs &a, hipStream_t st) {
    static_assert(kBkTileKeys == 1024, "the stage-1 tile is the block: one key per thread");
    hipLaunchKernelGGL((k_bk_stage1<KLEN, KMAX, 1024, 1>), dim3(a.grid1), dim3(1024), 0, st, a.keys, a.base,
                       a.nchunk, a.bm, a.mp, a.k, a.nb, a.capS, a.pairs, a.segcnt, a.alive, a.miss, a.flags);
    constexpr uint32_t kGroup = 8 * kBkCS, kMaxProbe = 256;
    const uint32_t gp = std::max(kGroup, std::min(a.nb * kBkCS, kMaxProbe) / kGroup * kGroup);
    if (kDiag && a.stamps)
        hipLaunchKernelGGL((k_bk_probe<true>), dim3(gp), dim3(1024), 0, st, a.pairs, a.segcnt, a.grid1, a.capS, a.nb,
                           a.bm, a.nwords4, a.miss, a.mrec, a.mcnt, a.capm, a.nmranges, a.flags, a.stamps + 8);
    else
        hipLaunchKernelGGL((k_bk_probe<false>), dim3(gp), dim3(1024), 0, st, a.pairs, a.segcnt, a.grid1, a.capS, a.nb,
                           a.bm, a.nwords4, a.miss, a.mrec, a.mcnt, a.capm, a.nmranges, a.flags, nullptr);
    hipLaunchKernelGGL(k_bk_misses, dim3(2048), dim3(1024), 0, st, a.mrec, a.mcnt, a.capm, a.nmranges, a.miss);
    hipLaunchKernelGGL(k_bk_final, dim3(grid_for_pc(a.nchunk)), dim3(256), 0, st, a.alive, a.miss, a.nchunk, a.base,
                       a.out, a.count);
}

void launch_contains_partitioned_chunk(const PcArgs &a, int klen_fast, hipStream_t st) {
    with_klen(klen_fast, [&](auto klen) {
        with_kmax<16, 16>(a.k, [&](auto kmax) { bk_chunk<decltype(klen)::value, decltype(kmax)::value>(a, st); });
    });
}

}  // namespace rbx
