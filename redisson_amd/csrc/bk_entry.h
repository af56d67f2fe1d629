// bk_entry.h -- the partitioned contains' (contains_partitioned.hip) entry format and the geometry
// rules that make it fit: what stage 1 writes into a segment, what the probe reads back, and how the host sizes
// chunks and segments.  No HIP, no context: the kernels and api_bloom.cpp share it, and tests/c/bk_entry_test.cpp
// runs it alone under sanitizers.  (The constexpr functions are host and device code under hipcc.)
//
// An entry is one (bit index, key) pair in 40 bits.  The bit index is an offset inside its 2^21-bit region: the
// region is the bucket, so the segment says the rest.  The key is block-local: segment (b, blk) is written by
// stage-1 block blk alone, which hashes the 1024-key tiles blk, blk + G, blk + 2G, ... of its chunk (G blocks), so
// inside that segment a key is q = i * 1024 + tid (tile iteration i, thread tid), and the chunk-local key id comes
// back from (q, blk, G).  A chunk holds at most G * 2^19 keys, so i < 512 and q < 2^19: 21 + 19 = 40 bits.
//
// A 64-byte line holds twelve entries: twelve u32 words `off | (q & 0x7ff) << 21` (bytes 0-47), then twelve bytes
// `q >> 11` (bytes 48-59), then four unused bytes.  Entry s of a line is word s and byte 48 + s.  The probe's bit
// test needs the word alone; the byte is read only to name the key of a clear bit.
#pragma once
#include <cmath>
#include <cstdint>

namespace rbx {

constexpr uint32_t kBkBucketBits = 21;    // bits per region (bucket): an entry's offset
constexpr uint32_t kBkTileBits = 10;
constexpr uint32_t kBkTileKeys = 1u << kBkTileBits;  // keys per stage-1 tile: 1024 threads, one key each
constexpr uint32_t kBkMaxGrid1 = 256;     // stage-1 blocks (persistent), one per CU
constexpr uint32_t kBkQBits = 19;         // block-local key index q
constexpr uint32_t kBkChunkBits = 27;     // keys per chunk at the full grid
constexpr uint32_t kBkLineEntries = 12;   // entries per 64-byte line
constexpr uint32_t kBkLineWords = 8;      // u64 per 64-byte line: what a flush copies, one per lane
constexpr uint32_t kBkLineBytes = 64;
constexpr uint32_t kBkLineHiByte = 4 * kBkLineEntries;  // the byte plane's offset in the line
constexpr uint32_t kBkQLowBits = 32 - kBkBucketBits;    // q's bits in the word; the rest is the byte
constexpr uint32_t kBkOffMask = (1u << kBkBucketBits) - 1;

static_assert(kBkBucketBits + 19 == 40, "an entry is five bytes");
static_assert(kBkBucketBits + kBkQBits == 40 && kBkQBits - kBkQLowBits <= 8, "q's high part fits the byte");
static_assert(((1u << 27) / kBkTileKeys / kBkMaxGrid1) * kBkTileKeys <= (1u << 19),
              "a block's share of a full chunk fits q");
static_assert(kBkLineHiByte + kBkLineEntries <= kBkLineBytes && kBkLineWords * 8 == kBkLineBytes, "the line");

// the block-local index of the key thread tid hashes in its block's i-th tile
constexpr uint32_t bk_q(uint32_t i, uint32_t tid) { return i * kBkTileKeys + tid; }
// the chunk-local key id of q in block blk of G: tile blk + G * i, thread q % 1024
constexpr uint32_t bk_key(uint32_t q, uint32_t blk, uint32_t G) {
    return (((q >> kBkTileBits) * G + blk) << kBkTileBits) | (q & (kBkTileKeys - 1));
}
constexpr uint32_t bk_word(uint32_t off, uint32_t q) { return off | ((q & ((1u << kBkQLowBits) - 1)) << kBkBucketBits); }
constexpr uint8_t bk_hi(uint32_t q) { return (uint8_t)(q >> kBkQLowBits); }
constexpr uint32_t bk_off(uint32_t word) { return word & kBkOffMask; }
constexpr uint32_t bk_q_of(uint32_t word, uint32_t hi) { return (word >> kBkBucketBits) | (hi << kBkQLowBits); }

// Chunk rule.  Keys per chunk of a batch of n keys at a stage-1 grid of at most `grid` blocks (1..kBkMaxGrid1) and
// k hash iterations (2..16): at most grid * 2^19 (q), 2^27 (the key ids of the miss records and the final pass)
// and 2^30 / (k - 1) (a chunk's entries); the batch's chunks are balanced and whole tiles.  Every bound is a whole
// number of tiles after the rounding down, so rounding the balanced chunk up to a tile stays inside them.
constexpr uint64_t bk_chunk_keys(uint64_t n, uint32_t grid, uint32_t k) {
    uint64_t cap = (uint64_t)grid << kBkQBits;
    if (cap > (1ULL << kBkChunkBits)) cap = 1ULL << kBkChunkBits;
    const uint64_t byk = (1ULL << 30) / (k - 1) / kBkTileKeys * kBkTileKeys;
    if (cap > byk) cap = byk;
    const uint64_t nch = (n + cap - 1) / cap;
    const uint64_t chunk = nch ? (n + nch - 1) / nch : 0;
    return (chunk + kBkTileKeys - 1) / kBkTileKeys * kBkTileKeys;
}
// the stage-1 grid of a chunk of nchunk keys, and the tiles its busiest block runs (q < this * 1024)
constexpr uint32_t bk_grid(uint64_t nchunk, uint32_t grid) {
    const uint64_t tiles = (nchunk + kBkTileKeys - 1) / kBkTileKeys;
    return (uint32_t)(tiles < grid ? tiles : grid);
}
constexpr uint64_t bk_block_tiles(uint64_t nchunk, uint32_t G) {
    return G ? ((nchunk + kBkTileKeys - 1) / kBkTileKeys + G - 1) / G : 0;
}

// Segment capacity in entries, a whole number of lines.  Stage-1 block blk owns one segment per region.  With
// every key surviving stage 1 and the entries spread uniformly over [0, size), a segment's fill is Poisson with mean
//   lambda = (keys per block) * (k - 1) * min(1, 2^21 / size).
// Chernoff: P(X >= lambda + x) <= exp(-x^2 / (2 (lambda + x/3))); x = 7 sqrt(lambda) + 24 keeps that below 1e-9
// per segment for every lambda, i.e. below 1e-3 over the <= 2^19 segments of a chunk.  An entry past the capacity
// is probed directly (bk_direct): capacity never changes answers.
inline uint64_t bk_seg_cap(uint64_t chunk, uint32_t G, uint32_t k, uint64_t size) {
    const double region = (double)(1ULL << kBkBucketBits);
    const double lambda = (double)(bk_block_tiles(chunk, G) * kBkTileKeys) * (k - 1) *
                          (size > (1ULL << kBkBucketBits) ? region / (double)size : 1.0);
    const uint64_t cap = (uint64_t)(lambda + 7.0 * std::sqrt(lambda) + 24.0);
    return (cap + kBkLineEntries - 1) / kBkLineEntries * kBkLineEntries;
}
// segment (bucket b, block blk) of nb buckets starts at this line of the scratch; a segment is capS / 12 lines
constexpr uint64_t bk_seg_line(uint32_t b, uint32_t blk, uint32_t nb, uint64_t capS) {
    return ((uint64_t)blk * nb + b) * (capS / kBkLineEntries);
}

}  // namespace rbx
