// bk_entry_test.cpp -- the partitioned contains' 5-byte entry format and geometry rules (redisson_amd/csrc/
// bk_entry.h) at their corners, built with -fsanitize=address,undefined (tests/test_bk_entry_sanitized.py): entries
// are packed into and read back from an exactly sized 64-byte heap line, so a slot or a byte past it is an ASan
// report and a shift past a field's width a UBSan one.  No HIP.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../redisson_amd/csrc/bk_entry.h"

using namespace rbx;

static long cases = 0;
static int failures = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++cases;                                          \
        if (!(cond)) {                                    \
            ++failures;                                   \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

// what stage 1's placement and the probe's decode do, on a line of its own
static void put(uint8_t *line, uint32_t s, uint32_t off, uint32_t q) {
    const uint32_t w = bk_word(off, q);
    memcpy(line + 4 * s, &w, 4);
    line[kBkLineHiByte + s] = bk_hi(q);
}
static void get(const uint8_t *line, uint32_t s, uint32_t *off, uint32_t *q) {
    uint32_t w;
    memcpy(&w, line + 4 * s, 4);
    *off = bk_off(w);
    *q = bk_q_of(w, line[kBkLineHiByte + s]);
}

static void round_trips() {
    const uint32_t offs[] = {0, (1u << kBkBucketBits) - 1}, tids[] = {0, kBkTileKeys - 1};
    const uint32_t its[] = {0, 1, 2, 255, 256, 511}, grids[] = {1, 2, 255, 256};
    for (uint32_t G : grids)
        for (uint32_t blk : {0u, G - 1})
            for (uint32_t i : its)
                for (uint32_t tid : tids)
                    for (uint32_t off : offs)
                        for (uint32_t s = 0; s < kBkLineEntries; ++s) {
                            std::unique_ptr<uint8_t[]> line(new uint8_t[kBkLineBytes]);
                            memset(line.get(), 0xA5, kBkLineBytes);  // stale neighbours
                            const uint32_t q = bk_q(i, tid);
                            CHECK(q < (1u << kBkQBits), "q %u", q);
                            put(line.get(), s, off, q);
                            uint32_t off2, q2;
                            get(line.get(), s, &off2, &q2);
                            CHECK(off2 == off && q2 == q, "G %u blk %u i %u tid %u off %u slot %u: got off %u q %u", G, blk,
                                  i, tid, off, s, off2, q2);
                            // the neighbours and the four unused bytes are untouched
                            for (uint32_t t = 0; t < kBkLineBytes; ++t) {
                                const bool mine = (t >= 4 * s && t < 4 * s + 4) || t == kBkLineHiByte + s;
                                if (!mine) CHECK(line[t] == 0xA5, "slot %u wrote byte %u", s, t);
                            }
                            // the key the probe rebuilds against the plain tile * 1024 + tid
                            const uint64_t tile = blk + (uint64_t)G * i;
                            CHECK(bk_key(q2, blk, G) == tile * kBkTileKeys + tid, "key: G %u blk %u i %u tid %u: %u", G, blk,
                                  i, tid, bk_key(q2, blk, G));
                        }
}

// no chunk at any grid and k yields q >= 2^19, a key id >= 2^27 or more than 2^30 entries
static void chunk_rule() {
    for (uint32_t grid = 1; grid <= kBkMaxGrid1; ++grid)
        for (uint32_t k = 2; k <= 16; ++k) {
            const uint64_t full = (uint64_t)grid << kBkQBits;
            const uint64_t ns[] = {1, kBkTileKeys, kBkTileKeys + 1, full - 1, full, full + 1, full + kBkTileKeys,
                                   3 * full + 7, 100000000ULL, (1ULL << 27) + 1, (1ULL << 30) / (k - 1) + 1, 1ULL << 32};
            for (uint64_t n : ns) {
                const uint64_t chunk = bk_chunk_keys(n, grid, k);
                CHECK(chunk > 0 && chunk % kBkTileKeys == 0, "grid %u k %u n %llu chunk %llu", grid, k,
                      (unsigned long long)n, (unsigned long long)chunk);
                CHECK(chunk <= full && chunk <= (1ULL << 27) && chunk * (k - 1) <= (1ULL << 30),
                      "grid %u k %u n %llu chunk %llu", grid, k, (unsigned long long)n, (unsigned long long)chunk);
                // the full chunks and the last one (the launcher's nchunk)
                const uint64_t last = n % chunk ? n % chunk : chunk;
                for (uint64_t nchunk : {chunk < n ? chunk : n, last}) {
                    const uint32_t G = bk_grid(nchunk, grid);
                    CHECK(G >= 1 && G <= grid, "G %u", G);
                    const uint64_t its = bk_block_tiles(nchunk, G);
                    CHECK(its >= 1 && its <= 512, "grid %u k %u n %llu nchunk %llu: %llu tiles per block", grid, k,
                          (unsigned long long)n, (unsigned long long)nchunk, (unsigned long long)its);
                    const uint32_t qmax = bk_q((uint32_t)its - 1, kBkTileKeys - 1);
                    CHECK(qmax < (1u << kBkQBits), "q %u", qmax);
                    // the last key of the chunk, as the block that hashes it names it
                    const uint64_t t = nchunk - 1, tile = t / kBkTileKeys;
                    const uint32_t blk = (uint32_t)(tile % G), i = (uint32_t)(tile / G);
                    CHECK(bk_key(bk_q(i, (uint32_t)(t % kBkTileKeys)), blk, G) == t, "last key of %llu at G %u",
                          (unsigned long long)nchunk, G);
                }
            }
        }
}

// capS is whole lines and holds the mean; segments tile the scratch in whole 64-byte lines
static void capacity() {
    const uint64_t sizes[] = {1ULL << 21, (1ULL << 21) + 1, 1ULL << 27, (1ULL << 32) - 3};
    for (uint64_t size : sizes)
        for (uint32_t k : {2u, 7u, 16u})
            for (uint32_t grid : {1u, 2u, 255u, 256u})
                for (uint64_t n : {1ULL, 1025ULL, 200000ULL, 100000000ULL}) {
                    const uint64_t chunk = bk_chunk_keys(n, grid, k);
                    const uint32_t G = bk_grid(chunk, grid);
                    const uint32_t nb = (uint32_t)((size + (1ULL << kBkBucketBits) - 1) >> kBkBucketBits);
                    const uint64_t capS = bk_seg_cap(chunk, G, k, size);
                    CHECK(capS % kBkLineEntries == 0 && capS >= kBkLineEntries, "capS %llu", (unsigned long long)capS);
                    const double share = size > (1ULL << kBkBucketBits) ? (double)(1ULL << kBkBucketBits) / (double)size : 1.0;
                    const double lambda = (double)(bk_block_tiles(chunk, G) * kBkTileKeys) * (k - 1) * share;
                    CHECK((double)capS >= lambda + 24.0, "capS %llu below lambda %f", (unsigned long long)capS, lambda);
                    for (uint32_t blk : {0u, G - 1})
                        for (uint32_t b : {0u, nb - 1}) {
                            const uint64_t byte = bk_seg_line(b, blk, nb, capS) * kBkLineBytes;
                            CHECK(byte % 64 == 0, "segment (%u, %u) at byte %llu", b, blk, (unsigned long long)byte);
                            CHECK(byte == (((uint64_t)blk * nb + b) * capS / kBkLineEntries) * 64, "segment (%u, %u)", b, blk);
                            // the next segment (the next bucket, or the next block's first) starts where this one ends
                            const uint64_t next = b + 1 < nb ? bk_seg_line(b + 1, blk, nb, capS) : bk_seg_line(0, blk + 1, nb, capS);
                            CHECK(next * kBkLineBytes == byte + capS / kBkLineEntries * kBkLineBytes, "segment (%u, %u) length", b, blk);
                        }
                    // the last segment ends where the reservation does
                    CHECK(bk_seg_line(nb - 1, G - 1, nb, capS) + capS / kBkLineEntries == bk_seg_line(0, G, nb, capS),
                          "reservation");
                }
}

int main() {
    round_trips();
    chunk_rule();
    capacity();
    if (failures) {
        printf("bk_entry_test: %d of %ld checks failed\n", failures, cases);
        return 1;
    }
    printf("bk_entry_test: ok (%ld checks)\n", cases);
    return 0;
}
