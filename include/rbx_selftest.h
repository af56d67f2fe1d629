/*
 * rbx_selftest.h -- test-only exports of librbx.so: the device primitives compiled
 * for the host, so CPU tests can check them without a GPU (tests/test_abi.py).
 */
#ifndef RBX_SELFTEST_H
#define RBX_SELFTEST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* mismatches of the divide-free 63-bit modulo against '%' over n random (h, size) pairs x16 */
uint64_t rbx_selftest_mod(uint64_t n, uint64_t seed);
/* HighwayHash128 (Redisson KEY) through the host-compiled device code path */
void rbx_selftest_hash128(const uint8_t *data, uint64_t len, uint64_t out[2]);
/* out[0..k) = the Bloom indexes of RedissonBloomFilter.hash(h1, h2, k, size), 1 <= size <= 2^32, from the
 * host-compiled index cursor; returns how many of them its compact-modulus form computes differently (0) */
uint32_t rbx_selftest_bloom_indexes(uint64_t h1, uint64_t h2, uint32_t k, uint64_t size, uint32_t *out);
/* BigDecimal.valueOf(d).toPlainString() (the stored falseProbability string); returns length */
int rbx_selftest_plain_string(double d, char *out, int cap);
/* device and pinned buffers the contexts of this process hold: rbx_shutdown returns it to its earlier value */
int64_t rbx_selftest_live_buffers(void);
#ifdef __cplusplus
}
#endif
#endif
