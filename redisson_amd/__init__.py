"""redisson_amd -- MI355X-native batched sketch engine for Redisson's probabilistic
structures (RBloomFilter / RHyperLogLog), behind a C ABI (include/rbx.h, librbx.so).

Host mirror of the reference API: RedissonClient.getBloomFilter / getHyperLogLog / getBitSet / getBinaryStream / createBatch.
"""
from .client import (BatchResult, BloomHandle, RBatch, RBinaryStream, RBitSet, RBloomFilter, RedissonClient, RHyperLogLog,
                     string_stream, string_stream_call, string_stream_dev,
                     bitset_op_groups_call, bitset_range_stream, bitset_range_stream_call, bitset_range_stream_dev,
                     bitset_field_stream, bitset_field_stream_dev, bitset_stream, bitset_stream_dev, bloom_add_multi, bloom_stream, bloom_contains_multi, calc_slot,
                     crc16, hll_add_multi, hll_count_each, hll_count_groups, hll_count_groups_call, hll_merge_groups,
                     hll_merge_groups_call, hll_stream, hll_stream_call, hll_stream_dev, slot_to_gpu,
                     bitset_members_stream, bitset_members_stream_call, bitset_members_stream_dev)
from .codec import ByteArrayCodec, StringCodec
from .exceptions import (ArithmeticException, DeviceError, IllegalArgumentException, IllegalStateException,
                         RedisException, UnsupportedOperationException)
from .keys import Arena, device_keys

Redisson = RedissonClient

__all__ = [
    "Arena", "ArithmeticException", "BatchResult", "BloomHandle", "bloom_stream", "ByteArrayCodec", "DeviceError",
    "IllegalArgumentException", "IllegalStateException", "RBatch", "RBitSet", "RBloomFilter", "RHyperLogLog",
    "RedisException", "Redisson", "RedissonClient", "StringCodec", "UnsupportedOperationException",
    "bitset_field_stream", "bitset_field_stream_dev", "bitset_stream", "bitset_stream_dev", "bloom_add_multi", "bloom_contains_multi", "calc_slot", "crc16", "device_keys",
    "hll_add_multi", "hll_count_each", "hll_count_groups", "hll_count_groups_call", "hll_merge_groups",
    "hll_merge_groups_call", "bitset_op_groups_call", "bitset_range_stream", "bitset_range_stream_call",
    "bitset_range_stream_dev", "bitset_members_stream", "bitset_members_stream_call", "bitset_members_stream_dev",
    "hll_stream", "hll_stream_call", "hll_stream_dev", "slot_to_gpu", "RBinaryStream", "string_stream",
    "string_stream_call", "string_stream_dev",
]
