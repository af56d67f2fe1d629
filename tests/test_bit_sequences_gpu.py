"""Random mixed command sequences on shared bit strings, on the GPU (bitstring_driver.py): SETBIT, index batches,
range fills, BITOP, BITFIELD in every form, ranged BITCOUNT / BITPOS, SET / DEL / RENAME / PEXPIRE and the Bloom
commands take turns on the same five keys, and every reply, error and -- every 25 commands -- every key's bytes and
what lies behind them equal the keyspace model of bitstring_model.py.  What the sequences are there to check is the
contract between the families: the zero tail, the length word, growth and the keyspace
generation, BITOP onto one of its sources, and the path choices on strings that other families have written.

A failure names its seed and step; bitstring_driver.run(engine, seed, STEPS, stop_at=step + 1) replays it."""
import contextlib

import numpy as np
import pytest

import bitstring_driver as D
from redisson_amd import _lib as L
from test_bit_sequences_cpu import SEEDS, STEPS

pytestmark = pytest.mark.gpu

DEFAULTS = {"bitrange_dir": 2, "bitrange_pos_chunk": 256 << 10, "bitrange_chain_max": 128 << 10,
            "bitfield_sat_atomic": 1, "contains_partition": 2, "add_partition": 2, "add_single_seg_keys": 256}
# The knobs each seed runs under; a knob that is not named keeps its default.
#   seed  bitrange_dir  bitrange_pos_chunk  bitrange_chain_max  bitfield_sat_atomic  contains_partition  add_partition  add_single_seg_keys
#   0     2 (default)   256 KiB (default)   128 KiB (default)   1 (default)          2 (default)         2 (default)    256 (default)
#   1     0             4096                default             0                    0                   0              0
#   2     1             4096                64                  1                    1                   1              256
#   3     2             4096                64                  0                    1                   0              256
#   4     0             default             64                  1                    0                   1              0
#   5     1             default             default             0                    1                   1              0
#   6     2             default             64                  1                    0                   0              256
#   7     1             4096                default             0                    0                   1              256
# add_partition = 1 reaches the partitioned add only on the 70,001-bit key (it refuses sizes below 2^15 bits, so never
# on the 3,001-bit one) and only for batches past add_single_seg_keys: n = 257 or 1000 with 256 (seeds 2 and 7), n >= 2
# with 0 (seeds 4 and 5).  contains_partition = 1 has no such floor: it takes the contains batches on both keys.
SETTINGS = {
    0: {},
    1: dict(bitrange_dir=0, bitrange_pos_chunk=4096, bitfield_sat_atomic=0, contains_partition=0, add_partition=0,
            add_single_seg_keys=0),
    2: dict(bitrange_dir=1, bitrange_pos_chunk=4096, bitrange_chain_max=64, bitfield_sat_atomic=1, contains_partition=1,
            add_partition=1, add_single_seg_keys=256),
    3: dict(bitrange_dir=2, bitrange_pos_chunk=4096, bitrange_chain_max=64, bitfield_sat_atomic=0, contains_partition=1,
            add_partition=0, add_single_seg_keys=256),
    4: dict(bitrange_dir=0, bitrange_chain_max=64, bitfield_sat_atomic=1, contains_partition=0, add_partition=1,
            add_single_seg_keys=0),
    5: dict(bitrange_dir=1, bitfield_sat_atomic=0, contains_partition=1, add_partition=1, add_single_seg_keys=0),
    6: dict(bitrange_dir=2, bitrange_chain_max=64, bitfield_sat_atomic=1, contains_partition=0, add_partition=0,
            add_single_seg_keys=256),
    7: dict(bitrange_dir=1, bitrange_pos_chunk=4096, bitfield_sat_atomic=0, contains_partition=0, add_partition=1,
            add_single_seg_keys=256),
}


@contextlib.contextmanager
def tuned(knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            L.lib().rbx_tune(k.encode(), v)


def test_the_settings_cover_every_knob_value():
    def seen(knob):
        return {SETTINGS[s].get(knob, DEFAULTS[knob]) for s in SEEDS}

    assert set(SETTINGS) == set(SEEDS)
    assert seen("bitrange_dir") == {0, 1, 2}
    assert 4096 in seen("bitrange_pos_chunk")
    assert seen("bitrange_chain_max") == {64, DEFAULTS["bitrange_chain_max"]}
    assert seen("bitfield_sat_atomic") == {0, 1}
    assert seen("contains_partition") >= {0, 1} and seen("add_partition") >= {0, 1}
    assert seen("add_single_seg_keys") == {0, 256}


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_equals_the_model(client, fresh, seed):
    engine = D.GpuEngine(client, fresh + ":")
    try:
        with tuned(SETTINGS[seed]):
            D.run(engine, seed, STEPS)
    finally:
        engine.close()


def test_a_recycled_slab_reads_zero(client, fresh):
    """new_bitmap on a recycled slab: 200 short keys of four sizes are filled with ones and deleted, and 200 keys made
    by one SETBIT of value 0 at their last bit take the freed slabs -- freed allocations are reused by exact size, the
    most recently freed first, and no new key is deleted before all are checked, so each takes a slab of its own.
    Two sizes share each allocation size, and a new key never has the length of the string its slab held: 1 byte
    comes onto 255 bytes of ones and 255 onto 1 (256-byte allocations), 1,793 onto 2,000 and 2,000 onto 1,793
    (2,048-byte ones).  A fill that misses bytes behind the shorter new string, the rest of the allocation, or the
    length word kept behind it would show: every byte reads zero, up to the allocation's end, and the length is the
    new one."""
    made = []
    try:
        for round_, (old_sizes, new_sizes) in enumerate((((255, 2000), (1, 1793)), ((1, 1793), (255, 2000)))):
            olds = [(client.getBitSet(f"{fresh}:old{round_}:{i}"), old_sizes[i % 2]) for i in range(100)]
            for bs, n in olds:
                bs.setRange(0, 8 * n)
                made.append(bs)
            assert all(bs.cardinality() == 8 * n for bs, n in olds[:4])
            for bs, _n in olds:
                assert bs.delete()
            for i in range(100):
                bs, n = client.getBitSet(f"{fresh}:new{round_}:{i}"), new_sizes[i % 2]
                made.append(bs)
                cap = (n + 255) // 256 * 256
                assert bs.set(8 * n - 1, False) is False
                assert bs.size() == 8 * n and bs.toByteArray() == bytes(n), (round_, i)
                assert bs.cardinality() == 0 and not bs.getIndexes(np.arange(8 * n, 8 * cap)).any(), (round_, i)
    finally:
        for bs in made:
            bs.delete()
