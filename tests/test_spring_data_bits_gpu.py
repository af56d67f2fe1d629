"""Spring Data RedissonConnection's bit commands (getBit / setBit / bitCount / bitOp / strLen / bitPos) over the
engine, against the models of bitset_model.py and bitrange_model.py."""
import numpy as np
import pytest

import bitrange_model as M
from bitset_model import RedisString, bitop
from redisson_amd import IllegalArgumentException, RedisException, UnsupportedOperationException
from redisson_amd.spring_data import RedissonConnection

pytestmark = pytest.mark.gpu


def test_bit_commands_on_one_key(client, fresh):
    conn = RedissonConnection(client)
    key = fresh.encode() + b"\x00k"  # byte[] keys may hold any byte
    model = RedisString()
    assert conn.strLen(key) == 0 and conn.bitCount(key) == 0 and conn.bitPos(key, True) == -1 and conn.bitPos(key, False) == 0
    rng = np.random.default_rng(21)
    for i in rng.integers(0, 700, 300).tolist():
        value = bool(i % 3)
        assert conn.setBit(key, i, value) == bool(model.setbit(i, value)), i  # the old bit
    assert conn.setBit(key, 5, True) == bool(model.setbit(5, True))
    assert conn.setBit(key, 5, True) is True and model.setbit(5, True) == 1
    assert conn.setBit(key, 5, False) is True and model.setbit(5, False) == 1
    data = model.bytes()
    n = len(data)
    assert conn.strLen(key) == n == model.strlen()
    assert [conn.getBit(key, i) for i in range(0, 720, 7)] == [bool(model.getbit(i)) for i in range(0, 720, 7)]
    assert conn.bitCount(key) == model.bitcount() == M.bitcount(data, 0, -1)
    for begin, end in [(0, -1), (0, 0), (1, 1), (3, 40), (-5, -2), (-2, -5), (-10, -20), (n - 1, n + 7), (n, n + 1),
                       (-n - 3, 2), (50, 10)]:
        assert conn.bitCount(key, begin, end) == M.bitcount(data, begin, end), (begin, end)
    for bit in (True, False):
        assert conn.bitPos(key, bit) == conn.bitPos(key, bit, (None, None)) == M.bitpos(data, int(bit))
        for lower in (0, 1, 17, n - 1, n, -1, -3, -n - 2):
            assert conn.bitPos(key, bit, (lower, None)) == M.bitpos(data, int(bit), lower), (bit, lower)
            for upper in (0, lower, 40, -1, -2, n + 5):
                assert conn.bitPos(key, bit, (lower, upper)) == M.bitpos(data, int(bit), lower, upper), (bit, lower, upper)
    # the reference sends the upper bound only behind a bounded lower one: (None, upper) is BITPOS key bit
    ones = b"\xff" * 4
    client.getBitSet(fresh + ":ones").setBytes(ones)
    k1 = (fresh + ":ones").encode()
    assert conn.bitPos(k1, False, (None, 2)) == conn.bitPos(k1, False) == 32 == M.bitpos(ones, 0)
    assert conn.bitPos(k1, False, (0, 2)) == -1 == M.bitpos(ones, 0, 0, 2)
    with pytest.raises(IllegalArgumentException):
        conn.bitPos(k1, True, None)
    with pytest.raises(IllegalArgumentException):
        conn.getBit(None, 0)
    with pytest.raises(RedisException, match="bit offset"):
        conn.setBit(key, 1 << 32, True)
    assert client.getBitSet(fresh + ":ones").delete()


def test_bit_op_lengths_and_not_arity(client, fresh):
    conn = RedissonConnection(client)
    a, b, c, d = ((fresh + s).encode() for s in ("a", "b", "c", "d"))
    rng = np.random.default_rng(22)
    sa, sb = rng.bytes(300), rng.bytes(17)
    client.getBitSet(fresh + "a").setBytes(sa)
    client.getBitSet(fresh + "b").setBytes(sb)
    for op in ("AND", "OR", "XOR"):
        assert conn.bitOp(op, d, a, b, c) == 300  # the longest source; c is missing
        want = bitop(op.lower(), [sa, sb, b""])
        assert client.getBitSet(fresh + "d").toByteArray() == want
        assert conn.bitCount(d) == M.bitcount(want, 0, -1) and conn.strLen(d) == 300
    assert conn.bitOp("NOT", d, b) == 17
    assert client.getBitSet(fresh + "d").toByteArray() == bitop("not", [sb])
    assert conn.bitOp("not", d, c) == 0 and conn.strLen(d) == 0  # the empty result deletes dest
    # NOT with several sources fails before any command is sent
    client.getBitSet(fresh + "d").setBytes(b"\x01")
    with pytest.raises(UnsupportedOperationException, match="single source key"):
        conn.bitOp("NOT", d, a, b)
    assert client.getBitSet(fresh + "d").toByteArray() == b"\x01"
    with pytest.raises(IllegalArgumentException):
        conn.bitOp("NAND", d, a)
    for k in ("a", "b", "d"):
        client.getBitSet(fresh + k).delete()
