"""A numpy model of Redis strings used as bit sets: bytes, MSB-first bits (bit i = byte i>>3, mask
0x80 >> (i&7)), zero padding and the lazy length of SETBIT.  The expected values of
test_bitset_cpu.py / test_bitset_gpu.py come from here; semantics restated from redis 7.2
bitops.c (setbitCommand, getbitCommand, bitopCommand, bitposCommand) and from the Lua script of
RedissonBitSet.lengthAsync (M/RedissonBitSet.java:428-439)."""
import numpy as np

MAX_OFFSET = 1 << 32  # offsets end at 2^32 - 1


class RedisError(Exception):
    """an error reply (ERR bit offset is not an integer or out of range)"""


class RedisString:
    """One key: `data is None` = the key does not exist."""

    def __init__(self, data=None):
        self.data = None if data is None else np.frombuffer(bytes(data), np.uint8).copy()

    def bytes(self) -> bytes:
        return b"" if self.data is None else self.data.tobytes()

    def strlen(self) -> int:
        return 0 if self.data is None else int(self.data.size)

    def _grow(self, nbytes: int) -> None:
        if self.data is None:
            self.data = np.zeros(0, np.uint8)
        if self.data.size < nbytes:
            self.data = np.concatenate([self.data, np.zeros(nbytes - self.data.size, np.uint8)])

    def getbit(self, i: int) -> int:
        if not 0 <= i < MAX_OFFSET or i != int(i):
            raise RedisError("ERR bit offset is not an integer or out of range")
        i = int(i)
        if self.data is None or (i >> 3) >= self.data.size:
            return 0
        return int(self.data[i >> 3] >> (7 - (i & 7))) & 1

    def setbit(self, i: int, value) -> int:
        """SETBIT: grows the string to hold the bit whatever the value; returns the old bit"""
        if not 0 <= i < MAX_OFFSET:
            raise RedisError("ERR bit offset is not an integer or out of range")
        self._grow((i >> 3) + 1)
        old = self.getbit(i)
        mask = 0x80 >> (i & 7)
        if value:
            self.data[i >> 3] |= mask
        else:
            self.data[i >> 3] &= 0xFF ^ mask
        return old

    def set_indexes(self, idx, value) -> None:
        """BITFIELD set u1 .. per index: all parsed first (an offset error changes nothing)"""
        idx = np.asarray(idx, dtype=np.uint64)
        if idx.size == 0:
            return
        if int(idx.max()) >= MAX_OFFSET:
            raise RedisError("ERR bit offset is not an integer or out of range")
        self._grow((int(idx.max()) >> 3) + 1)
        byte = (idx >> np.uint64(3)).astype(np.int64)
        mask = (0x80 >> (idx & np.uint64(7)).astype(np.int64)).astype(np.uint8)
        if value:
            np.bitwise_or.at(self.data, byte, mask)
        else:
            np.bitwise_and.at(self.data, byte, ~mask)

    def get_indexes(self, idx) -> np.ndarray:
        idx = np.asarray(idx, dtype=np.uint64)
        out = np.zeros(idx.size, bool)
        n = self.strlen()
        byte = (idx >> np.uint64(3)).astype(np.int64)
        inside = byte < n
        if inside.any():
            sh = (7 - (idx[inside] & np.uint64(7)).astype(np.int64)).astype(np.uint8)
            out[inside] = (self.data[byte[inside]] >> sh) & 1
        return out

    def set_range(self, frm: int, to: int, value) -> None:
        """RBitSet.set(from, to, value): one SETBIT per index of [from, to) (empty: no command)"""
        if frm >= to:
            return
        self._grow(((to - 1) >> 3) + 1)
        bits = np.unpackbits(self.data)  # MSB-first, as Redis numbers them
        bits[frm:to] = 1 if value else 0
        self.data = np.packbits(bits)

    def bitcount(self) -> int:
        return 0 if self.data is None else int(np.unpackbits(self.data).sum())

    def bitpos_1_last_byte(self) -> int:
        """BITPOS key 1 -1: the first set bit of the last byte, -1 if none (or no key)"""
        if self.strlen() == 0:
            return -1
        last = int(self.data[-1])
        for j in range(8):
            if last & (0x80 >> j):
                return (self.strlen() - 1) * 8 + j
        return -1


def bitop(op: str, srcs) -> bytes:
    """BITOP op dest srcs..: the value dest receives (b"" = dest is deleted).  srcs: bytes, b"" for a
    missing key.  The result is as long as the longest source; shorter ones are zero-padded."""
    n = max(len(s) for s in srcs)
    cols = []
    for s in srcs:
        a = np.zeros(n, np.uint8)
        a[: len(s)] = np.frombuffer(bytes(s), np.uint8)
        cols.append(a)
    if op == "not":
        assert len(cols) == 1
        return (~cols[0]).tobytes()
    fn = {"and": np.bitwise_and, "or": np.bitwise_or, "xor": np.bitwise_xor}[op]
    r = cols[0]
    for a in cols[1:]:
        r = fn(r, a)
    return r.tobytes()


def lua_length(data: bytes):
    """The script of lengthAsync, line by line (Lua 5.1: numbers are doubles, `/` is real division,
    `%` is floored -- as Python's float `/` and `%`).  Returns its integer reply, or None when the
    script fails on an error reply."""
    key = RedisString(data if data else None)
    try:
        fromBit = float(key.bitpos_1_last_byte())      # local fromBit = redis.call('bitpos', KEYS[1], 1, -1);
        toBit = 8 * (fromBit / 8 + 1) - fromBit % 8    # local toBit = 8*(fromBit/8 + 1) - fromBit % 8;
        i = toBit                                      # for i = toBit, fromBit, -1 do
        while i >= fromBit:
            if key.getbit(i) == 1:                     # if redis.call('getbit', KEYS[1], i) == 1 then
                return int(i + 1)                      # return i+1;
            i -= 1
        return int(fromBit + 1)                        # return fromBit+1
    except RedisError:
        return None


def bits_of(data: bytes) -> list:
    """the set bits, as RBitSet.toString() lists them"""
    return np.flatnonzero(np.unpackbits(np.frombuffer(data, np.uint8))).tolist() if data else []
