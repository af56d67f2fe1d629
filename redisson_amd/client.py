"""Host mirror of the reference's object API for this path, over librbx.so.

Names, argument meaning and error behaviour follow the Java API so code (and tests)
read like the reference's own:

  RedissonClient.getBloomFilter / getHyperLogLog   M/api/RedissonClient.java:272,283,1038,1049
  RBloomFilter   M/api/RBloomFilter.java:27-113     (impl M/RedissonBloomFilter.java)
  RHyperLogLog   M/api/RHyperLogLog.java:27-68      (impl M/RedissonHyperLogLog.java)

M/ = /root/reference/redisson/src/main/java/org/redisson/
"""
from __future__ import annotations

import ctypes as C
import threading
from collections.abc import Collection

import numpy as np

from . import _lib as L
from .codec import DEFAULT_CODEC, Codec
from .exceptions import (IllegalArgumentException, IllegalStateException, RedisException, RedissonAmdError,
                         raise_for)
from .keys import Arena, _OneKey


def _check(rc: int) -> None:
    if rc != L.RBX_OK:
        raise_for(rc, L.last_error())


def _is_collection(x) -> bool:
    return isinstance(x, (list, tuple)) or (isinstance(x, Collection) and not isinstance(x, (str, bytes, bytearray)))


class RedissonClient:
    """Redisson.create(...) for one GPU (M/Redisson.java).  One engine context per device."""

    def __init__(self, device: int = 0):
        self._ctx = C.c_void_p()
        _check(L.lib().rbx_init(device, C.byref(self._ctx)))
        self.device = device
        self._lock = threading.Lock()

    @classmethod
    def create(cls, device: int = 0) -> "RedissonClient":
        return cls(device)

    @property
    def ctx(self):
        if not self._ctx:
            raise RuntimeError("client has been shut down")
        return self._ctx

    def getBloomFilter(self, name: str, codec: Codec | None = None) -> "RBloomFilter":
        return RBloomFilter(self, name, codec or DEFAULT_CODEC)

    def getHyperLogLog(self, name: str, codec: Codec | None = None) -> "RHyperLogLog":
        return RHyperLogLog(self, name, codec or DEFAULT_CODEC)

    def getBitSet(self, name: str) -> "RBitSet":
        """M/api/RedissonClient.java getBitSet(name)"""
        return RBitSet(self, name)

    def getBinaryStream(self, name: str) -> "RBinaryStream":
        """M/api/RedissonClient.java getBinaryStream(name)"""
        return RBinaryStream(self, name)

    def createBatch(self) -> "RBatch":
        """M/api/RedissonClient.java createBatch()"""
        return RBatch(self, range_stream_call=lambda *a: _engine_bitset_range_stream_call(self, *a),
                      members_stream_call=lambda *a: _engine_bitset_members_stream_call(self, *a))

    def shutdown(self) -> None:
        if self._ctx:
            _check(L.lib().rbx_shutdown(self._ctx))
            self._ctx = C.c_void_p()

    def synchronize(self) -> None:
        _check(L.lib().rbx_synchronize(self.ctx))

    def stream(self) -> int:
        return L.lib().rbx_stream(self.ctx) or 0

    get_bloom_filter = getBloomFilter
    get_hyper_log_log = getHyperLogLog
    get_bit_set = getBitSet
    get_binary_stream = getBinaryStream
    create_batch = createBatch

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.shutdown()


def _config_name(name: str) -> str:
    """suffixName(name, "config") (M/RedissonObject.java): the config hash shares the name's slot."""
    return name + ":config" if "{" in name else "{" + name + "}:config"


class _Expirable:
    """RExpirable (M/RedissonExpirable.java:53-251) over rbx_pexpire / rbx_persist / rbx_pttl.
    Times are milliseconds; `_expire_keys()` lists the keys a timeout applies to."""

    _COND = {None: 0, "NX": 1, "XX": 2, "GT": 3, "LT": 4}

    def _pexpire(self, when_ms: int, absolute: bool, cond=None) -> bool:
        keys = [k.encode() for k in self._expire_keys()]
        arr = (C.c_char_p * len(keys))(*keys)
        r = C.c_int()
        _check(L.lib().rbx_pexpire(self._client.ctx, arr, len(keys), int(when_ms), int(absolute), self._COND[cond],
                                   C.byref(r)))
        return bool(r.value)

    def expire(self, ttl_ms: int) -> bool:
        """expire(Duration) :118-125 -- PEXPIRE on every key"""
        return self._pexpire(ttl_ms, False)

    def expireAt(self, unix_ms: int) -> bool:
        """expireAt(long) :58-65 -- PEXPIREAT"""
        return self._pexpire(unix_ms, True)

    def expireIfSet(self, ttl_ms: int) -> bool:
        """:138-145 -- PEXPIRE .. XX"""
        return self._pexpire(ttl_ms, False, "XX")

    def expireIfNotSet(self, ttl_ms: int) -> bool:
        """:148-155 -- PEXPIRE .. NX"""
        return self._pexpire(ttl_ms, False, "NX")

    def expireIfGreater(self, ttl_ms: int) -> bool:
        """PEXPIRE .. GT"""
        return self._pexpire(ttl_ms, False, "GT")

    def expireIfLess(self, ttl_ms: int) -> bool:
        """PEXPIRE .. LT"""
        return self._pexpire(ttl_ms, False, "LT")

    def clearExpire(self) -> bool:
        """clearExpireAsync :183-185 / :241-251 -- PERSIST"""
        keys = [k.encode() for k in self._expire_keys()]
        arr = (C.c_char_p * len(keys))(*keys)
        r = C.c_int()
        _check(L.lib().rbx_persist(self._client.ctx, arr, len(keys), C.byref(r)))
        return bool(r.value)

    def remainTimeToLive(self) -> int:
        """:188-195 -- PTTL name (-2 missing, -1 no timeout)"""
        out = C.c_int64()
        _check(L.lib().rbx_pttl(self._client.ctx, self._expire_keys()[0].encode(), C.byref(out)))
        return int(out.value)

    def getExpireTime(self) -> int:
        """:198-205 -- PEXPIRETIME name"""
        out = C.c_int64()
        _check(L.lib().rbx_pexpiretime(self._client.ctx, self._expire_keys()[0].encode(), C.byref(out)))
        return int(out.value)


class RBloomFilter(_Expirable):
    """M/RedissonBloomFilter.java.  size/hashIterations are cached like the reference's
    volatile fields (:61-62) and re-validated on every batch (addConfigCheck :207-213)."""

    def __init__(self, client: RedissonClient, name: str, codec: Codec):
        self._client = client
        self._name = name
        self._codec = codec
        self._size = 0
        self._k = 0

    # ---- naming --------------------------------------------------------------------
    def getName(self) -> str:
        return self._name

    def _bname(self) -> bytes:
        return self._name.encode("utf-8")

    # ---- init / config -----------------------------------------------------------------
    def tryInit(self, expectedInsertions: int, falseProbability: float) -> bool:
        """:262-300 -- False (and the existing config cached) when already initialized."""
        created = C.c_int()
        _check(L.lib().rbx_bloom_try_init(self._client.ctx, self._bname(), int(expectedInsertions),
                                          float(falseProbability), C.byref(created)))
        self._read_config()
        return bool(created.value)

    def tryInitRaw(self, size: int, hashIterations: int) -> bool:
        """Engine-level init with an explicit (size, k); reaches size = 2^32."""
        created = C.c_int()
        _check(L.lib().rbx_bloom_init_raw(self._client.ctx, self._bname(), int(size), int(hashIterations),
                                          C.byref(created)))
        self._read_config()
        return bool(created.value)

    def _config(self) -> L.RbxBloomConfig:
        cfg = L.RbxBloomConfig()
        _check(L.lib().rbx_bloom_read_config(self._client.ctx, self._bname(), C.byref(cfg)))
        return cfg

    def _read_config(self) -> None:  # readConfig() :240-255
        cfg = self._config()
        self._size = cfg.size
        self._k = cfg.hash_iterations

    def getSize(self) -> int:
        return int(self._config().size)

    def getHashIterations(self) -> int:
        return int(self._config().hash_iterations)

    def getExpectedInsertions(self) -> int:
        return int(self._config().expected_insertions)

    def getFalseProbability(self) -> float:
        return float(self._config().false_probability_str.decode())

    # ---- hot path ------------------------------------------------------------------
    def _encode_all(self, objects) -> Arena:
        return Arena([self._codec.encode(o) for o in objects])

    def _one(self, obj) -> "_OneKey":
        return _OneKey(self._codec.encode(obj))

    def _batch(self, fn, objects, flags: bool):
        if self._size == 0:  # :106-108
            self._read_config()
        a = objects if isinstance(objects, (Arena, _OneKey)) else self._encode_all(objects)
        out = np.zeros(max(a.n, 1), np.uint8) if flags else None
        cnt = C.c_uint64()
        _check(fn(self._client.ctx, self._bname(), self._size, self._k, a.ptr(),
                  out.ctypes.data_as(L.u8p) if flags else None, C.byref(cnt)))
        return (int(cnt.value), out[: a.n]) if flags else int(cnt.value)

    def add(self, objects):
        """add(T) -> bool  |  add(Collection<T>) -> long  (:99-137)"""
        if isinstance(objects, Arena) or _is_collection(objects):
            return self._batch(L.lib().rbx_bloom_add, objects, False)
        return self._batch(L.lib().rbx_bloom_add, self._one(objects), False) > 0

    def contains(self, objects):
        """contains(T) -> bool  |  contains(Collection<T>) -> long  (:153-201)"""
        if isinstance(objects, Arena) or _is_collection(objects):
            return self._batch(L.lib().rbx_bloom_contains, objects, False)
        return self._batch(L.lib().rbx_bloom_contains, self._one(objects), False) > 0

    def addEach(self, objects):
        """(count, per-key 'newly added' flags) -- engine extension of add(Collection)."""
        return self._batch(L.lib().rbx_bloom_add, objects, True)

    def containsEach(self, objects):
        """(count, per-key presence flags) -- engine extension of contains(Collection)."""
        return self._batch(L.lib().rbx_bloom_contains, objects, True)

    def count(self) -> int:
        """:215-227"""
        out = C.c_int64()
        _check(L.lib().rbx_bloom_count(self._client.ctx, self._bname(), C.byref(out)))
        self._read_config()
        return int(out.value)

    # ---- RObject / RExpirable --------------------------------------------------------
    def delete(self) -> bool:
        n = C.c_int()
        _check(L.lib().rbx_bloom_delete(self._client.ctx, self._bname(), C.byref(n)))
        return n.value > 0

    def isExists(self) -> bool:
        e = C.c_int()
        _check(L.lib().rbx_bloom_is_exists(self._client.ctx, self._bname(), C.byref(e)))
        return bool(e.value)

    def sizeInMemory(self) -> int:
        """:234-238 -- the bitmap and the config hash (engine bytes)"""
        out = C.c_uint64()
        _check(L.lib().rbx_bloom_size_in_memory(self._client.ctx, self._bname(), C.byref(out)))
        return int(out.value)

    def _expire_keys(self):
        # M/RedissonBloomFilter.java:303-314: the bitmap and its config hash
        return [self._name, _config_name(self._name)]

    def rename(self, newName: str) -> None:
        _check(L.lib().rbx_bloom_rename(self._client.ctx, self._bname(), newName.encode()))
        self._name = newName

    def renamenx(self, newName: str) -> bool:
        r = C.c_int()
        _check(L.lib().rbx_bloom_renamenx(self._client.ctx, self._bname(), newName.encode(), C.byref(r)))
        if r.value:
            self._name = newName
        return bool(r.value)

    # ---- persistence (Redis string format) ----------------------------------------------
    def exportBitmap(self) -> bytes:
        n = C.c_uint64()
        _check(L.lib().rbx_bloom_export(self._client.ctx, self._bname(), None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.uint8)
        _check(L.lib().rbx_bloom_export(self._client.ctx, self._bname(), buf.ctypes.data_as(L.u8p), n.value,
                                        C.byref(n)))
        return buf[: n.value].tobytes()

    def importBitmap(self, data: bytes) -> None:
        buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
        _check(L.lib().rbx_bloom_import(self._client.ctx, self._bname(), buf.ctypes.data_as(L.u8p), len(data)))

    def digest(self) -> int:
        """Order-independent 64-bit digest of `GET name` (0 = no bitmap): replica comparison."""
        out = C.c_uint64()
        _check(L.lib().rbx_bloom_digest(self._client.ctx, self._bname(), C.byref(out)))
        return int(out.value)

    def bitcount(self) -> int:
        out = C.c_uint64()
        _check(L.lib().rbx_bloom_bitcount(self._client.ctx, self._bname(), C.byref(out)))
        return int(out.value)

    # snake_case aliases
    try_init = tryInit
    get_size = getSize
    get_hash_iterations = getHashIterations
    is_exists = isExists


class RBitSet(_Expirable):
    """M/RedissonBitSet.java over rbx_bitset_*: the Redis string under `name` as a bit set -- for a
    Bloom filter's name, the filter's own bits (createBitSet, M/RedissonBloomFilter.java:203-205)."""

    def __init__(self, client: RedissonClient, name: str):
        self._client = client
        self._name = name

    def getName(self) -> str:
        return self._name

    def _n(self, name: str | None = None):
        """(rbx_name, keep-alive) of this key or another"""
        return L.name_struct(self._name if name is None else name)

    @staticmethod
    def _indexes(indexes) -> np.ndarray:
        a = np.asarray(indexes)
        if a.size and (a.dtype.kind not in "iu" or (a.dtype.kind == "i" and int(a.min()) < 0)):
            raise IllegalArgumentException("bit indexes are non-negative integers")
        return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)

    # ---- single bits ------------------------------------------------------------------
    def get(self, bitIndex: int) -> bool:
        """:277-279 GETBIT"""
        nm, _keep = self._n()
        bit = C.c_int()
        _check(L.lib().rbx_bitset_get(self._client.ctx, nm, int(bitIndex), C.byref(bit)))
        return bool(bit.value)

    def set(self, bitIndex: int, value: bool = True) -> bool:
        """:302-305 SETBIT -> the bit before"""
        nm, _keep = self._n()
        old = C.c_int()
        _check(L.lib().rbx_bitset_set(self._client.ctx, nm, int(bitIndex), int(bool(value)), C.byref(old)))
        return bool(old.value)

    def clearBit(self, bitIndex: int) -> bool:
        """clear(bitIndex) :487-489"""
        return self.set(bitIndex, False)

    # ---- ranges and batches ---------------------------------------------------------------
    def setRange(self, fromIndex: int, toIndex: int, value: bool = True) -> None:
        """set(fromIndex, toIndex, value) :442-454 -- bits [fromIndex, toIndex)"""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_set_range(self._client.ctx, nm, int(fromIndex), int(toIndex), int(bool(value))))

    def clearRange(self, fromIndex: int, toIndex: int) -> None:
        """clear(fromIndex, toIndex) :452-454"""
        self.setRange(fromIndex, toIndex, False)

    def setIndexes(self, indexes, value: bool = True) -> None:
        """set(long[] indexArray, value) :312-324"""
        idx = self._indexes(indexes)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_set_indexes(self._client.ctx, nm, idx.ctypes.data_as(L.u64p), idx.size,
                                              int(bool(value))))

    def getIndexes(self, indexes) -> np.ndarray:
        """One GETBIT per index -- engine extension, like containsEach."""
        idx = self._indexes(indexes)
        out = np.zeros(max(idx.size, 1), np.uint8)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_get_indexes(self._client.ctx, nm, idx.ctypes.data_as(L.u64p), idx.size,
                                              out.ctypes.data_as(L.u8p)))
        return out[: idx.size].astype(bool)

    def setIndexesDev(self, d_indexes: int, n: int, value: bool = True, stream: int | None = None) -> None:
        """setIndexes over a device array of n u64 indexes (rbx_bitset_set_indexes_dev)."""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_set_indexes_dev(self._client.ctx, nm, d_indexes, int(n), int(bool(value)), stream))

    def getIndexesDev(self, d_indexes: int, n: int, d_out: int, stream: int | None = None) -> None:
        """getIndexes over device arrays: d_out receives n bytes (rbx_bitset_get_indexes_dev)."""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_get_indexes_dev(self._client.ctx, nm, d_indexes, int(n), d_out, stream))

    # ---- typed fields: BITFIELD GET / SET / INCRBY (:71-254) --------------------------------
    @staticmethod
    def _java(value: int, bits: int, what: str) -> int:
        """a Java argument of a `bits`-wide integral type"""
        value = int(value)
        if not -(1 << (bits - 1)) <= value < (1 << (bits - 1)):
            raise IllegalArgumentException(f"{what} {value} is outside the Java type's range ({bits} bits)")
        return value

    def _field(self, op: int, signed: bool, size: int, offset: int, value: int = 0) -> int:
        nm, _keep = self._n()
        size = self._java(size, 32, "size")
        offset = self._java(offset, 64, "offset") & 0xFFFFFFFFFFFFFFFF  # a negative long is past the limit too
        reply = C.c_int64()
        _check(L.lib().rbx_bitset_field(self._client.ctx, nm, op, int(signed), size, offset,
                                        self._java(value, 64, "value"), C.byref(reply)))
        return int(reply.value)

    def getSigned(self, size: int, offset: int) -> int:
        """:71-77 BITFIELD GET i<size> offset"""
        return self._field(L.RBX_FIELD_GET, True, size, offset)

    def setSigned(self, size: int, offset: int, value: int) -> int:
        """:80-86 BITFIELD SET i<size> offset value -> the old value"""
        return self._field(L.RBX_FIELD_SET, True, size, offset, value)

    def incrementAndGetSigned(self, size: int, offset: int, increment: int) -> int:
        """:89-95 BITFIELD INCRBY i<size> offset increment -> the new value"""
        return self._field(L.RBX_FIELD_INCRBY, True, size, offset, increment)

    def getUnsigned(self, size: int, offset: int) -> int:
        """:98-104 BITFIELD GET u<size> offset"""
        return self._field(L.RBX_FIELD_GET, False, size, offset)

    def setUnsigned(self, size: int, offset: int, value: int) -> int:
        """:107-113"""
        return self._field(L.RBX_FIELD_SET, False, size, offset, value)

    def incrementAndGetUnsigned(self, size: int, offset: int, increment: int) -> int:
        """:116-122"""
        return self._field(L.RBX_FIELD_INCRBY, False, size, offset, increment)

    def getByte(self, offset: int) -> int:
        """:185-200 the i8 forms (Java byte)"""
        return self._field(L.RBX_FIELD_GET, True, 8, offset)

    def setByte(self, offset: int, value: int) -> int:
        return self._field(L.RBX_FIELD_SET, True, 8, offset, self._java(value, 8, "value"))

    def incrementAndGetByte(self, offset: int, increment: int) -> int:
        return self._field(L.RBX_FIELD_INCRBY, True, 8, offset, self._java(increment, 8, "increment"))

    def getShort(self, offset: int) -> int:
        """:203-218 the i16 forms (Java short)"""
        return self._field(L.RBX_FIELD_GET, True, 16, offset)

    def setShort(self, offset: int, value: int) -> int:
        return self._field(L.RBX_FIELD_SET, True, 16, offset, self._java(value, 16, "value"))

    def incrementAndGetShort(self, offset: int, increment: int) -> int:
        return self._field(L.RBX_FIELD_INCRBY, True, 16, offset, self._java(increment, 16, "increment"))

    def getInteger(self, offset: int) -> int:
        """:221-236 the i32 forms (Java int)"""
        return self._field(L.RBX_FIELD_GET, True, 32, offset)

    def setInteger(self, offset: int, value: int) -> int:
        return self._field(L.RBX_FIELD_SET, True, 32, offset, self._java(value, 32, "value"))

    def incrementAndGetInteger(self, offset: int, increment: int) -> int:
        return self._field(L.RBX_FIELD_INCRBY, True, 32, offset, self._java(increment, 32, "increment"))

    def getLong(self, offset: int) -> int:
        """:239-254 the i64 forms (Java long)"""
        return self._field(L.RBX_FIELD_GET, True, 64, offset)

    def setLong(self, offset: int, value: int) -> int:
        return self._field(L.RBX_FIELD_SET, True, 64, offset, value)

    def incrementAndGetLong(self, offset: int, increment: int) -> int:
        return self._field(L.RBX_FIELD_INCRBY, True, 64, offset, increment)

    @staticmethod
    def _values(values, n: int) -> np.ndarray:
        a = np.asarray(values)
        if a.size and (a.dtype.kind not in "iu" or (a.dtype == np.uint64 and int(a.max()) >= 1 << 63)):
            raise IllegalArgumentException("field values are Java longs")
        a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        if a.size != n:
            raise IllegalArgumentException("one value per offset")
        return a

    @staticmethod
    def _overflow(overflow) -> int:
        """BITFIELD's OVERFLOW mode: 'WRAP' / 'SAT' / 'FAIL' or an RBX_OVERFLOW_* value"""
        modes = {"WRAP": L.RBX_OVERFLOW_WRAP, "SAT": L.RBX_OVERFLOW_SAT, "FAIL": L.RBX_OVERFLOW_FAIL}
        if isinstance(overflow, str):
            code = modes.get(overflow.upper())
        else:
            code = overflow if overflow in modes.values() else None
        if code is None:
            raise IllegalArgumentException(f"unknown OVERFLOW mode {overflow!r}")
        return code

    def _fields(self, op: int, signed: bool, size: int, offsets, values, replies: bool, overflow="WRAP"):
        """one BITFIELD of len(offsets) sub-commands of one operation and type (rbx_bitset_fields, and
        rbx_bitset_fields_ov under OVERFLOW SAT / FAIL).  FAIL returns (replies, nil)."""
        mode = self._overflow(overflow)
        offs = self._indexes(offsets)
        vals = None if values is None else self._values(values, offs.size)
        out = np.zeros(max(offs.size, 1), np.int64) if replies else None
        nm, _keep = self._n()
        args = (offs.ctypes.data_as(L.u64p), None if vals is None else vals.ctypes.data_as(L.i64p), offs.size,
                None if out is None else out.ctypes.data_as(L.i64p))
        size = self._java(size, 32, "size")
        if mode == L.RBX_OVERFLOW_WRAP:
            _check(L.lib().rbx_bitset_fields(self._client.ctx, nm, op, int(signed), size, *args))
            return None if out is None else out[: offs.size]
        nil = np.zeros(max(offs.size, 1), np.uint8)
        _check(L.lib().rbx_bitset_fields_ov(self._client.ctx, nm, op, int(signed), size, mode, *args,
                                            nil.ctypes.data_as(L.u8p)))
        rep = None if out is None else out[: offs.size]
        return (rep, nil[: offs.size].astype(bool)) if mode == L.RBX_OVERFLOW_FAIL else rep

    def getFields(self, size: int, offsets, signed: bool = True) -> np.ndarray:
        """One GET per offset, in one BITFIELD -- engine extension, like getIndexes."""
        return self._fields(L.RBX_FIELD_GET, signed, size, offsets, None, True)

    def setFields(self, size: int, offsets, values, signed: bool = True, replies: bool = True, overflow="WRAP"):
        """One SET per (offset, value), in array order -> the old values (int64), or None.  overflow: 'WRAP' /
        'SAT' / 'FAIL' (rbx.h: OVERFLOW); FAIL returns (replies, nil), nil[i] = reply i is nil (field untouched)."""
        return self._fields(L.RBX_FIELD_SET, signed, size, offsets, values, replies, overflow)

    def incrementFields(self, size: int, offsets, increments, signed: bool = True, replies: bool = True,
                        overflow="WRAP"):
        """One INCRBY per (offset, increment), in array order -> the new values (int64), or None.  overflow as
        for setFields: SAT makes packed fields saturating counters."""
        return self._fields(L.RBX_FIELD_INCRBY, signed, size, offsets, increments, replies, overflow)

    def _fields_dev(self, op, signed, size, d_offsets, d_values, n, d_replies, stream, overflow="WRAP",
                    d_nil=None) -> None:
        nm, _keep = self._n()
        mode = self._overflow(overflow)
        size = self._java(size, 32, "size")
        if mode == L.RBX_OVERFLOW_WRAP and d_nil is None:
            _check(L.lib().rbx_bitset_fields_dev(self._client.ctx, nm, op, int(signed), size, d_offsets, d_values,
                                                 int(n), d_replies, stream))
        else:
            _check(L.lib().rbx_bitset_fields_ov_dev(self._client.ctx, nm, op, int(signed), size, mode, d_offsets,
                                                    d_values, int(n), d_replies, d_nil, stream))

    def getFieldsDev(self, size: int, d_offsets: int, n: int, d_replies: int, signed: bool = True,
                     stream: int | None = None) -> None:
        """getFields over device arrays: n u64 offsets, n i64 replies (rbx_bitset_fields_dev)."""
        self._fields_dev(L.RBX_FIELD_GET, signed, size, d_offsets, None, n, d_replies, stream)

    def setFieldsDev(self, size: int, d_offsets: int, d_values: int, n: int, d_replies: int | None = None,
                     signed: bool = True, stream: int | None = None, overflow="WRAP", d_nil: int | None = None) -> None:
        """setFields over device arrays; d_replies (n i64) may be None.  d_nil (n bytes) receives the nil mask;
        FAIL with d_replies needs it (rbx_bitset_fields_ov_dev)."""
        self._fields_dev(L.RBX_FIELD_SET, signed, size, d_offsets, d_values, n, d_replies, stream, overflow, d_nil)

    def incrementFieldsDev(self, size: int, d_offsets: int, d_increments: int, n: int, d_replies: int | None = None,
                           signed: bool = True, stream: int | None = None, overflow="WRAP",
                           d_nil: int | None = None) -> None:
        """incrementFields over device arrays; without d_replies an aligned batch of a size dividing 64
        is one atomic per element (packed counters) -- under WRAP always, under SAT when every increment has
        one sign (saturating counters).  d_nil as for setFieldsDev."""
        self._fields_dev(L.RBX_FIELD_INCRBY, signed, size, d_offsets, d_increments, n, d_replies, stream, overflow,
                         d_nil)

    # ---- whole-string reads -----------------------------------------------------------------
    def cardinality(self) -> int:
        """:482-484 BITCOUNT"""
        nm, _keep = self._n()
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_cardinality(self._client.ctx, nm, C.byref(out)))
        return int(out.value)

    def size(self) -> int:
        """:472-474 STRLEN * 8"""
        nm, _keep = self._n()
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_size(self._client.ctx, nm, C.byref(out)))
        return int(out.value)

    def length(self) -> int:
        """:428-439 -- the script's answer (see rbx_bitset_length), not java.util.BitSet.length()"""
        nm, _keep = self._n()
        out = C.c_int64()
        _check(L.lib().rbx_bitset_length(self._client.ctx, nm, C.byref(out)))
        return int(out.value)

    # ---- ranged BITCOUNT / BITPOS: engine extensions, the reference's RBitSet has none of them ----
    @staticmethod
    def _unit(unit) -> int:
        u = unit.upper() if isinstance(unit, str) else unit
        if u not in ("BYTE", "BIT", L.RBX_RANGE_BYTE, L.RBX_RANGE_BIT):
            raise IllegalArgumentException("the unit is 'BYTE' or 'BIT'")
        return L.RBX_RANGE_BIT if u in ("BIT", L.RBX_RANGE_BIT) else L.RBX_RANGE_BYTE

    @staticmethod
    def _bounds(values, what: str) -> np.ndarray:
        a = np.asarray(values)
        if a.size and (a.dtype.kind not in "iu" or (a.dtype == np.uint64 and int(a.max()) >= 1 << 63)):
            raise IllegalArgumentException(f"range {what} are signed 64-bit integers")
        return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)

    def bitCount(self, start: int | None = None, end: int | None = None, unit="BYTE") -> int:
        """Engine extension (rbx_bitset_count_range): BITCOUNT name start end [BYTE|BIT], both ends inclusive,
        negative values counting from the end.  Without arguments it is cardinality()."""
        if start is None and end is None:
            return self.cardinality()
        if start is None or end is None:
            raise IllegalArgumentException("BITCOUNT takes both start and end, or neither")
        nm, _keep = self._n()
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_count_range(self._client.ctx, nm, self._java(start, 64, "start"),
                                              self._java(end, 64, "end"), self._unit(unit), C.byref(out)))
        return int(out.value)

    def bitPos(self, bit, start: int | None = None, end: int | None = None, unit="BYTE") -> int:
        """Engine extension (rbx_bitset_pos): BITPOS name bit [start [end [BYTE|BIT]]] -> the first position
        holding `bit` as an absolute bit offset, or -1 (see rbx.h for the string's zero-padded right side)."""
        if start is None and end is not None:
            raise IllegalArgumentException("BITPOS takes an end only after a start")
        nargs = 0 if start is None else (1 if end is None else 2)
        nm, _keep = self._n()
        out = C.c_int64()
        _check(L.lib().rbx_bitset_pos(self._client.ctx, nm, self._java(int(bit), 32, "bit"), nargs,
                                      self._java(start or 0, 64, "start"), self._java(end or 0, 64, "end"),
                                      self._unit(unit), C.byref(out)))
        return int(out.value)

    def countRanges(self, starts, ends, unit="BYTE") -> np.ndarray:
        """Engine extension (rbx_bitset_count_ranges): one bitCount(starts[i], ends[i], unit) per element, in one
        call -> uint64 counts."""
        s, e = self._bounds(starts, "starts"), self._bounds(ends, "ends")
        if s.size != e.size:
            raise IllegalArgumentException("one end per start")
        out = np.zeros(max(s.size, 1), np.uint64)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_count_ranges(self._client.ctx, nm, s.ctypes.data_as(L.i64p), e.ctypes.data_as(L.i64p),
                                               s.size, self._unit(unit), out.ctypes.data_as(L.u64p)))
        return out[: s.size]

    def posRanges(self, bit, starts, ends=None, unit="BYTE") -> np.ndarray:
        """Engine extension (rbx_bitset_pos_ranges): one bitPos(bit, starts[i], ends[i], unit) per element, in one
        call -> int64 positions; ends=None makes every query bitPos(bit, starts[i])."""
        s = self._bounds(starts, "starts")
        e = None if ends is None else self._bounds(ends, "ends")
        if e is not None and s.size != e.size:
            raise IllegalArgumentException("one end per start")
        out = np.zeros(max(s.size, 1), np.int64)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_pos_ranges(self._client.ctx, nm, self._java(int(bit), 32, "bit"),
                                             s.ctypes.data_as(L.i64p), None if e is None else e.ctypes.data_as(L.i64p),
                                             s.size, self._unit(unit), out.ctypes.data_as(L.i64p)))
        return out[: s.size]

    def countRangesDev(self, d_starts: int, d_ends: int, n: int, d_out: int, unit="BYTE",
                       stream: int | None = None) -> None:
        """Engine extension: countRanges over device arrays, n i64 starts and ends, n u64 counts
        (rbx_bitset_count_ranges_dev; waits once on the stream)."""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_count_ranges_dev(self._client.ctx, nm, d_starts, d_ends, int(n), self._unit(unit),
                                                   d_out, stream))

    def posRangesDev(self, bit, d_starts: int, d_ends: int | None, n: int, d_out: int, unit="BYTE",
                     stream: int | None = None) -> None:
        """Engine extension: posRanges over device arrays; d_ends may be None (rbx_bitset_pos_ranges_dev)."""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_pos_ranges_dev(self._client.ctx, nm, self._java(int(bit), 32, "bit"), d_starts, d_ends,
                                                 int(n), self._unit(unit), d_out, stream))

    def toByteArray(self) -> bytes:
        """:327-334 GET (empty for a missing key)"""
        nm, _keep = self._n()
        n = C.c_uint64()
        _check(L.lib().rbx_bitset_export_n(self._client.ctx, nm, None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.uint8)
        _check(L.lib().rbx_bitset_export_n(self._client.ctx, nm, buf.ctypes.data_as(L.u8p), n.value, C.byref(n)))
        return buf[: n.value].tobytes()

    def setBytes(self, data: bytes) -> None:
        """set(BitSet) :457-459 -- SET name <bytes> (the caller lays the bits out MSB-first)"""
        buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_import_n(self._client.ctx, nm, buf.ctypes.data_as(L.u8p), len(data)))

    # ---- the exchange with java.util.BitSet: asBitSet() :391-408, set(BitSet) :411-420, :457-459 ----
    def asBitSet(self) -> np.ndarray:
        """asBitSet().toLongArray(): the BitSet's words in use as uint64, bit j of word w = bit 64 w + j
        (rbx_bitset_as_words; empty for no set bit or a missing key)."""
        nm, _keep = self._n()
        n = C.c_uint64()
        _check(L.lib().rbx_bitset_as_words(self._client.ctx, nm, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint64)
        _check(L.lib().rbx_bitset_as_words(self._client.ctx, nm, out.ctypes.data_as(L.u64p), n.value, C.byref(n)))
        return out[: n.value]

    def asBitSetDev(self, d_words: int | None, cap_words: int, d_nwords: int, stream: int | None = None) -> None:
        """asBitSet over device memory: min(cap_words, nwords) u64 words at d_words, the u64 nwords at d_nwords
        (rbx_bitset_as_words_dev; does not wait)."""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_as_words_dev(self._client.ctx, nm, d_words, int(cap_words), d_nwords, stream))

    def setBitSet(self, words) -> None:
        """set(BitSet.valueOf(words)): stores toByteArrayReverse's string, length() / 8 + 1 bytes -- one zero byte
        for the empty BitSet (rbx_bitset_set_words)."""
        w = np.ascontiguousarray(np.asarray(words, dtype=np.uint64)).reshape(-1)
        buf = w if w.size else np.zeros(1, np.uint64)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_set_words(self._client.ctx, nm, buf.ctypes.data_as(L.u64p), w.size))

    def setBitSetDev(self, d_words: int | None, nwords: int, stream: int | None = None) -> None:
        """setBitSet of nwords u64 device words (rbx_bitset_set_words_dev; waits once on the stream)."""
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_set_words_dev(self._client.ctx, nm, d_words, int(nwords), stream))

    # ---- set-bit enumeration: an engine extension, the inverse of setIndexes ----
    def _members_args(self, start, end, unit):
        if (start is None) != (end is None):
            raise IllegalArgumentException("members takes both start and end, or neither")
        nargs = 0 if start is None else 2
        return nargs, self._java(start or 0, 64, "start"), self._java(end or 0, 64, "end"), self._unit(unit)

    def members(self, start: int | None = None, end: int | None = None, unit="BYTE", skip: int = 0,
                limit: int | None = None) -> np.ndarray:
        """Engine extension (rbx_bitset_members): the positions of the set bits of bitCount(start, end, unit)'s
        interval, ascending, as uint64 -- those of rank skip .. skip + limit - 1; limit=None means all.  Two calls: a
        count-only one sizes the array (each builds the string's block directory; membersDev into a buffer of the
        caller's is the one-call form)."""
        nargs, s, e, u = self._members_args(start, end, unit)
        if skip < 0 or (limit is not None and limit < 0):
            raise IllegalArgumentException("skip and limit are not negative")
        nm, _keep = self._n()
        written, total = C.c_uint64(), C.c_uint64()
        # size the page first, by a count-only call: the array then holds what is left, whatever limit says
        _check(L.lib().rbx_bitset_members(self._client.ctx, nm, nargs, s, e, u, int(skip), 0, None,
                                          C.byref(written), C.byref(total)))
        cap = total.value - min(int(skip), total.value)
        if limit is not None:
            cap = min(cap, int(limit))
        out = np.zeros(max(cap, 1), np.uint64)
        if cap:
            _check(L.lib().rbx_bitset_members(self._client.ctx, nm, nargs, s, e, u, int(skip), cap,
                                              out.ctypes.data_as(L.u64p), C.byref(written), C.byref(total)))
        return out[: written.value]

    def membersDev(self, d_out: int | None, cap: int, d_counts: int, start: int | None = None, end: int | None = None,
                   unit="BYTE", skip: int = 0, stream: int | None = None) -> None:
        """members over device memory: up to cap u64 positions at d_out, {written, total} as two u64 at d_counts
        (rbx_bitset_members_dev; waits once on the stream)."""
        nargs, s, e, u = self._members_args(start, end, unit)
        nm, _keep = self._n()
        _check(L.lib().rbx_bitset_members_dev(self._client.ctx, nm, nargs, s, e, u, int(skip), int(cap), d_out,
                                              d_counts, stream))

    def toString(self) -> str:
        """toString() :423-425 = asBitSet().toString(): java.util.BitSet's "{1, 5, 9}" form, built on members()."""
        return "{" + ", ".join(str(int(p)) for p in self.members()) + "}"

    # ---- BITOP ------------------------------------------------------------------------------
    def _op(self, op: int, names) -> int:
        """opAsync :381-388 -- BITOP op name name others..; returns the reply (the result's length)"""
        nm, _keep = self._n()
        arr, _keep2 = L.names_array([self._name, *names])
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_op(self._client.ctx, op, nm, arr, 1 + len(names), C.byref(out)))
        return int(out.value)

    def or_(self, *bitSetNames: str) -> None:
        self._op(L.RBX_BITOP_OR, bitSetNames)

    def and_(self, *bitSetNames: str) -> None:
        self._op(L.RBX_BITOP_AND, bitSetNames)

    def xor(self, *bitSetNames: str) -> None:
        self._op(L.RBX_BITOP_XOR, bitSetNames)

    def not_(self) -> None:
        """:462-464 BITOP NOT name name"""
        self._op(L.RBX_BITOP_NOT, ())

    # ---- RObject / RExpirable ---------------------------------------------------------------
    def clear(self) -> None:
        """:492-494 DEL name"""
        self.delete()

    def delete(self) -> bool:
        arr, _keep = L.names_array([self._name])
        n = C.c_int()
        _check(L.lib().rbx_del_n(self._client.ctx, arr, 1, C.byref(n)))
        return n.value > 0

    def isExists(self) -> bool:
        arr, _keep = L.names_array([self._name])
        n = C.c_int()
        _check(L.lib().rbx_exists_n(self._client.ctx, arr, 1, C.byref(n)))
        return n.value > 0

    def rename(self, newName: str) -> None:
        """M/RedissonObject.java:151-153 RENAME name newName"""
        nm, _keep = self._n()
        new, _keep2 = self._n(newName)
        _check(L.lib().rbx_bitset_rename(self._client.ctx, nm, new))
        self._name = newName

    def _expire_keys(self):
        return [self._name]

    clear_bit = clearBit
    set_range = setRange
    clear_range = clearRange
    set_indexes = setIndexes
    get_indexes = getIndexes
    get_signed = getSigned
    set_signed = setSigned
    increment_and_get_signed = incrementAndGetSigned
    get_unsigned = getUnsigned
    set_unsigned = setUnsigned
    increment_and_get_unsigned = incrementAndGetUnsigned
    get_byte = getByte
    set_byte = setByte
    increment_and_get_byte = incrementAndGetByte
    get_short = getShort
    set_short = setShort
    increment_and_get_short = incrementAndGetShort
    get_integer = getInteger
    set_integer = setInteger
    increment_and_get_integer = incrementAndGetInteger
    get_long = getLong
    set_long = setLong
    increment_and_get_long = incrementAndGetLong
    get_fields = getFields
    set_fields = setFields
    increment_fields = incrementFields
    get_fields_dev = getFieldsDev
    set_fields_dev = setFieldsDev
    increment_fields_dev = incrementFieldsDev
    to_byte_array = toByteArray
    is_exists = isExists


# ---- RBatch: queued commands, executed in submission order (M/RedissonBatch.java, M/api/RBatch.java) --------
GETBIT, SETBIT0, SETBIT1 = 0, 1, 2  # cmd_op of rbx_bitset_stream
_FAILED_REPLY = 0xFF
_BIT_OFFSET_LIMIT = 1 << 32


class RBinaryStream(_Expirable):
    """M/RedissonBinaryStream.java (a bucket of bytes, M/RedissonBucket.java) over the key's Redis string: the one the
    bit commands of RBitSet reach.  The streams and the channel move bytes with APPEND, GETRANGE and SETRANGE on the
    device; nothing but the caller's own bytes crosses the host link."""

    def __init__(self, client: RedissonClient, name: str):
        self._client = client
        self._name = name

    def getName(self) -> str:
        return self._name

    def _expire_keys(self) -> list[str]:
        return [self._name]

    def get(self) -> bytes | None:
        """RBucket.get = GET: None for a missing key"""
        _r, status, _off, out = string_stream(self._client, [self._name], [0], [(L.RBX_STR_GET, 0, 0, b"")])
        return None if int(status[0]) == STRING_NIL else out

    def set(self, value: bytes) -> None:
        """RBucket.set = SET: replaces the key whatever it held and drops its timeout"""
        nm, _keep = L.name_struct(self._name)
        ptr, n, _buf = _u8(value)
        _check(L.lib().rbx_bitset_import_n(self._client.ctx, nm, ptr, n))

    def size(self) -> int:
        """RBucket.size = STRLEN"""
        nm, _keep = L.name_struct(self._name)
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_size(self._client.ctx, nm, C.byref(out)))
        return int(out.value) // 8

    def delete(self) -> bool:
        arr, _keep = L.names_array([self._name])
        n = C.c_int()
        _check(L.lib().rbx_del_n(self._client.ctx, arr, 1, C.byref(n)))
        return n.value > 0

    def isExists(self) -> bool:
        arr, _keep = L.names_array([self._name])
        n = C.c_int()
        _check(L.lib().rbx_exists_n(self._client.ctx, arr, 1, C.byref(n)))
        return n.value > 0

    def getOutputStream(self) -> "_BinaryOutputStream":
        return _BinaryOutputStream(self)

    def getInputStream(self) -> "_BinaryInputStream":
        return _BinaryInputStream(self)

    def getChannel(self) -> "_BinaryChannel":
        return _BinaryChannel(self)

    get_name = getName
    is_exists = isExists
    get_output_stream = getOutputStream
    get_input_stream = getInputStream
    get_channel = getChannel


class _BinaryOutputStream:
    """RedissonOutputStream :44-65: write = APPEND"""

    def __init__(self, owner: RBinaryStream):
        self._o = owner

    def write(self, data: bytes) -> None:
        string_append(self._o._client, self._o._name, data)


class _BinaryInputStream:
    """RedissonInputStream :67-140: read = GETRANGE index index+len-1"""

    def __init__(self, owner: RBinaryStream):
        self._o = owner
        self.index = 0

    def skip(self, n: int) -> int:
        """:86-98"""
        if n <= 0:
            return 0
        old = self.index
        self.index = min(self._o.size(), self.index + int(n))
        return self.index - old

    def available(self) -> int:
        """:103-105"""
        return self._o.size() - self.index

    def read(self, n: int):
        """:118-137 -- up to n bytes, or -1 at the end; the index advances by the REQUESTED length (:132)"""
        if n < 0:
            raise IndexError("len < 0")
        if n == 0:
            return b""
        data = string_getrange(self._o._client, self._o._name, self.index, self.index + int(n) - 1)
        if not data:
            return -1
        self.index += int(n)
        return data


class _BinaryChannel:
    """RedissonByteChannel :142-201: read = GETRANGE, write = SETRANGE at the position, truncate = the script"""

    def __init__(self, owner: RBinaryStream):
        self._o = owner
        self._position = 0

    def read(self, n: int):
        """:147-156 -- up to n bytes, or -1 on the empty reply; the position advances by the bytes received (:150).
        n = 0 reads nothing: GETRANGE p p-1 would be GETRANGE 0 -1 at position 0, the whole string, which the
        reference's empty buffer could not take either (the input stream's guard, :121-123)."""
        if n <= 0:
            return b""
        data = string_getrange(self._o._client, self._o._name, self._position, self._position + int(n) - 1)
        if not data:
            return -1
        self._position += len(data)
        return data

    def write(self, data: bytes) -> int:
        """:159-165"""
        string_setrange(self._o._client, self._o._name, self._position, data)
        self._position += len(data)
        return len(data)

    def position(self, newPosition: int | None = None):
        """:168-176 -- position() reads it, position(p) sets it and returns the channel"""
        if newPosition is None:
            return self._position
        self._position = int(newPosition)
        return self

    def size(self) -> int:
        return self._o.size()

    def truncate(self, size: int) -> "_BinaryChannel":
        """:184-195"""
        string_truncate(self._o._client, self._o._name, size)
        return self


def bitset_stream_call(client: RedissonClient, names, cmd_key, cmd_op, cmd_index, replies: bool = True):
    """rbx_bitset_stream over host arrays without raising: (rc, message, replies).  names: str or bytes keys;
    replies is a uint8 array (0xFF = that command failed alone) or None when not asked for."""
    key = np.ascontiguousarray(cmd_key, dtype=np.uint32).reshape(-1)
    op = np.ascontiguousarray(cmd_op, dtype=np.uint8).reshape(-1)
    idx = np.ascontiguousarray(cmd_index, dtype=np.uint64).reshape(-1)
    if not key.size == op.size == idx.size:
        raise IllegalArgumentException("cmd_key, cmd_op and cmd_index have one entry per command")
    arr, _keep = L.names_array(names)
    out = np.zeros(max(key.size, 1), np.uint8) if replies else None
    rc = L.lib().rbx_bitset_stream(client.ctx, arr, len(names), key.ctypes.data_as(L.u32p), op.ctypes.data_as(L.u8p),
                                   idx.ctypes.data_as(L.u64p), key.size, out.ctypes.data_as(L.u8p) if replies else None)
    return rc, (L.last_error() if rc != L.RBX_OK else ""), (out[: key.size] if replies else None)


def bitset_stream(client: RedissonClient, names, cmd_key, cmd_op, cmd_index, replies: bool = True):
    """An ordered stream of GETBIT (0) / SETBIT 0 (1) / SETBIT 1 (2) commands over many keys in one call
    (rbx_bitset_stream): the replies, in order.  Raises the first failing command's exception after every
    other command has run."""
    rc, msg, out = bitset_stream_call(client, names, cmd_key, cmd_op, cmd_index, replies)
    raise_for(rc, msg)
    return out


def bitset_stream_dev(client: RedissonClient, names, d_cmd_key: int, d_cmd_op: int, d_cmd_index: int, n: int,
                      d_replies: int | None = None, stream: int | None = None) -> None:
    """bitset_stream over device arrays (u32 keys, u8 ops, u64 indexes, u8 replies), enqueued on `stream`."""
    arr, _keep = L.names_array(names)
    _check(L.lib().rbx_bitset_stream_dev(client.ctx, arr, len(names), d_cmd_key, d_cmd_op, d_cmd_index, int(n),
                                         d_replies, stream))


FIELD_FAILED = 0xFF  # status of a field-stream command that failed alone; 1 = nil (OVERFLOW FAIL)
_FIELD_TYPE_MSG = "ERR Invalid bitfield type. Use something like i16 u8. Note that u64 is not supported but i64 is."


def _field_cmds_array(cmds):
    """rows of (op, signed, size, overflow, offset, value) -> an array of rbx_field_cmd"""
    arr = (L.RbxFieldCmd * max(len(cmds), 1))()
    for a, (op, signed, size, overflow, offset, value) in zip(arr, cmds):
        a.op, a.is_signed, a.size, a.overflow, a.offset, a.value = op, int(signed), size, overflow, offset, value
    return arr


def bitset_field_stream_call(client: RedissonClient, names, cmd_key, cmds, replies: bool = True):
    """rbx_bitset_field_stream over host arrays without raising: (rc, message, replies, status).  cmds: rows of
    (op, signed, size, overflow, offset, value) with RBX_FIELD_* / RBX_OVERFLOW_* codes, or an array of
    RbxFieldCmd.  replies: int64; status: uint8 with 0 = valid, 1 = nil, 0xFF = that command failed alone."""
    key = np.ascontiguousarray(cmd_key, dtype=np.uint32).reshape(-1)
    arr = cmds if isinstance(cmds, C.Array) else _field_cmds_array(list(cmds))
    n = key.size
    if len(arr) < n or (not isinstance(cmds, C.Array) and len(cmds) != n):
        raise IllegalArgumentException("cmd_key and cmds have one entry per command")
    names_arr, _keep = L.names_array(names)
    out = np.zeros(max(n, 1), np.int64) if replies else None
    status = np.zeros(max(n, 1), np.uint8)
    rc = L.lib().rbx_bitset_field_stream(client.ctx, names_arr, len(names), key.ctypes.data_as(L.u32p), arr, n,
                                         out.ctypes.data_as(L.i64p) if replies else None, status.ctypes.data_as(L.u8p))
    return rc, (L.last_error() if rc != L.RBX_OK else ""), (out[:n] if replies else None), status[:n]


def bitset_field_stream(client: RedissonClient, names, cmd_key, cmds, replies: bool = True):
    """An ordered stream of single-sub-command BITFIELDs over many keys in one call (rbx_bitset_field_stream):
    (replies, status) in order.  Raises the first failing command's exception after every other command ran."""
    rc, msg, out, status = bitset_field_stream_call(client, names, cmd_key, cmds, replies)
    raise_for(rc, msg)
    return out, status


def bitset_field_stream_dev(client: RedissonClient, names, d_cmd_key: int, d_cmds: int, n: int,
                            d_replies: int | None = None, d_status: int | None = None,
                            stream: int | None = None) -> None:
    """bitset_field_stream over device arrays (u32 keys, 24-byte rbx_field_cmd records, i64 replies, u8 status),
    enqueued on `stream`."""
    arr, _keep = L.names_array(names)
    _check(L.lib().rbx_bitset_field_stream_dev(client.ctx, arr, len(names), d_cmd_key, d_cmds, int(n), d_replies,
                                               d_status, stream))


PFADD, PFCOUNT = L.RBX_HLL_PFADD, L.RBX_HLL_PFCOUNT  # cmd_op of rbx_hll_stream
HLL_FAILED = 0xFF  # status of an HLL-stream command that failed alone
_HLL_WRONGTYPE_MSG = "WRONGTYPE Key is not a valid HyperLogLog string value."


class _HllStreamArrays:
    """the command arrays of one rbx_hll_stream[_dev] call, checked, and the arrays it answers into"""

    def __init__(self, names, cmd_key, cmd_op, seg):
        self.key = np.ascontiguousarray(cmd_key, dtype=np.uint32).reshape(-1)
        self.op = np.ascontiguousarray(cmd_op, dtype=np.uint8).reshape(-1)
        self.offs = np.ascontiguousarray(seg, dtype=np.uint64).reshape(-1)
        self.n = n = self.key.size
        if self.op.size != n or self.offs.size != n + 1:
            raise IllegalArgumentException("cmd_key and cmd_op have one entry per command, seg one more")
        self.names_arr, self._keep = L.names_array(names)
        self.out = np.zeros(max(n, 1), np.uint64)
        self.status = np.zeros(max(n, 1), np.uint8)
        self.commands = (self.names_arr, len(names), self.key.ctypes.data_as(L.u32p), self.op.ctypes.data_as(L.u8p),
                         self.offs.ctypes.data_as(L.u64p), n)
        self.answers = (self.out.ctypes.data_as(L.u64p), self.status.ctypes.data_as(L.u8p))

    def result(self, rc):
        return rc, (L.last_error() if rc != L.RBX_OK else ""), self.out[: self.n], self.status[: self.n]


def hll_stream_call(client: RedissonClient, names, cmd_key, cmd_op, seg, arena):
    """rbx_hll_stream over host arrays without raising: (rc, message, replies, status).  names: str or bytes keys;
    command i is cmd_op[i] (PFADD / PFCOUNT) on names[cmd_key[i]] with the elements [seg[i], seg[i + 1]) of
    `arena` (an Arena, or a list of bytes).  replies: uint64 (1 / 0 for a PFADD, the cardinality for a PFCOUNT);
    status: uint8 with 0 = the command ran, 0xFF = it failed alone."""
    s = _HllStreamArrays(names, cmd_key, cmd_op, seg)
    a = arena if isinstance(arena, (Arena, _OneKey)) else Arena([bytes(e) for e in arena])
    return s.result(L.lib().rbx_hll_stream(client.ctx, *s.commands, a.ptr(), *s.answers))


_engine_hll_stream_call = hll_stream_call  # (RBatch.__init__ has a parameter of that name)


def hll_stream(client: RedissonClient, names, cmd_key, cmd_op, seg, arena):
    """An ordered stream of PFADD (0) / single-key PFCOUNT (1) commands over many keys in one call
    (rbx_hll_stream): (replies, status) in order.  Raises the first failing command's exception after every other
    command has run."""
    rc, msg, out, status = hll_stream_call(client, names, cmd_key, cmd_op, seg, arena)
    raise_for(rc, msg)
    return out, status


def hll_stream_dev_call(client: RedissonClient, names, cmd_key, cmd_op, seg, d_elements: L.RbxKeys,
                        stream: int | None = None):
    """rbx_hll_stream_dev without raising: (rc, message, replies, status) over device-resident elements
    (device_keys); the command arrays stay host arrays."""
    s = _HllStreamArrays(names, cmd_key, cmd_op, seg)
    return s.result(L.lib().rbx_hll_stream_dev(client.ctx, *s.commands, C.byref(d_elements), *s.answers, stream))


def hll_stream_dev(client: RedissonClient, names, cmd_key, cmd_op, seg, d_elements: L.RbxKeys,
                   stream: int | None = None):
    """hll_stream over device-resident elements: (replies, status); raises as hll_stream does."""
    rc, msg, out, status = hll_stream_dev_call(client, names, cmd_key, cmd_op, seg, d_elements, stream)
    raise_for(rc, msg)
    return out, status


class _HllGroupArrays:
    """the CSR arrays of one rbx_hll_count_groups / rbx_hll_merge_groups call: groups = one list of indexes into
    `names` per group"""

    def __init__(self, names, groups):
        groups = [list(g) for g in groups]
        self.n = n = len(groups)
        self.off = np.zeros(n + 1, np.uint64)
        self.off[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64)
        self.key = np.ascontiguousarray([k for g in groups for k in g] or [0], dtype=np.uint32)
        self.names_arr, self._keep = L.names_array(names)
        self.nkeys = len(names)
        self.status = np.zeros(max(n, 1), np.uint8)


def hll_count_groups_call(client: RedissonClient, names, groups):
    """rbx_hll_count_groups without raising: (rc, message, counts, status).  names: str or bytes keys; group g is
    PFCOUNT of names[k] for k in groups[g] (one entry: the single-key count with the header cache; more: the
    union).  counts: uint64; status: uint8 with 0 = the group ran, 0xFF = it failed alone."""
    a = _HllGroupArrays(names, groups)
    out = np.zeros(max(a.n, 1), np.uint64)
    rc = L.lib().rbx_hll_count_groups(client.ctx, a.names_arr, a.nkeys, a.off.ctypes.data_as(L.u64p),
                                      a.key.ctypes.data_as(L.u32p), a.n, out.ctypes.data_as(L.u64p),
                                      a.status.ctypes.data_as(L.u8p))
    return rc, (L.last_error() if rc != L.RBX_OK else ""), out[: a.n], a.status[: a.n]


def hll_merge_groups_call(client: RedissonClient, names, dests, groups):
    """rbx_hll_merge_groups without raising: (rc, message, status).  Group g is PFMERGE names[dests[g]] <names[k]
    for k in groups[g]>, in order: a later group sees what an earlier one wrote."""
    a = _HllGroupArrays(names, groups)
    dest = np.ascontiguousarray(list(dests) or [0], dtype=np.uint32).reshape(-1)
    if len(dests) != a.n:
        raise IllegalArgumentException("dests and groups have one entry per group")
    rc = L.lib().rbx_hll_merge_groups(client.ctx, a.names_arr, a.nkeys, dest.ctypes.data_as(L.u32p),
                                      a.off.ctypes.data_as(L.u64p), a.key.ctypes.data_as(L.u32p), a.n,
                                      a.status.ctypes.data_as(L.u8p))
    return rc, (L.last_error() if rc != L.RBX_OK else ""), a.status[: a.n]


_engine_hll_count_groups_call, _engine_hll_merge_groups_call = hll_count_groups_call, hll_merge_groups_call


def hll_count_groups(client: RedissonClient, names, groups):
    """Many PFCOUNTs, unions among them, in one call (rbx_hll_count_groups): (counts, status) in order.  Raises the
    first failing group's exception after every other group has run."""
    rc, msg, out, status = hll_count_groups_call(client, names, groups)
    raise_for(rc, msg)
    return out, status


def hll_merge_groups(client: RedissonClient, names, dests, groups):
    """Many PFMERGEs in one call, in order (rbx_hll_merge_groups): the status bytes.  Raises the first failing
    group's exception after every other group has run."""
    rc, msg, status = hll_merge_groups_call(client, names, dests, groups)
    raise_for(rc, msg)
    return status


def bitset_op_groups_call(client: RedissonClient, names, ops, dests, groups):
    """rbx_bitset_op_groups without raising: (rc, message, lens, counts, status).  Group g is BITOP ops[g]
    names[dests[g]] <names[k] for k in groups[g]>, in order: a later group sees what an earlier one wrote.  ops:
    RBX_BITOP_* values; dests[g] = None (or RBX_BITGROUP_NO_DEST): the combination is counted and stored nowhere.
    lens: uint64, each result's length; counts: uint64, its one bits; status: uint8 with 0 = the group ran, 0xFF =
    it failed alone."""
    a = _HllGroupArrays(names, groups)
    if len(ops) != a.n or len(dests) != a.n:
        raise IllegalArgumentException("ops, dests and groups have one entry per group")
    op = np.ascontiguousarray(list(ops) or [0], dtype=np.uint8).reshape(-1)
    dest = np.ascontiguousarray([L.RBX_BITGROUP_NO_DEST if d is None else d for d in dests] or [0],
                                dtype=np.uint32).reshape(-1)
    lens, counts = np.zeros(max(a.n, 1), np.uint64), np.zeros(max(a.n, 1), np.uint64)
    rc = L.lib().rbx_bitset_op_groups(client.ctx, a.names_arr, a.nkeys, op.ctypes.data_as(L.u8p),
                                      dest.ctypes.data_as(L.u32p), a.off.ctypes.data_as(L.u64p),
                                      a.key.ctypes.data_as(L.u32p), a.n, lens.ctypes.data_as(L.u64p),
                                      counts.ctypes.data_as(L.u64p), a.status.ctypes.data_as(L.u8p))
    return rc, (L.last_error() if rc != L.RBX_OK else ""), lens[: a.n], counts[: a.n], a.status[: a.n]


_engine_bitset_op_groups_call = bitset_op_groups_call

RANGE_FAILED = 0xFF  # status of a command of rbx_bitset_range_stream that failed alone


def _range_cmds_array(rows):
    """rows of (op, bit, nargs, start, end, unit) -> an array of rbx_range_cmd"""
    arr = (L.RbxRangeCmd * max(len(rows), 1))()
    for a, (op, bit, nargs, start, end, unit) in zip(arr, rows):
        a.op, a.bit, a.nargs, a.start, a.end, a.unit = op, bit, nargs, start, end, unit
    return arr


def bitset_range_stream_call(client: RedissonClient, names, cmd_key, rows):
    """rbx_bitset_range_stream over host arrays without raising: (rc, message, replies, status).  Command i runs on
    names[cmd_key[i]]; rows: (op, bit, nargs, start, end, unit) with RBX_RANGE_* codes, or an array of RbxRangeCmd.
    replies: int64, what the single calls return; status: uint8 with 0 = the command ran, 0xFF = it failed alone."""
    key = np.ascontiguousarray(cmd_key, dtype=np.uint32).reshape(-1)
    arr = rows if isinstance(rows, C.Array) else _range_cmds_array(list(rows))
    n = key.size
    if len(arr) < n or (not isinstance(rows, C.Array) and len(rows) != n):
        raise IllegalArgumentException("cmd_key and rows have one entry per command")
    names_arr, _keep = L.names_array(names)
    out, status = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint8)
    rc = L.lib().rbx_bitset_range_stream(client.ctx, names_arr, len(names), key.ctypes.data_as(L.u32p), arr, n,
                                         out.ctypes.data_as(L.i64p), status.ctypes.data_as(L.u8p))
    return rc, (L.last_error() if rc != L.RBX_OK else ""), out[:n], status[:n]


def bitset_range_stream(client: RedissonClient, names, cmd_key, rows):
    """BITCOUNT / BITPOS / STRLEN / length() commands over many keys in one call (rbx_bitset_range_stream):
    (replies, status) in order.  Raises the first failing command's exception after every other command ran."""
    rc, msg, out, status = bitset_range_stream_call(client, names, cmd_key, rows)
    raise_for(rc, msg)
    return out, status


def bitset_range_stream_dev(client: RedissonClient, names, d_cmd_key: int, d_cmds: int, n: int,
                            d_replies: int | None = None, d_status: int | None = None,
                            stream: int | None = None) -> None:
    """bitset_range_stream over device arrays (u32 keys, 24-byte rbx_range_cmd records, i64 replies, u8 status),
    enqueued on `stream`."""
    arr, _keep = L.names_array(names)
    _check(L.lib().rbx_bitset_range_stream_dev(client.ctx, arr, len(names), d_cmd_key, d_cmds, int(n), d_replies,
                                               d_status, stream))


_engine_bitset_range_stream_call = bitset_range_stream_call


def _members_cmds_array(rows):
    """rows of (nargs, start, end, unit, skip, limit) -> an array of rbx_members_cmd; limit None = all"""
    arr = (L.RbxMembersCmd * max(len(rows), 1))()
    for a, (nargs, start, end, unit, skip, limit) in zip(arr, rows):
        a.nargs, a.start, a.end, a.unit, a.skip = nargs, start, end, unit, skip
        a.limit = (1 << 64) - 1 if limit is None else limit
    return arr


def bitset_members_stream_call(client: RedissonClient, names, cmd_key, rows, cap: int | None = None):
    """rbx_bitset_members_stream over host arrays without raising: (rc, message, off, out, status).  Command i runs on
    names[cmd_key[i]]; rows: (nargs, start, end, unit, skip, limit) with RBX_RANGE_* units, or an array of
    RbxMembersCmd.  off: n + 1 uint64, exact whatever cap is; out: the first min(off[n], cap) positions of the
    concatenation (cap None: all of them -- one counting call, then one with room for the total); status: uint8, 0xFF =
    the command failed alone and yields nothing."""
    key = np.ascontiguousarray(cmd_key, dtype=np.uint32).reshape(-1)
    arr = rows if isinstance(rows, C.Array) else _members_cmds_array(list(rows))
    n = key.size
    if len(arr) < n or (not isinstance(rows, C.Array) and len(rows) != n):
        raise IllegalArgumentException("cmd_key and rows have one entry per command")
    names_arr, _keep = L.names_array(names)
    off, status, total = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8), C.c_uint64()

    def call(room, out):
        return L.lib().rbx_bitset_members_stream(client.ctx, names_arr, len(names), key.ctypes.data_as(L.u32p), arr, n, room,
                                                 off.ctypes.data_as(L.u64p),
                                                 None if out is None else out.ctypes.data_as(L.u64p),
                                                 status.ctypes.data_as(L.u8p), C.byref(total))

    out = None
    rc = call(0, None) if cap is None else L.RBX_OK
    if rc in (L.RBX_OK, L.RBX_E_WRONGTYPE):
        room = int(total.value) if cap is None else int(cap)
        if room or cap is not None:
            out = np.zeros(max(room, 1), np.uint64)
            rc = call(room, out)
    msg = L.last_error() if rc != L.RBX_OK else ""
    got = min(int(total.value), 0 if out is None else out.size)
    return rc, msg, off, (np.zeros(0, np.uint64) if out is None else out[:got]), status[:n]


def bitset_members_stream(client: RedissonClient, names, cmd_key, rows, cap: int | None = None):
    """The members of many keys in one call (rbx_bitset_members_stream): (off, out, status); command i's positions are
    out[off[i]: off[i + 1]].  Raises the first failing command's exception after every other command ran."""
    rc, msg, off, out, status = bitset_members_stream_call(client, names, cmd_key, rows, cap)
    raise_for(rc, msg)
    return off, out, status


def bitset_members_stream_dev(client: RedissonClient, names, d_cmd_key: int, d_cmds: int, n: int, cap: int, d_off: int,
                              d_out: int | None = None, d_status: int | None = None, stream: int | None = None) -> None:
    """bitset_members_stream over device arrays (u32 keys, 40-byte rbx_members_cmd records, n + 1 u64 offsets, cap u64
    positions, u8 status), enqueued on `stream`."""
    arr, _keep = L.names_array(names)
    _check(L.lib().rbx_bitset_members_stream_dev(client.ctx, arr, len(names), d_cmd_key, d_cmds, int(n), int(cap), d_off,
                                                 d_out, d_status, stream))


_engine_bitset_members_stream_call = bitset_members_stream_call


# ---- the byte-level string commands (rbx_string_*, include/rbx.h "Redis string commands on the same keys") ----
STRING_NIL, STRING_FAILED = 1, 0xFF  # status of a command of rbx_string_stream: GET on a missing key, failed alone
_STRING_OFFSET_MSG = "ERR offset is out of range"
_STRING_SIZE_MSG = "ERR string exceeds maximum allowed size (proto-max-bulk-len)"


def _u8(data):
    """(u8 pointer or None, length, keep-alive) of a bytes-like value"""
    b = bytes(data)
    buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")
    return (buf if b else None), len(b), buf


def string_getrange(client: RedissonClient, name, start: int, end: int) -> bytes:
    """GETRANGE name start end (rbx_string_getrange): a second call only when the first buffer was too small"""
    nm, _keep = L.name_struct(name)
    n, cap = C.c_uint64(), 4096
    while True:
        buf = (C.c_uint8 * cap)()
        _check(L.lib().rbx_string_getrange(client.ctx, nm, int(start), int(end), buf, cap, C.byref(n)))
        if n.value <= cap:
            return bytes(buf[:n.value])
        cap = n.value


def string_setrange(client: RedissonClient, name, offset: int, value) -> int:
    """SETRANGE name offset value -> the new length (rbx_string_setrange)"""
    nm, _keep = L.name_struct(name)
    ptr, n, _buf = _u8(value)
    out = C.c_uint64()
    _check(L.lib().rbx_string_setrange(client.ctx, nm, int(offset), ptr, n, C.byref(out)))
    return int(out.value)


def string_append(client: RedissonClient, name, value) -> int:
    """APPEND name value -> the new length (rbx_string_append)"""
    nm, _keep = L.name_struct(name)
    ptr, n, _buf = _u8(value)
    out = C.c_uint64()
    _check(L.lib().rbx_string_append(client.ctx, nm, ptr, n, C.byref(out)))
    return int(out.value)


def string_truncate(client: RedissonClient, name, size: int) -> None:
    """the script of RBinaryStream's channel truncate (rbx_string_truncate)"""
    nm, _keep = L.name_struct(name)
    _check(L.lib().rbx_string_truncate(client.ctx, nm, int(size)))


def _string_cmds(rows):
    """rows of (op, a, b, value bytes) -> (an array of rbx_string_cmd, the value buffer)"""
    arr = (L.RbxStringCmd * max(len(rows), 1))()
    vals = bytearray()
    for c, (op, a, b, value) in zip(arr, rows):
        c.op, c.a, c.b, c.val_off, c.val_len = op, a, b, len(vals), len(value)
        vals += value
    return arr, bytes(vals)


def string_stream_call(client: RedissonClient, names, cmd_key, rows, cap: int | None = None):
    """rbx_string_stream over host arrays without raising: (rc, message, replies, status, off, out).  Command i runs on
    names[cmd_key[i]]; rows: (op, a, b, value) with RBX_STR_* codes -- GETRANGE start, end; SETRANGE offset in a.
    replies: int64, the new length of a write and the byte count of a read; status: 0, 1 (GET on a missing key: nil) or
    0xFF (failed alone); read i's bytes are out[off[i]:off[i + 1]].  cap None: the reads' bytes are asked for again
    with the exact size when they do not fit a first guess (such a call is refused before any write)."""
    key = np.ascontiguousarray(cmd_key, dtype=np.uint32).reshape(-1)
    rows = list(rows)
    n = key.size
    if len(rows) != n:
        raise IllegalArgumentException("cmd_key and rows have one entry per command")
    arr, vals = _string_cmds(rows)
    vptr, vlen, _vbuf = _u8(vals)
    names_arr, _keep = L.names_array(names)
    replies, status = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint8)
    off, total = np.zeros(n + 1, np.uint64), C.c_uint64()
    room = 65536 if cap is None else int(cap)
    while True:
        out = np.zeros(max(room, 1), np.uint8)
        rc = L.lib().rbx_string_stream(client.ctx, names_arr, len(names), key.ctypes.data_as(L.u32p), arr, n, vptr, vlen,
                                       room, off.ctypes.data_as(L.u64p), out.ctypes.data_as(L.u8p) if room else None,
                                       replies.ctypes.data_as(L.i64p), status.ctypes.data_as(L.u8p), C.byref(total))
        if cap is None and rc == L.RBX_E_ILLEGAL_ARGUMENT and total.value > room:
            room = total.value
            continue
        break
    return rc, (L.last_error() if rc != L.RBX_OK else ""), replies[:n], status[:n], off, out[:min(total.value, room)].tobytes()


def string_stream(client: RedissonClient, names, cmd_key, rows, cap: int | None = None):
    """GETRANGE / SETRANGE / APPEND / GET commands over many keys in one call (rbx_string_stream): (replies, status,
    off, out).  Raises the first failing command's exception after every other command ran."""
    rc, msg, replies, status, off, out = string_stream_call(client, names, cmd_key, rows, cap)
    raise_for(rc, msg)
    return replies, status, off, out


def string_stream_dev(client: RedissonClient, names, d_cmd_key: int, d_cmds: int, n: int, d_vals: int | None, vals_len: int,
                      cap: int, d_off: int, d_out: int | None, d_replies: int | None = None, d_status: int | None = None,
                      stream: int | None = None) -> int:
    """string_stream over device arrays (u32 keys, 32-byte rbx_string_cmd records, the value bytes, n + 1 u64 offsets,
    the reads' bytes, i64 replies, u8 status), enqueued on `stream`.  Returns the reads' total bytes."""
    arr, _keep = L.names_array(names)
    total = C.c_uint64()
    _check(L.lib().rbx_string_stream_dev(client.ctx, arr, len(names), d_cmd_key, d_cmds, int(n), d_vals, int(vals_len),
                                         int(cap), d_off, d_out, d_replies, d_status, C.byref(total), stream))
    return int(total.value)


def string_failure(client: RedissonClient, name, row) -> RedissonAmdError:
    """what a string command that failed alone failed with, in the order of the single calls: SETRANGE's offset, the
    key's type -- which a command that failed did not change, so a STRLEN tells it now --, else the size"""
    op, a, _b, _value = row
    if op == L.RBX_STR_SETRANGE and a < 0:
        return RedisException(_STRING_OFFSET_MSG)
    nm, _keep = L.name_struct(name)
    out = C.c_uint64()
    if L.lib().rbx_bitset_size(client.ctx, nm, C.byref(out)) == L.RBX_E_WRONGTYPE:
        return RedisException(_WRONGTYPE_MSG)
    return RedisException(_STRING_SIZE_MSG)


class BatchFuture:
    """What a queued command returns: get() is its reply once the batch has executed (RFuture of the *Async
    methods), or raises what the command failed with."""

    def __init__(self):
        self._done, self._value, self._error = False, None, None

    def _set(self, value=None, error=None) -> None:
        self._done, self._value, self._error = True, value, error

    def isDone(self) -> bool:
        return self._done

    def get(self):
        if not self._done:
            raise IllegalStateException("the batch has not been executed")
        if self._error is not None:
            raise self._error
        return self._value

    is_done = isDone


class _Queued:
    """One queued command: a bit command (name, op, index) that coalesces, a field command (name, field =
    (op, signed, size, overflow, offset, value), fn) that coalesces where a field stream call is at hand and
    runs through fn otherwise, an HLL command (name, hll = (PFADD, [element bytes]) or (PFCOUNT, []), fn) that
    coalesces where an HLL stream call is at hand and runs through fn otherwise, a grouped HLL command (group =
    ("count", [names]) for a multi-key PFCOUNT or ("merge", dest, [sources]) for a PFMERGE, fn) that coalesces with
    its like where the grouped call is at hand and runs through fn otherwise, a BITOP or whole-string BITCOUNT
    (bitop = (RBX_BITOP_*, destination or None, [sources]), fn; convert(length, count) is its reply) that coalesces
    with its like where the grouped bit call is at hand and runs through fn otherwise, or a callable that runs
    singly.  A read query (range = (RBX_RANGE_*, bit, nargs, start, end, unit), fn; convert(reply) is its reply)
    coalesces with its like where the range stream call is at hand and runs through fn otherwise; a whole-string
    BITCOUNT carries both a bitop and a range row.  An enumeration (members = (nargs, start, end, unit, skip,
    limit), fn) coalesces with its like where the members stream call is at hand and runs through fn otherwise.
    A byte-level string command (string = (RBX_STR_*, a, b, value bytes), fn; convert(number, bytes, status) is its
    reply) coalesces with its like where the string stream call is at hand and runs through fn otherwise.
    convert: applied to a field or HLL command's reply."""

    __slots__ = ("name", "op", "index", "fn", "future", "field", "convert", "hll", "group", "bitop", "range", "members",
                 "string")

    def __init__(self, name=None, op=None, index=0, fn=None, field=None, convert=None, hll=None, group=None,
                 bitop=None, range=None, members=None, string=None):  # noqa: A002
        self.name, self.op, self.index, self.fn, self.future = name, op, index, fn, BatchFuture()
        self.field, self.convert, self.hll, self.group, self.bitop = field, convert, hll, group, bitop
        self.range, self.members, self.string = range, members, string

    def as_field(self):
        """the command as a BITFIELD sub-command: GETBIT / SETBIT are GET / SET of a u1, which leave the same
        string and the same growth"""
        if self.field is not None:
            return self.field
        if self.op == GETBIT:
            return (L.RBX_FIELD_GET, 0, 1, L.RBX_OVERFLOW_WRAP, self.index, 0)
        return (L.RBX_FIELD_SET, 0, 1, L.RBX_OVERFLOW_WRAP, self.index, 1 if self.op == SETBIT1 else 0)


def _bit_index(index) -> int:
    i = int(index)
    if i < 0:
        raise IllegalArgumentException("bit indexes are non-negative integers")
    return min(i, (1 << 64) - 1)  # past the offset limit either way


def _bit_error(q: _Queued) -> RedissonAmdError:
    """what a bit command that failed alone failed with: the offset is checked first, as in the single calls"""
    if q.index >= _BIT_OFFSET_LIMIT:
        return RedisException("ERR bit offset is not an integer or out of range")
    return RedisException("WRONGTYPE Operation against a key holding the wrong kind of value")


def _field_error(q: _Queued) -> RedissonAmdError:
    """what a field command that failed alone failed with: the type, the offset limit, the key's type, in the
    order of the single call"""
    _op, signed, size, _mode, offset, _value = q.field
    if size < 1 or size > (64 if signed else 63):
        return RedisException(_FIELD_TYPE_MSG)
    if offset >= _BIT_OFFSET_LIMIT or offset + size > _BIT_OFFSET_LIMIT:
        return RedisException("ERR bit offset is not an integer or out of range")
    return RedisException("WRONGTYPE Operation against a key holding the wrong kind of value")


def _run_stream(run, call, accepted_rcs, settle):
    """One stream call for a run of coalesced commands: call(run, names, cmd_key) -> (rc, message, replies, status)
    over the run's distinct names and each command's place among them.  An rc outside accepted_rcs refuses the run as a
    whole, and every future gets that error; otherwise settle(command, reply, status) sets each command's future.
    Returns the first error."""
    ids: dict = {}
    keys = [ids.setdefault(c.name, len(ids)) for c in run]
    rc, msg, replies, status = call(run, list(ids), keys)
    if rc not in accepted_rcs:
        try:
            raise_for(rc, msg)
        except RedissonAmdError as e:
            for c in run:
                c.future._set(error=e)
            return e
    first_error = None
    for c, r, s in zip(run, replies, status):
        settle(c, r, s)
        first_error = first_error or c.future._error
    return first_error


def _settle_bit(c: _Queued, reply, _status) -> None:
    """a bit command of a bit run: the reply is its own status"""
    if int(reply) == _FAILED_REPLY:
        c.future._set(error=_bit_error(c))
    else:
        c.future._set(bool(reply))


def _settle_field(c: _Queued, reply, status) -> None:
    """a bit or field command of a field run"""
    if int(status) == FIELD_FAILED:
        c.future._set(error=_bit_error(c) if c.field is None else _field_error(c))
    elif c.field is None:
        c.future._set(bool(reply))
    else:
        value = None if int(status) == 1 else int(reply)  # nil
        c.future._set(c.convert(value) if c.convert else value)


def _settle_hll(c: _Queued, reply, status) -> None:
    if int(status) == HLL_FAILED:
        c.future._set(error=RedisException(_HLL_WRONGTYPE_MSG))
    else:
        value = bool(reply) if c.hll[0] == PFADD else int(reply)
        c.future._set(c.convert(value) if c.convert else value)


def _settle_group(c: _Queued, reply, status) -> None:
    """a multi-key PFCOUNT (the cardinality) or a PFMERGE (None) of a grouped run"""
    if int(status) == HLL_FAILED:
        c.future._set(error=RedisException(_HLL_WRONGTYPE_MSG))
    else:
        value = int(reply) if c.group[0] == "count" else None
        c.future._set(c.convert(value) if c.convert else value)


BITGROUP_FAILED = 0xFF  # status of a group of rbx_bitset_op_groups that failed alone
_BITOP_NOT_MSG = "ERR BITOP NOT must be called with a single source key."


def _settle_bitop(c: _Queued, reply, status) -> None:
    """a BITOP or whole-string BITCOUNT of a grouped bit run; reply = (length, count)"""
    if int(status) == BITGROUP_FAILED:
        op, _dest, sources = c.bitop
        c.future._set(error=RedisException(_BITOP_NOT_MSG if op == L.RBX_BITOP_NOT and len(sources) != 1
                                           else "WRONGTYPE Operation against a key holding the wrong kind of value"))
    else:
        c.future._set(c.convert(int(reply[0]), int(reply[1])))


_RANGE_BIT_MSG = "ERR The bit argument must be 1 or 0."
_WRONGTYPE_MSG = "WRONGTYPE Operation against a key holding the wrong kind of value"


def _range_row(op: int, bit: int = 0, nargs: int = 0, start: int = 0, end: int = 0, unit: int = L.RBX_RANGE_BYTE):
    """one row of bitset_range_stream_call; a bit outside a byte is as wrong as 2"""
    return (op, bit if 0 <= bit <= 255 else 2, nargs, start, end, unit)


def _settle_range(c: _Queued, reply, status) -> None:
    """a read query of a range run; a failure is worked out in the order of the single calls: BITPOS's bit, its
    unit without an end, then the key's type.  A failed length() has either the wrong type or a failing script,
    which the status does not tell apart: its own call, which only reads, says which."""
    if int(status) != RANGE_FAILED:
        # a whole-string BITCOUNT keeps the converter of its bitop row: convert(length, count)
        c.future._set(c.convert(0, int(reply)) if c.bitop is not None else
                      c.convert(int(reply)) if c.convert else int(reply))
        return
    op, bit, nargs, _start, _end, unit = c.range
    if op == L.RBX_RANGE_POS and bit > 1:
        msg = _RANGE_BIT_MSG
    elif op == L.RBX_RANGE_POS and nargs < 2 and unit == L.RBX_RANGE_BIT:
        msg = "ERR syntax error"
    elif op == L.RBX_RANGE_LENGTH:
        try:
            c.future._set(c.fn())
        except RedissonAmdError as e:
            c.future._set(error=e)
        return
    else:
        msg = _WRONGTYPE_MSG
    c.future._set(error=RedisException(msg))


MEMBERS_FAILED = 0xFF  # status of a command of rbx_bitset_members_stream that failed alone


def _settle_members(c: _Queued, reply, status) -> None:
    """an enumeration of a members run: its slice of the positions"""
    if int(status) == MEMBERS_FAILED:
        c.future._set(error=RedisException(_WRONGTYPE_MSG))
    else:
        c.future._set(reply)


def _settle_string(c: _Queued, reply, status) -> None:
    """a byte-level string command of a string run; reply = (number, bytes, the error of a failed command)"""
    if int(status) == STRING_FAILED:
        c.future._set(error=reply[2])
    else:
        c.future._set(c.convert(int(reply[0]), reply[1], int(status)) if c.convert else int(reply[0]))


def run_queue(queue, stream_call, field_stream_call=None, hll_stream_call=None, hll_count_groups_call=None,
              hll_merge_groups_call=None, bit_groups_call=None, range_stream_call=None, members_stream_call=None,
              string_stream_call=None, string_failure=None):
    """Executes queued commands in submission order.  Every maximal run of consecutive bit commands, over any
    keys, is ONE stream_call(names, cmd_key, cmd_op, cmd_index) -> (rc, message, replies).  With a
    field_stream_call, field commands join the runs, and a run that holds at least one of them is ONE
    field_stream_call(names, cmd_key, cmds) -> (rc, message, replies, status) in which the bit commands travel as
    u1 GET / SET.  With an hll_stream_call, every maximal run of consecutive PFADD / single-key PFCOUNT commands,
    over any keys, is ONE hll_stream_call(names, cmd_key, cmd_op, seg, elements) -> (rc, message, replies,
    status); bit and field runs and HLL runs never mix, and each closes the other.  With an hll_count_groups_call,
    every maximal run of consecutive multi-key PFCOUNTs, over any keys, is ONE hll_count_groups_call(names, groups)
    -> (rc, message, counts, status); with an hll_merge_groups_call, every maximal run of consecutive PFMERGEs is
    ONE hll_merge_groups_call(names, dests, groups) -> (rc, message, status).  With a bit_groups_call, every maximal
    run of consecutive BITOPs and whole-string BITCOUNTs, over any keys, is ONE bit_groups_call(names, ops, dests,
    groups) -> (rc, message, lens, counts, status), a BITCOUNT travelling as a one-source OR without a destination.
    With a range_stream_call, every maximal run of consecutive read queries (ranged and whole-string BITCOUNT,
    BITPOS, STRLEN, length()), over any keys, is ONE range_stream_call(names, cmd_key, rows) -> (rc, message,
    replies, status); a whole-string BITCOUNT joins an open range run and otherwise starts a grouped bit run as
    before.  With a members_stream_call, every maximal run of consecutive enumerations (membersAsync), over any
    keys, is ONE members_stream_call(names, cmd_key, rows) -> (rc, message, off, out, status).  With a
    string_stream_call, every maximal run of consecutive GETRANGE / SETRANGE / APPEND / GET commands, over any keys, is
    ONE string_stream_call(names, cmd_key, rows) -> (rc, message, replies, status, off, out); string_failure(name, row)
    names the error of a command of it that failed alone.  A count run, a merge run, an HLL stream run, a grouped bit
    run, a range run, a members run, a string run and a bit / field run each close the others.
    Every other command runs through its own call at its position.  Each command's future is set; returns
    (responses, first error)."""
    def joins(q):
        return q.op is not None or (q.field is not None and field_stream_call is not None)

    def joins_hll(q):
        return q.hll is not None and hll_stream_call is not None

    def joins_counts(q):
        return q.group is not None and q.group[0] == "count" and hll_count_groups_call is not None

    def joins_merges(q):
        return q.group is not None and q.group[0] == "merge" and hll_merge_groups_call is not None

    def joins_bitops(q):
        return q.bitop is not None and bit_groups_call is not None

    def joins_ranges(q):
        return q.range is not None and range_stream_call is not None

    def joins_members(q):
        return q.members is not None and members_stream_call is not None

    def members_call(run, names, keys):
        rc, msg, off, out, status = members_stream_call(names, keys, [c.members for c in run])
        return rc, msg, [out[int(off[i]): int(off[i + 1])] for i in range(len(run))], status

    def joins_strings(q):
        return q.string is not None and string_stream_call is not None

    def strings_call(run, names, keys):
        rc, msg, replies, status, off, out = string_stream_call(names, keys, [c.string for c in run])
        if rc not in alone:
            return rc, msg, None, None
        rows = [(int(replies[i]), out[int(off[i]): int(off[i + 1])],
                 string_failure(c.name, c.string) if int(status[i]) == STRING_FAILED else None) for i, c in enumerate(run)]
        return rc, msg, rows, status

    def starts_ranges(q):  # a whole-string BITCOUNT starts a grouped bit run where that call is at hand
        return joins_ranges(q) and not joins_bitops(q)

    def run_from(i, belongs):
        """the maximal run of commands from queue[i] on that belong together"""
        j = i
        while j < len(queue) and belongs(queue[j]):
            j += 1
        return queue[i:j]

    def hll_call(run, names, keys):
        seg, elements = [0], []
        for c in run:
            elements.extend(c.hll[1])
            seg.append(len(elements))
        return hll_stream_call(names, keys, [c.hll[0] for c in run], seg, elements)

    def counts_call(run, _names, _keys):
        ids: dict = {}
        groups = [[ids.setdefault(n, len(ids)) for n in c.group[1]] for c in run]
        return hll_count_groups_call(list(ids), groups)

    def merges_call(run, _names, _keys):
        ids: dict = {}
        dests = [ids.setdefault(c.group[1], len(ids)) for c in run]
        groups = [[ids.setdefault(n, len(ids)) for n in c.group[2]] for c in run]
        rc, msg, status = hll_merge_groups_call(list(ids), dests, groups)
        return rc, msg, [None] * len(status), status

    def bitops_call(run, _names, _keys):
        ids: dict = {}
        dests = [None if c.bitop[1] is None else ids.setdefault(c.bitop[1], len(ids)) for c in run]
        groups = [[ids.setdefault(n, len(ids)) for n in c.bitop[2]] for c in run]
        rc, msg, lens, counts, status = bit_groups_call(list(ids), [c.bitop[0] for c in run], dests, groups)
        return rc, msg, list(zip(lens, counts)), status

    def ranges_call(run, names, keys):
        return range_stream_call(names, keys, [c.range for c in run])

    def field_call(run, names, keys):
        return field_stream_call(names, keys, [c.as_field() for c in run])

    def bit_call(run, names, keys):
        rc, msg, replies = stream_call(names, keys, [c.op for c in run], [c.index for c in run])
        return rc, msg, replies, replies

    alone = (L.RBX_OK, L.RBX_E_REDIS, L.RBX_E_WRONGTYPE)  # what a run returns whose commands ran or failed alone
    first_error = None
    i = 0
    while i < len(queue):  # (every run executes, whether or not an earlier command failed)
        if joins_hll(queue[i]):
            run = run_from(i, joins_hll)
            error = _run_stream(run, hll_call, (L.RBX_OK, L.RBX_E_WRONGTYPE), _settle_hll)
        elif joins_counts(queue[i]):
            run = run_from(i, joins_counts)
            error = _run_stream(run, counts_call, (L.RBX_OK, L.RBX_E_WRONGTYPE), _settle_group)
        elif joins_merges(queue[i]):
            run = run_from(i, joins_merges)
            error = _run_stream(run, merges_call, (L.RBX_OK, L.RBX_E_WRONGTYPE), _settle_group)
        elif starts_ranges(queue[i]):
            run = run_from(i, joins_ranges)
            error = _run_stream(run, ranges_call, alone, _settle_range)
        elif joins_members(queue[i]):
            run = run_from(i, joins_members)
            error = _run_stream(run, members_call, (L.RBX_OK, L.RBX_E_WRONGTYPE), _settle_members)
        elif joins_strings(queue[i]):
            run = run_from(i, joins_strings)
            error = _run_stream(run, strings_call, alone, _settle_string)
        elif joins_bitops(queue[i]):
            run = run_from(i, joins_bitops)
            error = _run_stream(run, bitops_call, alone, _settle_bitop)
        elif joins(queue[i]):
            run = run_from(i, joins)
            if any(c.field is not None for c in run):
                error = _run_stream(run, field_call, alone, _settle_field)
            else:
                error = _run_stream(run, bit_call, alone, _settle_bit)
        else:
            run = queue[i:i + 1]
            try:
                run[0].future._set(run[0].fn())
            except RedissonAmdError as e:
                run[0].future._set(error=e)
            error = run[0].future._error
        first_error = first_error or error
        i += len(run)
    return [None if c.future._error is not None else c.future._value for c in queue], first_error


class BatchResult:
    """M/api/BatchResult.java: the replies in submission order"""

    def __init__(self, responses: list):
        self._responses = responses

    def getResponses(self) -> list:
        """:41"""
        return self._responses

    get_responses = getResponses


class RBatchBitSet:
    """RBatch.getBitSet(name) (M/RedissonBatch.java:182-184): RBitSetAsync, every method queued.  get / set /
    clearBit and the typed-field methods of consecutive commands travel together (one rbx_bitset_stream call,
    or one rbx_bitset_field_stream call when a field command is among them); so do consecutive or / and / xor /
    not / cardinality commands (one rbx_bitset_op_groups call, in order); the others run through RBitSet's own
    call."""

    def __init__(self, batch: "RBatch", name: str):
        self._batch, self._name = batch, name

    def _single(self, method: str, *args) -> BatchFuture:
        bitset = self._batch._bitset(self._name)
        return self._batch._add(_Queued(fn=lambda: getattr(bitset, method)(*args)))

    def getAsync(self, bitIndex: int) -> BatchFuture:
        return self._batch._add(_Queued(self._name, GETBIT, _bit_index(bitIndex)))

    def setAsync(self, bitIndex: int, value: bool = True) -> BatchFuture:
        return self._batch._add(_Queued(self._name, SETBIT1 if value else SETBIT0, _bit_index(bitIndex)))

    def clearBitAsync(self, bitIndex: int) -> BatchFuture:
        return self.setAsync(bitIndex, False)

    # ---- typed fields (M/api/RBitSetAsync.java:36-206): one BITFIELD sub-command each, travelling together --
    def _field(self, method: str, op: int, signed: bool, size: int, offset: int, value: int = 0,
               bits: int = 64) -> BatchFuture:
        """Queues `method`'s BITFIELD.  Redisson's own argument checks fire now, as in the synchronous methods
        (M/RedissonBitSet.java:72-73, :99-100); what Redis checks fails the command when the batch runs."""
        size = RBitSet._java(size, 32, "size")
        if size > (64 if signed else 63):
            raise IllegalArgumentException(f"Size can't be greater than {64 if signed else 63} bits")
        off = RBitSet._java(offset, 64, "offset") & 0xFFFFFFFFFFFFFFFF  # a negative long is past the limit too
        value = RBitSet._java(RBitSet._java(value, bits, "value"), 64, "value")
        args = (offset,) if op == L.RBX_FIELD_GET else (offset, value)
        if method.endswith("igned"):  # the Signed / Unsigned forms take the size as their first argument
            args = (size, *args)
        bitset = self._batch._bitset
        name = self._name
        return self._batch._add(_Queued(name, fn=lambda: getattr(bitset(name), method)(*args),
                                        field=(op, int(signed), max(size, 0), L.RBX_OVERFLOW_WRAP, off, value)))

    def getSignedAsync(self, size: int, offset: int) -> BatchFuture:
        return self._field("getSigned", L.RBX_FIELD_GET, True, size, offset)

    def setSignedAsync(self, size: int, offset: int, value: int) -> BatchFuture:
        return self._field("setSigned", L.RBX_FIELD_SET, True, size, offset, value)

    def incrementAndGetSignedAsync(self, size: int, offset: int, increment: int) -> BatchFuture:
        return self._field("incrementAndGetSigned", L.RBX_FIELD_INCRBY, True, size, offset, increment)

    def getUnsignedAsync(self, size: int, offset: int) -> BatchFuture:
        return self._field("getUnsigned", L.RBX_FIELD_GET, False, size, offset)

    def setUnsignedAsync(self, size: int, offset: int, value: int) -> BatchFuture:
        return self._field("setUnsigned", L.RBX_FIELD_SET, False, size, offset, value)

    def incrementAndGetUnsignedAsync(self, size: int, offset: int, increment: int) -> BatchFuture:
        return self._field("incrementAndGetUnsigned", L.RBX_FIELD_INCRBY, False, size, offset, increment)

    def getByteAsync(self, offset: int) -> BatchFuture:
        return self._field("getByte", L.RBX_FIELD_GET, True, 8, offset)

    def setByteAsync(self, offset: int, value: int) -> BatchFuture:
        return self._field("setByte", L.RBX_FIELD_SET, True, 8, offset, value, 8)

    def incrementAndGetByteAsync(self, offset: int, increment: int) -> BatchFuture:
        return self._field("incrementAndGetByte", L.RBX_FIELD_INCRBY, True, 8, offset, increment, 8)

    def getShortAsync(self, offset: int) -> BatchFuture:
        return self._field("getShort", L.RBX_FIELD_GET, True, 16, offset)

    def setShortAsync(self, offset: int, value: int) -> BatchFuture:
        return self._field("setShort", L.RBX_FIELD_SET, True, 16, offset, value, 16)

    def incrementAndGetShortAsync(self, offset: int, increment: int) -> BatchFuture:
        return self._field("incrementAndGetShort", L.RBX_FIELD_INCRBY, True, 16, offset, increment, 16)

    def getIntegerAsync(self, offset: int) -> BatchFuture:
        return self._field("getInteger", L.RBX_FIELD_GET, True, 32, offset)

    def setIntegerAsync(self, offset: int, value: int) -> BatchFuture:
        return self._field("setInteger", L.RBX_FIELD_SET, True, 32, offset, value, 32)

    def incrementAndGetIntegerAsync(self, offset: int, increment: int) -> BatchFuture:
        return self._field("incrementAndGetInteger", L.RBX_FIELD_INCRBY, True, 32, offset, increment, 32)

    def getLongAsync(self, offset: int) -> BatchFuture:
        return self._field("getLong", L.RBX_FIELD_GET, True, 64, offset)

    def setLongAsync(self, offset: int, value: int) -> BatchFuture:
        return self._field("setLong", L.RBX_FIELD_SET, True, 64, offset, value)

    def incrementAndGetLongAsync(self, offset: int, increment: int) -> BatchFuture:
        return self._field("incrementAndGetLong", L.RBX_FIELD_INCRBY, True, 64, offset, increment)

    def setRangeAsync(self, fromIndex: int, toIndex: int, value: bool = True) -> BatchFuture:
        return self._single("setRange", fromIndex, toIndex, value)

    def clearRangeAsync(self, fromIndex: int, toIndex: int) -> BatchFuture:
        return self._single("clearRange", fromIndex, toIndex)

    def cardinalityAsync(self) -> BatchFuture:
        """:482-484 BITCOUNT: a one-source OR without a destination of the grouped call"""
        bitset, name = self._batch._bitset, self._name
        return self._batch._add(_Queued(name, fn=lambda: bitset(name).cardinality(),
                                        bitop=(L.RBX_BITOP_OR, None, [name]), convert=lambda _length, count: count,
                                        range=_range_row(L.RBX_RANGE_COUNT)))

    def _range(self, method: str, args: tuple, row: tuple, convert=None) -> BatchFuture:
        """a read query: consecutive ones, over any keys, travel together in one rbx_bitset_range_stream call"""
        bitset, name = self._batch._bitset, self._name
        return self._batch._add(_Queued(name, fn=lambda: getattr(bitset(name), method)(*args), range=row,
                                        convert=convert))

    def sizeAsync(self) -> BatchFuture:
        """:472-474 STRLEN * 8"""
        return self._range("size", (), _range_row(L.RBX_RANGE_STRLEN), lambda length: 8 * length)

    def lengthAsync(self) -> BatchFuture:
        return self._range("length", (), _range_row(L.RBX_RANGE_LENGTH))

    def bitCountAsync(self, start: int | None = None, end: int | None = None, unit="BYTE") -> BatchFuture:
        """Engine extension, RBitSet.bitCount queued: BITCOUNT name [start end [BYTE|BIT]]"""
        if start is None and end is None:
            return self.cardinalityAsync()
        if start is None or end is None:
            raise IllegalArgumentException("BITCOUNT takes both start and end, or neither")
        row = _range_row(L.RBX_RANGE_COUNT, 0, 2, RBitSet._java(start, 64, "start"), RBitSet._java(end, 64, "end"),
                         RBitSet._unit(unit))
        return self._range("bitCount", (start, end, unit), row)

    def bitPosAsync(self, bit, start: int | None = None, end: int | None = None, unit="BYTE") -> BatchFuture:
        """Engine extension, RBitSet.bitPos queued: BITPOS name bit [start [end [BYTE|BIT]]]"""
        if start is None and end is not None:
            raise IllegalArgumentException("BITPOS takes an end only after a start")
        nargs = 0 if start is None else (1 if end is None else 2)
        row = _range_row(L.RBX_RANGE_POS, RBitSet._java(int(bit), 32, "bit"), nargs,
                         RBitSet._java(start or 0, 64, "start"), RBitSet._java(end or 0, 64, "end"), RBitSet._unit(unit))
        return self._range("bitPos", (bit, start, end, unit), row)

    def membersAsync(self, start: int | None = None, end: int | None = None, unit="BYTE", skip: int = 0,
                     limit: int | None = None) -> BatchFuture:
        """Engine extension, RBitSet.members queued: consecutive ones, over any keys, travel together in one
        rbx_bitset_members_stream call"""
        if (start is None) != (end is None):
            raise IllegalArgumentException("members takes both start and end, or neither")
        if skip < 0 or (limit is not None and limit < 0):
            raise IllegalArgumentException("skip and limit are not negative")
        bitset, name = self._batch._bitset, self._name
        row = (0 if start is None else 2, RBitSet._java(start or 0, 64, "start"), RBitSet._java(end or 0, 64, "end"),
               RBitSet._unit(unit), int(skip), None if limit is None else int(limit))
        return self._batch._add(_Queued(name, fn=lambda: bitset(name).members(start, end, unit, skip, limit), members=row))

    def toByteArrayAsync(self) -> BatchFuture:
        return self._single("toByteArray")

    # ---- BITOP (M/api/RBitSetAsync.java:208-353, M/RedissonBitSet.java:362-388, :462-464): consecutive ones, and
    # cardinalityAsync among them, travel together in one rbx_bitset_op_groups call ----
    def _bitop(self, method: str, op: int, names) -> BatchFuture:
        """opAsync :381-388 -- BITOP op name name others..: the destination is also the first source"""
        bitset, name = self._batch._bitset, self._name
        return self._batch._add(_Queued(name, fn=lambda: getattr(bitset(name), method)(*names),
                                        bitop=(op, name, [name, *names]), convert=lambda _length, _count: None))

    def orAsync(self, *bitSetNames: str) -> BatchFuture:
        return self._bitop("or_", L.RBX_BITOP_OR, bitSetNames)

    def andAsync(self, *bitSetNames: str) -> BatchFuture:
        return self._bitop("and_", L.RBX_BITOP_AND, bitSetNames)

    def xorAsync(self, *bitSetNames: str) -> BatchFuture:
        return self._bitop("xor", L.RBX_BITOP_XOR, bitSetNames)

    def notAsync(self) -> BatchFuture:
        """:462-464 BITOP NOT name name"""
        return self._bitop("not_", L.RBX_BITOP_NOT, ())

    def clearAsync(self) -> BatchFuture:
        return self._single("clear")

    get_async = getAsync
    set_async = setAsync
    clear_bit_async = clearBitAsync
    get_signed_async = getSignedAsync
    set_signed_async = setSignedAsync
    increment_and_get_signed_async = incrementAndGetSignedAsync
    get_unsigned_async = getUnsignedAsync
    set_unsigned_async = setUnsignedAsync
    increment_and_get_unsigned_async = incrementAndGetUnsignedAsync
    get_byte_async = getByteAsync
    set_byte_async = setByteAsync
    increment_and_get_byte_async = incrementAndGetByteAsync
    get_short_async = getShortAsync
    set_short_async = setShortAsync
    increment_and_get_short_async = incrementAndGetShortAsync
    get_integer_async = getIntegerAsync
    set_integer_async = setIntegerAsync
    increment_and_get_integer_async = incrementAndGetIntegerAsync
    get_long_async = getLongAsync
    set_long_async = setLongAsync
    increment_and_get_long_async = incrementAndGetLongAsync
    set_range_async = setRangeAsync
    clear_range_async = clearRangeAsync
    cardinality_async = cardinalityAsync
    size_async = sizeAsync
    length_async = lengthAsync
    bit_count_async = bitCountAsync
    bit_pos_async = bitPosAsync
    to_byte_array_async = toByteArrayAsync
    or_async = orAsync
    and_async = andAsync
    xor_async = xorAsync
    not_async = notAsync
    clear_async = clearAsync


class RBatchHyperLogLog:
    """RBatch.getHyperLogLog(name) (M/RedissonBatch.java:57-64): RHyperLogLogAsync, every method queued.
    addAsync / addAllAsync / countAsync of consecutive commands, over any keys, travel together (one
    rbx_hll_stream call); so do consecutive countWithAsync commands with other names (one rbx_hll_count_groups
    call) and consecutive mergeWithAsync commands (one rbx_hll_merge_groups call, in order)."""

    def __init__(self, batch: "RBatch", name: str, codec: Codec):
        self._batch, self._name, self._codec = batch, name, codec

    def _single(self, method: str, *args) -> BatchFuture:
        hll, name = self._batch._hyperloglog, self._name
        return self._batch._add(_Queued(fn=lambda: getattr(hll(name, self._codec), method)(*args)))

    def addAsync(self, obj) -> BatchFuture:
        return self.addAllAsync([obj])

    def addAllAsync(self, objects) -> BatchFuture:
        elements = [self._codec.encode(o) for o in objects]
        hll, name = self._batch._hyperloglog, self._name
        return self._batch._add(_Queued(name, fn=lambda: hll(name, self._codec).addAll(Arena(elements)),
                                        hll=(PFADD, elements)))

    def countAsync(self) -> BatchFuture:
        hll, name = self._batch._hyperloglog, self._name
        return self._batch._add(_Queued(name, fn=lambda: hll(name, self._codec).count(), hll=(PFCOUNT, [])))

    def countWithAsync(self, *otherLogNames: str) -> BatchFuture:
        if not otherLogNames:
            return self.countAsync()
        hll, name = self._batch._hyperloglog, self._name
        return self._batch._add(_Queued(name, fn=lambda: hll(name, self._codec).countWith(*otherLogNames),
                                        group=("count", [name, *otherLogNames])))

    def mergeWithAsync(self, *otherLogNames: str) -> BatchFuture:
        hll, name = self._batch._hyperloglog, self._name
        return self._batch._add(_Queued(name, fn=lambda: hll(name, self._codec).mergeWith(*otherLogNames),
                                        group=("merge", name, list(otherLogNames))))

    add_async = addAsync
    add_all_async = addAllAsync
    count_async = countAsync
    count_with_async = countWithAsync
    merge_with_async = mergeWithAsync


class RBatch:
    """RedissonClient.createBatch() (M/RedissonBatch.java): commands queue across any number of keys, execute()
    runs them in submission order (M/command/CommandBatchService.java:115-134,335) and returns their replies
    in that order.  stream_call / bitset / field_stream_call / hll_stream_call / hyperloglog /
    hll_count_groups_call / hll_merge_groups_call / bit_groups_call replace the engine's calls (tests); without a
    client and without a field_stream_call (an hll_stream_call, a grouped call), field (HLL, multi-key PFCOUNT /
    PFMERGE, BITOP / BITCOUNT) commands run singly through bitset(name) (hyperloglog(name, codec)).
    range_stream_call carries the read queries (size / length / bitCount / bitPos) and members_stream_call the
    enumerations (membersAsync); createBatch() passes the engine's, and without one they run singly."""

    def __init__(self, client: RedissonClient | None, stream_call=None, bitset=None, field_stream_call=None,
                 hll_stream_call=None, hyperloglog=None, hll_count_groups_call=None, hll_merge_groups_call=None,
                 bit_groups_call=None, range_stream_call=None, members_stream_call=None):
        self._client = client
        self._stream_call = stream_call or (lambda *a: bitset_stream_call(client, *a))
        if field_stream_call is None and client is not None:
            field_stream_call = lambda *a: bitset_field_stream_call(client, *a)  # noqa: E731
        self._field_stream_call = field_stream_call
        if hll_stream_call is None and client is not None:
            hll_stream_call = lambda *a: _engine_hll_stream_call(client, *a)  # noqa: E731
        self._hll_stream_call = hll_stream_call
        if hll_count_groups_call is None and client is not None:
            hll_count_groups_call = lambda *a: _engine_hll_count_groups_call(client, *a)  # noqa: E731
        if hll_merge_groups_call is None and client is not None:
            hll_merge_groups_call = lambda *a: _engine_hll_merge_groups_call(client, *a)  # noqa: E731
        self._hll_groups_calls = (hll_count_groups_call, hll_merge_groups_call)
        if bit_groups_call is None and client is not None:
            bit_groups_call = lambda *a: _engine_bitset_op_groups_call(client, *a)  # noqa: E731
        self._bit_groups_call = bit_groups_call
        self._range_stream_call = range_stream_call
        self._members_stream_call = members_stream_call
        self._hyperloglog = hyperloglog or (lambda name, codec: RHyperLogLog(client, name, codec))
        self._bitset = bitset or (lambda name: RBitSet(client, name))
        self._queue: list = []
        self._executed = False

    def _add(self, q: _Queued) -> BatchFuture:
        if self._executed:
            raise IllegalStateException("Batch already executed!")
        self._queue.append(q)
        return q.future

    def getBitSet(self, name: str) -> RBatchBitSet:
        return RBatchBitSet(self, name)

    def getHyperLogLog(self, name: str, codec: Codec | None = None) -> RBatchHyperLogLog:
        return RBatchHyperLogLog(self, name, codec or DEFAULT_CODEC)

    def execute(self) -> BatchResult:
        """Every command runs, the ones after a failed one too; then the first failure is raised."""
        if self._executed:
            raise IllegalStateException("Batch already executed!")
        self._executed = True
        responses, error = run_queue(self._queue, self._stream_call, self._field_stream_call, self._hll_stream_call,
                                     *self._hll_groups_calls, self._bit_groups_call, self._range_stream_call,
                                     self._members_stream_call)
        if error is not None:
            raise error
        return BatchResult(responses)

    def discard(self) -> None:
        if self._executed:
            raise IllegalStateException("Batch already executed!")
        self._queue.clear()

    get_bit_set = getBitSet
    get_hyper_log_log = getHyperLogLog


class BloomHandle:
    """Open handle for the device-resident batch path (rbx_bloom_*_dev)."""

    def __init__(self, client: RedissonClient, name: str):
        self._client = client
        self.h = C.c_void_p()
        _check(L.lib().rbx_bloom_open(client.ctx, name.encode(), C.byref(self.h)))
        s, k = C.c_uint64(), C.c_uint32()
        _check(L.lib().rbx_bloom_handle_config(self.h, C.byref(s), C.byref(k)))
        self.size, self.k = int(s.value), int(k.value)

    def contains_dev(self, keys: L.RbxKeys, d_count: int, d_out: int | None = None, stream: int | None = None):
        _check(L.lib().rbx_bloom_contains_dev(self._client.ctx, self.h, C.byref(keys), d_out, d_count, stream))

    def add_dev(self, keys: L.RbxKeys, d_count: int, d_out: int | None = None, stream: int | None = None):
        _check(L.lib().rbx_bloom_add_dev(self._client.ctx, self.h, C.byref(keys), d_out, d_count, stream))

    def close(self):
        if self.h:
            _check(L.lib().rbx_bloom_close(self.h))
            self.h = C.c_void_p()


def _handles(hs):
    arr = (C.c_void_p * len(hs))(*[h.h.value for h in hs])
    return arr


def bloom_contains_multi(client: RedissonClient, handles: list[BloomHandle], seg_offsets: np.ndarray,
                         arena: Arena, per_key: bool = False):
    """One contains(Collection) per segment (multi-tenant host path)."""
    nseg = len(handles)
    seg = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    counts = np.zeros(nseg, np.uint64)
    out = np.zeros(max(arena.n, 1), np.uint8) if per_key else None
    _check(L.lib().rbx_bloom_contains_multi(client.ctx, _handles(handles), nseg, seg.ctypes.data_as(L.u64p),
                                            arena.ptr(), out.ctypes.data_as(L.u8p) if per_key else None,
                                            counts.ctypes.data_as(L.u64p)))
    return (counts, out[: arena.n]) if per_key else counts


def bloom_add_multi(client: RedissonClient, handles: list[BloomHandle], seg_offsets: np.ndarray,
                    arena: Arena, per_key: bool = False):
    """One add(Collection) per segment, applied in segment order (multi-tenant host path)."""
    nseg = len(handles)
    seg = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    counts = np.zeros(nseg, np.uint64)
    out = np.zeros(max(arena.n, 1), np.uint8) if per_key else None
    _check(L.lib().rbx_bloom_add_multi(client.ctx, _handles(handles), nseg, seg.ctypes.data_as(L.u64p),
                                       arena.ptr(), out.ctypes.data_as(L.u8p) if per_key else None,
                                       counts.ctypes.data_as(L.u64p)))
    return (counts, out[: arena.n]) if per_key else counts


def bloom_stream(client: RedissonClient, handles: list[BloomHandle], key_filter, key_op, arena: Arena):
    """Ordered mixed stream of single-key contains (op 0) / add (op 1) commands on
    handles[key_filter[i]]; returns (per-key results, [present contains, newly added])."""
    kf = np.ascontiguousarray(key_filter, dtype=np.uint32)
    op = np.ascontiguousarray(key_op, dtype=np.uint8)
    out = np.zeros(max(arena.n, 1), np.uint8)
    counts = np.zeros(2, np.uint64)
    _check(L.lib().rbx_bloom_stream(client.ctx, _handles(handles), len(handles), kf.ctypes.data_as(L.u32p),
                                    op.ctypes.data_as(L.u8p), arena.ptr(), out.ctypes.data_as(L.u8p),
                                    counts.ctypes.data_as(L.u64p)))
    return out[: arena.n], counts


class RFuture:
    """org.redisson.api.RFuture over an rbx_future: the asynchronous call runs on the context's
    serial executor; get() waits and returns the converted result (or raises the call's error)."""

    def __init__(self, fut: C.c_void_p, convert, keep):
        self._f = fut
        self._convert = convert
        self._keep = keep  # buffers the call reads / writes until it completes
        self._done = False

    def isDone(self) -> bool:
        d = C.c_int()
        _check(L.lib().rbx_future_done(self._f, C.byref(d)))
        return bool(d.value)

    def get(self, timeout_ms: int = -1):
        """Result of the call; TimeoutError if it has not completed within timeout_ms."""
        rc = C.c_int()
        r = L.lib().rbx_future_wait(self._f, int(timeout_ms), C.byref(rc))
        if r == L.RBX_E_TIMEOUT:
            raise TimeoutError("the call has not completed")
        _check(r)
        _check(rc.value)
        return self._convert()

    def __del__(self):
        f = getattr(self, "_f", None)
        if f:
            try:
                L.lib().rbx_future_wait(f, -1, None)  # the buffers in _keep must outlive the call
                L.lib().rbx_future_free(f)
            except Exception:  # interpreter shutdown
                pass

    is_done = isDone


class RHyperLogLog(_Expirable):
    """M/RedissonHyperLogLog.java (PFADD / PFCOUNT / PFMERGE) and RHyperLogLogAsync
    (M/api/RHyperLogLogAsync.java:37-70: the *Async methods return an RFuture)."""

    def __init__(self, client: RedissonClient, name: str, codec: Codec):
        self._client = client
        self._name = name
        self._codec = codec

    def getName(self) -> str:
        return self._name

    def add(self, obj) -> bool:
        """:71-73 PFADD name e"""
        return self.addAll(_OneKey(self._codec.encode(obj)))

    def addAll(self, objects) -> bool:
        """:76-81 PFADD name e1..en"""
        a = objects if isinstance(objects, (Arena, _OneKey)) else Arena([self._codec.encode(o) for o in objects])
        ch = C.c_int()
        _check(L.lib().rbx_hll_add(self._client.ctx, self._name.encode(), a.ptr(), C.byref(ch)))
        return bool(ch.value)

    def count(self) -> int:
        """:84-86 PFCOUNT name"""
        return self.countWith()

    def countWith(self, *otherLogNames: str) -> int:
        """:89-94 PFCOUNT name o1..on"""
        names = [self._name, *otherLogNames]
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        out = C.c_uint64()
        _check(L.lib().rbx_hll_count(self._client.ctx, arr, len(names), C.byref(out)))
        return int(out.value)

    def mergeWith(self, *otherLogNames: str) -> None:
        """:97-102 PFMERGE name o1..on"""
        arr = (C.c_char_p * max(len(otherLogNames), 1))(*[n.encode() for n in otherLogNames])
        _check(L.lib().rbx_hll_merge(self._client.ctx, self._name.encode(), arr, len(otherLogNames)))

    # ---- RHyperLogLogAsync ------------------------------------------------------------------
    def addAsync(self, obj) -> RFuture:
        return self.addAllAsync([obj])

    def addAllAsync(self, objects) -> RFuture:
        a = objects if isinstance(objects, Arena) else Arena([self._codec.encode(o) for o in objects])
        ch = C.c_int()
        f = C.c_void_p()
        _check(L.lib().rbx_hll_add_async(self._client.ctx, self._name.encode(), a.ptr(), C.byref(ch), None, None,
                                         C.byref(f)))
        return RFuture(f, lambda: bool(ch.value), (a, ch))

    def countAsync(self) -> RFuture:
        return self.countWithAsync()

    def countWithAsync(self, *otherLogNames: str) -> RFuture:
        names = [self._name, *otherLogNames]
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        out = C.c_uint64()
        f = C.c_void_p()
        _check(L.lib().rbx_hll_count_async(self._client.ctx, arr, len(names), C.byref(out), None, None, C.byref(f)))
        return RFuture(f, lambda: int(out.value), (arr, out))

    def mergeWithAsync(self, *otherLogNames: str) -> RFuture:
        arr = (C.c_char_p * max(len(otherLogNames), 1))(*[n.encode() for n in otherLogNames])
        f = C.c_void_p()
        _check(L.lib().rbx_hll_merge_async(self._client.ctx, self._name.encode(), arr, len(otherLogNames), None,
                                           None, C.byref(f)))
        return RFuture(f, lambda: None, (arr,))

    def delete(self) -> bool:
        n = C.c_int()
        _check(L.lib().rbx_hll_delete(self._client.ctx, self._name.encode(), C.byref(n)))
        return n.value > 0

    def isExists(self) -> bool:
        e = C.c_int()
        _check(L.lib().rbx_hll_exists(self._client.ctx, self._name.encode(), C.byref(e)))
        return bool(e.value)

    def _expire_keys(self):
        return [self._name]

    def exportDense(self) -> bytes:
        """GET name, as the Redis dense HLL string."""
        n = C.c_uint64()
        buf = np.zeros(16 + 12288, np.uint8)
        _check(L.lib().rbx_hll_export(self._client.ctx, self._name.encode(), buf.ctypes.data_as(L.u8p),
                                      buf.size, C.byref(n)))
        return buf[: n.value].tobytes()

    _ENCODINGS = {"dense": 0, "sparse": 1, "stored": 2}

    def exportString(self, encoding: str = "stored") -> bytes:
        """GET name as a Redis HLL string: "stored" = the encoding Redis would hold (sparse until
        promoted), "dense", or "sparse" (IllegalArgumentException if a register exceeds 32).
        Empty bytes if the key does not exist."""
        if encoding not in self._ENCODINGS:
            raise IllegalArgumentException("encoding must be one of %s" % sorted(self._ENCODINGS))
        n = C.c_uint64()
        # a sparse string can be longer than the dense one: the fewest-bytes form of a dense key has up to one opcode
        # byte per register, a SET string up to 16384 opcodes of two bytes
        buf = np.zeros(16 + 2 * 16384, np.uint8)
        _check(L.lib().rbx_hll_export_enc(self._client.ctx, self._name.encode(), self._ENCODINGS[encoding],
                                          buf.ctypes.data_as(L.u8p), buf.size, C.byref(n)))
        assert n.value <= buf.size, "a sparse HLL string holds at most 16384 opcodes"
        return buf[: n.value].tobytes()

    def importString(self, data: bytes) -> None:
        """SET name <Redis HLL string> (dense or sparse)."""
        buf = np.frombuffer(data, np.uint8)
        _check(L.lib().rbx_hll_import(self._client.ctx, self._name.encode(), buf.ctypes.data_as(L.u8p), len(data)))

    add_all = addAll
    count_with = countWith
    merge_with = mergeWith
    add_all_async = addAllAsync
    count_async = countAsync
    merge_with_async = mergeWithAsync


def hll_add_multi(client: RedissonClient, names: list[str], seg_offsets, arena: Arena) -> np.ndarray:
    """A pipeline of PFADD commands (segment s -> names[s]); returns each reply."""
    nseg = len(names)
    arr = (C.c_char_p * nseg)(*[n.encode() for n in names])
    seg = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    out = np.zeros(max(nseg, 1), np.uint8)
    _check(L.lib().rbx_hll_add_multi(client.ctx, arr, nseg, seg.ctypes.data_as(L.u64p), arena.ptr(),
                                     out.ctypes.data_as(L.u8p)))
    return out[:nseg]


def hll_count_each(client: RedissonClient, names: list[str]) -> np.ndarray:
    n = len(names)
    arr = (C.c_char_p * max(n, 1))(*[x.encode() for x in names])
    out = np.zeros(max(n, 1), np.uint64)
    _check(L.lib().rbx_hll_count_each(client.ctx, arr, n, out.ctypes.data_as(L.u64p)))
    return out[:n]


def crc16(data: bytes) -> int:
    b = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    return int(L.lib().rbx_crc16(b, len(data)))


def calc_slot(key: bytes | str) -> int:
    """ClusterConnectionManager.calcSlot (M/cluster/ClusterConnectionManager.java:777-830)."""
    if isinstance(key, str):
        key = key.encode("utf-8")
    b = (C.c_uint8 * max(1, len(key))).from_buffer_copy(key or b"\0")
    return int(L.lib().rbx_calc_slot(b, len(key)))


def slot_to_gpu(slot: int, n_gpus: int) -> int:
    return int(L.lib().rbx_slot_to_gpu(slot, n_gpus))
