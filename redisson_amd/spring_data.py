"""Spring Data Redis connection surface: HyperLogLog (second caller of the HLL path) and the bit commands
on strings (second caller of the RBitSet path).

Mirrors redisson-spring-data's RedissonConnection.pfAdd / pfCount / pfMerge
(redisson-spring-data/redisson-spring-data-32/src/main/java/org/redisson/spring/data/connection/
RedissonConnection.java:2200-2226): raw byte[] keys and members, no codec (ByteArrayCodec /
StringCodec pass the bytes through), PFADD's integer reply as a Long.

The bit commands mirror redisson-spring-data-31's RedissonConnection (S/ = redisson-spring-data/
redisson-spring-data-31/src/main/java/org/redisson/spring/data/connection/RedissonConnection.java): getBit /
setBit S:628-636, bitCount S:638-646, bitOp S:650-661, strLen S:663-666, bitField S:2241-2291,
bitPos S:2337-2359.  The byte-level commands on the same strings sit directly above them: get S:487, mGet S:499,
set S:506, append S:610, getRange S:617, setRange S:624.

Keys are binary-safe: they travel as (bytes, length) pairs through the *_n entry points
(rbx_hll_add_multi_n / rbx_hll_count_n / rbx_hll_merge_n), so a key may hold any byte, zero
bytes included, exactly as a Redis key can.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib as L
from .client import (GETBIT, PFADD, PFCOUNT, SETBIT0, SETBIT1, RedissonClient, _bit_index, _check, _Queued, _range_row,
                     bitset_field_stream_call, bitset_op_groups_call, bitset_range_stream_call, bitset_stream_call,
                     hll_count_groups_call, hll_merge_groups_call, hll_stream_call, run_queue, STRING_FAILED, STRING_NIL,
                     string_append, string_failure, string_getrange, string_setrange, string_stream_call, _u8)
from .exceptions import IllegalArgumentException, UnsupportedOperationException
from .keys import Arena


def _key(k) -> bytes:
    if k is None:
        raise IllegalArgumentException("Keys must not contain 'null'.")
    return bytes(k)


# ---- BitFieldSubCommands (org.springframework.data.redis.connection.BitFieldSubCommands) ------------
class BitFieldType:
    """BitFieldSubCommands.BitFieldType: INT_8 is BitFieldType(True, 8); asString() is 'i8' (S:2262-2266)"""

    def __init__(self, signed: bool, bits: int):
        self.signed, self.bits = bool(signed), int(bits)

    def asString(self) -> str:
        return ("i" if self.signed else "u") + str(self.bits)

    as_string = asString


class Offset:
    """BitFieldSubCommands.Offset: zero_based sends the plain bit offset, otherwise '#N' = N * bits (S:2256-2260)"""

    def __init__(self, value: int, zero_based: bool = True):
        self.value, self.zero_based = int(value), bool(zero_based)

    def asString(self) -> str:
        return str(self.value) if self.zero_based else "#" + str(self.value)

    as_string = asString


def _offset(offset) -> Offset:
    return offset if isinstance(offset, Offset) else Offset(offset)


class BitFieldGet:
    def __init__(self, type: BitFieldType, offset):
        self.type, self.offset = type, _offset(offset)


class BitFieldSet:
    def __init__(self, type: BitFieldType, offset, value: int):
        self.type, self.offset, self.value = type, _offset(offset), int(value)


class BitFieldIncrBy:
    """overflow: None, 'WRAP', 'SAT' or 'FAIL' (BitFieldIncrBy.Overflow)"""

    def __init__(self, type: BitFieldType, offset, value: int, overflow: str | None = None):
        self.type, self.offset, self.value = type, _offset(offset), int(value)
        self.overflow = None if overflow is None else str(overflow).upper()
        if self.overflow not in (None, "WRAP", "SAT", "FAIL"):
            raise IllegalArgumentException(f"unknown OVERFLOW mode {overflow!r}")


def resolve_overflow(subCommands) -> list:
    """The OVERFLOW mode each sub-command of bitField runs under, as 'WRAP' / 'SAT' / 'FAIL'.  S:2272-2283
    appends `OVERFLOW <mode>` AFTER the INCRBY that carries it, and in Redis an OVERFLOW governs the SET /
    INCRBY sub-commands that FOLLOW it: an INCRBY runs under the mode of the previous INCRBY that carried
    one (the first under WRAP), and its own mode holds from the next sub-command on.  Needs no library."""
    mode, out = "WRAP", []
    for cmd in subCommands:
        out.append(mode)
        if isinstance(cmd, BitFieldIncrBy) and cmd.overflow is not None:
            mode = cmd.overflow
    return out


_MODES = {"WRAP": L.RBX_OVERFLOW_WRAP, "SAT": L.RBX_OVERFLOW_SAT, "FAIL": L.RBX_OVERFLOW_FAIL}


def _field_row(cmd, mode: str) -> tuple:
    """one sub-command of bitField under `mode` as (op, signed, size, overflow, offset, value) of rbx_field_cmd"""
    if isinstance(cmd, BitFieldGet):
        op = L.RBX_FIELD_GET
    elif isinstance(cmd, BitFieldSet):
        op = L.RBX_FIELD_SET
    elif isinstance(cmd, BitFieldIncrBy):
        op = L.RBX_FIELD_INCRBY
    else:
        raise IllegalArgumentException(f"unknown BITFIELD sub-command {cmd!r}")
    bits = cmd.type.bits
    offset = cmd.offset.value if cmd.offset.zero_based else cmd.offset.value * bits
    value = getattr(cmd, "value", 0)
    if not -(1 << 63) <= value < 1 << 63:
        raise IllegalArgumentException("field values are Java longs")
    return (op, int(cmd.type.signed), bits if 0 <= bits <= 255 else 0,  # no such type: Redis's error
            _MODES[mode], offset if 0 <= offset < 1 << 64 else (1 << 64) - 1,  # past the limit either way
            value)


def _one_sub_command(key, subCommands):
    """(key, row, convert) for a pipelined bitField of exactly one sub-command (it runs under WRAP: an OVERFLOW
    governs what follows it), whose result is [reply] or [None]; None for any other list"""
    cmds = list(subCommands)
    if len(cmds) != 1:
        return None
    return key, _field_row(cmds[0], "WRAP"), lambda reply: [reply]


def _pf_add(key, *values):
    """(key, (PFADD, elements), convert) of a pipelined pfAdd: the reply is the Long 1 / 0"""
    return key, (PFADD, [bytes(v) for v in values]), int


def _pf_count(*keys):
    """(key, (PFCOUNT, []), None) of a pipelined single-key pfCount; None for any other (a pfCount of several keys
    is _pf_count_group's; what is left runs singly, and raises there what it has to raise)"""
    if len(keys) != 1 or keys[0] is None:
        return None
    return keys[0], (PFCOUNT, []), None


def _pf_count_group(*keys):
    """("count", keys) of a pipelined pfCount with two or more keys; None for any other"""
    if len(keys) < 2 or any(k is None for k in keys):
        return None
    return ("count", [_key(k) for k in keys])


def _pf_merge_group(destinationKey, *sourceKeys):
    """("merge", destination, sources) of a pipelined pfMerge"""
    return ("merge", _key(destinationKey), [_key(k) for k in sourceKeys])


_BITOPS = {"AND": L.RBX_BITOP_AND, "OR": L.RBX_BITOP_OR, "XOR": L.RBX_BITOP_XOR, "NOT": L.RBX_BITOP_NOT}


def _bit_op_code(op, keys) -> int:
    """bitOp's own checks (S:650-661): the RBX_BITOP_* value of an operation's name or value; NOT takes one source"""
    code = _BITOPS.get(op.upper()) if isinstance(op, str) else (op if op in _BITOPS.values() else None)
    if code is None:
        raise IllegalArgumentException(f"unknown BITOP operation {op!r}")
    if code == L.RBX_BITOP_NOT and len(keys) > 1:
        raise UnsupportedOperationException("NOT operation doesn't support more than single source key")
    return code


def _bit_op_group(op, destination, *keys):
    """((RBX_BITOP_*, destination, sources), convert) of a pipelined bitOp: the reply is the result's length.  NOT with
    several sources raises before anything is queued (S:652-654)."""
    try:
        code = _bit_op_code(op, keys)
    except IllegalArgumentException:
        return None  # the single call raises it at its position
    if not keys:
        return None
    return (code, _key(destination), [_key(k) for k in keys]), lambda length, _count: length


def _bit_count_group(key, begin=None, end=None):
    """the same of a pipelined bitCount(key): a one-source OR that is stored nowhere; a ranged one runs singly"""
    if begin is not None or end is not None:
        return None
    return (L.RBX_BITOP_OR, None, [_key(key)]), lambda _length, count: count


def _bit_count_range(key, begin=None, end=None):
    """(key, row, convert) of a pipelined bitCount as a read query: BITCOUNT key, or BITCOUNT key begin end"""
    if begin is None and end is None:
        return key, _range_row(L.RBX_RANGE_COUNT), None
    if begin is None or end is None:
        return None  # the single call raises it at its position
    return key, _range_row(L.RBX_RANGE_COUNT, 0, 2, int(begin), int(end), L.RBX_RANGE_BYTE), None


def _bit_pos_range(key, bit, range=(None, None)):  # noqa: A002
    """the same of a pipelined bitPos: the upper bound travels only behind a bounded lower one (S:2351-2356)"""
    if range is None:
        return None
    lower, upper = range
    nargs = 0 if lower is None else (1 if upper is None else 2)
    return key, _range_row(L.RBX_RANGE_POS, int(bool(bit)), nargs, int(lower or 0), int(upper or 0) if nargs == 2 else 0,
                           L.RBX_RANGE_BYTE), None


def _string_get(key):
    """(key, row, convert) of a pipelined get: the bytes, None for a missing key"""
    return key, (L.RBX_STR_GET, 0, 0, b""), lambda _n, data, status: None if status == STRING_NIL else data


def _string_get_range(key, start, end):
    return key, (L.RBX_STR_GETRANGE, int(start), int(end), b""), lambda _n, data, _status: data


def _string_set_range(key, value, offset):
    """setRange is void (S:624-627)"""
    return key, (L.RBX_STR_SETRANGE, _int64(offset), 0, bytes(value)), lambda _n, _data, _status: None


def _string_append(key, value):
    return key, (L.RBX_STR_APPEND, 0, 0, bytes(value)), lambda n, _data, _status: n


def _int64(v) -> int:
    """a Java long; what lies outside is as wrong as its nearest end"""
    return max(-(1 << 63), min((1 << 63) - 1, int(v)))


def _pipelined(fn=None, *, bit=None, field=None, hll=None, group=None, bitop=None, rng=None, string=None):
    """A command method of RedissonConnection: while a pipeline is open it queues itself and returns None
    (the result comes back from closePipeline); bit = (key, op, index) of a GETBIT / SETBIT, which travels with
    its neighbours in one rbx_bitset_stream call; field = (key, row, convert) of a BITFIELD with one sub-command
    (or None for any other), which travels with its bit and field neighbours in one rbx_bitset_field_stream call;
    hll = (key, (op, elements), convert) of a PFADD / single-key PFCOUNT (or None for any other), which travels
    with its HLL neighbours in one rbx_hll_stream call; group = ("count", keys) of a multi-key PFCOUNT or ("merge",
    destination, sources) of a PFMERGE (or None for any other), which travels with its like in one
    rbx_hll_count_groups / rbx_hll_merge_groups call; bitop = ((RBX_BITOP_*, destination or None, sources), convert)
    of a BITOP or a whole-string BITCOUNT (or None for any other), which travels with its like in one
    rbx_bitset_op_groups call; rng = (key, row, convert) of a read query (BITCOUNT, BITPOS, STRLEN; or None for any
    other), which travels with its like in one rbx_bitset_range_stream call -- a whole-string BITCOUNT carries both;
    string = (key, row, convert) of a GET / GETRANGE / SETRANGE / APPEND, which travels with its like in one
    rbx_string_stream call."""

    def wrap(f):
        @functools.wraps(f)
        def method(self, *args, **kwargs):
            if self._pipeline is None:
                return f(self, *args, **kwargs)
            if bit is not None:
                key, op, index = bit(*args, **kwargs)
                self._pipeline.append(_Queued(_key(key), op, _bit_index(index)))
                return None
            single = lambda: f(self, *args, **kwargs)  # noqa: E731
            if string is not None:
                try:
                    key, row, convert = string(*args, **kwargs)
                    self._pipeline.append(_Queued(_key(key), fn=single, string=row, convert=convert))
                except (IllegalArgumentException, TypeError, ValueError):
                    self._pipeline.append(_Queued(fn=single))  # the single call raises it at its position
                return None
            query = None
            if rng is not None:
                try:
                    query = rng(*args, **kwargs)
                except (IllegalArgumentException, TypeError, ValueError):
                    query = None  # the single call raises it at its position
            row = bitop(*args, **kwargs) if bitop is not None else None
            if row is not None:
                self._pipeline.append(_Queued(row[0][2][0], fn=single, bitop=row[0], convert=row[1],
                                              range=query[1] if query else None))
                return None
            if query is not None:
                self._pipeline.append(_Queued(_key(query[0]), fn=single, range=query[1], convert=query[2]))
                return None
            if bitop is not None:
                self._pipeline.append(_Queued(fn=single))
                return None
            if group is not None:
                try:
                    row = group(*args, **kwargs)
                except (IllegalArgumentException, TypeError):
                    row = None  # the single call raises it at its position
                if row is not None:
                    self._pipeline.append(_Queued(row[1] if row[0] == "merge" else row[1][0], fn=single, group=row))
                    return None
            if hll is not None:
                try:
                    row = hll(*args, **kwargs)
                except (IllegalArgumentException, TypeError):
                    row = None  # the single call raises it at its position
                if row is not None and row[0] is not None:
                    key, cmd, convert = row
                    self._pipeline.append(_Queued(_key(key), fn=single, hll=cmd, convert=convert))
                else:
                    self._pipeline.append(_Queued(fn=single))
                return None
            try:
                row = field(*args, **kwargs) if field is not None else None
            except IllegalArgumentException:
                row = None  # the single call raises it at its position
            if row is not None:
                key, cmd, convert = row
                self._pipeline.append(_Queued(_key(key), fn=single, field=cmd, convert=convert))
            else:
                self._pipeline.append(_Queued(fn=single))
            return None

        return method

    return wrap(fn) if fn is not None else wrap


class RedissonConnection:
    def __init__(self, client: RedissonClient):
        self._client = client
        self._pipeline = None  # the queued commands while a pipeline is open

    # ---- pipelining (redisson-spring-data-32 RedissonConnection.java:118-163) ----------------------
    def isPipelined(self) -> bool:
        return self._pipeline is not None

    def openPipeline(self) -> None:
        """:139-143 -- an IN_MEMORY batch: commands queue until closePipeline"""
        self._pipeline = []

    def closePipeline(self) -> list:
        """:146-163 -- runs the queued commands in order and returns their results; [] outside a pipeline.
        Consecutive getBit / setBit commands, over any keys, are one rbx_bitset_stream call; with a bitField of
        exactly one sub-command among them they are one rbx_bitset_field_stream call.  Consecutive pfAdd and
        single-key pfCount commands, over any keys, are one rbx_hll_stream call; consecutive pfCount commands of
        two or more keys are one rbx_hll_count_groups call, consecutive pfMerge commands one rbx_hll_merge_groups
        call.  Consecutive bitOp and bitCount(key) commands, over any keys, are one rbx_bitset_op_groups call;
        consecutive bitCount(key, begin, end), bitPos and strLen commands one rbx_bitset_range_stream call, which a
        bitCount(key) behind them joins.  Consecutive get / getRange / setRange / append commands, over any keys, are
        one rbx_string_stream call; set runs singly at its position.  Every command runs; then the first failure is
        raised."""
        if self._pipeline is None:
            return []
        queue, self._pipeline = self._pipeline, None
        results, error = run_queue(queue, lambda *a: bitset_stream_call(self._client, *a),
                                   lambda *a: bitset_field_stream_call(self._client, *a),
                                   lambda *a: hll_stream_call(self._client, *a),
                                   lambda *a: hll_count_groups_call(self._client, *a),
                                   lambda *a: hll_merge_groups_call(self._client, *a),
                                   lambda *a: bitset_op_groups_call(self._client, *a),
                                   lambda *a: bitset_range_stream_call(self._client, *a),
                                   string_stream_call=lambda *a: string_stream_call(self._client, *a)[:6],
                                   string_failure=lambda *a: string_failure(self._client, *a))
        if error is not None:
            raise error
        return results

    is_pipelined = isPipelined
    open_pipeline = openPipeline
    close_pipeline = closePipeline

    @_pipelined(hll=_pf_add)
    def pfAdd(self, key: bytes, *values: bytes) -> int:
        """PFADD key v1..vn -> 1 if the HLL was created or a register changed, else 0."""
        a = Arena([bytes(v) for v in values])
        names, keep = L.names_array([_key(key)])
        seg = np.array([0, a.n], dtype=np.uint64)
        ch = np.zeros(1, np.uint8)
        _check(L.lib().rbx_hll_add_multi_n(self._client.ctx, names, 1, seg.ctypes.data_as(L.u64p), a.ptr(),
                                           ch.ctypes.data_as(L.u8p)))
        return int(ch[0])

    @_pipelined(hll=_pf_count, group=_pf_count_group)
    def pfCount(self, *keys: bytes) -> int:
        """PFCOUNT k1..kn (union when n > 1)."""
        if not keys:
            raise IllegalArgumentException("PFCOUNT requires at least one non 'null' key.")
        if any(k is None for k in keys):
            raise IllegalArgumentException("Keys for PFOUNT must not contain 'null'.")
        names, keep = L.names_array([_key(k) for k in keys])
        out = C.c_uint64()
        _check(L.lib().rbx_hll_count_n(self._client.ctx, names, len(keys), C.byref(out)))
        return int(out.value)

    @_pipelined(group=_pf_merge_group)
    def pfMerge(self, destinationKey: bytes, *sourceKeys: bytes) -> None:
        """PFMERGE dest s1..sn (dest's own registers included)."""
        srcs, keep = L.names_array([_key(k) for k in sourceKeys])
        dest, keep_d = L.name_struct(_key(destinationKey))
        _check(L.lib().rbx_hll_merge_n(self._client.ctx, dest, srcs, len(sourceKeys)))

    # ---- byte-level commands on strings (rbx_string_*, binary names) ---------------------------
    def _string_one(self, key, row):
        """one command through rbx_string_stream: (number, bytes, status); raises what the command fails with"""
        rc, msg, replies, status, off, out = string_stream_call(self._client, [_key(key)], [0], [row])
        if rc != L.RBX_OK:
            if rc in (L.RBX_E_REDIS, L.RBX_E_WRONGTYPE) and int(status[0]) == STRING_FAILED:
                raise string_failure(self._client, _key(key), row)
            _check(rc)
        return int(replies[0]), out, int(status[0])

    @_pipelined(string=_string_get)
    def get(self, key: bytes):
        """GET key -> the bytes, None for a missing key  S:487-490"""
        _n, data, status = self._string_one(key, (L.RBX_STR_GET, 0, 0, b""))
        return None if status == STRING_NIL else data

    @_pipelined
    def set(self, key: bytes, value: bytes) -> bool:  # noqa: A003
        """SET key value  S:506-509: replaces the key whatever it held and drops its timeout"""
        nm, _keep = L.name_struct(_key(key))
        ptr, n, _buf = _u8(value)
        _check(L.lib().rbx_bitset_import_n(self._client.ctx, nm, ptr, n))
        return True

    def mGet(self, *keys: bytes) -> list:
        """MGET k1..kn  S:499-503: one rbx_string_stream call of GETs; a missing key and a key of another type are
        None, and nothing is raised for them.  While pipelined it queues itself as one command."""
        def run():
            ks = [_key(k) for k in keys]
            if not ks:
                return []
            rc, msg, _r, status, off, out = string_stream_call(self._client, ks, list(range(len(ks))),
                                                               [(L.RBX_STR_GET, 0, 0, b"")] * len(ks))
            if rc not in (L.RBX_OK, L.RBX_E_WRONGTYPE):
                _check(rc)
            return [out[int(off[i]): int(off[i + 1])] if int(status[i]) == 0 else None for i in range(len(ks))]
        if self._pipeline is not None:
            self._pipeline.append(_Queued(fn=run))
            return None
        return run()

    @_pipelined(string=_string_append)
    def append(self, key: bytes, value: bytes) -> int:
        """APPEND key value -> the new length  S:610-614"""
        return string_append(self._client, _key(key), value)

    @_pipelined(string=_string_get_range)
    def getRange(self, key: bytes, start: int, end: int) -> bytes:
        """GETRANGE key start end  S:617-621"""
        return string_getrange(self._client, _key(key), _int64(start), _int64(end))

    @_pipelined(string=_string_set_range)
    def setRange(self, key: bytes, value: bytes, offset: int) -> None:
        """SETRANGE key offset value  S:624-627 (void)"""
        string_setrange(self._client, _key(key), _int64(offset), value)

    m_get = mGet
    get_range = getRange
    set_range = setRange

    # ---- bit commands on strings (rbx_bitset_*, binary names) ---------------------------------
    @_pipelined(bit=lambda key, offset: (key, GETBIT, offset))
    def getBit(self, key: bytes, offset: int) -> bool:
        """GETBIT key offset  S:628-631"""
        nm, _keep = L.name_struct(_key(key))
        bit = C.c_int()
        _check(L.lib().rbx_bitset_get(self._client.ctx, nm, int(offset), C.byref(bit)))
        return bool(bit.value)

    @_pipelined(bit=lambda key, offset, value: (key, SETBIT1 if value else SETBIT0, offset))
    def setBit(self, key: bytes, offset: int, value: bool) -> bool:
        """SETBIT key offset value -> the bit before  S:633-636"""
        nm, _keep = L.name_struct(_key(key))
        old = C.c_int()
        _check(L.lib().rbx_bitset_set(self._client.ctx, nm, int(offset), int(bool(value)), C.byref(old)))
        return bool(old.value)

    @_pipelined(bitop=_bit_count_group, rng=_bit_count_range)
    def bitCount(self, key: bytes, begin: int | None = None, end: int | None = None) -> int:
        """BITCOUNT key  S:638-641, BITCOUNT key begin end  S:643-646 (bytes, both inclusive)"""
        nm, _keep = L.name_struct(_key(key))
        out = C.c_uint64()
        if begin is None and end is None:
            _check(L.lib().rbx_bitset_cardinality(self._client.ctx, nm, C.byref(out)))
        elif begin is None or end is None:
            raise IllegalArgumentException("bitCount takes both begin and end, or neither")
        else:
            _check(L.lib().rbx_bitset_count_range(self._client.ctx, nm, int(begin), int(end), L.RBX_RANGE_BYTE,
                                                  C.byref(out)))
        return int(out.value)

    @_pipelined(bitop=_bit_op_group)
    def bitOp(self, op, destination: bytes, *keys: bytes) -> int:
        """BITOP op destination k1..kn -> the result's length  S:650-661.  op: AND / OR / XOR / NOT (a name or
        an RBX_BITOP_* value).  NOT with more than one source fails before any command is sent (S:652-654)."""
        code = _bit_op_code(op, keys)
        dest, _keep_d = L.name_struct(_key(destination))
        srcs, _keep = L.names_array([_key(k) for k in keys])
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_op(self._client.ctx, code, dest, srcs, len(keys), C.byref(out)))
        return int(out.value)

    @_pipelined(rng=lambda key: (key, _range_row(L.RBX_RANGE_STRLEN), None))
    def strLen(self, key: bytes) -> int:
        """STRLEN key  S:663-666"""
        nm, _keep = L.name_struct(_key(key))
        out = C.c_uint64()
        _check(L.lib().rbx_bitset_size(self._client.ctx, nm, C.byref(out)))
        return int(out.value) // 8

    @_pipelined(field=lambda key, subCommands: _one_sub_command(key, subCommands))
    def bitField(self, key: bytes, subCommands) -> list:
        """BITFIELD key sub-commands -> one reply each, None for nil  S:2241-2291.  subCommands: BitFieldGet /
        BitFieldSet / BitFieldIncrBy in order.  A non-zero-based Offset is sent as '#N' = N * bits
        (S:2256-2260); the type travels as 'i' | 'u' + bits with no size check of Redisson's own (S:2262-2266),
        so u64 or i65 is Redis's "ERR Invalid bitfield type".  An INCRBY's overflow is appended after it
        (S:2272-2283) and so governs the sub-commands that follow (resolve_overflow).  An empty list returns []."""
        cmds = list(subCommands)
        if not cmds:
            return []
        arr = (L.RbxFieldCmd * len(cmds))()
        for a, cmd, mode in zip(arr, cmds, resolve_overflow(cmds)):
            a.op, a.is_signed, a.size, a.overflow, a.offset, a.value = _field_row(cmd, mode)
        replies = np.zeros(len(cmds), np.int64)
        nil = np.zeros(len(cmds), np.uint8)
        nm, _keep = L.name_struct(_key(key))
        _check(L.lib().rbx_bitset_bitfield(self._client.ctx, nm, arr, len(cmds), replies.ctypes.data_as(L.i64p),
                                           nil.ctypes.data_as(L.u8p)))
        return [None if z else int(r) for r, z in zip(replies, nil)]

    bit_field = bitField

    @_pipelined(rng=_bit_pos_range)
    def bitPos(self, key: bytes, bit: bool, range=(None, None)) -> int:
        """BITPOS key bit [lower [upper]]  S:2337-2359.  range = (lower, upper), each an int or None
        (Range.unbounded()).  As in the reference the upper bound is sent only when the lower one is bounded
        (S:2351-2356): (None, 5) is BITPOS key bit."""
        if range is None:
            raise IllegalArgumentException("Range must not be null! Use Range.unbounded() instead.")
        lower, upper = range
        nargs = 0 if lower is None else (1 if upper is None else 2)
        nm, _keep = L.name_struct(_key(key))
        out = C.c_int64()
        _check(L.lib().rbx_bitset_pos(self._client.ctx, nm, int(bool(bit)), nargs, int(lower or 0),
                                      int(upper or 0) if nargs == 2 else 0, L.RBX_RANGE_BYTE, C.byref(out)))
        return int(out.value)
