"""The byte-level string commands without a GPU: the model's GETRANGE (bytestream_model) against brute-force Python
slicing and rbx_string_range_of against the model, for every string length 0..5 and every start and end in
[-len - 2, len + 2] plus the ends of int64_t; SETRANGE and APPEND at offsets and lengths around the 2^29 limit (no
such buffer is allocated: the call answers from the lengths alone); every failure kind and the order they are looked
at in; the model's stream as n single calls; the truncate script's quirks; the symbols and the knobs."""
import ctypes as C
import itertools

import pytest

import bytestream_model as M
from redisson_amd import _lib as L

INT64_MIN, INT64_MAX = M.INT64_MIN, M.INT64_MAX
KMAX = M.KMAX
MSG = {M.OFFSET: "ERR offset is out of range", M.WRONGTYPE: "WRONGTYPE",
       M.TOO_BIG: "ERR string exceeds maximum allowed size (proto-max-bulk-len)"}
CODE = {M.OFFSET: L.RBX_E_REDIS, M.TOO_BIG: L.RBX_E_REDIS, M.WRONGTYPE: L.RBX_E_WRONGTYPE}


def range_of(data, missing, op, a=0, b=0, val_len=0, cap=None, length=None):
    """rbx_string_range_of -> (rc, message, reply, new_len, bytes read)"""
    n = len(data) if length is None else length
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0") if length is None else None
    cmd = L.RbxStringCmd(a=a, b=b, val_off=0, val_len=val_len, op=op)
    cap = (n if length is None else 0) if cap is None else cap
    out = (C.c_uint8 * max(1, cap))(*([0xEE] * max(1, cap)))
    reply, new_len = C.c_int64(-7), C.c_uint64(7)
    rc = L.lib().rbx_string_range_of(buf, n, int(missing), C.byref(cmd), None, out, cap, C.byref(reply), C.byref(new_len))
    got = bytes(out[:max(0, min(cap, reply.value))]) if rc == 0 and op in (M.GETRANGE, M.GET) else None
    return rc, L.last_error() if rc else "", reply.value, new_len.value, got


def brute_getrange(s, start, end):
    """GETRANGE as a filter over positions: no clamping arithmetic to get wrong"""
    n = len(s)
    if start < 0 and end < 0 and start > end:
        return b""
    lo = start if start >= 0 else n + start
    hi = end if end >= 0 else n + end
    if hi < 0:  # a negative end clamps to 0: position 0 stays in reach
        hi = 0
    return bytes(s[p] for p in range(n) if lo <= p <= hi)


def grid(n):
    return list(range(-n - 2, n + 3)) + [INT64_MIN, INT64_MAX]


def test_getrange_model_against_slicing_and_of_against_model():
    for n in range(6):
        s = bytes(range(0x41, 0x41 + n))
        for start, end in itertools.product(grid(n), grid(n)):
            want = M.getrange_of(s, start, end)
            assert want == brute_getrange(s, start, end), (n, start, end)
            for missing in (0, 1):
                rc, _m, reply, new_len, got = range_of(s, missing, M.GETRANGE, start, end)
                w = b"" if missing else want
                assert (rc, reply, got, new_len) == (0, len(w), w, 0 if missing else n), (n, start, end, missing)


def test_getrange_cap_and_get():
    s = b"hello world"
    rc, _m, reply, _n, got = range_of(s, 0, M.GETRANGE, 2, -2, cap=3)
    assert (rc, reply, got) == (0, 8, b"llo")  # min(cap, reply) bytes are written
    assert range_of(s, 0, M.GET)[2:] == (11, 11, s)
    assert range_of(b"", 0, M.GET)[2:] == (0, 0, b"")   # the empty string is not nil
    rc, _m, reply, _n, _g = range_of(b"", 1, M.GET)
    assert (rc, reply) == (0, -1)                       # a missing key is


def model_write(data, missing, op, a, v):
    """the model on a string of len(data) bytes -> (kind or None, reply, new length)"""
    ks = M.Strings()
    if not missing:
        ks.data["k"] = bytearray(data)
    try:
        n = ks.setrange("k", a, bytes(v)) if op == M.SETRANGE else ks.append("k", bytes(v))
        return None, n, ks.strlen("k")
    except M.Failed as e:
        return e.kind, 0, ks.strlen("k")


def test_setrange_append_small_against_model():
    for n, missing in [(0, 1), (0, 0), (1, 0), (5, 0)]:
        s = bytes(range(n))
        for v in (0, 1, 3):
            for a in list(range(-2, n + 4)) + [INT64_MIN, INT64_MAX]:
                kind, reply, new = model_write(s, missing, M.SETRANGE, a, v)
                rc, msg, r, nl, _ = range_of(s, missing, M.SETRANGE, a, 0, v)
                assert (rc, r, nl) == (CODE.get(kind, 0), reply, new), (n, missing, v, a)
                assert (MSG[kind] in msg) if kind else msg == ""
            kind, reply, new = model_write(s, missing, M.APPEND, 0, v)
            assert range_of(s, missing, M.APPEND, INT64_MIN, INT64_MAX, v)[:4] == (0, "", reply, new)


class Lengths(M.Strings):
    """the model's rules on a string known by its length alone (no 512 MiB value is built)"""

    def write(self, length, missing, op, a, v):
        if op == M.SETRANGE:
            if a < 0:
                return M.OFFSET, 0, length
            if v == 0:
                return None, length, length
            if a + v > KMAX:
                return M.TOO_BIG, 0, length
            return None, max(length, a + v), max(length, a + v)
        if (0 if missing else length) + v > KMAX:
            return M.TOO_BIG, 0, length
        return None, length + v, length + v


def test_setrange_append_around_the_limit():
    rules = Lengths()
    for length in (0, 1, KMAX - 2, KMAX - 1, KMAX):
        for v in (0, 1, 2, 3, (1 << 32) - 1):
            for a in (0, 1, KMAX - 3, KMAX - 2, KMAX - 1, KMAX, KMAX + 1, INT64_MAX - 1, INT64_MAX, -1, INT64_MIN):
                kind, reply, new = rules.write(length, False, M.SETRANGE, a, v)
                rc, msg, r, nl, _ = range_of(b"", 0, M.SETRANGE, a, 0, v, length=length)
                assert (rc, r, nl) == (CODE.get(kind, 0), reply, new), (length, v, a)
                assert (MSG[kind] in msg) if kind else msg == ""
            kind, reply, new = rules.write(length, False, M.APPEND, 0, v)
            rc, msg, r, nl, _ = range_of(b"", 0, M.APPEND, 0, 0, v, length=length)
            assert (rc, r, nl) == (CODE.get(kind, 0), reply, new), (length, v)
    # the small cases of the length-only rules are the model's
    for length, v, a in itertools.product((0, 1, 4), (0, 1, 2), (-1, 0, 1, 3, 6)):
        assert rules.write(length, False, M.SETRANGE, a, v) == model_write(bytes(length), 0, M.SETRANGE, a, v)
    # a GETRANGE at the limit reads by the same rule (the bytes themselves: the GPU tests)
    rc, _m, reply, _nl, _g = range_of(b"", 0, M.GETRANGE, INT64_MIN, INT64_MAX, cap=0, length=0)
    assert (rc, reply) == (0, 0)


def test_caller_errors_of():
    lib = L.lib()
    reply = C.c_int64()
    cmd = L.RbxStringCmd(op=4)
    assert lib.rbx_string_range_of(None, 0, 0, C.byref(cmd), None, None, 0, C.byref(reply), None) == L.RBX_E_ILLEGAL_ARGUMENT
    cmd.op = M.GET
    assert lib.rbx_string_range_of(None, 0, 0, None, None, None, 0, C.byref(reply), None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_string_range_of(None, 0, 0, C.byref(cmd), None, None, 0, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_string_range_of(None, KMAX + 1, 0, C.byref(cmd), None, None, 0, C.byref(reply), None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_string_range_of(None, 3, 0, C.byref(cmd), None, None, 0, C.byref(reply), None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_string_range_of(None, 0, 0, C.byref(cmd), None, None, 0, C.byref(reply), None) == 0  # new_len nullable


def test_model_failure_kinds_and_their_order():
    ks = M.Strings()
    ks.other.add("hll")
    ks.data["s"] = bytearray(b"abc")
    ks.timeout.add("s")
    for call, kind in [(lambda: ks.setrange("hll", -1, b"x"), M.OFFSET),       # the offset before the key's type
                       (lambda: ks.setrange("hll", KMAX, b"x"), M.WRONGTYPE),  # the type before the size
                       (lambda: ks.setrange("hll", 0, b""), M.WRONGTYPE),
                       (lambda: ks.setrange("s", KMAX, b"x"), M.TOO_BIG),
                       (lambda: ks.setrange("s", -1, b""), M.OFFSET),
                       (lambda: ks.append("hll", b""), M.WRONGTYPE),
                       (lambda: ks.getrange("hll", 0, -1), M.WRONGTYPE),
                       (lambda: ks.get("hll"), M.WRONGTYPE),
                       (lambda: ks.truncate("hll", 0), M.WRONGTYPE)]:
        with pytest.raises(M.Failed) as e:
            call()
        assert e.value.kind == kind
    assert ks.setrange("s", KMAX, b"") == 3 and ks.setrange("missing", KMAX + 5, b"") == 0  # no size check, no key
    assert not ks.exists("missing") and ks.mget(["s", "hll", "missing"]) == [b"abc", None, None]
    assert ks.append("new", b"") == 0 and ks.get("new") == b"" and ks.exists("new")  # APPEND creates the empty string
    assert ks.getrange("missing", 0, -1) == b"" and ks.get("missing") is None
    assert ks.setrange("s", 5, b"Z") == 6 and ks.get("s") == b"abc\0\0Z" and ks.ttl("s") == "set"
    assert ks.append("s", b"!") == 7 and ks.ttl("s") == "set"
    ks.set("hll", b"now a string")
    assert ks.get("hll") == b"now a string"


def test_model_truncate_quirks():
    ks = M.Strings()
    ks.data["k"] = bytearray(b"0123456789")
    ks.timeout.add("k")
    ks.truncate("k", 10)
    assert ks.get("k") == b"0123456789" and ks.ttl("k") == "set"   # size >= len: nothing, the timeout stays
    ks.truncate("k", 0)
    assert ks.get("k") == b"0123456789" and ks.ttl("k") == "none"  # GETRANGE 0 -1: the content stays, the timeout goes
    ks.truncate("k", 4)
    assert ks.get("k") == b"0123"
    ks.truncate("k", -1)
    assert ks.get("k") == b"012"                                   # GETRANGE 0 -2
    ks.truncate("k", -9)
    assert ks.get("k") == b"0" and ks.exists("k")                  # both ends clamp to 0: one byte stays
    ks.truncate("missing", 0)
    assert not ks.exists("missing")
    ks.truncate("missing", -1)
    assert ks.get("missing") == b""                                # SET key "" creates the empty string


def test_model_stream_is_n_single_calls():
    ks = M.Strings()
    ks.other.add("hll")
    ks.data["a"] = bytearray(b"abcdef")
    names = ["a", "b", "hll", "a"]
    vals = b"XYZ0123456789"
    cmds = [(M.SETRANGE, 2, 0, 0, 3), (M.GETRANGE, 0, -1, 0, 0), (M.APPEND, 0, 0, 3, 2), (M.GET, 0, 0, 0, 0),
            (M.SETRANGE, -1, 0, 0, 1), (M.APPEND, 0, 0, 0, 1), (M.GET, 0, 0, 0, 0), (M.GETRANGE, -2, -1, 0, 0),
            (M.APPEND, 0, 0, 5, 2)]
    keys = [0, 3, 0, 1, 1, 2, 2, 0, 1]
    r = ks.stream(names, keys, cmds, vals, 100)
    assert r["kind"] == M.OFFSET  # the first failure in array order
    assert r["replies"] == [6, 6, 8, 0, 0, 0, 0, 2, 2]
    assert r["status"] == [0, 0, 0, M.NIL, M.FAILED, M.FAILED, M.FAILED, 0, 0]
    assert r["out"] == b"abXYZf" + b"01" and r["off"] == [0, 0, 6, 6, 6, 6, 6, 6, 8, 8] and r["total"] == 8
    assert ks.get("a") == b"abXYZf01" and ks.get("b") == b"23"
    # total > cap: refused before any write, off and total exact; the caller's errors change nothing either
    before = (dict(ks.data), set(ks.timeout))
    r = ks.stream(names, [0, 0], [(M.APPEND, 0, 0, 0, 3), (M.GET, 0, 0, 0, 0)], vals, 10)
    assert r["kind"] == M.ILLEGAL and r["off"] == [0, 0, 11] and r["total"] == 11 and ks.get("a") == b"abXYZf01"
    for bad_keys, bad in [([4], [(M.GET, 0, 0, 0, 0)]), ([0], [(4, 0, 0, 0, 0)]), ([0], [(M.APPEND, 0, 0, 12, 2)]),
                          ([0], [(M.SETRANGE, 0, 0, 14, 0)])]:
        assert ks.stream(names, bad_keys, bad, vals, 100)["kind"] == M.ILLEGAL
    assert (dict(ks.data), set(ks.timeout)) == before
    # a key whose only writes failed is not created; a value slice may be empty at the buffer's end
    r = ks.stream(["c"], [0, 0], [(M.SETRANGE, -5, 0, 0, 1), (M.SETRANGE, KMAX, 0, 13, 0)], vals, 0)
    assert r["kind"] == M.OFFSET and r["replies"] == [0, 0] and not ks.exists("c")


def test_symbols_struct_and_knobs():
    lib = L.lib()
    assert C.sizeof(L.RbxStringCmd) == 32
    for sym in ("rbx_string_getrange", "rbx_string_setrange", "rbx_string_append", "rbx_string_truncate",
                "rbx_string_getrange_dev", "rbx_string_setrange_dev", "rbx_string_append_dev", "rbx_string_stream",
                "rbx_string_stream_dev", "rbx_string_range_of", "rbx_bench_bytestream_last"):
        assert hasattr(lib, sym), sym
    good = {b"bytestream_lanes": (4, 8, 16, 32, 64), b"bytestream_short_max": (64, 4096, 1 << 20),
            b"bytestream_tile": (4096, 65536, 1 << 20), b"bytestream_chunk": (1, 7, 1 << 30),
            b"bytestream_serial_max": (0, 64, 1000)}
    bad = {b"bytestream_lanes": (0, 2, 12, 128), b"bytestream_short_max": (32, 100, 1 << 21),
           b"bytestream_tile": (2048, 5000, 1 << 21), b"bytestream_chunk": (0, (1 << 30) + 1),
           b"bytestream_serial_max": (-1,)}
    default = {b"bytestream_lanes": 16, b"bytestream_short_max": 4096, b"bytestream_tile": 65536,
               b"bytestream_chunk": 1 << 25, b"bytestream_serial_max": 64}
    try:
        for key, values in good.items():
            for v in values:
                assert lib.rbx_tune(key, v) == 0, (key, v)
        for key, values in bad.items():
            for v in values:
                assert lib.rbx_tune(key, v) == L.RBX_E_ILLEGAL_ARGUMENT, (key, v)
    finally:
        for key, v in default.items():
            assert lib.rbx_tune(key, v) == 0
    assert lib.rbx_bench_bytestream_last(None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_abi_version() == 1
