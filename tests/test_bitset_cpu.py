"""RBitSet without a GPU: the rbx_bitset_* symbols are declared, exported and bound, NULL
arguments are refused before any device call, and rbx_bitset_length_of equals the Lua script of
RedissonBitSet.lengthAsync (M/RedissonBitSet.java:428-439) transcribed in bitset_model.lua_length."""
import ctypes as C
import os
import re

from bitset_model import lua_length
from redisson_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {
    "rbx_bitset_get", "rbx_bitset_set", "rbx_bitset_set_indexes", "rbx_bitset_get_indexes", "rbx_bitset_set_range",
    "rbx_bitset_op", "rbx_bitset_cardinality", "rbx_bitset_size", "rbx_bitset_length", "rbx_bitset_length_of",
    "rbx_bitset_export_n", "rbx_bitset_import_n", "rbx_bitset_set_indexes_dev", "rbx_bitset_get_indexes_dev",
}


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rbx_bitset_[a-z0-9_]+)\s*\(", hdr))
    assert ENTRY_POINTS <= declared, sorted(ENTRY_POINTS - declared)
    lib = L.lib()
    for s in sorted(declared):
        assert hasattr(lib, s), s
        assert s in L.SIGNATURES, s
    for op, v in (("AND", 0), ("OR", 1), ("XOR", 2), ("NOT", 3)):
        assert re.search(r"\bRBX_BITOP_%s = %d\b" % (op, v), hdr), op
        assert getattr(L, "RBX_BITOP_" + op) == v


def test_null_arguments_are_illegal_argument():
    lib = L.lib()
    nm, _keep = L.name_struct("k")
    bad = L.RbxName(None, 3)  # a length without bytes
    i, u, l64 = C.c_int(), C.c_uint64(), C.c_int64()
    idx = (C.c_uint64 * 2)(1, 2)
    out = (C.c_uint8 * 2)()
    E = L.RBX_E_ILLEGAL_ARGUMENT
    # no context (nothing here reaches a device)
    assert lib.rbx_bitset_get(None, nm, 0, C.byref(i)) == E
    assert lib.rbx_bitset_set(None, nm, 0, 1, C.byref(i)) == E
    assert lib.rbx_bitset_set_indexes(None, nm, idx, 2, 1) == E
    assert lib.rbx_bitset_get_indexes(None, nm, idx, 2, out) == E
    assert lib.rbx_bitset_set_indexes_dev(None, nm, None, 2, 1, None) == E
    assert lib.rbx_bitset_get_indexes_dev(None, nm, None, 2, None, None) == E
    assert lib.rbx_bitset_set_range(None, nm, 0, 8, 1) == E
    assert lib.rbx_bitset_op(None, L.RBX_BITOP_OR, nm, C.pointer(nm), 1, C.byref(u)) == E
    assert lib.rbx_bitset_cardinality(None, nm, C.byref(u)) == E
    assert lib.rbx_bitset_size(None, nm, C.byref(u)) == E
    assert lib.rbx_bitset_length(None, nm, C.byref(l64)) == E
    assert lib.rbx_bitset_export_n(None, nm, None, 0, C.byref(u)) == E
    assert lib.rbx_bitset_import_n(None, nm, out, 2) == E
    assert lib.rbx_bitset_rename(None, nm, nm) == E
    assert "NULL" in L.last_error()
    # the host-only entry point
    assert lib.rbx_bitset_length_of(None, 3, C.byref(l64)) == E
    assert lib.rbx_bitset_length_of(out, 2, None) == E
    assert bad.len == 3


def _length_of(data: bytes):
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = C.c_int64(-7)
    rc = L.lib().rbx_bitset_length_of(buf, len(data), C.byref(out))
    if rc == L.RBX_E_REDIS:
        assert "bit offset" in L.last_error()
        return None
    assert rc == L.RBX_OK, (data, rc)
    return int(out.value)


def test_length_of_empty_and_one_byte_strings():
    assert lua_length(b"") is None and _length_of(b"") is None
    fails = 0
    for b in range(256):
        s = bytes([b])
        want = lua_length(s)
        assert _length_of(s) == want, (b, want)
        fails += want is None
    assert fails == 1  # "\x00" alone
    # spot values: the highest set bit of the byte, + 1
    assert _length_of(b"\x80") == 1 and _length_of(b"\x01") == 8 and _length_of(b"\x48") == 5


def test_length_of_all_two_byte_strings():
    fails = []
    for v in range(65536):
        s = bytes([v >> 8, v & 0xFF])
        want = lua_length(s)
        assert _length_of(s) == want, (s, want)
        if want is None:
            fails.append(v)
    # the script fails exactly where the last byte is zero and bit 0 is clear ...
    assert fails == [h << 8 for h in range(0x80)]
    # ... and answers 1, whatever else the first byte holds, where bit 0 is set above a zero last byte
    assert all(lua_length(bytes([h, 0])) == 1 for h in range(0x80, 0x100))
