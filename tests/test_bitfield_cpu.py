"""BITFIELD without a GPU: the model (bitfield_model.py) against byte strings worked out by hand from
the reference's own tests, and the host-only rbx_bitset_field_of against the model.
T/ = /root/reference/redisson/src/test/java/org/redisson/"""
import ctypes as C
import random

import pytest

import bitfield_model as M
from redisson_amd import _lib as L


def run(data, *cmds):
    """cmds: (op, signed, size, offset, value) in order -> (string, replies)"""
    out = []
    for op, signed, size, offset, value in cmds:
        data, r = M.field(data, op, signed, size, offset, value)
        out.append(r)
    return data, out


def test_model_reference_vectors():
    # T/RedissonBitSetTest.java:15-57 assert the replies; the strings were computed by hand
    s, r = run(b"", (M.SET, False, 8, 1, 120))  # testUnsigned
    assert (s, r) == (bytes.fromhex("3c00"), [0])
    s, r = run(s, (M.INCRBY, False, 8, 1, 1), (M.GET, False, 8, 1, 0))
    assert r == [121, 121]
    s, r = run(b"", (M.SET, True, 8, 1, -120))  # testSigned
    assert (s, r) == (bytes.fromhex("4400"), [0])
    s, r = run(s, (M.INCRBY, True, 8, 1, 1), (M.GET, True, 8, 1, 0))
    assert (s, r) == (bytes.fromhex("4480"), [-119, -119])
    s, r = run(b"", (M.SET, True, 8, 2, 12), (M.GET, True, 8, 2, 0))  # testIncrement
    assert (s, r) == (bytes.fromhex("0300"), [0, 12])
    s, r = run(s, (M.INCRBY, True, 8, 2, 12), (M.GET, True, 8, 2, 0))
    assert (s, r) == (bytes.fromhex("0600"), [24, 24])
    s, r = run(b"", (M.SET, True, 16, 2, 2312), (M.GET, True, 16, 2, 0))  # testSetGetNumber
    assert (s, r) == (bytes.fromhex("024200"), [0, 2312])
    s, r = run(b"", (M.SET, True, 32, 2, 323241), (M.GET, True, 32, 2, 0))
    assert (s, r) == (bytes.fromhex("00013baa40"), [0, 323241])
    s, r = run(b"", (M.SET, True, 64, 2, 12), (M.GET, True, 64, 2, 0))
    assert (s, r) == (bytes(7) + bytes.fromhex("0300"), [0, 12]) and len(s) == 9


def test_model_wraps_and_growth():
    assert run(b"\xff", (M.INCRBY, False, 8, 0, 1)) == (b"\x00", [0])
    assert run(b"\x7f", (M.INCRBY, True, 8, 0, 1)) == (b"\x80", [-128])
    assert run(b"\x01", (M.INCRBY, False, 8, 0, -2)) == (b"\xff", [255])
    assert run(b"", (M.SET, False, 4, 4, 0x1F5), (M.GET, False, 4, 4, 0)) == (b"\x05", [0, 5])
    assert run(b"", (M.INCRBY, False, 3, 30, 0)) == (bytes(5), [0])  # INCRBY 0 creates and grows
    assert run(b"\xab", (M.GET, True, 24, 100, 0)) == (b"\xab", [0])  # GET grows nothing
    s, r = M.fields(b"\xfe", M.INCRBY, False, 8, [0, 0, 0], [1, 1, 1])
    assert (s, r) == (b"\x01", [255, 0, 1])
    s, r = M.fields(b"\x03", M.SET, False, 8, [0, 0], [5, 9])
    assert (s, r) == (b"\x09", [3, 5])
    with pytest.raises(M.RedisError):
        M.fields(b"", M.SET, False, 8, [0, 1 << 32], [1, 1])


def field_of(data: bytes, signed: bool, size: int, offset: int):
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    out = C.c_int64(-12345)
    rc = L.lib().rbx_bitset_field_of(buf, len(data), int(signed), size, offset, C.byref(out))
    return rc, int(out.value)


def test_field_of_matches_model():
    rng = random.Random(64)
    strings = [bytes(rng.randrange(256) for _ in range(n)) for n in range(4) for _ in range(16)]
    for data in strings:
        for size in (1, 5, 8, 13, 24):
            for signed in (False, True):
                for offset in range(25):
                    want = M.field(data, M.GET, signed, size, offset)[1]
                    assert field_of(data, signed, size, offset) == (0, want), (data, signed, size, offset)


def test_field_of_wide_types():
    data = bytes(range(0x80, 0x92))
    for signed, size in ((True, 64), (False, 63), (True, 33), (False, 32)):
        for offset in (0, 1, 7, 9, 63, 64, 100, 143, 200):
            want = M.field(data, M.GET, signed, size, offset)[1]
            assert field_of(data, signed, size, offset) == (0, want), (signed, size, offset)


def test_field_of_argument_errors():
    assert field_of(b"\x01", True, 0, 0)[0] == L.RBX_E_REDIS
    assert "Invalid bitfield type" in L.last_error()
    assert field_of(b"\x01", False, 0, 0)[0] == L.RBX_E_REDIS
    assert field_of(b"\x01", False, 64, 0)[0] == L.RBX_E_ILLEGAL_ARGUMENT
    assert "Size can't be greater than 63 bits" in L.last_error()
    assert field_of(b"\x01", True, 65, 0)[0] == L.RBX_E_ILLEGAL_ARGUMENT
    assert "Size can't be greater than 64 bits" in L.last_error()
    assert field_of(b"\x01", True, 8, 1 << 32)[0] == L.RBX_E_REDIS
    assert "bit offset is not an integer or out of range" in L.last_error()
    assert field_of(b"\x01", True, 8, (1 << 32) - 7)[0] == L.RBX_E_REDIS  # the field's last bit past the limit
    assert field_of(b"\x01", True, 8, (1 << 32) - 8) == (0, 0)
    assert field_of(b"\x01", False, 63, 0)[0] == 0 and field_of(b"\x01", True, 64, 0)[0] == 0
