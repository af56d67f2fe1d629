"""Set-bit enumeration and the java.util.BitSet exchange without a GPU: the host-string entry points
rbx_bitset_members_of / rbx_bitset_as_words_of / rbx_bitset_bytes_of_words against members_model over every small
string, range and page, the length() / 8 + 1 rule at its edges, and the caller's errors."""
import ctypes as C
import itertools

import numpy as np
import pytest

import members_model as M
from redisson_amd import _lib as L

ALPHABET = (0x00, 0xFF, 0x08, 0xF7)
STRINGS = [bytes(t) for n in range(4) for t in itertools.product(ALPHABET, repeat=n)]  # b"" = an existing empty string
SENTINEL = 0xDEADBEEFDEADBEEF


def _buf(data):
    return (C.c_uint8 * max(len(data or b""), 1)).from_buffer_copy(data or b"\0")


def _members_of(data, nargs=0, start=0, end=0, unit=M.BYTE, skip=0, limit=M.ALL, cap=M.ALL, room=None):
    """(page, total); the page's array has `room` entries behind which nothing may be written"""
    cmd = L.RbxMembersCmd(start, end, skip, limit, nargs, unit)
    room = 8 * len(data or b"") if room is None else room
    out = np.full(room + 1, SENTINEL, np.uint64)
    written, total = C.c_uint64(77), C.c_uint64(77)
    rc = L.lib().rbx_bitset_members_of(_buf(data), len(data or b""), int(data is None), C.byref(cmd), cap,
                                       out.ctypes.data_as(L.u64p), C.byref(written), C.byref(total))
    assert rc == L.RBX_OK, (data, nargs, start, end, unit, skip, limit, cap, rc)
    assert written.value <= room and (out[written.value:] == SENTINEL).all()
    return out[: written.value].copy(), int(total.value)


def _count_of(data, start, end, unit):
    out = C.c_uint64(77)
    assert L.lib().rbx_bitset_count_of(_buf(data), len(data or b""), int(data is None), start, end, unit,
                                       C.byref(out)) == L.RBX_OK
    return int(out.value)


def test_model_known_answers():
    """a check of members_model.py itself (it calls nothing of the engine and passes without the feature)"""
    assert M.all_members(b"\x80\x01").tolist() == [0, 15]
    assert M.all_members(b"\xff", 2, 1, 2, M.BIT).tolist() == [1, 2]
    assert M.all_members(b"\xff\xff\xff", 2, -10, -20).size == 0  # BITCOUNT's pre-check
    assert M.all_members(None).size == 0 and M.all_members(b"").size == 0
    page, total = M.members(b"\xff", skip=3, limit=2)
    assert page.tolist() == [3, 4] and total == 8
    assert M.to_byte_array_reverse(0) == b"\0"
    assert M.to_byte_array_reverse(1 << 7) == b"\x01\x00" and M.to_byte_array_reverse(1 << 6) == b"\x02"
    assert M.from_byte_array_reverse(b"\x80\x01") == (1 << 0) | (1 << 15)


def test_members_of_every_small_string_and_range():
    for data in [None] + STRINGS:
        n = len(data or b"")
        whole, total = _members_of(data)
        assert np.array_equal(whole, M.all_members(data)) and total == whole.size, data
        for unit in (M.BYTE, M.BIT):
            t = 8 * n if unit == M.BIT else n
            for start in range(-(t + 4), t + 5):
                for end in range(-(t + 4), t + 5):
                    got, total = _members_of(data, 2, start, end, unit)
                    want = M.all_members(data, 2, start, end, unit)
                    assert np.array_equal(got, want), (data, start, end, unit)
                    assert total == want.size == _count_of(data, start, end, unit), (data, start, end, unit)


def test_members_of_every_page():
    cases = [(data, 0, 0, 0, M.BYTE) for data in [None] + STRINGS]
    cases += [(b"\xff\x08\xf7", 2, 3, -2, M.BIT), (b"\xf7\xff\x00", 2, 1, 1, M.BYTE), (b"\x08\x08\x08", 2, -20, 13, M.BIT)]
    for data, nargs, start, end, unit in cases:
        total = M.all_members(data, nargs, start, end, unit).size
        for skip in range(total + 2):
            for cap in range(total + 2):
                want, _ = M.members(data, nargs, start, end, unit, skip=skip, cap=cap)
                got, tot = _members_of(data, nargs, start, end, unit, skip=skip, cap=cap, room=cap)
                assert np.array_equal(got, want) and tot == total, (data, nargs, start, end, unit, skip, cap)
                got, tot = _members_of(data, nargs, start, end, unit, skip=skip, limit=cap)  # the same page by limit
                assert np.array_equal(got, want) and tot == total


def test_members_of_extreme_pages_do_not_wrap():
    data = b"\xff\x08"
    for skip, limit, cap in [(M.ALL, M.ALL, M.ALL), (1, M.ALL, M.ALL), (M.ALL - 1, 2, M.ALL), (3, M.ALL - 1, M.ALL),
                             (0, M.ALL, 4), (5, 3, M.ALL), (M.ALL, 0, 0)]:
        want, total = M.members(data, skip=skip, limit=limit, cap=cap)
        got, tot = _members_of(data, skip=skip, limit=limit, cap=cap)
        assert np.array_equal(got, want) and tot == total == 9, (skip, limit, cap)
    ext = 1 << 62
    for start, end in [(-(1 << 63), (1 << 63) - 1), (-ext, ext), ((1 << 63) - 1, (1 << 63) - 1), (-(1 << 63), -(1 << 63))]:
        for unit in (M.BYTE, M.BIT):
            got, tot = _members_of(data, 2, start, end, unit)
            assert np.array_equal(got, M.all_members(data, 2, start, end, unit)), (start, end, unit)


def test_members_of_count_only_and_errors():
    lib = L.lib()
    written, total = C.c_uint64(7), C.c_uint64(7)
    cmd = L.RbxMembersCmd(0, 0, 0, M.ALL, 0, 0)
    assert lib.rbx_bitset_members_of(_buf(b"\xff"), 1, 0, C.byref(cmd), 0, None, C.byref(written), C.byref(total)) == 0
    assert (written.value, total.value) == (0, 8)
    assert lib.rbx_bitset_members_of(_buf(b"\xff"), 1, 0, C.byref(cmd), 1, None, C.byref(written),
                                     C.byref(total)) == L.RBX_E_ILLEGAL_ARGUMENT  # NULL out with cap > 0
    out = np.zeros(8, np.uint64)
    for nargs, unit in [(1, 0), (3, 0), (255, 0), (0, 2), (2, 2), (2, 255)]:
        bad = L.RbxMembersCmd(0, 0, 0, M.ALL, nargs, unit)
        assert lib.rbx_bitset_members_of(_buf(b"\xff"), 1, 0, C.byref(bad), 8, out.ctypes.data_as(L.u64p),
                                         C.byref(written), C.byref(total)) == L.RBX_E_ILLEGAL_ARGUMENT, (nargs, unit)
    assert C.sizeof(L.RbxMembersCmd) == 40


# ---- the BitSet exchange ----
def _as_words_of(data, cap=None):
    n = C.c_uint64(77)
    assert L.lib().rbx_bitset_as_words_of(_buf(data), len(data), None, 0, C.byref(n)) == L.RBX_OK
    cap = n.value if cap is None else cap
    out = np.full(cap + 1, SENTINEL, np.uint64)
    n2 = C.c_uint64(77)
    assert L.lib().rbx_bitset_as_words_of(_buf(data), len(data), out.ctypes.data_as(L.u64p), cap, C.byref(n2)) == L.RBX_OK
    assert n2.value == n.value and (out[min(cap, n.value):] == SENTINEL).all()
    return out[: min(cap, n.value)].copy(), int(n.value)


def _bytes_of_words(words, cap=None):
    w = np.ascontiguousarray(np.asarray(words, np.uint64))
    p = (w if w.size else np.zeros(1, np.uint64)).ctypes.data_as(L.u64p)
    n = C.c_uint64(77)
    rc = L.lib().rbx_bitset_bytes_of_words(p, w.size, None, 0, C.byref(n))
    if rc != L.RBX_OK:
        return rc
    cap = n.value if cap is None else cap
    out = np.full(cap + 1, 0xA5, np.uint8)
    assert L.lib().rbx_bitset_bytes_of_words(p, w.size, out.ctypes.data_as(L.u8p), cap, C.byref(n)) == L.RBX_OK
    assert out[min(cap, n.value)] == 0xA5
    return out[: min(cap, n.value)].tobytes() if cap >= n.value else (out[:cap].tobytes(), int(n.value))


def _check_string(data):
    bs = M.from_byte_array_reverse(data)
    words, n = _as_words_of(data)
    want = M.to_long_array(bs)
    assert n == want.size and np.array_equal(words, want), data
    assert np.array_equal(M.as_words_fast(data), want), data
    stored = _bytes_of_words(words)
    assert stored == M.to_byte_array_reverse(bs) == M.bytes_of_words_fast(words), data
    back, _ = _as_words_of(stored)  # the round trip
    assert np.array_equal(back, want), data


def test_words_of_strings_with_one_or_two_set_bits():
    for n in range(18):
        _check_string(bytes(n))
        for i in range(8 * n):
            for j in ({i, 0, 8 * n - 1, (i + 63) % (8 * n), (i + 64) % (8 * n)} if n > 8 else range(i, 8 * n)):
                d = bytearray(n)
                d[i >> 3] |= 0x80 >> (i & 7)
                d[j >> 3] |= 0x80 >> (j & 7)
                _check_string(bytes(d))


def test_words_of_random_strings():
    rng = np.random.default_rng(0xB175E7)
    for n in list(range(1, 40)) + [255, 256, 257, 1000]:
        _check_string(rng.bytes(n))
        _check_string(rng.bytes(n) + bytes(int(rng.integers(0, 20))))  # zero bytes behind the last set bit


def test_words_length_rule_and_trailing_zero_words():
    for bit, nbytes in [(6, 1), (7, 2), (8, 2), (63, 8 + 1), (64, 9), (62, 8), (15, 3), (16, 3)]:
        words = M.to_long_array(1 << bit)
        got = _bytes_of_words(words)
        assert len(got) == nbytes == bit // 8 + 1 + (1 if bit % 8 == 7 else 0), bit
        assert got == M.to_byte_array_reverse(1 << bit)
        assert _bytes_of_words(list(words) + [0, 0, 0]) == got  # trailing zero words
    assert _bytes_of_words([]) == b"\0" and _bytes_of_words([0, 0]) == b"\0"  # the empty BitSet: one zero byte
    assert _as_words_of(b"")[1] == 0 and _as_words_of(b"\0\0\0")[1] == 0
    # a short output buffer gets the first bytes, and the length still comes back
    assert _bytes_of_words([1 | 1 << 63, 1], cap=3) == (b"\x80\x00\x00", 9)
    words, n = _as_words_of(b"\x80" + bytes(15) + b"\x01", cap=1)
    assert n == 3 and words.tolist() == [1]


def test_words_refuse_a_bit_java_cannot_count():
    w = np.zeros((1 << 25), np.uint64)
    w[-1] = 1 << 62  # bit 2^31 - 2: the last one length() can report
    got = _bytes_of_words(w, cap=0)
    assert got == (b"", (1 << 28))
    w[-1] = 1 << 63  # bit 2^31 - 1
    assert _bytes_of_words(w) == L.RBX_E_ILLEGAL_ARGUMENT
    with pytest.raises(OverflowError):
        M.to_byte_array_reverse(1 << 0x7FFFFFFF)
    assert _bytes_of_words(list(w[:4]) + [1]) == M.to_byte_array_reverse(1 << 256)
