"""Ranged BITCOUNT / BITPOS without a GPU: the model's known answers (the Redis command pages), the host-string
entry points rbx_bitset_count_of / rbx_bitset_pos_of against the model over every small range, the error
replies, and the new symbols' declarations."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import bitrange_model as M
from redisson_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {
    "rbx_bitset_count_range", "rbx_bitset_pos", "rbx_bitset_count_ranges", "rbx_bitset_pos_ranges",
    "rbx_bitset_count_ranges_dev", "rbx_bitset_pos_ranges_dev", "rbx_bitset_count_of", "rbx_bitset_pos_of",
}
ALPHABET = (0x00, 0xFF, 0x08, 0xF7)
STRINGS = [bytes(t) for n in range(4) for t in itertools.product(ALPHABET, repeat=n)]  # b"" = an existing empty string


def test_known_answers_of_the_command_pages():
    assert M.bitcount(b"foobar", 0, -1) == 26
    assert M.bitcount(b"foobar", 0, 0) == 4
    assert M.bitcount(b"foobar", 1, 1) == 6
    assert M.bitcount(b"foobar", 5, 30, M.BIT) == 17
    assert M.bitpos(b"\xff\xf0\x00", 0) == 12
    s = b"\x00\xff\xf0"
    assert M.bitpos(s, 1, 0) == 8
    assert M.bitpos(s, 1, 2) == 16
    assert M.bitpos(s, 1, 2, -1) == 16
    assert M.bitpos(s, 1, 7, 15, M.BIT) == 8
    assert M.bitpos(b"\0\0\0", 1) == -1
    assert M.bitpos(b"\0\0\0", 1, 7, -3, M.BIT) == -1
    assert M.bitpos(b"\xff\xff\xff", 0) == 24
    assert M.bitpos(b"\xff\xff\xff", 0, 0, -1) == -1
    assert M.bitpos(b"\xff\xff\xff", 0, 1) == 24
    # the pre-check is BITCOUNT's alone
    assert M.bitcount(b"\xff\xff\xff", -10, -20) == 0 and M.bitpos(b"\xff\xff\xff", 1, -10, -20) == 0
    # keys: missing, and existing but empty
    assert M.bitcount(None, 0, -1) == 0 and M.bitpos(None, 1) == -1 and M.bitpos(None, 0) == 0
    assert M.bitcount(b"", 0, -1) == 0 and M.bitpos(b"", 1) == -1 and M.bitpos(b"", 0) == -1


def _buf(data):
    return (C.c_uint8 * max(len(data or b""), 1)).from_buffer_copy(data or b"\0")


def _count_of(data, start, end, unit):
    out = C.c_uint64(77)
    rc = L.lib().rbx_bitset_count_of(_buf(data), len(data or b""), int(data is None), start, end, unit, C.byref(out))
    assert rc == L.RBX_OK, (data, start, end, unit, rc)
    return int(out.value)


def _pos_of(data, bit, nargs, start, end, unit):
    out = C.c_int64(77)
    rc = L.lib().rbx_bitset_pos_of(_buf(data), len(data or b""), int(data is None), bit, nargs, start, end, unit,
                                   C.byref(out))
    assert rc == L.RBX_OK, (data, bit, nargs, start, end, unit, rc)
    return int(out.value)


def test_the_batch_model_equals_the_scalar_model():
    """the cumulative forms the large expectations come from, against one slice per query"""
    rng = np.random.default_rng(5)
    for data in [None, b"", b"\x08", b"\xf7\x00", b"\xff\xff\xff", b"\x00\x00", rng.bytes(5)]:
        for unit in (M.BYTE, M.BIT):
            t = len(data or b"") * (8 if unit == M.BIT else 1)
            pairs = [(s, e) for s in range(-t - 4, t + 5) for e in range(-t - 4, t + 5)]
            starts, ends = [p[0] for p in pairs], [p[1] for p in pairs]
            assert M.count_ranges(data, starts, ends, unit).tolist() == [M.bitcount(data, s, e, unit) for s, e in pairs]
            for bit in (0, 1):
                assert M.pos_ranges(data, bit, starts, ends, unit).tolist() == \
                    [M.bitpos(data, bit, s, e, unit) for s, e in pairs]
                if unit == M.BYTE:
                    assert M.pos_ranges(data, bit, starts[:50]).tolist() == [M.bitpos(data, bit, s) for s in starts[:50]]


@pytest.mark.parametrize("unit", [M.BYTE, M.BIT])
def test_host_string_forms_equal_the_model_on_every_small_range(unit):
    for data in [None] + STRINGS:
        t = len(data or b"") * (8 if unit == M.BIT else 1)
        span = range(-t - 4, t + 5)
        pairs = [(s, e) for s in span for e in span]
        starts, ends = [p[0] for p in pairs], [p[1] for p in pairs]
        want = M.count_ranges(data, starts, ends, unit).tolist()
        assert [_count_of(data, s, e, unit) for s, e in pairs] == want, (data, unit)
        for bit in (0, 1):
            want = M.pos_ranges(data, bit, starts, ends, unit).tolist()
            assert [_pos_of(data, bit, 2, s, e, unit) for s, e in pairs] == want, (data, unit, bit)
            if unit == M.BYTE:  # a unit needs an end
                assert [_pos_of(data, bit, 1, s, 99, unit) for s in span] == M.pos_ranges(data, bit, list(span)).tolist()
                assert _pos_of(data, bit, 0, 99, 99, unit) == M.bitpos(data, bit)


def test_scalar_model_spot_checks_of_the_host_string_forms():
    """a sample straight against the slice-per-query model, nargs forms included"""
    rng = np.random.default_rng(6)
    for data in [None, b"", b"\x08\xf7\x00", b"\xff\xff\xff", rng.bytes(4)]:
        t = 8 * len(data or b"")
        for _ in range(300):
            s, e = (int(x) for x in rng.integers(-t - 4, t + 5, 2))
            unit, bit, nargs = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 3))
            assert _count_of(data, s, e, unit) == M.bitcount(data, s, e, unit)
            if nargs < 2:
                unit = M.BYTE
            assert _pos_of(data, bit, nargs, s, e, unit) == M.bitpos_nargs(data, bit, nargs, s, e, unit)


def test_error_replies():
    lib = L.lib()
    b, out, cnt = _buf(b"\xff"), C.c_int64(), C.c_uint64()
    for bit in (2, -1):
        assert lib.rbx_bitset_pos_of(b, 1, 0, bit, 0, 0, 0, M.BYTE, C.byref(out)) == L.RBX_E_REDIS
        assert L.last_error() == "ERR The bit argument must be 1 or 0."
    for nargs in (0, 1):  # a unit needs an end
        assert lib.rbx_bitset_pos_of(b, 1, 0, 1, nargs, 0, 0, M.BIT, C.byref(out)) == L.RBX_E_REDIS
        assert L.last_error() == "ERR syntax error"
    with pytest.raises(M.RedisError, match="syntax error"):
        M.bitpos(b"\xff", 1, 0, None, M.BIT)
    with pytest.raises(M.RedisError, match="must be 1 or 0"):
        M.bitpos(b"\xff", 2)
    E = L.RBX_E_ILLEGAL_ARGUMENT
    for unit in (2, -1):
        assert lib.rbx_bitset_pos_of(b, 1, 0, 1, 2, 0, 0, unit, C.byref(out)) == E
        assert lib.rbx_bitset_count_of(b, 1, 0, 0, 0, unit, C.byref(cnt)) == E
    for nargs in (3, -1):
        assert lib.rbx_bitset_pos_of(b, 1, 0, 1, nargs, 0, 0, M.BYTE, C.byref(out)) == E
    # NULL arguments, as the neighbouring calls refuse them; none of these reaches a device
    nm, _keep = L.name_struct("k")
    s = (C.c_int64 * 2)(0, 0)
    assert lib.rbx_bitset_count_of(None, 1, 0, 0, 0, M.BYTE, C.byref(cnt)) == E
    assert lib.rbx_bitset_count_of(b, 1, 0, 0, 0, M.BYTE, None) == E
    assert lib.rbx_bitset_pos_of(None, 1, 0, 1, 0, 0, 0, M.BYTE, C.byref(out)) == E
    assert lib.rbx_bitset_pos_of(b, 1, 0, 1, 0, 0, 0, M.BYTE, None) == E
    assert lib.rbx_bitset_count_range(None, nm, 0, 0, M.BYTE, C.byref(cnt)) == E
    assert lib.rbx_bitset_pos(None, nm, 1, 0, 0, 0, M.BYTE, C.byref(out)) == E
    assert lib.rbx_bitset_count_ranges(None, nm, s, s, 2, M.BYTE, C.cast(s, L.u64p)) == E
    assert lib.rbx_bitset_pos_ranges(None, nm, 1, s, s, 2, M.BYTE, s) == E
    assert lib.rbx_bitset_count_ranges_dev(None, nm, None, None, 2, M.BYTE, None, None) == E
    assert lib.rbx_bitset_pos_ranges_dev(None, nm, 1, None, None, 2, M.BYTE, None, None) == E
    assert "NULL" in L.last_error()
    # a missing key may come without bytes
    assert lib.rbx_bitset_pos_of(None, 0, 1, 0, 0, 0, 0, M.BYTE, C.byref(out)) == L.RBX_OK and out.value == 0
    assert lib.rbx_bitset_count_of(None, 0, 1, 0, -1, M.BYTE, C.byref(cnt)) == L.RBX_OK and cnt.value == 0


def test_symbols_units_and_knobs():
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rbx_bitset_[a-z0-9_]+)\s*\(", bare))
    assert ENTRY_POINTS <= declared, sorted(ENTRY_POINTS - declared)
    lib = L.lib()
    for s in sorted(ENTRY_POINTS):
        assert hasattr(lib, s) and s in L.SIGNATURES, s
    assert re.search(r"\bRBX_RANGE_BYTE = 0\b", bare) and re.search(r"\bRBX_RANGE_BIT = 1\b", bare)
    assert (L.RBX_RANGE_BYTE, L.RBX_RANGE_BIT) == (M.BYTE, M.BIT) == (0, 1)
    assert "RedissonConnection.java" in hdr and "S:2337-2359" in hdr and "S:638-646" in hdr
    assert lib.rbx_abi_version() == 1
    # the three knobs: documented, ranged, and back at their defaults
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    for key in ("bitrange_pos_chunk", "bitrange_chain_max", "bitrange_dir"):
        assert '"%s"' % key in bench, key
    for bad in (4095, 5000, 2048, 1 << 21):
        assert lib.rbx_tune(b"bitrange_pos_chunk", bad) == -1, bad
    assert lib.rbx_tune(b"bitrange_dir", 3) == -1 and lib.rbx_tune(b"bitrange_chain_max", -1) == -1
    for key, val in ((b"bitrange_pos_chunk", 4096), (b"bitrange_pos_chunk", 1 << 20), (b"bitrange_pos_chunk", 256 << 10),
                     (b"bitrange_dir", 0), (b"bitrange_dir", 1), (b"bitrange_dir", 2), (b"bitrange_chain_max", 128 << 10)):
        assert lib.rbx_tune(key, val) == 0, (key, val)


def test_batch_path_rule():
    """S > L + n * 8192 or M > bitrange_chain_max takes the directory, at the exact bytes; bitrange_dir 0 / 1
    override both"""
    lib = L.lib()
    path = lib.rbx_bench_bitrange_path
    length, n = 1 << 20, 5
    edge = length + n * 8192
    try:
        assert lib.rbx_tune(b"bitrange_chain_max", 9000) == 0
        assert path(length, n, edge, 9000) == 0 and path(length, n, edge + 1, 9000) == 1  # the bytes read
        assert path(length, n, 100, 9000) == 0 and path(length, n, 100, 9001) == 1  # the longest range
        assert path(length, n, 0, 0) == 0 and path(length, n + 1, edge + 1, 1) == 0  # 8 KiB more per query
        assert lib.rbx_tune(b"bitrange_chain_max", 0) == 0
        assert path(length, n, 1, 1) == 1 and path(length, n, 0, 0) == 0
        assert lib.rbx_tune(b"bitrange_dir", 0) == 0
        assert path(length, n, 1 << 40, 1 << 30) == 0
        assert lib.rbx_tune(b"bitrange_dir", 1) == 0
        assert path(length, n, 0, 0) == 1
    finally:
        assert lib.rbx_tune(b"bitrange_dir", 2) == 0 and lib.rbx_tune(b"bitrange_chain_max", 128 << 10) == 0
    assert path(length, n, 100, 128 << 10) == 0 and path(length, n, 100, (128 << 10) + 1) == 1  # the defaults
