"""BITFIELD's overflow rule without a GPU: rbx_bitset_field_rule (field_rule.h, the one function the kernels
and the host share) against the big-integer model of bitfield_overflow_model.py, and the mode resolution of
RedissonConnection.bitField, which needs no library."""
import ctypes as C
import os
import re

import pytest

import bitfield_overflow_model as M
from redisson_amd import _lib as L
from redisson_amd.spring_data import (BitFieldGet, BitFieldIncrBy, BitFieldSet, BitFieldType, Offset,
                                      resolve_overflow)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = M.I64_MIN, M.I64_MAX
EDGES = [I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX]
MODES = (M.WRAP, M.SAT, M.FAIL)


def engine(op, signed, size, mode, old, value):
    now, reply, nil = C.c_int64(), C.c_int64(), C.c_int(7)
    rc = L.lib().rbx_bitset_field_rule(op, int(signed), size, mode, old, value, C.byref(now), C.byref(reply),
                                       C.byref(nil))
    assert rc == L.RBX_OK, L.last_error()
    assert nil.value in (0, 1)
    if nil.value:
        assert reply.value == 0
    return now.value, (None if nil.value else reply.value)


def compare(op, signed, size, mode, old, value):
    assert engine(op, signed, size, mode, old, value) == M.rule(op, signed, size, mode, old, value), \
        (op, signed, size, mode, old, value)


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5])
def test_rule_exhaustively_on_small_types(size):
    values = list(range(-(1 << size) - 2, (1 << size) + 3)) + EDGES
    for signed in (False, True):
        lo, hi = M.bounds(signed, size)
        for op in (M.SET, M.INCRBY):
            for mode in MODES:
                for old in range(lo, hi + 1):
                    for value in values:
                        compare(op, signed, size, mode, old, value)


@pytest.mark.parametrize("size,signed", [(s, sg) for s in (8, 31, 32, 33, 63) for sg in (False, True)] + [(64, True)])
def test_rule_at_the_edges_of_wide_types(size, signed):
    lo, hi = M.bounds(signed, size)
    olds = sorted({o for o in (lo, lo + 1, -1, 0, 1, hi - 1, hi) if lo <= o <= hi})
    values = sorted({v for v in (I64_MIN, I64_MIN + 1, -hi - 1, -hi, -1, 0, 1, hi, hi + 1, I64_MAX - 1, I64_MAX)
                     if I64_MIN <= v <= I64_MAX})
    assert len(olds) >= 4 and len(values) >= 7
    for op in (M.SET, M.INCRBY, M.GET):
        for mode in MODES:
            for old in olds:
                for value in values:
                    compare(op, signed, size, mode, old, value)


def test_unsigned_set_of_a_negative_value_overflows_upwards():
    for size in (1, 4, 8, 63):
        hi = (1 << size) - 1
        assert engine(M.SET, False, size, M.SAT, 3 & hi, -1) == (hi, 3 & hi)  # stores hi, not 0
        assert engine(M.SET, False, size, M.FAIL, 3 & hi, -1) == (3 & hi, None)
        assert engine(M.SET, False, size, M.WRAP, 0, -1) == (hi, 0)
    assert engine(M.SET, True, 8, M.SAT, 0, -1) == (-1, 0) and engine(M.SET, True, 8, M.SAT, 0, -300) == (-128, 0)
    # the counting-filter cases of DESIGN 11.1: the 16th increment of a u4, a decrement of an empty slot
    assert engine(M.INCRBY, False, 4, M.SAT, 15, 1) == (15, 15) and engine(M.INCRBY, False, 4, M.WRAP, 15, 1) == (0, 0)
    assert engine(M.INCRBY, False, 4, M.SAT, 0, -1) == (0, 0) and engine(M.INCRBY, False, 4, M.WRAP, 0, -1) == (15, 15)
    assert engine(M.INCRBY, True, 64, M.SAT, I64_MAX, I64_MAX) == (I64_MAX, I64_MAX)
    assert engine(M.INCRBY, True, 64, M.FAIL, I64_MIN, -1) == (I64_MIN, None)


def test_rule_argument_checks():
    lib = L.lib()
    now, reply, nil = C.c_int64(), C.c_int64(), C.c_int()
    out = (C.byref(now), C.byref(reply), C.byref(nil))
    E = L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_bitset_field_rule(M.INCRBY, 0, 8, 3, 0, 1, *out) == E and "OVERFLOW" in L.last_error()
    assert lib.rbx_bitset_field_rule(M.INCRBY, 0, 8, -1, 0, 1, *out) == E
    assert lib.rbx_bitset_field_rule(3, 0, 8, 0, 0, 1, *out) == E
    assert lib.rbx_bitset_field_rule(M.SET, 0, 8, 0, 256, 1, *out) == E  # old outside u8
    assert lib.rbx_bitset_field_rule(M.SET, 1, 8, 0, 128, 1, *out) == E
    assert lib.rbx_bitset_field_rule(M.SET, 0, 8, 0, 0, 1, None, None, None) == E
    for signed, size in ((0, 64), (1, 65), (0, 0), (1, 0)):
        assert lib.rbx_bitset_field_rule(M.SET, signed, size, 0, 0, 1, *out) == L.RBX_E_REDIS
        assert "Invalid bitfield type" in L.last_error()


def test_symbols_modes_and_the_knob():
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.lib()
    for s in ("rbx_bitset_fields_ov", "rbx_bitset_fields_ov_dev", "rbx_bitset_bitfield", "rbx_bitset_field_rule"):
        assert re.search(r"\b%s\s*\(" % s, bare) and hasattr(lib, s) and s in L.SIGNATURES, s
    assert re.search(r"RBX_OVERFLOW_WRAP = 0, RBX_OVERFLOW_SAT = 1, RBX_OVERFLOW_FAIL = 2", bare)
    assert (L.RBX_OVERFLOW_WRAP, L.RBX_OVERFLOW_SAT, L.RBX_OVERFLOW_FAIL) == (M.WRAP, M.SAT, M.FAIL) == (0, 1, 2)
    assert C.sizeof(L.RbxFieldCmd) == 24 and L.RbxFieldCmd.value.offset == 8 and L.RbxFieldCmd.op.offset == 16
    assert "S:2241-2291" in hdr and lib.rbx_abi_version() == 1
    assert '"bitfield_sat_atomic"' in open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    assert lib.rbx_tune(b"bitfield_sat_atomic", 2) == -1 and lib.rbx_tune(b"bitfield_sat_atomic", -1) == -1
    assert lib.rbx_tune(b"bitfield_sat_atomic", 0) == 0 and lib.rbx_tune(b"bitfield_sat_atomic", 1) == 0


# ---- the mode resolution of RedissonConnection.bitField (no library) ---------------------------
def run_resolved(data: bytes, cmds):
    """the sub-commands under their resolved modes, through the model"""
    names = {"WRAP": M.WRAP, "SAT": M.SAT, "FAIL": M.FAIL}
    ops = {BitFieldGet: M.GET, BitFieldSet: M.SET, BitFieldIncrBy: M.INCRBY}
    rows = []
    for cmd, mode in zip(cmds, resolve_overflow(cmds)):
        off = cmd.offset.value if cmd.offset.zero_based else cmd.offset.value * cmd.type.bits
        rows.append((ops[type(cmd)], cmd.type.signed, cmd.type.bits, names[mode], off, getattr(cmd, "value", 0)))
    return M.bitfield(data, rows)


def test_overflow_applies_to_the_sub_commands_that_follow():
    u8, i5 = BitFieldType(False, 8), BitFieldType(True, 5)
    assert (u8.asString(), i5.asString()) == ("u8", "i5")
    assert Offset(3).asString() == "3" and Offset(3, zero_based=False).asString() == "#3"
    assert resolve_overflow([]) == []
    # the quirk: the mode is appended AFTER the INCRBY that carries it
    two = [BitFieldIncrBy(u8, 0, 200, "SAT"), BitFieldIncrBy(u8, 0, 100)]
    assert resolve_overflow(two) == ["WRAP", "SAT"]
    assert run_resolved(b"", two) == (b"\xff", [200, 255])  # 255, not 44
    lone = [BitFieldIncrBy(u8, 0, 300, "SAT")]
    assert resolve_overflow(lone) == ["WRAP"]
    assert run_resolved(b"", lone) == (b"\x2c", [44])
    # a mode stays until the next INCRBY that carries one; GET and SET carry none but SET obeys it
    many = [BitFieldIncrBy(u8, 0, 1, "FAIL"), BitFieldSet(u8, 0, 256), BitFieldGet(u8, 0),
            BitFieldIncrBy(u8, 0, 255, "sat"), BitFieldIncrBy(u8, 0, 255), BitFieldIncrBy(u8, 0, 1, "WRAP"),
            BitFieldIncrBy(u8, 0, 1)]
    assert resolve_overflow(many) == ["WRAP", "FAIL", "FAIL", "FAIL", "SAT", "SAT", "WRAP"]
    assert run_resolved(b"", many) == (b"\x00", [1, None, 1, None, 255, 255, 0])
    # '#N' is N * bits
    assert run_resolved(b"", [BitFieldSet(i5, Offset(2, zero_based=False), -1), BitFieldGet(i5, 10)]) == \
        (b"\x00\x3e", [0, -1])
    with pytest.raises(Exception, match="OVERFLOW"):
        BitFieldIncrBy(u8, 0, 1, "CLAMP")
