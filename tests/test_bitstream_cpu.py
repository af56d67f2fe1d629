"""The ordered GETBIT / SETBIT stream without a GPU: the model of bitstream_model.py against cases worked out
by hand, the two new C-ABI symbols, the tunables, and RBatch's queue with the engine calls replaced by
recording stubs."""
import os
import re

import pytest

import bitstream_model as M
from redisson_amd import IllegalStateException, RBatch, RedisException
from redisson_amd import _lib as L
from redisson_amd.client import GETBIT, SETBIT0, SETBIT1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, S0, S1 = M.GETBIT, M.SETBIT0, M.SETBIT1


# ---- the model ---------------------------------------------------------------------------------------
def test_model_one_bit_in_order():
    m = M.StreamModel()
    rc, rep = m.run([b"a"], [0] * 7, [G, S1, G, S1, S0, G, S1], [5] * 7)
    assert rc == M.OK and rep == [0, 0, 1, 1, 1, 0, 0]
    assert m.strings == {b"a": bytearray(b"\x04")}  # bit 5 = mask 0x80 >> 5


def test_model_setbit_grows_whatever_it_writes_and_getbit_grows_nothing():
    m = M.StreamModel({b"k": b"\xff"})
    rc, rep = m.run([b"new", b"k", b"ghost"], [0, 1, 1, 2, 1], [S0, G, G, G, S0], [2400, 7, 8, 99, 15])
    assert rc == M.OK and rep == [0, 1, 0, 0, 0]
    assert m.strings[b"new"] == bytearray(301)
    assert m.strings[b"k"] == bytearray(b"\xff\x00")
    assert b"ghost" not in m.strings


def test_model_equal_names_are_one_key():
    m = M.StreamModel()
    rc, rep = m.run([b"a", b"b", b"a"], [0, 1, 2, 1, 2, 0], [S1, G, G, S1, S0, G], [9] * 6)
    assert rc == M.OK and rep == [0, 0, 1, 0, 1, 0]
    assert m.strings == {b"a": bytearray(b"\x00\x00"), b"b": bytearray(b"\x00\x40")}


def test_model_failed_commands_fail_alone_and_the_first_decides_the_code():
    m = M.StreamModel({b"s": b"\x80"}, wrong=[b"h"])
    names = [b"s", b"h", b"only"]
    rc, rep = m.run(names, [0, 0, 1, 2, 0, 0], [G, S1, S1, S1, S1, G], [0, 1 << 32, 3, 1 << 32, 23, (1 << 32) - 1])
    assert rc == M.E_REDIS and rep == [1, M.FAILED, M.FAILED, M.FAILED, 0, 0]
    assert b"only" not in m.strings and b"h" not in m.strings
    assert m.strings[b"s"] == bytearray(b"\x80\x00\x01")
    m = M.StreamModel(wrong=[b"h"])
    rc, rep = m.run(names, [1, 0], [G, G], [3, 1 << 32])
    assert rc == M.E_WRONGTYPE and rep == [M.FAILED, M.FAILED]
    # a command that is out of range on a key of another type: the offset is looked at first
    rc, rep = m.run(names, [1, 1], [G, G], [1 << 32, 3])
    assert rc == M.E_REDIS


def test_model_caller_errors_change_nothing():
    m = M.StreamModel()
    assert m.run([b"a"], [0, 1], [S1, S1], [1, 2]) == (M.E_ILLEGAL_ARGUMENT, None)
    assert m.run([b"a"], [0, 0], [S1, 3], [1, 2]) == (M.E_ILLEGAL_ARGUMENT, None)
    assert m.strings == {}
    assert m.run([], [], [], []) == (M.OK, [])


# ---- the library ---------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    lib = L.lib()
    for sym in ("rbx_bitset_stream", "rbx_bitset_stream_dev"):
        assert re.search(r"\bint %s\(rbx_ctx \*ctx, const rbx_name \*names, uint32_t nkeys," % sym, hdr), sym
        assert hasattr(lib, sym) and sym in L.SIGNATURES
    assert (GETBIT, SETBIT0, SETBIT1) == (G, S0, S1) == (0, 1, 2)
    assert (L.RBX_E_ILLEGAL_ARGUMENT, L.RBX_E_WRONGTYPE, L.RBX_E_REDIS) == (M.E_ILLEGAL_ARGUMENT, M.E_WRONGTYPE, M.E_REDIS)


def test_null_context_is_the_callers_error():
    assert L.lib().rbx_bitset_stream(None, None, 0, None, None, None, 0, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_bitset_stream_dev(None, None, 0, None, None, None, 0, None, None) == L.RBX_E_ILLEGAL_ARGUMENT


def test_tunables_documented_and_range_checked():
    lib = L.lib()
    doc = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    for key in ("bitstream_path", "bitstream_serial_max", "bitstream_chunk"):
        assert '"%s"' % key in doc, key
    assert lib.rbx_tune(b"bitstream_path", 3) == -1 and lib.rbx_tune(b"bitstream_path", -1) == -1
    assert lib.rbx_tune(b"bitstream_chunk", 0) == -1 and lib.rbx_tune(b"bitstream_serial_max", -1) == -1
    for key, val in ((b"bitstream_path", 1), (b"bitstream_path", 2), (b"bitstream_path", 0), (b"bitstream_chunk", 1000),
                     (b"bitstream_chunk", 1 << 25), (b"bitstream_serial_max", 0), (b"bitstream_serial_max", 64)):
        assert lib.rbx_tune(key, val) == 0, key


# ---- RBatch's queue ---------------------------------------------------------------------------------------
class Recorder:
    """Stands in for the engine: records every call, answers bit commands from the model."""

    def __init__(self, wrong=()):
        self.calls = []
        self.model = M.StreamModel(wrong=wrong)

    def stream_call(self, names, cmd_key, cmd_op, cmd_index):
        self.calls.append(("stream", list(names), list(cmd_key), list(cmd_op), list(cmd_index)))
        rc, rep = self.model.run([n.encode() for n in names], cmd_key, cmd_op, cmd_index)
        return rc, "ERR bit offset is not an integer or out of range" if rc else "", rep

    def bitset(self, name):
        rec = self

        class Stub:
            def cardinality(self):
                rec.calls.append(("cardinality", name))
                return sum(bin(b).count("1") for b in rec.model.strings.get(name.encode(), b""))

            def size(self):
                rec.calls.append(("size", name))
                return 8 * len(rec.model.strings.get(name.encode(), b""))

            def setRange(self, lo, hi, value=True):
                rec.calls.append(("setRange", name, lo, hi, value))
                for i in range(lo, hi):
                    rec.model.setbit(name.encode(), i, int(value))

            def clearRange(self, lo, hi):
                self.setRange(lo, hi, False)

            def clear(self):
                rec.calls.append(("clear", name))
                rec.model.strings.pop(name.encode(), None)

        return Stub()


def batch_with(rec):
    return RBatch(None, stream_call=rec.stream_call, bitset=rec.bitset)


def test_consecutive_bit_commands_over_any_keys_are_one_call():
    rec = Recorder()
    b = batch_with(rec)
    a, c = b.getBitSet("a"), b.getBitSet("c")
    futs = [a.setAsync(3), c.getAsync(3), c.setAsync(3, False), a.getAsync(3), a.clearBitAsync(3), a.getAsync(3)]
    assert not futs[0].isDone()
    with pytest.raises(IllegalStateException):
        futs[0].get()
    res = b.execute()
    assert rec.calls == [("stream", ["a", "c"], [0, 1, 1, 0, 0, 0], [S1, G, S0, G, S0, G], [3] * 6)]
    assert res.getResponses() == [False, False, False, True, True, False]
    assert [f.get() for f in futs] == res.getResponses()
    assert all(type(r) is bool for r in res.getResponses())


def test_a_single_command_splits_the_run_and_sees_exactly_the_earlier_commands():
    rec = Recorder()
    b = batch_with(rec)
    a, c = b.getBitSet("a"), b.getBitSet("c")
    a.setAsync(1)
    c.setAsync(9)
    card = a.cardinalityAsync()
    a.setAsync(2)
    rng = c.setRangeAsync(0, 4)
    size = c.sizeAsync()
    got = a.getAsync(2)
    clr = a.clearAsync()
    after = a.getAsync(2)
    res = b.execute()
    assert [call[0] for call in rec.calls] == ["stream", "cardinality", "stream", "setRange", "size", "stream", "clear",
                                               "stream"]
    assert rec.calls[0][1:] == (["a", "c"], [0, 1], [S1, S1], [1, 9])
    assert rec.calls[2][1:] == (["a"], [0], [S1], [2])
    assert res.getResponses() == [False, False, 1, False, None, 16, True, None, False]
    assert (card.get(), rng.get(), size.get(), got.get(), clr.get(), after.get()) == (1, None, 16, True, None, False)


def test_first_error_is_raised_after_every_command_ran():
    rec = Recorder(wrong=[b"h"])
    b = batch_with(rec)
    a, h = b.getBitSet("a"), b.getBitSet("h")
    f0 = a.setAsync(1)
    f1 = h.setAsync(1)
    f2 = a.getAsync(1 << 32)
    f3 = a.getAsync(1)
    f4 = a.cardinalityAsync()
    with pytest.raises(RedisException, match="WRONGTYPE"):
        b.execute()
    assert [call[0] for call in rec.calls] == ["stream", "cardinality"]
    assert (f0.get(), f3.get(), f4.get()) == (False, True, 1)
    with pytest.raises(RedisException, match="WRONGTYPE"):
        f1.get()
    with pytest.raises(RedisException, match="bit offset"):
        f2.get()


def test_executing_twice_and_queuing_after_execute_are_errors():
    rec = Recorder()
    b = batch_with(rec)
    bs = b.getBitSet("a")
    bs.setAsync(1)
    b.execute()
    with pytest.raises(IllegalStateException, match="Batch already executed!"):
        b.execute()
    with pytest.raises(IllegalStateException, match="Batch already executed!"):
        bs.getAsync(1)
    assert len(rec.calls) == 1


def test_discard_empties_the_queue():
    rec = Recorder()
    b = batch_with(rec)
    b.getBitSet("a").setAsync(1)
    b.getBitSet("a").cardinalityAsync()
    b.discard()
    b.getBitSet("c").getAsync(0)
    assert b.execute().getResponses() == [False]
    assert rec.calls == [("stream", ["c"], [0], [G], [0])]


def test_an_empty_batch_makes_no_call():
    rec = Recorder()
    assert batch_with(rec).execute().getResponses() == []
    assert rec.calls == []
