"""The ordered BITFIELD stream without a GPU: the model of fieldstream_model.py against cases worked out by hand,
the two new C-ABI symbols, the tunables, RBatch's queue with the engine calls replaced by recording stubs, and
the seeded batches held to what each must contain."""
import os
import re

import pytest

import fieldstream_model as M
from redisson_amd import IllegalArgumentException, RBatch, RedisException
from redisson_amd import _lib as L
from redisson_amd.client import GETBIT, SETBIT0, SETBIT1, RBatchBitSet, RBitSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, S, I = M.GET, M.SET, M.INCRBY
W, SAT, FAIL = M.WRAP, M.SAT, M.FAIL


# ---- the model ---------------------------------------------------------------------------------------
def test_model_order_on_one_field_and_a_get_sees_earlier_writes():
    m = M.FieldStreamModel()
    cmds = [(S, 0, 8, W, 8, 200), (I, 0, 8, W, 8, 100), (G, 0, 8, W, 8, 0), (I, 0, 8, SAT, 8, 250), (G, 1, 8, W, 8, 0),
            (I, 0, 8, FAIL, 8, 1), (S, 1, 8, W, 8, -2), (G, 0, 16, W, 0, 0)]
    rc, rep, st = m.run([b"a"], [0] * len(cmds), cmds)
    assert rc == M.OK and rep == [0, 44, 44, 255, -1, 0, -1, 0xFE] and st == [0, 0, 0, 0, 0, M.NIL, 0, 0]
    assert m.strings == {b"a": bytearray(b"\x00\xfe")}


def test_model_growth_on_a_nil_and_a_get_grows_nothing():
    m = M.FieldStreamModel()
    rc, rep, st = m.run([b"k", b"ghost"], [0, 1, 1], [(I, 0, 8, FAIL, 0, 300), (G, 1, 64, W, 4000, 0), (G, 0, 5, W, 3, 0)])
    assert (rc, rep, st) == (M.OK, [0, 0, 0], [M.NIL, 0, 0])
    assert m.strings == {b"k": bytearray(b"\x00")}  # INCRBY u8 0 300 under FAIL leaves 00 and nil


def test_model_a_key_with_only_failed_writes_is_not_created_and_the_first_failure_decides_the_code():
    m = M.FieldStreamModel({b"s": b"\x80"}, wrong=[b"h"])
    names = [b"s", b"h", b"only"]
    cmds = [(G, 0, 1, W, 0, 0), (S, 0, 8, W, 1 << 32, 1), (S, 0, 64, W, 0, 1), (I, 1, 65, W, 0, 1), (S, 0, 0, W, 0, 1),
            (S, 0, 8, W, (1 << 32) - 7, 1), (S, 1, 8, W, 0, 1), (S, 0, 4, W, 20, 9)]
    rc, rep, st = m.run(names, [0, 2, 2, 2, 2, 2, 1, 0], cmds)
    assert rc == M.E_REDIS and m.first_failure == "offset"
    assert st == [0, M.FAILED, M.FAILED, M.FAILED, M.FAILED, M.FAILED, M.FAILED, 0] and rep == [1, 0, 0, 0, 0, 0, 0, 0]
    assert m.events[1:7] == ["offset", "type", "type", "type", "offset", "wrong"]
    assert b"only" not in m.strings and b"h" not in m.strings and m.strings[b"s"] == bytearray(b"\x80\x00\x09")
    m = M.FieldStreamModel(wrong=[b"h"])
    rc, _rep, _st = m.run(names, [1, 0], [(G, 0, 8, W, 0, 0), (G, 0, 64, W, 0, 0)])
    assert rc == M.E_WRONGTYPE and m.first_failure == "wrong"
    # on a key of another type the type and the offset are still looked at first
    rc, _rep, _st = m.run(names, [1, 1], [(G, 0, 8, W, 1 << 32, 0), (G, 0, 8, W, 0, 0)])
    assert rc == M.E_REDIS and m.events == ["offset", "wrong"]
    rc, _rep, _st = m.run(names, [1], [(G, 0, 64, W, 1 << 32, 0)])
    assert rc == M.E_REDIS and m.events == ["type"]


def test_model_equal_names_are_one_key_and_caller_errors_change_nothing():
    m = M.FieldStreamModel()
    rc, rep, _st = m.run([b"a", b"b", b"a"], [0, 2, 1, 2], [(S, 0, 8, W, 0, 7), (I, 0, 8, W, 0, 1), (G, 0, 8, W, 0, 0), (G, 0, 8, W, 0, 0)])
    assert rc == M.OK and rep == [0, 8, 0, 8] and m.strings == {b"a": bytearray(b"\x08")}
    m = M.FieldStreamModel()
    for key, cmd in (([1], (S, 0, 8, W, 0, 1)), ([0], (3, 0, 8, W, 0, 1)), ([0], (S, 0, 8, 3, 0, 1)), ([0], (S, 2, 8, W, 0, 1))):
        assert m.run([b"a"], [0] + key, [(S, 0, 8, W, 0, 1), cmd]) == (M.E_ILLEGAL_ARGUMENT, None, None)
    assert m.strings == {} and m.run([], [], []) == (M.OK, [], [])


# ---- the library ---------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    lib = L.lib()
    for sym in ("rbx_bitset_field_stream", "rbx_bitset_field_stream_dev"):
        assert re.search(r"\bint %s\(rbx_ctx \*ctx, const rbx_name \*names, uint32_t nkeys," % sym, hdr), sym
        assert hasattr(lib, sym) and sym in L.SIGNATURES
    assert "rbx_bitset_field_stream" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert (L.RBX_FIELD_GET, L.RBX_FIELD_SET, L.RBX_FIELD_INCRBY) == (G, S, I)
    assert (L.RBX_OVERFLOW_WRAP, L.RBX_OVERFLOW_SAT, L.RBX_OVERFLOW_FAIL) == (W, SAT, FAIL)
    assert (L.RBX_E_ILLEGAL_ARGUMENT, L.RBX_E_WRONGTYPE, L.RBX_E_REDIS) == (M.E_ILLEGAL_ARGUMENT, M.E_WRONGTYPE, M.E_REDIS)
    import ctypes as C

    assert C.sizeof(L.RbxFieldCmd) == 24  # the struct is unchanged


def test_null_context_is_the_callers_error():
    assert L.lib().rbx_bitset_field_stream(None, None, 0, None, None, 0, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_bitset_field_stream_dev(None, None, 0, None, None, 0, None, None, None) == L.RBX_E_ILLEGAL_ARGUMENT


def test_tunables_documented_and_range_checked():
    lib = L.lib()
    doc = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    for key in ("fieldstream_path", "fieldstream_serial_max", "fieldstream_chunk"):
        assert '"%s"' % key in doc, key
    assert lib.rbx_tune(b"fieldstream_path", 4) == -1 and lib.rbx_tune(b"fieldstream_path", -1) == -1
    assert lib.rbx_tune(b"fieldstream_chunk", 0) == -1 and lib.rbx_tune(b"fieldstream_serial_max", -1) == -1
    for key, val in ((b"fieldstream_path", 1), (b"fieldstream_path", 2), (b"fieldstream_path", 3), (b"fieldstream_path", 0),
                     (b"fieldstream_chunk", 64), (b"fieldstream_chunk", 1 << 30), (b"fieldstream_chunk", 1 << 25),
                     (b"fieldstream_serial_max", 0), (b"fieldstream_serial_max", 64)):
        assert lib.rbx_tune(key, val) == 0, key
    assert lib.rbx_bench_fieldstream_last_path() in range(6)


# ---- RBatch's queue ---------------------------------------------------------------------------------------
class Recorder:
    """Stands in for the engine: records every call, answers from the model."""

    def __init__(self, wrong=()):
        self.calls = []
        self.model = M.FieldStreamModel(wrong=wrong)

    def stream_call(self, names, cmd_key, cmd_op, cmd_index):
        self.calls.append(("stream", list(names), list(cmd_key), list(cmd_op), list(cmd_index)))
        cmds = [(G, 0, 1, W, i, 0) if op == GETBIT else (S, 0, 1, W, i, op - 1) for op, i in zip(cmd_op, cmd_index)]
        rc, rep, st = self.model.run([n.encode() for n in names], cmd_key, cmds)
        return rc, "some command failed" if rc else "", [0xFF if s == M.FAILED else r for r, s in zip(rep, st)]

    def field_stream_call(self, names, cmd_key, cmds):
        self.calls.append(("fields", list(names), list(cmd_key), list(cmds)))
        rc, rep, st = self.model.run([n.encode() for n in names], cmd_key, cmds)
        return rc, "some command failed" if rc else "", rep, st

    def bitset(self, name):
        rec = self

        class Stub:
            def cardinality(self):
                rec.calls.append(("cardinality", name))
                return sum(bin(b).count("1") for b in rec.model.strings.get(name.encode(), b""))

            def incrementAndGetInteger(self, offset, increment):
                rec.calls.append(("incrementAndGetInteger", name, offset, increment))
                return rec.model.run([name.encode()], [0], [(I, 1, 32, W, offset, increment)])[1][0]

            def getSigned(self, size, offset):
                rec.calls.append(("getSigned", name, size, offset))
                return rec.model.run([name.encode()], [0], [(G, 1, size, W, offset, 0)])[1][0]

        return Stub()


def batch_with(rec, fields=True):
    return RBatch(None, stream_call=rec.stream_call, bitset=rec.bitset,
                  field_stream_call=rec.field_stream_call if fields else None)


def test_a_mixed_bit_and_field_run_is_one_field_call_with_the_bits_as_u1():
    rec = Recorder()
    b = batch_with(rec)
    a, c = b.getBitSet("u:1"), b.getBitSet("u:2")
    futs = [a.setAsync(3), c.incrementAndGetIntegerAsync(32, 5), a.getAsync(3), c.setByteAsync(0, -2), a.clearBitAsync(3),
            c.getUnsignedAsync(8, 0), c.incrementAndGetShortAsync(32, -1), a.getAsync(3), c.getLongAsync(0)]
    assert not futs[1].isDone()
    res = b.execute()
    assert rec.calls == [("fields", ["u:1", "u:2"], [0, 1, 0, 1, 0, 1, 1, 0, 1],
                          [(S, 0, 1, W, 3, 1), (I, 1, 32, W, 32, 5), (G, 0, 1, W, 3, 0), (S, 1, 8, W, 0, -2),
                           (S, 0, 1, W, 3, 0), (G, 0, 8, W, 0, 0), (I, 1, 16, W, 32, -1), (G, 0, 1, W, 3, 0),
                           (G, 1, 64, W, 0, 0)])]
    assert res.getResponses() == [False, 5, True, 0, True, 254, -1, False, (0xFE << 56) - (1 << 64) + 0xFFFF0005]
    assert [f.get() for f in futs] == res.getResponses()
    assert [type(r) for r in res.getResponses()] == [bool, int, bool, int, bool, int, int, bool, int]


def test_a_bit_only_run_still_uses_stream_call_and_a_single_command_splits_the_run():
    rec = Recorder()
    b = batch_with(rec)
    a = b.getBitSet("a")
    a.setAsync(1)
    a.getAsync(1)
    card = a.cardinalityAsync()
    inc = a.incrementAndGetByteAsync(8, 7)
    a.setAsync(2)
    res = b.execute()
    assert [c[0] for c in rec.calls] == ["stream", "cardinality", "fields"]
    assert rec.calls[0][1:] == (["a"], [0, 0], [SETBIT1, GETBIT], [1, 1])
    assert rec.calls[2][1:] == (["a"], [0, 0], [(I, 1, 8, W, 8, 7), (S, 0, 1, W, 2, 1)])
    assert res.getResponses() == [False, True, 1, 7, False] and (card.get(), inc.get()) == (1, 7)


def test_without_a_field_call_field_commands_run_singly_through_the_bit_set():
    rec = Recorder()
    b = batch_with(rec, fields=False)
    a = b.getBitSet("a")
    futs = [a.setAsync(1), a.incrementAndGetIntegerAsync(32, 9), a.getSignedAsync(32, 32), a.getAsync(1)]
    b.execute()
    assert [c[0] for c in rec.calls] == ["stream", "incrementAndGetInteger", "getSigned", "stream"]
    assert rec.calls[1] == ("incrementAndGetInteger", "a", 32, 9) and rec.calls[2] == ("getSigned", "a", 32, 32)
    assert [f.get() for f in futs] == [False, 9, 9, True]


def test_the_first_error_is_raised_after_everything_ran_and_a_nil_is_none():
    rec = Recorder(wrong=[b"h"])
    b = batch_with(rec)
    a, h = b.getBitSet("a"), b.getBitSet("h")
    f0 = a.setByteAsync(0, 5)
    f1 = h.incrementAndGetIntegerAsync(0, 1)
    f2 = a.getUnsignedAsync(8, 1 << 32)
    f3 = a.getSignedAsync(0, 0)
    f4 = h.getAsync(1)
    f5 = a.getAsync(1 << 32)
    f6 = a.getByteAsync(0)
    with pytest.raises(RedisException, match="WRONGTYPE"):
        b.execute()
    assert len(rec.calls) == 1 and rec.calls[0][0] == "fields"
    assert (f0.get(), f6.get()) == (0, 5)
    for fut, text in ((f1, "WRONGTYPE"), (f2, "bit offset"), (f3, "Invalid bitfield type"), (f4, "WRONGTYPE"), (f5, "bit offset")):
        with pytest.raises(RedisException, match=text):
            fut.get()
    # a nil reply (status 1) is None
    rec = Recorder()
    b = RBatch(None, stream_call=rec.stream_call, bitset=rec.bitset,
               field_stream_call=lambda names, key, cmds: (0, "", [0, 7], [1, 0]))
    g = b.getBitSet("a")
    g.getByteAsync(0)
    g.getByteAsync(8)
    assert b.execute().getResponses() == [None, 7]


def test_redissons_own_checks_fire_at_queue_time():
    rec = Recorder()
    a = batch_with(rec).getBitSet("a")
    with pytest.raises(IllegalArgumentException, match="Size can't be greater than 64 bits"):
        a.getSignedAsync(65, 0)
    with pytest.raises(IllegalArgumentException, match="Size can't be greater than 63 bits"):
        a.incrementAndGetUnsignedAsync(64, 0, 1)
    with pytest.raises(IllegalArgumentException):
        a.setByteAsync(0, 128)  # not a Java byte
    with pytest.raises(IllegalArgumentException):
        a.incrementAndGetShortAsync(0, 1 << 15)
    assert rec.calls == [] and a._batch._queue == []
    a.getSignedAsync(64, 0)
    a.getUnsignedAsync(63, 0)
    assert len(a._batch._queue) == 2


def test_every_typed_field_method_of_rbitset_has_its_async_form_and_alias():
    names = [op + ty for op in ("get", "set", "incrementAndGet") for ty in ("Signed", "Unsigned", "Byte", "Short", "Integer", "Long")]
    assert len(names) == 18
    for name in names:
        assert callable(getattr(RBitSet, name))
        snake = re.sub(r"([A-Z])", lambda m: "_" + m.group(1).lower(), name + "Async")
        assert getattr(RBatchBitSet, name + "Async") is getattr(RBatchBitSet, snake), name


# ---- the seeded batches ---------------------------------------------------------------------------------
START = {b"s0": b"\xa5" * 40, b"s1": b"\xff" * 100, b"s2": b"", b"bloom": b"\x3c" * 150}


@pytest.mark.parametrize("contained", [False, True])
@pytest.mark.parametrize("seed", M.SEEDS)
def test_every_seeded_batch_contains_one_of_each_category(seed, contained):
    key, cmds = M.random_batch(seed, contained)
    assert len(cmds) == M.NCMD and max(key) == len(M.KEYS) - 1
    m = M.FieldStreamModel(START, wrong=[b"hll"])
    rc, _rep, st = m.run([k.encode() for k in M.KEYS], key, cmds)
    assert rc in (M.E_REDIS, M.E_WRONGTYPE)
    have = M.coverage(key, cmds, m.events)
    want = set(M.CATEGORIES) - ({"straddling"} if contained else set())
    assert have >= want, sorted(want - have)
    assert ("straddling" in have) == (not contained)
    assert b"ghost" not in m.strings and b"new" in m.strings
    assert {M.VALID, M.NIL, M.FAILED} == set(st)
