"""rbx_bitset_op_groups without a GPU: the model (bitgroups_model) against hand-worked cases, the symbols and the
tile knob, the caller errors (refused ahead of any device work), and run_queue / RBatch / the Spring Data pipeline
over a recording fake of the grouped call: where runs begin and end, reply types, failures, the fallback to single
calls, discard and a second execute.  The seeded plan of the GPU driver is checked here for its share of failing
groups."""
import os
import re

import numpy as np
import pytest

import bitgroups_model as M
from redisson_amd import IllegalStateException, RBatch, RedisException, UnsupportedOperationException
from redisson_amd import _lib as L
from redisson_amd.client import _Queued, run_queue
from redisson_amd.spring_data import RedissonConnection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AND, OR, XOR, NOT = M.AND, M.OR, M.XOR, M.NOT


def keyspace(**strings):
    ks = M.Keyspace()
    for k, v in strings.items():
        ks.data[k] = bytes(v)
    return ks


# ---- the model against hand-worked cases ------------------------------------------------------------------------------
def test_model_hand_worked_cases():
    ks = keyspace(a=b"\xF0\x0F", b=b"\x3C", t=b"\xFF\xFF\xFF")
    ks.timeout |= {"a", "t"}
    names = ["a", "b", "t", "u", "missing"]
    rc, lens, counts, status = M.apply_groups(ks, names, [AND, OR, XOR, NOT, OR, OR, AND],
                                              [2, None, 3, None, 3, None, 2],
                                              [[0, 1], [2], [0, 1], [1], [3, 4], [4], [4]])
    # t = a AND b = 30 00 (b reads as zero past its end), shorter than before; BITCOUNT t; u = a XOR b = CC 0F;
    # NOT b counted over its one byte; u = u OR missing; BITCOUNT missing; t = AND(missing) is empty: t is deleted
    assert rc == M.OK and status == [0] * 7
    assert lens == [2, 2, 2, 1, 2, 0, 0]
    assert counts == [2, 2, 8, 4, 8, 0, 0]
    assert ks.data == {"a": b"\xF0\x0F", "b": b"\x3C", "u": b"\xCC\x0F"}
    assert ks.timeout == {"a"}  # a source keeps its timeout, a destination loses it, a deleted key has none


def test_model_failures_fail_alone_and_caller_errors_change_nothing():
    ks = keyspace(a=b"\x01", b=b"\x03")
    ks.hll.add("h")
    names = ["a", "b", "h", "d"]
    rc, lens, counts, status = M.apply_groups(ks, names, [OR, OR, NOT, OR, OR], [3, 2, 3, None, 3],
                                              [[0], [0], [0, 1], [2], [3, 1]])
    assert (rc, status) == (M.E_WRONGTYPE, [0, 0xFF, 0xFF, 0xFF, 0]) and M.message(rc) == M.WRONGTYPE_MSG
    assert lens == [1, 0, 0, 0, 1] and counts == [1, 0, 0, 0, 2] and ks.data["d"] == b"\x03"
    rc, *_ = M.apply_groups(ks, names, [NOT, OR], [3, 2], [[0, 1], [0]])
    assert rc == M.E_REDIS and M.message(rc) == M.NOT_MSG  # the first failing group's code
    before = dict(ks.data)
    for ops, dests, groups in (([4], [0], [[1]]), ([OR], [0], [[]]), ([OR], [0], [[4]]), ([OR], [4], [[0]])):
        assert M.apply_groups(ks, names, ops, dests, groups)[0] == M.E_ILLEGAL_ARGUMENT and ks.data == before


def test_model_phases_and_forwarding():
    names = ["a", "b"] + ["t%d" % i for i in range(1000)]
    pairs_ops, pairs_dests, pairs_groups, same_dests, same_groups = [], [], [], [], []
    for i in range(1000):
        pairs_ops += [AND, OR]
        pairs_dests += [2 + i, None]
        pairs_groups += [[0, 1], [2 + i]]
        same_dests += [2, None]
        same_groups += [[0, 1], [2]]
    none = [False] * 2000
    phases, fwd = M.plan(names, pairs_ops, pairs_dests, pairs_groups, none)
    assert phases == 1 and fwd[1::2] == list(range(0, 2000, 2)) and fwd[0::2] == [None] * 1000
    assert M.plan(names, pairs_ops, same_dests, same_groups, none)[0] == 1000
    # read after write, write after read, write after write; a destination among its own sources; NOT is not forwarded
    assert M.plan(names, [OR, OR], [0, 2], [[1], [0]], [False] * 2)[0] == 2
    assert M.plan(names, [OR, OR], [0, 1], [[1], [2]], [False] * 2)[0] == 2
    assert M.plan(names, [OR, OR], [0, 0], [[1], [2]], [False] * 2)[0] == 2
    assert M.plan(names, [XOR, AND], [0, 2], [[1, 0], [1, 3]], [False] * 2)[0] == 1
    assert M.plan(names, [OR, NOT], [0, None], [[1], [0]], [False] * 2) == (2, [None, None])
    assert M.plan(names, [OR, OR], [0, None], [[1], [0]], [True, False]) == (1, [None, None])
    assert M.plan(names, [], [], [], []) == (0, [])
    # equal names are one key
    assert M.plan(["x", "y", "x"], [OR, OR], [0, 1], [[1], [2]], [False] * 2)[0] == 2


# ---- the symbols, the tunable, the caller errors --------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    assert hasattr(lib, "rbx_bitset_op_groups") and "rbx_bitset_op_groups" in L.SIGNATURES
    assert re.search(r"\brbx_bitset_op_groups\(", hdr) and re.search(r"#define RBX_BITGROUP_NO_DEST 0xFFFFFFFFu", hdr)
    assert hasattr(lib, "rbx_bench_bitgroups_last") and "rbx_bench_bitgroups_last" in L.SIGNATURES
    assert re.search(r"\brbx_bench_bitgroups_last\(", bench) and L.RBX_BITGROUP_NO_DEST == 0xFFFFFFFF
    import redisson_amd

    assert callable(redisson_amd.bitset_op_groups_call) and "bitset_op_groups_call" in redisson_amd.__all__


def test_the_tile_knob_is_documented_and_range_checked():
    lib = L.lib()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    tun = open(os.path.join(ROOT, "redisson_amd", "csrc", "tunables.h")).read()
    assert '"bitgroups_tile"' in bench and '"bitgroups_tile"' in tun
    for v in (-1, 1, 2048, 4097, 12288, 1 << 21):
        assert lib.rbx_tune(b"bitgroups_tile", v) == -1, v
    for v in (4096, 8192, 65536, 1 << 20, 0):
        assert lib.rbx_tune(b"bitgroups_tile", v) == 0, v


def test_caller_errors_are_refused_before_any_device_work():
    """the checks run ahead of the context's device: a context pointer that is never dereferenced is enough"""
    lib = L.lib()
    bad = L.RBX_E_ILLEGAL_ARGUMENT
    u64 = lambda *x: np.array(x, np.uint64)  # noqa: E731
    u32 = lambda *x: np.array(x or (0,), np.uint32)  # noqa: E731
    u8 = lambda *x: np.array(x or (0,), np.uint8)  # noqa: E731
    lens, counts, status = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint8)
    names, _keep = L.names_array(["a", "b"])
    ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731

    def call(op, dest, off, key, n, nkeys=2, ctx=1, names=names):
        return lib.rbx_bitset_op_groups(ctx, names, nkeys, ptr(op, L.u8p), ptr(dest, L.u32p), ptr(off, L.u64p),
                                        ptr(key, L.u32p), n, ptr(lens, L.u64p), ptr(counts, L.u64p), ptr(status, L.u8p))

    assert call(u8(1), u32(0), u64(0, 1), u32(1), 1, ctx=None) == bad  # NULL context
    assert call(u8(1), u32(0), u64(0, 1), u32(1), 1, names=None) == bad
    assert call(u8(4), u32(0), u64(0, 1), u32(1), 1) == bad and "unknown BITOP" in L.last_error()
    assert call(u8(1, 1), u32(0, 1), u64(0, 1, 1), u32(1), 2) == bad  # a group without a source
    assert call(u8(1), u32(0), u64(0, 1), u32(2), 1) == bad  # an entry >= nkeys
    assert call(u8(1), u32(2), u64(0, 1), u32(1), 1) == bad  # a destination >= nkeys ...
    assert call(u8(1), u32(0xFFFFFFFE), u64(0, 1), u32(1), 1) == bad  # ... that is not RBX_BITGROUP_NO_DEST
    assert call(u8(1), u32(0), u64(1, 2), u32(0, 1), 1) == bad  # offsets from 1
    assert call(u8(1, 1), u32(0, 0), u64(0, 2, 1), u32(0, 1), 2) == bad  # descending
    assert call(None, u32(0), u64(0, 1), u32(1), 1) == bad and call(u8(1), None, u64(0, 1), u32(1), 1) == bad
    assert call(u8(1), u32(0), None, u32(1), 1) == bad and call(u8(1), u32(0), u64(0, 1), None, 1) == bad
    assert "NULL" in L.last_error()
    assert call(None, None, None, None, 0) == L.RBX_OK  # ngroups = 0 sends nothing


# ---- run_queue, RBatch and the pipeline over a fake engine --------------------------------------------------------------
HLL = "an-hll"


class Recorder:
    """the grouped bit call, the bit stream call and RBitSet's single calls over one model keyspace"""

    def __init__(self):
        self.ks = keyspace(a=b"\xF0\x0F", b=b"\x3C\xFF\x01")
        self.ks.hll.add(HLL)
        self.calls = []

    @staticmethod
    def _k(name):
        return name.decode() if isinstance(name, bytes) else name

    def bit_groups_call(self, names, ops, dests, groups):
        assert len(set(names)) == len(names)  # each distinct name once
        names = [self._k(n) for n in names]
        self.calls.append(("groups", [(op, None if d is None else names[d], tuple(names[k] for k in g))
                                      for op, d, g in zip(ops, dests, groups)]))
        rc, lens, counts, status = M.apply_groups(self.ks, names, ops, dests, groups)
        return ({M.OK: L.RBX_OK, M.E_WRONGTYPE: L.RBX_E_WRONGTYPE, M.E_REDIS: L.RBX_E_REDIS}[rc], M.message(rc),
                np.array(lens, np.uint64), np.array(counts, np.uint64), np.array(status, np.uint8))

    def stream_call(self, names, cmd_key, cmd_op, cmd_index):
        self.calls.append(("bits", len(cmd_key)))
        return L.RBX_OK, "", [0] * len(cmd_key)

    def bitset(self, name):
        rec = self

        class Single:
            def _op(self, op, others):
                rec.calls.append((op, name, others))
                _reply, err = rec.ks.bitop("obj", name, op, (name, *others))
                if err:
                    raise RedisException(M.WRONGTYPE_MSG)

            def or_(self, *others):
                self._op("or", others)

            def and_(self, *others):
                self._op("and", others)

            def xor(self, *others):
                self._op("xor", others)

            def not_(self):
                rec.calls.append(("not", name, ()))
                rec.ks.bitop_not("obj", name, name)

            def cardinality(self):
                rec.calls.append(("cardinality", name))
                return rec.ks.cardinality("obj", name)[0]

            def length(self):
                rec.calls.append(("length", name))
                return rec.ks.length("obj", name)[0]

            def toByteArray(self):
                rec.calls.append(("toByteArray", name))
                return rec.ks.to_bytes("obj", name)[0]

        return Single()

    def batch(self, grouped=True) -> RBatch:
        extra = dict(bit_groups_call=self.bit_groups_call) if grouped else {}
        return RBatch(None, stream_call=self.stream_call, bitset=self.bitset, **extra)


def test_or_cardinality_or_cardinality_is_one_call_and_a_set_between_two_ors_gives_two():
    rec = Recorder()
    b = rec.batch()
    futures = [b.getBitSet("d").orAsync("a"), b.getBitSet("d").cardinalityAsync(),
               b.getBitSet("d").orAsync("b"), b.getBitSet("d").cardinalityAsync()]
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["groups"]
    assert rec.calls[0][1] == [(OR, "d", ("d", "a")), (OR, None, ("d",)), (OR, "d", ("d", "b")), (OR, None, ("d",))]
    assert res == [None, 8, None, 15] and [f.get() for f in futures] == res and type(res[1]) is int
    assert rec.ks.data["d"] == b"\xFC\xFF\x01"
    rec = Recorder()
    b = rec.batch()
    b.getBitSet("d").orAsync("a")
    b.getBitSet("s").setAsync(3)
    b.getBitSet("d").orAsync("b")
    b.execute()
    assert [c[0] for c in rec.calls] == ["groups", "bits", "groups"]


def test_runs_split_where_the_rule_says_and_reply_types():
    rec = Recorder()
    b = rec.batch()
    futures = [b.getBitSet("x").andAsync("a", "b"),       # groups: x is missing, so AND(x, a, b) over 3 bytes is zero
               b.getBitSet("y").xorAsync("a"),            # groups
               b.getBitSet("y").notAsync(),               # groups
               b.getBitSet("y").lengthAsync(),            # single
               b.getBitSet("y").cardinalityAsync(),       # groups
               b.getBitSet("y").toByteArrayAsync(),       # single
               b.getBitSet("y").getAsync(0),              # bits
               b.getBitSet("a").cardinalityAsync(),       # groups
               b.getBitSet("a").cardinality_async()]      # groups (the alias)
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["groups", "length", "groups", "toByteArray", "bits", "groups"]
    assert rec.calls[0][1] == [(AND, "x", ("x", "a", "b")), (XOR, "y", ("y", "a")), (NOT, "y", ("y",))]
    assert rec.calls[2][1] == [(OR, None, ("y",))] and len(rec.calls[5][1]) == 2
    assert res == [None, None, None, 12, 8, b"\x0F\xF0", False, 8, 8]
    assert [f.get() for f in futures] == res
    assert rec.ks.data["x"] == b"\x00\x00\x00"
    for alias in ("or_async", "and_async", "xor_async", "not_async", "length_async", "to_byte_array_async"):
        assert callable(getattr(b.getBitSet("a"), alias))


def test_without_the_grouped_call_everything_runs_singly():
    rec = Recorder()
    b = rec.batch(grouped=False)
    b.getBitSet("d").orAsync("a")
    b.getBitSet("d").cardinalityAsync()
    b.getBitSet("d").andAsync("b")
    b.getBitSet("d").notAsync()
    res = b.execute().getResponses()
    assert rec.calls == [("or", "d", ("a",)), ("cardinality", "d"), ("and", "d", ("b",)), ("not", "d", ())]
    assert res == [None, 8, None, None]
    # run_queue itself: the trailing parameter defaults to None, and the others still pass positionally
    ran = []
    queue = [_Queued("a", fn=lambda: ran.append("op"), bitop=(OR, "a", ["a", "b"]), convert=lambda *_: 1 / 0)]
    assert run_queue(queue, None) == ([None], None) and ran == ["op"]
    assert run_queue(list(queue), None, None, None, None, None) == ([None], None) and ran == ["op", "op"]
    queue = [_Queued("d", fn=None, bitop=(OR, "d", ["a"]), convert=lambda length, _count: length),
             _Queued("d", fn=None, bitop=(OR, None, ["d"]), convert=lambda _length, count: count)]
    assert run_queue(queue, None, None, None, None, None, Recorder().bit_groups_call) == ([2, 8], None)


def test_a_failed_group_raises_its_own_exception_after_every_command_ran():
    rec = Recorder()
    b = rec.batch()
    ok = b.getBitSet("d").orAsync("a")
    bad = b.getBitSet("d").orAsync(HLL)
    bad_dest = b.getBitSet(HLL).notAsync()
    count = b.getBitSet("d").cardinalityAsync()
    bad_count = b.getBitSet(HLL).cardinalityAsync()
    after = b.getBitSet("e").xorAsync("d")
    with pytest.raises(RedisException, match="WRONGTYPE Operation against a key"):
        b.execute()
    assert ok.get() is None and count.get() == 8 and after.get() is None
    for f in (bad, bad_dest, bad_count):
        with pytest.raises(RedisException, match="WRONGTYPE"):
            f.get()
    assert rec.ks.data["e"] == b"\xF0\x0F" and [c[0] for c in rec.calls] == ["groups"]
    # NOT with several sources (only the raw queue can hold one) fails with Redis's own message
    queue = [_Queued("d", fn=None, bitop=(NOT, "d", ["a", "b"]), convert=lambda *_: None),
             _Queued("d", fn=None, bitop=(OR, None, ["a"]), convert=lambda _l, count: count)]
    responses, error = run_queue(queue, None, None, None, None, None, Recorder().bit_groups_call)
    assert responses == [None, 8] and isinstance(error, RedisException) and "BITOP NOT" in str(error)


def test_a_refused_run_fails_every_command_of_it():
    def refuse(*_a):
        return L.RBX_E_ILLEGAL_ARGUMENT, "a group's key is not below nkeys", [], [], []

    b = RBatch(None, stream_call=None, bit_groups_call=refuse)
    f, g = b.getBitSet("a").orAsync("b"), b.getBitSet("a").cardinalityAsync()
    with pytest.raises(Exception, match="not below nkeys"):
        b.execute()
    for x in (f, g):
        with pytest.raises(Exception, match="not below nkeys"):
            x.get()


def test_discard_and_execute_twice():
    rec = Recorder()
    b = rec.batch()
    b.getBitSet("d").orAsync("a")
    b.discard()
    assert b.execute().getResponses() == [] and rec.calls == [] and "d" not in rec.ks.data
    with pytest.raises(IllegalStateException):
        b.execute()
    with pytest.raises(IllegalStateException):
        b.getBitSet("d").orAsync("a")
    with pytest.raises(IllegalStateException):
        b.discard()


def test_the_pipeline_groups_bitop_and_whole_string_bitcount(monkeypatch):
    import redisson_amd.spring_data as S

    rec = Recorder()
    monkeypatch.setattr(S, "bitset_op_groups_call", lambda client, *a: rec.bit_groups_call(*a))
    monkeypatch.setattr(S, "bitset_stream_call", lambda client, *a: rec.stream_call(*a))
    conn = RedissonConnection(None)
    conn.openPipeline()
    assert conn.bitOp("AND", b"t", b"a", b"b") is None and conn.bitCount(b"t") is None
    assert conn.bitOp(L.RBX_BITOP_NOT, b"n", b"a") is None
    conn.getBit(b"s", 1)
    conn.bitCount(b"a")
    conn.bitOp("or", b"u", b"a", HLL.encode())
    conn.bitCount(b"b")
    with pytest.raises(UnsupportedOperationException, match="single source key"):
        conn.bitOp("NOT", b"n", b"a", b"b")  # before anything is queued
    with pytest.raises(RedisException, match="WRONGTYPE"):
        conn.closePipeline()
    assert [c[0] for c in rec.calls] == ["groups", "bits", "groups"]
    assert rec.calls[0][1] == [(AND, "t", ("a", "b")), (OR, None, ("t",)), (NOT, "n", ("a",))]
    assert rec.calls[2][1] == [(OR, None, ("a",)), (OR, "u", ("a", HLL)), (OR, None, ("b",))]
    assert rec.ks.data["t"] == b"\x30\x0F\x00" and "u" not in rec.ks.data
    conn.openPipeline()
    conn.bitOp("XOR", b"t", b"t", b"a")
    conn.bitCount(b"t")
    conn.bitOp("NOT", b"n", b"zz")
    assert conn.closePipeline() == [3, 2, 0]  # bitOp replies the length, bitCount the count
    assert rec.ks.data["t"] == b"\xC0\x00\x00" and "n" not in rec.ks.data


def test_a_ranged_bitcount_stays_a_single_call(monkeypatch):
    import redisson_amd.spring_data as S

    rec = Recorder()
    monkeypatch.setattr(S, "bitset_op_groups_call", lambda client, *a: rec.bit_groups_call(*a))
    conn = RedissonConnection(None)
    conn.openPipeline()
    conn.bitCount(b"a", 0, 0)
    conn.bitCount(b"a")
    queue = conn._pipeline
    assert queue[0].bitop is None and queue[0].fn is not None and queue[1].bitop == (OR, None, [b"a"])
    conn._pipeline = None


# ---- the seeded driver's plan (test_bitgroups_gpu.py runs it on the engine) ------------------------------------------------
def test_the_seeded_plan_keeps_failing_groups_under_the_cap():
    import bitgroups_driver as D

    calls = D.seeded_calls()
    groups = [g for call in calls for g in zip(*call[1:])]
    assert len(calls) == 300 and all(1 <= len(call[1]) <= 40 for call in calls)
    failing = D.failing_groups(calls)
    assert 0 < failing <= len(groups) // 10, (failing, len(groups))
    ops = {op for op, _d, _g in groups}
    assert ops == {AND, OR, XOR, NOT}
    assert sum(d is None for _op, d, _g in groups) > len(groups) // 8
    assert sum(d is not None and d in g for _op, d, g in groups) > len(groups) // 8
