"""rbx_bitset_range_stream without a GPU: the model (rangestream_model) against hand-worked cases, rbx_bitset_range_of
against the model on seeded commands, the symbols and the four knobs, the caller errors (refused ahead of any device
work), and run_queue / RBatch / the Spring Data pipeline over a recording fake of the range call: where runs begin
and end, reply types, failures, the fallback to single calls.  The seeded plan of the GPU driver is checked here for
its share of failing commands."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bitrange_model as RM
import bitstring_model as BM
import rangestream_driver as D
import rangestream_model as M
from redisson_amd import RBatch, RedisException
from redisson_amd import _lib as L
from redisson_amd.client import _Queued, _range_row, run_queue
from redisson_amd.spring_data import RedissonConnection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, POS, STRLEN, LENGTH, BYTE, BIT = M.COUNT, M.POS, M.STRLEN, M.LENGTH, M.BYTE, M.BIT
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
HLL = "an-hll"


def keyspace(**strings):
    ks = BM.Keyspace()
    for k, v in strings.items():
        ks.data[k] = bytes(v)
    ks.hll.add(HLL)
    return ks


# ---- the model against hand-worked cases ------------------------------------------------------------------------------
def test_model_hand_worked_cases():
    # a = 1111 0000 0000 1111 0000 0001; z's last byte is zero and its first bit is set; y's is zero and clear
    ks = keyspace(a=b"\xF0\x0F\x01", z=b"\x80\x00", y=b"\x40\x00")
    names = ["a", "missing", "z", "y", "a"]
    rows = [(COUNT, 0, 0, 0, 0, BYTE),        # BITCOUNT a = 4 + 4 + 1
            (COUNT, 0, 2, 1, -1, BYTE),       # bytes 1..2 = 4 + 1
            (COUNT, 0, 2, -9, -1, BIT),       # bits 15..23 = 1 + 1
            (COUNT, 0, 2, -1, -2, BYTE),      # both negative, start > end: 0 before anything is normalised
            (POS, 1, 0, 0, 0, BYTE),          # the first one: bit 0
            (POS, 0, 0, 0, 0, BYTE),          # the first zero: bit 4
            (POS, 1, 1, 1, 0, BYTE),          # from byte 1: bit 12
            (POS, 1, 2, 16, 22, BIT),         # bits 16..22 are clear: -1
            (POS, 0, 2, 0, 3, BIT),           # bits 0..3 are set and an end is given: -1
            (STRLEN, 0, 0, 0, 0, BYTE),       # 3
            (LENGTH, 0, 0, 0, 0, BYTE)]       # the last byte's lowest set bit is bit 23: 24
    rc, replies, status, _kinds = M.apply_stream(ks, names, [0] * len(rows), rows)
    assert rc == M.OK and status == [0] * len(rows)
    assert replies == [9, 5, 2, 0, 0, 4, 12, -1, -1, 3, 24]
    # the same name twice is one key; a missing key: COUNT 0, POS -1 for 1 and 0 for 0, STRLEN 0
    rc, replies, status, _ = M.apply_stream(ks, names, [4, 1, 1, 1, 1], [rows[0], rows[0], rows[4], rows[5], rows[9]])
    assert (rc, replies, status) == (M.OK, [9, 0, -1, 0, 0], [0] * 5)
    # BITPOS 0 on a string of ones: 8 * length without an end, -1 with one
    ks.data["o"] = b"\xFF" * 5
    rc, replies, _s, _ = M.apply_stream(ks, ["o"], [0, 0, 0], [(POS, 0, 0, 0, 0, BYTE), (POS, 0, 1, 2, 0, BYTE),
                                                               (POS, 0, 2, 0, -1, BYTE)])
    assert replies == [40, 40, -1]
    # length(): z answers 1 through the script's odd path, y and a missing key fail in it
    rc, replies, status, kinds = M.apply_stream(ks, names, [2, 3, 1], [rows[10]] * 3)
    assert (rc, replies, status) == (M.E_REDIS, [1, 0, 0], [0, 0xFF, 0xFF]) and kinds == [None, M.SCRIPT, M.SCRIPT]
    assert M.message(kinds) == "ERR bit offset is not an integer or out of range"


def test_model_failures_their_order_and_the_return_code():
    ks = keyspace(a=b"\x01")
    names = ["a", HLL]
    bad_bit, syntax = (POS, 2, 0, 0, 0, BIT), (POS, 1, 1, 0, 0, BIT)
    good = (COUNT, 0, 0, 0, 0, BYTE)
    # each kind alone, on the key of another type too: the arguments are looked at before the key
    for key in (0, 1):
        assert M.apply_stream(ks, names, [key], [bad_bit])[3] == [M.BAD_BIT]  # (a bad bit AND a unit without an end)
        assert M.apply_stream(ks, names, [key], [syntax])[3] == [M.SYNTAX]
    for op in (COUNT, POS, STRLEN, LENGTH):
        rc, replies, status, kinds = M.apply_stream(ks, names, [1], [(op, 1, 0, 0, 0, BYTE)])
        assert (rc, replies, status, kinds) == (M.E_WRONGTYPE, [0], [0xFF], [M.WRONGTYPE])
    # every other command gets its exact reply, and the first failure decides the code and the message
    rc, replies, status, kinds = M.apply_stream(ks, names, [0, 1, 0, 0, 0], [good, good, syntax, bad_bit, good])
    assert (rc, replies, status) == (M.E_WRONGTYPE, [1, 0, 0, 0, 1], [0, 0xFF, 0xFF, 0xFF, 0])
    assert M.message(kinds).startswith("WRONGTYPE")
    rc, _r, _s, kinds = M.apply_stream(ks, names, [0, 1], [syntax, good])
    assert rc == M.E_REDIS and M.message(kinds) == "ERR syntax error"
    # the caller's errors refuse the call
    for key, row in ((2, good), (0, (4, 0, 0, 0, 0, BYTE)), (0, (COUNT, 0, 0, 0, 0, 2)), (0, (POS, 0, 3, 0, 0, BYTE)),
                     (0, (COUNT, 0, 1, 0, 0, BYTE))):
        assert M.apply_stream(ks, names, [0, key], [good, row])[0] == M.E_ILLEGAL_ARGUMENT


# ---- rbx_bitset_range_of against the model ------------------------------------------------------------------------------
def expected_of(data, missing, row):
    """the model's answer over a host string; an existing EMPTY string, which the keyspace model cannot hold, is
    answered from bitrange_model directly"""
    if missing or data:
        ks = BM.Keyspace()
        if not missing:
            ks.data["s"] = data
        return M.run_one(ks, "s", row)
    op, bit, nargs, start, end, unit = row
    if op == POS and bit not in (0, 1):
        return 0, M.BAD_BIT
    if op == POS and nargs < 2 and unit == BIT:
        return 0, M.SYNTAX
    if op == COUNT:
        return RM.bitcount(b"", start, end, unit) if nargs else 0, None
    if op == POS:
        return RM.bitpos_nargs(b"", bit, nargs, start, end, unit), None
    return (0, None) if op == STRLEN else (0, M.SCRIPT)


def range_of(data, missing, row):
    cmd = L.RbxRangeCmd()
    cmd.op, cmd.bit, cmd.nargs, cmd.start, cmd.end, cmd.unit = row
    buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
    out = C.c_int64(77)
    rc = L.lib().rbx_bitset_range_of(buf.ctypes.data_as(L.u8p), len(data), int(missing), C.byref(cmd), C.byref(out))
    return rc, int(out.value), (L.last_error() if rc else "")


def test_range_of_equals_the_model_on_seeded_commands():
    rng = np.random.default_rng(20261021)
    lengths = (0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)
    strings = [(b"", True)] + [(rng.bytes(n), False) for n in lengths] + \
              [(bytes(n), False) for n in (1, 17)] + [(b"\xFF" * n, False) for n in (1, 17, 256)] + \
              [(b"\x80" + bytes(16), False), (b"\x40" + bytes(16), False)]
    checked = 0
    for data, missing in strings:
        for _ in range(160):
            op = int(rng.integers(0, 4))
            unit = int(rng.integers(0, 2))
            nargs = 2 * int(rng.integers(0, 2)) if op == COUNT else int(rng.integers(0, 3))
            bit = int(rng.choice((0, 0, 0, 1, 1, 1, 2, 255)))
            row = (op, bit, nargs, D.bound(rng, len(data), unit), D.bound(rng, len(data), unit), unit)
            reply, kind = expected_of(data, missing, row)
            rc, got, msg = range_of(data, missing, row)
            assert (rc, got) == (M.CODES[kind] if kind else 0, reply), (len(data), missing, row)
            assert msg == (M.MESSAGES[kind] if kind else "")
            checked += 1
    assert checked >= 2000
    # the extremes by hand: no bound overflows
    for start, end in ((INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN), (INT64_MIN, INT64_MIN), (INT64_MAX, INT64_MAX)):
        for unit in (BYTE, BIT):
            for row in ((COUNT, 0, 2, start, end, unit), (POS, 1, 2, start, end, unit), (POS, 0, 1, start, end, BYTE)):
                data = b"\x0F" * 17
                assert range_of(data, False, row)[:2] == (0, expected_of(data, False, row)[0]), row
    bad = L.RBX_E_ILLEGAL_ARGUMENT
    for row in ((4, 0, 0, 0, 0, 0), (COUNT, 0, 1, 0, 0, 0), (POS, 0, 3, 0, 0, 0), (STRLEN, 0, 0, 0, 0, 2)):
        assert range_of(b"\x01", False, row)[0] == bad
    assert L.lib().rbx_bitset_range_of(None, 0, 0, None, None) == bad


# ---- the symbols, the knobs, the caller errors -----------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    for sym in ("rbx_bitset_range_stream", "rbx_bitset_range_stream_dev", "rbx_bitset_range_of"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and re.search(r"\b%s\(" % sym, hdr), sym
    assert hasattr(lib, "rbx_bench_rangestream_last") and "rbx_bench_rangestream_last" in L.SIGNATURES
    assert re.search(r"\brbx_bench_rangestream_last\(", bench)
    assert re.search(r"RBX_RANGE_COUNT = 0, RBX_RANGE_POS = 1, RBX_RANGE_STRLEN = 2, RBX_RANGE_LENGTH = 3", hdr)
    assert (L.RBX_RANGE_COUNT, L.RBX_RANGE_POS, L.RBX_RANGE_STRLEN, L.RBX_RANGE_LENGTH) == (0, 1, 2, 3)
    assert C.sizeof(L.RbxRangeCmd) == 24 and L.RbxRangeCmd.op.offset == 16 and L.RbxRangeCmd.unit.offset == 19
    assert lib.rbx_abi_version() == 1
    import redisson_amd

    for name in ("bitset_range_stream", "bitset_range_stream_call", "bitset_range_stream_dev"):
        assert callable(getattr(redisson_amd, name)) and name in redisson_amd.__all__


def test_the_four_knobs_are_documented_and_range_checked():
    lib = L.lib()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    tun = open(os.path.join(ROOT, "redisson_amd", "csrc", "tunables.h")).read()
    knobs = {"rangestream_lanes": ((0, 2, 3, 12, 128, -1), (4, 8, 32, 64, 16)),
             "rangestream_short_max": ((0, 32, 96, 4097, 1 << 21), (64, 128, 1 << 20, 4096)),
             "rangestream_tile": ((0, 2048, 4097, 12288, 1 << 21), (4096, 1 << 20, 65536)),
             "rangestream_chunk": ((0, -1, (1 << 30) + 1), (1, 1000, 1 << 30, 1 << 25))}
    for key, (refused, taken) in knobs.items():  # (the last value taken is the default)
        assert '"%s"' % key in bench and '"%s"' % key in tun
        for v in refused:
            assert lib.rbx_tune(key.encode(), v) == -1, (key, v)
        for v in taken:
            assert lib.rbx_tune(key.encode(), v) == 0, (key, v)


def test_caller_errors_are_refused_before_any_device_work():
    """the checks run ahead of the context's device: a context pointer that is never dereferenced is enough"""
    lib = L.lib()
    bad = L.RBX_E_ILLEGAL_ARGUMENT
    names, _keep = L.names_array(["a", "b"])
    replies, status = np.zeros(4, np.int64), np.zeros(4, np.uint8)

    def call(keys, rows, ctx=1, names=names, nkeys=2, n=None, cmds=True):
        key = np.array(keys or [0], np.uint32)
        arr = (L.RbxRangeCmd * max(len(rows), 1))()
        for a, (op, bit, nargs, start, end, unit) in zip(arr, rows):
            a.op, a.bit, a.nargs, a.start, a.end, a.unit = op, bit, nargs, start, end, unit
        return lib.rbx_bitset_range_stream(ctx, names, nkeys, key.ctypes.data_as(L.u32p) if keys is not None else None,
                                           arr if cmds else None, len(rows) if n is None else n,
                                           replies.ctypes.data_as(L.i64p), status.ctypes.data_as(L.u8p))

    good = (COUNT, 0, 0, 0, 0, BYTE)
    assert call([0], [good], ctx=None) == bad  # NULL context
    assert call([0], [good], names=None) == bad
    assert call([0, 2], [good, good]) == bad and "nkeys" in L.last_error()  # a key >= nkeys
    assert call([0], [good], nkeys=0, names=None) == bad
    assert call([0], [(4, 0, 0, 0, 0, BYTE)]) == bad  # an op above 3
    assert call([0], [(STRLEN, 0, 0, 0, 0, 2)]) == bad  # a unit above 1
    assert call([0], [(POS, 0, 3, 0, 0, BYTE)]) == bad  # nargs above 2
    assert call([0, 1], [good, (COUNT, 0, 1, 0, 0, BYTE)]) == bad  # BITCOUNT with a start alone
    assert call(None, [good]) == bad and "NULL" in L.last_error()
    assert call([0], [good], cmds=False) == bad
    assert call(None, [], n=0, cmds=False) == L.RBX_OK  # n = 0 sends nothing
    dev = lib.rbx_bitset_range_stream_dev
    assert dev(None, names, 2, 8, 8, 1, None, None, None) == bad and dev(1, names, 2, None, 8, 1, None, None, None) == bad
    assert dev(1, names, 2, None, None, 0, None, None, None) == L.RBX_OK
    assert lib.rbx_bench_rangestream_last(None) == bad


# ---- run_queue, RBatch and the pipeline over a fake engine --------------------------------------------------------------
class Recorder:
    """the range call, the grouped bit call, the bit stream call and RBitSet's single calls over one model keyspace"""

    def __init__(self):
        self.ks = keyspace(a=b"\xF0\x0F", b=b"\x3C\xFF\x01", y=b"\x40\x00")
        self.calls = []

    @staticmethod
    def _k(name):
        return name.decode() if isinstance(name, bytes) else name

    def range_stream_call(self, names, cmd_key, rows):
        assert len(set(names)) == len(names)  # each distinct name once
        names = [self._k(n) for n in names]
        self.calls.append(("ranges", [(names[k], row) for k, row in zip(cmd_key, rows)]))
        rc, replies, status, kinds = M.apply_stream(self.ks, names, cmd_key, rows)
        return ({M.OK: L.RBX_OK, M.E_WRONGTYPE: L.RBX_E_WRONGTYPE, M.E_REDIS: L.RBX_E_REDIS}[rc], M.message(kinds),
                np.array(replies, np.int64), np.array(status, np.uint8))

    def bit_groups_call(self, names, ops, dests, groups):
        names = [self._k(n) for n in names]
        self.calls.append(("groups", len(ops)))
        counts = [self.ks.cardinality("obj", names[g[0]])[0] for g in groups]  # (whole-string BITCOUNTs only)
        return L.RBX_OK, "", np.zeros(len(ops), np.uint64), np.array(counts, np.uint64), np.zeros(len(ops), np.uint8)

    def stream_call(self, names, cmd_key, cmd_op, cmd_index):
        self.calls.append(("bits", len(cmd_key)))
        return L.RBX_OK, "", [0] * len(cmd_key)

    def bitset(self, name):
        rec = self

        class Single:
            def _run(self, what, *args):
                rec.calls.append((what, name, *args))
                reply, err = getattr(rec.ks, what)("obj", name, *args)
                if err:
                    raise RedisException(M.MESSAGES[M.WRONGTYPE if err == BM.WRONGTYPE else M.SCRIPT])
                return reply

            def size(self):
                return self._run("size")

            def length(self):
                return self._run("length")

            def cardinality(self):
                return self._run("cardinality")

            def bitCount(self, start=None, end=None, unit="BYTE"):
                return self._run("bitcount", start, end, unit)

            def bitPos(self, bit, start=None, end=None, unit="BYTE"):
                nargs = 0 if start is None else (1 if end is None else 2)
                return self._run("bitpos", bit, nargs, start or 0, end or 0, unit)

        return Single()

    def batch(self, ranged=True, grouped=True) -> RBatch:
        extra = dict(range_stream_call=self.range_stream_call) if ranged else {}
        if grouped:
            extra["bit_groups_call"] = self.bit_groups_call
        return RBatch(None, stream_call=self.stream_call, bitset=self.bitset, **extra)


def test_a_run_of_read_queries_over_several_keys_is_one_call():
    rec = Recorder()
    b = rec.batch()
    futures = [b.getBitSet("a").sizeAsync(), b.getBitSet("b").lengthAsync(), b.getBitSet("a").bitCountAsync(1, 1),
               b.getBitSet("b").bitCountAsync(-9, -1, "BIT"), b.getBitSet("a").bitPosAsync(0),
               b.getBitSet("b").bitPosAsync(1, 1), b.getBitSet("zz").bitPosAsync(False, 0, -1, "bit"),
               b.getBitSet("zz").size_async(), b.getBitSet("a").bit_count_async(0, 0), b.getBitSet("a").bit_pos_async(1),
               b.getBitSet("a").length_async()]
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["ranges"]
    assert rec.calls[0][1][:4] == [("a", (STRLEN, 0, 0, 0, 0, BYTE)), ("b", (LENGTH, 0, 0, 0, 0, BYTE)),
                                   ("a", (COUNT, 0, 2, 1, 1, BYTE)), ("b", (COUNT, 0, 2, -9, -1, BIT))]
    assert rec.calls[0][1][4:7] == [("a", (POS, 0, 0, 0, 0, BYTE)), ("b", (POS, 1, 1, 1, 0, BYTE)),
                                    ("zz", (POS, 0, 2, 0, -1, BIT))]
    assert res == [16, 24, 4, 2, 4, 8, 0, 0, 4, 0, 16] and [f.get() for f in futures] == res
    assert all(type(r) is int for r in res)


def test_a_cardinality_joins_an_open_range_run_and_starts_a_groups_call():
    rec = Recorder()
    b = rec.batch()
    b.getBitSet("a").sizeAsync()
    b.getBitSet("a").cardinalityAsync()   # joins the range run
    b.getBitSet("b").bitCountAsync()      # BITCOUNT b without a range is cardinalityAsync: joins too
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["ranges"] and res == [16, 8, 13]
    assert rec.calls[0][1][1] == ("a", (COUNT, 0, 0, 0, 0, BYTE))
    rec = Recorder()
    b = rec.batch()
    b.getBitSet("a").cardinalityAsync()   # starts a grouped bit run, as before
    b.getBitSet("a").sizeAsync()          # which a read query closes
    b.getBitSet("b").cardinalityAsync()
    res = b.execute().getResponses()
    assert rec.calls[0] == ("groups", 1) and [c[0] for c in rec.calls] == ["groups", "ranges"] and res == [8, 16, 13]
    # without the grouped call a whole-string BITCOUNT starts a range run
    rec = Recorder()
    b = rec.batch(grouped=False)
    b.getBitSet("a").cardinalityAsync()
    b.getBitSet("a").sizeAsync()
    assert b.execute().getResponses() == [8, 16] and [c[0] for c in rec.calls] == ["ranges"]


def test_a_set_between_two_read_queries_gives_range_bits_range():
    rec = Recorder()
    b = rec.batch()
    b.getBitSet("a").sizeAsync()
    b.getBitSet("s").setAsync(3)
    b.getBitSet("a").lengthAsync()
    b.execute()
    assert [c[0] for c in rec.calls] == ["ranges", "bits", "ranges"]


def test_a_failed_command_raises_its_own_exception_after_every_command_ran():
    rec = Recorder()
    b = rec.batch()
    ok = b.getBitSet("a").sizeAsync()
    wrong = b.getBitSet(HLL).bitCountAsync(0, -1)
    bad_bit = b.getBitSet("a").bitPosAsync(2)
    syntax = b.getBitSet(HLL).bitPosAsync(1, 0, None, "BIT")  # the arguments come before the key's type
    script = b.getBitSet("y").lengthAsync()
    wrong_length = b.getBitSet(HLL).lengthAsync()
    after = b.getBitSet("b").bitPosAsync(1)
    with pytest.raises(RedisException, match="WRONGTYPE Operation against a key"):
        b.execute()  # the first failure
    assert ok.get() == 16 and after.get() == 2
    for f, what in ((wrong, "WRONGTYPE"), (bad_bit, "bit argument must be 1 or 0"), (syntax, "syntax error"),
                    (script, "bit offset is not an integer"), (wrong_length, "WRONGTYPE")):
        with pytest.raises(RedisException, match=what):
            f.get()
    # one call for the run; a failed length() asks its own call which of its two failures it was
    assert [c[0] for c in rec.calls] == ["ranges", "length", "length"]


def test_a_refused_run_fails_every_command_of_it():
    def refuse(*_a):
        return L.RBX_E_ILLEGAL_ARGUMENT, "a command's key is not below nkeys", [], []

    b = RBatch(None, stream_call=None, range_stream_call=refuse)
    f, g = b.getBitSet("a").sizeAsync(), b.getBitSet("a").bitPosAsync(1)
    with pytest.raises(Exception, match="not below nkeys"):
        b.execute()
    for x in (f, g):
        with pytest.raises(Exception, match="not below nkeys"):
            x.get()


def test_without_the_range_call_every_command_runs_singly():
    rec = Recorder()
    b = rec.batch(ranged=False, grouped=False)
    b.getBitSet("a").sizeAsync()
    b.getBitSet("a").lengthAsync()
    b.getBitSet("b").bitCountAsync(1, 1)
    b.getBitSet("b").bitPosAsync(1, 1)
    b.getBitSet("a").cardinalityAsync()
    assert b.execute().getResponses() == [16, 16, 8, 8, 8]
    assert rec.calls == [("size", "a"), ("length", "a"), ("bitcount", "b", 1, 1, "BYTE"),
                         ("bitpos", "b", 1, 1, 1, 0, "BYTE"), ("cardinality", "a")]
    # run_queue itself: the trailing parameter defaults to None, and a range row alone changes nothing
    ran = []
    queue = [_Queued("a", fn=lambda: ran.append("op"), range=_range_row(STRLEN), convert=lambda *_: 1 / 0)]
    assert run_queue(queue, None) == ([None], None) and ran == ["op"]
    assert run_queue(list(queue), None, None, None, None, None, None) == ([None], None) and ran == ["op", "op"]
    queue = [_Queued("a", fn=None, range=_range_row(STRLEN), convert=lambda n: 8 * n)]
    assert run_queue(queue, None, None, None, None, None, None, Recorder().range_stream_call) == ([16], None)
    # argument checks of the methods' own fire when the command is queued
    from redisson_amd import IllegalArgumentException

    with pytest.raises(IllegalArgumentException):
        rec.batch().getBitSet("a").bitCountAsync(1)
    with pytest.raises(IllegalArgumentException):
        rec.batch().getBitSet("a").bitPosAsync(1, None, 3)
    with pytest.raises(IllegalArgumentException):
        rec.batch().getBitSet("a").bitCountAsync(0, 1, "NIBBLE")


def test_the_pipeline_sends_ranged_bitcount_bitpos_and_strlen_as_one_call(monkeypatch):
    import redisson_amd.spring_data as S

    rec = Recorder()
    monkeypatch.setattr(S, "bitset_range_stream_call", lambda client, *a: rec.range_stream_call(*a))
    monkeypatch.setattr(S, "bitset_op_groups_call", lambda client, *a: rec.bit_groups_call(*a))
    monkeypatch.setattr(S, "bitset_stream_call", lambda client, *a: rec.stream_call(*a))
    conn = RedissonConnection(None)
    conn.openPipeline()
    assert conn.bitCount(b"a", 1, 1) is None and conn.bitPos(b"b", True) is None and conn.strLen(b"b") is None
    conn.bitPos(b"a", False, (1, None))
    conn.bitPos(b"a", True, (1, 1))
    conn.bitPos(b"a", True, (None, 5))   # the upper bound travels only behind a bounded lower one
    conn.bitCount(b"a")                   # joins the open run
    conn.setBit(b"s", 1, True)
    conn.bitCount(b"b")                   # starts a grouped run
    conn.strLen(b"zz")
    assert conn.closePipeline() == [4, 2, 3, 8, 12, 0, 8, False, 13, 0]
    assert [c[0] for c in rec.calls] == ["ranges", "bits", "groups", "ranges"]
    assert rec.calls[0][1] == [("a", (COUNT, 0, 2, 1, 1, BYTE)), ("b", (POS, 1, 0, 0, 0, BYTE)),
                               ("b", (STRLEN, 0, 0, 0, 0, BYTE)), ("a", (POS, 0, 1, 1, 0, BYTE)),
                               ("a", (POS, 1, 2, 1, 1, BYTE)), ("a", (POS, 1, 0, 0, 0, BYTE)),
                               ("a", (COUNT, 0, 0, 0, 0, BYTE))]
    conn.openPipeline()
    conn.strLen(b"a")
    conn.bitCount(HLL.encode(), 0, 0)
    conn.bitPos(b"a", True)
    with pytest.raises(RedisException, match="WRONGTYPE"):
        conn.closePipeline()
    assert [c[0] for c in rec.calls][4:] == ["ranges"]


# ---- the seeded driver's plan (test_rangestream_gpu.py runs it on the engine) ---------------------------------------------
def test_the_seeded_plan_keeps_failing_commands_under_the_cap():
    calls = D.seeded_calls()
    assert len(calls) == 200 and all(1 <= len(call[1]) <= 60 for call in calls)
    ks, nm = BM.Keyspace(), D.names("")
    ks.hll.update(nm[D.NKEYS:])
    kinds, ops, long_ones = [], set(), 0
    for writes, cmd_key, rows in calls:
        for w in writes:
            D.write_on_model(ks, nm, w)
        rc, _replies, _status, k = M.apply_stream(ks, nm, cmd_key, rows)
        assert rc != M.E_ILLEGAL_ARGUMENT
        kinds += k
        ops |= {(row[0], row[2], row[5]) for row in rows}
        long_ones += sum(ks.strlen(nm[key]) > 64 for key in cmd_key if key < D.NKEYS)
    failing = sum(k is not None for k in kinds)
    assert 0 < failing <= len(kinds) // 8, (failing, len(kinds))
    assert {k for k in kinds if k} == {M.BAD_BIT, M.SYNTAX, M.WRONGTYPE, M.SCRIPT}
    assert {(op, nargs) for op, nargs, _u in ops} >= {(COUNT, 0), (COUNT, 2), (POS, 0), (POS, 1), (POS, 2), (STRLEN, 0),
                                                      (LENGTH, 0)}
    assert long_ones > len(kinds) // 4  # strings past the test's short_max are common
    assert {w[0] for writes, _k, _r in calls for w in writes} == {"set_bytes", "set", "or", "delete", "expire"}
