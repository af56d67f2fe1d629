"""rbx_hll_stream without a GPU: the model's phase splitter against one command at a time, run_queue / RBatch /
the Spring Data pipeline over a fake hll_stream_call backed by the model, the deliberately wrong streams, and what
the seeded streams of the GPU test contain."""
import os
import re

import pytest

import hll_model as HM
import hllstream_model as M
from hll_model import BITS, BLOOM, WRONGTYPE, Keyspace
from hllstream_model import FAILED, NONE, PFADD, PFCOUNT
from redisson_amd import _lib as L
from redisson_amd.client import RBatch, _Queued, hll_stream_call, run_queue  # noqa: F401
from redisson_amd.exceptions import IllegalStateException, RedisException
from redisson_amd.spring_data import RedissonConnection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS_PER_ROUND = 1137  # the default of "hllstream_elems_per_round" (DESIGN 11.7 has the two measured times behind it)


def prepared(seed) -> Keyspace:
    ks = Keyspace()
    for cmd in M.setup(seed):
        getattr(ks, cmd[0])(*cmd[1:])
    return ks


# ---- the phase splitter -----------------------------------------------------------------------------------------
def at(register, count, serial=1):
    return ("at", serial, ((register, count, 16),))


def test_adds_then_counts_are_two_phases_whatever_the_keys():
    cmds = [(k, PFADD, at(5, 2, i)) for i, k in enumerate("abcab")] + [(k, PFCOUNT, NONE) for k in "abcz"]
    assert M.phases(cmds) == [([], [0, 1, 2, 3, 4]), ([5, 6, 7, 8], [])]


def test_alternating_on_one_key_is_one_phase_per_pair():
    cmds = [("a", PFADD if i % 2 == 0 else PFCOUNT, at(i, 1, i) if i % 2 == 0 else NONE) for i in range(12)]
    got = M.phases(cmds)
    assert len(got) == 7 and got[0] == ([], [0]) and got[1] == ([1], [2]) and got[-1] == ([11], [])
    # count first: n / 2 phases
    cmds = cmds[1:] + [("a", PFADD, at(99, 1, 99))]
    assert M.phases(cmds) == [([2 * i], [2 * i + 1]) for i in range(6)]


def test_a_count_then_an_add_of_one_key_share_a_phase_and_failed_commands_join_none():
    cmds = [("a", PFCOUNT, NONE), ("a", PFADD, at(1, 1)), (BITS, PFADD, at(2, 2)), ("b", PFCOUNT, NONE),
            (BLOOM, PFCOUNT, NONE), ("b", PFADD, NONE)]
    assert M.phases(cmds) == [([0, 3], [1, 5])]
    ks, ks2 = Keyspace(), Keyspace()
    assert M.stream_by_phases(ks, cmds) == M.stream(ks2, cmds) == (WRONGTYPE, [0, 1, 0, 0, 0, 1], [0, 0, FAILED, 0, FAILED, 0])
    assert M.state(ks) == M.state(ks2) and set(ks.keys) == {"a", "b"}


@pytest.mark.parametrize("seed", M.SEEDS)
def test_counts_then_adds_per_phase_equal_one_command_at_a_time(seed):
    a, b = prepared(seed), prepared(seed)
    for cmds in M.seeded(seed):
        assert M.stream_by_phases(a, cmds) == M.stream(b, cmds)
        assert M.state(a) == M.state(b)


# ---- deliberately wrong streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", M.DEFECTS)
def test_the_seeded_streams_catch_a_wrong_stream(defect):
    caught = []
    for seed in M.SEEDS:
        ks = prepared(seed)
        for cmds in M.seeded(seed):
            bad = M.wrong_stream(defect, ks, cmds)
            good = (M.stream(ks, cmds), M.state(ks))
            if bad != good:
                caught.append(seed)
                break
    assert len(caught) >= 3, (defect, caught)


def test_the_seeded_streams_contain_every_event():
    got = M.coverage()
    assert all(v >= 3 for v in got.values()), got


def test_the_model_keeps_the_low_63_bits_and_a_failed_command_creates_nothing():
    ks = Keyspace()
    ks.set("obj", "a", HM.header(1, 1234) + bytes([0x7F, 0xFF]))
    cmds = [("a", PFCOUNT, NONE), ("a", PFADD, NONE), ("a", PFADD, at(9, 3)), ("a", PFADD, at(9, 3)), (BITS, PFADD, at(1, 1)),
            ("z", PFCOUNT, NONE)]
    assert M.stream(ks, cmds) == (WRONGTYPE, [1234, 0, 1, 0, 0, 0], [0, 0, 0, 0, FAILED, 0])
    assert ks.keys["a"].card == HM.INVALID | 1234 and set(ks.keys) == {"a"}


# ---- the symbols and the tunables ---------------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    for sym in ("rbx_hll_stream", "rbx_hll_stream_dev"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and re.search(r"\b%s\(" % sym, hdr), sym
    assert hasattr(lib, "rbx_bench_hllstream_last") and re.search(r"\brbx_bench_hllstream_last\(", bench)
    assert (L.RBX_HLL_PFADD, L.RBX_HLL_PFCOUNT) == (0, 1)
    assert re.search(r"RBX_HLL_PFADD = 0, RBX_HLL_PFCOUNT = 1", hdr)


def test_null_context_and_null_arrays_are_the_callers_error():
    assert L.lib().rbx_hll_stream(None, None, 0, None, None, None, 0, None, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_hll_stream_dev(None, None, 0, None, None, None, 1, None, None, None, None) == L.RBX_E_ILLEGAL_ARGUMENT


def test_tunables_documented_and_range_checked():
    """each key is documented, refuses values outside its range, takes the ones inside, and is left at its default
    (the last accepted value, which is tunables.h's and the one rbx_bench.h documents)"""
    lib = L.lib()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    tun = open(os.path.join(ROOT, "redisson_amd", "csrc", "tunables.h")).read()
    for key, field, good, bad in ((b"hllstream_path", "hllstream_path", (1, 2, 0), (3, -1)),
                                  (b"hllstream_chunk", "hllstream_chunk", (1, 256, 1 << 25), (0, (1 << 30) + 1)),
                                  (b"hllstream_elems_per_round", "hllstream_elems_per_round", (1, 4096, ELEMS_PER_ROUND), (0,))):
        assert '"%s"' % key.decode() in bench, key
        for v in bad:
            assert lib.rbx_tune(key, v) == -1, (key, v)
        for v in good:
            assert lib.rbx_tune(key, v) == 0, (key, v)
        m = re.search(r"%s\{([^}]*)\}" % field, tun)  # the default in tunables.h: a number or 1 << k
        assert m and eval(m.group(1), {"__builtins__": {}}) == good[-1], (key, m and m.group(1))


# ---- run_queue, RBatch and the pipeline over a fake engine ------------------------------------------------------
class Recorder:
    """hll_stream_call, the single HLL calls and the bit stream call over one model keyspace; calls are logged"""

    def __init__(self):
        self.ks = Keyspace()
        self.calls = []

    @staticmethod
    def _k(name):
        return name.decode() if isinstance(name, bytes) else name

    def hll_stream_call(self, names, cmd_key, cmd_op, seg, elements):
        cmds = [(self._k(names[k]), op, ("lit", tuple(elements[seg[i]:seg[i + 1]])))
                for i, (k, op) in enumerate(zip(cmd_key, cmd_op))]
        self.calls.append(("hll", [(k, op, len(s[1])) for k, op, s in cmds]))
        kind, replies, status = M.stream(self.ks, cmds)
        return (L.RBX_E_WRONGTYPE if kind else L.RBX_OK), ("WRONGTYPE" if kind else ""), replies, status

    def stream_call(self, names, cmd_key, cmd_op, cmd_index):
        self.calls.append(("bits", len(cmd_key)))
        return L.RBX_OK, "", [0] * len(cmd_key)

    def hyperloglog(self, name, codec):
        rec = self

        class Single:
            def mergeWith(self, *others):
                rec.calls.append(("merge", name, others))
                return rec.ks.pfmerge("obj", name, others)[0]

            def countWith(self, *others):
                rec.calls.append(("countWith", name, others))
                return rec.ks.pfcount_multi("obj", name, others)[0]

        return Single()

    def batch(self) -> RBatch:
        return RBatch(None, stream_call=self.stream_call, hll_stream_call=self.hll_stream_call,
                      hyperloglog=self.hyperloglog)


def test_one_call_per_maximal_hll_run_and_replies_in_submission_order():
    rec = Recorder()
    b = rec.batch()
    futures = [b.getHyperLogLog("a").addAsync("x"), b.getHyperLogLog("b").addAllAsync(["x", "y"]),
               b.getHyperLogLog("a").countAsync(), b.getHyperLogLog("a").addAsync("x"),
               b.getHyperLogLog("z").countAsync(), b.getHyperLogLog("b").addAllAsync([])]
    res = b.execute().getResponses()
    assert rec.calls == [("hll", [("a", PFADD, 1), ("b", PFADD, 2), ("a", PFCOUNT, 0), ("a", PFADD, 1), ("z", PFCOUNT, 0),
                                  ("b", PFADD, 0)])]
    assert res == [True, True, 1, False, 0, False] and [f.get() for f in futures] == res
    assert type(res[0]) is bool and type(res[2]) is int


def test_a_bit_command_or_a_merge_splits_the_runs():
    rec = Recorder()
    b = rec.batch()
    b.getHyperLogLog("a").addAsync("x")
    b.getBitSet("s").setAsync(3)
    b.getBitSet("s").getAsync(3)
    b.getHyperLogLog("a").addAsync("y")
    b.getHyperLogLog("b").countAsync()
    b.getHyperLogLog("b").mergeWithAsync("a")
    b.getHyperLogLog("b").countWithAsync("a")
    b.getHyperLogLog("b").countWithAsync()
    b.getHyperLogLog("b").addAsync("y")
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["hll", "bits", "hll", "merge", "countWith", "hll"]
    assert rec.calls[1] == ("bits", 2) and [len(c[1]) for c in rec.calls if c[0] == "hll"] == [1, 2, 2]
    assert res == [True, False, False, True, 0, None, 2, 2, False]


def test_a_command_that_failed_alone_raises_after_everything_ran():
    rec = Recorder()
    b = rec.batch()
    ok = b.getHyperLogLog("a").addAsync("x")
    bad = b.getHyperLogLog(BITS).addAsync("x")
    bad2 = b.getHyperLogLog(BLOOM).countAsync()
    after = b.getHyperLogLog("a").countAsync()
    with pytest.raises(RedisException, match="WRONGTYPE Key is not a valid HyperLogLog"):
        b.execute()
    assert ok.get() is True and after.get() == 1 and set(rec.ks.keys) == {"a"}
    for f in (bad, bad2):
        with pytest.raises(RedisException, match="WRONGTYPE"):
            f.get()
    with pytest.raises(IllegalStateException, match="Batch already executed"):
        b.execute()
    with pytest.raises(IllegalStateException, match="Batch already executed"):
        b.getHyperLogLog("a").addAsync("y")


def test_run_queue_without_the_parameter_runs_hll_commands_singly():
    ran = []
    queue = [_Queued("a", fn=lambda: ran.append("single") or True, hll=(PFADD, [b"x"])),
             _Queued("a", fn=lambda: ran.append("single") or 1, hll=(PFCOUNT, []))]
    responses, error = run_queue(queue, None, None)
    assert ran == ["single", "single"] and responses == [True, 1] and error is None
    rec = Recorder()
    queue = [_Queued("a", fn=None, hll=(PFADD, [b"x"])), _Queued("a", fn=None, hll=(PFCOUNT, []), convert=lambda v: v + 10)]
    responses, error = run_queue(queue, None, None, rec.hll_stream_call)
    assert responses == [True, 11] and error is None and len(rec.calls) == 1


def test_a_refused_run_fails_every_command_of_it():
    def refuse(*_a):
        return L.RBX_E_ILLEGAL_ARGUMENT, "a command's key is not below nkeys", [], []

    b = RBatch(None, stream_call=None, hll_stream_call=refuse)
    f = b.getHyperLogLog("a").addAsync("x")
    with pytest.raises(Exception, match="not below nkeys"):
        b.execute()
    with pytest.raises(Exception, match="not below nkeys"):
        f.get()


def test_the_pipeline_coalesces_pfadd_and_single_key_pfcount(monkeypatch):
    import redisson_amd.spring_data as S

    rec = Recorder()
    singles = []
    monkeypatch.setattr(S, "hll_stream_call", lambda client, *a: rec.hll_stream_call(*a))
    monkeypatch.setattr(S, "bitset_stream_call", lambda client, *a: rec.stream_call(*a))
    conn = RedissonConnection(None)
    monkeypatch.setattr(RedissonConnection, "pfMerge", S._pipelined(lambda self, d, *s: singles.append(("merge", d, s))))
    multi = S._pipelined(hll=S._pf_count)(lambda self, *keys: singles.append(("count", keys)) or 7)
    monkeypatch.setattr(RedissonConnection, "pfCount", multi)
    conn.openPipeline()
    assert conn.pfAdd(b"a", b"x", b"y") is None and conn.pfAdd(b"b") is None and conn.pfCount(b"a") is None
    conn.pfCount(b"a", b"b")
    conn.pfAdd(b"a", b"x")
    conn.getBit(b"s", 1)
    conn.pfAdd(BITS.encode(), b"x")
    conn.pfCount(b"b")
    conn.pfMerge(b"b", b"a")
    conn.pfCount(b"b")
    with pytest.raises(RedisException, match="WRONGTYPE"):
        conn.closePipeline()
    assert [c[0] for c in rec.calls] == ["hll", "hll", "bits", "hll", "hll"]
    assert rec.calls[0][1] == [("a", PFADD, 2), ("b", PFADD, 0), ("a", PFCOUNT, 0)]
    assert rec.calls[3][1] == [(BITS, PFADD, 1), ("b", PFCOUNT, 0)]
    assert singles == [("count", (b"a", b"b")), ("merge", b"b", (b"a",))]
    conn.openPipeline()
    conn.pfAdd(b"q", b"x")
    conn.pfAdd(b"q", b"x")
    conn.pfCount(b"q")
    assert conn.closePipeline() == [1, 0, 1]
