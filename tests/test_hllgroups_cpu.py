"""rbx_hll_count_groups / rbx_hll_merge_groups without a GPU: the model against one command at a time and against
the deliberately wrong models (on the very inputs the GPU file runs), the phase rule restated, run_queue / RBatch /
the Spring Data pipeline over recording stand-ins backed by the model, the symbols, the tunable and the caller
errors the library checks before it touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hll_model as HM
import hllgroups_model as G
import hllstream_model as SM
from hll_model import BITS, BLOOM, WRONGTYPE, Keyspace
from hllgroups_model import FAILED, at
from redisson_amd import _lib as L
from redisson_amd.client import RBatch, _Queued, run_queue
from redisson_amd.exceptions import RedisException
from redisson_amd.spring_data import RedissonConnection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ------------------------------------------------------------------------------------------------------
def test_counts_one_entry_is_the_cached_count_and_two_are_a_union():
    ks = Keyspace()
    ks.set("obj", "k0", HM.header(1, 4321) + bytes([0x7F, 0xFF]))  # a valid cache that is wrong
    ks.pfadd("obj", "k1", at(7, 2))
    got = G.count_groups(ks, [("k0",), ("k0", "k0"), ("k0", "k1"), ("k9",), ("k9", "k8"), (BITS, "k0"), ("k1",)])
    assert got == (WRONGTYPE, [4321, 0, 1, 0, 0, 0, 1], [0, 0, 0, 0, 0, FAILED, 0])
    assert ks.keys["k0"].card == 4321 and ks.keys["k1"].card == 1 and set(ks.keys) == {"k0", "k1"}


def test_merges_see_earlier_merges_and_fail_alone():
    ks = Keyspace()
    ks.pfadd("obj", "k1", at(5, 3))
    ks.pfadd("obj", "k2", at(9, 2))
    merges = [("k0", ("k1",)), (BLOOM, ("k1",)), ("k3", ("k0", BITS)), ("k1", ("k2",)), ("k4", ("k0", "k1"))]
    assert G.merge_groups(ks, merges) == (WRONGTYPE, [0, FAILED, FAILED, 0, 0])
    assert set(ks.keys) == {"k0", "k1", "k2", "k4"}
    assert G.union_count(ks, ["k0"]) == 1 and G.union_count(ks, ["k4"]) == 2
    assert ks.keys["k4"].card == HM.INVALID and not ks.keys["k4"].dense


def test_the_phase_rule_restated():
    assert G.merge_phases([]) == []
    assert G.merge_phases([("a", ("b",)), ("c", ("a",))]) == [[0], [1]]  # read after write
    assert G.merge_phases([("a", ("b",)), ("b", ("c",))]) == [[0], [1]]  # write after read
    assert G.merge_phases([("a", ("b",)), ("a", ("c",))]) == [[0], [1]]  # write after write
    assert G.merge_phases([("a", ("a", "b"))]) == [[0]]
    assert G.merge_phases([("a", ("a", "b")), ("c", ("b", "d"))]) == [[0, 1]]
    assert G.merge_phases([("a", ("b",)), ("b", (BITS,)), ("c", ("a",))]) == [[0], [2]]
    assert G.merge_phases([("a", ("b",)), ("a", (BLOOM,)), ("d", ("b",))]) == [[0, 2]]
    assert G.merge_phases([(BITS, ())]) == []
    assert G.merge_phases([("k%d" % (i + 1), ("k%d" % i,)) for i in range(50)]) == [[i] for i in range(50)]
    assert G.merge_phases([("d%d" % i, ("s%d" % i, "s%d" % (i + 1))) for i in range(300)]) == [list(range(300))]


def test_executing_by_phases_equals_one_at_a_time():
    """within a phase the merges read the state before it: that equals array order on the seeded merges"""
    for seed in G.SEEDS:
        ks = G.prepared(G.setup(seed))
        for step in G.seeded(seed):
            if step[0] != "merge":
                G.apply_step(ks, step)
                continue
            merges = step[1]
            by_phase = G.copy_keyspace(ks)
            for phase in G.merge_phases(merges):
                before = G.copy_keyspace(by_phase)
                for i in phase:
                    dest, srcs = merges[i]
                    tmp = []
                    for j, s in enumerate(srcs):  # sources as they stood before the phase, the destination itself aside
                        if s != dest and s in before.keys:
                            by_phase.keys["\0%d" % j] = HM.Hll(HM.clone(before.keys[s].h), before.keys[s].card, False)
                        tmp.append(s if s == dest else "\0%d" % j)
                    by_phase.pfmerge("groups", dest, tuple(tmp))
                    for j in range(len(srcs)):
                        by_phase.keys.pop("\0%d" % j, None)
            G.merge_groups(ks, merges)
            assert G.state(by_phase) == G.state(ks), (seed, merges)


def test_every_wrong_model_differs_on_an_input_of_the_gpu_file():
    caught = {d: [] for d in G.DEFECTS}
    for name, (setup, merges, groups) in G.CASES.items():
        ks = G.prepared(setup)
        ref = G.copy_keyspace(ks)
        want = (G.merge_groups(ref, merges), G.count_groups(ref, groups), G.state(ref))
        for d in G.DEFECTS:
            if G.wrong_groups(d, ks, merges, groups) != want:
                caught[d].append(name)
    assert caught["snapshot"] and "raw" in caught["snapshot"], caught
    assert "war" in caught["no_war"] and "union_cache" in caught["cache"], caught
    assert "no_sources" in caught["no_inval"] and "dense_source" in caught["dest"], caught
    # and the seeded sequences catch the ordering defects too
    seeded = {d: 0 for d in ("snapshot", "no_war")}
    for seed in G.SEEDS:
        ks = G.prepared(G.setup(seed))
        for step in G.seeded(seed):
            if step[0] == "merge":
                ref = G.copy_keyspace(ks)
                want = (G.merge_groups(ref, step[1]), G.count_groups(ref, []), G.state(ref))
                for d in seeded:
                    seeded[d] += G.wrong_groups(d, ks, step[1]) != want
            G.apply_step(ks, step)
    assert all(seeded.values()), seeded


def test_the_seeded_sequences_contain_what_they_are_for():
    kinds, hazards, failed = set(), 0, 0
    for seed in G.SEEDS:
        for step in G.seeded(seed):
            kinds.add(step[0])
            if step[0] == "merge":
                hazards += len(G.merge_phases(step[1])) > 1
                failed += any(G.wrong(d, *s) for d, s in step[1])
    assert kinds == {"count", "merge", "stream", "countWith", "mergeWith", "set", "delete"}
    assert hazards >= 10 and failed >= 1


# ---- the symbols, the tunable, the caller errors ------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    for sym in ("rbx_hll_count_groups", "rbx_hll_merge_groups"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and re.search(r"\b%s\(" % sym, hdr), sym
    assert hasattr(lib, "rbx_bench_hllgroups_last") and "rbx_bench_hllgroups_last" in L.SIGNATURES
    assert re.search(r"\brbx_bench_hllgroups_last\(", bench)
    import redisson_amd

    for name in ("hll_count_groups", "hll_count_groups_call", "hll_merge_groups", "hll_merge_groups_call"):
        assert callable(getattr(redisson_amd, name)) and name in redisson_amd.__all__


def test_the_split_knob_is_documented_and_range_checked():
    lib = L.lib()
    bench = open(os.path.join(ROOT, "include", "rbx_bench.h")).read()
    tun = open(os.path.join(ROOT, "redisson_amd", "csrc", "tunables.h")).read()
    assert '"hllgroups_split"' in bench and '"hllgroups_split"' in tun
    for v in (-1, 3, 5, 32, 17):
        assert lib.rbx_tune(b"hllgroups_split", v) == -1, v
    for v in (1, 2, 4, 8, 16, 0):
        assert lib.rbx_tune(b"hllgroups_split", v) == 0, v
    assert re.search(r"hllgroups_split\{0\}", tun)


def test_caller_errors_are_refused_before_any_device_work():
    """the checks run ahead of the context's device: a context pointer that is never dereferenced is enough"""
    lib = L.lib()
    bad = L.RBX_E_ILLEGAL_ARGUMENT
    u64 = lambda *x: np.array(x, np.uint64)  # noqa: E731
    u32 = lambda *x: np.array(x or (0,), np.uint32)  # noqa: E731
    out, status = np.zeros(4, np.uint64), np.zeros(4, np.uint8)
    names, _keep = L.names_array(["a", "b"])

    def count(off, key, n, nkeys=2, ctx=1, names=names, out=out):
        return lib.rbx_hll_count_groups(ctx, names, nkeys, off.ctypes.data_as(L.u64p) if off is not None else None,
                                        key.ctypes.data_as(L.u32p) if key is not None else None, n,
                                        out.ctypes.data_as(L.u64p) if out is not None else None, status.ctypes.data_as(L.u8p))

    def merge(dest, off, key, n, nkeys=2, ctx=1):
        return lib.rbx_hll_merge_groups(ctx, names, nkeys, dest.ctypes.data_as(L.u32p) if dest is not None else None,
                                        off.ctypes.data_as(L.u64p) if off is not None else None,
                                        key.ctypes.data_as(L.u32p) if key is not None else None, n, status.ctypes.data_as(L.u8p))

    assert count(u64(0, 1), u32(0), 1, ctx=None) == bad  # NULL context
    assert count(u64(0, 1), u32(0), 1, names=None) == bad
    assert count(u64(0, 1, 1), u32(0), 2) == bad  # a group with no entries
    assert count(u64(0, 1), u32(2), 1) == bad  # an entry >= nkeys
    assert count(u64(1, 2), u32(0, 1), 1) == bad  # offsets from 1
    assert count(u64(0, 2, 1), u32(0, 1), 2) == bad  # descending
    assert count(None, u32(0), 1) == bad and count(u64(0, 1), None, 1) == bad and count(u64(0, 1), u32(0), 1, out=None) == bad
    assert "NULL" in L.last_error()
    assert merge(u32(0), u64(0, 1), u32(2), 1) == bad and merge(u32(2), u64(0, 1), u32(1), 1) == bad
    assert merge(None, u64(0, 1), u32(1), 1) == bad and merge(u32(0), None, u32(1), 1) == bad
    assert merge(u32(0), u64(0, 1), None, 1) == bad and merge(u32(0), u64(0, 1), u32(1), 1, ctx=None) == bad
    assert merge(u32(0, 1), u64(0, 2, 1), u32(1, 0), 2) == bad
    # ngroups = 0 sends nothing
    assert count(None, None, 0) == L.RBX_OK and merge(None, None, None, 0) == L.RBX_OK


# ---- run_queue, RBatch and the pipeline over a fake engine ------------------------------------------------------------
class Recorder:
    """the grouped calls, the HLL stream call, the single HLL calls and the bit stream call over one model keyspace"""

    def __init__(self):
        self.ks = Keyspace()
        self.calls = []

    @staticmethod
    def _k(name):
        return name.decode() if isinstance(name, bytes) else name

    def hll_count_groups_call(self, names, groups):
        groups = [tuple(self._k(names[k]) for k in g) for g in groups]
        self.calls.append(("counts", groups))
        assert len(set(names)) == len(names)  # each distinct name once
        kind, counts, status = G.count_groups(self.ks, groups)
        return (L.RBX_E_WRONGTYPE if kind else L.RBX_OK), ("WRONGTYPE" if kind else ""), counts, status

    def hll_merge_groups_call(self, names, dests, groups):
        merges = [(self._k(names[d]), tuple(self._k(names[k]) for k in g)) for d, g in zip(dests, groups)]
        self.calls.append(("merges", merges))
        assert len(set(names)) == len(names)
        kind, status = G.merge_groups(self.ks, merges)
        return (L.RBX_E_WRONGTYPE if kind else L.RBX_OK), ("WRONGTYPE" if kind else ""), status

    def hll_stream_call(self, names, cmd_key, cmd_op, seg, elements):
        cmds = [(self._k(names[k]), op, ("lit", tuple(elements[seg[i]:seg[i + 1]])))
                for i, (k, op) in enumerate(zip(cmd_key, cmd_op))]
        self.calls.append(("hll", len(cmds)))
        kind, replies, status = SM.stream(self.ks, cmds)
        return (L.RBX_E_WRONGTYPE if kind else L.RBX_OK), ("WRONGTYPE" if kind else ""), replies, status

    def stream_call(self, names, cmd_key, cmd_op, cmd_index):
        self.calls.append(("bits", len(cmd_key)))
        return L.RBX_OK, "", [0] * len(cmd_key)

    def hyperloglog(self, name, codec):
        rec = self

        class Single:
            def mergeWith(self, *others):
                rec.calls.append(("merge", name, others))
                reply, err = rec.ks.pfmerge("obj", name, others)
                if err:
                    raise RedisException("WRONGTYPE Key is not a valid HyperLogLog string value.")
                return reply

            def countWith(self, *others):
                rec.calls.append(("countWith", name, others))
                return rec.ks.pfcount_multi("obj", name, others)[0]

        return Single()

    def batch(self, grouped=True) -> RBatch:
        extra = dict(hll_count_groups_call=self.hll_count_groups_call, hll_merge_groups_call=self.hll_merge_groups_call)
        return RBatch(None, stream_call=self.stream_call, hll_stream_call=self.hll_stream_call,
                      hyperloglog=self.hyperloglog, **(extra if grouped else {}))


def queue_mixed(b):
    return [b.getHyperLogLog("a").addAsync("x"),                # stream
            b.getHyperLogLog("a").countAsync(),                 # stream
            b.getHyperLogLog("a").countWithAsync("b"),          # counts
            b.getHyperLogLog("b").countWithAsync("a", "c"),     # counts
            b.getHyperLogLog("a").countWithAsync("a"),          # counts
            b.getHyperLogLog("c").mergeWithAsync("a"),          # merges
            b.getHyperLogLog("d").mergeWithAsync("c", "a"),     # merges
            b.getHyperLogLog("c").countWithAsync("d"),          # counts
            b.getHyperLogLog("b").addAsync("y"),                # stream
            b.getBitSet("s").getAsync(3),                       # bits
            b.getHyperLogLog("e").mergeWithAsync(),             # merges
            b.getHyperLogLog("e").countWithAsync(),             # stream: no other name is the single-key count
            b.getHyperLogLog("e").countWithAsync("b")]          # counts


def test_runs_split_where_the_rule_says_and_are_one_call_each():
    rec = Recorder()
    b = rec.batch()
    futures = queue_mixed(b)
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["hll", "counts", "merges", "counts", "hll", "bits", "merges", "hll", "counts"]
    assert rec.calls[1][1] == [("a", "b"), ("b", "a", "c"), ("a", "a")]
    assert rec.calls[2][1] == [("c", ("a",)), ("d", ("c", "a"))]
    assert rec.calls[6][1] == [("e", ())]
    assert res == [True, 1, 1, 1, 1, None, None, 1, True, False, None, 0, 1]
    assert [f.get() for f in futures] == res and type(res[2]) is int


def test_without_the_new_calls_everything_runs_singly():
    rec = Recorder()
    b = rec.batch(grouped=False)
    queue_mixed(b)
    res = b.execute().getResponses()
    assert [c[0] for c in rec.calls] == ["hll", "countWith", "countWith", "countWith", "merge", "merge", "countWith", "hll",
                                         "bits", "merge", "hll", "countWith"]
    assert res == [True, 1, 1, 1, 1, None, None, 1, True, False, None, 0, 1]
    # and run_queue itself: the two trailing parameters default to None
    ran = []
    queue = [_Queued("a", fn=lambda: ran.append("c") or 5, group=("count", ["a", "b"])),
             _Queued("a", fn=lambda: ran.append("m"), group=("merge", "a", ["b"]))]
    assert run_queue(queue, None) == ([5, None], None) and ran == ["c", "m"]
    queue = [_Queued("a", fn=None, group=("count", ["a", "b"])), _Queued("a", fn=None, group=("merge", "a", ["b"])),
             _Queued("a", fn=None, group=("count", ["a", "b"]), convert=lambda v: v + 10)]
    responses, error = run_queue(queue, None, None, None, rec.hll_count_groups_call, rec.hll_merge_groups_call)
    assert responses == [2, None, 12] and error is None  # a holds x, b holds y


def test_a_failed_group_settles_only_its_own_future():
    rec = Recorder()
    b = rec.batch()
    b.getHyperLogLog("a").addAsync("x")
    ok = b.getHyperLogLog("a").countWithAsync("b")
    bad = b.getHyperLogLog("a").countWithAsync(BITS)
    ok2 = b.getHyperLogLog("b").countWithAsync("a")
    m_bad = b.getHyperLogLog(BLOOM).mergeWithAsync("a")
    m_ok = b.getHyperLogLog("c").mergeWithAsync("a")
    m_bad2 = b.getHyperLogLog("d").mergeWithAsync("a", BITS)
    after = b.getHyperLogLog("c").countWithAsync("z")
    with pytest.raises(RedisException, match="WRONGTYPE Key is not a valid HyperLogLog"):
        b.execute()
    assert ok.get() == 1 and ok2.get() == 1 and m_ok.get() is None and after.get() == 1
    for f in (bad, m_bad, m_bad2):
        with pytest.raises(RedisException, match="WRONGTYPE"):
            f.get()
    assert set(rec.ks.keys) == {"a", "c"} and [c[0] for c in rec.calls] == ["hll", "counts", "merges", "counts"]


def test_a_refused_run_fails_every_command_of_it():
    def refuse(*_a):
        return L.RBX_E_ILLEGAL_ARGUMENT, "a group's key is not below nkeys", [], []

    b = RBatch(None, stream_call=None, hll_count_groups_call=refuse)
    f, g = b.getHyperLogLog("a").countWithAsync("b"), b.getHyperLogLog("a").countWithAsync("c")
    with pytest.raises(Exception, match="not below nkeys"):
        b.execute()
    for x in (f, g):
        with pytest.raises(Exception, match="not below nkeys"):
            x.get()


def test_the_pipeline_groups_multi_key_pfcount_and_pfmerge(monkeypatch):
    import redisson_amd.spring_data as S

    rec = Recorder()
    monkeypatch.setattr(S, "hll_stream_call", lambda client, *a: rec.hll_stream_call(*a))
    monkeypatch.setattr(S, "hll_count_groups_call", lambda client, *a: rec.hll_count_groups_call(*a))
    monkeypatch.setattr(S, "hll_merge_groups_call", lambda client, *a: rec.hll_merge_groups_call(*a))
    monkeypatch.setattr(S, "bitset_stream_call", lambda client, *a: rec.stream_call(*a))
    conn = RedissonConnection(None)
    conn.openPipeline()
    assert conn.pfAdd(b"a", b"x", b"y") is None and conn.pfCount(b"a") is None
    assert conn.pfCount(b"a", b"b") is None and conn.pfCount(b"b", b"a", b"a") is None
    assert conn.pfMerge(b"c", b"a") is None and conn.pfMerge(b"d") is None and conn.pfMerge(b"c", BITS.encode()) is None
    conn.pfCount(b"c", b"d")
    conn.getBit(b"s", 1)
    conn.pfCount(b"c", b"d")
    conn.pfCount(b"c")
    with pytest.raises(RedisException, match="WRONGTYPE"):
        conn.closePipeline()
    assert [c[0] for c in rec.calls] == ["hll", "counts", "merges", "counts", "bits", "counts", "hll"]
    assert rec.calls[1][1] == [("a", "b"), ("b", "a", "a")]
    assert rec.calls[2][1] == [("c", ("a",)), ("d", ()), ("c", (BITS,))]
    conn.openPipeline()
    conn.pfCount(b"a", b"c")
    conn.pfMerge(b"e", b"a")
    conn.pfCount(b"e", b"zz")
    assert conn.closePipeline() == [2, None, 2]
