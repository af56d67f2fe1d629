"""Bloom filter command sequences on the GPU against the keyspace model (bloom_driver.py, bloom_model.py), and a few
targeted cases at the turns a sequence reaches only by luck.

The sequences: add / contains by object, by name with and without a cached config, asynchronously, through handles on
device keys, through the multi-tenant calls and the ordered stream in their host and device forms, take turns with
DEL, RENAME, PEXPIRE, SET and RBitSet commands on nine shared filters, each seed under knob settings of its own; every
reply, error kind and -- every 10 commands -- every filter's exported string, config, PTTL sign, count() and 200
contains replies over three paths equal the model.  What they are there to check is the host state of api_bloom.cpp,
api_bloom_multi.cpp, api_staging.cpp and keyspace.cpp (the cached descriptor table, the handles' re-binding, the
length word, the choice of path, the order of replies across paths).

A failure names its seed and step; bloom_driver.run(engine, seed, STEPS, stop_at=step + 1) replays it."""
import contextlib

import pytest

import bloom_driver as D
import bloom_model as M
from redisson_amd import _lib as L
from test_bloom_sequences_cpu import SEEDS, STEPS

pytestmark = pytest.mark.gpu

DEFAULTS = {"add_partition": 2, "contains_partition": 2, "add_records": 2, "add_single_seg_keys": 256, "add_one_key": 1,
            "contains_stage1_grid": 256, "host_small_batches": 1, "host_tiny_keys": 16384, "host_tiny_spin": 1,
            "host_small_bytes": 4 << 20, "contains_multi_slots": 2, "add_multi_table8": 2, "add_multi_conflict_log2": 17,
            "add_multi_segment": 1, "add_multi_segmax": 16384, "stream_table8": 1, "stream_chunk": 0}
GROUPS = {"partition": ("add_partition", "contains_partition", "add_records", "contains_stage1_grid"),
          "single": ("add_single_seg_keys", "add_one_key"),
          "host": ("host_small_batches", "host_tiny_keys", "host_tiny_spin", "host_small_bytes"),
          "multi": ("contains_multi_slots", "add_multi_table8", "add_multi_conflict_log2", "add_multi_segment",
                    "add_multi_segmax"),
          "stream": ("stream_table8", "stream_chunk")}
# The knobs each seed runs under; a knob that is not named keeps its default.  With add_partition = 1 and
# contains_partition = 1 the 65,537-bit and the 5,000,011-bit filter take the partitioned kernels at every batch size
# (k <= 16, size >= 2^15); add_single_seg_keys = 0 and add_one_key = 0 send the small adds there too, or to the table.
SETTINGS = {
    0: {},
    1: dict(add_partition=1, contains_partition=1, add_records=0, add_single_seg_keys=0, host_tiny_keys=0),
    2: dict(add_partition=1, contains_partition=1, add_records=1, contains_stage1_grid=1, add_one_key=0, stream_chunk=37),
    3: dict(add_partition=1, add_records=3, host_small_batches=0, contains_multi_slots=0, add_multi_table8=0),
    4: dict(contains_partition=1, host_small_bytes=65536, contains_multi_slots=1, add_multi_segment=0, stream_table8=0),
    5: dict(add_partition=1, contains_partition=1, add_single_seg_keys=0, add_one_key=0, host_tiny_spin=0,
            add_multi_segmax=300, add_multi_conflict_log2=6),
    6: dict(host_tiny_keys=0, host_small_bytes=65536, add_multi_segmax=300, stream_chunk=37, stream_table8=0),
    7: dict(add_partition=1, contains_partition=1, add_records=3, contains_stage1_grid=1, add_multi_conflict_log2=6,
            add_multi_table8=0, host_tiny_spin=0),
}
COVER = {"add_partition": {1, 2}, "contains_partition": {1, 2}, "add_records": {0, 1, 2, 3},
         "add_single_seg_keys": {0, 256}, "add_one_key": {0, 1}, "contains_stage1_grid": {1, 256},
         "host_small_batches": {0, 1}, "host_tiny_keys": {0, 16384}, "host_tiny_spin": {0, 1},
         "host_small_bytes": {65536, DEFAULTS["host_small_bytes"]}, "contains_multi_slots": {0, 1, 2},
         "add_multi_table8": {0, 2}, "add_multi_conflict_log2": {6, 17}, "add_multi_segment": {0, 1},
         "add_multi_segmax": {300, 16384}, "stream_table8": {0, 1}, "stream_chunk": {0, 37}}

# a key one of whose indexes is the last bit of the 65,537-bit filter, the only one its last byte holds (all k = 10
# indexes there would take 65537^10 candidates): added alone to an empty filter, it alone makes the string 8,193 bytes
LAST_SIZE = D.CONFIGS[D.REGION][0]
LAST_KEY = D.crafted_last_bit_key()


@contextlib.contextmanager
def tuned(knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            L.lib().rbx_tune(k.encode(), v)


def test_the_settings_cover_every_knob_value():
    def seen(knob):
        return {SETTINGS[s].get(knob, DEFAULTS[knob]) for s in SEEDS}

    assert set(SETTINGS) == set(SEEDS) and set(COVER) == set(DEFAULTS) == {k for g in GROUPS.values() for k in g}
    for knob, values in COVER.items():
        assert seen(knob) == values, knob
    assert any(SETTINGS[s] == {} for s in SEEDS)  # one seed at all defaults
    for s in SEEDS:  # no seed changes one group alone
        touched = {g for g, knobs in GROUPS.items() if any(k in SETTINGS[s] for k in knobs)}
        assert len(touched) != 1, s


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_equals_the_model(client, fresh, seed):
    engine = D.GpuEngine(client, fresh + ":")
    try:
        with tuned(SETTINGS[seed]):
            D.run(engine, seed, STEPS)
    finally:
        engine.shutdown()


# ---- targeted --------------------------------------------------------------------------------------------------------
class Pair:
    """the same commands to the engine and to the model, replies compared (names live under the test's prefix)"""

    def __init__(self, client, prefix):
        self.engine, self.model = D.GpuEngine(client, prefix), M.BloomKeyspace()

    def do(self, *cmd):
        got, want = D.call(self.engine, cmd), D.call(self.model, cmd)
        assert got == want, f"{D.short(cmd)!r}: engine / model: {D.first_difference(got[0], want[0])} ({got[1]!r} / {want[1]!r})"
        return want

    def init(self, *keys):
        for hid, key in enumerate(keys):
            assert self.do("init_raw", "raw", key, *D.CONFIGS[key]) == (True, None)
            self.do("open", "handle", key, hid)

    def check(self, *keys):
        for key in keys:
            for kind in ("export", "ttl", "exists", "count"):
                self.do(kind, "obj", key)
            self.do("contains", "obj", key, D.PROBE, True, None, ())


@pytest.fixture
def pair(client, fresh):
    p = Pair(client, fresh + ":")
    yield p
    p.engine.shutdown()


def keys(lo, hi, pool="v"):
    return (pool, tuple(range(lo, hi)))


def test_one_handle_list_reads_writes_and_reads_with_a_tenant_missing_at_first(pair):
    """contains_multi (the missing string is served from zeros and stays missing), add_multi on the same handles (the
    create flag flips: the table is built again and the string comes into being), contains_multi again."""
    pair.init(D.SMALL, D.MISSING, D.REGION)
    pair.do("add", "obj", D.SMALL, keys(0, 300), True, None, ())
    for via in D.VIAS["add_multi"]:
        segs = tuple((h, keys(100, 400)) for h in (0, 1, 2))
        pair.do("contains_multi", via, D.SMALL, segs, True)
        assert pair.do("ttl", "obj", D.MISSING) == ("missing", None)
        assert pair.do("add_multi", via, D.SMALL, segs, True)[0][0][1] >= 290  # into the empty 3,001-bit filter
        assert pair.do("contains_multi", via, D.SMALL, segs, True)[0][0] == [300, 300, 300]
        pair.check(D.SMALL, D.MISSING, D.REGION)
        pair.do("delete", "obj", D.MISSING)
        pair.do("init_raw", "raw", D.MISSING, *D.CONFIGS[D.MISSING])


def test_a_tenant_deleted_and_re_created_between_two_add_multis_of_one_handle_list(pair):
    pair.init(D.SMALL, D.REINIT)
    for via in D.VIAS["add_multi"]:
        segs = ((0, keys(0, 257)), (1, keys(0, 257)))
        pair.do("add_multi", via, D.SMALL, segs, True)
        pair.do("delete", "obj", D.REINIT)
        assert pair.do("init_raw", "raw", D.REINIT, *D.CONFIGS[D.REINIT]) == (True, None)
        counts, flags = pair.do("add_multi", via, D.SMALL, segs, True)[0]
        assert counts[0] == 0 and counts[1] > 200  # the first tenant holds them all, the second starts empty again
        pair.check(D.SMALL, D.REINIT)
        pair.do("delete", "obj", D.REINIT)
        pair.do("init_raw", "raw", D.REINIT, *D.CONFIGS[D.REINIT])


def test_a_new_handle_in_the_place_of_a_closed_one(pair):
    """same list length, same keyspace generation, most likely the same address: only the serial tells the table
    that slot 0 is another filter now"""
    pair.init(D.REGION)
    for key in (D.SMALL, D.K17):
        pair.do("init_raw", "raw", key, *D.CONFIGS[key])
        pair.do("add", "obj", key, keys(0, 2, "s16"), True, None, ())  # both strings exist: opening creates nothing
    pair.do("add", "obj", D.SMALL, keys(0, 300, "s16"), True, None, ())
    for via in D.VIAS["contains_multi"]:
        pair.do("open", "handle", D.SMALL, 100)
        assert pair.do("contains_multi", via, D.SMALL, ((100, keys(0, 300, "s16")), (0, keys(0, 300, "s16"))), True)[0][0][0] == 300
        pair.do("close", "handle", D.SMALL, 100)
        pair.do("open", "handle", D.K17, 101)
        assert pair.do("contains_multi", via, D.K17, ((101, keys(0, 300, "s16")), (0, keys(0, 300, "s16"))), True)[0][0][0] == 2
        pair.do("close", "handle", D.K17, 101)


def add_forms(key, hid, spec):
    n = len(spec[1])
    return {"obj": ("add", "obj", key, spec, False, None, ()), "obj flags": ("add", "obj", key, spec, True, None, ()),
            "raw": ("add", "raw", key, spec, True, D.CONFIGS[key], ()),
            "async": ("add", "async", key, spec, True, None, (("contains", key, spec, True, None),)),
            "handle": ("add_dev", "handle", key, hid, spec, True, "odd offsets"),
            "handle stream2": ("add_dev", "handle", key, hid, spec, True, "stream2"),
            "multi": ("add_multi", "multi", key, ((hid, spec),), True),
            "multi_dev": ("add_multi", "multi_dev", key, ((hid, spec),), True),
            "multi repeated": ("add_multi", "multi", key, ((hid, spec), (hid, spec)), True),
            "stream": ("stream", "stream", key, (hid,), (0,) * n, (1,) * n, spec),
            "stream_dev": ("stream", "stream_dev", key, (hid,), (0,) * n, (1,) * n, spec)}


@pytest.mark.parametrize("knobs", [{}, dict(add_partition=1, add_one_key=0), dict(add_one_key=0, add_single_seg_keys=0),
                                   dict(add_multi_table8=0), dict(add_multi_segment=0), dict(stream_table8=0)],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_the_string_length_comes_from_each_add_path_alone(pair, knobs):
    """One key whose highest index is the filter's last bit, added alone to the EMPTY 65,537-bit filter on each add
    path in turn: the 8,193 bytes of the string are that path's doing.  Then 300 keys behind it, on the same path."""
    assert LAST_KEY is not None, "no candidate key has an index on the filter's last bit"
    one = ("lit", (LAST_KEY,))
    pair.init(D.REGION)
    with tuned(knobs):
        for name in add_forms(D.REGION, 0, one):
            for spec in (one, ("lit", tuple(M.VAR[:300]) + one[1])):
                pair.do(*add_forms(D.REGION, 0, spec)[name])
                assert len(pair.do("export", "obj", D.REGION)[0]) == (LAST_SIZE + 7) // 8, name
                pair.do("contains_dev", "handle", D.REGION, 0, spec, True, "offsets")
                pair.do("delete", "obj", D.REGION)
                pair.do("init_raw", "raw", D.REGION, *D.CONFIGS[D.REGION])


def test_a_refused_multi_call_leaves_no_empty_string_behind(pair):
    """add_multi and the stream bind every filter for writing before any kernel runs.  When a later handle of the
    list is refused -- its config has changed, its name holds another type, its k is past the stream's 32 -- the
    strings created for the handles before it must go again: PTTL says the key is missing, as the model does, and
    a renamenx from it finds no such key.  Nor does the host stream create the string of a filter it only reads."""
    pair.init(D.MISSING, D.REINIT, D.K40)
    pair.do("init_raw", "raw", D.HLL, *D.CONFIGS[D.HLL])
    pair.do("open", "handle", D.HLL, D.HLL_HANDLE)
    pair.do("hll_init", "obj", D.HLL)
    pair.do("delete", "obj", D.REINIT)
    pair.do("init_raw", "raw", D.REINIT, *D.OTHER_CONFIG)
    n = 5
    for via, bad, kind in (("multi", 1, M.CONFIG), ("multi_dev", 1, M.CONFIG), ("multi", D.HLL_HANDLE, M.WRONGTYPE),
                           ("multi_dev", D.HLL_HANDLE, M.WRONGTYPE)):
        assert pair.do("add_multi", via, D.MISSING, ((0, keys(0, n)), (bad, keys(0, n))), True) == (None, kind)
        assert pair.do("ttl", "obj", D.MISSING) == ("missing", None)
    for via in D.VIAS["stream"]:
        for bad, kind in ((2, M.ILLEGAL), (1, M.CONFIG)):
            assert pair.do("stream", via, D.MISSING, (0, bad), (0,) * n, (1,) * n, keys(0, n)) == (None, kind)
            assert pair.do("ttl", "obj", D.MISSING) == ("missing", None)
    pair.do("init_raw", "raw", D.SMALL, *D.CONFIGS[D.SMALL])
    pair.do("open", "handle", D.SMALL, 3)
    # the host stream binds for writing only the filters an add names: reads alone, then an add on the other filter
    # (the table of the first call stands on zeros for both and must not serve the second), then one on this filter
    for ops, after in (((0,) * n, "missing"), ((0, 0, 1, 0, 0), "missing"), ((0, 1, 0, 0, 0), "none")):
        if after == "none":
            assert pair.do("renamenx", "obj", D.MISSING, D.SPARE) == (None, M.NO_SUCH_KEY)
        pair.do("stream", "stream", D.SMALL, (3, 0), (0, 1, 0, 1, 1), ops, keys(0, n))
        assert pair.do("ttl", "obj", D.MISSING) == (after, None)
    pair.check(D.SMALL, D.MISSING)
    pair.do("delete", "obj", D.MISSING)
    pair.do("init_raw", "raw", D.MISSING, *D.CONFIGS[D.MISSING])
    assert pair.do("add_multi", "multi", D.MISSING, ((0, keys(0, n)),), True)[0][0] == [n]  # and the handle still works
    pair.check(D.MISSING)
