"""HyperLogLog command sequences on the GPU against the keyspace model (hll_driver.py, hll_model.py), and targeted
multi-key PFADDs of crafted elements (hll_elements.py) at the places where the sparse replay's kernels index.

The sequences: PFADD / PFCOUNT / PFMERGE / SET / GET / DEL / copy / pack / unpack_max through the name-based, multi-key,
handle, async and Spring Data paths take turns on seven shared keys, and every reply, error and -- every 10
commands -- every key's stored bytes, header included, equal the model.  Nothing here takes header bytes 8..15 from
the engine: the model predicts them.  What they are there to check is the host state of api_hll.cpp (the lazily
learnt promotion word, the dense flag, recycled slots, the separate list of long SET strings, the cached tables,
the host tiers, the handles' re-binding, the cached cardinality).

A failure names its seed and step; hll_driver.run(engine, seed, STEPS, stop_at=step + 1) replays it."""
import contextlib

import numpy as np
import pytest

import hll_driver as D
import hll_elements as E
import hll_model as M
from oracle import oracle as O
from redisson_amd import _lib as L
from test_hll_sequences_cpu import SEEDS, STEPS

pytestmark = pytest.mark.gpu

DEFAULTS = {"host_small_batches": 1, "host_tiny_keys": 16384, "host_tiny_spin": 1, "host_small_bytes": 4 << 20}
# The knobs each seed runs under; a knob that is not named keeps its default.  host_small_batches = 0 sends every call
# down the pipelined path (both staging tiers off); host_tiny_keys = 0 sends the tiny tier's calls to the small tier;
# host_small_bytes = 65536 sends the 4,097-element PFADDs (65,552 bytes) and everything larger down the pipelined path.
SETTINGS = {
    0: {},
    1: dict(host_small_batches=0),
    2: dict(host_tiny_keys=0),
    3: dict(host_tiny_spin=0),
    4: dict(host_small_bytes=65536),
    5: dict(host_tiny_keys=0, host_small_bytes=65536),
    6: dict(host_tiny_spin=0, host_small_bytes=65536),
    7: dict(host_tiny_keys=0, host_tiny_spin=0),
}


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

    assert set(SETTINGS) == set(SEEDS)
    assert seen("host_small_batches") == {0, 1}
    assert seen("host_tiny_keys") == {0, 16384}
    assert seen("host_tiny_spin") == {0, 1}
    assert seen("host_small_bytes") == {65536, DEFAULTS["host_small_bytes"]}
    assert any(SETTINGS[s] == {} for s in SEEDS)  # one seed at all defaults


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_equals_the_model(client, fresh, seed):
    engine = D.GpuEngine(client, fresh + ":")
    try:
        with tuned(SETTINGS[seed]):
            D.run(engine, seed, STEPS)
    finally:
        engine.close()


# ---- targeted: crafted elements in one or two multi-key PFADDs ------------------------------------------------------
class Pair:
    """the same commands to the engine and to the model, replies compared (keys live under the test's prefix)"""

    def __init__(self, client, prefix):
        self.engine, self.model, self.names = D.GpuEngine(client, prefix), M.Keyspace(), set()

    def do(self, *cmd):
        got, want = D.call(self.engine, cmd), D.call(self.model, cmd)
        assert got == want, f"{D.short(cmd)!r}: engine / model: {D.first_difference(got[0], want[0])} ({got[1]!r} / {want[1]!r})"
        return want[0]

    def pfadd_multi(self, cmds):
        """cmds: [(key, [element, ...]), ...] in one rbx_hll_add_multi call"""
        self.names |= {k for k, _ in cmds}
        return self.do("pfadd_multi", "names", cmds[0][0], tuple((k, ("lit", tuple(els))) for k, els in cmds))

    def close(self):
        for k in self.names:
            self.engine._hll(k).delete()


@pytest.fixture
def pair(client, fresh):
    p = Pair(client, fresh + ":")
    yield p
    p.close()


def low_elements(rng, registers, length=16):
    return [E.element(int(r), int(rng.integers(1, 4)), length, rng) for r in registers]


def test_promotion_by_value_inside_a_pfadd(pair):
    """Counts a search by brute force never finds (33: probability 2^-32), through the PFADD kernels: a command whose
    first, a middle or the last element has count 33 promotes; count 32 alone is the largest VAL and stays sparse;
    counts 50 and 51 promote, and 51 sends PFCOUNT to the host's hllTau.  On fresh keys and on keys that hold 300
    random elements.  Replies, the stored bytes with their header, PFCOUNT, and the registers of the elements behind
    the promoting one."""
    rng = np.random.default_rng(0x33)
    cases = {"first": (0, 33), "middle": (4, 33), "last": (8, 33), "val32": (None, 32), "tau50": (3, 50), "tau51": (5, 51)}
    keys = [(start, case) for start in ("fresh", "held") for case in cases]
    held = [(f"{start}-{case}", list(rng.integers(0, 256, size=(300, 16), dtype=np.uint8)))
            for start, case in keys if start == "held"]
    pair.pfadd_multi([(k, [bytes(r) for r in rows]) for k, rows in held])
    cmds, after = [], {}
    for start, case in keys:
        at, count = cases[case]
        registers = rng.choice(np.arange(2000, 2400), size=9, replace=False)  # distinct, clustered: runs form
        els = low_elements(rng, registers)
        if at is None:
            els = [E.element(int(registers[0]), count, 16, rng)]
        else:
            els[at] = E.element(int(registers[at]), count, 16, rng)
            after[f"{start}-{case}"] = [O.hll_patlen(e) for e in els[at + 1:]]
        cmds.append((f"{start}-{case}", els))
    assert pair.pfadd_multi(cmds) == [1] * len(cmds)
    for key, _ in cmds:
        stored = pair.do("get", "obj", key, "stored")
        assert stored[4] == (1 if key.endswith("val32") else 0), key  # promoted, or the largest VAL
        assert stored[8:16] == M.INVALID.to_bytes(8, "little")
        regs = pair.model.registers(key)
        assert all(regs[i] >= c for i, c in after.get(key, [])), key  # the elements behind the promoting one
        assert pair.do("get", "obj", key, "dense")[16:] == O.hll_dense_pack(regs)
        assert pair.do("pfcount", "obj", key) == O.hll_count(regs)
        assert pair.do("get", "obj", key, "stored")[8:16] == O.hll_count(regs).to_bytes(8, "little")  # stored, valid


def test_sparse_strings_longer_than_the_dense_one(pair):
    """A sparse string can be longer than the 12,304 bytes of the dense one: the fewest-bytes form of a dense key
    whose neighbours all differ (16,384 VAL opcodes), and a SET string of 8,001 two-byte XZEROs.  GET returns them
    whole (RHyperLogLog.exportString once cut them at the dense length), and the long SET string goes on replaying
    in its own opcode list."""
    rng = np.random.default_rng(0x10)
    regs = (1 + np.arange(M.REGS) % 2).astype(np.uint8)
    pair.names |= {"alternating", "xzeros"}
    pair.do("set", "obj", "alternating", M.header(0, 9) + O.hll_dense_pack(regs))
    assert pair.do("get", "obj", "alternating", "sparse") == M.header(1, 9) + O.hll_sparse_pack(regs)
    assert len(O.hll_sparse_pack(regs)) == M.REGS
    rest = M.REGS - 8000
    ops = bytes([0x40, 0x00]) * 8000 + bytes([0x40 | ((rest - 1) >> 8), (rest - 1) & 0xFF])
    pair.do("set", "obj", "xzeros", M.header(1, M.INVALID) + ops)
    assert len(pair.do("get", "obj", "xzeros", "stored")) == 16 + 16002
    assert pair.pfadd_multi([("xzeros", low_elements(rng, [3, 4, 5, 7999, 8000, 9000]))]) == [1]  # shrinks, then grows
    pair.do("get", "obj", "xzeros", "stored")
    assert pair.do("pfcount", "obj", "xzeros") == O.hll_count(pair.model.registers("xzeros"))


def test_many_commands_in_one_tiny_call(pair):
    """1,700 commands of two 8-byte elements in one call of the tiny tier (3,400 elements, 27 KiB): the first round's
    1,500 tiles fit the call's 64 KiB table block and its 1,500 replay items do not (they go through the cached
    device table, beside elements and changed words in host memory); 200 keys are named again, a second round whose
    tables fit behind the first's.  Every fourth of those repeats its elements: reply 0."""
    rng = np.random.default_rng(0x7)
    first = [(f"k{i}", low_elements(rng, rng.integers(0, M.REGS, size=2), 8)) for i in range(1500)]
    again = [(k, els if i % 4 == 0 else [els[0]] + low_elements(rng, rng.integers(0, M.REGS, size=1), 8))
             for i, (k, els) in enumerate(first[:200])]
    replies = pair.pfadd_multi(first + again)
    assert replies[:1500] == [1] * 1500 and replies[1500::4] == [0] * 50 and sum(replies[1500:]) >= 100
    for k, _ in first:
        pair.do("get", "obj", k, "stored")


def test_a_multi_key_pfadd_naming_another_type_changes_nothing(pair):
    """rbx_hll_add_multi has one return code: a key of another type anywhere in the call is WRONGTYPE, and neither
    the missing key named before it is created (it once was left behind, empty) nor the existing key updated."""
    rng = np.random.default_rng(0xB1)
    pair.do("other_types", "obj", M.BITS)
    pair.pfadd_multi([("there", low_elements(rng, [1, 2, 3]))])
    before = pair.do("get", "obj", "there", "stored")
    cmds = (("missing", ("lit", tuple(low_elements(rng, [9])))), ("there", ("lit", tuple(low_elements(rng, [77])))),
            (M.BITS, ("lit", tuple(low_elements(rng, [5])))), ("after", ("lit", tuple(low_elements(rng, [6])))))
    assert D.call(pair.engine, ("pfadd_multi", "names", "missing", cmds)) == (None, M.WRONGTYPE)
    assert pair.do("pfadd_multi", "names", "missing", cmds) is None
    for key in ("missing", "after"):
        assert pair.do("exists", "obj", key) is False
    assert pair.do("get", "obj", "there", "stored") == before
    pair.engine.bits.delete(), pair.engine.bloom.delete()


def boundary_cases():
    """name -> {register: value}: runs of four and five at the chunk boundaries of the scan (thread t takes registers
    [64t, 64t + 64)) and at both ends; zero runs of exactly 64 and 65 (ZERO / XZERO) inside a chunk and across one;
    zero runs over whole chunks, whose threads have no run start of their own in the suffix minimum"""
    cases = {}
    for name, (lo, hi) in {"60..63": (60, 63), "61..64": (61, 64), "62..66": (62, 66), "0..3": (0, 3),
                           "16380..16383": (16380, 16383), "16379..16383": (16379, 16383)}.items():
        for v in (1, 2):
            cases[f"run {name} of {v}"] = {r: v for r in range(lo, hi + 1)}
        cases[f"run {name} mixed"] = {r: 1 + (r == hi) for r in range(lo, hi + 1)}
    for at in (10, 63, 64, 100, 127, 16383 - 66):
        for gap in (64, 65):
            cases[f"{gap} zeros after {at}"] = {at: 1, at + gap + 1: 2}
    cases["three empty chunks"] = {70: 1, 71: 1, 330: 3}
    cases["empty chunks to the end"] = {5: 2, 6: 2, 7: 1}
    cases["empty chunks from the start"] = {16000: 1, 16383: 2}
    cases["first and last"] = {0: 1, 16383: 1}
    return cases


def test_runs_and_zero_runs_at_chunk_boundaries(pair):
    rng = np.random.default_rng(0x64)
    cases = boundary_cases()
    cmds = []
    for name, regs in cases.items():
        els = [E.element(r, v, int(rng.choice(M.LENGTHS)), rng) for r, v in regs.items()]
        cmds.append((name, [els[int(i)] for i in rng.permutation(len(els))]))
    assert pair.pfadd_multi(cmds) == [1] * len(cmds)
    shortcut = sum(ev == ("shortcut",) for ev in pair.model.events)
    assert shortcut >= 20 and len(cases) - shortcut >= 4  # runs of five take the element-by-element replay
    for name, regs in cases.items():
        stored = pair.do("get", "obj", name, "stored")  # the model: RedisHll, element by element
        want = O.hll_new()
        want[list(regs)] = list(regs.values())
        assert np.array_equal(pair.model.registers(name), want)
        if max(len(run) for run in runs_of(want)) <= 4:  # the shortcut took it: the normalized string
            assert stored == M.header(1, M.INVALID) + O.hll_sparse_pack(want), name


def runs_of(regs):
    """the nonzero runs of equal registers, as index arrays"""
    nz = np.flatnonzero(regs)
    cuts = np.flatnonzero((np.diff(nz) != 1) | (np.diff(regs[nz].astype(np.int16)) != 0)) + 1
    return np.split(nz, cuts)


def test_the_oracles_shortcut_windows_through_the_kernel(pair):
    """test_oracle.py::test_sparse_normalized_shortcut's generator (its window widths, its bases -- with multiples of
    64 minus 2 added -- and its maxv values), about 400 cases, one key each: SET builds the base string
    (hll_sparse_pack of the base registers), one multi-key PFADD carries every case's update list, in its random
    order, as crafted elements.  The cases the CPU test skips stay in: they take the element-by-element replay."""
    rng = np.random.default_rng(1000)
    cases = []
    while len(cases) < 400:
        W = int(rng.choice([int(rng.integers(2, 13)), int(rng.integers(2, 13)), 40, 400, 16384]))
        base = int(rng.choice([0, 16384 - W, int(rng.integers(0, 16384 - W + 1)),
                               min(64 * int(rng.integers(1, 256)) - 2, 16384 - W)]))
        maxv = int(rng.choice([1, 2, 3, 32]))
        regs = np.zeros(16384, np.uint8)
        nv = int(rng.integers(0, W))
        if nv and rng.random() < 0.7:
            regs[rng.integers(base, base + W, size=nv)] = rng.integers(1, maxv + 1, size=nv)
        nu = int(rng.integers(1, 2 * min(W, 400) + 4))
        ur, uc = rng.integers(base, base + W, size=nu), rng.integers(1, maxv + 1, size=nu)
        if W == 16384 and len(cases) % 4:  # most of the widest windows: fewer updates (the elements are made in Python)
            ur, uc = ur[:40], uc[:40]
        cases.append((regs, ur, uc))
    cmds = []
    for i, (regs, ur, uc) in enumerate(cases):
        pair.do("set", "obj", f"w{i}", M.header(1, M.INVALID | 5) + O.hll_sparse_pack(regs))
        cmds.append((f"w{i}", [E.element(int(r), int(c), 16, rng) for r, c in zip(ur, uc)]))
    pair.pfadd_multi(cmds)
    shortcut = sum(ev == ("shortcut",) for ev in pair.model.events)
    replay = sum(ev == ("replay",) for ev in pair.model.events)
    assert shortcut >= 100 and replay >= 50
    for i in range(len(cases)):
        pair.do("get", "obj", f"w{i}", "stored")
