"""Random, seeded, model-checked HyperLogLog command sequences over a few shared keys (the shape of
bitstring_driver.py).

commands(seed, steps) yields plain tuples (kind, via, key, *args); run(engine, seed, steps) sends each to an engine
adapter and to the keyspace model of hll_model.py, compares reply and error kind, and every `check_every` commands
reads every key back: the stored GET bytes -- header included, predicted by the model, never taken from the engine --
EXISTS, the PTTL sign, and `PFCOUNT key <missing key>`, which takes the several-keys path, writes no header and
must equal hll_count of the model's registers.  Engines: GpuEngine (librbx.so through RHyperLogLog and its *Async
forms, hll_add_multi, hll_count_each, RedissonConnection.pfAdd / pfCount / pfMerge inside and outside a pipeline, and
one rbx_hll handle per key kept open for the whole sequence), ModelEngine (a second Keyspace) and FaultyModelEngine
(the model with one injected defect).

What the sequences are there to check is the host state behind the kernels (api_hll.cpp): the promotion word the
host learns lazily, the dense flag PFMERGE sets on its own, recycled pool slots, the separate opcode list of long SET
strings, the tile and replay tables cached by content, the three host tiers, handles that re-bind by keyspace
generation, and the cached cardinality of the header.

To replay a failure: run(engine, seed, steps, stop_at=step + 1); list(commands(seed, steps))[step] is the command."""
import ctypes as C

import numpy as np

import hll_elements as E
import hll_model as M
from hll_model import BITS, BLOOM, ILLEGAL, INVALID, NO_SUCH_KEY, REDIS, WRONGTYPE, Keyspace
from oracle import oracle as O

SMALL, CROSS, DENSE, ODD, LONG, DEST, GONE = "s", "x", "d", "n", "l", "m", "z"
HLLS = (SMALL, CROSS, DENSE, ODD, LONG, DEST, GONE)
ABSENT = "never"  # no command ever creates it: the second key of the full check's PFCOUNT
TTL_MS = 3_600_000
SIZES = (0, 1, 2, 255, 256, 257, 1000, 4097)  # 4097 x 16 bytes: past the tiny tier's 64 KiB

FAMILY = {}
for _family, _kinds in {"add": "pfadd pfadd_multi pfadd_dev", "count": "pfcount pfcount_multi count_each",
                        "merge": "pfmerge", "string": "set get", "key": "delete exists expire persist ttl",
                        "copy": "copy", "image": "pack unpack_max", "setup": "open other_types"}.items():
    for _k in _kinds.split():
        FAMILY[_k] = _family

VIAS = {"pfadd": ("obj", "async", "conn", "pipe"), "pfadd_multi": ("names",), "pfadd_dev": ("handle",),
        "pfcount": ("obj", "async", "conn", "pipe"), "pfcount_multi": ("obj", "async", "conn"),
        "count_each": ("names", "handle"), "pfmerge": ("obj", "async", "conn", "pipe"), "set": ("obj",),
        "get": ("obj",), "delete": ("obj",), "exists": ("obj",), "expire": ("obj",), "persist": ("obj",),
        "ttl": ("obj",), "copy": ("ctx",), "pack": ("handle",), "unpack_max": ("handle",)}
WEIGHTS = {"pfadd": 16, "pfadd_multi": 5, "pfadd_dev": 4, "pfcount": 9, "pfcount_multi": 4, "count_each": 4,
           "pfmerge": 7, "set": 4, "get": 4, "delete": 1.5, "exists": 1, "expire": 1.5, "persist": 1.5, "ttl": 1.5,
           "copy": 2.5, "pack": 1.5, "unpack_max": 3}
WRONGTYPE_OK = {"pfadd", "pfcount", "pfcount_multi", "count_each", "pfmerge", "get", "copy"}


def label(cmd) -> str:
    return f"{cmd[0]}:{cmd[1]}"


# ---- the scripted strings ---------------------------------------------------------------------------------------
def dense_string(seed) -> bytes:
    """a dense SET string, registers up to 63, with a valid cached cardinality that is wrong for them"""
    rng = np.random.default_rng([0xDE5E, seed])
    regs = rng.integers(0, 12, size=M.REGS, dtype=np.uint8)
    regs[rng.integers(0, M.REGS, size=40)] = rng.integers(33, 64, size=40)
    return M.header(0, 1234 + seed) + O.hll_dense_pack(regs)


def odd_string(seed) -> bytes:
    """a sparse SET string that is not normalized: adjacent VALs of one value, a split zero run, an XZERO a ZERO could
    hold; its cached cardinality is valid and wrong"""
    rng = np.random.default_rng([0x0DD, seed])
    ops = bytes([0x84, 0x84, 0x80, 0x05, 0x02, 0x40, 0x09])  # VAL(2,1) VAL(2,1) VAL(1,1) ZERO(6) ZERO(3) XZERO(10)
    at = 1 + 1 + 1 + 6 + 3 + 10
    for _ in range(int(rng.integers(3, 30))):
        v, n = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        ops += bytes([0x80 | ((v - 1) << 2) | (n - 1), int(rng.integers(0, 40))])
        at += n + ops[-1] + 1
    rest = M.REGS - at
    return M.header(1, 77) + ops + bytes([0x40 | ((rest - 1) >> 8), (rest - 1) & 0xFF])


def long_string(seed) -> bytes:
    """a sparse SET string of more than 3,072 opcodes (past a pool slot's list, and past hll-sparse-max-bytes)"""
    n = 1600 + 10 * seed
    ops = bytes([0x80 | ((1 + seed % 3) << 2), 0x00]) * n  # VAL(v, 1) ZERO(1), n times
    rest = M.REGS - 2 * n
    return M.header(1, INVALID) + ops + bytes([0x40 | ((rest - 1) >> 8), (rest - 1) & 0xFF])


INVALID_STRINGS = (b"HYLX" + bytes(12300), M.header(1, 0) + bytes([0x7F, 0xFE]))  # bad magic; covers 16383 registers


# ---- the generator ----------------------------------------------------------------------------------------------
def commands(seed: int, steps: int):
    """`steps` command tuples, a pure function of the seed.  It steps a model of its own to know the keys' state."""
    rng = np.random.default_rng([0x4771, seed])
    ks = Keyspace()
    state = {"prev": None, "serial": 0}
    added = {k: [] for k in HLLS}  # the element specs a key took since it was last created or replaced
    pending = []

    def integer(lo, hi):
        return int(rng.integers(lo, hi, endpoint=True))

    def choice(seq):
        return seq[int(rng.integers(len(seq)))]

    def serial():
        state["serial"] += 1
        return 1000 * seed + state["serial"]

    def pick_key(kind, pool=HLLS):
        if kind in WRONGTYPE_OK and rng.random() < 0.07:
            return choice((BITS, BLOOM))
        if state["prev"] in pool and rng.random() < 0.5:
            return state["prev"]
        return choice(pool)

    def spec_for(key, sizes=SIZES):
        """an element spec for a PFADD on key"""
        if key == SMALL:  # stays small and sparse
            return choice((("low", serial(), integer(1, 4)), ("rows", serial(), integer(0, 2)),
                           ("var", serial(), integer(1, 2)), ("none",)))
        if key in (ODD, LONG) and rng.random() < 0.7:  # mostly small updates: the SET string lives a while
            return choice((("low", serial(), integer(1, 6)), ("crafted", serial(), integer(1, 6)),
                           ("rows", serial(), integer(0, 2))))
        r = rng.random()
        n = choice(sizes)
        if r < 0.45:
            return ("rows", serial(), n)
        if r < 0.6:
            return ("var", serial(), max(n, 1))
        if r < 0.8:
            return ("crafted", serial(), integer(1, 40))
        return ("low", serial(), integer(1, 40))

    def repeat_for(key):
        return choice(added[key]) if added.get(key) else None

    def add_spec(key):
        if key in added and rng.random() < 0.22:
            old = repeat_for(key)
            if old is not None:
                return old, True
        return spec_for(key) if key in added else ("rows", serial(), 2), False

    def set_string(key):
        r = rng.random()
        src = choice(HLLS)
        if r < 0.25 and key in ks.keys:
            return ks.get("obj", key, "stored")[0]  # its own earlier GET
        if r < 0.5 and src in ks.keys:
            return ks.get("obj", src, choice(("stored", "dense")))[0]  # another key's GET
        if r < 0.62:
            return choice(INVALID_STRINGS)
        return choice((dense_string, odd_string, long_string))(serial() % 7)

    def build(kind):
        via = choice(VIAS[kind])
        key = pick_key(kind)
        if kind == "pfadd":
            spec, again = add_spec(key)
            if again and rng.random() < 0.7:  # a count first: the repeat then meets a valid cache
                pending.append((kind, via, key, spec))
                return ("pfcount", choice(VIAS["pfcount"]), key)
            return (kind, via, key, spec)
        if kind == "pfadd_multi":
            n = integer(2, 9)
            keys = [pick_key(kind, HLLS[1:]) for _ in range(n)]
            if rng.random() < 0.55:  # successive rounds: a key named again
                i, j = rng.choice(n, size=2, replace=False)
                keys[int(j)] = keys[int(i)]
            if rng.random() < 0.1:  # a key of another type behind a missing one: an error, and nothing is created
                keys[:2] = [GONE, choice((BITS, BLOOM))]
            cmds = []
            for k in keys:
                old = repeat_for(k) if rng.random() < 0.15 else None
                cmds.append((k, old if old is not None else spec_for(k, (0, 1, 2, 255, 256, 257, 1000))))
            first = {}
            for at, (k, spec) in enumerate(cmds):  # a key named again: sometimes with the elements of its first command,
                if k in first and rng.random() < 0.4:  # which change nothing by then -- its reply sees that command
                    cmds[at] = (k, cmds[first[k]][1])
                first.setdefault(k, at)
            return (kind, via, keys[0], tuple(cmds))
        if kind == "pfadd_dev":
            key = pick_key(kind, HLLS[1:])
            return (kind, via, key, choice((("rows", serial(), choice((0, 1, 257, 1000))),
                                            ("crafted", serial(), integer(1, 30)), ("var", serial(), integer(1, 300)))))
        if kind == "pfcount":
            return (kind, via, key)
        if kind == "pfcount_multi":
            return (kind, via, key, tuple(pick_key(kind) for _ in range(integer(1, 4))))
        if kind == "count_each":
            pool = HLLS if via == "handle" else HLLS + (BITS,) * (rng.random() < 0.1)
            keys = tuple(choice(pool) for _ in range(integer(1, 6)))
            return (kind, via, keys[0], keys)
        if kind == "pfmerge":
            if key == SMALL:
                key = DEST
            r = rng.random()
            if r < 0.2:
                srcs = (GONE,) if GONE not in ks.keys else (ABSENT,)  # only missing sources
            elif r < 0.4:
                srcs = (key, pick_key(kind))  # dest among the sources
            elif r < 0.55:
                s = pick_key(kind)
                srcs = (s, choice(HLLS), s)  # a source named twice
            else:
                srcs = tuple(pick_key(kind) for _ in range(integer(1, 3)))
            if key in (BITS, BLOOM):
                via = choice(("obj", "conn"))
            return (kind, via, key, srcs)
        if kind == "set":
            key = pick_key(kind, HLLS[1:])
            return (kind, via, key, set_string(key))
        if kind == "get":
            return (kind, via, key, choice(("stored", "dense", "sparse")))
        if kind == "delete":
            key = pick_key(kind, HLLS[1:])
            if key != GONE:  # the other keys come back at once: a re-created key on a recycled slot
                pending.append(("pfadd", choice(VIAS["pfadd"]), key, ("rows", serial(), choice((1, 2, 300)))))
            return (kind, via, key)
        if kind in ("exists", "expire", "persist", "ttl"):
            return (kind, via, pick_key(kind, HLLS))
        if kind == "copy":
            dst = pick_key("", HLLS[1:])
            src = pick_key(kind, HLLS + (GONE,))
            if rng.random() < 0.3 and dst in ks.keys and dst != src:
                pending.append((kind, via, src, dst))
                return ("expire", "obj", dst)  # the copy has a TTL to clear
            return (kind, via, src, dst)
        if kind == "pack":
            return (kind, via, pick_key(kind, HLLS))
        if kind == "unpack_max":
            key = pick_key(kind, HLLS[1:])
            r = rng.random()
            return (kind, via, key, ("few" if r < 0.75 else "value" if r < 0.9 else "bytes", serial()))
        raise AssertionError(kind)

    def step(cmd):
        kind, key = cmd[0], cmd[2]
        if kind in ("pfadd", "pfadd_dev") and key in added:
            added[key].append(cmd[3])
        elif kind == "pfadd_multi" and not any(k in (BITS, BLOOM) for k, _ in cmd[3]):
            for k, spec in cmd[3]:
                added[k].append(spec)
        elif kind in ("delete", "set") and key in added:
            added[key] = []
        elif kind == "copy" and cmd[3] in added:
            added[cmd[3]] = []
        getattr(ks, kind)(*cmd[1:])
        state["prev"] = key
        return cmd

    def recreate(key, n):
        return [("delete", "obj", key), ("pfadd", "obj", key, ("rows", serial(), n))]

    kinds = list(WEIGHTS)
    p = np.array([WEIGHTS[k] for k in kinds], float)
    p /= p.sum()
    script = {0: [("other_types", "obj", BITS), ("set", "obj", DENSE, dense_string(seed)),
                  ("set", "obj", ODD, odd_string(seed)), ("set", "obj", LONG, long_string(seed)),
                  ("pfadd", "obj", SMALL, ("low", serial(), 3)), ("pfadd", "conn", CROSS, ("rows", serial(), 300)),
                  ("pfadd", "obj", DEST, ("rows", serial(), 5)), ("pfadd", "obj", GONE, ("rows", serial(), 1))]
              + [("open", "handle", k) for k in HLLS]
              + [("delete", "obj", GONE), ("pfcount", "obj", DENSE), ("pfcount", "conn", ODD)]}
    for i, at in enumerate(range(30, steps, 70)):  # the key that crosses the limit, is deleted and comes back
        script[at] = [("pfadd", choice(VIAS["pfadd"]), CROSS, ("rows", serial(), 1000))]
        script[at + 8] = [("pfadd", choice(VIAS["pfadd"]), CROSS, ("rows", serial(), 1000))]
        script[at + 30] = recreate(CROSS, 200) + [("pfadd_multi", "names", CROSS, (
            (CROSS, ("rows", serial(), 900)), (DEST, ("low", serial(), 3)), (CROSS, ("rows", serial(), 900))))]
        script[at + 45] = recreate(CROSS, 100)
    script[20] = recreate(DEST, 40) + [("pfadd", "obj", DEST, ("at", serial(), ((7, 33, 16),)))]  # by value
    script[64] = [("pfadd", "obj", CROSS, ("rows", serial(), 70_000))]  # two tiles for one key
    script[95] = recreate(DEST, 3) + ["dense source"]  # (its SET string is built at its turn, from the model)
    script[135] = recreate(GONE, 1000) + recreate(DEST, 1000) + [("pfmerge", "obj", DEST, (GONE,)),
                                                                ("delete", "obj", GONE)]  # the write-back promotes
    script[165] = [("pfadd", "obj", CROSS, ("rows", serial(), 263_000))]  # past host_small_bytes (4 MiB)
    script[205] = recreate(DEST, 4) + [("unpack_max", "handle", DEST, ("value", serial()))]
    script[235] = recreate(ODD, 2)[:1] + [("set", "obj", ODD, odd_string(seed + 8)),
                                          ("pfmerge", "conn", ODD, (SMALL, DEST))]  # into a string that is not normalized
    for done in range(steps):
        pending += script.get(done, [])
        if pending and pending[0] == "dense source":  # a dense string of few registers makes a sparse dest dense
            pending[0:1] = [("set", "obj", GONE, ks.get("obj", SMALL, "dense")[0]),
                            ("pfmerge", "obj", DEST, (SMALL, GONE)), ("delete", "obj", GONE)]
        cmd = pending.pop(0) if pending else build(kinds[int(rng.choice(len(kinds), p=p))])
        yield step(cmd)


# ---- what a sequence covers (test_hll_sequences_cpu.py asserts on it) ----------------------------------------
def stats(seed: int, steps: int) -> dict:
    ks = Keyspace()
    out = {"kinds": {}, "after_other_family": set(), "errors": 0, "n": 0, "promoted": {}, "recreated": 0,
           "cache hits": 0, "recounts": 0, "wrong cache hits": 0, "unchanged on a valid cache": 0, "shortcut": 0,
           "replay": 0, "repeated key in multi": 0, "multi": 0}
    prev = None
    for cmd in commands(seed, steps):
        kind, key = cmd[0], cmd[2]
        ks.events = []
        _reply, err = getattr(ks, kind)(*cmd[1:])
        out["n"] += 1
        out["errors"] += err is not None
        out["kinds"][label(cmd)] = out["kinds"].get(label(cmd), 0) + 1
        if prev is not None and prev[2] == key and FAMILY[prev[0]] != FAMILY[kind]:
            out["after_other_family"].add(kind)
        if kind == "pfadd_multi":
            names = [k for k, _ in cmd[3]]
            out["multi"] += 1
            out["repeated key in multi"] += len(set(names)) < len(names)
        for ev in ks.events:
            if ev[0] == "promoted":
                out["promoted"][ev[1]] = out["promoted"].get(ev[1], 0) + 1
            elif ev[0] == "recreated":
                out["recreated"] += 1
            elif ev[0] == "cache hit":
                out["cache hits"] += kind == "pfcount"
                out["wrong cache hits"] += ev[1]
            elif ev[0] == "recount":
                out["recounts"] += kind == "pfcount"
            else:
                out[ev[0]] += 1
        prev = cmd
    return out


# ---- the full check -------------------------------------------------------------------------------------------
def probes(model: Keyspace):
    out = []
    for key in HLLS:
        out += [("get", "obj", key, "stored"), ("exists", "obj", key), ("ttl", "obj", key),
                ("pfcount_multi", "obj", key, (ABSENT,))]
    return out


def short(x, keep=6):
    if isinstance(x, (tuple, list)):
        if len(x) > 12 and all(isinstance(v, int) for v in x):
            return f"<{len(x)} ints: {', '.join(map(str, x[:keep]))}, ...>"
        return type(x)(short(v, keep) for v in x)
    if isinstance(x, bytes) and len(x) > 24:
        return f"<{len(x)} bytes: {x[:20].hex()}...>"
    return x


def first_difference(got, want):
    if isinstance(got, bytes) and isinstance(want, bytes):
        n = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        return f"lengths {len(got)} / {len(want)}, first difference at byte {n}: {got[n:n + 8].hex()} / {want[n:n + 8].hex()}"
    if isinstance(got, (list, tuple)) and isinstance(want, (list, tuple)) and len(got) == len(want):
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w:
                return f"element {i}: {first_difference(g, w)}"
    return f"{short(got)!r} / {short(want)!r}"


def call(engine, cmd):
    reply, err = getattr(engine, cmd[0])(*cmd[1:])
    if isinstance(reply, tuple):
        reply = list(reply)
    return reply, err


def run(engine, seed: int, steps: int, check_every: int = 10, stop_at=None) -> None:
    """The sequence of `seed` through `engine` and the model: every reply and error kind equal, and the full check
    every `check_every` commands and at the end.  stop_at = run only the first stop_at commands."""
    model = Keyspace()
    history = []

    def compare(cmd, step, what):
        want, got = call(model, cmd), call(engine, cmd)
        if got != want:
            last = "\n".join(f"  {i}: {short(c)!r}" for i, c in history[-20:])
            raise AssertionError(
                f"seed {seed}, step {step} ({what}): {short(cmd)!r}\n  engine / model error kind: {got[1]!r} / {want[1]!r}\n"
                f"  engine / model reply: {first_difference(got[0], want[0])}\nthe last commands:\n{last}")

    def full_check(step):
        for probe in probes(model):
            compare(probe, step, "full check after it")

    step = -1
    for step, cmd in enumerate(commands(seed, steps)):
        if stop_at is not None and step >= stop_at:
            step -= 1
            break
        history.append((step, cmd))
        compare(cmd, step, "command")
        if (step + 1) % check_every == 0:
            full_check(step)
    full_check(step)


# ---- engines ----------------------------------------------------------------------------------------------------
class ModelEngine(Keyspace):
    """a second model: the generator, the model and the checker agree with themselves"""

    def other_types(self, via, key):
        return None, None


Keyspace.other_types = ModelEngine.other_types  # setup: the engine creates its bit set and its Bloom filter


class FaultyModelEngine(ModelEngine):
    """The model with one wrong answer, `defect` in 'a' .. 'k' (test_hll_sequences_cpu.py lists them)."""

    def __init__(self, defect: str):
        super().__init__()
        assert defect in "abcdefghijk" and len(defect) == 1
        self.defect = defect
        self.left = {}   # (g) the opcode list a deleted key left in its slot
        self.bound = {}  # (j) the object a handle was first bound to

    def _store_count(self, k, value):
        if self.defect != "a":
            super()._store_count(k, value)

    def _invalidate(self, k, changed):
        super()._invalidate(k, changed or self.defect == "b")

    def _after_merge(self, k):
        if self.defect != "c":
            super()._after_merge(k)

    def _use_dense(self, d, sources):
        return d.dense if self.defect == "d" else super()._use_dense(d, sources)

    def _elements(self, k, x):
        if self.defect != "e" or k.dense or len(x) == 0:
            return x
        x = [bytes(r) for r in x]
        rng = np.random.default_rng(5)
        for i, e in enumerate(x):
            index, count = O.hll_patlen(e)
            if count > 32:  # stored as the largest VAL, and no promotion
                x[i] = E.element(index, 32, 16, rng)
        return x

    def _write_back(self, k, maxima, use_dense):
        ops = None if use_dense or k.dense else O.hll_sparse_pack(maxima)
        if self.defect != "f" or ops is None or 16 + len(ops) > M.MAX_BYTES:
            return super()._write_back(k, maxima, use_dense)
        k.h.ops[:len(ops)] = np.frombuffer(ops, np.uint8)  # the fewest-bytes string, not the replay's
        k.h.len.value, k.h.regs = len(ops), maxima.astype(np.uint8)

    def _deleted(self, key, k):
        self.left[key] = k.h.sparse_ops

    def _new_key(self, key):
        k = super()._new_key(key)
        ops = self.left.pop(key, None)
        if self.defect == "g" and ops:
            k.h.ops[:len(ops)] = np.frombuffer(ops, np.uint8)
            k.h.len.value = len(ops)
        return k

    def _imported_card(self, card):
        return card | INVALID if self.defect == "h" else card

    def pfadd_multi(self, via, key, cmds):
        if self.defect != "i" or self._wrong(*[k for k, _ in cmds]):
            return super().pfadd_multi(via, key, cmds)
        before = {k: M.clone(self.keys[k].h) for k, _ in cmds if k in self.keys}
        replies, seen = [], set()
        for k, spec in cmds:
            reply = self._pfadd_one(k, spec)
            if k in seen and k in before and M.count_of(spec):  # against the registers from before the call
                reply = int(bool(M.clone(before[k]).pfadd(*M.oracle_arena(M.materialize(spec)))))
            seen.add(k)
            replies.append(reply)
        return replies, None

    def _handle_target(self, key, create=True):
        if self.defect != "j":
            return super()._handle_target(key, create)
        if key not in self.bound:
            self.bound[key] = super()._handle_target(key, create)
        return self.bound[key]

    def open(self, via, key):
        if self.defect == "j":
            self.bound[key] = self.keys[key]
        return super().open(via, key)

    def _copied_ttl(self, dst):
        return self.defect == "k" and dst in self.keys and self.keys[dst].ttl


class GpuEngine:
    """The commands through librbx.so.  Keys are `prefix + key`; engine exceptions become the model's error kinds.
    One rbx_hll handle per key stays open from the script's `open` command to close()."""

    def __init__(self, client, prefix: str):
        from redisson_amd.spring_data import RedissonConnection

        self.client, self.prefix = client, prefix
        self.conn = RedissonConnection(client)
        self.handles = {}
        self.bits = self.bloom = None

    def close(self):
        from redisson_amd import _lib as L

        for h in self.handles.values():
            L.lib().rbx_hll_close(h)
        for key in HLLS:
            self._hll(key).delete()
        if self.bits is not None:
            self.bits.delete()
            self.bloom.delete()

    # ---- plumbing --------------------------------------------------------------------------------------------
    def _name(self, key) -> str:
        return self.prefix + key

    def _raw(self, key) -> bytes:
        return self._name(key).encode()

    def _hll(self, key):
        return self.client.getHyperLogLog(self._name(key))

    def _arena(self, spec):
        from redisson_amd import Arena

        x = M.materialize(spec)
        return Arena.fixed(x) if isinstance(x, np.ndarray) and len(x) else Arena([bytes(r) for r in x])

    def _piped(self, fn, *args):
        self.conn.openPipeline()
        try:
            assert fn(*args) is None
        finally:
            results = self.conn.closePipeline()
        assert len(results) == 1
        return results[0]

    def _handle_array(self, keys):
        return (C.c_void_p * len(keys))(*[self.handles[k] for k in keys])

    # ---- setup ------------------------------------------------------------------------------------------------
    def other_types(self, via, key):
        self.bits = self.client.getBitSet(self._name(BITS))
        self.bits.set(5, True)
        self.bloom = self.client.getBloomFilter(self._name(BLOOM))
        assert self.bloom.tryInitRaw(3001, 5)
        self.bloom.add([b"one"])

    def open(self, via, key):
        from redisson_amd import _lib as L
        from redisson_amd.client import _check

        hp = C.c_void_p()
        _check(L.lib().rbx_hll_open(self.client.ctx, self._raw(key), 0, C.byref(hp)))
        self.handles[key] = hp.value

    # ---- PFADD ------------------------------------------------------------------------------------------------
    def pfadd(self, via, key, spec):
        a = self._arena(spec)
        if via == "obj":
            return self._hll(key).addAll(a)
        if via == "async":
            return self._hll(key).addAllAsync(a).get()
        values = [bytes(r) for r in M.materialize(spec)]
        if via == "conn":
            return bool(self.conn.pfAdd(self._raw(key), *values))
        return bool(self._piped(self.conn.pfAdd, self._raw(key), *values))

    def pfadd_multi(self, via, key, cmds):
        from redisson_amd import Arena, hll_add_multi

        parts = [[bytes(r) for r in M.materialize(spec)] for _k, spec in cmds]
        segs = np.zeros(len(cmds) + 1, np.uint64)
        segs[1:] = np.cumsum([len(x) for x in parts])
        els = [e for x in parts for e in x]
        same = {len(e) for e in els}
        arena = Arena.fixed(np.frombuffer(b"".join(els), np.uint8).reshape(len(els), -1)) \
            if len(same) == 1 and same != {0} else Arena(els)
        return hll_add_multi(self.client, [self._name(k) for k, _ in cmds], segs, arena).astype(int).tolist()

    def pfadd_dev(self, via, key, spec):
        import torch

        from redisson_amd import _lib as L
        from redisson_amd import device_keys
        from redisson_amd.client import _check

        x = M.materialize(spec)
        n = len(x)
        if isinstance(x, np.ndarray) and n:
            d_bytes, d_offs, stride = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda(), None, 16
        else:
            buf, offs = O.arena([bytes(r) for r in x])
            d_bytes, stride = torch.from_numpy(buf).cuda(), 0
            d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        d_changed = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        keys = device_keys(d_bytes.data_ptr(), n, stride, None if d_offs is None else d_offs.data_ptr())
        segs = np.array([0, n], np.uint64)
        _check(L.lib().rbx_hll_add_multi_dev(self.client.ctx, self._handle_array([key]), 1, None,
                                             segs.ctypes.data_as(L.u64p), C.byref(keys), d_changed.data_ptr(), None))
        self.client.synchronize()
        return bool(d_changed.item())

    # ---- PFCOUNT ----------------------------------------------------------------------------------------------
    def pfcount(self, via, key):
        if via == "obj":
            return self._hll(key).count()
        if via == "async":
            return self._hll(key).countAsync().get()
        if via == "conn":
            return self.conn.pfCount(self._raw(key))
        return self._piped(self.conn.pfCount, self._raw(key))

    def pfcount_multi(self, via, key, others):
        if via == "obj":
            return self._hll(key).countWith(*[self._name(k) for k in others])
        if via == "async":
            return self._hll(key).countWithAsync(*[self._name(k) for k in others]).get()
        return self.conn.pfCount(self._raw(key), *[self._raw(k) for k in others])

    def count_each(self, via, key, keys):
        from redisson_amd import _lib as L
        from redisson_amd import hll_count_each
        from redisson_amd.client import _check

        if via == "names":
            return [int(x) for x in hll_count_each(self.client, [self._name(k) for k in keys])]
        out = np.full(len(keys), 77, np.uint64)
        _check(L.lib().rbx_hll_count_each_handles(self.client.ctx, self._handle_array(keys), len(keys),
                                                  out.ctypes.data_as(L.u64p)))
        return [int(x) for x in out]

    # ---- PFMERGE, SET / GET, keys -----------------------------------------------------------------------------------
    def pfmerge(self, via, key, srcs):
        if via == "obj":
            return self._hll(key).mergeWith(*[self._name(s) for s in srcs])
        if via == "async":
            return self._hll(key).mergeWithAsync(*[self._name(s) for s in srcs]).get()
        if via == "conn":
            return self.conn.pfMerge(self._raw(key), *[self._raw(s) for s in srcs])
        return self._piped(self.conn.pfMerge, self._raw(key), *[self._raw(s) for s in srcs])

    def set(self, via, key, s):
        self._hll(key).importString(s)

    def get(self, via, key, encoding):
        return self._hll(key).exportString(encoding)

    def delete(self, via, key):
        return self._hll(key).delete()

    def exists(self, via, key):
        return self._hll(key).isExists()

    def expire(self, via, key):
        return self._hll(key).expire(TTL_MS)

    def persist(self, via, key):
        return self._hll(key).clearExpire()

    def ttl(self, via, key):
        t = self._hll(key).remainTimeToLive()
        return "missing" if t == -2 else "none" if t == -1 else "set" if 0 < t <= TTL_MS else f"a time to live of {t}"

    def copy(self, via, key, dst):
        from redisson_amd import _lib as L
        from redisson_amd.client import _check

        src, _keep1 = L.name_struct(self._name(key))
        to, _keep2 = L.name_struct(self._name(dst))
        _check(L.lib().rbx_hll_copy_to(self.client.ctx, src, self.client.ctx, to))

    # ---- the handles' register exchange ---------------------------------------------------------------------------
    def pack(self, via, key):
        import torch

        from redisson_amd import _lib as L
        from redisson_amd.client import _check

        buf = torch.full((M.REGS,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _check(L.lib().rbx_hll_pack_registers(self.client.ctx, self._handle_array([key]), 1, buf.data_ptr(), None))
        self.client.synchronize()
        return buf.cpu().numpy().tobytes()

    def unpack_max(self, via, key, spec):
        import torch

        from redisson_amd import _lib as L
        from redisson_amd.client import _check

        buf = torch.from_numpy(M.image(spec)).cuda()
        torch.cuda.synchronize()
        _check(L.lib().rbx_hll_unpack_max_registers(self.client.ctx, self._handle_array([key]), 1, buf.data_ptr(), None))
        self.client.synchronize()


def _guarded(fn):
    """an engine exception becomes (None, the model's error kind); a device error is no reply and propagates"""
    def run(self, *args):
        from redisson_amd import IllegalArgumentException, RedisException

        try:
            return fn(self, *args), None
        except IllegalArgumentException:
            return None, ILLEGAL
        except RedisException as e:
            for kind in (WRONGTYPE, NO_SUCH_KEY):
                if kind in str(e):
                    return None, kind
            return None, REDIS
    run.__name__ = fn.__name__
    return run


for _k in FAMILY:
    setattr(GpuEngine, _k, _guarded(getattr(GpuEngine, _k)))
