"""Random, seeded, model-checked command sequences over a few shared bit-string keys.

commands(seed, steps) yields plain tuples (kind, via, key, *args); run(engine, seed, steps) sends each to an engine
adapter and to the keyspace model of bitstring_model.py, compares reply and error kind, and every `check_every`
commands reads every key back through the readers that look past a string's end.  Engines: GpuEngine (librbx.so
through RBitSet, RedissonConnection, RBloomFilter and one BloomHandle per Bloom key kept open for the whole
sequence), ModelEngine (a second Keyspace) and FaultyModelEngine (the model with one injected defect, to show
that the sequences and the full check would notice it).

To replay a failure: run(engine, seed, steps, stop_at=step + 1) repeats the prefix that ends with the failing
command; list(commands(seed, steps))[step] is that command."""
import numpy as np

import bitfield_overflow_model as OM
import bitset_model as SM
from bitstring_model import (BIT_OFFSET, FORMS, GET, ILLEGAL, INCRBY, NO_SUCH_KEY, NOT_INIT, POOL, REDIS, SET, WRONGTYPE,
                             Keyspace)

LIMIT = 1 << 23  # offsets stay below 2^23 bits: strings of at most 1 MiB
BITSETS = ("a", "b", "c")
BLOOM, LATE_BLOOM, HLL, MISSING = "f", "g", "h", "m"
STRINGS = BITSETS + (BLOOM, LATE_BLOOM)
BLOOM_CONFIG = {BLOOM: (3001, 5), LATE_BLOOM: (70_001, 7)}
NS = (1, 2, 63, 64, 65, 257, 1000)
BOUNDARIES = (0, 8 * 16, 8 * 256, 8 * 512, 8 * 4096, 8 * 65536)  # bits; the length and twice the length join them
TTL_MS = 3_600_000
I64_MIN, I64_MAX = OM.I64_MIN, OM.I64_MAX
BATCH_TYPES = [(1, False), (2, False), (4, False), (8, False), (16, False), (32, False), (8, True), (16, True),
               (32, True), (64, True), (3, False), (5, True), (7, True), (12, True), (33, False), (63, False)]

FAMILY = {}
for _family, _kinds in {
    "bit": "setbit clearbit getbit", "index": "set_indexes get_indexes", "range": "set_range clear_range",
    "bitop": "bitop bitop_not", "field": "field_get field_set field_incr get_fields set_fields incr_fields bitfield",
    "bitrange": "bitcount bitpos count_ranges pos_ranges",
    "string": "cardinality size length to_bytes set_bytes clear",
    "key": "delete rename expire clear_expire ttl exists", "bloom": "bloom_add bloom_contains bloom_count bloom_init",
    "setup": "hll_init",
}.items():
    for _k in _kinds.split():
        FAMILY[_k] = _family

WEIGHTS = {
    "setbit": 5, "clearbit": 4, "getbit": 3, "set_indexes": 5, "get_indexes": 4, "set_range": 4, "clear_range": 3,
    "bitop": 8, "bitop_not": 2.5, "field_get": 2.5, "field_set": 3, "field_incr": 3, "get_fields": 3.5,
    "set_fields": 4.5, "incr_fields": 5, "bitfield": 3, "bitcount": 3, "bitpos": 4, "count_ranges": 3.5,
    "pos_ranges": 3.5, "cardinality": 1.5, "size": 1.5, "length": 1.5, "to_bytes": 1.5, "set_bytes": 6, "clear": 1.5,
    "delete": 1.5, "rename": 3.5, "expire": 1.5, "clear_expire": 1.2, "ttl": 1.5, "bloom_add": 4, "bloom_contains": 4,
    "bloom_count": 1.2,
}
WRITES = {"setbit", "clearbit", "set_indexes", "set_range", "clear_range", "bitop", "bitop_not", "field_set",
          "field_incr", "set_fields", "incr_fields", "bitfield", "set_bytes", "clear", "delete", "expire", "clear_expire"}
SPRING = {"setbit", "getbit", "bitcount", "bitpos", "bitop", "bitop_not", "size"}  # RedissonConnection has these too
DEVICE = {"set_indexes", "get_indexes", "get_fields", "set_fields", "incr_fields", "count_ranges", "pos_ranges"}
# the kinds that answer WRONGTYPE on a key of another type (the ones taken out do not: they replace, remove or
# time the key whatever it holds, or belong to the Bloom filter)
HLL_OK = set(WEIGHTS) - {"set_bytes", "clear", "delete", "rename", "expire", "clear_expire", "ttl", "bloom_add",
                         "bloom_contains", "bloom_count"}


def label(cmd) -> str:
    """the command kind the coverage conditions count: the device and handle forms are kinds of their own"""
    return cmd[0] + ("_dev" if cmd[1] in ("dev", "handle") else "")


# ---- the generator ------------------------------------------------------------------------------------------
def commands(seed: int, steps: int):
    """`steps` command tuples, a pure function of the seed.  It steps a model of its own to know the lengths."""
    rng = np.random.default_rng([0xB175E9, seed])
    ks = Keyspace()
    state = {"prev": None, "late": False}
    pending = []  # commands that are already decided: the scripted ones, and the second of a pair

    def integer(lo, hi):  # inclusive
        return int(rng.integers(lo, hi, endpoint=True))

    def choice(seq):
        return seq[int(rng.integers(len(seq)))]

    def offset(key, room=1):
        n = ks.strlen(key)
        r = rng.random()
        if r < 0.70:
            o = choice(BOUNDARIES + (8 * n, 16 * n)) + integer(-9, 9)
        elif r < 0.95:
            o = integer(0, 8 * n + 63)
        else:
            o = integer(0, LIMIT - 1)
        return min(max(o, 0), LIMIT - room)

    def strings():
        return STRINGS if state["late"] else BITSETS + (BLOOM,)

    def pick_key(kind):
        if kind in HLL_OK and rng.random() < 0.045:
            return HLL
        pool = strings() if kind in WRITES else strings() + (MISSING,)
        if state["prev"] in pool and rng.random() < 0.5:
            return state["prev"]
        return choice(pool)

    def via_for(kind):
        if kind in DEVICE:
            return choice(("obj", "dev"))
        if kind in SPRING:
            return choice(("obj", "conn"))
        return "obj"

    def indexes(key, n):
        base, spread = offset(key), choice((64, 4096))
        idx = np.clip(base + rng.integers(-spread, spread, n), 0, LIMIT - 1)
        if n >= 4:
            idx[: n // 4] = idx[n // 4: 2 * (n // 4)]  # duplicates for certain
        return tuple(int(i) for i in idx)

    def java(v, bits=64):
        return int(min(max(v, -(1 << (bits - 1))), (1 << (bits - 1)) - 1))

    def value(signed, size, bits=64):
        lo, hi = OM.bounds(signed, size)
        v = choice((integer(-4, 4), choice((lo, hi, hi + 1, lo - 1, hi - lo, lo - hi)), integer(I64_MIN, I64_MAX),
                    integer(lo, hi)))
        return java(v, bits)

    def batch_values(signed, size, n, zero_ok):
        lo, hi = OM.bounds(signed, size)
        m = min(choice((4, max(1, (hi - lo) // 3), hi - lo + 2)), I64_MAX)
        mag = rng.integers(0 if zero_ok else 1, m, n, endpoint=True, dtype=np.int64)
        sign = choice((1, -1, 0))
        signs = rng.choice((1, -1), n) if sign == 0 else np.full(n, sign)
        return tuple(int(v) for v in mag * signs)

    def bound(key, unit):
        t = ks.strlen(key) * (8 if unit == "BIT" else 1)
        if rng.random() < 0.3:
            return -integer(1, t + 12)
        scale = 8 if unit == "BIT" else 1
        return max(0, choice((0, t, t // 2, 16 * scale, 256 * scale, 4096 * scale)) + integer(-9, 9))

    def ranges(key, unit, n):
        t = ks.strlen(key) * (8 if unit == "BIT" else 1)
        starts = bound(key, unit) + rng.integers(-40, 40, n)
        ends = starts + rng.integers(-4, choice((16, 5000, 70_000)), n)
        neg = rng.random(n) < 0.15
        starts = np.where(neg, -rng.integers(1, t + 6, n), starts)
        neg = rng.random(n) < 0.15
        ends = np.where(neg, -rng.integers(1, t + 6, n), ends)
        return tuple(int(s) for s in starts), tuple(int(e) for e in ends)

    def build(kind):
        key = pick_key(kind)
        via = via_for(kind)
        if kind == "setbit":
            return (kind, via, key, offset(key), integer(0, 1))
        if kind == "clearbit" and rng.random() < 0.3:  # a SETBIT 0 behind the end: it lengthens the string all the same
            return (kind, via, key, min(8 * ks.strlen(key) + integer(0, 600), LIMIT - 1))
        if kind in ("clearbit", "getbit"):
            return (kind, via, key, offset(key))
        if kind == "set_indexes":
            return (kind, via, key, indexes(key, choice(NS)), integer(0, 1))
        if kind == "get_indexes":
            return (kind, via, key, indexes(key, choice(NS)))
        if kind in ("set_range", "clear_range"):
            frm = offset(key)
            to = min(LIMIT, max(0, choice((frm + integer(-2, 70), frm + integer(100, 5000), offset(key)))))
            return (kind, "obj", key, frm, to)
        if kind == "bitop":
            return bitop(key, via)
        if kind == "bitop_not":
            src = key if via == "obj" or rng.random() < 0.5 else choice(strings() + (MISSING,))
            if key == HLL:
                via = "conn"
            return (kind, via, key, src)
        if kind in ("field_get", "field_set", "field_incr"):
            form = choice(tuple(FORMS))
            signed, fixed = FORMS[form]
            size = fixed or integer(1, 64 if signed else 63)
            if fixed is None and key != HLL and rng.random() < 0.04:
                size = 65 if signed else 64  # Redisson's own limit: illegal argument
            off = offset(key, min(size, 64))
            if kind == "field_get":
                return (kind, "obj", key, form, size, off)
            return (kind, "obj", key, form, size, off, value(signed, min(size, 64 if signed else 63), fixed or 64))
        if kind in ("get_fields", "set_fields", "incr_fields"):
            size, signed = choice(BATCH_TYPES)
            n = choice(NS)
            base = offset(key, 64 * 30)
            if rng.random() < 0.6:
                offs = (base // size + rng.integers(0, 24, n)) * size
            else:
                offs = base + rng.integers(0, 3 * size + 1, n)  # unaligned, partly overlapping
            offs = tuple(int(o) for o in offs)
            if kind == "get_fields":
                return (kind, via, key, size, signed, offs)
            return (kind, via, key, size, signed, offs, batch_values(signed, size, n, kind == "set_fields"),
                    choice(("WRAP", "SAT", "FAIL")), bool(integer(0, 1)))
        if kind == "bitfield":
            base = offset(key, 300)
            rows = []
            for _ in range(integer(1, 10)):
                signed = bool(integer(0, 1))
                size = integer(1, 64 if signed else 63)
                op = integer(0, 2)
                rows.append((op, signed, size, base + integer(0, 150), value(signed, size),
                             choice((None, "WRAP", "SAT", "FAIL")) if op == INCRBY else None))
            return (kind, "conn", key, tuple(rows))
        if kind == "bitcount":
            if rng.random() < 0.25:
                return (kind, via, key, None, None, "BYTE")
            unit = "BYTE" if via == "conn" else choice(("BYTE", "BIT"))
            return (kind, via, key, bound(key, unit), bound(key, unit), unit)
        if kind == "bitpos" and key != HLL and rng.random() < 0.25:
            # a run of ones first, then the search for a 0 inside it: the end bound is all that keeps the reply at -1
            first = offset(key, 8 * 70) // 8
            last = first + integer(0, 60)
            pending.append((kind, via, key, 0, 2, first, last, "BYTE"))
            return ("set_range", "obj", key, 8 * first, 8 * last + 8)
        if kind == "bitpos":
            nargs = integer(0, 2)
            unit = "BYTE" if via == "conn" or nargs < 2 else choice(("BYTE", "BIT"))
            start = bound(key, unit)
            end = choice((bound(key, unit), start + integer(-3, 40)))
            return (kind, via, key, integer(0, 1), nargs, start if nargs else 0, end if nargs == 2 else 0, unit)
        if kind == "count_ranges":
            unit = choice(("BYTE", "BIT"))
            return (kind, via, key, *ranges(key, unit, choice(NS)), unit)
        if kind == "pos_ranges":
            unit = choice(("BYTE", "BIT"))
            starts, ends = ranges(key, unit, choice(NS))
            if rng.random() < 0.3:
                unit, ends = "BYTE", None
            return (kind, via, key, integer(0, 1), starts, ends, unit)
        if kind in ("cardinality", "length", "to_bytes", "clear", "delete", "expire", "clear_expire", "ttl"):
            return (kind, "obj", key)
        if kind == "size":
            return (kind, via, key)
        if kind == "set_bytes":
            n = ks.strlen(key)
            shorter = [m for m in (1, 15, 16, 17, 255, 256, 257, n // 2, n - 1) if 1 <= m < n]
            longer = [min(LIMIT // 8, n + m) for m in (1, 15, 16, 17, 255, 256, 300, 4096, max(n, 1))]
            return (kind, "obj", key, choice(shorter) if shorter and rng.random() < 0.65 else choice(longer),
                    integer(0, 1 << 30))
        if kind == "rename":
            src = MISSING if rng.random() < 0.08 else choice(BITSETS)
            gone = [k for k in strings() if k != src and ks.strlen(k) == 0]
            there = [k for k in strings() if k != src and ks.strlen(k)]
            new = choice(gone) if gone and (not there or rng.random() < 0.7) else choice(there or [k for k in BITSETS if k != src])
            if src != MISSING and new in there and rng.random() < 0.35:  # DEL the target first: a rename onto a missing key
                pending.append((kind, "obj", src, new))
                return ("clear", "obj", new)
            return (kind, "obj", src, new)
        if kind in ("bloom_add", "bloom_contains"):
            key = LATE_BLOOM if state["late"] and rng.random() < 0.5 else BLOOM
            n = choice(NS)
            ids = rng.integers(0, len(POOL), n)
            if n >= 4:
                ids[: n // 4] = ids[n // 4: 2 * (n // 4)]
            return (kind, choice(("obj", "handle")), key, tuple(int(i) for i in ids))
        if kind == "bloom_count":
            return (kind, "obj", LATE_BLOOM if state["late"] and rng.random() < 0.5 else BLOOM)
        raise AssertionError(kind)

    def bitop(dest, via):
        op = choice(("and", "or", "xor"))
        pool = strings() + (MISSING,)
        if dest == HLL:
            return ("bitop", "conn", choice(strings()), op, (choice(pool), HLL))
        by_len = sorted(strings(), key=ks.strlen)
        r = rng.random()
        if r < 0.4 and ks.strlen(by_len[0]) < ks.strlen(by_len[-1]):
            dest = by_len[0]  # dest among its sources, and the result is longer than dest
            srcs = [dest, by_len[-1]] + [choice(pool) for _ in range(integer(0, 2))]
        elif r < 0.6 and 0 < ks.strlen(by_len[-2]) < ks.strlen(by_len[-1]):
            dest = by_len[-1]  # a result shorter than dest
            srcs = [choice([k for k in by_len[:-1] if ks.strlen(k)]) for _ in range(integer(1, 3))]
            via = "conn"
        else:
            srcs = [choice(pool) for _ in range(integer(1, 4))]
            if rng.random() < 0.4:
                srcs[integer(0, len(srcs) - 1)] = dest
        if via == "obj":  # RBitSet's own forms: the object is the destination and the first source
            srcs = [dest] + [s for s in srcs if s != dest][:3]
        else:
            srcs = [srcs[i] for i in rng.permutation(len(srcs))]
        return ("bitop", via, dest, op, tuple(srcs))

    def step(cmd):
        getattr(ks, cmd[0])(*cmd[1:])
        state["prev"] = cmd[2]
        return cmd

    kinds = list(WEIGHTS)
    p = np.array([WEIGHTS[k] for k in kinds], float)
    p /= p.sum()
    late_at = steps // 3
    script = {0: [("hll_init", "obj", HLL), ("bloom_init", "obj", BLOOM, *BLOOM_CONFIG[BLOOM])],
              # a 256-byte string first, its config after it: the next contains has to grow the allocation
              late_at: [("setbit", "obj", LATE_BLOOM, 2047, 1), ("setbit", "conn", LATE_BLOOM, 5, 1),
                        ("bloom_init", "obj", LATE_BLOOM, *BLOOM_CONFIG[LATE_BLOOM]),
                        ("bloom_contains", "obj", LATE_BLOOM, tuple(range(0, 130, 2))),
                        ("bloom_add", "handle", LATE_BLOOM, tuple(range(64)))]}
    for done in range(steps):
        pending += script.get(done, [])
        cmd = pending.pop(0) if pending else build(kinds[int(rng.choice(len(kinds), p=p))])
        if cmd[0] == "bloom_init" and cmd[2] == LATE_BLOOM:
            state["late"] = True
        yield step(cmd)


# ---- what a sequence covers (test_bit_sequences_cpu.py asserts on it) ------------------------------------------
def stats(seed: int, steps: int) -> dict:
    ks = Keyspace()
    out = {"kinds": {}, "after_other_family": set(), "errors": 0, "growths": 0, "shrinks": 0, "self_growing_bitops": 0,
           "forms": {}, "renames": {"existing": 0, "missing": 0}, "n": 0}
    prev = None
    for cmd in commands(seed, steps):
        kind, key = cmd[0], cmd[2]
        before = {k: ks.strlen(k) for k in STRINGS}
        if kind == "rename":
            out["renames"]["existing" if ks.strlen(cmd[3]) else "missing"] += ks.strlen(key) > 0
        _reply, err = getattr(ks, kind)(*cmd[1:])
        out["n"] += 1
        out["errors"] += err is not None
        out["kinds"][label(cmd)] = out["kinds"].get(label(cmd), 0) + 1
        if kind.startswith("field_"):
            out["forms"][cmd[3]] = out["forms"].get(cmd[3], 0) + 1
        if prev is not None and prev[2] == key and FAMILY[prev[0]] != FAMILY[kind]:
            out["after_other_family"].add(label(cmd))
        for k in STRINGS:
            was, now = before[k], ks.strlen(k)
            out["growths"] += kind != "rename" and now > was and (now + 255) // 256 > (was + 255) // 256
            out["shrinks"] += kind in ("set_bytes", "bitop", "bitop_not") and k == key and 0 < now < was
        if kind in ("bitop", "bitop_not") and err is None:
            srcs = cmd[4] if kind == "bitop" else (cmd[3],)
            # dest among the sources, and the result needs a larger allocation than dest had (a multiple of 256 bytes)
            out["self_growing_bitops"] += key in srcs and (ks.strlen(key) + 255) // 256 > (before[key] + 255) // 256
        prev = cmd
    return out


# ---- the full check -------------------------------------------------------------------------------------------
def probes(model: Keyspace, seed: int, step: int):
    """Read-only commands over every key: existence, the bytes, the counts, and the readers that look past the
    string's end -- the gather kernel over the 4,096 bits after it, the range kernels across it, 64-bit fields over
    its last 9 bytes and the 16 after them -- and the Bloom keys through their long-lived handles."""
    rng = np.random.default_rng([0xC4EC, seed, step])
    out = [("exists", "obj", HLL)]
    for i, key in enumerate(STRINGS + (MISSING,)):
        n = model.strlen(key)
        via = "dev" if (step + i) % 2 else "obj"
        tail = tuple(range(8 * n, 8 * n + 4096)) + tuple(int(x) for x in rng.integers(0, LIMIT, 64))
        first = 8 * max(n - 9, 0)
        ones = np.flatnonzero(np.frombuffer(model.data.get(key, b""), np.uint8) == 0xFF)
        full = int(ones[0]) if ones.size else 0  # a byte of ones if there is one: BITPOS 0 inside it finds nothing
        out += [("exists", "obj", key), ("to_bytes", "obj", key), ("size", "obj", key), ("cardinality", "obj", key),
                ("ttl", "obj", key), ("get_indexes", via, key, tail),
                ("bitcount", "obj", key, n - 1, n + 300, "BYTE"), ("bitpos", "obj", key, 1, 1, n, 0, "BYTE"),
                ("bitpos", "obj", key, 0, 1, max(n - 2, 0), 0, "BYTE"), ("bitpos", "obj", key, 0, 2, full, full, "BYTE"),
                ("get_fields", via, key, 64, True, tuple(range(first, first + 137, 3)))]
        if key in model.cfg:
            out.append(("bloom_contains", "handle", key, tuple(range(200))))
    return out


def short(x, keep=6):
    """a command tuple with its long arrays cut, for messages"""
    if isinstance(x, (tuple, list)):
        if len(x) > 12 and all(isinstance(v, int) for v in x):
            return f"<{len(x)} ints: {', '.join(map(str, x[:keep]))}, ...>"
        return type(x)(short(v, keep) for v in x)
    if isinstance(x, bytes) and len(x) > 24:
        return f"<{len(x)} bytes: {x[:12].hex()}...>"
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


def run(engine, seed: int, steps: int, check_every: int = 25, stop_at=None) -> None:
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
        for probe in probes(model, seed, step):
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


class FaultyModelEngine(Keyspace):
    """The model with one wrong answer, `defect` in 'a' .. 'h' (test_bit_sequences_cpu.py lists them).  It keeps what
    a correct model has no use for: per key the stale bytes behind the string's end (`stale`), which the readers
    that look past the end see and which a SETBIT-style growth turns into part of the string, and the bytes an
    open Bloom handle was left reading (`frozen`)."""

    def __init__(self, defect: str):
        super().__init__()
        assert defect in "abcdefgh" and len(defect) == 1
        self.defect = defect
        self.stale = {}
        self.frozen = {}

    def _padded(self, key):
        data = self._get(key)
        return (data or b"") + self.stale[key] if self.stale.get(key) else data

    def _handle_view(self, key):
        return self.frozen.get(key, self._get(key))

    def _allocation(self, key, n):
        floor = (self.cfg[key][0] + 7) // 8 if key in self.cfg else 1
        return (max(n, floor, 1) + 255) // 256

    def _put(self, key, new, how="write"):
        old = self.data.get(key, b"")
        new = bytearray(new or b"")
        tail = self.stale.pop(key, b"")
        if how == "write" and new:
            grown = len(new) - len(old)
            if grown > 0 and tail:  # the growth uncovers what was left behind the end
                for i, t in enumerate(tail[:grown]):
                    new[len(old) + i] |= t
            if tail[max(grown, 0):]:
                self.stale[key] = tail[max(grown, 0):]
            if self.defect == "b" and grown >= 2:
                new[len(old)] ^= 0x04
            if self.defect == "g" and key in self.cfg and self._allocation(key, len(new)) > self._allocation(key, len(old)):
                self.frozen.setdefault(key, old or None)
        else:
            self.frozen.pop(key, None)
            shrinks = 0 < len(new) < len(old)
            if shrinks and ((self.defect == "a" and how == "bitop") or (self.defect == "d" and how == "set")):
                self.stale[key] = old[len(new):]
        super()._put(key, bytes(new), how)

    def _zero_past_the_end(self, key, i):
        return self.defect == "c" and (i >> 3) >= self.strlen(key) and key not in self.hll

    def setbit(self, via, key, i, value):
        if not value and self._zero_past_the_end(key, i):
            return False, None
        return super().setbit(via, key, i, value)

    def clearbit(self, via, key, i):
        if self._zero_past_the_end(key, i):
            return False, None
        return super().clearbit(via, key, i)

    def bitpos(self, via, key, bit, nargs, start, end, unit):
        if self.defect == "e" and bit == 0 and nargs == 2:
            end = -1
        return super().bitpos(via, key, bit, nargs, start, end, unit)

    def _fields_model(self, win, op, signed, size, mode, offsets, values):
        if not (self.defect == "f" and mode == OM.SAT and signed and op != GET):
            return super()._fields_model(win, op, signed, size, mode, offsets, values)
        # one sub-command at a time: where a signed field saturates upwards it gets the unsigned bound, all ones
        replies = []
        for o, v in zip(offsets, values):
            before = win
            win, (reply,) = OM.fields(before, op, True, size, OM.SAT, [o], [v])
            overflowed = OM.fields(before, op, True, size, OM.FAIL, [o], [v])[1][0] is None
            if overflowed and OM.fields(win, GET, True, size, OM.WRAP, [o])[1][0] == OM.bounds(True, size)[1]:
                win = OM.fields(win, SET, True, size, OM.WRAP, [o], [-1])[0]
                reply = -1 if op == INCRBY else reply
            replies.append(reply)
        return win, replies

    def _bitop_value(self, op, dest, srcs, values):
        res = SM.bitop(op, values)
        if self.defect == "h" and dest in srcs:
            return SM.bitop(op, [res if s == dest else v for s, v in zip(srcs, values)])
        return res


class GpuEngine:
    """The commands through librbx.so.  Keys are `prefix + key`; engine exceptions become the model's error kinds.
    One BloomHandle per Bloom key stays open from its first use (the first key's: from its config) to close()."""

    def __init__(self, client, prefix: str):
        from redisson_amd.spring_data import RedissonConnection

        self.client, self.prefix = client, prefix
        self.conn = RedissonConnection(client)
        self.filters, self.handles, self.hlls = {}, {}, {}

    def close(self):
        for h in self.handles.values():
            h.close()
        for f in self.filters.values():
            f.delete()
        for h in self.hlls.values():
            h.delete()
        for key in STRINGS:
            self._bs(key).delete()

    # ---- plumbing --------------------------------------------------------------------------------------------
    def _name(self, key) -> str:
        return self.prefix + key

    def _bs(self, key):
        return self.client.getBitSet(self._name(key))

    def _raw(self, key) -> bytes:
        return self._name(key).encode()

    def _dev(self, values, dtype=np.int64):
        import torch

        t = torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype).reshape(-1).view(np.int64))).cuda()
        torch.cuda.synchronize()
        return t

    def _out(self, n, dtype):
        import torch

        t = torch.full((max(n, 1),), 77, dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        return t

    def _back(self, t, n):
        self.client.synchronize()
        return t.cpu().numpy()[:n]

    # ---- single bits, index batches, ranges -----------------------------------------------------------------------
    def setbit(self, via, key, i, value):
        if via == "conn":
            return self.conn.setBit(self._raw(key), i, bool(value))
        return self._bs(key).set(i, bool(value))

    def clearbit(self, via, key, i):
        return self._bs(key).clearBit(i)

    def getbit(self, via, key, i):
        return self.conn.getBit(self._raw(key), i) if via == "conn" else self._bs(key).get(i)

    def set_indexes(self, via, key, idx, value):
        if via == "dev":
            d = self._dev(idx, np.uint64)
            self._bs(key).setIndexesDev(d.data_ptr(), len(idx), bool(value))
            self.client.synchronize()
        else:
            self._bs(key).setIndexes(np.asarray(idx, np.uint64), bool(value))

    def get_indexes(self, via, key, idx):
        if via == "dev":
            import torch

            d, out = self._dev(idx, np.uint64), self._out(len(idx), torch.uint8)
            self._bs(key).getIndexesDev(d.data_ptr(), len(idx), out.data_ptr())
            return self._back(out, len(idx)).astype(int).tolist()
        return self._bs(key).getIndexes(np.asarray(idx, np.uint64)).astype(int).tolist()

    def set_range(self, via, key, frm, to):
        self._bs(key).setRange(frm, to)

    def clear_range(self, via, key, frm, to):
        self._bs(key).clearRange(frm, to)

    # ---- BITOP ------------------------------------------------------------------------------------------------------
    def bitop(self, via, dest, op, srcs):
        if via == "conn":
            return self.conn.bitOp(op.upper(), self._raw(dest), *[self._raw(s) for s in srcs])
        assert srcs[0] == dest
        bs = self._bs(dest)
        {"and": bs.and_, "or": bs.or_, "xor": bs.xor}[op](*[self._name(s) for s in srcs[1:]])

    def bitop_not(self, via, dest, src):
        if via == "conn":
            return self.conn.bitOp("NOT", self._raw(dest), self._raw(src))
        assert src == dest
        self._bs(dest).not_()

    # ---- typed fields ---------------------------------------------------------------------------------------------
    def _field(self, key, what, form, size, offset, *value):
        bs = self._bs(key)
        names = {"get": "get{}", "set": "set{}", "incr": "incrementAndGet{}"}
        fn = getattr(bs, names[what].format(form.capitalize()))
        return fn(size, offset, *value) if FORMS[form][1] is None else fn(offset, *value)

    def field_get(self, via, key, form, size, offset):
        return self._field(key, "get", form, size, offset)

    def field_set(self, via, key, form, size, offset, value):
        return self._field(key, "set", form, size, offset, value)

    def field_incr(self, via, key, form, size, offset, value):
        return self._field(key, "incr", form, size, offset, value)

    def get_fields(self, via, key, size, signed, offsets):
        if via == "dev":
            import torch

            d, out = self._dev(offsets, np.uint64), self._out(len(offsets), torch.int64)
            self._bs(key).getFieldsDev(size, d.data_ptr(), len(offsets), out.data_ptr(), signed)
            return self._back(out, len(offsets)).tolist()
        return self._bs(key).getFields(size, np.asarray(offsets, np.uint64), signed).tolist()

    def _write_fields(self, via, key, op, size, signed, offsets, values, mode, replies):
        bs, n = self._bs(key), len(offsets)
        if via == "dev":
            import torch

            d_offs, d_vals = self._dev(offsets, np.uint64), self._dev(values)
            d_rep = self._out(n, torch.int64) if replies else None
            d_nil = self._out(n, torch.uint8) if mode != "WRAP" else None
            fn = bs.setFieldsDev if op == SET else bs.incrementFieldsDev
            fn(size, d_offs.data_ptr(), d_vals.data_ptr(), n, None if d_rep is None else d_rep.data_ptr(), signed,
               overflow=mode, d_nil=None if d_nil is None else d_nil.data_ptr())
            rep = None if d_rep is None else self._back(d_rep, n)
            nil = None if d_nil is None else self._back(d_nil, n).astype(bool)
            if mode != "FAIL":
                assert nil is None or not nil.any()
                nil = None
        else:
            fn = bs.setFields if op == SET else bs.incrementFields
            got = fn(size, np.asarray(offsets, np.uint64), np.asarray(values, np.int64), signed, replies, overflow=mode)
            rep, nil = got if mode == "FAIL" else (got, None)
        if rep is not None:
            rep = [None if nil is not None and nil[i] else int(r) for i, r in enumerate(rep)]
        return rep, None if nil is None else [bool(z) for z in nil]

    def set_fields(self, via, key, size, signed, offsets, values, mode, replies):
        return self._write_fields(via, key, SET, size, signed, offsets, values, mode, replies)

    def incr_fields(self, via, key, size, signed, offsets, values, mode, replies):
        return self._write_fields(via, key, INCRBY, size, signed, offsets, values, mode, replies)

    def bitfield(self, via, key, rows):
        from redisson_amd.spring_data import BitFieldGet, BitFieldIncrBy, BitFieldSet, BitFieldType

        cmds = []
        for op, signed, size, offset, value, overflow in rows:
            t = BitFieldType(signed, size)
            cmds.append(BitFieldGet(t, offset) if op == GET else BitFieldSet(t, offset, value) if op == SET
                        else BitFieldIncrBy(t, offset, value, overflow))
        return self.conn.bitField(self._raw(key), cmds)

    # ---- ranged BITCOUNT / BITPOS ----------------------------------------------------------------------------------------
    def bitcount(self, via, key, start, end, unit):
        if via == "conn":
            return self.conn.bitCount(self._raw(key), start, end)
        return self._bs(key).bitCount(start, end, unit)

    def bitpos(self, via, key, bit, nargs, start, end, unit):
        lower, upper = (start if nargs >= 1 else None), (end if nargs == 2 else None)
        if via == "conn":
            return self.conn.bitPos(self._raw(key), bool(bit), (lower, upper))
        return self._bs(key).bitPos(bit, lower, upper, unit)

    def count_ranges(self, via, key, starts, ends, unit):
        if via == "dev":
            import torch

            d_s, d_e, out = self._dev(starts), self._dev(ends), self._out(len(starts), torch.int64)
            self._bs(key).countRangesDev(d_s.data_ptr(), d_e.data_ptr(), len(starts), out.data_ptr(), unit)
            return self._back(out, len(starts)).tolist()
        return [int(x) for x in self._bs(key).countRanges(np.asarray(starts, np.int64), np.asarray(ends, np.int64), unit)]

    def pos_ranges(self, via, key, bit, starts, ends, unit):
        if via == "dev":
            import torch

            d_s, d_e = self._dev(starts), None if ends is None else self._dev(ends)
            out = self._out(len(starts), torch.int64)
            self._bs(key).posRangesDev(bit, d_s.data_ptr(), None if d_e is None else d_e.data_ptr(), len(starts),
                                       out.data_ptr(), unit)
            return self._back(out, len(starts)).tolist()
        return self._bs(key).posRanges(bit, np.asarray(starts, np.int64),
                                       None if ends is None else np.asarray(ends, np.int64), unit).tolist()

    # ---- the whole string, key level -----------------------------------------------------------------------------------------
    def cardinality(self, via, key):
        return self._bs(key).cardinality()

    def size(self, via, key):
        return 8 * self.conn.strLen(self._raw(key)) if via == "conn" else self._bs(key).size()

    def length(self, via, key):
        return self._bs(key).length()

    def to_bytes(self, via, key):
        return self._bs(key).toByteArray()

    def set_bytes(self, via, key, nbytes, seed):
        self._bs(key).setBytes(np.random.default_rng(seed).bytes(nbytes))

    def exists(self, via, key):
        return self._bs(key).isExists()

    def delete(self, via, key):
        return self._bs(key).delete()

    def clear(self, via, key):
        self._bs(key).clear()

    def rename(self, via, key, new):
        self._bs(key).rename(self._name(new))

    def expire(self, via, key):
        return self._bs(key).expire(TTL_MS)

    def clear_expire(self, via, key):
        return self._bs(key).clearExpire()

    def ttl(self, via, key):
        t = self._bs(key).remainTimeToLive()
        return "missing" if t == -2 else "none" if t == -1 else "set" if 0 < t <= TTL_MS else f"a time to live of {t}"

    # ---- the other type, and Bloom ---------------------------------------------------------------------------------------------
    def hll_init(self, via, key):
        self.hlls[key] = self.client.getHyperLogLog(self._name(key))
        assert self.hlls[key].addAll([b"one", b"two"])

    def bloom_init(self, via, key, size, k):
        f = self.client.getBloomFilter(self._name(key))
        created = f.tryInitRaw(size, k)
        self.filters[key] = f
        if key == BLOOM:  # open before the first write; the late key's opens after the contains that grows its string
            self._handle(key)
        return created

    def _handle(self, key):
        from redisson_amd import BloomHandle

        if key not in self.handles:
            self.handles[key] = BloomHandle(self.client, self._name(key))  # stays open until close()
        return self.handles[key]

    def _bloom(self, via, key, ids, add):
        from redisson_amd import Arena, device_keys

        mat = POOL[np.asarray(ids, np.int64)]
        if via == "handle":
            import torch

            d_keys = torch.from_numpy(np.ascontiguousarray(mat)).cuda()
            out, cnt = self._out(len(ids), torch.uint8), torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            h = self._handle(key)
            (h.add_dev if add else h.contains_dev)(device_keys(d_keys.data_ptr(), len(ids), 16), cnt.data_ptr(), out.data_ptr())
            flags = self._back(out, len(ids))
            return int(cnt.item()), flags.astype(int).tolist()
        f = self.filters[key]
        count, flags = (f.addEach if add else f.containsEach)(Arena([row.tobytes() for row in mat]))
        return count, flags.astype(int).tolist()

    def bloom_add(self, via, key, ids):
        return self._bloom(via, key, ids, True)

    def bloom_contains(self, via, key, ids):
        return self._bloom(via, key, ids, False)

    def bloom_count(self, via, key):
        return self.filters[key].count()


def _guarded(fn):
    """an engine exception becomes (None, the model's error kind); a device error is no reply and propagates"""
    def run(self, *args):
        from redisson_amd import IllegalArgumentException, RedisException
        from redisson_amd.exceptions import IllegalStateException

        try:
            return fn(self, *args), None
        except IllegalArgumentException:
            return None, ILLEGAL
        except IllegalStateException:
            return None, NOT_INIT
        except RedisException as e:
            for kind in (WRONGTYPE, BIT_OFFSET, NO_SUCH_KEY):
                if kind in str(e):
                    return None, kind
            return None, REDIS
    run.__name__ = fn.__name__
    return run


for _k in FAMILY:
    setattr(GpuEngine, _k, _guarded(getattr(GpuEngine, _k)))
