"""The seeded random plan for rbx_bitset_range_stream: 200 calls of 1 to 60 read queries over 18 bit-string keys plus
two keys of another type (an HLL and a Bloom filter's {name}:config), with writes through the single calls between
them.  It is data only: test_rangestream_cpu.py checks the plan's share of failing commands on the model alone,
test_rangestream_gpu.py runs it on the engine.

A call is (writes, cmd_key, rows).  writes are applied first, in order: ("set_bytes", key, length, seed) = SET key
<length random bytes>, ("set", key, bit) = SETBIT key bit 1, ("or", dest, src) = BITOP OR dest dest src, ("delete",
key), ("expire", key).  rows are (op, bit, nargs, start, end, unit) as bitset_range_stream_call takes them.  Lengths
come from LENGTHS: the edges of the 16-byte vectors, of the test's short_max (64) and of its tile (4096); starts and
ends are drawn around 0, around the string's ends in both units, and far outside.  Key 0 starts out missing, so a
length() on it fails in its script; with P_BAD_BIT / P_SYNTAX a BITPOS gets a bad bit or a unit without an end, and
with P_WRONG a command goes to a key of another type."""
import numpy as np

import rangestream_model as M

SEED = 20261021
LENGTHS = (1, 15, 16, 17, 46, 63, 64, 65, 255, 256, 4095, 4096, 4097, 12293)
NKEYS = 18  # bit strings; the names' entries NKEYS and NKEYS + 1 are the two keys of another type
OPS = (M.COUNT, M.COUNT, M.COUNT, M.COUNT, M.POS, M.POS, M.POS, M.POS, M.STRLEN, M.LENGTH)
# 1 command in 8 may fail; these three make about 1 in 20 fail, and a length() on a missing key or on a string whose
# last byte is zero adds under 1 in 50, so the committed seed stays under the cap with room
P_BAD_BIT, P_SYNTAX, P_WRONG = 0.03, 0.03, 0.03
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def names(prefix):
    """the call's names: 18 bit strings, an HLL, a {name}:config"""
    return [prefix + "k%d" % i for i in range(NKEYS)] + [prefix + "hll", "{" + prefix + "bloom}:config"]


def bound(rng, length, unit):
    """a start or an end: near 0, near the string's end counted from either side, or far outside"""
    t = length * 8 if unit == M.BIT else length
    u = rng.random()
    if u < 0.35:
        return int(rng.integers(-3, 4))
    if u < 0.7:
        return int(t - 1 + rng.integers(-3, 4)) * (1 if rng.random() < 0.5 else -1)
    if u < 0.9:
        return int(rng.integers(-t - 2, t + 3))
    return int(rng.choice((INT64_MIN, INT64_MAX, -(1 << 40), 1 << 40)))


def seeded_calls(seed=SEED, ncalls=200):
    rng = np.random.default_rng(seed)
    lengths = [0] * NKEYS  # what the plan believes each string's length to be: it only shapes the bounds
    calls = []
    for c in range(ncalls):
        writes = []
        for _ in range(int(rng.integers(0, 4)) if c else NKEYS - 1):
            key = int(rng.integers(0, NKEYS)) if c else 1 + len(writes)
            u = rng.random() if c else 0.0
            if u < 0.5:
                lengths[key] = int(rng.choice(LENGTHS))
                writes.append(("set_bytes", key, lengths[key], int(rng.integers(0, 1 << 31))))
            elif u < 0.65:
                bit = int(rng.integers(0, 8 * max(lengths[key], 1) + 64))
                lengths[key] = max(lengths[key], bit // 8 + 1)
                writes.append(("set", key, bit))
            elif u < 0.8:
                src = int(rng.integers(0, NKEYS))
                lengths[key] = max(lengths[key], lengths[src])
                writes.append(("or", key, src))
            elif u < 0.9:
                lengths[key] = 0
                writes.append(("delete", key))
            else:
                writes.append(("expire", key))
        cmd_key, rows = [], []
        for _ in range(int(rng.integers(1, 61))):
            key = int(rng.integers(0, NKEYS))
            op = int(rng.choice(OPS))
            unit = int(rng.integers(0, 2))
            nargs = 2 * int(rng.integers(0, 2)) if op == M.COUNT else int(rng.integers(0, 3))
            bit = int(rng.integers(0, 2))
            if op == M.POS and nargs < 2:
                unit = M.BIT if rng.random() < P_SYNTAX else M.BYTE
            if op == M.POS and rng.random() < P_BAD_BIT:
                bit = int(rng.choice((2, 3, 255)))
            if rng.random() < P_WRONG:
                key = NKEYS + int(rng.integers(0, 2))
            length = lengths[key] if key < NKEYS else 16
            cmd_key.append(key)
            rows.append((op, bit, nargs, bound(rng, length, unit), bound(rng, length, unit), unit))
        calls.append((writes, cmd_key, rows))
    return calls


def write_on_model(ks, nm, write):
    """one write of the plan on a bitstring_model.Keyspace"""
    what, key = write[0], nm[write[1]]
    if what == "set_bytes":
        ks.set_bytes("plan", key, write[2], write[3])
    elif what == "set":
        ks.setbit("plan", key, write[2], 1)
    elif what == "or":
        ks.bitop("plan", key, "or", [key, nm[write[2]]])
    elif what == "delete":
        ks.delete("plan", key)
    else:
        ks.expire("plan", key)
