"""Random, seeded, model-checked Bloom filter command sequences over a few shared filters (the shape of
hll_driver.py and bitstring_driver.py).

commands(seed, steps) yields plain tuples (kind, via, key, *args); run(engine, seed, steps) sends each to an engine
adapter and to the keyspace model of bloom_model.py, compares reply and error kind, and every `check_every` commands
reads every filter back: the exported string byte for byte, isExists, the config, the PTTL sign, count(), and 200
keys through containsEach by name, through the filter's long-lived handle and through one contains_multi that names
every handle whose config still holds.  Engines: GpuEngine (librbx.so through RBloomFilter, rbx_bloom_add /
_contains with and without a cached config, their async forms, BloomHandle.add_dev / contains_dev, the multi-tenant
calls and the ordered stream in their host and device forms, RBitSet on a filter's name, and one BloomHandle per
filter kept open for the whole sequence beside short-lived ones), ModelEngine (a second keyspace) and
FaultyModelEngine (the model with one injected defect).

What the sequences are there to check is the host state behind the kernels (api_bloom.cpp, api_bloom_multi.cpp,
api_staging.cpp, keyspace.cpp): the descriptor table cached by handle, serial, generation and the create flag; the
handles' re-binding by keyspace generation; the Redis length word that every add path writes; the choice of kernel
by (k, size, n) and of host tier by the batch; and the in-order replies across calls, paths and streams.

What they leave out, on purpose: a stream in its DEVICE form that only reads a filter without a string, and an empty
segment of add_multi's device form on one.  Both bind the filter for writing before the host can know whether a
bit will be set (upload_filters, create = true), which leaves an empty string behind where Redis would have none
(rbx_bloom_stream_dev documents it).  The host form of the stream reads its ops and is held to the model.

To replay a failure: run(engine, seed, steps, stop_at=step + 1); list(commands(seed, steps))[step] is the command."""
import ctypes as C

import numpy as np

import bloom_model as M
from bloom_model import ARITH, CONFIG, ILLEGAL, NO_SUCH_KEY, NOT_INIT, REDIS, WRONGTYPE, BloomKeyspace
from oracle import oracle as O

TINY, SMALL, REGION, BIG, K17, K40, LATE, MISSING, REINIT = "a", "b", "c", "d", "e", "f", "g", "m", "r"
HLL, SPARE = "h", "s"
CONFIGS = {TINY: (64, 7), SMALL: (729, 5), REGION: (65_537, 10), BIG: (5_000_011, 7), K17: (100_003, 17),
           K40: (1000, 40), LATE: (70_001, 7), MISSING: (3001, 5), REINIT: (4099, 6), HLL: (512, 3)}
OTHER_CONFIG = (8191, 9)  # what REINIT is sometimes re-initialised with
FILTERS = (TINY, SMALL, REGION, BIG, K17, K40, LATE, MISSING, REINIT)
CHECKED = FILTERS + (SPARE,)
LONG_LIVED = {key: hid for hid, key in enumerate(FILTERS)}  # handle ids; HLL's is 9, short-lived ones from 100
HLL_HANDLE = 9
LATE_BIT = 80_003  # the RBitSet string LATE holds before its tryInitRaw: longer than the filter
TTL_MS = 3_600_000
SIZES = (0, 1, 2, 255, 256, 257, 1000, 4097, 16385)
SIZE_P = (0.05, 0.2, 0.14, 0.1, 0.1, 0.12, 0.18, 0.1, 0.01)
SEG_SIZES = (1, 2, 255, 256, 257, 1000)
PROBE = ("v", tuple(range(200)))

FAMILY = {}
for _family, _kinds in {"add": "add add_dev add_multi", "contains": "contains contains_dev contains_multi",
                        "stream": "stream", "read": "count bitcount digest export size_in_memory exists config",
                        "image": "import_bitmap",
                        "key": "try_init init_raw delete rename renamenx expire clear_expire ttl",
                        "bits": "setbit clearbit set_range set_bytes bitop_not",
                        "setup": "open close hll_init"}.items():
    for _k in _kinds.split():
        FAMILY[_k] = _family

VIAS = {"add": ("obj", "raw", "async"), "contains": ("obj", "raw", "async"), "add_dev": ("handle",),
        "contains_dev": ("handle",), "add_multi": ("multi", "multi_dev"), "contains_multi": ("multi", "multi_dev"),
        "stream": ("stream", "stream_dev"), "count": ("obj",), "bitcount": ("obj",), "digest": ("obj",),
        "export": ("obj",), "size_in_memory": ("obj",), "exists": ("obj",), "config": ("obj",),
        "import_bitmap": ("host", "dev"), "try_init": ("obj",), "init_raw": ("raw",), "delete": ("obj",),
        "rename": ("obj",), "renamenx": ("obj",), "expire": ("obj",), "clear_expire": ("obj",), "ttl": ("obj",),
        "setbit": ("bits",), "clearbit": ("bits",), "set_range": ("bits",), "set_bytes": ("bits",),
        "bitop_not": ("bits",), "open": ("handle",), "close": ("handle",)}
WEIGHTS = {"add": 17, "contains": 10, "add_dev": 8, "contains_dev": 6, "add_multi": 9, "contains_multi": 6, "stream": 7,
           "count": 2.5, "bitcount": 2.5, "digest": 3, "export": 2.5, "size_in_memory": 2.5, "exists": 2.5, "config": 2.5,
           "import_bitmap": 3.5, "try_init": 2.5, "init_raw": 2.5, "delete": 2.5, "rename": 2.5, "renamenx": 2.5,
           "expire": 2.5, "clear_expire": 2.5, "ttl": 2.5, "setbit": 2.5, "clearbit": 2.5, "set_range": 2.5,
           "set_bytes": 2.5, "bitop_not": 2.5, "open": 2.5, "close": 2.5}


def label(cmd) -> str:
    return f"{cmd[0]}:{cmd[1]}"


def crafted_last_bit_key(size=CONFIGS[REGION][0], k=CONFIGS[REGION][1], cap=400_000):
    """The first key b"last-<i>" one of whose k indexes is the last bit of a `size`-bit filter, by brute force with
    the oracle; None when the first `cap` candidates hold none (about k * cap / size are expected to)."""
    for base in range(0, cap, 20_000):
        keys = [b"last-%d" % i for i in range(base, base + 20_000)]
        hit = np.flatnonzero((M.indexes(size, k, keys) == size - 1).any(axis=1))
        if len(hit):
            return keys[int(hit[0])]
    return None


# ---- the generator ----------------------------------------------------------------------------------------------
def commands(seed: int, steps: int):
    """`steps` command tuples, a pure function of the seed.  It steps a model of its own to know the filters' state."""
    rng = np.random.default_rng([0xB10F, seed])
    ks = BloomKeyspace()
    state = {"prev": None, "serial": 0, "short": [], "exports": {}}
    pending = []

    def integer(lo, hi):
        return int(rng.integers(lo, hi, endpoint=True))

    def choice(seq):
        return seq[int(rng.integers(len(seq)))]

    def chance(p):
        return rng.random() < p

    def pick_key(pool=FILTERS):
        if state["prev"] in pool and chance(0.5):
            return state["prev"]
        return choice(pool)

    def batch(n, pool=None):
        """n keys drawn with replacement, half the time from a window of 600: repeats within and across batches"""
        pool = pool or choice(("v", "v", "v", "s16", "s16", "s32"))
        ids = rng.integers(0, 600 if chance(0.5) else M.POOLS[pool], size=n).tolist()
        if n >= 2 and chance(0.4):
            ids[-1] = ids[0]  # a duplicate, last: it is not new whatever the first was
        return (pool, tuple(ids))

    def size():
        return SIZES[int(rng.choice(len(SIZES), p=SIZE_P))]

    def layout(spec):
        return choice(("offsets", "odd offsets", "stream2") if spec[0] == "v" else
                      ("stride", "offsets", "odd stride", "stream2"))

    def current(hid):
        return hid in ks.handles and ks.handle_is_current(hid)

    def handle_for(key, any_state=False):
        """a handle of `key`: mostly the long-lived one, else a short-lived one that is open on it"""
        short = [h for h in state["short"] if ks.handles[h][0] == key and (any_state or current(h))]
        if short and chance(0.3):
            return choice(short)
        return LONG_LIVED.get(key, HLL_HANDLE)

    def new_hid():
        state["serial"] += 1
        return 100 + state["serial"]

    def by_name(kind, via, key):
        cached = None
        if via != "obj" and chance(0.5):
            cached = ks.cfg.get(key)
            if key == REINIT and chance(0.2):
                cached = OTHER_CONFIG if cached == CONFIGS[REINIT] else CONFIGS[REINIT]  # the caller's is stale
        n = size()
        if n == 16385 and key == K40:
            n = 4097
        more = ()
        if via == "async":
            more = tuple((choice(("add", "contains")), choice((key, key, pick_key())), batch(choice((1, 2, 257))),
                          chance(0.5), None) for _ in range(integer(1, 2)))
        return (kind, via, key, batch(n), chance(0.6), cached, more)

    def multi(kind, via):
        usable = [k for k in FILTERS if current(LONG_LIVED[k])]
        nseg = integer(2, 9)
        r = rng.random()
        if r < 0.35 and len(usable) >= 2:  # all distinct: the per-segment kernel
            names = [usable[int(i)] for i in rng.permutation(len(usable))[:min(nseg, len(usable))]]
        else:  # a tenant repeated
            names = [choice(usable or [SMALL]) for _ in range(nseg)]
            names[-1] = names[0]
        if MISSING in usable and MISSING not in ks.data and chance(0.5):
            names[integer(0, len(names) - 1)] = MISSING
        hids = [handle_for(k) for k in names]
        if chance(0.04):
            hids[integer(0, len(hids) - 1)] = HLL_HANDLE if chance(0.5) else LONG_LIVED[choice(FILTERS)]  # WRONGTYPE, or
        sizes = [choice(SEG_SIZES) for _ in hids]                                   # whatever state that handle is in
        if chance(0.08):
            sizes[integer(0, len(sizes) - 1)] = choice((4097, 16385))
        empty = integer(0, len(sizes) - 1)
        if via == "multi" and chance(0.05):
            sizes[empty] = 0  # the host form: / by zero
        elif via == "multi_dev" and chance(0.3) and ks.handles[hids[empty]][0] in ks.data:
            sizes[empty] = 0  # the device form runs it as nothing (on a filter that has its string: see above)
        segs = tuple((h, batch(n)) for h, n in zip(hids, sizes))
        cmd = (kind, via, ks.handles[hids[0]][0], segs, chance(0.7))
        r = rng.random()
        other = "contains_multi" if kind == "add_multi" else "add_multi"
        if r < 0.3:  # the same handle list at once again, add and contains swapped
            pending.append((other, choice(VIAS[other]), cmd[2], tuple((h, batch(max(len(s[1]), 1))) for h, s in segs),
                            chance(0.7)))
        elif r < 0.45:  # the same list permuted
            order = rng.permutation(len(segs))
            pending.append((kind, via, ks.handles[segs[int(order[0])][0]][0], tuple(segs[int(i)] for i in order), True))
        return cmd

    def stream(kind, via):
        pool = [k for k in FILTERS if k != K40 and current(LONG_LIVED[k])]
        names = [pool[int(i)] for i in rng.permutation(len(pool))[:integer(1, 5)]] or [SMALL]
        if chance(0.06):
            names[-1] = K40  # refused: k <= 32
        hids = tuple(handle_for(k) for k in names)
        n = choice((8, 8, 255, 256, 257, 1000))
        spec = batch(n, choice(("v", "s16")))
        ids = list(spec[1])
        window = ids[:max(3, n // 8)]
        ids = [choice(window) if chance(0.5) else i for i in ids]
        kf = rng.integers(0, len(names), size=n).tolist()
        ops = (rng.random(n) < 0.5).astype(int).tolist()
        at = sorted(rng.choice(n, size=3, replace=False).tolist())  # contains, add, contains of one key on one filter
        for a, op in zip(at, (0, 1, 0)):
            ids[a], kf[a], ops[a] = ids[at[0]], kf[at[0]], op
        if via == "stream_dev":  # the device form gives every filter a string: an add for those that have none
            free = [i for i in range(n) if i not in at]
            for f, name in enumerate(names):
                if name not in ks.data and not any(o and g == f for g, o in zip(kf, ops)):
                    i = free.pop(int(rng.integers(len(free))))
                    kf[i], ops[i] = f, 1
        return (kind, via, names[0], hids, tuple(kf), tuple(ops), (spec[0], tuple(ids)))

    def image(key):
        r = rng.random()
        have = ks.data.get(key) or b""
        nbytes = (ks.cfg.get(key, (64, 1))[0] + 7) // 8
        if r < 0.25 and state["exports"].get(key) is not None:
            return state["exports"][key]  # its own earlier export
        if r < 0.5:
            return ks.data.get(choice([k for k in FILTERS if k != BIG])) or b"\x01"  # another filter's
        if r < 0.7 and len(have) > 1:
            return rng.bytes(integer(1, len(have) - 1))  # shorter than the string
        if r < 0.9:
            return rng.bytes(min(nbytes, 9000) + integer(1, 300))  # longer than the filter
        return b""

    def recreate(key, cfg=None):
        return [("delete", "obj", key) if chance(0.7) else ("expire", "obj", key, "past"),
                ("init_raw", "raw", key, *(cfg or CONFIGS[key]))]

    def build(kind):
        via = choice(VIAS[kind])
        if kind in ("add", "contains"):
            key = HLL if chance(0.03) else pick_key()
            return by_name(kind, via, key)
        if kind in ("add_dev", "contains_dev"):
            key = pick_key()
            hid = handle_for(key, any_state=True)
            spec = batch(choice((0, 1, 1, 2, 255, 256, 257, 1000, 1000, 4097)))
            return (kind, via, key, hid, spec, chance(0.7), layout(spec))
        if kind in ("add_multi", "contains_multi"):
            return multi(kind, via)
        if kind == "stream":
            return stream(kind, via)
        if kind in ("count", "bitcount", "digest", "export", "size_in_memory", "exists", "config"):
            key = pick_key(CHECKED) if kind != "digest" or chance(0.2) else pick_key()
            if kind == "digest" and chance(0.5):
                pending.append(("contains", "obj", key, batch(2), True, None, ()))  # no write in between: the same
                pending.append(("digest", "obj", key))
            return (kind, via, key)
        if kind == "import_bitmap":
            key = pick_key(FILTERS[:3] + FILTERS[4:])
            if chance(0.5):
                pending.append(("contains_dev", "handle", key, LONG_LIVED[key], batch(257), True, "offsets"))
            return (kind, via, key, image(key))
        if kind == "try_init":
            return (kind, via, pick_key(), 1000, 0.03)
        if kind == "init_raw":
            return (kind, via, pick_key(), 977, 4)
        if kind == "delete":
            key = pick_key((TINY, SMALL, REINIT, MISSING, K17))
            pending.extend(recreate(key)[1:])
            if key != MISSING:
                pending.append(("add_dev", "handle", key, LONG_LIVED[key], batch(choice((1, 2, 257))), True, "offsets"))
            return (kind, via, key)
        if kind in ("rename", "renamenx"):
            key = pick_key((SMALL, REGION, K17, LATE, TINY))
            if kind == "renamenx" and chance(0.4):
                return (kind, via, key, choice([k for k in FILTERS if k in ks.data and k != key] or [SPARE]))
            if key not in ks.data and kind == "renamenx":
                return (kind, via, key, SPARE)  # no such key
            hid, back = new_hid(), choice(("rename", "renamenx"))
            pending.extend([("contains_dev", "handle", key, LONG_LIVED[key], batch(2), True, "offsets"),  # no config now
                            ("open", "handle", SPARE, hid),
                            ("add_dev", "handle", SPARE, hid, batch(choice((1, 257))), True, "offsets"),
                            (back, "obj", SPARE, key),
                            ("contains_dev", "handle", key, LONG_LIVED[key], batch(257), True, "offsets"),
                            ("close", "handle", SPARE, hid)])
            return (kind, via, key, SPARE)
        if kind == "expire":
            if chance(0.25):
                key = pick_key((TINY, SMALL, REINIT))
                pending.extend(recreate(key)[1:])
                return (kind, via, key, "past")
            return (kind, via, pick_key(CHECKED), "hour")
        if kind in ("clear_expire", "ttl"):
            return (kind, via, pick_key(CHECKED))
        if kind == "setbit":
            key = pick_key()
            return (kind, via, key, integer(0, ks.cfg.get(key, (64, 1))[0] + 20), 1)
        if kind == "clearbit":
            key = pick_key()
            return (kind, via, key, integer(0, ks.cfg.get(key, (64, 1))[0] - 1))
        if kind == "set_range":
            key = pick_key(FILTERS[:3] + FILTERS[4:])
            top = ks.cfg.get(key, (64, 1))[0]
            return (kind, via, key, top - integer(1, 9), top + integer(1, 70))  # past the filter's size
        if kind == "set_bytes":
            return (kind, via, pick_key(FILTERS[:3] + FILTERS[4:]), integer(1, 2000), integer(0, 1 << 30))
        if kind == "bitop_not":
            key = pick_key(FILTERS[:3] + FILTERS[4:])
            return (kind, via, key, key)
        if kind == "open":
            key = HLL if chance(0.1) else pick_key()
            if len(state["short"]) >= 4:
                pending.append(("close", "handle", ks.handles[state["short"][0]][0], state["short"][0]))
            return (kind, via, key, new_hid())
        if kind == "close":
            if not state["short"]:
                return ("open", "handle", pick_key(), new_hid())
            hid = choice(state["short"])
            return (kind, via, ks.handles[hid][0], hid)
        raise AssertionError(kind)

    def step(cmd):
        kind, key = cmd[0], cmd[2]
        if kind == "export":
            state["exports"][key] = ks.data.get(key)
        reply, err = getattr(ks, kind)(*cmd[1:])
        if kind == "open" and err is None and cmd[3] >= 100:
            state["short"].append(cmd[3])
        if kind == "close":
            state["short"].remove(cmd[3])
        state["prev"] = key
        return cmd

    def tiny_block():
        """TINY anew, filled until one to three bits are zero; then two different keys whose only zero bit is the
        same one, a duplicate behind them; then keys that are all present; each on a path of its own"""
        size_, k = CONFIGS[TINY]
        idx = M.indexes(size_, k, M.VAR[:600])
        bits, ids = np.zeros(size_, bool), []
        for i in rng.permutation(600).tolist():
            after = bits.copy()
            after[idx[i]] = True
            if (~after).sum() >= 1:
                bits = after
                ids.append(i)
            if (~bits).sum() <= 3:
                break
        target = int(np.flatnonzero(~bits)[0])
        zero = ~bits[idx.astype(np.int64)]
        pair = [i for i in range(600) if zero[i].any() and set(idx[i][zero[i]].tolist()) == {target}][:2]
        hid = LONG_LIVED[TINY]
        fill, shared, present = ("v", tuple(ids)), ("v", tuple(pair + pair[:1])), ("v", tuple(ids[:5] + ids[:1]))
        forms = [lambda s: ("add", "obj", TINY, s, True, None, ()), lambda s: ("add", "raw", TINY, s, True, CONFIGS[TINY], ()),
                 lambda s: ("add_dev", "handle", TINY, hid, s, True, "offsets"),
                 lambda s: ("add_multi", choice(VIAS["add_multi"]), TINY, ((hid, s), (LONG_LIVED[SMALL], batch(2))), True),
                 lambda s: ("stream", choice(VIAS["stream"]), TINY, (hid,), (0,) * len(s[1]), (1,) * len(s[1]), s)]
        return recreate(TINY) + [choice(forms[:3])(fill)] + ([choice(forms)(shared)] if len(pair) == 2 else []) + \
            [choice(forms[:4])(present), ("contains_dev", "handle", TINY, hid, shared, True, "offsets")]

    def reinit_block():
        """the same handle list before and after a tenant was deleted and re-created with its config; then another
        config, under which the old handle must fail; then back"""
        hid, via = LONG_LIVED[REINIT], choice(VIAS["add_multi"])
        segs = lambda: ((hid, batch(choice((2, 257)))), (LONG_LIVED[SMALL], batch(2)), (LONG_LIVED[REGION], batch(257)))
        new = new_hid()
        return recreate(REINIT) + [("add_multi", via, REINIT, segs(), True)] + recreate(REINIT) + \
            [("add_multi", via, REINIT, segs(), True), ("contains_multi", via, REINIT, segs(), True)] + \
            recreate(REINIT, OTHER_CONFIG) + \
            [("add_dev", "handle", REINIT, hid, batch(257), True, "offsets"),
             ("open", "handle", REINIT, new), ("add_dev", "handle", REINIT, new, batch(1000), True, "offsets"),
             ("count", "obj", REINIT),
             ("add", "raw", REINIT, batch(2), True, CONFIGS[REINIT], ()), ("close", "handle", REINIT, new)] + \
            recreate(REINIT) + [("contains_dev", "handle", REINIT, hid, batch(257), True, "offsets")]

    def missing_block():
        """a contains_multi that reads the filter without a string, then at once an add_multi on the same handles"""
        hids = (LONG_LIVED[SMALL], LONG_LIVED[MISSING], LONG_LIVED[TINY])
        via = choice(VIAS["add_multi"])
        segs = lambda: tuple((h, batch(choice((2, 257)))) for h in hids)
        return recreate(MISSING) + [("contains_dev", "handle", MISSING, hids[1], batch(257), True, "offsets"),
                                   ("contains", "obj", MISSING, batch(257), True, None, ()), ("ttl", "obj", MISSING),
                                   ("contains_multi", via, SMALL, segs(), True), ("add_multi", via, SMALL, segs(), True),
                                   ("contains_multi", via, SMALL, segs(), True)]

    def image_block():
        key = choice((REGION, K17, LATE))
        return [("export", "obj", key), ("add", "obj", key, batch(257), True, None, ()), "own export",
                ("contains_dev", "handle", key, LONG_LIVED[key], batch(257), True, "offsets")]

    kinds = list(WEIGHTS)
    p = np.array([WEIGHTS[k] for k in kinds], float)
    p /= p.sum()
    script = {0: [("init_raw", "raw", HLL, *CONFIGS[HLL]), ("open", "handle", HLL, HLL_HANDLE), ("hll_init", "obj", HLL),
                  ("setbit", "bits", LATE, LATE_BIT, 1), ("setbit", "bits", LATE, 5, 1)]
              + [("init_raw", "raw", k, *CONFIGS[k]) for k in FILTERS]
              + [("open", "handle", k, LONG_LIVED[k]) for k in FILTERS]}  # all but LATE's: before the first SETBIT
    for at in range(22, steps, 95):
        script[at] = "tiny"
        script[at + 18] = "reinit"
        script[at + 45] = "image"
        script[at + 60] = "missing"
    for done in range(steps):
        block = script.get(done, [])
        if isinstance(block, str):
            block = {"tiny": tiny_block, "reinit": reinit_block, "image": image_block, "missing": missing_block}[block]()
        pending += block
        if pending and pending[0] == "own export":
            key = pending[1][2]
            pending[0] = ("import_bitmap", choice(VIAS["import_bitmap"]), key, state["exports"].get(key) or b"\x80")
        cmd = pending.pop(0) if pending else build(kinds[int(rng.choice(len(kinds), p=p))])
        yield step(cmd)


# ---- what a sequence covers (test_bloom_sequences_cpu.py asserts on it) ------------------------------------------
def stats(seed: int, steps: int) -> dict:
    ks = BloomKeyspace()
    out = {"kinds": {}, "after_other_family": set(), "errors": 0, "n": 0, "recreated": 0, "duplicate": 0,
           "all present": 0, "lengthens, last key not new": 0, "shared zero bit": 0, "repeated tenant": 0,
           "stream add then contains": 0, "missing read then written": 0, "list again after a re-creation": 0,
           "handle call after": set(), "old handle refused": 0}
    prev, prev_multi = None, None
    deleted, after, mismatched, lists = set(), {}, set(), {}
    for at, cmd in enumerate(commands(seed, steps)):
        kind, key = cmd[0], cmd[2]
        ks.events = []
        existed = key in ks.cfg
        _reply, err = getattr(ks, kind)(*cmd[1:])
        out["n"] += 1
        out["errors"] += err is not None
        out["kinds"][label(cmd)] = out["kinds"].get(label(cmd), 0) + 1
        if prev is not None and prev[2] == key and FAMILY[prev[0]] != FAMILY[kind]:
            out["after_other_family"].add(kind)
        if kind in ("delete", "expire") and existed and key not in ks.cfg:
            deleted.add(key)
            after.setdefault(key, set()).add("delete")
        this_multi = None
        for ev in ks.events:
            if ev[0] == "created" and ev[1] in deleted:
                deleted.discard(ev[1])
                out["recreated"] += 1
                after.setdefault(ev[1], set()).add("re-init")
                for hids in lists:
                    if ev[1] in lists[hids]:
                        lists[hids][ev[1]] = True
                if any(h[0] == ev[1] and h[1:] != ev[2] for h in ks.handles.values()):
                    mismatched.add(ev[1])
            elif ev[0] == "renamed":
                after.setdefault(ev[2], set()).add("rename")
            elif ev[0] == "imported":
                after.setdefault(ev[1], set()).add("import")
            elif ev[0] == "handle call":
                if err is None:
                    out["handle call after"] |= after.pop(ev[1], set())
                elif err == CONFIG and ev[1] in mismatched and ev[1] in ks.cfg:
                    out["old handle refused"] += 1
                    mismatched.discard(ev[1])
            elif ev[0] == "multi":
                _e, is_add, hids, names, missing = ev
                this_multi = (is_add, hids, missing)
                if err is None:
                    out["list again after a re-creation"] += any(lists.get(hids, {}).values())
                    lists[hids] = {n: False for n in names}
                if (is_add and err is None and prev_multi is not None and not prev_multi[0] and prev_multi[1] == hids
                        and prev_multi[2]):
                    out["missing read then written"] += 1
            elif ev[0] in out:
                out[ev[0]] += 1
        prev_multi = this_multi if err is None else None
        prev = cmd
    return out


# ---- the full check -------------------------------------------------------------------------------------------
def probes(model: BloomKeyspace):
    out = []
    for key in CHECKED:
        out += [("export", "obj", key), ("exists", "obj", key), ("config", "obj", key), ("ttl", "obj", key),
                ("count", "obj", key), ("contains", "obj", key, PROBE, True, None, ())]
        if key in LONG_LIVED and LONG_LIVED[key] in model.handles:
            out.append(("contains_dev", "handle", key, LONG_LIVED[key], PROBE, True, "offsets"))
    hids = [LONG_LIVED[k] for k in FILTERS if LONG_LIVED[k] in model.handles and model.handle_is_current(LONG_LIVED[k])]
    if hids:  # one call over every filter whose handle still holds (the others answered an error above)
        out.append(("contains_multi", "multi", model.handles[hids[0]][0], tuple((h, PROBE) for h in hids), True))
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


def plain(x):
    """tuples as lists, all the way down: replies compare by value"""
    return [plain(v) for v in x] if isinstance(x, (tuple, list)) else x


def call(engine, cmd):
    reply, err = getattr(engine, cmd[0])(*cmd[1:])
    return plain(reply), err


def run(engine, seed: int, steps: int, check_every: int = 10, stop_at=None) -> None:
    """The sequence of `seed` through `engine` and the model: every reply and error kind equal, and the full check
    every `check_every` commands and at the end.  stop_at = run only the first stop_at commands."""
    model = BloomKeyspace()
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
class ModelEngine(BloomKeyspace):
    """a second model: the generator, the model and the checker agree with themselves"""


DEFECTS = {
    "a": "a duplicate key in a batch replies new twice",
    "b": "two keys that share their only zero bit both reply new",
    "c": "the second segment of a repeated tenant replies against the bits from before the call",
    "d": "a stream contains after an add of the same key in the same call reads the old bits",
    "e": "an add whose last key is not new does not lengthen the string",
    "f": "a contains lengthens the string",
    "g": "a contains on a missing bitmap creates the key",
    "h": "the long-lived handle keeps the deleted filter's bits after a re-creation",
    "i": "a multi call after a tenant's re-creation uses the tenant's old bits",
    "j": "rename leaves the config under the old name",
    "k": "import keeps the previous string's tail",
    "l": "count() uses the previous config after a re-init",
    "m": "a handle whose config no longer matches writes anyway",
}


class FaultyModelEngine(BloomKeyspace):
    """The model with one wrong answer, `defect` in DEFECTS."""

    def __init__(self, defect: str):
        super().__init__()
        assert defect in DEFECTS
        self.defect = defect
        self.left = {}      # (h, i) the string a deleted filter had
        self.old_cfg = {}   # (l) the config a deleted filter had

    def _add_flags(self, keys, was, first, k):
        flags = super()._add_flags(keys, was, first, k)
        if self.defect in "ab":
            alone = ~was.reshape(-1, k).all(axis=1)  # each key against the string alone
            seen = set()
            for i, key in enumerate(keys):
                again = key in seen
                seen.add(key)
                if again == (self.defect == "a"):
                    flags[i] = alone[i]
        return flags

    def _multi_add(self, name, size, k, keys, again):
        if self.defect == "c" and again:
            before = self._before_call.get(name)
            flags = super()._multi_add(name, size, k, keys, again)
            idx = M.indexes(size, k, keys).reshape(-1)
            was = M.SM.RedisString(before).get_indexes(idx)
            _u, first = np.unique(idx, return_index=True)
            return BloomKeyspace._add_flags(self, keys, was, first, k)
        return super()._multi_add(name, size, k, keys, again)

    def _segments(self, via, segs, is_add):
        self._before_call = dict(self.data)
        return super()._segments(via, segs, is_add)

    def _stream_view(self, now, before, name, added_before):
        return before[name] if self.defect == "d" and added_before else now[name]

    def _lengthens(self, flags):
        return self.defect != "e" or bool(flags[-1])

    def _contains_side_effect(self, key, idx):
        if self.defect == "f" and key in self.data:
            self.data[key] += bytes(max(0, (int(idx.max()) >> 3) + 1 - len(self.data[key])))
        if self.defect == "g" and key not in self.data and key not in self.hll:
            self.data[key] = b""

    def _deleted(self, key):
        if key in self.data:
            self.left[key] = self.data[key]
        if key in self.cfg:
            self.old_cfg[key] = self.cfg[key]

    def _read_view(self, key, how):
        if (self.defect, how) in (("h", "handle"), ("i", "multi")) and key in self.left and key in self.cfg:
            return self.left[key]
        return super()._read_view(key, how)

    def _rename_config(self, key, new):
        cfg, exp = self.cfg[key], self.expected[key]
        super()._rename_config(key, new)
        if self.defect == "j":
            self.cfg[key], self.expected[key] = cfg, exp

    def _imported(self, key, data):
        old = self.data.get(key, b"")
        return data + old[len(data):] if self.defect == "k" else data

    def _count_config(self, key):
        return self.old_cfg.get(key, self.cfg[key]) if self.defect == "l" else self.cfg[key]

    def _mismatch_writes(self, name, size, k, keys):
        if self.defect == "m":
            s = M.SM.RedisString(self.data.get(name))
            s.set_indexes(M.indexes(size, k, keys).reshape(-1), 1)
            self.data[name] = s.bytes()


class GpuEngine:
    """The commands through librbx.so.  Names are `prefix + key`; engine exceptions become the model's error kinds.
    Handles live from their `open` command to their `close`, the long-lived ones to shutdown()."""

    def __init__(self, client, prefix: str):
        self.client, self.prefix = client, prefix
        self.handles = {}
        self.digests = {}
        self.side = None

    def shutdown(self):
        for h in self.handles.values():
            h.close()
        self.handles = {}
        for key in CHECKED:
            self._f(key).delete()
        self._f(HLL).delete()

    # ---- plumbing --------------------------------------------------------------------------------------------
    def _name(self, key) -> str:
        return self.prefix + key

    def _f(self, key):
        return self.client.getBloomFilter(self._name(key))

    def _bs(self, key):
        return self.client.getBitSet(self._name(key))

    @staticmethod
    def _arena(spec):
        from redisson_amd import Arena

        mat = M.matrix_of(spec)
        return Arena(M.keys_of(spec)) if mat is None or not len(mat) else Arena.fixed(mat)

    def _stream(self, layout):
        """None (the context's stream) or a second torch stream's"""
        import torch

        if "stream2" not in (layout or ""):
            return None
        if self.side is None:
            self.side = torch.cuda.Stream()
        return self.side.cuda_stream

    def _device_keys(self, spec, layout):
        """(rbx_keys over device memory, the tensors that hold it)"""
        import torch

        from redisson_amd import device_keys

        odd = "odd" in layout
        mat = M.matrix_of(spec)
        n = len(spec[1])
        if mat is not None and n and "offsets" not in layout:
            flat = np.concatenate([np.zeros(int(odd), np.uint8), mat.reshape(-1)])
            d = torch.from_numpy(flat).cuda()
            return device_keys(d.data_ptr() + int(odd), n, mat.shape[1]), (d,)
        buf, offs = O.arena(M.keys_of(spec))
        d = torch.from_numpy(np.concatenate([np.zeros(int(odd), np.uint8), buf])).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        return device_keys(d.data_ptr() + int(odd), n, 0, d_offs.data_ptr()), (d, d_offs)

    def _wait(self):
        import torch

        self.client.synchronize()
        torch.cuda.synchronize()

    @staticmethod
    def _check(rc):
        from redisson_amd.client import _check

        _check(rc)

    # ---- by name -----------------------------------------------------------------------------------------------
    def _raw_call(self, op, key, spec, per_key, cached, submit=None):
        from redisson_amd import _lib as L

        a = self._arena(spec)
        out = np.full(max(a.n, 1), 77, np.uint8) if per_key else None
        cnt = C.c_uint64(0)
        size, k = cached or (0, 0)
        head = (self.client.ctx, self._name(key).encode(), size, k, a.ptr())
        done = lambda: [int(cnt.value), out[:a.n].astype(int).tolist() if per_key else None]
        if submit is None:
            self._check(getattr(L.lib(), f"rbx_bloom_{op}")(*head, out.ctypes.data_as(L.u8p) if per_key else None,
                                                            C.byref(cnt)))
            return done()
        fut = C.c_void_p()
        self._check(getattr(L.lib(), f"rbx_bloom_{op}_async")(*head, out.ctypes.data if per_key else None, C.byref(cnt),
                                                              None, None, C.byref(fut)))
        submit.append((fut, done, (a, out, cnt)))

    def _obj(self, op, key, spec, per_key):
        f = self._f(key)
        if per_key:
            count, flags = (f.addEach if op == "add" else f.containsEach)(self._arena(spec))
            return [count, flags.astype(int).tolist()]
        keys = M.keys_of(spec)
        fn = f.add if op == "add" else f.contains
        return [int(fn(keys[0])) if len(keys) == 1 else fn(keys), None]  # a single object, or a collection

    def _by_name(self, op, via, key, spec, per_key, cached, more):
        from redisson_amd import _lib as L

        if via == "obj":
            return self._obj(op, key, spec, per_key)
        if via == "raw":
            return self._raw_call(op, key, spec, per_key, cached)
        queued = []
        for o, k, s, p, c in ((op, key, spec, per_key, cached),) + tuple(more):  # all queued before any is waited for
            self._raw_call(o, k, s, p, c, queued)
        results = []
        for fut, done, _keep in queued:
            rc = C.c_int(-99)
            self._check(L.lib().rbx_future_wait(fut, 120_000, C.byref(rc)))
            L.lib().rbx_future_free(fut)
            results.append([done(), None] if rc.value == 0 else [None, _KIND_OF_CODE()[rc.value]])
        if results[0][1] is not None:
            raise _Kind(results[0][1], results[1:] if more else None)
        return [results[0][0], results[1:]] if more else results[0][0]

    def add(self, via, key, spec, per_key, cached=None, more=()):
        return self._by_name("add", via, key, spec, per_key, cached, more)

    def contains(self, via, key, spec, per_key, cached=None, more=()):
        return self._by_name("contains", via, key, spec, per_key, cached, more)

    # ---- handles -------------------------------------------------------------------------------------------------
    def open(self, via, key, hid):
        from redisson_amd import BloomHandle

        h = BloomHandle(self.client, self._name(key))
        self.handles[hid] = h
        return [h.size, h.k]

    def close(self, via, key, hid):
        self.handles.pop(hid).close()

    def _dev(self, op, hid, spec, per_key, layout):
        import torch

        keys, _keep = self._device_keys(spec, layout)
        n = len(spec[1])
        out = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda") if per_key else None
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h = self.handles[hid]
        (h.add_dev if op == "add" else h.contains_dev)(keys, cnt.data_ptr(), out.data_ptr() if per_key else None,
                                                       self._stream(layout))
        self._wait()
        return [int(cnt.item()), out.cpu().numpy()[:n].astype(int).tolist() if per_key else None]

    def add_dev(self, via, key, hid, spec, per_key, layout="offsets"):
        return self._dev("add", hid, spec, per_key, layout)

    def contains_dev(self, via, key, hid, spec, per_key, layout="offsets"):
        return self._dev("contains", hid, spec, per_key, layout)

    # ---- many filters in one call ---------------------------------------------------------------------------------
    def _multi(self, op, via, segs, per_key):
        import torch

        from redisson_amd import Arena, bloom_add_multi, bloom_contains_multi
        from redisson_amd import _lib as L
        from redisson_amd.client import _handles

        handles = [self.handles[h] for h, _ in segs]
        parts = [M.keys_of(spec) for _h, spec in segs]
        keys = [k for part in parts for k in part]
        seg = np.zeros(len(segs) + 1, np.uint64)
        seg[1:] = np.cumsum([len(part) for part in parts])
        same = {len(k) for k in keys}
        fixed = len(same) == 1 and same != {0}
        if via == "multi":
            arena = Arena.fixed(np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), -1)) if fixed else Arena(keys)
            r = (bloom_add_multi if op == "add" else bloom_contains_multi)(self.client, handles, seg, arena, per_key)
            counts, flags = r if per_key else (r, None)
            return [[int(c) for c in counts], flags.astype(int).tolist() if per_key else None]
        d_keys, _keep = self._lit_device_keys(keys, fixed)
        n = len(keys)
        d_seg = torch.from_numpy(seg.view(np.int64)).cuda()
        out = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda") if per_key else None
        cnt = torch.zeros(len(segs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        fn = L.lib().rbx_bloom_add_multi_dev if op == "add" else L.lib().rbx_bloom_contains_multi_dev
        self._check(fn(self.client.ctx, _handles(handles), len(segs), d_seg.data_ptr(), C.byref(d_keys),
                       out.data_ptr() if per_key else None, cnt.data_ptr(), None))
        self._wait()
        return [cnt.cpu().numpy().astype(int).tolist(), out.cpu().numpy()[:n].astype(int).tolist() if per_key else None]

    def _lit_device_keys(self, keys, fixed):
        import torch

        from redisson_amd import device_keys

        if fixed:
            d = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
            return device_keys(d.data_ptr(), len(keys), len(keys[0])), (d,)
        buf, offs = O.arena(keys)
        d, d_offs = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
        return device_keys(d.data_ptr(), len(keys), 0, d_offs.data_ptr()), (d, d_offs)

    def add_multi(self, via, key, segs, per_key):
        return self._multi("add", via, segs, per_key)

    def contains_multi(self, via, key, segs, per_key):
        return self._multi("contains", via, segs, per_key)

    def stream(self, via, key, hids, kf, ops, spec):
        import torch

        from redisson_amd import bloom_stream
        from redisson_amd import _lib as L
        from redisson_amd.client import _handles

        handles = [self.handles[h] for h in hids]
        n = len(kf)
        if via == "stream":
            out, counts = bloom_stream(self.client, handles, np.asarray(kf, np.uint32), np.asarray(ops, np.uint8),
                                       self._arena(spec))
            return [out.astype(int).tolist(), [int(c) for c in counts]]
        d_keys, _keep = self._device_keys(spec, "stride" if spec[0] != "v" else "offsets")
        d_kf = torch.from_numpy(np.asarray(kf, np.uint32).view(np.int32)).cuda()
        d_op = torch.from_numpy(np.asarray(ops, np.uint8)).cuda()
        out = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self._check(L.lib().rbx_bloom_stream_dev(self.client.ctx, _handles(handles), len(handles), d_kf.data_ptr(),
                                                 d_op.data_ptr(), C.byref(d_keys), out.data_ptr(), cnt.data_ptr(), None))
        self._wait()
        return [out.cpu().numpy()[:n].astype(int).tolist(), cnt.cpu().numpy().astype(int).tolist()]

    # ---- the string as a whole, the config, the keys ---------------------------------------------------------------
    def count(self, via, key):
        return self._f(key).count()

    def bitcount(self, via, key):
        return self._f(key).bitcount()

    def digest(self, via, key):
        now = self._f(key).digest()
        reply = "first" if key not in self.digests else "same" if self.digests[key] == now else "changed"
        self.digests[key] = now
        return reply

    def export(self, via, key):
        return self._f(key).exportBitmap()

    def import_bitmap(self, via, key, data):
        import torch

        from redisson_amd import _lib as L

        if via == "host":
            return self._f(key).importBitmap(data)
        d = torch.from_numpy(np.frombuffer(data or b"\0", np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        self._check(L.lib().rbx_bloom_import_dev(self.client.ctx, self._name(key).encode(), d.data_ptr(), len(data), None))

    def size_in_memory(self, via, key):
        return self._f(key).sizeInMemory() != 0

    def exists(self, via, key):
        return self._f(key).isExists()

    def config(self, via, key):
        f = self._f(key)
        return [f.getSize(), f.getHashIterations(), f.getExpectedInsertions()]

    def try_init(self, via, key, n, p):
        return self._f(key).tryInit(n, p)

    def init_raw(self, via, key, size, k):
        return self._f(key).tryInitRaw(size, k)

    def delete(self, via, key):
        return self._f(key).delete()

    def rename(self, via, key, new):
        self._f(key).rename(self._name(new))

    def renamenx(self, via, key, new):
        return self._f(key).renamenx(self._name(new))

    def expire(self, via, key, when):
        return self._f(key).expireAt(1) if when == "past" else self._f(key).expire(TTL_MS)

    def clear_expire(self, via, key):
        return self._f(key).clearExpire()

    def ttl(self, via, key):
        t = self._f(key).remainTimeToLive()
        return "missing" if t == -2 else "none" if t == -1 else "set" if 0 < t <= TTL_MS else f"a time to live of {t}"

    # ---- RBitSet on a filter's name, and the other type ------------------------------------------------------------------
    def setbit(self, via, key, i, value):
        return self._bs(key).set(i, bool(value))

    def clearbit(self, via, key, i):
        return self._bs(key).clearBit(i)

    def set_range(self, via, key, frm, to):
        self._bs(key).setRange(frm, to)

    def set_bytes(self, via, key, nbytes, seed):
        self._bs(key).setBytes(np.random.default_rng(seed).bytes(nbytes))

    def bitop_not(self, via, dest, src):
        assert src == dest
        self._bs(dest).not_()

    def hll_init(self, via, key):
        assert self.client.getHyperLogLog(self._name(key)).addAll([b"one", b"two"])


class _Kind(Exception):
    """an async call's error kind (its message stays on the executor's thread), with the replies queued behind it"""

    def __init__(self, kind, rest):
        super().__init__(kind)
        self.kind, self.rest = kind, rest


def _KIND_OF_CODE():
    from redisson_amd import _lib as L

    return {L.RBX_E_ILLEGAL_ARGUMENT: ILLEGAL, L.RBX_E_ILLEGAL_STATE: NOT_INIT, L.RBX_E_CONFIG_CHANGED: CONFIG,
            L.RBX_E_ARITHMETIC: ARITH, L.RBX_E_WRONGTYPE: WRONGTYPE, L.RBX_E_NO_SUCH_KEY: NO_SUCH_KEY, L.RBX_E_REDIS: REDIS}


def _guarded(fn):
    """an engine exception becomes (None, the model's error kind); a device error is no reply and propagates"""
    def run(self, *args):
        from redisson_amd import ArithmeticException, IllegalArgumentException, IllegalStateException, RedisException

        try:
            return fn(self, *args), None
        except _Kind as e:
            return (None if e.rest is None else [None, e.rest]), e.kind
        except IllegalArgumentException:
            return None, ILLEGAL
        except IllegalStateException:
            return None, NOT_INIT
        except ArithmeticException:
            return None, ARITH
        except RedisException as e:
            for kind in (WRONGTYPE, NO_SUCH_KEY, CONFIG, M.BIT_OFFSET):
                if kind in str(e):
                    return None, kind
            return None, REDIS
    run.__name__ = fn.__name__
    return run


for _k in FAMILY:
    setattr(GpuEngine, _k, _guarded(getattr(GpuEngine, _k)))
