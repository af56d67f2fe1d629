"""GETRANGE / SETRANGE / APPEND / GET on device strings on the GPU: the single calls (rbx_string_getrange / _setrange /
_append / _truncate, host and device forms), the ordered stream over many keys (rbx_string_stream[_dev],
bytestream_kernels.hip), Spring Data's methods and pipeline, and RBinaryStream.  Replies, status, off, out, the return
code and its message, and behind every call each key's GET, STRLEN, existence and timeout are compared for equality
with the one-command-at-a-time model of bytestream_model.py; the stream is also held against the engine's own single
calls.  Forced tiers: bytestream_short_max = 64 and bytestream_tile = 4096 send every command of more than 64 bytes to
the tiles."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest

import bytestream_model as M
from redisson_amd import Arena, BloomHandle, RBinaryStream, RedisException, bloom_add_multi, bloom_contains_multi
from redisson_amd import _lib as L
from redisson_amd.client import _config_name
from redisson_amd.spring_data import RedissonConnection

pytestmark = pytest.mark.gpu

GETRANGE, SETRANGE, APPEND, GET = M.GETRANGE, M.SETRANGE, M.APPEND, M.GET
DEFAULTS = {"bytestream_lanes": 16, "bytestream_short_max": 4096, "bytestream_tile": 65536, "bytestream_chunk": 1 << 25,
            "bytestream_serial_max": 64}
LANES = [4, 8, 16, 32, 64]
BIG = 9 * (1 << 20) + 3  # 2,305 tiles of 4 KiB: more than the grid has workgroups
SENTINEL = 0xEE
RC = {None: L.RBX_OK, M.OFFSET: L.RBX_E_REDIS, M.TOO_BIG: L.RBX_E_REDIS, M.WRONGTYPE: L.RBX_E_WRONGTYPE,
      M.ILLEGAL: L.RBX_E_ILLEGAL_ARGUMENT}
MSG = {M.OFFSET: "ERR offset is out of range", M.WRONGTYPE: "WRONGTYPE",
       M.TOO_BIG: "ERR string exceeds maximum allowed size (proto-max-bulk-len)"}


@contextlib.contextmanager
def tuned(**knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(("bytestream_" + k).encode(), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0


def last():
    out = (C.c_uint32 * 4)()
    assert L.lib().rbx_bench_bytestream_last(out) == 0
    return list(out)  # commands finished by lane groups, long commands, tiles, rounds


# ---- the engine's keys ---------------------------------------------------------------------------------------------------
def put(client, key, data):
    nm, _keep = L.name_struct(key)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    assert L.lib().rbx_bitset_import_n(client.ctx, nm, buf if data else None, len(data)) == 0


def export(client, key):
    nm, _keep = L.name_struct(key)
    n = C.c_uint64()
    assert L.lib().rbx_bitset_export_n(client.ctx, nm, None, 0, C.byref(n)) == 0
    buf = np.zeros(max(n.value, 1), np.uint8)
    assert L.lib().rbx_bitset_export_n(client.ctx, nm, buf.ctypes.data_as(L.u8p), n.value, C.byref(n)) == 0
    return buf[:n.value].tobytes()


def exists(client, key):
    arr, _keep = L.names_array([key])
    n = C.c_int()
    assert L.lib().rbx_exists_n(client.ctx, arr, 1, C.byref(n)) == 0
    return n.value > 0


def ttl(client, key):
    out = C.c_int64()
    assert L.lib().rbx_pttl(client.ctx, key.encode() if isinstance(key, str) else key, C.byref(out)) == 0
    return "missing" if out.value == -2 else "none" if out.value == -1 else "set"


def memory(client, key):
    """the bytes the key's allocation takes (rbx_memory_usage_n: the string's allocation plus its length word's 256)"""
    arr, _keep = L.names_array([key])
    n = C.c_uint64()
    assert L.lib().rbx_memory_usage_n(client.ctx, arr, 1, C.byref(n)) == 0
    return n.value


def expire(client, key):
    arr = (C.c_char_p * 1)(key.encode())
    r = C.c_int()
    assert L.lib().rbx_pexpire(client.ctx, arr, 1, 3_600_000, 0, 0, C.byref(r)) == 0 and r.value == 1


class Both:
    """the model and the engine side by side"""

    def __init__(self, client):
        self.client, self.ks = client, M.Strings()

    def put(self, key, data, timeout=False):
        put(self.client, key, data)
        self.ks.set(key, data)
        if timeout:
            expire(self.client, key)
            self.ks.timeout.add(key)

    def hll(self, key):
        assert self.client.getHyperLogLog(key).addAll([b"x"])
        self.ks.other.add(key)

    def same(self, keys):
        """every key's GET, STRLEN, existence and timeout"""
        for k in keys:
            if k in self.ks.other:
                continue
            want = self.ks.get(k)
            assert exists(self.client, k) == (want is not None), k
            got = export(self.client, k)
            assert got == (want or b""), (k, len(got), len(want or b""))
            assert ttl(self.client, k) == self.ks.ttl(k), k

    def stream(self, run, names, keys, cmds, vals, cap=None, replies=True, status=True):
        """one call on both; everything it returns compared.  cap None: exactly what the reads need."""
        if cap is None:
            cap = copy.deepcopy(self.ks).stream(names, keys, cmds, vals, 1 << 62)["total"] or 0
        want = self.ks.stream(names, keys, cmds, vals, cap)
        got = run(self.client, names, keys, cmds, vals, cap, replies, status)
        assert got["rc"] == RC[want["kind"]], (got["rc"], got["msg"], want["kind"])
        if want["kind"] in MSG:
            assert MSG[want["kind"]] in got["msg"], got["msg"]
        if want["off"] is not None:
            assert got["off"] == want["off"] and got["total"] == want["total"]
        if want["out"] is not None:
            assert got["out"][:want["total"]] == want["out"]
            assert got["out"][want["total"]:] == bytes([SENTINEL]) * (len(got["out"]) - want["total"])  # untouched
            if replies:
                assert got["replies"] == want["replies"]
            if status:
                assert got["status"] == want["status"]
        self.same(dict.fromkeys(names))
        return want


def cmds_bytes(cmds, vals_unused=None):
    """rows (op, a, b, val_off, val_len) -> an array of rbx_string_cmd"""
    arr = (L.RbxStringCmd * max(len(cmds), 1))()
    for c, (op, a, b, vo, vl) in zip(arr, cmds):
        c.op, c.a, c.b, c.val_off, c.val_len = op, a, b, vo, vl
    return arr


def run_host(client, names, keys, cmds, vals, cap, replies=True, status=True):
    n = len(keys)
    k = np.asarray(keys if n else [0], np.uint32)
    v = (C.c_uint8 * max(1, len(vals))).from_buffer_copy(bytes(vals) or b"\0")
    rep = np.full(max(n, 1), 77, np.int64)
    st = np.full(max(n, 1), 77, np.uint8)
    off = np.full(n + 1, 77, np.uint64)
    out = np.full(max(cap, 1), SENTINEL, np.uint8)
    total = C.c_uint64(77)
    names_arr, _keep = L.names_array(names)
    rc = L.lib().rbx_string_stream(client.ctx, names_arr, len(names), k.ctypes.data_as(L.u32p), cmds_bytes(cmds), n,
                                   v if vals else None, len(vals), cap, off.ctypes.data_as(L.u64p),
                                   out.ctypes.data_as(L.u8p) if cap else None, rep.ctypes.data_as(L.i64p) if replies else None,
                                   st.ctypes.data_as(L.u8p) if status else None, C.byref(total))
    return dict(rc=rc, msg=L.last_error() if rc else "", replies=rep[:n].tolist(), status=st[:n].tolist(),
                off=off.tolist(), out=out[:cap].tobytes(), total=total.value)


def run_dev(client, names, keys, cmds, vals, cap, replies=True, status=True):
    """the device form over torch tensors, enqueued on the context's stream"""
    import torch

    n = len(keys)
    d_key = torch.from_numpy(np.asarray(keys if n else [0], np.uint32).view(np.int32).copy()).cuda()
    raw = np.frombuffer(bytes(cmds_bytes(cmds)), np.uint8)[: 32 * max(n, 1)].copy()
    d_cmds = torch.from_numpy(raw).cuda()
    d_vals = torch.from_numpy(np.frombuffer(bytes(vals) or b"\0", np.uint8).copy()).cuda()
    d_rep = torch.full((max(n, 1),), 77, dtype=torch.int64, device="cuda")
    d_st = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), 77, dtype=torch.int64, device="cuda")
    d_out = torch.full((max(cap, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    arr, _keep = L.names_array(names)
    total = C.c_uint64(77)
    rc = L.lib().rbx_string_stream_dev(client.ctx, arr, len(names), d_key.data_ptr(), d_cmds.data_ptr(), n,
                                       d_vals.data_ptr() if vals else None, len(vals), cap, d_off.data_ptr(),
                                       d_out.data_ptr() if cap else None, d_rep.data_ptr() if replies else None,
                                       d_st.data_ptr() if status else None, C.byref(total), None)
    client.synchronize()
    return dict(rc=rc, msg=L.last_error() if rc else "", replies=d_rep.cpu().numpy()[:n].tolist(),
                status=d_st.cpu().numpy()[:n].tolist(), off=d_off.cpu().numpy().view(np.uint64).tolist(),
                out=d_out.cpu().numpy()[:cap].tobytes(), total=total.value)


RUNNERS = {"host": run_host, "dev": run_dev}


class Vals:
    """the call's value buffer: add(value, residue) places a value at an offset of that residue mod 16"""

    def __init__(self):
        self.buf = bytearray()

    def add(self, value, residue=None):
        if residue is not None:
            self.buf += bytes((residue - len(self.buf)) % 16)
        at = len(self.buf)
        self.buf += value
        return at, len(value)


# ---- alignment -------------------------------------------------------------------------------------------------------------
VAL_LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 65]
STR_LENS = [0, 1, 15, 16, 17, 255, 256, 257]


@pytest.mark.parametrize("lanes", LANES)
def test_alignment_grid(client, fresh, lanes):
    """every destination offset mod 16 x source offset mod 16 x value length, one command per key; then the same grid
    of GETRANGEs, whose neighbouring output slices must not disturb each other"""
    run = RUNNERS["dev" if lanes in (8, 32) else "host"]
    rng = np.random.default_rng(lanes)
    both = Both(client)
    names, keys, cmds, vals = [], [], [], Vals()
    for d in range(16):
        for s in range(16):
            for j, v in enumerate(VAL_LENS):
                name = f"{fresh}:{d}:{s}:{v}"
                n = STR_LENS[(d + s + j) % len(STR_LENS)]
                if n or (d + s) % 2:  # (some of the empty ones are missing keys)
                    both.put(name, rng.bytes(n))
                at, ln = vals.add(rng.bytes(v), s)
                keys.append(len(names))
                names.append(name)
                cmds.append((SETRANGE, d + 16 * (j % 3), 0, at, ln) if (d + j) % 4 else (APPEND, 0, 0, at, ln))
    with tuned(lanes=lanes):
        both.stream(run, names, keys, cmds, bytes(vals.buf))
        # the reads: a filler read ahead of each command sets the residue of its output slice
        filler = fresh + ":filler"
        both.put(filler, rng.bytes(15))
        names.append(filler)
        rkeys, rcmds, at_out, i = [], [], 0, 0
        for d in range(16):
            for s in range(16):
                for v in VAL_LENS:
                    pad = (d - at_out) % 16
                    rkeys += [len(names) - 1, i]
                    rcmds += [(GETRANGE, 0, pad - 1, 0, 0) if pad else (GETRANGE, 5, 4, 0, 0), (GETRANGE, s, s + v - 1, 0, 0)]
                    got = len(both.ks.getrange(names[i], s, s + v - 1)) if v else 0
                    at_out += pad + got
                    i += 1
        both.stream(run, names, rkeys, rcmds, b"")


# ---- order on one key --------------------------------------------------------------------------------------------------------
def order_commands(rng):
    """one key's commands (key 0), a wrong-type key's (key 1) and a late key's (key 2) in one call"""
    vals, keys, cmds = Vals(), [], []

    def add(k, op, a=0, b=0, value=b""):
        at, ln = vals.add(value) if op in (SETRANGE, APPEND) else (0, 0)
        keys.append(k)
        cmds.append((op, a, b, at, ln))

    # overlapping SETRANGEs with a GETRANGE between each pair
    for off, n in [(0, 40), (10, 40), (5, 3), (30, 100), (29, 2), (0, 1)]:
        add(0, SETRANGE, off, value=rng.bytes(n))
        add(0, GETRANGE, 0, -1)
    # a chain of 100 APPENDs of 1..7 bytes with a GETRANGE -8 -1 after each
    for i in range(100):
        add(0, APPEND, value=rng.bytes(1 + i % 7))
        add(0, GETRANGE, -8, -1)
    # a SETRANGE past the end, then an APPEND
    add(0, SETRANGE, 1000, value=b"past")
    add(0, APPEND, value=b"then")
    add(0, GETRANGE, 990, -1)
    # a failed command of each kind in the middle: the running length is unchanged behind it
    add(0, SETRANGE, -1, value=b"x")
    add(0, APPEND, value=b"A")
    add(0, SETRANGE, M.KMAX, value=b"x")
    add(0, APPEND, value=b"B")
    add(1, APPEND, value=b"wrong type")
    add(1, GET)
    add(1, SETRANGE, -3, value=b"offset first")
    add(0, GET)
    # a key created by its third command after two failed ones
    add(2, SETRANGE, -1, value=b"no")
    add(2, SETRANGE, M.KMAX - 1, value=b"no")
    add(2, GET)
    add(2, SETRANGE, 3, value=b"yes")
    add(2, GET)
    add(0, SETRANGE, 7, value=b"")  # an empty value replies the length
    return keys, cmds, bytes(vals.buf)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("how", ["sorted", "serial", "chunks", "tiers-4", "tiers-64"])
def test_order_on_one_key(client, fresh, form, how):
    both = Both(client)
    names = [fresh + "k", fresh + "hll", fresh + "late", fresh + "k"]
    both.put(names[0], b"start", timeout=True)
    both.hll(names[1])
    keys, cmds, vals = order_commands(np.random.default_rng(5))
    keys = [3 if k == 0 and i % 3 == 0 else k for i, k in enumerate(keys)]  # the same name twice is one key
    knobs = {"sorted": {}, "serial": dict(serial_max=10_000), "chunks": dict(chunk=7),
             "tiers-4": dict(short_max=64, tile=4096, lanes=4), "tiers-64": dict(short_max=64, tile=4096, lanes=64)}[how]
    with tuned(**knobs):
        want = both.stream(RUNNERS[form], names, keys, cmds, vals)
    assert want["kind"] == M.OFFSET and M.FAILED in want["status"]
    assert both.ks.ttl(names[0]) == "set"  # SETRANGE and APPEND keep the timeout
    # the same commands through the engine's single calls give the same strings
    solo = Both(client)
    snames = [n + "s" for n in names[:3]] + [names[0] + "s"]
    solo.put(snames[0], b"start")
    solo.hll(snames[1])
    for k, (op, a, b, vo, vl) in zip(keys, cmds):
        single(client, snames[k], op, a, b, vals[vo:vo + vl], "host")
    assert export(client, snames[0]) == export(client, names[0])
    assert export(client, snames[2]) == export(client, names[2]) == b"\0\0\0yes"


def single(client, name, op, a=0, b=0, value=b"", form="host", cap=1 << 16):
    """one engine single call -> (rc, message, number, bytes); cap: the room a read gets"""
    lib = client.ctx and L.lib()
    nm, _keep = L.name_struct(name)
    n = C.c_uint64(77)
    if op in (GETRANGE, GET):
        if op == GET:
            a, b = 0, -1
        if form == "host":
            buf = np.full(cap, SENTINEL, np.uint8)
            rc = lib.rbx_string_getrange(client.ctx, nm, a, b, buf.ctypes.data_as(L.u8p), cap, C.byref(n))
            data = buf
        else:
            import torch

            d = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = lib.rbx_string_getrange_dev(client.ctx, nm, a, b, d.data_ptr(), cap, C.byref(n), None)
            client.synchronize()
            data = d.cpu().numpy()
        if rc:
            return rc, L.last_error(), 0, None
        assert bytes(data[min(n.value, cap):]) == bytes([SENTINEL]) * (cap - min(n.value, cap))
        return rc, "", n.value, bytes(data[:min(n.value, cap)])
    if form == "host":
        buf = (C.c_uint8 * max(1, len(value))).from_buffer_copy(bytes(value) or b"\0")
        ptr = buf if value else None
        rc = (lib.rbx_string_setrange(client.ctx, nm, a, ptr, len(value), C.byref(n)) if op == SETRANGE
              else lib.rbx_string_append(client.ctx, nm, ptr, len(value), C.byref(n)))
    else:
        import torch

        d = torch.from_numpy(np.frombuffer(bytes(value) or b"\0", np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        ptr = d.data_ptr() if value else None
        rc = (lib.rbx_string_setrange_dev(client.ctx, nm, a, ptr, len(value), C.byref(n), None) if op == SETRANGE
              else lib.rbx_string_append_dev(client.ctx, nm, ptr, len(value), C.byref(n), None))
        client.synchronize()
    return rc, (L.last_error() if rc else ""), (n.value if rc == 0 else 0), None


# ---- the single calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_single_calls_against_the_model(client, fresh, form):
    rng = np.random.default_rng(11)
    both = Both(client)
    k, hll, missing = fresh + "k", fresh + "hll", fresh + "missing"
    both.put(k, rng.bytes(300), timeout=True)
    both.hll(hll)
    steps = [(k, GETRANGE, 0, -1, b""), (k, GETRANGE, -10, -3, b""), (k, GETRANGE, 5, 2, b""), (k, GETRANGE, -1, -5, b""),
             (k, GETRANGE, M.INT64_MIN, M.INT64_MAX, b""), (missing, GETRANGE, 0, -1, b""), (hll, GETRANGE, 0, -1, b""),
             (k, SETRANGE, 299, 0, rng.bytes(2)), (k, SETRANGE, 7, 0, rng.bytes(33)), (k, SETRANGE, 400, 0, b""),
             (k, SETRANGE, -1, 0, b"x"), (hll, SETRANGE, -1, 0, b"x"), (hll, SETRANGE, 0, 0, b"x"), (hll, APPEND, 0, 0, b""),
             (k, SETRANGE, M.KMAX, 0, b"x"), (k, SETRANGE, M.INT64_MAX, 0, b"x"), (missing, SETRANGE, M.KMAX + 9, 0, b""),
             (k, APPEND, 0, 0, rng.bytes(5000)), (k, SETRANGE, 70_001, 0, rng.bytes(70_000)),  # more than one tile
             (k, GETRANGE, 3, 50_000, b""), (k, APPEND, 0, 0, b""), (fresh + "new", APPEND, 0, 0, b""),
             (fresh + "new2", SETRANGE, 1000, 0, b"created at an offset"), (fresh + "new", GETRANGE, 0, -1, b"")]
    for name, op, a, b, value in steps:
        rc, msg, num, data = single(client, name, op, a, b, value, form)
        try:
            d, n, _st = both.ks.command(name, op, a, b, value)
            assert (rc, num, data) == (0, n, d), (name, op, a, b, len(value))
        except M.Failed as e:
            assert rc == RC[e.kind] and MSG[e.kind] in msg, (name, op, a, e.kind, msg)
        both.same([name])
    assert not exists(client, missing) and exists(client, fresh + "new") and export(client, fresh + "new") == b""
    assert ttl(client, k) == "set"
    # getrange writes min(cap, len) bytes and reports len
    nm, _keep = L.name_struct(k)
    buf, n = np.full(8, SENTINEL, np.uint8), C.c_uint64()
    assert L.lib().rbx_string_getrange(client.ctx, nm, 0, -1, buf.ctypes.data_as(L.u8p), 5, C.byref(n)) == 0
    assert n.value == both.ks.strlen(k) and buf.tobytes() == both.ks.get(k)[:5] + bytes([SENTINEL]) * 3
    assert L.lib().rbx_string_getrange(client.ctx, nm, 0, -1, None, 5, C.byref(n)) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_string_append(client.ctx, nm, None, 5, None) == L.RBX_E_ILLEGAL_ARGUMENT


def test_truncate_script_and_the_zero_padding(client, fresh):
    both = Both(client)
    k = fresh + "k"
    nm, _keep = L.name_struct(k)

    def truncate(size, key=k):
        n2, _k2 = L.name_struct(key)
        assert L.lib().rbx_string_truncate(client.ctx, n2, size) == 0
        both.ks.truncate(key, size)
        both.same([key])

    both.put(k, b"\xFF" * 4099, timeout=True)
    truncate(5000)
    assert ttl(client, k) == "set"      # size >= len: nothing happens
    truncate(0)
    assert ttl(client, k) == "none"     # GETRANGE 0 -1: the content stays, the SET drops the timeout
    assert export(client, k) == b"\xFF" * 4099
    truncate(3)
    old = C.c_int()
    assert L.lib().rbx_bitset_set(client.ctx, nm, 32000, 1, C.byref(old)) == 0
    got = export(client, k)
    assert got == b"\xFF" * 3 + bytes(3997) + b"\x80"   # what the cut took off reads zero
    both.ks.set(k, got)
    truncate(-1)
    truncate(-(1 << 63))                # both ends clamp to 0: one byte stays
    assert export(client, k) == b"\xFF"
    truncate(-1, fresh + "missing")     # SET key "" creates the empty string
    assert exists(client, fresh + "missing")
    truncate(0, fresh + "missing2")
    assert not exists(client, fresh + "missing2")
    both.hll(fresh + "hll")
    n3, _k3 = L.name_struct(fresh + "hll")
    assert L.lib().rbx_string_truncate(client.ctx, n3, 0) == L.RBX_E_WRONGTYPE
    # SETRANGE at len + 1000: the gap reads zero through GETRANGE and through BITCOUNT
    g = fresh + "gap"
    both.put(g, b"\xFF" * 100)
    rc, _m, num, _d = single(client, g, SETRANGE, 1100, 0, b"\xFF\xFF")
    assert (rc, num) == (0, 1102)
    assert single(client, g, GETRANGE, 100, 1099)[3] == bytes(1000)
    ng, _kg = L.name_struct(g)
    ones = C.c_uint64()
    assert L.lib().rbx_bitset_cardinality(client.ctx, ng, C.byref(ones)) == 0 and ones.value == 102 * 8
    # a string that shrank and grows again shows none of its old bytes
    truncate_to = fresh + "regrow"
    both.put(truncate_to, b"\xAB" * 600)
    truncate(10, truncate_to)
    both.stream(run_host, [truncate_to], [0, 0], [(SETRANGE, 500, 0, 0, 1), (GET, 0, 0, 0, 0)], b"Z")
    assert export(client, truncate_to) == b"\xAB" * 10 + bytes(490) + b"Z"


# ---- growth and creation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_growth_and_creation(client, fresh, form):
    rng = np.random.default_rng(3)
    both = Both(client)
    a, b, c, only, cfg, cfg2 = (fresh + s for s in ("a", "b", "c", "only", "cfg", "cfg2"))
    both.put(a, rng.bytes(200))
    both.put(b, rng.bytes(4000), timeout=True)
    # a Bloom filter's bit string under a {name}:config keeps the config's capacity; a handle opened BEFORE the call
    # that grows the string past its allocation still answers after it
    f = client.getBloomFilter(cfg)
    assert f.tryInit(20_000, 0.01)
    assert f.add("one")
    handle = BloomHandle(client, cfg)
    assert bloom_add_multi(client, [handle], [0, 1], Arena([b"through the handle"]))[0] == 1
    both.ks.set(cfg, export(client, cfg))
    both.ks.other.add(_config_name(cfg))
    # a second filter that has its config but no bit string yet: a byte command creates the string
    f2 = client.getBloomFilter(cfg2)
    assert f2.tryInit(20_000, 0.01) and not exists(client, cfg2)
    handle2 = BloomHandle(client, cfg2)
    config_bytes = (f.getSize() + 7) // 8
    assert memory(client, cfg) - 256 >= config_bytes and config_bytes < 30_000
    vals = Vals()
    keys, cmds = [], []

    def add(k, op, a_=0, b_=0, value=b""):
        at, ln = vals.add(value) if op in (SETRANGE, APPEND) else (0, 0)
        keys.append(k)
        cmds.append((op, a_, b_, at, ln))

    add(0, APPEND, value=rng.bytes(100))        # across 256
    add(0, GET)
    add(1, SETRANGE, 4090, value=rng.bytes(20))  # across 4096
    add(1, APPEND, value=rng.bytes(5000))
    add(1, GETRANGE, 4000, 4200)
    add(2, SETRANGE, -1, value=b"x")             # c: created by its third command after two failed ones
    add(2, SETRANGE, M.KMAX, value=b"x")
    add(2, APPEND, value=b"third")
    add(3, SETRANGE, -1, value=b"x")             # only failed writes: not created
    add(3, SETRANGE, M.KMAX - 2, value=b"xyz")
    add(3, SETRANGE, 5, value=b"")               # an empty value creates nothing either
    add(4, SETRANGE, 30_000, value=b"far")       # the filter's string grows past the config's size
    add(5, APPEND, value=b"x")                   # the config hash itself is another type
    add(6, SETRANGE, 0, value=b"\0")             # created by a byte command under its config
    names = [a, b, c, only, cfg, _config_name(cfg), cfg2]
    want = both.stream(RUNNERS[form], names, keys, cmds, bytes(vals.buf))
    assert want["kind"] == M.OFFSET
    assert not exists(client, only) and export(client, c) == b"third" and ttl(client, b) == "set"
    assert f.contains("one") and f.add("two") and f.contains("two")  # by name, on the grown string
    assert export(client, cfg)[30_000:] == b"far"
    # the allocations: the grown string covers its new length, the created one its config's size though it holds 1 byte
    assert memory(client, cfg) - 256 >= 30_003
    assert export(client, cfg2) == b"\0" and memory(client, cfg2) - 256 >= config_bytes
    # the handles opened before the call, through the multi-tenant host calls
    three = [b"through the handle", b"never added", b"added behind the growth"]
    counts, flags = bloom_contains_multi(client, [handle], [0, 3], Arena(three), per_key=True)
    assert (int(counts[0]), flags.tolist()) == (1, [1, 0, 0])
    assert bloom_add_multi(client, [handle, handle2], [0, 3, 6], Arena(three * 2)).tolist() == [2, 3]
    counts, flags = bloom_contains_multi(client, [handle, handle2], [0, 3, 6], Arena(three * 2), per_key=True)
    assert counts.tolist() == [3, 3] and flags.all()
    assert export(client, cfg)[30_000:30_003] == b"far" and len(export(client, cfg2)) > 1  # the adds grew cfg2's string
    handle.close()
    handle2.close()


# ---- tiers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_tiers_rounds_and_the_counter(client, fresh, form):
    rng = np.random.default_rng(17)
    run = RUNNERS[form]
    both = Both(client)
    k1, k2, k3 = fresh + "one", fresh + "two", fresh + "three"
    both.put(k1, rng.bytes(500))
    both.put(k2, rng.bytes(100))
    with tuned(short_max=64, tile=4096):
        # commands of 64 and 65 bytes: the threshold between the tiers
        vals = Vals()
        c64, c65 = vals.add(rng.bytes(64)), vals.add(rng.bytes(65))
        both.stream(run, [k1], [0] * 4, [(SETRANGE, 3, 0, *c64), (SETRANGE, 100, 0, *c65), (GETRANGE, 0, 63, 0, 0),
                                         (GETRANGE, 1, 65, 0, 0)], bytes(vals.buf))
        assert last() == [2, 2, 2, 3]  # two long commands on the one key: three rounds
        # short, long, short, long, short on one key, all overlapping; a second key with one long command: the two
        # keys' first long commands share a round, and rounds = 1 + 3 with the third long command of key one
        vals = Vals()
        rows = [(0, SETRANGE, 10, rng.bytes(20)), (0, SETRANGE, 0, rng.bytes(9000)), (0, SETRANGE, 8990, rng.bytes(30)),
                (0, GETRANGE, 5, None), (0, APPEND, 0, rng.bytes(7)), (1, APPEND, 0, rng.bytes(5000)), (1, GETRANGE, -9, None),
                (0, SETRANGE, 4000, rng.bytes(4097)), (0, GETRANGE, 3990, 4010)]
        keys, cmds = [], []
        for k, op, a, v in rows:
            at, ln = vals.add(v) if op != GETRANGE else (0, 0)
            keys.append(k)
            cmds.append((op, a, -1 if v is None else (v if op == GETRANGE else 0), at, ln))
        both.stream(run, [k1, k2], keys, cmds, bytes(vals.buf))
        assert last() == [5, 4, 3 + 3 + 2 + 2, 4]  # tiles: 9000 -> 3, GETRANGE of 9,020 bytes -> 3, 5000 -> 2, 4097 -> 2
        # one SETRANGE and one GETRANGE of 9 MiB + 3 bytes: 2,305 tiles each, more than the grid has workgroups
        big = rng.bytes(BIG)
        both.stream(run, [k3], [0, 0, 0], [(SETRANGE, 5, 0, 0, BIG), (GETRANGE, 5, -1, 0, 0), (GETRANGE, -3, -1, 0, 0)], big)
        assert last() == [1, 2, 2 * 2305, 3]


# ---- chunks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_chunks_carry_the_running_length_and_off(client, fresh, form):
    rng = np.random.default_rng(29)
    both = Both(client)
    names = [fresh + "a", fresh + "b", fresh + "c"]
    both.put(names[0], rng.bytes(20))
    vals, keys, cmds = Vals(), [], []
    for i in range(50):
        k = int(rng.integers(0, 3))
        op = [APPEND, GETRANGE, SETRANGE, GET][int(rng.integers(0, 4))]
        at, ln = vals.add(rng.bytes(int(rng.integers(0, 90)))) if op in (APPEND, SETRANGE) else (0, 0)
        keys.append(k)
        cmds.append((op, int(rng.integers(-20, 200)), int(rng.integers(-20, 200)), at, ln))
    with tuned(chunk=7, short_max=64, tile=4096):
        want = both.stream(RUNNERS[form], names, keys, cmds, bytes(vals.buf))
    assert want["total"] > 0 and M.FAILED in want["status"]


# ---- the caller's errors, total > cap, names -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_caller_errors_and_reads_that_do_not_fit(client, fresh, form):
    run = RUNNERS[form]
    both = Both(client)
    a, b = fresh + "a", fresh + "b"
    both.put(a, b"0123456789", timeout=True)
    vals = b"ABCDEFGH"
    for keys, cmds in [([2], [(GET, 0, 0, 0, 0)]), ([0, 0], [(APPEND, 0, 0, 0, 2), (4, 0, 0, 0, 0)]),
                       ([0, 1], [(APPEND, 0, 0, 0, 2), (APPEND, 0, 0, 7, 2)]), ([1], [(SETRANGE, 0, 0, 9, 0)])]:
        both.stream(run, [a, b], keys, cmds, vals, cap=64)
    assert not exists(client, b) and export(client, a) == b"0123456789"
    # the reads do not fit: refused before any write, off and total exact; the repeat with enough room succeeds
    keys, cmds = [0, 1, 0, 1], [(APPEND, 0, 0, 0, 8), (APPEND, 0, 0, 2, 3), (GET, 0, 0, 0, 0), (GET, 0, 0, 0, 0)]
    want = both.stream(run, [a, b], keys, cmds, vals, cap=20)
    assert want["kind"] == M.ILLEGAL and want["off"] == [0, 0, 0, 18, 21] and not exists(client, b)
    want = both.stream(run, [a, b], keys, cmds, vals, cap=21)
    assert want["kind"] is None and want["out"] == b"0123456789ABCDEFGH" + b"CDE"
    # NULL arrays, n = 0
    lib, names_arr = L.lib(), L.names_array([a])[0]
    off, total = np.full(1, 77, np.uint64), C.c_uint64(77)
    assert lib.rbx_string_stream(client.ctx, names_arr, 1, None, None, 0, None, 0, 0, off.ctypes.data_as(L.u64p), None, None,
                                 None, C.byref(total)) == 0 and (off[0], total.value) == (0, 0)
    key = np.zeros(1, np.uint32)
    arr = cmds_bytes([(GET, 0, 0, 0, 0)])
    for args in [(None, arr, None, 0, 0, off.ctypes.data_as(L.u64p), None), (key.ctypes.data_as(L.u32p), None, None, 0, 0, off.ctypes.data_as(L.u64p), None),
                 (key.ctypes.data_as(L.u32p), arr, None, 0, 0, None, None), (key.ctypes.data_as(L.u32p), arr, None, 4, 0, off.ctypes.data_as(L.u64p), None),
                 (key.ctypes.data_as(L.u32p), arr, None, 0, 16, off.ctypes.data_as(L.u64p), None)]:
        k_, c_, v_, vl, cap, o_, out_ = args
        assert lib.rbx_string_stream(client.ctx, names_arr, 1, k_, c_, 1, v_, vl, cap, o_, out_, None, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    both.same([a, b])
    assert ttl(client, a) == "set"


@pytest.mark.parametrize("form", ["host", "dev"])
def test_names_duplicates_and_binary(client, fresh, form):
    both = Both(client)
    raw = fresh.encode() + b"\x00\xff\x00bin"
    names = [raw, fresh + "x", raw, fresh + "x", raw]
    keys = [0, 2, 1, 4, 3, 0, 1]
    vals = b"abcdefghij"
    cmds = [(APPEND, 0, 0, 0, 3), (APPEND, 0, 0, 3, 3), (APPEND, 0, 0, 0, 2), (GET, 0, 0, 0, 0), (SETRANGE, 1, 0, 8, 2),
            (GETRANGE, -4, -1, 0, 0), (GET, 0, 0, 0, 0)]
    # the model knows names by their bytes
    mnames = [n if isinstance(n, bytes) else n.encode() for n in names]
    want = both.ks.stream(mnames, keys, cmds, vals, 64)
    got = RUNNERS[form](client, names, keys, cmds, vals, 64)
    assert (got["rc"], got["replies"], got["status"], got["off"]) == (0, want["replies"], want["status"], want["off"])
    assert got["out"][:want["total"]] == want["out"] == b"abcdef" + b"cdef" + b"aij"
    assert export(client, raw) == b"abcdef" and export(client, fresh + "x") == b"aij"


# ---- Spring Data and RBinaryStream ----------------------------------------------------------------------------------------------
def test_spring_data_methods_and_pipeline(client, fresh):
    conn = RedissonConnection(client)
    a, b, hll = [(fresh + s).encode() for s in ("a", "b", "hll")]
    assert client.getHyperLogLog(hll.decode()).addAll([b"x"])
    assert conn.get(a) is None and conn.set(a, b"hello") is True and conn.get(a) == b"hello"
    assert conn.append(a, b" world") == 11 and conn.getRange(a, 6, -1) == b"world" and conn.getRange(a, -100, 100) == b"hello world"
    assert conn.setRange(a, b"W", 6) is None and conn.get(a) == b"hello World"
    assert conn.getRange(b, 0, -1) == b"" and conn.append(b, b"") == 0 and conn.get(b) == b""  # the empty string exists
    assert conn.mGet(a, fresh.encode() + b"missing", hll, b) == [b"hello World", None, None, b""]
    for call, msg in [(lambda: conn.get(hll), "WRONGTYPE"), (lambda: conn.append(hll, b"x"), "WRONGTYPE"),
                      (lambda: conn.setRange(a, b"x", -1), "offset is out of range"),
                      (lambda: conn.setRange(a, b"x", M.KMAX), "string exceeds maximum"),
                      (lambda: conn.getRange(hll, 0, 1), "WRONGTYPE")]:
        with pytest.raises(RedisException, match=msg):
            call()
    assert conn.set(hll, b"a string now") and conn.get(hll) == b"a string now"  # SET replaces any type
    # a pipeline: the four byte commands are ONE rbx_string_stream call, then one bit call
    conn.openPipeline()
    assert conn.setRange(a, b"J", 0) is None
    conn.append(b, b"tail")
    conn.getRange(a, 0, 4)
    conn.get(b)
    conn.setBit(a, 7, True)
    res = conn.closePipeline()
    assert res == [None, 4, b"Jello", b"tail", False]
    assert sum(last()[:2]) == 4  # the run ahead of the bit command was one call of four commands
    assert conn.get(a) == b"Kello World"
    # failures inside a pipeline: every command runs, then the first failure is raised
    conn.openPipeline()
    conn.append(a, b"!")
    conn.setRange(a, b"x", -5)
    conn.append(a, b"?")
    conn.set(b, b"reset")
    conn.mGet(a, b)
    with pytest.raises(RedisException, match="offset is out of range"):
        conn.closePipeline()
    assert conn.mGet(a, b) == [b"Kello World!?", b"reset"]


def test_binary_stream(client, fresh):
    s = client.getBinaryStream(fresh + "stream")
    assert isinstance(s, RBinaryStream) and s.get() is None and s.size() == 0
    out = s.getOutputStream()
    chunks = [b"0123456", b"789abcdefghij", b"klm"]
    for c in chunks:
        out.write(c)
    whole = b"".join(chunks)
    assert s.get() == whole and s.size() == 23 and s.isExists()
    inp, got = s.getInputStream(), []
    assert inp.available() == 23
    while True:
        r = inp.read(5)
        if r == -1:
            break
        got.append(r)
    assert b"".join(got) == whole and [len(g) for g in got] == [5, 5, 5, 5, 3]
    assert inp.index == 25  # the index advances by the requested length, as the reference's does
    ch = s.getChannel()
    assert ch.position(2) is ch and ch.write(b"XY") == 2 and ch.position() == 4
    assert s.get() == b"01XY" + whole[4:]
    assert ch.read(4) == whole[4:8] and ch.position() == 8
    assert ch.position(21).read(10) == b"lm" and ch.position() == 23 and ch.read(10) == -1
    assert ch.position(0).read(0) == b"" and ch.position() == 0  # an empty buffer reads nothing (not GETRANGE 0 -1)
    assert s.expire(3_600_000) and s.remainTimeToLive() > 0
    ch.truncate(0)
    assert s.size() == 23 and s.remainTimeToLive() == -1  # the size-0 quirk: the content stays, the timeout goes
    ch.truncate(4)
    assert s.get() == b"01XY" and ch.size() == 4
    ch.position(6).write(b"!")
    assert s.get() == b"01XY\0\0!"  # what the cut took off reads zero
    s.set(b"fresh")
    assert s.get() == b"fresh" and s.delete() and s.get() is None


# ---- mixed families: byte commands between the bit families' on shared keys ------------------------------------------------
import bitstring_driver as D  # noqa: E402
import bitstring_model as BM  # noqa: E402
from redisson_amd.client import (_range_row, bitset_range_stream_call, string_stream_call, string_truncate)  # noqa: E402
from redisson_amd.exceptions import raise_for  # noqa: E402

MIXED_SEEDS, MIXED_STEPS = (0, 1), 300
BYTE_SHARE = 0.45  # of the steps; the others are bitstring_driver's next command
BYTE_KINDS = {"setrange": 3, "append": 3, "getrange": 2, "get": 1, "truncate": 1.5, "byte_stream": 3, "range_stream": 2}
BYTE_BOUNDARIES = (0, 16, 256, 512, 4096, 65536)
VALUE_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 300, 5000)
FAILED_ROW = "failed"


def value_of(seed, n):
    return np.random.default_rng([0xB7E, seed]).bytes(n)


class ByteKeyspace(BM.Keyspace):
    """bitstring_model's keyspace plus the byte commands, by the rules of bytestream_model.  A string there is never
    empty (an empty value is a missing key), so the sequences draw no command that would leave one: no APPEND of
    nothing, no truncate below one byte."""

    def _value(self, key):
        return self._get(key) or b""  # raises WRONGTYPE first

    @BM.command
    def getrange(self, via, key, start, end):
        return M.getrange_of(self._value(key), start, end)

    @BM.command
    def get(self, via, key):
        return self._get(key)

    @BM.command
    def setrange(self, via, key, offset, seed, n):
        if offset < 0:
            raise BM.Failed(BM.REDIS)
        s = self._value(key)
        if n == 0:
            return len(s)
        if offset + n > M.KMAX:
            raise BM.Failed(BM.REDIS)
        new = bytearray(s) + bytes(max(0, offset + n - len(s)))
        new[offset:offset + n] = value_of(seed, n)
        self._put(key, bytes(new))
        return len(new)

    @BM.command
    def append(self, via, key, seed, n):
        new = self._value(key) + value_of(seed, n)
        self._put(key, new)
        return len(new)

    @BM.command
    def truncate(self, via, key, size):
        s = self._value(key)
        if size >= len(s):
            return None
        self._put(key, M.getrange_of(s, 0, size - 1), "set")
        return None

    @BM.command
    def byte_stream(self, via, rows):
        """rows of (key, op, a, b, seed, n), as n single calls in order: a read's bytes (None: nil), a write's length"""
        out = []
        for key, op, a, b, seed, n in rows:
            reply, err = (self.getrange(via, key, a, b) if op == GETRANGE else self.get(via, key) if op == GET
                          else self.setrange(via, key, a, seed, n) if op == SETRANGE else self.append(via, key, seed, n))
            out.append(FAILED_ROW if err else reply)
        return out

    @BM.command
    def range_stream(self, via, rows):
        """rows of (key, 'count', start, end) / (key, 'pos', bit, nargs, start, end) / (key, 'strlen')"""
        out = []
        for key, what, *args in rows:
            reply, err = (self.bitcount(via, key, *args, "BYTE") if what == "count"
                          else self.bitpos(via, key, *args, "BYTE") if what == "pos" else self.size(via, key))
            out.append(FAILED_ROW if err else reply // 8 if what == "strlen" else reply)
        return out


class ByteGpuEngine(D.GpuEngine):
    def _single(self, key, op, a=0, b=0, value=b"", form="dev"):
        rc, msg, num, data = single(self.client, self._name(key), op, a, b, value, form, cap=1 << 22)
        raise_for(rc, msg)
        assert data is None or num == len(data)
        return num, data

    def getrange(self, via, key, start, end):
        if via == "conn":
            return self.conn.getRange(self._raw(key), start, end)
        return self._single(key, GETRANGE, start, end, form=via)[1]

    def get(self, via, key):
        return self.conn.get(self._raw(key))

    def setrange(self, via, key, offset, seed, n):
        if via == "conn":
            self.conn.setRange(self._raw(key), value_of(seed, n), offset)
            return self.conn.strLen(self._raw(key)) if n == 0 or offset >= 0 else None
        return self._single(key, SETRANGE, offset, 0, value_of(seed, n), via)[0]

    def append(self, via, key, seed, n):
        if via == "conn":
            return self.conn.append(self._raw(key), value_of(seed, n))
        return self._single(key, APPEND, 0, 0, value_of(seed, n), via)[0]

    def truncate(self, via, key, size):
        string_truncate(self.client, self._name(key), size)

    def byte_stream(self, via, rows):
        names = list(dict.fromkeys(self._name(r[0]) for r in rows))
        keys = [names.index(self._name(r[0])) for r in rows]
        if via == "host":
            rc, msg, replies, status, off, out = string_stream_call(
                self.client, names, keys, [(op, a, b, value_of(seed, n) if op in (SETRANGE, APPEND) else b"")
                                           for _k, op, a, b, seed, n in rows])
        else:
            vals, cmds = Vals(), []
            for _k, op, a, b, seed, n in rows:
                at, ln = vals.add(value_of(seed, n)) if op in (SETRANGE, APPEND) else (0, 0)
                cmds.append((op, a, b, at, ln))
            got = run_dev(self.client, names, keys, cmds, bytes(vals.buf), 4096)
            if got["rc"] == L.RBX_E_ILLEGAL_ARGUMENT and got["total"] > 4096:  # refused before any write: ask again
                got = run_dev(self.client, names, keys, cmds, bytes(vals.buf), got["total"])
            rc, msg, replies, status, off, out = got["rc"], got["msg"], got["replies"], got["status"], got["off"], got["out"]
        if rc not in (L.RBX_OK, L.RBX_E_REDIS, L.RBX_E_WRONGTYPE):
            raise_for(rc, msg)
        return [FAILED_ROW if int(status[i]) == M.FAILED else
                (None if int(status[i]) == M.NIL else out[int(off[i]):int(off[i + 1])]) if r[1] in (GETRANGE, GET)
                else int(replies[i]) for i, r in enumerate(rows)]

    def range_stream(self, via, rows):
        names = list(dict.fromkeys(self._name(r[0]) for r in rows))
        keys = [names.index(self._name(r[0])) for r in rows]
        table = [_range_row(L.RBX_RANGE_COUNT, 0, 2, r[2], r[3]) if r[1] == "count"
                 else _range_row(L.RBX_RANGE_POS, r[2], r[3], r[4], r[5]) if r[1] == "pos" else _range_row(L.RBX_RANGE_STRLEN)
                 for r in rows]
        rc, msg, replies, status = bitset_range_stream_call(self.client, names, keys, table)
        if rc not in (L.RBX_OK, L.RBX_E_REDIS, L.RBX_E_WRONGTYPE):
            raise_for(rc, msg)
        return [FAILED_ROW if int(s) == 0xFF else int(r) for r, s in zip(replies, status)]


for _k in BYTE_KINDS:
    setattr(ByteGpuEngine, _k, D._guarded(getattr(ByteGpuEngine, _k)))


def draw_byte_command(rng, model):
    """one byte-family command on the shared keys, from the model's lengths"""
    def integer(lo, hi):
        return int(rng.integers(lo, hi, endpoint=True))

    def choice(seq):
        return seq[int(rng.integers(len(seq)))]

    def key_for(write):
        if rng.random() < 0.05:
            return D.HLL
        return choice(D.BITSETS + (D.BLOOM,)) if write else choice(D.BITSETS + (D.BLOOM, D.MISSING))

    def offset(key):
        n = model.strlen(key)
        if rng.random() < 0.06:
            return choice((-1, -integer(2, 1 << 40), M.KMAX, M.KMAX - 1))  # the two failures of SETRANGE
        return min(max(choice(BYTE_BOUNDARIES + (n, 2 * n)) + integer(-9, 9), 0), 1 << 20)

    def ends(key):
        n = model.strlen(key)
        return tuple(choice((integer(-n - 3, n + 3), choice(BYTE_BOUNDARIES) + integer(-2, 2), -1, 0)) for _ in range(2))

    def row():
        op = choice((GETRANGE, GETRANGE, GET, SETRANGE, SETRANGE, APPEND, APPEND))
        key = key_for(op in (SETRANGE, APPEND))
        if op in (GETRANGE, GET):
            return (key, op, *ends(key), 0, 0)
        return (key, op, offset(key) if op == SETRANGE else 0, 0, integer(0, 1 << 30),
                choice(VALUE_SIZES + ((0,) if op == SETRANGE else ())))

    kinds = list(BYTE_KINDS)
    p = np.array([BYTE_KINDS[k] for k in kinds], float)
    kind = kinds[int(rng.choice(len(kinds), p=p / p.sum()))]
    via = choice(("conn", "host", "dev"))
    if kind == "getrange":
        key = key_for(False)
        return (kind, via, key, *ends(key))
    if kind == "get":
        return (kind, "conn", key_for(False))
    if kind == "setrange":
        key = key_for(True)
        return (kind, via, key, offset(key), integer(0, 1 << 30), choice(VALUE_SIZES + (0,)))
    if kind == "append":
        return (kind, via, key_for(True), integer(0, 1 << 30), choice(VALUE_SIZES))
    if kind == "truncate":
        key = key_for(True)
        n = model.strlen(key)
        return (kind, "obj", key, max(choice((0, 1, 3, n // 2, n - 1, n, n + 5)), 0) if n != 1 or rng.random() < 0.5 else 1)
    if kind == "byte_stream":
        rows = [row() for _ in range(integer(2, 12))]
        # the model's strings are never empty: the first row on a key it would create writes at least one byte
        return (kind, choice(("host", "dev")), tuple(rows))
    keys = [key_for(False) for _ in range(integer(2, 10))]
    return (kind, "host", tuple(choice(((k, "count", *ends(k)), (k, "pos", integer(0, 1), 2, *ends(k)), (k, "strlen")))
                                for k in keys))


def byte_probes(model):
    out = []
    for key in D.STRINGS + (D.MISSING,):
        n = model.strlen(key)
        out += [("get", "conn", key), ("getrange", "dev", key, -40, -1), ("getrange", "host", key, max(n - 3, 0), n + 300),
                ("range_stream", "host", ((key, "strlen"), (key, "count", 0, -1)))]
    return out


@pytest.mark.parametrize("seed", MIXED_SEEDS)
def test_mixed_families_on_shared_keys(client, fresh, seed):
    """2 seeds x 300 steps: bitstring_driver's SETBIT / index / range-fill / BITOP / BITFIELD / BITCOUNT / BITPOS / key /
    Bloom commands and, between them, byte commands and range streams on the same keys; every reply and error kind, and
    every 25 steps the driver's full check plus the byte readers, equal the model.  Seed 1 runs with the tiers forced."""
    rng = np.random.default_rng([0xB17E, seed])
    engine, model = ByteGpuEngine(client, fresh + ":"), ByteKeyspace()
    base = D.commands(seed, MIXED_STEPS)
    history, counts = [], {}

    def compare(cmd, step, what):
        want, got = D.call(model, cmd), D.call(engine, cmd)
        if got != want:
            tail = "\n".join(f"  {i}: {D.short(c)!r}" for i, c in history[-15:])
            raise AssertionError(f"seed {seed}, step {step} ({what}): {D.short(cmd)!r}\n  engine / model error kind: "
                                 f"{got[1]!r} / {want[1]!r}\n  engine / model reply: {D.first_difference(got[0], want[0])}\n"
                                 f"the last commands:\n{tail}")

    def full_check(step):
        for probe in D.probes(model, seed, step) + byte_probes(model):
            compare(probe, step, "full check after it")

    knobs = dict(short_max=64, tile=4096, serial_max=4) if seed else {}
    try:
        with tuned(**knobs):
            for step in range(MIXED_STEPS):
                cmd = next(base) if step < 2 or rng.random() >= BYTE_SHARE else draw_byte_command(rng, model)
                history.append((step, cmd))
                counts[cmd[0]] = counts.get(cmd[0], 0) + 1
                compare(cmd, step, "command")
                if (step + 1) % 25 == 0:
                    full_check(step)
            full_check(MIXED_STEPS - 1)
    finally:
        engine.close()
    assert all(counts.get(k, 0) >= 3 for k in BYTE_KINDS), counts
    assert sum(counts.get(k, 0) for k in ("setbit", "bitop", "bitcount", "set_fields", "incr_fields", "bitfield")) >= 20, counts
