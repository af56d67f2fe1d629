#!/usr/bin/env python3
"""BITCOUNT / BITPOS / STRLEN over many keys in one call (rbx_bitset_range_stream_dev) against what one call per
command offers, in one process on one MI355X.

  a  100,000 keys of 46 bytes, one BITCOUNT k -30 -1 BIT each; and the first 4,096 of those commands
                                                                  vs a loop of 4,096 rbx_bitset_count_range calls
  b  the same keys, BITPOS k 1 and STRLEN interleaved             (recorded)
  c  2^20 ranged counts on one 128 MiB key                        vs rbx_bitset_count_ranges_dev of the same ranges
  d  rangestream_lanes 4 .. 64 at string sizes 46 B, 1 KiB and 64 KiB (whole-string counts, walked by the group)
  e  rangestream_short_max and rangestream_tile swept on 99 % 46-byte keys and 1 % 8 MiB keys, whole-string counts
  f  10,000 whole-string BITCOUNTs of 128 KiB                     vs the same through rbx_bitset_op_groups

Row a's 4,096-command pair carries the one requirement: the stream takes less time than the loop of single calls in
the same run (`faster`: yes / no); --rows a runs it alone, for the three separate processes DESIGN 11.10 asks for.

Each figure is a call time: a host clock around the call (the loop of calls) and the stream synchronise that ends
it; the _dev call's own wait for its summary is part of the call.  Operation and baseline alternate inside one
loop; the median of the repetitions is reported.  `ratio` = the operation's time over its baseline's.  Writes one
JSON document (default profiles/bitset/rangestream_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from redisson_amd import RedissonClient  # noqa: E402
from redisson_amd import _lib as L  # noqa: E402
from redisson_amd.client import _range_cmds_array, bitset_op_groups_call  # noqa: E402

USERS, USER_BYTES, PAIR = 100_000, 46, 4096
COUNT, POS, STRLEN, BYTE, BIT = L.RBX_RANGE_COUNT, L.RBX_RANGE_POS, L.RBX_RANGE_STRLEN, L.RBX_RANGE_BYTE, L.RBX_RANGE_BIT
DEFAULTS = {"rangestream_lanes": 16, "rangestream_short_max": 4096, "rangestream_tile": 65536}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abcdef")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "rangestream_bench.json"))
    a = ap.parse_args()

    client = RedissonClient(0)
    lib = L.lib()
    rng = np.random.default_rng(0x7A96E)
    rows = []

    def tune(**knobs):
        for k, v in knobs.items():
            assert lib.rbx_tune(k.encode(), v) == 0, (k, v)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def put(name, data):
        client.getBitSet(name).setBytes(data)

    def device_cmds(keys, cmd_rows):
        """(d_key, d_cmds, d_replies, d_status) of a batch"""
        n = len(keys)
        d_key = torch.from_numpy(np.asarray(keys, np.uint32).view(np.int32).copy()).cuda()
        raw = np.frombuffer(bytes(_range_cmds_array(cmd_rows)), np.uint8)[: 24 * n].copy()
        return (d_key, torch.from_numpy(raw).cuda(), torch.empty(n, dtype=torch.int64, device="cuda"),
                torch.empty(n, dtype=torch.uint8, device="cuda"))

    def stream(names, batch, n):
        arr, keep = L.names_array(names)
        d_key, d_cmds, d_rep, d_st = batch

        def run(_keep=keep):
            rc = lib.rbx_bitset_range_stream_dev(client.ctx, arr, len(names), d_key.data_ptr(), d_cmds.data_ptr(), n,
                                                 d_rep.data_ptr(), d_st.data_ptr(), None)
            assert rc == 0, L.last_error()
            client.synchronize()
        return run

    def measure(row, label, n, op, base_label=None, base=None, **extra):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x = clock(op)
            y = clock(base) if base else 0.0
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op = statistics.median(t_op)
        last = (C.c_uint32 * 4)()
        lib.rbx_bench_rangestream_last(last)
        r = dict({"row": row, "operation": label, "commands": n, "call_ms_median": m_op * 1e3, "call_ms_min": min(t_op) * 1e3,
                  "call_ms_max": max(t_op) * 1e3, "call_ms_p10": float(np.percentile(t_op, 10)) * 1e3,
                  "call_ms_p90": float(np.percentile(t_op, 90)) * 1e3, "M_commands_per_s": n / m_op / 1e6, "reps": a.reps,
                  "last_short_long_tiles_waits": list(last)}, **extra)
        if base:
            m_base = statistics.median(t_base)
            r.update({"baseline": base_label, "baseline_ms_median": m_base * 1e3, "baseline_ms_min": min(t_base) * 1e3,
                      "baseline_ms_max": max(t_base) * 1e3, "ratio": m_op / m_base})
            if row == "a-pair":
                r["faster"] = "yes" if m_op < m_base else "no"
        rows.append(r)
        print(json.dumps(r), flush=True)

    # ---- rows a and b: 100,000 users, a year of daily activity each ----
    users = ["bench:range:u%06d" % i for i in range(USERS)]
    if set(a.rows) & set("abde"):
        blob = rng.bytes(USERS * USER_BYTES)
        for i, name in enumerate(users):
            put(name, blob[i * USER_BYTES: (i + 1) * USER_BYTES])
        client.synchronize()
    last30 = (COUNT, 0, 2, -30, -1, BIT)
    if "a" in a.rows:
        measure("a", "stream, BITCOUNT k -30 -1 BIT, 100,000 keys of 46 bytes", USERS,
                stream(users, device_cmds(range(USERS), [last30] * USERS), USERS))
        structs = [L.name_struct(n.encode()) for n in users[:PAIR]]
        out = C.c_uint64()

        def loop():
            for nm, _keep in structs:
                lib.rbx_bitset_count_range(client.ctx, nm, -30, -1, BIT, C.byref(out))
            client.synchronize()

        measure("a-pair", "stream, the first 4,096 of those commands", PAIR,
                stream(users[:PAIR], device_cmds(range(PAIR), [last30] * PAIR), PAIR),
                "4,096 rbx_bitset_count_range calls", loop)
    if "b" in a.rows:
        mixed = [(POS, 1, 0, 0, 0, BYTE) if i % 2 == 0 else (STRLEN, 0, 0, 0, 0, BYTE) for i in range(USERS)]
        measure("b", "stream, BITPOS k 1 and STRLEN interleaved, 100,000 keys of 46 bytes", USERS,
                stream(users, device_cmds(range(USERS), mixed), USERS))

    # ---- row c: 2^20 ranged counts on one 128 MiB key ----
    if "c" in a.rows:
        one, nbytes, n = "bench:range:one", 1 << 27, 1 << 20
        put(one, rng.bytes(nbytes))
        starts = rng.integers(0, nbytes - 4096, size=n)
        ends = starts + rng.integers(0, 4096, size=n)
        batch = device_cmds([0] * n, [(COUNT, 0, 2, int(s), int(e), BYTE) for s, e in zip(starts, ends)])
        d_s, d_e = torch.from_numpy(starts.astype(np.int64)).cuda(), torch.from_numpy(ends.astype(np.int64)).cuda()
        d_out = torch.empty(n, dtype=torch.int64, device="cuda")
        nm, _keep = L.name_struct(one.encode())

        def ranges():
            assert lib.rbx_bitset_count_ranges_dev(client.ctx, nm, d_s.data_ptr(), d_e.data_ptr(), n, BYTE, d_out.data_ptr(), None) == 0
            client.synchronize()

        measure("c", "stream, 2^20 ranged counts of up to 4 KiB on one 128 MiB key", n, stream([one], batch, n),
                "rbx_bitset_count_ranges_dev", ranges)
        client.getBitSet(one).delete()

    # ---- row d: the lane group's width at three string sizes (short_max raised so that the group walks) ----
    if "d" in a.rows:
        sized = {46: users[:20000]}
        for size, count in ((1024, 20000), (65536, 2000)):
            sized[size] = ["bench:range:s%d:%05d" % (size, i) for i in range(count)]
            blob = rng.bytes(size * 64)
            for i, name in enumerate(sized[size]):
                put(name, blob[(i % 64) * size: (i % 64 + 1) * size])
        whole = (COUNT, 0, 0, 0, 0, BYTE)
        for size, names in sized.items():
            batch = device_cmds(range(len(names)), [whole] * len(names))
            for lanes in (4, 8, 16, 32, 64):
                tune(rangestream_lanes=lanes, rangestream_short_max=65536)
                measure("d", "stream, whole-string counts, %d keys of %d bytes" % (len(names), size), len(names),
                        stream(names, batch, len(names)), lanes=lanes, string_bytes=size)
        tune(**DEFAULTS)
        for size in (1024, 65536):
            for name in sized[size]:
                client.getBitSet(name).delete()

    # ---- row e: short_max and the tile on a mix of tiny and huge strings ----
    if "e" in a.rows:
        huge = ["bench:range:huge%d" % i for i in range(4)]
        for name in huge:
            put(name, rng.bytes(8 << 20))
        n = 10000
        names = users[:n - 100] + huge
        keys = list(range(n - 100)) + [n - 100 + i % 4 for i in range(100)]
        order = rng.permutation(n)
        batch = device_cmds([keys[i] for i in order], [(COUNT, 0, 0, 0, 0, BYTE)] * n)
        for short_max in (64, 1024, 4096, 65536, 1 << 20):
            for tile in (4096, 16384, 65536, 262144, 1 << 20):
                tune(rangestream_short_max=short_max, rangestream_tile=tile)
                measure("e", "stream, whole-string counts, 99 % 46-byte keys and 1 % 8 MiB keys", n,
                        stream(names, batch, n), short_max=short_max, tile=tile)
        tune(**DEFAULTS)
        for name in huge:
            client.getBitSet(name).delete()

    # ---- row f: 10,000 whole-string BITCOUNTs of 128 KiB ----
    if "f" in a.rows:
        n, size = 10000, 128 << 10
        names = ["bench:range:f%05d" % i for i in range(n)]
        blob = rng.bytes(size * 16)
        for i, name in enumerate(names):
            put(name, blob[(i % 16) * size: (i % 16 + 1) * size])
        batch = device_cmds(range(n), [(COUNT, 0, 0, 0, 0, BYTE)] * n)
        ops, dests, groups = [L.RBX_BITOP_OR] * n, [None] * n, [[i] for i in range(n)]

        def grouped():
            rc, msg, _lens, _counts, _status = bitset_op_groups_call(client, names, ops, dests, groups)
            assert rc == 0, msg

        measure("f", "stream, 10,000 whole-string BITCOUNTs of 128 KiB", n, stream(names, batch, n),
                "rbx_bitset_op_groups (host arrays)", grouped)
        for name in names:
            client.getBitSet(name).delete()

    doc = {"bench": "rangestream", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call (or loop of calls) + stream synchronise", "users": USERS, "user_bytes": USER_BYTES,
           "requirement": "row a-pair: the stream's median below the loop's, in each of three processes", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    client.shutdown()


if __name__ == "__main__":
    main()
