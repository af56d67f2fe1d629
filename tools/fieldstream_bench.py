#!/usr/bin/env python3
"""The ordered BITFIELD stream over many keys (rbx_bitset_field_stream_dev) against what one call per key
offers, in one process on one MI355X.

  a  2^24 u16 INCRBYs with replies on one 128 MiB key (sorted by word)   vs incrementFieldsDev of the same batch
  b  the same without replies (one compare-and-swap loop per command)    vs incrementFieldsDev without replies
  c  2^24 u16 INCRBYs with replies over 4,096 keys of 1 MiB, keys uniform random
                                                                  vs a loop of 4,096 incrementFieldsDev calls on the
                                                                     same commands split by key
  d  100,000 keys x 16 commands of mixed Byte / Short / Integer methods (i8 / i16 / i32 GET / SET / INCRBY at
     multiples of their size), with replies: word cells           times only
  e  the same with unaligned u5 fields: key cells                  times only

Row c carries the one requirement: the multi-key batch takes less time than its per-key loop in the same run
(`faster`: yes / no).  Rows a and b are reported as ratios and carry no bound; rows d and e have no single-call
baseline worth a loop of 100,000 calls.

Each figure is a call time: a host clock around the call (the loop of calls) and the stream synchronise that
ends it; the *_dev calls' own wait for their batch summary is part of the call.  Operation and baseline
alternate inside one loop; the median of the repetitions is reported.  `ratio` = the operation's time over its
baseline's.  Writes one JSON document (default profiles/bitset/fieldstream_bench.json).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from redisson_amd import RedissonClient  # noqa: E402
from redisson_amd import _lib as L  # noqa: E402

ONE_KEY_BYTES = 1 << 27
MANY_KEYS, MANY_KEY_BYTES = 4096, 1 << 20
USERS, PER_USER, USER_BYTES = 100_000, 16, 64
PATHS = {1: "one lane", 2: "sorted by word", 3: "sorted by key", 4: "gather", 5: "compare-and-swap"}


def pack(offsets, values, op, signed, size, overflow=0):
    """n rbx_field_cmd records on the device: {u64 offset, i64 value, u8 op, is_signed, size, overflow, pad[4]};
    op, signed and size are numbers or int64 tensors"""
    cmds = torch.zeros(offsets.numel(), 3, dtype=torch.int64, device="cuda")
    cmds[:, 0] = offsets
    cmds[:, 1] = values
    cmds[:, 2] = op + signed * 256 + size * 65536 + overflow * 16777216  # little-endian bytes
    return cmds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 24, help="commands per batch of rows a to c")
    ap.add_argument("--users", type=int, default=USERS, help="keys of rows d and e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "fieldstream_bench.json"))
    a = ap.parse_args()
    n = a.n

    client = RedissonClient(0)
    lib = L.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(0xF1E1D5)
    zeros = torch.zeros(ONE_KEY_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def make(name, nbytes):
        assert lib.rbx_bloom_import_dev(client.ctx, name.encode(), zeros.data_ptr(), nbytes, None) == 0

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def stream(names_arr, nkeys, keys, cmds, rep, status, took):
        m = keys.numel()

        def run():
            rc = lib.rbx_bitset_field_stream_dev(client.ctx, names_arr, nkeys, keys.data_ptr(), cmds.data_ptr(), m,
                                                 rep.data_ptr() if rep is not None else None,
                                                 status.data_ptr() if status is not None else None, None)
            assert rc == 0, L.last_error()
            client.synchronize()
            took.append(lib.rbx_bench_fieldstream_last_path())
        return run

    rows = []

    def measure(row, label, commands, keys, op, took, base_label=None, base=None):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x = clock(op)
            y = clock(base) if base else 0.0
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op = statistics.median(t_op)
        r = {"row": row, "operation": label, "commands": commands, "keys": keys, "path": PATHS.get(took[-1], "?"),
             "call_ms_median": m_op * 1e3, "call_ms_min": min(t_op) * 1e3, "call_ms_max": max(t_op) * 1e3,
             "M_commands_per_s": commands / m_op / 1e6, "reps": a.reps}
        if base:
            m_base = statistics.median(t_base)
            r.update({"baseline": base_label, "baseline_ms_median": m_base * 1e3, "baseline_ms_min": min(t_base) * 1e3,
                      "baseline_ms_max": max(t_base) * 1e3, "ratio": m_op / m_base})
            if row.startswith("c"):
                r["faster"] = "yes" if m_op < m_base else "no"
        rows.append(r)
        print(json.dumps(r), flush=True)

    incs = torch.randint(-1000, 1000, (n,), dtype=torch.int64, device="cuda", generator=g)
    most = max(n, a.users * PER_USER)
    replies = torch.empty(most, dtype=torch.int64, device="cuda")
    status = torch.empty(most, dtype=torch.uint8, device="cuda")

    # ---- rows a and b: one 128 MiB key ----
    one = "bench:fields:one"
    make(one, ONE_KEY_BYTES)
    client.synchronize()
    bs = client.getBitSet(one)
    offs = 16 * torch.randint(0, ONE_KEY_BYTES // 2, (n,), dtype=torch.int64, device="cuda", generator=g)
    cmds = pack(offs, incs, L.RBX_FIELD_INCRBY, 0, 16)
    key0 = torch.zeros(n, dtype=torch.int32, device="cuda")
    one_arr, _keep1 = L.names_array([one])
    torch.cuda.synchronize()

    def increment(rep):
        def run():
            bs.incrementFieldsDev(16, offs.data_ptr(), incs.data_ptr(), n, rep.data_ptr() if rep is not None else None,
                                  signed=False)
            client.synchronize()
        return run

    took = []
    measure("a", "stream, u16 INCRBYs with replies, one key", n, 1, stream(one_arr, 1, key0, cmds, replies, status, took),
            took, "incrementFieldsDev u16 with replies", increment(replies))
    measure("b", "stream, u16 INCRBYs without replies, one key", n, 1, stream(one_arr, 1, key0, cmds, None, None, took),
            took, "incrementFieldsDev u16 without replies", increment(None))
    bs.delete()
    del key0

    # ---- row c: 4,096 keys of 1 MiB; the baseline's commands sorted by key, one slice per key ----
    many = ["bench:fields:%04d" % i for i in range(MANY_KEYS)]
    for name in many:
        make(name, MANY_KEY_BYTES)
    client.synchronize()
    del zeros
    keys = torch.randint(0, MANY_KEYS, (n,), dtype=torch.int32, device="cuda", generator=g)
    offs = 16 * torch.randint(0, MANY_KEY_BYTES // 2, (n,), dtype=torch.int64, device="cuda", generator=g)
    cmds = pack(offs, incs, L.RBX_FIELD_INCRBY, 0, 16)
    many_arr, _keep2 = L.names_array(many)
    order = torch.argsort(keys.to(torch.int64), stable=True)
    offs_by_key, incs_by_key = offs[order].contiguous(), incs[order].contiguous()
    counts = torch.bincount(keys.to(torch.int64), minlength=MANY_KEYS).cpu().tolist()
    starts = [0]
    for c in counts:
        starts.append(starts[-1] + c)
    sets = [client.getBitSet(name) for name in many]
    torch.cuda.synchronize()

    def loop(with_replies):
        def run():
            for k in range(MANY_KEYS):
                if counts[k]:
                    o = starts[k]
                    sets[k].incrementFieldsDev(16, offs_by_key.data_ptr() + 8 * o, incs_by_key.data_ptr() + 8 * o, counts[k],
                                               replies.data_ptr() + 8 * o if with_replies else None, signed=False)
            client.synchronize()
        return run

    measure("c", "stream, u16 INCRBYs with replies, 4096 keys", n, MANY_KEYS,
            stream(many_arr, MANY_KEYS, keys, cmds, replies, status, took), took,
            "4096 incrementFieldsDev calls with replies", loop(True))
    measure("c-b", "stream, u16 INCRBYs without replies, 4096 keys", n, MANY_KEYS,
            stream(many_arr, MANY_KEYS, keys, cmds, None, None, took), took,
            "4096 incrementFieldsDev calls without replies", loop(False))
    for s in sets:
        s.delete()
    del keys, offs, cmds, offs_by_key, incs_by_key, order

    # ---- rows d and e: a few packed counters per user, 100,000 users, 16 commands each in random order ----
    users = ["bench:fields:u:%06d" % i for i in range(a.users)]
    users_arr, _keep3 = L.names_array(users)
    m = a.users * PER_USER
    keys = torch.randint(0, a.users, (m,), dtype=torch.int32, device="cuda", generator=g)
    size = 8 << torch.randint(0, 3, (m,), dtype=torch.int64, device="cuda", generator=g)  # Byte, Short, Integer
    slot = torch.randint(0, 1 << 30, (m,), dtype=torch.int64, device="cuda", generator=g)
    op = torch.randint(0, 3, (m,), dtype=torch.int64, device="cuda", generator=g)
    vals = torch.randint(-100, 100, (m,), dtype=torch.int64, device="cuda", generator=g)
    aligned = pack(size * (slot % (USER_BYTES * 8 // size)), vals, op, 1, size)
    unaligned = pack(slot % (USER_BYTES * 8 - 5), vals, op, 0, 5)
    torch.cuda.synchronize()
    measure("d", "stream, mixed i8 / i16 / i32 methods with replies, %d keys x %d" % (a.users, PER_USER), m, a.users,
            stream(users_arr, a.users, keys, aligned, replies, status, took), took)
    measure("e", "stream, unaligned u5 fields with replies, %d keys x %d" % (a.users, PER_USER), m, a.users,
            stream(users_arr, a.users, keys, unaligned, replies, status, took), took)

    doc = {"bench": "fieldstream", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call (or loop of calls) + stream synchronise", "one_key_bytes": ONE_KEY_BYTES,
           "many_keys": MANY_KEYS, "many_key_bytes": MANY_KEY_BYTES, "users": a.users, "commands_per_user": PER_USER,
           "user_bytes": USER_BYTES, "requirement": "row c: the stream's median below its per-key loop's",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    client.shutdown()  # frees the keys with the context


if __name__ == "__main__":
    main()
