#!/usr/bin/env python3
"""The ordered GETBIT / SETBIT stream over many keys (rbx_bitset_stream_dev) against what one call per key
offers, in one process on one MI355X.  Every batch is 2^24 commands at uniform random indexes.

  a  GETBITs over one 128 MiB key (gather)                       vs getIndexesDev of the same indexes
  b  SETBIT 1s without replies over that key (scatter)            vs setIndexesDev of the same indexes
  c  GETBIT / SETBIT 0 / SETBIT 1 mixed, with replies, over that key (sorted by cell)
                                                                  vs setFieldsDev u1 with replies (the single-key
                                                                     grouped path) of the same offsets
  d  the three shapes over 4,096 keys of 1 MiB, keys uniform random
                                                                  vs a loop of 4,096 single-key *_dev calls on the
                                                                     same commands split by key

Rows a to c are reported as ratios.  Row d carries the one requirement: each multi-key batch takes less time
than its per-key loop in the same run (`faster`: yes / no).

Each figure is a call time: a host clock around the call (the loop of calls) and the stream synchronise that
ends it; the *_dev calls' own wait for their batch summary is part of the call.  Operation and baseline
alternate inside one loop; the median of the repetitions is reported.  `ratio` = the operation's time over its
baseline's.  Writes one JSON document (default profiles/bitset/bitstream_bench.json).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 24, help="commands per batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "bitstream_bench.json"))
    a = ap.parse_args()
    n = a.n

    client = RedissonClient(0)
    lib = L.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB175712E)
    zeros = torch.zeros(ONE_KEY_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def make(name, nbytes):
        assert lib.rbx_bloom_import_dev(client.ctx, name.encode(), zeros.data_ptr(), nbytes, None) == 0

    one = "bench:stream:one"
    many = ["bench:stream:%04d" % i for i in range(MANY_KEYS)]
    make(one, ONE_KEY_BYTES)
    for name in many:
        make(name, MANY_KEY_BYTES)
    client.synchronize()
    del zeros

    ops_get = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ops_set1 = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    ops_mixed = torch.randint(0, 3, (n,), dtype=torch.uint8, device="cuda", generator=g)
    values = torch.randint(0, 2, (n,), dtype=torch.int64, device="cuda", generator=g)  # the u1 baseline's
    replies = torch.empty(n, dtype=torch.uint8, device="cuda")
    replies64 = torch.empty(n, dtype=torch.int64, device="cuda")

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def stream(names_arr, nkeys, keys, ops, idx, rep):
        def run():
            rc = lib.rbx_bitset_stream_dev(client.ctx, names_arr, nkeys, keys.data_ptr(), ops.data_ptr(), idx.data_ptr(), n,
                                           rep.data_ptr() if rep is not None else None, None)
            assert rc == 0, L.last_error()
            client.synchronize()
        return run

    rows = []

    def measure(row, label, keys, op, base_label, base):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x, y = clock(op), clock(base)
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        r = {"row": row, "operation": label, "commands": n, "keys": keys, "call_ms_median": m_op * 1e3,
             "call_ms_min": min(t_op) * 1e3, "call_ms_max": max(t_op) * 1e3, "M_commands_per_s": n / m_op / 1e6,
             "baseline": base_label, "baseline_ms_median": m_base * 1e3, "baseline_ms_min": min(t_base) * 1e3,
             "baseline_ms_max": max(t_base) * 1e3, "ratio": m_op / m_base, "reps": a.reps}
        if row.startswith("d"):
            r["faster"] = "yes" if m_op < m_base else "no"
        rows.append(r)
        print(json.dumps(r), flush=True)

    # ---- rows a to c: one 128 MiB key ----
    bs = client.getBitSet(one)
    idx = torch.randint(0, ONE_KEY_BYTES * 8, (n,), dtype=torch.int64, device="cuda", generator=g)
    key0 = torch.zeros(n, dtype=torch.int32, device="cuda")
    one_arr, _keep1 = L.names_array([one])
    torch.cuda.synchronize()

    def get_indexes():
        bs.getIndexesDev(idx.data_ptr(), n, replies.data_ptr())
        client.synchronize()

    def set_indexes():
        bs.setIndexesDev(idx.data_ptr(), n, True)
        client.synchronize()

    def set_fields():
        bs.setFieldsDev(1, idx.data_ptr(), values.data_ptr(), n, replies64.data_ptr(), signed=False)
        client.synchronize()

    measure("a", "stream, GETBITs, one key (gather)", 1, stream(one_arr, 1, key0, ops_get, idx, replies),
            "getIndexesDev", get_indexes)
    measure("b", "stream, SETBIT 1s, no replies, one key (scatter)", 1, stream(one_arr, 1, key0, ops_set1, idx, None),
            "setIndexesDev", set_indexes)
    measure("c", "stream, mixed with replies, one key (grouped)", 1, stream(one_arr, 1, key0, ops_mixed, idx, replies),
            "setFieldsDev u1 with replies", set_fields)
    bs.delete()

    # ---- row d: 4,096 keys of 1 MiB; the baseline's commands sorted by key, one slice per key ----
    keys = torch.randint(0, MANY_KEYS, (n,), dtype=torch.int32, device="cuda", generator=g)
    idx = torch.randint(0, MANY_KEY_BYTES * 8, (n,), dtype=torch.int64, device="cuda", generator=g)
    many_arr, _keep2 = L.names_array(many)
    order = torch.argsort(keys.to(torch.int64), stable=True)
    idx_by_key, values_by_key = idx[order].contiguous(), values[order].contiguous()
    counts = torch.bincount(keys.to(torch.int64), minlength=MANY_KEYS).cpu().tolist()
    starts = [0]
    for c in counts:
        starts.append(starts[-1] + c)
    sets = [client.getBitSet(name) for name in many]
    torch.cuda.synchronize()

    def loop(call):
        def run():
            for k in range(MANY_KEYS):
                if counts[k]:
                    call(sets[k], starts[k], counts[k])
            client.synchronize()
        return run

    loop_get = loop(lambda s, o, m: s.getIndexesDev(idx_by_key.data_ptr() + 8 * o, m, replies.data_ptr() + o))
    loop_set = loop(lambda s, o, m: s.setIndexesDev(idx_by_key.data_ptr() + 8 * o, m, True))
    loop_fields = loop(lambda s, o, m: s.setFieldsDev(1, idx_by_key.data_ptr() + 8 * o, values_by_key.data_ptr() + 8 * o, m,
                                                      replies64.data_ptr() + 8 * o, signed=False))
    measure("d-a", "stream, GETBITs, 4096 keys (gather)", MANY_KEYS, stream(many_arr, MANY_KEYS, keys, ops_get, idx, replies),
            "4096 getIndexesDev calls", loop_get)
    measure("d-b", "stream, SETBIT 1s, no replies, 4096 keys (scatter)", MANY_KEYS,
            stream(many_arr, MANY_KEYS, keys, ops_set1, idx, None), "4096 setIndexesDev calls", loop_set)
    measure("d-c", "stream, mixed with replies, 4096 keys (grouped)", MANY_KEYS,
            stream(many_arr, MANY_KEYS, keys, ops_mixed, idx, replies), "4096 setFieldsDev u1 calls with replies",
            loop_fields)

    doc = {"bench": "bitstream", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call (or loop of calls) + stream synchronise", "one_key_bytes": ONE_KEY_BYTES,
           "many_keys": MANY_KEYS, "many_key_bytes": MANY_KEY_BYTES,
           "requirement": "rows d-*: the stream's median below its per-key loop's", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for s in sets:
        s.delete()
    client.shutdown()


if __name__ == "__main__":
    main()
