#!/usr/bin/env python3
"""The ordered PFADD / PFCOUNT stream over many keys (rbx_hll_stream) against the single batched calls, in one
process on one MI355X.  Elements are random 16-byte rows in host memory; the keys are warm and dense.

  a  2^20 one-element PFADDs, keys uniform over 4,096      vs rbx_hll_add_multi_n of the same commands
  b  the same with Zipf keys (p ~ 1 / rank)                 vs the same
  c  4,096 PFADDs x 4,096 elements on distinct keys (the auto rule takes rounds)
                                                            vs rbx_hll_add_multi_n
  d  shape c and shape a under hllstream_path 1 (rounds) and 2 (grouped): the two constants of the auto rule,
     the time of one round (shape a by rounds / its rounds) and the grouped time per element (shape a grouped /
     its elements), and their quotient, elements per round
  e  row a's commands followed by 4,096 PFCOUNTs (two phases)  vs rbx_hll_add_multi_n + rbx_hll_count_each
  f  an RBatch of 10^5 addAsync + execute()                 vs a loop of 10^5 RHyperLogLog.add
  g  a short run: PFADD, PFADD, PFCOUNT of one element each on two keys, one stream call
                                                            vs the three single calls (rbx_hll_add_multi_n with one
                                                               segment twice, rbx_hll_count_n)

Rows a and b carry the requirement: the stream takes less time than its baseline in the same run (`faster`).
Each figure is a call time: a host clock around the call (both sides wait for the device themselves).  Operation
and baseline alternate inside one loop; the median of the repetitions after the warm-ups is reported.  `ratio` = the
operation's time over its baseline's.  --rows picks rows; the results of earlier runs stay in the JSON document
(default profiles/hll/hllstream_bench.json).
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

from redisson_amd import Arena, ByteArrayCodec, RedissonClient  # noqa: E402
from redisson_amd import _lib as L  # noqa: E402

NKEYS = 4096
DENSE_EMPTY = b"HYLL" + bytes(12) + bytes(12288)


def greedy_rounds(keys) -> int:
    """pfadd_run's rule: a command on a key of the current round opens the next one"""
    rounds, seen = 1, set()
    for k in keys.tolist():
        if k in seen:
            rounds += 1
            seen = set()
        seen.add(k)
    return rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20, help="commands of rows a, b and e")
    ap.add_argument("--per-key", type=int, default=4096, help="elements per command of row c")
    ap.add_argument("--batch", type=int, default=100_000, help="commands of row f")
    ap.add_argument("--rows", default="abcdefg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hll", "hllstream_bench.json"))
    a = ap.parse_args()
    n = a.n

    import torch

    client = RedissonClient(0)
    lib = L.lib()
    rng = np.random.default_rng(0x5712EA)
    names = ["bench:hll:%04d" % i for i in range(NKEYS)]
    for name in names:  # warm and dense: SET an empty dense string
        client.getHyperLogLog(name).importString(DENSE_EMPTY)
    names_arr, _keep = L.names_array(names)
    rows = []

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def hook():
        out = (C.c_uint32 * 4)()
        lib.rbx_bench_hllstream_last(out)
        return dict(zip(("phases", "runs_by_rounds", "runs_grouped", "chunks"), list(out)))

    def stream_call(keys, ops, seg, arena, replies, names_arr=names_arr, nkeys=NKEYS):
        status = np.zeros(keys.size, np.uint8)

        def run():
            rc = lib.rbx_hll_stream(client.ctx, names_arr, nkeys, keys.ctypes.data_as(L.u32p), ops.ctypes.data_as(L.u8p),
                                    seg.ctypes.data_as(L.u64p), keys.size, arena.ptr(), replies.ctypes.data_as(L.u64p),
                                    status.ctypes.data_as(L.u8p))
            assert rc == 0, L.last_error()
        return run

    def multi_call(keys, seg, arena):
        per_cmd, _keep2 = L.names_array([names[k] for k in keys.tolist()])
        out = np.zeros(keys.size, np.uint8)

        def run():
            rc = lib.rbx_hll_add_multi_n(client.ctx, per_cmd, keys.size, seg.ctypes.data_as(L.u64p), arena.ptr(),
                                         out.ctypes.data_as(L.u8p))
            assert rc == 0, L.last_error()
        run.keep = _keep2
        return run

    def measure(row, label, commands, elements, op, base_label=None, base=None, extra=None, required=False):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x = clock(op)
            took = hook()
            y = clock(base) if base else 0.0
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op = statistics.median(t_op)
        r = {"row": row, "operation": label, "commands": commands, "elements": elements, "call_ms_median": m_op * 1e3,
             "call_ms_min": min(t_op) * 1e3, "call_ms_max": max(t_op) * 1e3, "reps": a.reps, **took, **(extra or {})}
        if base:
            m_base = statistics.median(t_base)
            r.update({"baseline": base_label, "baseline_ms_median": m_base * 1e3, "baseline_ms_min": min(t_base) * 1e3,
                      "baseline_ms_max": max(t_base) * 1e3, "ratio": m_op / m_base})
            if required:
                r["faster"] = "yes" if m_op < m_base else "no"
        rows.append(r)
        print(json.dumps(r), flush=True)
        return m_op

    # ---- shapes ----
    ones = Arena.fixed(rng.integers(0, 256, size=(n, 16), dtype=np.uint8))
    seg1 = np.arange(n + 1, dtype=np.uint64)
    adds = np.zeros(n, np.uint8)
    uniform = rng.integers(0, NKEYS, size=n).astype(np.uint32)
    p = 1.0 / np.arange(1, NKEYS + 1)
    zipf = rng.choice(NKEYS, size=n, p=p / p.sum()).astype(np.uint32)
    replies = np.zeros(n + NKEYS, np.uint64)

    if "a" in a.rows:
        measure("a", "stream, one-element PFADDs, uniform keys", n, n, stream_call(uniform, adds, seg1, ones, replies),
                "rbx_hll_add_multi_n", multi_call(uniform, seg1, ones), {"rounds": greedy_rounds(uniform)}, required=True)
    if "b" in a.rows:
        measure("b", "stream, one-element PFADDs, Zipf keys", n, n, stream_call(zipf, adds, seg1, ones, replies),
                "rbx_hll_add_multi_n", multi_call(zipf, seg1, ones), {"rounds": greedy_rounds(zipf)}, required=True)
    if "e" in a.rows:
        keys_e = np.concatenate([uniform, np.arange(NKEYS, dtype=np.uint32)])
        ops_e = np.concatenate([adds, np.ones(NKEYS, np.uint8)])
        seg_e = np.concatenate([seg1, np.full(NKEYS, n, np.uint64)])
        base_add = multi_call(uniform, seg1, ones)
        cnames = (C.c_char_p * NKEYS)(*[x.encode() for x in names])
        counts = np.zeros(NKEYS, np.uint64)

        def base_e():
            base_add()
            assert lib.rbx_hll_count_each(client.ctx, cnames, NKEYS, counts.ctypes.data_as(L.u64p)) == 0

        measure("e", "stream, row a's PFADDs then 4,096 PFCOUNTs", n + NKEYS, n, stream_call(keys_e, ops_e, seg_e, ones, replies),
                "rbx_hll_add_multi_n + rbx_hll_count_each", base_e)
    if "c" in a.rows or "d" in a.rows:
        big = Arena.fixed(rng.integers(0, 256, size=(NKEYS * a.per_key, 16), dtype=np.uint8))
        seg_c = (np.arange(NKEYS + 1, dtype=np.uint64) * a.per_key).astype(np.uint64)
        keys_c = np.arange(NKEYS, dtype=np.uint32)
        adds_c = np.zeros(NKEYS, np.uint8)
        if "c" in a.rows:
            measure("c", "stream, 4,096 PFADDs x %d elements, distinct keys" % a.per_key, NKEYS, NKEYS * a.per_key,
                    stream_call(keys_c, adds_c, seg_c, big, replies), "rbx_hll_add_multi_n", multi_call(keys_c, seg_c, big))
        if "d" in a.rows:
            got = {}
            for shape, args, cmds, elems in (("c", (keys_c, adds_c, seg_c, big, replies), NKEYS, NKEYS * a.per_key),
                                             ("a", (uniform, adds, seg1, ones, replies), n, n)):
                for path, what in ((1, "rounds"), (2, "grouped")):
                    assert lib.rbx_tune(b"hllstream_path", path) == 0
                    got[shape, what] = measure("d", "stream, shape %s forced by %s" % (shape, what), cmds, elems,
                                               stream_call(*args))
            assert lib.rbx_tune(b"hllstream_path", 0) == 0
            rounds = greedy_rounds(uniform)
            round_s, elem_s = got["a", "rounds"] / rounds, got["a", "grouped"] / n
            r = {"row": "d", "operation": "the auto rule's constants (shape a)", "rounds": rounds,
                 "us_per_round": round_s * 1e6, "ns_per_grouped_element": elem_s * 1e9,
                 "elements_per_round": round_s / elem_s,
                 "ns_per_grouped_element_shape_c": got["c", "grouped"] / (NKEYS * a.per_key) * 1e9,
                 "ns_per_rounds_element_shape_c": got["c", "rounds"] / (NKEYS * a.per_key) * 1e9}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del big
    if "f" in a.rows:
        m = a.batch
        elements = [rng.bytes(16) for _ in range(m)]
        which = rng.integers(0, NKEYS, size=m).tolist()
        codec = ByteArrayCodec()
        objects = [client.getHyperLogLog(name, codec) for name in names]

        def batch():
            b = client.createBatch()
            handles = [b.getHyperLogLog(name, codec) for name in names]
            for k, e in zip(which, elements):
                handles[k].addAsync(e)
            b.execute()

        def loop():
            for k, e in zip(which, elements):
                objects[k].add(e)

        measure("f", "RBatch of %d addAsync + execute()" % m, m, m, batch, "a loop of RHyperLogLog.add", loop)

    if "g" in a.rows:
        keys_g = np.array([0, 1, 0], np.uint32)
        ops_g = np.array([0, 0, 1], np.uint8)
        seg_g = np.array([0, 1, 2, 2], np.uint64)
        two = Arena.fixed(rng.integers(0, 256, size=(2, 16), dtype=np.uint8))
        halves = [Arena.fixed(two.bytes.reshape(2, 16)[i:i + 1]) for i in range(2)]
        one_name = [L.names_array([names[i]]) for i in range(2)]
        seg_one = np.array([0, 1], np.uint64)
        ch, cnt = np.zeros(1, np.uint8), C.c_uint64()

        def singles():
            for i in range(2):
                assert lib.rbx_hll_add_multi_n(client.ctx, one_name[i][0], 1, seg_one.ctypes.data_as(L.u64p), halves[i].ptr(),
                                               ch.ctypes.data_as(L.u8p)) == 0
            assert lib.rbx_hll_count_n(client.ctx, one_name[0][0], 1, C.byref(cnt)) == 0

        two_names, _keep_g = L.names_array(names[:2])
        measure("g", "stream, PFADD, PFADD, PFCOUNT on two keys", 3, 2,
                stream_call(keys_g, ops_g, seg_g, two, replies, two_names, 2), "the three single calls", singles)

    doc = {"bench": "hllstream", "device": torch.cuda.get_device_name(0), "timing": "host clock around the call",
           "keys": NKEYS, "requirement": "rows a and b: the stream's median below rbx_hll_add_multi_n's", "results": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc["results"] = [r for r in json.load(f).get("results", []) if r["row"] not in {x["row"] for x in rows}]
    doc["results"] = sorted(doc["results"] + rows, key=lambda r: r["row"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    client.shutdown()  # frees the keys with the context


if __name__ == "__main__":
    main()
