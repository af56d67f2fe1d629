#!/usr/bin/env python3
"""Grouped BITOPs and BITCOUNTs (rbx_bitset_op_groups) against loops of the single calls (rbx_bitset_op,
rbx_bitset_cardinality), in one process on one MI355X.

  a  10,000 ANDs of 2 x 128 KiB bitmaps drawn from 200 keys, counted and stored nowhere (cohort sizes)
                                             vs the loop: rbx_bitset_op into a temporary, rbx_bitset_cardinality
  b  5,000 independent ORs of 24 x 4 KiB sources into fresh destinations (one phase)   vs a loop of rbx_bitset_op
  c  BITCOUNT of each of 10,000 keys of 4 KiB                                  vs a loop of rbx_bitset_cardinality
  d  1, 16 and 256 ANDs of 2 x 1 MiB into destinations                                  vs a loop of rbx_bitset_op
  e  one AND of 2 x 512 MiB into a destination, uncounted (counts = NULL) and counted          vs one rbx_bitset_op
  f  the bitgroups_tile settings on rows a, d and e
  g  a chain of 1,000 dependent ORs (k[i + 1] <- k[i] | k[i + 1], 4 KiB): every group is its own phase
                                                                                         vs a loop of rbx_bitset_op

Each figure is a call time: a host clock around the call including its final wait (the loop of rbx_bitset_op, whose
launches are asynchronous, ends in a stream synchronise), names and arrays built beforehand.  The grouped call and
its baseline alternate in one loop; the medians after the warm-ups are reported, with the baseline's min and max
as its spread.  `ratio` = the grouped call's median over the baseline's; `below_baseline_min` is the bar of rows
a - d and g, `within_baseline_spread` that of row e.  Rows a and e also give the bytes of sources read per second
beside the stream-read rate of rbx_bench_stream_read from the same run.  --rows picks rows; the results of earlier
runs stay in the JSON document (default profiles/bitset/bitgroups_bench.json).
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

from redisson_amd import RedissonClient  # noqa: E402
from redisson_amd import _lib as L  # noqa: E402

AND, OR = L.RBX_BITOP_AND, L.RBX_BITOP_OR
NO_DEST = L.RBX_BITGROUP_NO_DEST
TILES = (0, 4096, 16384, 65536, 262144, 1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="abcdefg")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every shape (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "bitgroups_bench.json"))
    a = ap.parse_args()
    sc = lambda n: max(1, int(n * a.scale))  # noqa: E731

    import torch

    client = RedissonClient(0)
    lib, ctx = L.lib(), client.ctx
    rng = np.random.default_rng(0xB17609)
    rows = []

    def make(prefix, n, nbytes):
        names = ["bench:bg:%s:%05d" % (prefix, i) for i in range(n)]
        for name in names:
            client.getBitSet(name).setBytes(rng.bytes(nbytes))
        return names

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def hook():
        out = (C.c_uint32 * 4)()
        lib.rbx_bench_bitgroups_last(out)
        return dict(zip(("phases", "launches", "tile", "device_groups"), list(out)))

    def report(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def stats(prefix, t):
        return {prefix + "_ms_median": statistics.median(t) * 1e3, prefix + "_ms_min": min(t) * 1e3,
                prefix + "_ms_max": max(t) * 1e3}

    # ---- the same run's stream-read rate ----
    stream = torch.cuda.Stream()
    probe_bytes = 2 << 30
    buf = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
    sink = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.rbx_bench_stream_read(ctx, buf.data_ptr(), probe_bytes, sink.data_ptr(), stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(5):
        lib.rbx_bench_stream_read(ctx, buf.data_ptr(), probe_bytes, sink.data_ptr(), stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    stream_gbs = probe_bytes / (e0.elapsed_time(e1) / 5 / 1e3) / 1e9
    del buf
    report({"row": "probe", "operation": "rbx_bench_stream_read over 2 GiB", "stream_read_GBps": stream_gbs})

    def grouped_call(names, ops, dests, srcs, per_group, counted=True):
        """one rbx_bitset_op_groups call over `names`: group g is ops[g] into names[dests[g]] (None: nowhere) of the
        per_group sources srcs[g * per_group ..]; counted = False passes counts = NULL, as a BITOP whose caller wants
        no cardinality does"""
        n = len(ops)
        arr, keep = L.names_array(names)
        op = np.asarray(ops, np.uint8)
        dest = np.asarray([NO_DEST if d is None else d for d in dests], np.uint32)
        off = (np.arange(n + 1, dtype=np.uint64) * per_group).astype(np.uint64)
        key = np.ascontiguousarray(srcs, dtype=np.uint32).reshape(-1)
        lens, counts, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)

        def run():
            rc = lib.rbx_bitset_op_groups(ctx, arr, len(names), op.ctypes.data_as(L.u8p), dest.ctypes.data_as(L.u32p),
                                          off.ctypes.data_as(L.u64p), key.ctypes.data_as(L.u32p), n,
                                          lens.ctypes.data_as(L.u64p), counts.ctypes.data_as(L.u64p) if counted else None,
                                          status.ctypes.data_as(L.u8p))
            assert rc == 0, L.last_error()
        run.counts, run.keep = counts, keep
        return run

    def op_loop(names, ops, dests, srcs, per_group, count=False):
        """the same by the single calls: rbx_bitset_op per group (into names[dests[g]]), then rbx_bitset_cardinality of
        the destination when counted; ends in a stream synchronise (rbx_bitset_op alone does not wait)"""
        n = len(ops)
        one = [L.name_struct(nm) for nm in names]
        srcs = np.asarray(srcs).reshape(n, per_group)
        arrs = [L.names_array([names[k] for k in srcs[g].tolist()]) for g in range(n)]
        outs = (C.c_uint64 * n)()
        length = C.c_uint64()

        def run():
            for g in range(n):
                rc = lib.rbx_bitset_op(ctx, int(ops[g]), one[dests[g]][0], arrs[g][0], per_group, C.byref(length))
                assert rc == 0, L.last_error()
                if count:
                    rc = lib.rbx_bitset_cardinality(ctx, one[dests[g]][0], C.cast(C.byref(outs, 8 * g), L.u64p))
                    assert rc == 0, L.last_error()
            client.synchronize()
        run.counts = np.frombuffer(outs, np.uint64)
        return run

    def compare(row, label, grouped, base, base_label, extra=None, before=None, same_counts=True, read_bytes=0):
        """the grouped call and its baseline, alternating; before = (fn, fn): run, untimed, ahead of each side"""
        t_op, t_base = [], []
        for _ in range(a.warmup + a.reps):
            if before:
                before[0]()
            t_op.append(clock(grouped))
            took = hook()
            if before:
                before[1]()
            t_base.append(clock(base))
        t_op, t_base = t_op[a.warmup:], t_base[a.warmup:]
        if same_counts:
            assert np.array_equal(grouped.counts, base.counts), "the grouped call and the loop disagree"
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        r = {"row": row, "operation": label, **stats("call", t_op), "reps": a.reps, **took, "baseline": base_label,
             **stats("baseline", t_base), "ratio": m_op / m_base,
             "below_baseline_min": "yes" if m_op < min(t_base) else "no",
             "within_baseline_spread": "yes" if m_op <= max(t_base) else "no", **(extra or {})}
        if read_bytes:
            gbs = read_bytes / m_op / 1e9
            r.update({"source_read_GBps": gbs, "baseline_source_read_GBps": read_bytes / m_base / 1e9,
                      "stream_read_GBps": stream_gbs, "fraction_of_stream_read": gbs / stream_gbs})
        report(r)

    def tiles_of(row):
        return TILES if "f" in a.rows else (0,) if row in a.rows else ()

    def with_tile(t, row, label, *args, **kw):
        assert lib.rbx_tune(b"bitgroups_tile", t) == 0
        compare(row if t == 0 else "f", label + ("" if t == 0 else ", bitgroups_tile %d" % t), *args,
                extra={"knob": t, "shape": row}, **kw)
        assert lib.rbx_tune(b"bitgroups_tile", 0) == 0

    # ---- a: cohort sizes ----
    if tiles_of("a"):
        n, nb = sc(10_000), 128 << 10
        names = make("a", 200, nb) + ["bench:bg:a:tmp"]
        pairs = rng.integers(0, 200, size=(n, 2))
        grouped = grouped_call(names, [AND] * n, [None] * n, pairs, 2)
        base = op_loop(names, [AND] * n, [200] * n, pairs, 2, count=True)
        for t in tiles_of("a"):
            with_tile(t, "a", "%d ANDs of 2 x 128 KiB, counted, stored nowhere" % n, grouped, base,
                      "a loop of rbx_bitset_op into a temporary + rbx_bitset_cardinality", read_bytes=2 * n * nb)
        for nm in names:
            client.getBitSet(nm).delete()

    # ---- b: hourly into daily ----
    if "b" in a.rows:
        n, per = sc(5000), 24
        src = make("b", 2000, 4096)
        d1 = ["bench:bg:b:g%05d" % i for i in range(n)]
        d2 = ["bench:bg:b:l%05d" % i for i in range(n)]
        names = src + d1 + d2
        srcs = rng.integers(0, 2000, size=(n, per))
        grouped = grouped_call(names, [OR] * n, list(range(2000, 2000 + n)), srcs, per)
        base = op_loop(names, [OR] * n, list(range(2000 + n, 2000 + 2 * n)), srcs, per)
        arrs = [L.names_array(d1), L.names_array(d2)]

        def fresh(which):
            deleted = C.c_int()
            assert lib.rbx_del_n(ctx, arrs[which][0], n, C.byref(deleted)) == 0
        compare("b", "%d independent ORs of %d x 4 KiB into fresh destinations" % (n, per), grouped, base,
                "a loop of rbx_bitset_op", before=(lambda: fresh(0), lambda: fresh(1)), same_counts=False)
        got = [client.getBitSet(d1[i]).toByteArray() == client.getBitSet(d2[i]).toByteArray() for i in (0, n // 2, n - 1)]
        assert all(got), "the grouped call and the loop disagree"
        for nm in names:
            client.getBitSet(nm).delete()

    # ---- c: BITCOUNT of each key ----
    if "c" in a.rows:
        n = sc(10_000)
        names = make("c", n, 4096)
        grouped = grouped_call(names, [OR] * n, [None] * n, np.arange(n), 1)
        one = [L.name_struct(nm) for nm in names]
        outs = (C.c_uint64 * n)()

        def loop():
            for g in range(n):
                rc = lib.rbx_bitset_cardinality(ctx, one[g][0], C.cast(C.byref(outs, 8 * g), L.u64p))
                assert rc == 0, L.last_error()
        loop.counts = np.frombuffer(outs, np.uint64)
        compare("c", "BITCOUNT of each of %d keys of 4 KiB" % n, grouped, loop, "a loop of rbx_bitset_cardinality")
        # (the keys stay for row g)

    # ---- g: the chain ----
    if "g" in a.rows:
        n = sc(1000)
        names = make("g", n + 1, 4096)
        chain = np.stack([np.arange(n), np.arange(n) + 1], axis=1)
        grouped = grouped_call(names, [OR] * n, list(range(1, n + 1)), chain, 2)
        base = op_loop(names, [OR] * n, list(range(1, n + 1)), chain, 2)
        compare("g", "a chain of %d dependent ORs of 4 KiB" % n, grouped, base, "a loop of rbx_bitset_op",
                same_counts=False)  # (an OR chain is idempotent: the repetitions change nothing after the first)

    # ---- d: large groups ----
    if tiles_of("d"):
        nb = sc(1 << 20)
        src = make("d", 64, nb)
        for n in (1, 16, 256):
            dg = ["bench:bg:d:g%03d" % i for i in range(n)]
            dl = ["bench:bg:d:l%03d" % i for i in range(n)]
            names = src + dg + dl
            pairs = rng.integers(0, 64, size=(n, 2))
            grouped = grouped_call(names, [AND] * n, list(range(64, 64 + n)), pairs, 2, counted=False)
            base = op_loop(names, [AND] * n, list(range(64 + n, 64 + 2 * n)), pairs, 2)
            for t in tiles_of("d"):
                with_tile(t, "d", "%d ANDs of 2 x 1 MiB into destinations" % n, grouped, base, "a loop of rbx_bitset_op",
                          same_counts=False)
            assert client.getBitSet(dg[-1]).toByteArray() == client.getBitSet(dl[-1]).toByteArray()
            for nm in dg + dl:
                client.getBitSet(nm).delete()
        for nm in src:
            client.getBitSet(nm).delete()

    # ---- e: one very large group ----
    if tiles_of("e"):
        nb = sc(512 << 20)
        names = make("e", 2, nb) + ["bench:bg:e:g", "bench:bg:e:l"]
        grouped = grouped_call(names, [AND], [2], [[0, 1]], 2, counted=False)  # (the single call counts nothing either)
        base = op_loop(names, [AND], [3], [[0, 1]], 2)
        for t in tiles_of("e"):
            with_tile(t, "e", "one AND of 2 x %d MiB into a destination" % (nb >> 20), grouped, base, "one rbx_bitset_op",
                      same_counts=False, read_bytes=2 * nb)
        counted = grouped_call(names, [AND], [2], [[0, 1]], 2)
        if "e" in a.rows:
            compare("e", "the same, counted as well", counted, base, "one rbx_bitset_op (which does not count)",
                    same_counts=False, read_bytes=2 * nb)
        else:
            counted()
        assert client.getBitSet(names[2]).cardinality() == client.getBitSet(names[3]).cardinality() == int(counted.counts[0])

    doc = {"bench": "bitgroups", "device": torch.cuda.get_device_name(0),
           "timing": "host clock around the call, final wait included; grouped call and baseline alternate",
           "bar": "rows a - d and g: the grouped call's median below the loop's minimum; row e: within the single "
                  "call's min - max spread", "results": []}
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
