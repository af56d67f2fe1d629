#!/usr/bin/env python3
"""RBitSet packed counters (BITFIELD batches over device arrays) against the bit-set batches of the
same shape, in one process on one MI355X.  The counter array is a 128 MiB string: 2^26 u16 slots.

  a  incrementFieldsDev u16, no replies, uniform random slots (one atomic compare-and-swap loop per
     element)                        vs setIndexesDev of as many random indexes on the same bitmap
  b  the same increments with replies (sort by slot + one lane per slot)          vs row a
  c  getFieldsDev u16 at the same offsets                    vs getIndexesDev of as many indexes
  d  2^20 increments with replies that all hit ONE slot (one lane walks them all)
                                     vs a duplicate-free batch of the same size, with replies

Each figure is a call time: a host clock around the call and the stream synchronise that ends it
(every *_dev call here waits once for its batch check; that is part of the call).  Operation and
baseline alternate inside one loop; the median of the repetitions is reported.  `ratio` = the
operation's time over its baseline's (above 1: slower than the baseline).  Writes one JSON document
(default profiles/bitset/bitfield_bench.json).

--overflow measures OVERFLOW SAT instead, for u4 and u16 counters over the same 128 MiB, each
row from a freshly imported string, and writes profiles/bitset/bitfield_overflow_bench.json:

  e  SAT +1 on an all-zero string, re-imported before every call, no replies (k_fields_incr_sat; nothing
     saturates)
                                     vs WRAP incrementFieldsDev of the same arrays (row a's path)
  f  SAT +1 on a string whose counters all sit at the maximum (every element a load, no atomic)   vs row e
  g  SAT with increments of both signs, no replies (the grouped path)
                                     vs WRAP with replies (the grouped path, row b's)

Row e carries a bound: the baseline's median plus the baseline's own spread (p90 - p10 of its calls); the
document says whether the operation's median lies within it.  Rows f and g carry none.

--only b runs row b's operation alone, for a kernel trace that splits it into its sort and apply
parts (rocprofv3 --kernel-trace --stats -- python tools/bitfield_bench.py --only b): the sort is
k_fields_slots plus rocPRIM's kernels, the apply is k_fields_runs.  --kernel-split SORT_MS APPLY_MS
records the per-call figures read from that trace in the JSON document.
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

import torch  # noqa: E402

from redisson_amd import RedissonClient  # noqa: E402
from redisson_amd import _lib as L  # noqa: E402

NBYTES = 1 << 27  # 2^30 bits
SIZE = 16
SLOTS = NBYTES * 8 // SIZE  # 2^26


def overflow_rows(a):
    """rows e-g: the saturating paths against the wrapping ones, operation and baseline alternating"""
    client = RedissonClient(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB17F1E1D)
    n = a.n
    names = ("bench:sat", "bench:wrap")
    sat, wrap = (client.getBitSet(nm) for nm in names)

    bufs = {b: torch.full((NBYTES,), b, dtype=torch.uint8, device="cuda") for b in (0, 0xFF)}
    torch.cuda.synchronize()

    def fill(nm, byte):
        assert L.lib().rbx_bloom_import_dev(client.ctx, nm.encode(), bufs[byte].data_ptr(), NBYTES, None) == 0
        client.synchronize()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    rows = []
    for size in (4, 16):
        slots = NBYTES * 8 // size
        offs = torch.randint(0, slots, (n,), dtype=torch.int64, device="cuda", generator=g) * size
        ones = torch.ones(n, dtype=torch.int64, device="cuda")
        signs = torch.randint(0, 2, (n,), dtype=torch.int64, device="cuda", generator=g) * 2 - 1
        rep = torch.empty(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def run(bs, vals, replies, overflow):
            bs.incrementFieldsDev(size, offs.data_ptr(), vals.data_ptr(), n, rep.data_ptr() if replies else None,
                                  signed=False, overflow=overflow)
            client.synchronize()

        def sat_ones():
            run(sat, ones, False, "SAT")

        def wrap_ones():
            run(wrap, ones, False, "WRAP")

        def sat_full():  # the string under bench:wrap here: every counter at its maximum
            run(wrap, ones, False, "SAT")

        def sat_mixed():
            run(sat, signs, False, "SAT")

        def wrap_replies():
            run(wrap, signs, True, "WRAP")

        for row, label, op, base_label, base, start in (
                ("e", "SAT +1, no replies, all-zero string (atomic)", sat_ones, "WRAP, the same arrays (row a's path)",
                 wrap_ones, (0, 0)),
                ("f", "SAT +1, no replies, every counter at its maximum (loads only)", sat_full, "row e", sat_ones,
                 (0, 0xFF)),
                ("g", "SAT, both signs, no replies (grouped)", sat_mixed, "WRAP with replies (grouped, row b's path)",
                 wrap_replies, (0, 0))):
            fill(names[0], start[0])
            fill(names[1], start[1])
            assert sat.size() == 8 * NBYTES and wrap.size() == 8 * NBYTES
            t_op, t_base = [], []
            for i in range(a.warmup + a.reps):
                if row != "g":  # the same arrays every call would saturate the u4 counters by the 15th: start afresh
                    fill(names[0], 0)
                x, y = clock(op), clock(base)
                if i >= a.warmup:
                    t_op.append(x)
                    t_base.append(y)
            m_op, m_base = statistics.median(t_op), statistics.median(t_base)
            q = statistics.quantiles(t_base, n=10)
            r = {"row": row, "field": "u%d" % size, "operation": label, "elements": n, "slots": slots,
                 "call_ms_median": m_op * 1e3, "call_ms_min": min(t_op) * 1e3, "call_ms_max": max(t_op) * 1e3,
                 "M_elements_per_s": n / m_op / 1e6, "baseline": base_label, "baseline_ms_median": m_base * 1e3,
                 "baseline_ms_min": min(t_base) * 1e3, "baseline_ms_max": max(t_base) * 1e3,
                 "baseline_ms_p10": q[0] * 1e3, "baseline_ms_p90": q[-1] * 1e3, "ratio": m_op / m_base, "reps": a.reps}
            if row == "e":
                r["bound_ms"] = (m_base + q[-1] - q[0]) * 1e3
                r["within"] = "yes" if m_op * 1e3 <= r["bound_ms"] else "no"
            rows.append(r)
            print(json.dumps(r), flush=True)
    doc = {"bench": "bitfield_overflow", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call + stream synchronise", "counter_array_bytes": NBYTES,
           "bound": "row e: baseline median + (baseline p90 - p10)", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sat.delete()
    wrap.delete()
    client.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 24, help="elements per batch of rows a-c")
    ap.add_argument("--only", choices=["b"], default=None)
    ap.add_argument("--kernel-split", type=float, nargs=2, metavar=("SORT_MS", "APPLY_MS"), default=None)
    ap.add_argument("--overflow", action="store_true", help="rows e-g (OVERFLOW SAT) instead of rows a-d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bitset",
                             "bitfield_overflow_bench.json" if a.overflow else "bitfield_bench.json")
    if a.overflow:
        return overflow_rows(a)

    client = RedissonClient(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB17F1E1D)
    zeros = torch.zeros(NBYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.lib().rbx_bloom_import_dev(client.ctx, b"bench:counters", zeros.data_ptr(), NBYTES, None) == 0
    del zeros
    bs = client.getBitSet("bench:counters")
    assert bs.size() == 8 * NBYTES

    n, nd = a.n, 1 << 20
    slots = torch.randint(0, SLOTS, (n,), dtype=torch.int64, device="cuda", generator=g)
    offs = slots * SIZE  # field offsets; as raw bit indexes for the set/getIndexes baselines
    ones = torch.ones(n, dtype=torch.int64, device="cuda")
    rep = torch.empty(n, dtype=torch.int64, device="cuda")
    bits = torch.empty(n, dtype=torch.uint8, device="cuda")
    one_slot = torch.full((nd,), 12345 * SIZE, dtype=torch.int64, device="cuda")
    distinct = torch.randperm(SLOTS, device="cuda", generator=g)[:nd].to(torch.int64) * SIZE
    torch.cuda.synchronize()

    def incr():
        bs.incrementFieldsDev(SIZE, offs.data_ptr(), ones.data_ptr(), n, None, signed=False)
        client.synchronize()

    def incr_replies():
        bs.incrementFieldsDev(SIZE, offs.data_ptr(), ones.data_ptr(), n, rep.data_ptr(), signed=False)
        client.synchronize()

    def set_indexes():
        bs.setIndexesDev(offs.data_ptr(), n, True)
        client.synchronize()

    def get_fields():
        bs.getFieldsDev(SIZE, offs.data_ptr(), n, rep.data_ptr(), signed=False)
        client.synchronize()

    def get_indexes():
        bs.getIndexesDev(offs.data_ptr(), n, bits.data_ptr())
        client.synchronize()

    def incr_one_slot():
        bs.incrementFieldsDev(SIZE, one_slot.data_ptr(), ones.data_ptr(), nd, rep.data_ptr(), signed=False)
        client.synchronize()

    def incr_distinct():
        bs.incrementFieldsDev(SIZE, distinct.data_ptr(), ones.data_ptr(), nd, rep.data_ptr(), signed=False)
        client.synchronize()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    if a.only == "b":
        for _ in range(a.warmup + a.reps):
            incr_replies()
        client.shutdown()
        return

    rows = []
    for row, label, op, n_op, base_label, base in (
            ("a", "incrementFieldsDev u16, no replies (atomic)", incr, n, "setIndexesDev", set_indexes),
            ("b", "incrementFieldsDev u16, replies (grouped)", incr_replies, n, "row a", incr),
            ("c", "getFieldsDev u16", get_fields, n, "getIndexesDev", get_indexes),
            ("d", "incrementFieldsDev u16, replies, one slot", incr_one_slot, nd,
             "the same, duplicate-free", incr_distinct)):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x, y = clock(op), clock(base)
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        rows.append({"row": row, "operation": label, "elements": n_op, "slots": SLOTS,
                     "call_ms_median": m_op * 1e3, "call_ms_min": min(t_op) * 1e3, "call_ms_max": max(t_op) * 1e3,
                     "M_elements_per_s": n_op / m_op / 1e6,
                     "baseline": base_label, "baseline_ms_median": m_base * 1e3, "baseline_ms_min": min(t_base) * 1e3,
                     "baseline_ms_max": max(t_base) * 1e3, "ratio": m_op / m_base, "reps": a.reps})
        if row == "b" and a.kernel_split:
            rows[-1]["kernel_ms_sort"], rows[-1]["kernel_ms_apply"] = a.kernel_split
        print(json.dumps(rows[-1]), flush=True)
    doc = {"bench": "bitfield", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call + stream synchronise", "counter_array_bytes": NBYTES, "field": "u16",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bs.delete()
    client.shutdown()


if __name__ == "__main__":
    main()
