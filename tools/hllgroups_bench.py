#!/usr/bin/env python3
"""Grouped PFCOUNT unions and PFMERGEs (rbx_hll_count_groups, rbx_hll_merge_groups) against loops of the single
calls, in one process on one MI355X.  The keys are 10,000 warm dense HLLs (16 KiB of registers each, 164 MB).

  a  10,000 sliding-window unions of 24 members (window g = keys g .. g + 23), one rbx_hll_count_groups call
  b  the same unions by a loop of rbx_hll_count_n: the single-call path, the baseline of row a
  c  1, 16, 256, 4,096 and 10,000 such unions under hllgroups_split auto and every P, each against the loop of
     rbx_hll_count_n: where the auto rule's threshold belongs
  d  1 union of 10,000 members                                     vs one rbx_hll_count_n of the same keys
  e  5,000 independent merges of 2 sources into dense destinations, one rbx_hll_merge_groups call
                                                                   vs a loop of rbx_hll_merge_n
  f  a chain of 1,000 dependent merges (k[i + 1] <- k[i]): every group is its own phase, the planner's worst case
                                                                   vs the same loop

Each figure is a call time: a host clock around the call (both sides wait for the device themselves), arrays and
names built beforehand.  The median of the repetitions after the warm-ups is reported; a loop is repeated
--loop-reps times and its min and max are its run-to-run spread.  `ratio` = the grouped call's time over the
loop's.  Rows a and d also give the bytes of member registers read per second beside the stream-read rate of
rbx_bench_stream_read from the same run.  --rows picks rows; the results of earlier runs stay in the JSON document
(default profiles/hll/hllgroups_bench.json).
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

REG_BYTES = 16384


def dense_string(rng) -> bytes:
    """a dense HLL string of random registers 0..40 (6 bits each, LSB first)"""
    regs = rng.integers(0, 41, size=16384).astype(np.uint64)
    bits = ((regs[:, None] >> np.arange(6, dtype=np.uint64)) & 1).astype(np.uint8).reshape(-1)
    return b"HYLL" + bytes([0, 0, 0, 0]) + (1 << 63).to_bytes(8, "little") + np.packbits(bits, bitorder="little").tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=10_000)
    ap.add_argument("--members", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="abcdef")
    ap.add_argument("--no-loops", action="store_true", help="skip the loops of single calls (counter collection runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hll", "hllgroups_bench.json"))
    a = ap.parse_args()
    nkeys, members = a.keys, a.members

    import torch

    client = RedissonClient(0)
    lib, ctx = L.lib(), client.ctx
    rng = np.random.default_rng(0x6A0F5)
    names = ["bench:hg:%05d" % i for i in range(nkeys)]
    strings = [dense_string(rng) for _ in range(64)]
    for i, name in enumerate(names):
        client.getHyperLogLog(name).importString(strings[i % 64])
    names_arr, _keep = L.names_array(names)
    one = [L.name_struct(n) for n in names]  # (rbx_name, keep-alive) per key
    rows = []

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def hook():
        out = (C.c_uint32 * 4)()
        lib.rbx_bench_hllgroups_last(out)
        return dict(zip(("phases", "launches", "split", "device_groups"), list(out)))

    def times(fn, reps, warmup):
        return [clock(fn) for _ in range(warmup + reps)][warmup:]

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

    # ---- shapes ----
    def windows(ngroups):
        off = (np.arange(ngroups + 1, dtype=np.uint64) * members).astype(np.uint64)
        key = ((np.arange(ngroups, dtype=np.uint64)[:, None] + np.arange(members, dtype=np.uint64)[None, :]) % nkeys)
        return off, key.astype(np.uint32).reshape(-1)

    def count_groups_call(off, key, ngroups):
        """the call over the names its groups use, as a batch hands them over: the keys 0 .. max(key)"""
        out, status = np.zeros(ngroups, np.uint64), np.zeros(ngroups, np.uint8)
        used = int(key.max()) + 1
        used_arr, keep = L.names_array(names[:used])

        def run():
            rc = lib.rbx_hll_count_groups(ctx, used_arr, used, off.ctypes.data_as(L.u64p), key.ctypes.data_as(L.u32p),
                                          ngroups, out.ctypes.data_as(L.u64p), status.ctypes.data_as(L.u8p))
            assert rc == 0, L.last_error()
        run.out, run.keep = out, keep
        return run

    def count_loop(key, ngroups, per_group):
        arrs = [L.names_array([names[k] for k in key[g * per_group:(g + 1) * per_group].tolist()]) for g in range(ngroups)]
        outs = (C.c_uint64 * ngroups)()

        def run():
            for g in range(ngroups):
                rc = lib.rbx_hll_count_n(ctx, arrs[g][0], per_group, C.cast(C.byref(outs, 8 * g), L.u64p))
                assert rc == 0, L.last_error()
        run.out = np.frombuffer(outs, np.uint64)
        return run

    def compare(row, label, ngroups, per_group, op, base_label, base, extra=None, read_rate=False):
        t_op = times(op, a.reps, a.warmup)
        took = hook()
        if a.no_loops:
            report({"row": row, "operation": label, "groups": ngroups, "members": per_group, **stats("call", t_op),
                    "reps": a.reps, **took, "note": "loops skipped: not a comparison"})
            return
        if not hasattr(base, "times"):  # a loop shared by several rows is timed once
            base.times = times(base, a.loop_reps, 1)
        t_base = base.times
        assert np.array_equal(op.out, base.out), "the grouped call and the loop disagree"
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        r = {"row": row, "operation": label, "groups": ngroups, "members": per_group, **stats("call", t_op), "reps": a.reps,
             **took, "baseline": base_label, **stats("baseline", t_base), "baseline_reps": a.loop_reps,
             "ratio": m_op / m_base, "faster": "yes" if m_op < m_base else "no",
             "within_baseline_spread": "yes" if m_op <= max(t_base) else "no", **(extra or {})}
        if read_rate:
            gbs = ngroups * per_group * REG_BYTES / m_op / 1e9
            r.update({"member_read_GBps": gbs, "stream_read_GBps": stream_gbs, "fraction_of_stream_read": gbs / stream_gbs,
                      "distinct_member_bytes": min(nkeys, ngroups + per_group - 1) * REG_BYTES})
        report(r)
        if row == "a":
            report({"row": "b", "operation": "the same unions by a loop of rbx_hll_count_n", "groups": ngroups,
                    "members": per_group, **stats("call", t_base), "reps": a.loop_reps})

    if "a" in a.rows or "b" in a.rows:
        off, key = windows(nkeys)
        compare("a", "%d sliding-window unions, one rbx_hll_count_groups call" % nkeys, nkeys, members,
                count_groups_call(off, key, nkeys), "row b: a loop of rbx_hll_count_n", count_loop(key, nkeys, members),
                read_rate=True)
    if "c" in a.rows:
        for ngroups in (1, 16, 256, 4096, nkeys):
            off, key = windows(ngroups)
            base = count_loop(key, ngroups, members)
            for p in (0, 1, 2, 4, 8, 16):
                assert lib.rbx_tune(b"hllgroups_split", p) == 0
                compare("c", "%d unions, hllgroups_split %s" % (ngroups, p or "auto"), ngroups, members,
                        count_groups_call(off, key, ngroups), "a loop of rbx_hll_count_n", base, {"knob": p})
            assert lib.rbx_tune(b"hllgroups_split", 0) == 0
    if "d" in a.rows:
        off = np.array([0, nkeys], np.uint64)
        key = np.arange(nkeys, dtype=np.uint32)
        compare("d", "1 union of %d members" % nkeys, 1, nkeys, count_groups_call(off, key, 1),
                "one rbx_hll_count_n of the same keys", count_loop(key, 1, nkeys), read_rate=True)

    def merge_rows(row, label, dests, srcs, per_group):
        """dests[g] <- srcs[g * per_group ..]: the grouped call against the loop; both leave the same registers (a
        merge is idempotent, so the repetitions change nothing after the first)"""
        n = len(dests)
        dest = np.asarray(dests, np.uint32)
        off = (np.arange(n + 1, dtype=np.uint64) * per_group).astype(np.uint64)
        key = np.asarray(srcs, np.uint32)
        status = np.zeros(n, np.uint8)
        arrs = [L.names_array([names[k] for k in key[g * per_group:(g + 1) * per_group].tolist()]) for g in range(n)]

        def grouped():
            rc = lib.rbx_hll_merge_groups(ctx, names_arr, nkeys, dest.ctypes.data_as(L.u32p), off.ctypes.data_as(L.u64p),
                                          key.ctypes.data_as(L.u32p), n, status.ctypes.data_as(L.u8p))
            assert rc == 0, L.last_error()

        def loop():
            for g in range(n):
                rc = lib.rbx_hll_merge_n(ctx, one[int(dest[g])][0], arrs[g][0], per_group)
                assert rc == 0, L.last_error()

        t_op = times(grouped, a.reps, a.warmup)
        took = hook()
        if a.no_loops:
            return
        t_base = times(loop, a.loop_reps, 1)
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        report({"row": row, "operation": label, "groups": n, "members": per_group, **stats("call", t_op), "reps": a.reps,
                **took, "baseline": "a loop of rbx_hll_merge_n", **stats("baseline", t_base), "baseline_reps": a.loop_reps,
                "ratio": m_op / m_base, "faster": "yes" if m_op < m_base else "no",
                "within_baseline_spread": "yes" if m_op <= max(t_base) else "no"})

    if "e" in a.rows:
        n = min(5000, nkeys // 2)  # destinations 0 .. n - 1, sources among the n keys after them: independent
        srcs = np.stack([np.arange(n) + n, (np.arange(n) + 1) % n + n], axis=1).reshape(-1)
        merge_rows("e", "%d independent merges of 2 sources, one rbx_hll_merge_groups call" % n, np.arange(n), srcs, 2)
    if "f" in a.rows:
        n = min(1000, nkeys - 1)
        merge_rows("f", "a chain of %d dependent merges, one rbx_hll_merge_groups call" % n, np.arange(n) + 1, np.arange(n), 1)

    doc = {"bench": "hllgroups", "device": torch.cuda.get_device_name(0), "timing": "host clock around the call",
           "keys": nkeys, "members": members,
           "bar": "grouped faster than the loop on rows a, c from 16 groups up, d and e; within the loop's spread on the "
                  "one-group row of c and on f", "results": []}
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
