#!/usr/bin/env python3
"""Ranged BITCOUNT / BITPOS on a 512 MiB string against BITCOUNT of the whole string (rbx_bitset_cardinality),
in one process on one MI355X.

  scans     bitCount(0, -1); bitPos(1) on an all-zero string (a full scan); bitPos(1) with the only set bit in the
            first chunk (the early exit) -- the searches at bitrange_pos_chunk 64 KiB, 256 KiB and 1 MiB
  batches   2^20 queries over device arrays, ranges of 64 bytes, 4 KiB and 1 MiB at random offsets, on the direct
            path (bitrange_dir 0) and through the block directory (1); counts on a random string, searches for
            a set bit on the all-zero one (every range is walked to its end)

Each figure is a call time: a host clock around the call and the stream synchronise that ends it.  A scan and
its baseline -- cardinality() of the same string, which moves the same bytes -- alternate inside one loop; the
median of the repetitions is reported, with the baseline's own spread (p90 - p10).  `within` says whether the
scan took no longer than the baseline's median plus that spread.  Two one-byte calls show what a call costs
before it reads anything.  A batch alternates with the same baseline and reports its median over the same
number of repetitions and the bytes its clamped ranges cover.  Writes one JSON document (default
profiles/bitset/bitrange_bench.json).
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

NBYTES = 1 << 29  # the largest Redis string: 2^32 bits
NQ = 1 << 20
DEFAULT_CHUNK = 256 << 10


def tune(key: str, value: int) -> None:
    assert L.lib().rbx_tune(key.encode(), value) == 0, (key, value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-batches", action="store_true", help="the scans only")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunks", default="65536,262144,1048576", help="bitrange_pos_chunk values for the searches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "bitrange_bench.json"))
    a = ap.parse_args()
    chunks = [int(x) for x in a.chunks.split(",")]

    client = RedissonClient(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB17A)
    src = torch.randint(0, 256, (NBYTES,), dtype=torch.uint8, device="cuda", generator=g)
    zero = torch.zeros(NBYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for name, t in (("bench:R", src), ("bench:Z", zero)):
        assert L.lib().rbx_bloom_import_dev(client.ctx, name.encode(), t.data_ptr(), NBYTES, None) == 0
    del zero
    R, Z = client.getBitSet("bench:R"), client.getBitSet("bench:Z")
    ones = R.cardinality()

    def clock(fn):
        t0 = time.perf_counter()
        r = fn()
        client.synchronize()
        return time.perf_counter() - t0, r

    def pct(xs, q):
        xs = sorted(xs)
        return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]

    rows = []

    def scan(label, bs, op, want, **note):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            (x, r), (y, _) = clock(op), clock(bs.cardinality)
            assert r == want, (label, r, want)
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        spread = pct(t_base, 0.9) - pct(t_base, 0.1)
        rows.append({"operation": label, "bytes": NBYTES, "call_ms_median": m_op * 1e3, "call_ms_min": min(t_op) * 1e3,
                     "call_ms_max": max(t_op) * 1e3, "GB_per_s": NBYTES / m_op / 1e9,
                     "baseline": "cardinality() of the same string", "baseline_ms_median": m_base * 1e3,
                     "baseline_ms_p10": pct(t_base, 0.1) * 1e3, "baseline_ms_p90": pct(t_base, 0.9) * 1e3,
                     "baseline_spread_ms": spread * 1e3, "bound_ms": (m_base + spread) * 1e3,
                     "within": m_op <= m_base + spread, "reps": a.reps, **note})
        print(json.dumps(rows[-1]), flush=True)

    scan("bitCount(0, -1), random string", R, lambda: R.bitCount(0, -1), ones)
    cut = bin(int(src[0]) >> 5).count("1") + bin(int(src[-1]) & 0x1F).count("1")  # bits 0..2 and the last five
    scan("bitCount(3, 2^32 - 6, BIT), random string: both masks", R, lambda: R.bitCount(3, 8 * NBYTES - 6, "BIT"),
         ones - cut)
    # one vector of the same strings: what a call costs before it reads anything (launches, the wait, the reply's
    # way back); the baseline column is still cardinality() of the whole string
    scan("bitCount(0, 0), random string: one byte", R, lambda: R.bitCount(0, 0), bin(int(src[0])).count("1"))
    scan("bitPos(1, 0, 0), all-zero string: one byte", Z, lambda: Z.bitPos(1, 0, 0), -1)
    for chunk in chunks:
        tune("bitrange_pos_chunk", chunk)
        scan("bitPos(1), all-zero string: full scan", Z, lambda: Z.bitPos(1), -1, bitrange_pos_chunk=chunk)
    Z.set(1000, True)
    for chunk in chunks:
        tune("bitrange_pos_chunk", chunk)
        scan("bitPos(1), only bit 1000 set: early exit", Z, lambda: Z.bitPos(1), 1000, bitrange_pos_chunk=chunk)
    tune("bitrange_pos_chunk", DEFAULT_CHUNK)
    Z.set(1000, False)

    # ---- batches over device arrays ----
    d_out = torch.zeros(NQ, dtype=torch.int64, device="cuda")
    for width in () if a.no_batches else (64, 4096, 1 << 20):
        starts = torch.randint(0, NBYTES - width, (NQ,), dtype=torch.int64, device="cuda", generator=g)
        ends = starts + (width - 1)
        torch.cuda.synchronize()
        first = {}
        for kind, bs in (("countRanges", R), ("posRanges(1)", Z)):
            for use_dir in (0, 1):
                tune("bitrange_dir", use_dir)

                def op():
                    if kind == "countRanges":
                        bs.countRangesDev(starts.data_ptr(), ends.data_ptr(), NQ, d_out.data_ptr())
                    else:
                        bs.posRangesDev(1, starts.data_ptr(), ends.data_ptr(), NQ, d_out.data_ptr())

                ts, t_base = [], []
                for i in range(a.warmup + a.reps):
                    (t, _), (y, _) = clock(op), clock(bs.cardinality)
                    if i >= a.warmup:
                        ts.append(t)
                        t_base.append(y)
                got = d_out.clone()
                if kind in first:
                    assert torch.equal(got, first[kind]), (kind, width)  # both paths answer the same
                first[kind] = got
                m = statistics.median(ts)
                rows.append({"operation": f"{kind}, {NQ} ranges of {width} bytes", "bitrange_dir": use_dir,
                             "range_bytes_total": NQ * width, "string_bytes": NBYTES, "call_ms_median": m * 1e3,
                             "call_ms_min": min(ts) * 1e3, "call_ms_max": max(ts) * 1e3,
                             "queries_per_us": NQ / m / 1e6, "range_GB_per_s": NQ * width / m / 1e9,
                             "baseline": "cardinality() of the same string",
                             "baseline_ms_median": statistics.median(t_base) * 1e3, "reps": a.reps})
                print(json.dumps(rows[-1]), flush=True)
    tune("bitrange_dir", 2)

    doc = {"bench": "bitrange", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call + stream synchronise", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    R.delete()
    Z.delete()
    client.shutdown()


if __name__ == "__main__":
    main()
