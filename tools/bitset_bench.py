#!/usr/bin/env python3
"""RBitSet stream operations against the runtime's own streams, in one process on one MI355X.

  or_       two 512 MiB bit sets, A |= B          vs hipMemcpyAsync device-to-device of 512 MiB
  not_      one 512 MiB bit set,  A = ~A          vs the same copy
  setRange  bits [0, 2^32) of a 512 MiB string    vs hipMemsetAsync of 512 MiB

Each figure is a call time: a host clock around the call and the stream synchronise that ends it
(the BITOP calls first read their operands' lengths back, one wait; that is part of the call).
Operation and baseline alternate inside one loop; the median of the repetitions is reported.  Rates
count the bytes that cross HBM: or_ reads two strings and writes one (3 streams), not_ and the copy
read one and write one (2), setRange and the fill write one (1).  `ratio` = the operation's byte
rate over its baseline's.  Writes one JSON document (default profiles/bitset/bitset_bench.json).
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

NBYTES = 1 << 29  # the largest Redis string: 2^32 bits


def hip_runtime() -> C.CDLL:
    """The HIP runtime this process already runs on (torch's when torch is installed)."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "bitset_bench.json"))
    a = ap.parse_args()

    client = RedissonClient(0)
    hip = hip_runtime()
    st = client.stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB175E7)
    src = torch.randint(0, 256, (NBYTES,), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for name in ("bench:A", "bench:B"):
        assert L.lib().rbx_bloom_import_dev(client.ctx, name.encode(), src.data_ptr(), NBYTES, None) == 0
    A = client.getBitSet("bench:A")
    assert A.size() == 8 * NBYTES

    def sync():
        assert hip.hipStreamSynchronize(st) == 0

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), NBYTES, 3, st) == 0  # hipMemcpyDeviceToDevice
        sync()

    def fill():
        assert hip.hipMemsetAsync(dst.data_ptr(), 0, NBYTES, st) == 0
        sync()

    def op_or():
        A.or_("bench:B")
        sync()

    def op_not():
        A.not_()
        sync()

    def op_range():
        A.setRange(0, 8 * NBYTES, True)
        sync()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    rows = []
    for label, op, op_streams, base_label, base, base_streams in (
            ("or_", op_or, 3, "hipMemcpyAsync D2D", copy, 2),
            ("not_", op_not, 2, "hipMemcpyAsync D2D", copy, 2),
            ("setRange", op_range, 1, "hipMemsetAsync", fill, 1)):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x, y = clock(op), clock(base)
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        m_op, m_base = statistics.median(t_op), statistics.median(t_base)
        r_op, r_base = op_streams * NBYTES / m_op, base_streams * NBYTES / m_base
        rows.append({"operation": label, "bytes_per_string": NBYTES, "streams": op_streams,
                     "call_ms_median": m_op * 1e3, "call_ms_min": min(t_op) * 1e3, "call_ms_max": max(t_op) * 1e3,
                     "GB_per_s": r_op / 1e9,
                     "baseline": base_label, "baseline_streams": base_streams,
                     "baseline_ms_median": m_base * 1e3, "baseline_ms_min": min(t_base) * 1e3,
                     "baseline_ms_max": max(t_base) * 1e3, "baseline_GB_per_s": r_base / 1e9,
                     "ratio": r_op / r_base, "reps": a.reps})
        print(json.dumps(rows[-1]), flush=True)
    assert A.cardinality() == 8 * NBYTES  # the last operation set every bit
    doc = {"bench": "bitset", "device": torch.cuda.get_device_name(0), "timing": "host clock, call + stream synchronise",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    A.delete()
    client.getBitSet("bench:B").delete()
    client.shutdown()


if __name__ == "__main__":
    main()
