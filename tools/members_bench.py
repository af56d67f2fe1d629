#!/usr/bin/env python3
"""Set-bit enumeration and the java.util.BitSet exchange (rbx_bitset_members*, rbx_bitset_as_words / _set_words)
against what the engine offered before, in one process on one MI355X.

  a  members() of a 512 MiB string with 10^6 random ones          vs rbx_bitset_cardinality, and the count-only call
  b  the same length at fill 1/2, cap = 2^24, skip 0 and near the end   vs rbx_bitset_set_range of the whole string
  c  row a's string by the two older routes: toByteArray() + np.flatnonzero(np.unpackbits()) (once), and a loop of
     bitPos(1, next, -1, "BIT") for the first 1,000 members (per member)
  d  100,000 strings of 46 bytes, all members in one rbx_bitset_members_stream_dev
                                  vs rbx_bitset_range_stream_dev BITCOUNTs of the same keys, and 1,000 single members()
  e  asBitSetDev of 512 MiB and setBitSetDev of 256 MiB           vs a device-to-device copy of the same bytes
  f  members_lanes on row d's batch; members_short_max x members_tile on 9,900 46-byte keys and 100 commands on 8 MiB keys

Each figure is a call time: a host clock around the call (the loop of calls) and the stream synchronise that ends it.
Operation and baseline alternate inside one loop; the median of the repetitions is reported, with the baseline's
p10 and p90.  Writes one JSON document (default profiles/bitset/members_bench.json).
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
from redisson_amd.client import _members_cmds_array, _range_cmds_array  # noqa: E402

USERS, USER_BYTES = 100_000, 46
DEFAULTS = {"members_lanes": 16, "members_short_max": 4096, "members_tile": 65536}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abcdef")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "members_bench.json"))
    a = ap.parse_args()

    client = RedissonClient(0)
    lib = L.lib()
    rng = np.random.default_rng(0x3E3B)
    rows = []

    def tune(**knobs):
        for k, v in knobs.items():
            assert lib.rbx_tune(k.encode(), v) == 0, (k, v)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def measure(row, label, op, bases=(), reps=None, **extra):
        """op and every (label, fn) of bases alternate in one loop"""
        reps = a.reps if reps is None else reps
        t = [[] for _ in range(1 + len(bases))]
        for i in range(a.warmup + reps):
            for j, fn in enumerate([op] + [b[1] for b in bases]):
                x = clock(fn)
                if i >= a.warmup:
                    t[j].append(x)
        r = dict({"row": row, "operation": label, "call_ms_median": statistics.median(t[0]) * 1e3,
                  "call_ms_min": min(t[0]) * 1e3, "call_ms_max": max(t[0]) * 1e3,
                  "call_ms_p10": float(np.percentile(t[0], 10)) * 1e3, "call_ms_p90": float(np.percentile(t[0], 90)) * 1e3,
                  "reps": reps}, **extra)
        for (blabel, _fn), tb in zip(bases, t[1:]):
            q = np.percentile(np.array(tb) * 1e3, [10, 50, 90])
            r.setdefault("baselines", []).append({"baseline": blabel, "ms_p10": q[0], "ms_median": q[1], "ms_p90": q[2],
                                                  "ratio": statistics.median(t[0]) * 1e3 / q[1]})
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    def members_dev(name, cap, skip=0, d_out=None):
        nm, keep = L.name_struct(name)
        d_counts = torch.zeros(2, dtype=torch.int64, device="cuda")

        def run(_keep=keep):
            rc = lib.rbx_bitset_members_dev(client.ctx, nm, 0, 0, 0, 0, skip, cap, d_out.data_ptr() if cap else None,
                                            d_counts.data_ptr(), None)
            assert rc == 0, L.last_error()
            client.synchronize()
        return run, d_counts

    big = "bench:members:big"
    nbits = 1 << 32
    if set(a.rows) & set("ac"):
        bs = client.getBitSet(big)
        bs.setIndexes(np.concatenate([rng.integers(0, nbits, 1_000_000, dtype=np.uint64), [nbits - 1]]).astype(np.uint64))
        total = bs.cardinality()
        d_out = torch.empty(total, dtype=torch.int64, device="cuda")
        nm, _keep = L.name_struct(big)
        card = C.c_uint64()

        def cardinality():
            assert lib.rbx_bitset_cardinality(client.ctx, nm, C.byref(card)) == 0

        if "a" in a.rows:
            op, d_counts = members_dev(big, total, 0, d_out)
            count_only, _ = members_dev(big, 0)
            r = measure("a", "members_dev of a 512 MiB string with %d ones (sparse)" % total, op,
                        [("rbx_bitset_cardinality", cardinality), ("the count-only call (cap = 0): the directory", count_only)],
                        members=total)
            assert d_counts.cpu().tolist() == [total, total]
            b0, b1 = r["baselines"]
            bound = b0["ms_median"] + b1["ms_median"] + (b0["ms_p90"] - b0["ms_p10"])
            r["bound_ms"] = bound
            r["within_bound"] = "yes" if r["call_ms_median"] <= bound else "no"
            print(json.dumps({"row": "a", "bound_ms": bound, "within_bound": r["within_bound"]}), flush=True)
        if "c" in a.rows:
            def host_scan():
                got = np.flatnonzero(np.unpackbits(np.frombuffer(bs.toByteArray(), np.uint8)))
                assert got.size == total

            def pos_loop():
                nxt = 0
                for _ in range(1000):
                    nxt = bs.bitPos(1, nxt, -1, "BIT") + 1

            op, _ = members_dev(big, total, 0, d_out)
            measure("c", "members_dev of row a's string", op, [("toByteArray() + np.flatnonzero(np.unpackbits())", host_scan)],
                    reps=1, members=total)
            r = measure("c", "members_dev, first 1,000 members (cap = 1000)", members_dev(big, 1000, 0, d_out)[0],
                        [("1,000 bitPos(1, next, -1, BIT) calls", pos_loop)], reps=5)
            r["baseline_us_per_member"] = r["baselines"][0]["ms_median"]
        client.getBitSet(big).delete()
        del d_out

    if "b" in a.rows or "e" in a.rows:
        half = "bench:members:half"
        d_bytes = torch.randint(-(1 << 63), (1 << 63) - 1, (1 << 26,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert lib.rbx_bloom_import_dev(client.ctx, half.encode(), d_bytes.data_ptr(), 1 << 29, None) == 0
        bs = client.getBitSet(half)
        total = bs.cardinality()
        if "b" in a.rows:
            cap = 1 << 24
            d_out = torch.empty(cap, dtype=torch.int64, device="cuda")
            fill = client.getBitSet("bench:members:fill")
            fill.setRange(0, nbits, True)

            def fill_all():
                fill.setRange(0, nbits, False)
                client.synchronize()

            for skip, where in ((0, "skip 0"), (total - cap - 12345, "skip near the end")):
                r = measure("b", "members_dev of 512 MiB at fill 1/2, cap 2^24, " + where, members_dev(half, cap, skip, d_out)[0],
                            [("rbx_bitset_set_range of the whole 512 MiB string", fill_all)], members=cap)
                r["output_GB_per_s"] = cap * 8 / r["call_ms_median"] / 1e6
                r["fill_GB_per_s"] = (1 << 29) / r["baselines"][0]["ms_median"] / 1e6
            fill.delete()
            del d_out
        if "e" in a.rows:
            d_words = torch.empty(1 << 26, dtype=torch.int64, device="cuda")
            d_copy = torch.empty(1 << 26, dtype=torch.int64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
            nm, _keep = L.name_struct(half)

            def as_words():
                assert lib.rbx_bitset_as_words_dev(client.ctx, nm, d_words.data_ptr(), 1 << 26, d_n.data_ptr(), None) == 0
                client.synchronize()

            def copy(n):
                def run():
                    d_copy[:n].copy_(d_bytes[:n])
                    torch.cuda.synchronize()
                return run

            measure("e", "asBitSetDev of 512 MiB", as_words, [("device-to-device copy of 512 MiB", copy(1 << 26))])
            d_bytes[(1 << 25) - 1] &= (1 << 62) - 1  # the highest bit Java can count is 2^31 - 2: 256 MiB of words
            torch.cuda.synchronize()
            nm2, _keep2 = L.name_struct("bench:members:set")

            def set_words():
                assert lib.rbx_bitset_set_words_dev(client.ctx, nm2, d_bytes.data_ptr(), 1 << 25, None) == 0, L.last_error()
                client.synchronize()

            measure("e", "setBitSetDev of 256 MiB (a new key each call: allocation and zero fill included)", set_words,
                    [("device-to-device copy of 256 MiB", copy(1 << 25))])
            client.getBitSet("bench:members:set").delete()
        bs.delete()
        del d_bytes

    if set(a.rows) & set("df"):
        users = ["bench:members:u%06d" % i for i in range(USERS)]
        blob = rng.bytes(USERS * USER_BYTES)
        for i, name in enumerate(users):
            client.getBitSet(name).setBytes(blob[i * USER_BYTES: (i + 1) * USER_BYTES])
        client.synchronize()

        def stream(names, keys, cmd_rows, cap):
            n = len(keys)
            arr, keep = L.names_array(names)
            d_key = torch.from_numpy(np.asarray(keys, np.uint32).view(np.int32).copy()).cuda()
            d_cmds = torch.from_numpy(np.frombuffer(bytes(_members_cmds_array(cmd_rows)), np.uint8)[: 40 * n].copy()).cuda()
            d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            d_out = torch.empty(max(cap, 1), dtype=torch.int64, device="cuda")

            def run(_keep=(keep, d_key, d_cmds, d_out)):
                rc = lib.rbx_bitset_members_stream_dev(client.ctx, arr, len(names), d_key.data_ptr(), d_cmds.data_ptr(), n,
                                                       cap, d_off.data_ptr(), d_out.data_ptr(), None, None)
                assert rc == 0, L.last_error()
                client.synchronize()
            return run, d_off

        whole = (0, 0, 0, 0, 0, None)
        ones = int(np.unpackbits(np.frombuffer(blob, np.uint8)).sum())
        if "d" in a.rows:
            arr, keep = L.names_array(users)
            d_key = torch.arange(USERS, dtype=torch.int32, device="cuda")
            raw = np.frombuffer(bytes(_range_cmds_array([(L.RBX_RANGE_COUNT, 0, 0, 0, 0, 0)] * USERS)), np.uint8)[: 24 * USERS]
            d_rcmds, d_rep = torch.from_numpy(raw.copy()).cuda(), torch.empty(USERS, dtype=torch.int64, device="cuda")

            def counts():
                assert lib.rbx_bitset_range_stream_dev(client.ctx, arr, USERS, d_key.data_ptr(), d_rcmds.data_ptr(), USERS,
                                                       d_rep.data_ptr(), None, None) == 0
                client.synchronize()

            singles = [client.getBitSet(n) for n in users[:1000]]

            def loop():
                for s in singles:
                    s.members()

            op, d_off = stream(users, range(USERS), [whole] * USERS, ones)
            r = measure("d", "members_stream_dev, all members of 100,000 keys of 46 bytes", op,
                        [("rbx_bitset_range_stream_dev BITCOUNTs of the same keys", counts)], members=ones)
            assert int(d_off[-1]) == ones
            measure("d", "members_stream_dev, the first 1,000 of those keys",
                    stream(users[:1000], range(1000), [whole] * 1000, ones)[0], [("1,000 RBitSet.members() calls", loop)], reps=5)
        if "f" in a.rows:
            sub = users[:20000]
            sub_ones = int(np.unpackbits(np.frombuffer(blob[: 20000 * USER_BYTES], np.uint8)).sum())
            for lanes in (4, 8, 16, 32, 64):
                tune(members_lanes=lanes)
                measure("f", "members_stream_dev, all members of 20,000 keys of 46 bytes",
                        stream(sub, range(20000), [whole] * 20000, sub_ones)[0], lanes=lanes)
            tune(**DEFAULTS)
            huge = ["bench:members:huge%d" % i for i in range(4)]
            for name in huge:  # 8 MiB at one bit in 64
                b8 = np.frombuffer(rng.bytes(8 << 20), np.uint8)
                for _ in range(5):
                    b8 = b8 & np.frombuffer(rng.bytes(8 << 20), np.uint8)
                client.getBitSet(name).setBytes(b8.tobytes())
            n = 10000
            names = users[: n - 100] + huge
            keys = list(range(n - 100)) + [n - 100 + i % 4 for i in range(100)]
            order = rng.permutation(n)
            keys = [keys[i] for i in order]
            cap = 1 << 27
            for short_max in (64, 4096, 65536, 1 << 20):
                for tile in (4096, 65536, 1 << 20):
                    tune(members_short_max=short_max, members_tile=tile)
                    measure("f", "members_stream_dev, all members, 99 % 46-byte keys and 1 % 8 MiB keys (1 bit in 64)",
                            stream(names, keys, [whole] * n, cap)[0], reps=10, short_max=short_max, tile=tile)
            tune(**DEFAULTS)
            for name in huge:
                client.getBitSet(name).delete()

    doc = {"bench": "members", "device": torch.cuda.get_device_name(0),
           "timing": "host clock, call (or loop of calls) + stream synchronise", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    client.shutdown()


if __name__ == "__main__":
    main()
