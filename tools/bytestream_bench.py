#!/usr/bin/env python3
"""GETRANGE / SETRANGE / APPEND over many keys in one call (rbx_string_stream_dev) against the only route the engine
had to the same bytes before, in one process on one MI355X.

  a  USERS keys of 46 bytes, one 4-byte APPEND each, in one rbx_string_stream_dev call
                                     vs per key rbx_bitset_export_n, patch on the host, rbx_bitset_import_n
                                        (timed over the first PAIR keys and scaled; the requirement: the stream's
                                        time per command is below the baseline's, `faster`: yes / no)
  b  the same keys, "read the last 8 bytes of every user's string": one GETRANGE k -8 -1 each     (recorded)
  c  one SETRANGE of 4 KiB into a 64 MiB string through rbx_string_setrange_dev
                                     vs export, patch, import of the whole string
  d  bytestream_lanes 4 .. 64 on row a's call                                                        (recorded)

Each figure is a call time: a host clock around the _dev call and the stream synchronise that ends it; the call's own
waits are part of it.  Operation and baseline alternate inside one loop; the median of the repetitions after the
warm-ups is reported.  `ratio` = the operation's time over its baseline's.  Writes one JSON document (default
profiles/bitset/bytestream_bench.json).  The knobs' defaults are NOT measured until this has run.
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

USERS, USER_BYTES, PAIR = 100_000, 46, 1024
BIG = 64 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="abcd")
    ap.add_argument("--users", type=int, default=USERS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitset", "bytestream_bench.json"))
    a = ap.parse_args()

    client = RedissonClient(0)
    lib = L.lib()
    rng = np.random.default_rng(0xB17E5)
    rows = []
    users = a.users

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def put(name, data):
        nm, _k = L.name_struct(name)
        buf = np.frombuffer(data, np.uint8)
        assert lib.rbx_bitset_import_n(client.ctx, nm, buf.ctypes.data_as(L.u8p), len(data)) == 0

    def median_pair(op, base):
        t_op, t_base = [], []
        for i in range(a.warmup + a.reps):
            x, y = clock(op), (clock(base) if base else 0.0)
            if i >= a.warmup:
                t_op.append(x)
                t_base.append(y)
        return statistics.median(t_op), statistics.median(t_base)

    names = [f"user:{i}" for i in range(users)]
    names_arr, _keep = L.names_array(names)

    def reset_users():
        blob = rng.bytes(users * USER_BYTES)
        for i, nme in enumerate(names):
            put(nme, blob[i * USER_BYTES:(i + 1) * USER_BYTES])

    def dev_cmds(op, a_, b_, val_len):
        arr = (L.RbxStringCmd * users)()
        for i, c in enumerate(arr):
            c.op, c.a, c.b, c.val_off, c.val_len = op, a_, b_, 4 * i if val_len else 0, val_len
        return torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).cuda()

    d_key = torch.arange(users, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(users + 1, dtype=torch.int64, device="cuda")
    d_rep = torch.zeros(users, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(users, dtype=torch.uint8, device="cuda")
    total = C.c_uint64()

    def stream(d_cmds, d_vals, vals_len, d_out, cap):
        rc = lib.rbx_string_stream_dev(client.ctx, names_arr, users, d_key.data_ptr(), d_cmds.data_ptr(), users,
                                       d_vals.data_ptr() if d_vals is not None else None, vals_len, cap, d_off.data_ptr(),
                                       d_out.data_ptr() if d_out is not None else None, d_rep.data_ptr(), d_st.data_ptr(),
                                       C.byref(total), None)
        assert rc == 0, L.last_error()
        client.synchronize()

    if "a" in a.rows or "d" in a.rows or "b" in a.rows:
        reset_users()
    d_vals = torch.from_numpy(np.frombuffer(rng.bytes(4 * users), np.uint8).copy()).cuda()
    appends = dev_cmds(L.RBX_STR_APPEND, 0, 0, 4)

    def baseline_pair():
        buf = np.zeros(1 << 16, np.uint8)
        n = C.c_uint64()
        for i in range(min(PAIR, users)):
            nm, _k = L.name_struct(names[i])
            assert lib.rbx_bitset_export_n(client.ctx, nm, buf.ctypes.data_as(L.u8p), buf.size, C.byref(n)) == 0
            buf[n.value:n.value + 4] = 7
            assert lib.rbx_bitset_import_n(client.ctx, nm, buf.ctypes.data_as(L.u8p), n.value + 4) == 0

    if "a" in a.rows:
        t_op, t_base = median_pair(lambda: stream(appends, d_vals, 4 * users, None, 0), baseline_pair)
        per_op, per_base = t_op / users, t_base / min(PAIR, users)
        rows.append(dict(row="a", what=f"{users} keys, one 4-byte APPEND each, one call", ms=t_op * 1e3,
                         us_per_command=per_op * 1e6, baseline=f"export / patch / import per key over {min(PAIR, users)} keys",
                         baseline_us_per_command=per_base * 1e6, ratio=per_op / per_base,
                         faster="yes" if per_op < per_base else "no"))
    if "b" in a.rows:
        reads = dev_cmds(L.RBX_STR_GETRANGE, -8, -1, 0)
        d_out = torch.zeros(8 * users, dtype=torch.uint8, device="cuda")
        t_op, _ = median_pair(lambda: stream(reads, None, 0, d_out, 8 * users), None)
        rows.append(dict(row="b", what=f"{users} keys, GETRANGE k -8 -1 each, one call", ms=t_op * 1e3,
                         us_per_command=t_op / users * 1e6))
    if "c" in a.rows:
        put("big", rng.bytes(BIG))
        nm, _k = L.name_struct("big")
        d_patch = torch.from_numpy(np.frombuffer(rng.bytes(4096), np.uint8).copy()).cuda()
        host = np.zeros(BIG, np.uint8)
        n = C.c_uint64()

        def patch_dev():
            assert lib.rbx_string_setrange_dev(client.ctx, nm, 12_345_678, d_patch.data_ptr(), 4096, C.byref(n), None) == 0
            client.synchronize()

        def patch_host():
            assert lib.rbx_bitset_export_n(client.ctx, nm, host.ctypes.data_as(L.u8p), BIG, C.byref(n)) == 0
            host[12_345_678:12_345_678 + 4096] = 7
            assert lib.rbx_bitset_import_n(client.ctx, nm, host.ctypes.data_as(L.u8p), BIG) == 0

        t_op, t_base = median_pair(patch_dev, patch_host)
        rows.append(dict(row="c", what="SETRANGE of 4 KiB into a 64 MiB string (rbx_string_setrange_dev)", ms=t_op * 1e3,
                         baseline="export, patch, import of the whole string", baseline_ms=t_base * 1e3, ratio=t_op / t_base))
    if "d" in a.rows:
        for lanes in (4, 8, 16, 32, 64):
            assert lib.rbx_tune(b"bytestream_lanes", lanes) == 0
            t_op, _ = median_pair(lambda: stream(appends, d_vals, 4 * users, None, 0), None)
            rows.append(dict(row="d", what=f"row a's call with bytestream_lanes = {lanes}", ms=t_op * 1e3))
        assert lib.rbx_tune(b"bytestream_lanes", 16) == 0

    doc = dict(tool="tools/bytestream_bench.py", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    for r in rows:
        print(json.dumps(r))
    client.shutdown()


if __name__ == "__main__":
    main()
