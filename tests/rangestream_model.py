"""A model of rbx_bitset_range_stream: one command at a time over bitstring_model.Keyspace (bitcount, bitpos,
size, length -- which call bitrange_model and bitset_model and restate nothing), plus what the call adds of its
own: the caller's errors, the four ways a command fails alone and their order, and the call's return code.  A
command is a row (op, bit, nargs, start, end, unit) as redisson_amd.client.bitset_range_stream_call takes it."""
import bitstring_model as BM

COUNT, POS, STRLEN, LENGTH = 0, 1, 2, 3
BYTE, BIT = 0, 1
UNIT_NAMES = {BYTE: "BYTE", BIT: "BIT"}
OK, E_ILLEGAL_ARGUMENT, E_WRONGTYPE, E_REDIS = 0, -1, -5, -9
FAILED = 0xFF
BAD_BIT, SYNTAX, WRONGTYPE, SCRIPT = "bit", "syntax", "wrongtype", "script"  # the failure kinds, in checking order
MESSAGES = {BAD_BIT: "ERR The bit argument must be 1 or 0.", SYNTAX: "ERR syntax error",
            WRONGTYPE: "WRONGTYPE Operation against a key holding the wrong kind of value",
            SCRIPT: "ERR bit offset is not an integer or out of range"}
CODES = {BAD_BIT: E_REDIS, SYNTAX: E_REDIS, WRONGTYPE: E_WRONGTYPE, SCRIPT: E_REDIS}


def caller_error(nkeys, cmd_key, rows):
    """what refuses the whole call"""
    for k, (op, _bit, nargs, _start, _end, unit) in zip(cmd_key, rows):
        if k >= nkeys or op > LENGTH or unit > BIT or nargs > 2 or (op == COUNT and nargs == 1):
            return True
    return False


def run_one(ks, name, row):
    """-> (reply, None) or (0, failure kind).  The command's own arguments are looked at before the key's type, as
    the single calls do; length()'s script fails on the data."""
    op, bit, nargs, start, end, unit = row
    if op == POS:
        if bit not in (0, 1):
            return 0, BAD_BIT
        if nargs < 2 and unit == BIT:
            return 0, SYNTAX
    if op == COUNT:
        reply, err = ks.bitcount("range stream", name, start if nargs else None, end, UNIT_NAMES[unit])
    elif op == POS:
        reply, err = ks.bitpos("range stream", name, bit, nargs, start, end, UNIT_NAMES[unit])
    elif op == STRLEN:
        reply, err = ks.size("range stream", name)
        reply = None if err else reply // 8
    else:
        reply, err = ks.length("range stream", name)
    if err is None:
        return int(reply), None
    assert err in (BM.WRONGTYPE, BM.BIT_OFFSET), err
    return 0, WRONGTYPE if err == BM.WRONGTYPE else SCRIPT


def apply_stream(ks, names, cmd_key, rows):
    """-> (rc, replies, status, kinds): every command runs; rc is the first failing command's code.  The
    keyspace is only read."""
    if caller_error(len(names), cmd_key, rows):
        return E_ILLEGAL_ARGUMENT, None, None, None
    replies, status, kinds = [], [], []
    for k, row in zip(cmd_key, rows):
        reply, kind = run_one(ks, names[k], row)
        replies.append(reply)
        status.append(FAILED if kind else 0)
        kinds.append(kind)
    first = next((k for k in kinds if k), None)
    return (CODES[first] if first else OK), replies, status, kinds


def message(kinds):
    first = next((k for k in kinds if k), None)
    return MESSAGES[first] if first else ""
