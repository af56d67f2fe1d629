"""A model of rbx_bitset_op_groups: the groups applied to bitstring_model.Keyspace one command at a time, in array
order -- BITOP for a group with a destination followed by BITCOUNT of it, and for a group without one the same into
a temporary key that is deleted again -- plus the host's phase and forwarding rule (redisson_amd/csrc/
bit_groups_plan.h) restated, so that a test can assert how many launches' worth of phases a call makes.

A key of another type is a name in Keyspace.hll: tests put a Bloom filter's {name}:config there too, both are
"another type" to a bit command."""
import bitstring_model as BM

AND, OR, XOR, NOT = 0, 1, 2, 3
OPS = {AND: "and", OR: "or", XOR: "xor", NOT: "not"}
OK, E_ILLEGAL_ARGUMENT, E_WRONGTYPE, E_REDIS = 0, -1, -5, -9
FAILED = 0xFF
WRONGTYPE_MSG = "WRONGTYPE Operation against a key holding the wrong kind of value"
NOT_MSG = "ERR BITOP NOT must be called with a single source key."
_TMP = "\0bitgroups-model-temporary"


def caller_error(names, ops, dests, groups):
    """what the call refuses as a whole, with nothing changed"""
    n = len(names)
    for op, d, g in zip(ops, dests, groups):
        if op > NOT or not g or any(k >= n for k in g) or (d is not None and d >= n):
            return True
    return False


def group_failure(ks, names, op, dest, group):
    """the code a group fails alone with, or OK: NOT's source count first, as in the single call"""
    if op == NOT and len(group) != 1:
        return E_REDIS
    keys = [names[k] for k in group] + ([] if dest is None else [names[dest]])
    return E_WRONGTYPE if any(k in ks.hll for k in keys) else OK


def apply_groups(ks, names, ops, dests, groups):
    """-> (rc, lens, counts, status).  names: the call's keys; group g is BITOP ops[g] names[dests[g]] <names[k] for k
    in groups[g]>, dests[g] = None: stored nowhere.  ks changes as the engine's keyspace does."""
    n = len(groups)
    if caller_error(names, ops, dests, groups):
        return E_ILLEGAL_ARGUMENT, [0] * n, [0] * n, [0] * n
    rc, lens, counts, status = OK, [], [], []
    for op, d, g in zip(ops, dests, groups):
        code = group_failure(ks, names, op, d, g)
        if code != OK:
            rc = rc or code
            lens.append(0), counts.append(0), status.append(FAILED)
            continue
        dest = _TMP if d is None else names[d]
        srcs = [names[k] for k in g]
        if op == NOT:
            length, err = ks.bitop_not("conn", dest, srcs[0])
        else:
            length, err = ks.bitop("conn", dest, OPS[op], srcs)
        assert err is None, err
        count, err = ks.cardinality("conn", dest)
        assert err is None, err
        if d is None:
            ks.delete("conn", _TMP)
        lens.append(length), counts.append(count), status.append(0)
    return rc, lens, counts, status


def message(rc):
    return {OK: "", E_WRONGTYPE: WRONGTYPE_MSG, E_REDIS: NOT_MSG}.get(rc)


def plan(names, ops, dests, groups, failed):
    """bit_groups_plan restated: -> (phases, fwd) with fwd[g] = the group whose replies answer group g, or None.
    failed[g]: the group fails alone (it writes, closes and forwards nothing)."""
    ids: dict = {}
    canon = [ids.setdefault(bytes(nm, "utf-8") if isinstance(nm, str) else bytes(nm), i) for i, nm in enumerate(names)]
    written, read, writer = {}, {}, {}
    phase, phases, fwd = 1, 0, [None] * len(groups)
    for g, (op, d, grp) in enumerate(zip(ops, dests, groups)):
        if failed[g]:
            continue
        srcs = [canon[k] for k in grp]
        dk = None if d is None else canon[d]
        if dk is None and len(srcs) == 1 and op != NOT and written.get(srcs[0]) == phase:
            fwd[g] = writer[srcs[0]]
            continue
        hazard = dk is not None and (written.get(dk) == phase or read.get(dk) == phase)
        hazard = hazard or any(s != dk and written.get(s) == phase for s in srcs)
        if hazard:
            phase += 1
        phases = phase
        if dk is not None:
            written[dk], writer[dk] = phase, g
        for s in srcs:
            if s != dk:
                read[s] = phase
    return phases, fwd


def expected_phases(ks, names, ops, dests, groups):
    """the phases rbx_bench_bitgroups_last reports for this call on the keyspace as it stands BEFORE the call (a
    key's type does not change during one)"""
    if caller_error(names, ops, dests, groups):
        return None
    failed = [group_failure(ks, names, op, d, g) != OK for op, d, g in zip(ops, dests, groups)]
    return plan(names, ops, dests, groups, failed)[0]


Keyspace = BM.Keyspace
