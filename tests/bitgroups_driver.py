"""The seeded random plan for rbx_bitset_op_groups: 300 calls of 1 to 40 groups over 12 bit-string keys plus two keys
of another type (an HLL and a Bloom filter's {name}:config).  It is data only: test_bitgroups_cpu.py checks the
plan's share of failing groups on the model alone, test_bitgroups_gpu.py runs it on the engine.

A call is (resets, ops, dests, groups).  resets = [(key, length, seed, timeout)] are applied first: SET key <length
random bytes> (length 0: DEL), then a timeout when asked -- without them every string would soon be as long as the
longest, a BITOP's result never being shorter than a source.  Lengths come from LENGTHS, the edges of the 16-byte
vectors and of the smallest tile (T = 4096).  Per group: the op is random; NOT takes one source; the destination is
absent with probability 1/4 and among the group's own sources with probability 1/4; with probability P_WRONG one
operand is replaced by a key of another type, which makes the group fail alone."""
import numpy as np

SEED = 20261021
T = 4096
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, T - 1, T, T + 1, 3 * T + 5)
NKEYS = 12  # bit strings; the names' entries NKEYS and NKEYS + 1 are the two keys of another type
NSRC = (1, 2, 2, 2, 3, 8, 9, 17)
P_WRONG = 0.05  # 1 group in 20 fails: half the 10 % cap, so the committed seed stays under it with room


def names(prefix):
    """the call's names: 12 bit strings, an HLL, a {name}:config"""
    return [prefix + "k%d" % i for i in range(NKEYS)] + [prefix + "hll", "{" + prefix + "bloom}:config"]


def seeded_calls(seed=SEED, ncalls=300):
    rng = np.random.default_rng(seed)
    calls = []
    for c in range(ncalls):
        resets = []
        for _ in range(int(rng.integers(0, 4)) if c else NKEYS):
            key = int(rng.integers(0, NKEYS)) if c else len(resets)
            resets.append((key, int(rng.choice(LENGTHS)), int(rng.integers(0, 1 << 31)), bool(rng.random() < 0.3)))
        ops, dests, groups = [], [], []
        for _ in range(int(rng.integers(1, 41))):
            op = int(rng.integers(0, 4))
            srcs = [int(k) for k in rng.integers(0, NKEYS, size=1 if op == 3 else int(rng.choice(NSRC)))]
            u = rng.random()
            dest = None if u < 0.25 else int(rng.choice(srcs)) if u < 0.5 else int(rng.integers(0, NKEYS))
            if rng.random() < P_WRONG:
                wrong = NKEYS + int(rng.integers(0, 2))
                if dest is not None and rng.random() < 0.5:
                    dest = wrong
                else:
                    srcs[int(rng.integers(0, len(srcs)))] = wrong
            ops.append(op), dests.append(dest), groups.append(srcs)
        calls.append((resets, ops, dests, groups))
    return calls


def failing_groups(calls):
    """the groups of the plan that fail alone: those naming a key of another type (no NOT has several sources)"""
    return sum((d is not None and d >= NKEYS) or any(k >= NKEYS for k in g)
               for _r, ops, dests, groups in calls for d, g in zip(dests, groups))
