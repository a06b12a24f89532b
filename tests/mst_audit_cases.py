"""The integer model of the range audit (csrc/mst_audit.h, include/summa_snapshot.h: ss_mst_range_audit_dev) and the cases that
tests/test_mst_audit_cpu.py gives to the header's serial steps and tests/test_gpu_mst_audit.py to the kernels.  Stated from the
circuit, not from the header: a node is flagged with 1 + its lowest currency holding a balance >= top = 2^(8 n_bytes); leaf i's
mask has bit 0 for its own flag and bit l + 1 for the flag of its path's sibling at level l; the list is the leaves with a
non-zero mask in increasing order, cut at bad_cap.  Python integers and numpy only."""
import csv

import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001          # BN254 Fr
MONT = (1 << 256) % R
TILE, GROUP, THREADS = 64, 256, 256            # what csrc/mst_audit.h must say (the CPU test asserts it from the check program)
# a depth <= 16 whose per-tile counts span more than one workgroup of the prefix ("groups") step: 2^15 leaves are 512 tiles of
# 64 leaves, two groups of 256 tile counts, so the second group's leaves take their places from the first group's total
GROUPS_DEPTH = 15
DEPTHS = [0, 1, 6, 7, 8, 11]                  # 127 / 255 / 511 nodes: one short of and one past the 128- and 256-thread block edges
CURRENCIES = [1, 2, 3, 4]
N_BYTES = [1, 5, 8, 31]


def top_of(n_bytes):
    return 1 << (8 * n_bytes)


def levels_of(leaf_bal):
    """leaf balances [leaf][currency] -> node balances [level][node][currency], the sums mod r"""
    levels = [[list(b) for b in leaf_bal]]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([[(x + y) % R for x, y in zip(below[2 * p], below[2 * p + 1])] for p in range(len(below) // 2)])
    return levels


def level_major(levels):
    """[level][node][currency] -> the flat list of all balances, level-major"""
    return [v for level in levels for node in level for v in node]


def flags_of(levels, n_bytes):
    top = top_of(n_bytes)
    out = []
    for level in levels:
        for node in level:
            bad = [c for c, v in enumerate(node) if v >= top]
            out.append(1 + bad[0] if bad else 0)
    return out


def masks_of(levels, n_bytes):
    top = top_of(n_bytes)
    bad = [[any(v >= top for v in node) for node in level] for level in levels]
    depth = len(levels) - 1
    return [int(bad[0][i]) | sum(2 << l for l in range(depth) if bad[l][(i >> l) ^ 1]) for i in range(len(levels[0]))]


def model(levels, n_bytes, bad_cap):
    """{"flags", "masks", "bad", "summary"} of a tree given as [level][node][currency] integers"""
    flags, masks = flags_of(levels, n_bytes), masks_of(levels, n_bytes)
    unprovable = [i for i, m in enumerate(masks) if m]
    bad = unprovable[:bad_cap]
    return {"flags": flags, "masks": masks, "bad": bad,
            "summary": [sum(1 for f in flags if f), len(unprovable), len(bad), flags[-1]]}


def mont_bytes(values):
    """integers -> their Montgomery words back to back (uint8), what the tree keeps in HBM"""
    return np.frombuffer(b"".join((v * MONT % R).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def csv_levels(path):
    """a snapshot CSV -> [level][node][currency], balances summed as integers mod r, zero entries up to a power of two"""
    rows = list(csv.reader(open(path)))[1:]
    bal = [[int(v) for v in r[1:]] for r in rows]
    size = 1 << max(0, (len(bal) - 1).bit_length())
    return levels_of(bal + [[0] * len(bal[0])] * (size - len(bal)))


# ----------------------------------------------------------------------------- the predicate
def predicate_values(n_bytes):
    top = top_of(n_bytes)
    return [top - 1, top, top + 1, 0, R - 1, 1 << 224, (1 << 252) + 5]          # the last two: only word 7 set; word 7 and word 0


# ----------------------------------------------------------------------------- synthetic trees
def base_leaves(depth, nc, n_bytes):
    """in range at every level: zeros for n_bytes = 1 (top = 256), else values below 251 (sums below 2^16 * 251 < 2^40)"""
    if n_bytes < 5:
        return [[0] * nc for _ in range(1 << depth)]
    return [[(31 * i + 7 * c) % 251 for c in range(nc)] for i in range(1 << depth)]


def edge_leaves(depth):
    """the leaves on both sides of every edge of the geometry: the 64-leaf tiles (a wave), hence the 256-thread blocks and, at
    GROUPS_DEPTH, the 16384-leaf groups; thinned to the block and group edges above 2^11 leaves"""
    size = 1 << depth
    step = TILE if depth <= 11 else THREADS
    edges = set(range(step, size, step)) | set(range(TILE * GROUP, size, TILE * GROUP)) | {e for e in (TILE, 3 * TILE) if e < size}
    return sorted({e - 1 for e in edges} | edges)


def plants(depth, nc, n_bytes):
    """[(name, [(leaf, currency, value)], [bad_cap ..])]: each a case of its own; bad_cap None = room for every leaf"""
    size, top = 1 << depth, top_of(n_bytes)
    out = [("none", [], [None]),
           ("first leaf", [(0, 0, top)], [None, 0]),
           ("last leaf", [(size - 1, 0, top + 1)], [None]),
           ("last currency only", [(size // 3, nc - 1, top)], [None]),
           ("every leaf", [(i, i % nc, top + i) for i in range(size)], [None, size, max(size // 2 - 1, 0), 1, 0])]
    if depth >= 1:
        pair = 2 if size >= 4 else 0
        out.append(("two in-range siblings whose sum leaves the range", [(pair, 0, top - 1), (pair + 1, 0, 1)], [None]))
        out.append(("r - 1 beside 1", [(size - 2, nc - 1, R - 1), (size - 1, nc - 1, 1)], [None]))
    if edge_leaves(depth):
        # top at an edge leaf, r - top at its sibling: both are out of range and their parent's sum is 0, so exactly these pairs
        # are unprovable and the list is sparse on both sides of every edge
        e = edge_leaves(depth)
        out.append(("edges", [(i, 0, top) for i in e] + [(i ^ 1, 0, R - top) for i in e], [None, 2 * len(e), 2 * len(e) - 1, 1]))
    return out


def planted(depth, nc, n_bytes, plant):
    leaves = base_leaves(depth, nc, n_bytes)
    for leaf, c, v in plant:                                   # (a later plant of the same slot wins)
        leaves[leaf] = list(leaves[leaf])
        leaves[leaf][c] = v
    return levels_of(leaves)
