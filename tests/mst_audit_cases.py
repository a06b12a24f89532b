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
# The list's scatter sums the totals of the groups before a leaf's own by a wave: LANES = 64 totals a trip of its loop, then six
# shuffle steps.  A group is GROUP_ROWS = 16384 leaves, so a leaf's place takes a second trip only from group 65 on (leaf
# 65 * GROUP_ROWS); a leaf of group 64 still sums exactly 64 groups in one trip.  BIG is the smallest size with items
# 65 * GROUP_ROWS - 1 (the last place of one full trip) and the first two places that need a second.
LANES = 64
GROUP_ROWS = TILE * GROUP
TRIP_ROWS = LANES * GROUP_ROWS
BIG = 65 * GROUP_ROWS + 2
# depth -> n_currencies of the sparse synthetic trees: 4 groups; 64 groups (every lane one group, all six shuffle steps carry
# data); 128 groups (two trips, 134 MB of balances)
SPARSE_DEPTHS = {16: 3, 20: 2, 21: 1}
SPARSE_N_BYTES = 8
# the flags kernel's gather of a node's nc bits out of the workgroup's bit string: fields that straddle a 64-bit word of it
# (5, 33, 63) and the aligned one (64); 1, 255 and 511 nodes
MANY_CURRENCIES = [5, 33, 63, 64]
MANY_DEPTHS = [0, 7, 8]
MANY_N_BYTES = [5, 31]


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


# ----------------------------------------------------------------------------- many currencies: the flags kernel's bit gather
def straddling_leaf(size, nc, c):
    """a leaf of the first workgroup whose bit of currency c lies in the word after the one its field starts in (thread t is node
    t, its field starts at bit t * nc of the string); where there is none (c = 0, nc = 64, one leaf), a leaf a third in"""
    for i in range(min(size, THREADS)):
        if (i * nc) % 64 + c >= 64:
            return i
    return size // 3


def many_currency_plants(depth, nc, n_bytes):
    """beside plants(): only currency c out of range at one leaf (so at its ancestors: flags c + 1, up to nc), and every currency
    out of range at every leaf (a set bit at both ends of every node's field)"""
    size, top = 1 << depth, top_of(n_bytes)
    out = []
    for c in sorted({c for c in (0, 31, 32, nc - 2, nc - 1) if 0 <= c < nc}):
        out.append((f"only currency {c}", [(straddling_leaf(size, nc, c), c, top)], [None, 1]))
    out.append(("every currency at every leaf", [(i, c, top + i + c) for i in range(size) for c in range(nc)], [None, 1]))
    return out


# ----------------------------------------------------------------------------- sparse trees: the depths Python lists do not afford
def sparse_nodes(depth, nc, plant):
    """a tree of zeros but for the plant [(leaf, currency, value)] -> [level]{node: [nc balances]}, the non-zero nodes only, the
    sums mod r level by level"""
    level = {}
    for leaf, c, v in plant:                                   # (a later plant of the same slot wins, as in planted)
        level.setdefault(leaf, [0] * nc)[c] = v % R
    levels = [{i: b for i, b in level.items() if any(b)}]
    for _ in range(depth):
        above = {}
        for i, b in levels[-1].items():
            s = above.setdefault(i >> 1, [0] * nc)
            for c in range(nc):
                s[c] = (s[c] + b[c]) % R
        levels.append({i: b for i, b in above.items() if any(b)})
    return levels


def nonzero_nodes(levels):
    """[level][node][currency] -> the shape of sparse_nodes"""
    return [{i: list(b) for i, b in enumerate(level) if any(b)} for level in levels]


def level_first(level, depth):
    return (2 << depth) - (2 << (depth - level))


def sparse_bytes(depth, nc, nodes):
    """what the tree keeps in HBM for sparse nodes: zeros (0 in Montgomery form is 0) and the non-zero nodes' rows"""
    out = np.zeros((((2 << depth) - 1) * nc, 32), dtype=np.uint8)
    for level, some in enumerate(nodes):
        for i, b in some.items():
            at = (level_first(level, depth) + i) * nc
            out[at:at + nc] = mont_bytes(b).reshape(nc, 32)
    return out.reshape(-1)


def sparse_model(depth, n_bytes, nodes, bad_cap=None):
    """model() over sparse nodes, in numpy: {"flags": uint8, "masks": uint32, "bad": uint32, "summary": [4 integers]}"""
    top, leaves = top_of(n_bytes), 1 << depth
    flags = np.zeros((2 << depth) - 1, dtype=np.uint8)
    for level, some in enumerate(nodes):
        for i, b in some.items():
            out = [c for c, v in enumerate(b) if v >= top]
            if out:
                flags[level_first(level, depth) + i] = 1 + out[0]
    index = np.arange(leaves, dtype=np.int64)
    masks = (flags[:leaves] != 0).astype(np.uint32)
    for l in range(depth):
        bad_l = flags[level_first(l, depth):level_first(l, depth) + (leaves >> l)] != 0
        if bad_l.any():
            masks |= bad_l[(index >> l) ^ 1].astype(np.uint32) << np.uint32(l + 1)
    unprovable = np.flatnonzero(masks).astype(np.uint32)
    bad = unprovable if bad_cap is None else unprovable[:bad_cap]
    return {"flags": flags, "masks": masks, "bad": bad,
            "summary": [int(np.count_nonzero(flags)), int(unprovable.size), int(bad.size), int(flags[-1])]}


def cut(full, bad_cap):
    """a sparse_model with room for every leaf -> the same audit asked with bad_cap"""
    bad = full["bad"] if bad_cap is None else full["bad"][:bad_cap]
    return dict(full, bad=bad, summary=full["summary"][:2] + [int(bad.size), full["summary"][3]])


def sparse_spots(depth):
    """the leaves that get `top` (their siblings get r - top): 1 + g % 5 pairs in every group g of the list's compaction, so that
    the groups' totals differ, and the first and last leaf of groups 0, 63, 64, 65 and the last, where the tree has them"""
    size = 1 << depth
    span = min(GROUP_ROWS, size)
    groups = size // span
    by_pair = {}
    for g in range(groups):
        spots = [g * span + 2 * (613 * j + 29 * g + 1) % span for j in range(1 + g % 5)]
        if g in (0, 63, 64, 65, groups - 1):
            spots += [g * span, (g + 1) * span - 1]
        for i in spots:
            by_pair.setdefault(i >> 1, i)
    return sorted(by_pair.values()) if depth else []


def sparse_plants(depth, n_bytes):
    """[(name, plant, caps)] for sparse_nodes: the cancelling pairs at sparse_spots -- exactly those pairs are unprovable --, and
    `top` at leaf 0 alone: every ancestor of leaf 0 is out of range, so every leaf is listed and the place of leaf i is i (every
    group's total is GROUP_ROWS: a dropped or doubled group shifts every later place).  The caps: room for all, 0, 1, the count
    and one less, and past group 64 one that cuts the list one entry into group 65"""
    size, top = 1 << depth, top_of(n_bytes)
    spots = sparse_spots(depth)
    out = []
    for name, plant, in_group in (("pairs in every group", [(i, 0, top) for i in spots] + [(i ^ 1, 0, R - top) for i in spots],
                                   lambda g: 2 * sum(1 for i in spots if i // GROUP_ROWS == g)),
                                  ("top at leaf 0 alone", [(0, 0, top)], lambda g: min(GROUP_ROWS, size))):
        count = sum(in_group(g) for g in range(-(-size // GROUP_ROWS)))
        caps = [None, 0, 1, count, max(count - 1, 0)]
        if size > 65 * GROUP_ROWS:
            caps.append(sum(in_group(g) for g in range(65)) + 1)
        out.append((name, plant, caps))
    return out
