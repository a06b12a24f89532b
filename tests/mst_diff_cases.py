"""The pairs of snapshot CSVs the diff of a new round against a tree is checked with, on the host (test_mst_diff_cpu.py: the serial
steps of csrc/mst_diff.h behind the reader's and the sort's) and on the device (test_gpu_mst_diff.py), and the model both are
compared with, in pure Python over lists of names and integer balances.

A case is (name, rows of A, rows of B, n_currencies, sorted_tree): rows are [(name bytes, [balance texts])], A the file the tree T
was built from (its leaves in file order, or sorted stably by the names' bytes), B the next round's file.  The base file A uses
the names f"{k:06d}" in a seeded shuffle with distinct balances per row; B is derived from A.  Where a family speaks of leaves
(changed or gone at an edge), the leaf is one of the tree of the case's kind.

The lists are compacted by a ballot per wave of TILE = 64 items, a scan per workgroup over GROUP = 256 tile counts and the groups'
totals (MST_DIFF_TILE, MST_DIFF_GROUP and MST_DIFF_THREADS of csrc/mst_diff.h, restated; the check program prints them): the
edges are 64, 256 and 16384, and 16386 is the smallest size with leaf positions 16383, 16384 and 16385."""
import random

import numpy as np

from mst_csv_cases import header, write_case  # noqa: F401  (write_case: for the tests that import this module)
from mst_names_cases import caps_for  # noqa: F401

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
THREADS, TILE, GROUP = 256, 64, 256
GROUP_ROWS = TILE * GROUP
SIZES = (1, 2, 64, 65, 257, GROUP_ROWS + 2)
EDGES = (TILE, THREADS, GROUP_ROWS)
ABSENT = 0xFFFFFFFF
LEAF_PADDING, LEAF_SAME, LEAF_CHANGED, LEAF_GONE, LEAF_UNREACHABLE = 0, 1, 2, 3, 4
ROW_SAME, ROW_CHANGED, ROW_NEW, ROW_SHADOWED = 1, 2, 3, 4
SUMMARY = ("new", "shadowed", "changed", "same", "gone", "unreachable", "new_listed", "gone_listed")


def base(n: int, nc: int = 2, tag: str = ""):
    """A: n distinct names in a seeded shuffle, distinct balances per row"""
    names = [f"{k:06d}".encode() for k in range(n)]
    random.Random(f"mst_diff_cases.base.{n}.{nc}.{tag}").shuffle(names)
    return [(nm, [str(1000 + i * nc + c) for c in range(nc)]) for i, nm in enumerate(names)]


def leaf_order(rows, sorted_tree: bool):
    """the file row of A at every leaf of T"""
    order = list(range(len(rows)))
    if sorted_tree:
        order.sort(key=lambda r: rows[r][0])                  # stable: equal names keep file order
    return order


def edge_leaves(n: int):
    """leaf 0, the last leaf, and edge - 1, edge, edge + 1 of every edge, where the tree has them"""
    return sorted({0, n - 1} | {e + d for e in EDGES for d in (-1, 0, 1) if 0 <= e + d < n})


def bump(row, c: int):
    name, bal = row
    return (name, [str(int(b) + 1) if k == c else b for k, b in enumerate(bal)])


def shuffled(rows, tag: str):
    rows = list(rows)
    random.Random(f"mst_diff_cases.shuffle.{tag}.{len(rows)}").shuffle(rows)
    return rows


def cases():
    out = []

    def add(name, a, b, nc=2, kinds=(False, True)):
        for sorted_tree in kinds:
            out.append((f"{name}_{'sorted' if sorted_tree else 'file'}", a, b, nc, sorted_tree))

    for n in SIZES:
        a = base(n)
        add(f"equal_{n}", a, list(a))
        every = [bump(row, i % 2) for i, row in enumerate(a)]
        add(f"every_row_changed_{n}", a, every)
        add(f"every_row_changed_shuffled_{n}", a, shuffled(every, "every"))
        add(f"equal_shuffled_{n}", a, shuffled(a, "equal"))
        for sorted_tree in (False, True):
            order = leaf_order(a, sorted_tree)
            at = {order[leaf] for leaf in edge_leaves(n)}     # the file rows of A that stand in the edge leaves
            changed = [bump(row, (i + 1) % 2) if i in at else row for i, row in enumerate(a)]
            add(f"edges_changed_{n}", a, changed, kinds=(sorted_tree,))
            add(f"edges_changed_shuffled_{n}", a, shuffled(changed, "edges"), kinds=(sorted_tree,))
            gone = [row for i, row in enumerate(a) if i not in at]
            if gone:
                add(f"edges_gone_{n}", a, gone, kinds=(sorted_tree,))
                add(f"edges_gone_shuffled_{n}", a, shuffled([bump(row, 0) if i % 3 == 0 else row for i, row in enumerate(gone)], "gone"),
                    kinds=(sorted_tree,))
        # new names: fresh, empty, a proper prefix and an extension of an existing name, 65 bytes; more new rows than T has leaves
        fresh = [(b"zz0001", ["1", "2"]), (b"", ["3", "4"]), (a[0][0][:5], ["5", "6"]), (a[0][0] + b"0", ["7", "8"]), (b"n" * 65, ["9", "10"])]
        fresh += [(f"new{k:05d}".encode(), [str(k), str(k + 1)]) for k in range(n + 3 if n <= 65 else 3)]
        mixed = list(a)
        for k, row in enumerate(fresh):                       # spread over the file, the first before row 0
            mixed.insert(min(len(mixed), k * max(1, n // len(fresh))), row)
        add(f"new_names_{n}", a, mixed)
    # a name twice in B, the rows more than 256 apart, the higher row with the changed balances: the first row wins, the leaf is SAME
    for n in (257, GROUP_ROWS + 2):
        a = base(n)
        add(f"twice_in_b_{n}", a, list(a) + [bump(a[0], 0)])
        b = list(a) + [a[3]]
        b[3] = bump(a[3], 1)                                   # ... and the other way round: the lower row changed, the higher as it was
        add(f"twice_in_b_first_changed_{n}", a, b)
    # a name twice in A: the head is owned, the shadowed leaf is UNREACHABLE; B names it once
    for n in (2, 65, 257):
        a = base(n)
        twice = list(a) + [(a[0][0], ["77", "78"])] + ([(a[n // 2][0], ["87", "88"]), (a[n // 2][0], ["97", "98"])] if n > 2 else [])
        add(f"twice_in_a_{n}", twice, [bump(row, 0) for row in a])
        add(f"twice_in_a_gone_{n}", twice, a[1:])
    # the empty name in T: found
    a = base(5) + [(b"", ["11", "12"])]
    add("empty_name_in_tree", a, [(b"", ["11", "13"]), a[1]])
    # equal as field elements, not as text
    a = [(b"alice", ["007", "5"]), (b"bob", ["7", "0"]), (b"carol", [str(R + 5), "1"]), (b"dave", ["1", "2"])]
    b = [(b"alice", ["7", str(R + 5)]), (b"bob", ["0007", str(R)]), (b"carol", ["5", "001"]), (b"dave", ["1", str(R + 3)])]
    add("field_equal", a, b)
    # one currency, and three at 65 rows
    a = base(65, 1)
    add("one_currency_65", a, shuffled([bump(row, 0) if i % 2 else row for i, row in enumerate(a)], "one"), nc=1)
    a = base(65, 3)
    add("three_currencies_65", a, shuffled([bump(row, 2) if i % 4 == 0 else row for i, row in enumerate(a)] + [(b"fresh", ["1", "2", "3"])],
                                           "three"), nc=3)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def text_of(rows, nc: int) -> str:
    return header(nc) + "".join(",".join([nm.decode()] + list(bal)) + "\n" for nm, bal in rows)


def model(a, b, nc: int, sorted_tree: bool, cap=None):
    """The report of B against the tree of A: {"n_tree", "depth", "row_leaf", "row_state", "leaf_state", "owner", "changed", "new",
    "gone", "summary" (in SUMMARY's order), "balances" (the owner row's integers mod r for every changed leaf, in the list's
    order), "leaf_rows" (the file row of A at every leaf)}"""
    order = leaf_order(a, sorted_tree)
    n_tree = len(a)
    depth = max(0, (n_tree - 1).bit_length())
    leaves = 1 << depth
    first = {}
    for leaf, r in enumerate(order):
        first.setdefault(a[r][0], leaf)
    row_leaf = [first.get(nm, ABSENT) for nm, _ in b]
    owner = [ABSENT] * leaves
    for r, leaf in enumerate(row_leaf):
        if leaf != ABSENT:
            owner[leaf] = min(owner[leaf], r)
    value = lambda bal: [int(x) % R for x in bal]
    row_state, leaf_state = [], [LEAF_PADDING] * leaves
    for r, leaf in enumerate(row_leaf):
        if leaf == ABSENT:
            row_state.append(ROW_NEW)
        elif owner[leaf] != r:
            row_state.append(ROW_SHADOWED)
        else:
            same = value(b[r][1]) == value(a[order[leaf]][1])
            row_state.append(ROW_SAME if same else ROW_CHANGED)
            leaf_state[leaf] = LEAF_SAME if same else LEAF_CHANGED
    for leaf, r in enumerate(order):
        if first[a[r][0]] != leaf:
            leaf_state[leaf] = LEAF_UNREACHABLE
        elif owner[leaf] == ABSENT:
            leaf_state[leaf] = LEAF_GONE
    changed = [i for i, s in enumerate(leaf_state) if s == LEAF_CHANGED]
    new = [r for r, s in enumerate(row_state) if s == ROW_NEW]
    gone = [i for i, s in enumerate(leaf_state) if s == LEAF_GONE]
    new_listed = len(new) if cap is None else min(cap, len(new))
    gone_listed = len(gone) if cap is None else min(cap, len(gone))
    summary = [len(new), row_state.count(ROW_SHADOWED), row_state.count(ROW_CHANGED), row_state.count(ROW_SAME), len(gone),
               leaf_state.count(LEAF_UNREACHABLE), new_listed, gone_listed]
    return {"n_tree": n_tree, "depth": depth, "row_leaf": row_leaf, "row_state": row_state, "leaf_state": leaf_state, "owner": owner,
            "changed": changed, "new": new[:new_listed], "gone": gone[:gone_listed], "summary": summary,
            "balances": [value(b[owner[leaf]][1]) for leaf in changed], "leaf_rows": order}


def caps_of(m):
    """the caps a case is asked with: caps_for of its new rows and of its gone leaves"""
    return sorted(set(caps_for(m["summary"][0])) | set(caps_for(m["summary"][4])))


# ----------------------------------------------------------------------------- past 64 groups: numpy only
# Every list's scatter sums the totals of the groups before an item's own by a wave: LANES = 64 totals a trip of its loop, then six
# shuffle steps.  An item's place takes a second trip only from group 65 on, item 65 * GROUP_ROWS; one of group 64 still sums
# exactly 64 groups in one trip.  BIG is the smallest size with items 65 * GROUP_ROWS - 1 (the last place of one full trip) and
# the first two that need a second: the tree of BIG rows has depth 21, 128 groups of leaves, and a file of BIG rows 66 of rows.
LANES = 64
TRIP_ROWS = LANES * GROUP_ROWS
BIG = 65 * GROUP_ROWS + 2
BIG_WIDTH = 7                                               # digits a name above a million names: byte order is numeric order
BIG_EDGES = (GROUP_ROWS, TRIP_ROWS, 65 * GROUP_ROWS)
BIG_NC = 2


def pattern(n: int, offsets, start: int = 0):
    """items e + d for every edge e of BIG_EDGES and d of offsets, and 1 + g % 5 items from `start` on in every group g: every
    group's total is non-zero and neighbours' differ"""
    out = {e + d for e in BIG_EDGES for d in offsets}
    for g in range(-(-n // GROUP_ROWS)):
        out |= {g * GROUP_ROWS + start + j for j in range(1 + g % 5)}
    return np.array(sorted(p for p in out if 0 <= p < n), dtype=np.int64)


def big_case(sorted_tree: bool, n: int = BIG):
    """A, B1 (the report case) and B2 (the apply case) as numbers: {"a": (keys, balances [n, 2]), "b1": (..), "b2": (..),
    "changed", "gone": the chosen leaves, "new": the renamed rows, "shadowed": the rows repeated at the end}.
    A is n distinct names in a seeded permutation.  The chosen leaves are leaves of the tree's kind.  Group 65 has two items,
    which the lists share: the gone leaves are e - 2 and e + 1 of every edge e and 1 + g % 5 leaves from the ninth on in every
    group, the changed leaves e - 1 and e and the first 1 + g % 5 of every group, less the gone ones.  B1 has A's rows in A's
    order, the changed leaves' first balance or second bumped, the gone leaves' rows under fresh names -- in a sorted tree also
    the rows e - 1, e, e + 1 and the first 1 + g % 5 of every group of rows, whose leaves lie anywhere: there the new rows' list
    has both rows of group 65 --, and three rows once more at the end.  B2 has A's names in A's order and the same bumps."""
    seed = int.from_bytes(f"mst_diff_cases.big.{n}".encode(), "little") % (1 << 63)
    keys = np.random.default_rng(seed).permutation(n).astype(np.int64)
    rows = np.arange(n, dtype=np.int64)
    bal = np.stack([10_000_000 + 2 * rows, 20_000_000 + 2 * rows + 1], axis=1)
    order = np.argsort(keys, kind="stable") if sorted_tree else rows           # the file row of A at every leaf
    leaf_of_row = np.empty(n, dtype=np.int64)
    leaf_of_row[order] = rows
    new_rows = order[pattern(n, (-2, 1), 8)]
    if sorted_tree:
        new_rows = np.union1d(new_rows, pattern(n, (-1, 0, 1)))
    new_rows = np.sort(new_rows)
    gone = np.sort(leaf_of_row[new_rows])
    changed = np.setdiff1d(pattern(n, (-1, 0)), gone)
    bumped = bal.copy()
    at = order[changed]
    bumped[at, changed % 2] += 1
    b1_keys, b1_bal = keys.copy(), bumped.copy()
    b1_keys[new_rows] = n + np.arange(new_rows.size)
    again = np.setdiff1d(rows, new_rows)[[0, 5, -1]]         # (of rows that keep their names: the later row is shadowed)
    b1_keys, b1_bal = np.concatenate([b1_keys, b1_keys[again]]), np.concatenate([b1_bal, b1_bal[again] + 5])
    return {"a": (keys, bal), "b1": (b1_keys, b1_bal), "b2": (keys, bumped), "changed": changed, "gone": gone, "new": new_rows,
            "shadowed": n + np.arange(3)}


def write_big(path, keys, bal):
    """a file of 7-digit names and two balances of 8 digits a row, without a per-row step"""
    from mst_names_cases import fixed_rows, write_fixed
    return write_fixed(path, bal.shape[1], fixed_rows(keys, BIG_WIDTH, list(bal.T)))


def fixed_width(rows):
    """are these rows' names digits of one width (model_np's)?"""
    return bool(rows) and all(nm.isdigit() and len(nm) == len(rows[0][0]) for nm, _ in rows)


def as_numbers(rows):
    """rows [(name bytes, [balance texts])] with fixed-width names -> (keys, balances [n, nc]); the balances are below 2^62"""
    return np.array([int(nm) for nm, _ in rows], dtype=np.int64), np.array([[int(x) for x in bal] for _, bal in rows], dtype=np.int64)


def model_np(a, b, sorted_tree: bool, cap=None):
    """model() for names of fixed-width digits, a and b as (keys, balances [n, nc]) of integers below r: the same keys, arrays for
    lists ("balances": [changed, nc], the owner rows')"""
    (a_keys, a_bal), (b_keys, b_bal) = a, b
    n_tree, n = a_keys.size, b_keys.size
    depth = max(0, (n_tree - 1).bit_length())
    leaves = 1 << depth
    order = np.argsort(a_keys, kind="stable") if sorted_tree else np.arange(n_tree, dtype=np.int64)
    by_leaf = a_keys[order]
    by_name = np.argsort(by_leaf, kind="stable")             # the leaves by name, equal names by leaf: a run's first is found
    s = by_leaf[by_name]
    heads = np.ones(n_tree, dtype=bool)
    heads[1:] = s[1:] != s[:-1]
    names, first_leaf = s[heads], by_name[heads]
    at = np.minimum(np.searchsorted(names, b_keys), names.size - 1)
    found = names[at] == b_keys
    rows = np.arange(n, dtype=np.int64)
    row_leaf = np.where(found, first_leaf[at], ABSENT)
    owner = np.full(leaves, ABSENT, dtype=np.int64)
    owned, at_first = np.unique(row_leaf[found], return_index=True)           # the first occurrence: the lowest row
    owner[owned] = rows[found][at_first]
    owns = found.copy()
    owns[found] = owner[row_leaf[found]] == rows[found]
    same = np.zeros(n, dtype=bool)
    same[owns] = (b_bal[owns] == a_bal[order[row_leaf[owns]]]).all(axis=1)
    row_state = np.where(~found, ROW_NEW, np.where(~owns, ROW_SHADOWED, np.where(same, ROW_SAME, ROW_CHANGED))).astype(np.uint8)
    leaf_state = np.full(leaves, LEAF_PADDING, dtype=np.uint8)
    leaf_state[:n_tree] = LEAF_GONE
    leaf_state[row_leaf[owns]] = np.where(same[owns], LEAF_SAME, LEAF_CHANGED)
    leaf_state[by_name[~heads]] = LEAF_UNREACHABLE
    changed, new, gone = (np.flatnonzero(x).astype(np.uint32) for x in (leaf_state == LEAF_CHANGED, row_state == ROW_NEW, leaf_state == LEAF_GONE))
    new_listed, gone_listed = (x.size if cap is None else min(cap, x.size) for x in (new, gone))
    count = lambda states, code: int(np.count_nonzero(states == code))
    summary = [int(new.size), count(row_state, ROW_SHADOWED), count(row_state, ROW_CHANGED), count(row_state, ROW_SAME), int(gone.size),
               count(leaf_state, LEAF_UNREACHABLE), new_listed, gone_listed]
    return {"n_tree": n_tree, "depth": depth, "row_leaf": row_leaf.astype(np.uint32), "row_state": row_state, "leaf_state": leaf_state,
            "owner": owner.astype(np.uint32), "changed": changed, "new": new[:new_listed], "gone": gone[:gone_listed], "summary": summary,
            "balances": b_bal[owner[changed]], "leaf_rows": order}
