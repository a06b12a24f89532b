"""The snapshot CSVs the name index and the duplicate-username report are checked with, on the host (test_mst_names_cpu.py: the
serial steps of csrc/mst_names.h behind the reader's and the sort's) and on the device (test_gpu_mst_names.py), and the model
both are compared with.  Every case is (name, text or golden file name, n_currencies, refusal), as in mst_sort_cases.py.

The report compacts the shadowed positions by a ballot per wave of TILE = 64 sorted positions, a scan per workgroup over GROUP =
256 tile counts, and the groups' totals (MST_NAMES_TILE, MST_NAMES_GROUP and MST_NAMES_THREADS of csrc/mst_names.h, restated; the
check program prints them).  The generated family places duplicates by SORTED POSITION: from distinct names f"{k:06d}" the sorted
multiset M has M[p] = M[p - 1] for every p of a set of edges and a fresh name otherwise; the rows are M in a seeded shuffle, and
balances are distinct per row, so that file order shows in the leaves."""
import random

import numpy as np

import mst_sort_cases as sort_cases
from mst_csv_cases import GOLDENS, header, write_case  # noqa: F401  (write_case: for the tests that import this module)

THREADS, TILE, GROUP = 256, 64, 256
GROUP_ROWS = TILE * GROUP                                   # 16384 positions: one workgroup of the groups step
SIZES = (1, 2, 64, 65, 257, GROUP_ROWS + 2)                 # 16386: the smallest file with positions 16383, 16384 and 16385
WAVE_EDGE, BLOCK_EDGE, GROUP_EDGE = TILE, THREADS, GROUP_ROWS
# name -> the positions p with M[p] = M[p - 1]
EDGE_SETS = {
    "none": (),
    # the positions on both sides of the wave, workgroup and group edge: runs of four, heads at edge - 2
    "edges": tuple(e + d for e in (WAVE_EDGE, BLOCK_EDGE, GROUP_EDGE) for d in (-1, 0, 1)),
    # a run of 3 across each edge, its head the last position before it: the first lane of a wave is shadowed, the lane before not
    "run3_across": tuple(e + d for e in (WAVE_EDGE, BLOCK_EDGE, GROUP_EDGE) for d in (0, 1)),
    # a run of 3 that ends exactly on each edge: its last row is the last position of a tile, the next tile starts fresh
    "run3_ends_on": tuple(e + d for e in (WAVE_EDGE, BLOCK_EDGE, GROUP_EDGE) for d in (-2, -1)),
    # pairs: position 1 (the lowest that can be shadowed) and the first position of a tile, a workgroup and a group alone
    "pairs": (1, WAVE_EDGE, BLOCK_EDGE, GROUP_EDGE),
}


def multiset(n: int, edges, width: int = 6):
    """the sorted names: M[p] = M[p - 1] for p in edges, else the next fresh name"""
    edges, out, k = set(edges), [], 0
    for p in range(n):
        if p and p in edges:
            out.append(out[-1])
        else:
            out.append(f"{k:0{width}d}")
            k += 1
    return out


def generated(n: int, edge_set: str, width: int = 6):
    """the names of the rows in file order: the multiset in a seeded shuffle"""
    names = multiset(n, EDGE_SETS[edge_set], width)
    random.Random(f"mst_names_cases.{edge_set}.{n}").shuffle(names)
    return names


def cases(tile: int = 2048):
    """`tile`: the sort's tile (mst_sort_cases.cases places its duplicates by it)"""
    h = header(2)
    out = []
    for n in SIZES:
        for edge_set, edges in EDGE_SETS.items():
            if edge_set == "none" or any(0 < p < n for p in edges):
                out.append((f"{edge_set}_{n}", h + sort_cases.rows_text(generated(n, edge_set)), 2, None))
    out.append(("empty_name_twice", h + sort_cases.rows_text(["x", "", "a", "", "aa"]), 2, None))
    out.append(("a_against_aa", h + sort_cases.rows_text(["aa", "a", "aaa", "b"]), 2, None))          # prefixes are not equal names
    taken = {"all_equal", "duplicates_a_tile_apart", "prefix_chain", "name_of_65_bytes"} | {g[:-4] for g in GOLDENS}
    out += [c for c in sort_cases.cases(tile) if c[0] in taken]
    names = [c[0] for c in out]
    assert len(set(names)) == len(names) and taken <= set(names)
    return out


LARGE = "pool_300_32769"                                    # three groups, almost every row shadowed


def names_of(content):
    """the names of a case's rows in file order, as bytes: the text's, or a golden file's"""
    if content.endswith(".csv") and "\n" not in content:
        with open(write_case(None, "", content), "rb") as f:
            content = f.read().decode()
    lines = content.split("\n")
    delim = ";" if ";" in lines[0] else ","
    return [ln.rstrip("\r").split(delim, 1)[0].encode() for ln in lines[1:] if ln.rstrip("\r")]


def model(names, cap=None, in_file_order: bool = True):
    """The report for rows with these names (bytes, file order): {"summary": [repeated names, shadowed rows, rows listed],
    "shadowed": [...], "first": [...]}.  Sorted position i >= 1 is shadowed iff its name equals the one at i - 1; the leaves are
    file rows for a tree in file order, sorted positions for a sorted tree."""
    order = sort_cases.stable_order(names)
    leaf = (lambda i: order[i]) if in_file_order else (lambda i: i)
    shadowed, first, repeated, head = [], [], 0, 0
    for i in range(1, len(order)):
        if names[order[i]] != names[order[i - 1]]:
            head = i
            continue
        if head == i - 1:
            repeated += 1
        shadowed.append(leaf(i))
        first.append(leaf(head))
    listed = len(shadowed) if cap is None else min(cap, len(shadowed))
    return {"summary": [repeated, len(shadowed), listed], "shadowed": shadowed[:listed], "first": first[:listed]}


def caps_for(count: int):
    """the caps every case is asked with: none listed, one, all but one, all, more than all"""
    return sorted({0, 1, max(count - 1, 0), count, count + 5})


def first_rows(names):
    """{name: the lowest file row that holds it}: list.index"""
    out = {}
    for row, name in enumerate(names):
        out.setdefault(name, row)
    return out


# ----------------------------------------------------------------------------- past 64 groups: numpy only
# The scatter sums the totals of the groups before a position's own by a wave: LANES = 64 totals a trip of its loop, then six
# shuffle steps.  A position's place takes a second trip only from group 65 on, position 65 * GROUP_ROWS; one of group 64 still
# sums exactly 64 groups in one trip.  BIG is the smallest size with positions 65 * GROUP_ROWS - 1 (the last place of one full
# trip) and the first two that need a second.  Above a million names the width is 7 digits: byte order is numeric order.
LANES = 64
TRIP_ROWS = LANES * GROUP_ROWS
BIG = 65 * GROUP_ROWS + 2
BIG_WIDTH = 7
BIG_EDGES = (GROUP_ROWS, TRIP_ROWS, 65 * GROUP_ROWS)


def big_edges(n: int = BIG, edges=BIG_EDGES):
    """the positions p with M[p] = M[p - 1]: both sides of the group edge, of the end of a trip and of the start of group 65,
    and 1 + g % 5 positions at the start of every group g, so that every group's total is non-zero and neighbours' differ"""
    out = {e + d for e in edges for d in (-1, 0, 1)}
    for g in range(-(-n // GROUP_ROWS)):
        out |= {g * GROUP_ROWS + j for j in range(1 + g % 5)}
    return np.array(sorted(p for p in out if 0 < p < n), dtype=np.int64)


def big_keys(n: int = BIG, tag: str = "names"):
    """the big case's names as numbers, in file order: multiset(n, big_edges(n)) in a seeded permutation"""
    fresh = np.ones(n, dtype=bool)
    fresh[big_edges(n)] = False
    m = np.cumsum(fresh) - 1
    seed = int.from_bytes(f"mst_names_cases.big.{tag}.{n}".encode(), "little") % (1 << 63)
    return m[np.random.default_rng(seed).permutation(n)]


def digits(values, width: int):
    """integers -> their decimal digits, zero-padded: uint8 [len, width]"""
    values = np.asarray(values, dtype=np.int64)
    assert values.size == 0 or (values.min() >= 0 and values.max() < 10 ** width)
    return (values[:, None] // 10 ** np.arange(width - 1, -1, -1, dtype=np.int64) % 10 + ord("0")).astype(np.uint8)


def fixed_rows(keys, width: int, balances, balance_width: int = 8, delim: str = ","):
    """the body of a CSV whose rows have one width: the name's `width` digits and every column of `balances` in `balance_width`
    digits -> uint8, one allocation and no per-row Python"""
    cols = []
    for column in [digits(keys, width)] + [digits(b, balance_width) for b in balances]:
        cols += [column, np.full((len(keys), 1), ord(delim), dtype=np.uint8)]
    cols[-1] = np.full((len(keys), 1), ord("\n"), dtype=np.uint8)
    return np.concatenate(cols, axis=1).reshape(-1)


def write_fixed(path, nc: int, body):
    """header(nc) and a body of fixed_rows -> path"""
    with open(path, "wb") as f:
        f.write(header(nc).encode())
        body.tofile(f)
    return str(path)


def keys_of(names):
    """names (bytes, file order) -> integers that order as the names' bytes do: the numbers of fixed-width digits, else ranks"""
    if names and all(nm.isdigit() and len(nm) == len(names[0]) for nm in names):
        return np.array([int(nm) for nm in names], dtype=np.int64)
    rank = {nm: k for k, nm in enumerate(sorted(set(names)))}
    return np.array([rank[nm] for nm in names], dtype=np.int64)


def shadowed_positions(keys):
    """(the stable order, which sorted positions are shadowed: bool per position)"""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")
    s = keys[order]
    same = np.zeros(keys.size, dtype=bool)
    same[1:] = s[1:] == s[:-1]
    return order, same


def model_np(keys, cap=None, in_file_order: bool = True):
    """model() over integer keys, in numpy: the lists are uint32 arrays"""
    order, same = shadowed_positions(keys)
    pos = np.arange(order.size, dtype=np.int64)
    head = np.maximum.accumulate(np.where(same, 0, pos))      # the start of every position's run
    at = np.flatnonzero(same)
    leaf = order if in_file_order else pos
    listed = at.size if cap is None else min(cap, at.size)
    repeated = int(np.count_nonzero(same[1:] & ~same[:-1]))
    return {"summary": [repeated, int(at.size), listed], "shadowed": leaf[at[:listed]].astype(np.uint32),
            "first": leaf[head[at[:listed]]].astype(np.uint32)}
