"""The snapshot CSVs the name index and the duplicate-username report are checked with, on the host (test_mst_names_cpu.py: the
serial steps of csrc/mst_names.h behind the reader's and the sort's) and on the device (test_gpu_mst_names.py), and the model
both are compared with.  Every case is (name, text or golden file name, n_currencies, refusal), as in mst_sort_cases.py.

The report compacts the shadowed positions by a ballot per wave of TILE = 64 sorted positions, a scan per workgroup over GROUP =
256 tile counts, and the groups' totals (MST_NAMES_TILE, MST_NAMES_GROUP and MST_NAMES_THREADS of csrc/mst_names.h, restated; the
check program prints them).  The generated family places duplicates by SORTED POSITION: from distinct names f"{k:06d}" the sorted
multiset M has M[p] = M[p - 1] for every p of a set of edges and a fresh name otherwise; the rows are M in a seeded shuffle, and
balances are distinct per row, so that file order shows in the leaves."""
import random

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


def multiset(n: int, edges):
    """the sorted names: M[p] = M[p - 1] for p in edges, else the next fresh name"""
    edges, out, k = set(edges), [], 0
    for p in range(n):
        if p and p in edges:
            out.append(out[-1])
        else:
            out.append(f"{k:06d}")
            k += 1
    return out


def generated(n: int, edge_set: str):
    """the names of the rows in file order: the multiset in a seeded shuffle"""
    names = multiset(n, EDGE_SETS[edge_set])
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
