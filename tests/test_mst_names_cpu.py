"""The name index beside a tree in file order and the duplicate-username report without a GPU: the rules of csrc/mst_names.h, whose
text the kernels compile, run by the header's own serial steps in tests/cpp/mst_names_check.cpp (behind the CSV reader's and the
sort's; built by the host compiler under address / undefined sanitizers, a process of its own) and compared with the model of
mst_names_cases.py on every case.  And the geometry against the case module's restatement, the exports of
include/summa_snapshot.h with the four new names in their place, what the four entry points refuse before they touch a device,
and `duplicate_names` of trees whose entries are on the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mst_names_cases as cases
import mst_sort_cases as sort_cases
from circuits_halo2_amd import ffi
from circuits_halo2_amd import merkle_sum_tree as M

SG_ERR_INVALID = -1
ABSENT = 0xFFFFFFFF
SORT_TILE = 2048
CASES = cases.cases(SORT_TILE)
ACCEPTED = [c for c in CASES if c[3] is None]
REFUSED = [c for c in CASES if c[3] is not None]
NEW = ["ss_mst_csv_name_index_dev", "ss_mst_find_leaves", "ss_mst_duplicate_names_scratch", "ss_mst_duplicate_names_dev"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_names") / "mst_names_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_names_check.cpp"), "-o", out])
    return out


def ask(exe, lines):
    """command lines -> the program's output lines, split into words"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def ask_files(exe, files):
    """[(path, nc, caps)] -> per file {"n", "flags", "problem", "order", "spans", "leafspans", "find", "dups": {(cap, ordered): report}}"""
    words = ask(exe, [f"file {path} {nc} " + " ".join(map(str, caps)) for path, nc, caps in files])
    out, cur, report = [], None, None
    for w in words:
        ints = lambda: [int(x) for x in w[1:]]
        if w[0] == "sort":
            cur = {"n": int(w[1]), "flags": int(w[2], 16), "problem": (int(w[3]), int(w[4])), "order": None, "dups": {}}
        elif w[0] in ("order", "spans", "leafspans", "find"):
            cur[w[0]] = ints()
        elif w[0] == "dups":
            report = {"summary": ints()[2:]}
            cur["dups"][(int(w[1]), bool(int(w[2])))] = report
        elif w[0] in ("shadowed", "first"):
            report[w[0]] = ints()
        elif w[0] == "end":
            out.append(cur)
    assert len(out) == len(files)
    return out


def _caps(content):
    return cases.caps_for(cases.model(cases.names_of(content))["summary"][1])


@pytest.fixture(scope="module")
def answers(exe, tmp_path_factory):
    """the program's answer for every case, by name: one run"""
    d = tmp_path_factory.mktemp("mst_names_files")
    files = [(cases.write_case(d, c[0], c[1]), c[2], _caps(c[1]) if c[3] is None else [0]) for c in CASES]
    return {c[0]: dict(a, path=f[0]) for c, f, a in zip(CASES, files, ask_files(exe, files))}


def test_the_geometry_is_the_case_modules_and_the_list_holds_what_it_must(exe):
    assert ask(exe, ["geometry"]) == [["geometry", str(cases.THREADS), str(cases.TILE), str(cases.GROUP)]]
    assert (cases.TILE, cases.GROUP, cases.GROUP_ROWS) == (64, 256, 16384)
    names = {c[0] for c in CASES}
    assert {f"none_{n}" for n in (1, 2, 64, 65, 257, 16386)} <= names and {f"edges_{n}" for n in (65, 257, 16386)} <= names
    assert {"run3_across_16386", "run3_ends_on_16386", "pairs_2", "empty_name_twice", "a_against_aa", "all_equal",
            "duplicates_a_tile_apart", "prefix_chain", "name_of_65_bytes"} <= names and {g[:-4] for g in cases.GOLDENS} <= names
    assert [c[3] for c in REFUSED] == [(2, sort_cases.NAME_TOO_LONG)]
    # where the family puts its runs: around positions 64, 256 and 16384 of the sorted order
    big = cases.multiset(16386, cases.EDGE_SETS["edges"])
    assert big[62] == big[63] == big[64] == big[65] != big[66] and big[16382] == big[16385] and big[61] != big[62]
    across = cases.multiset(16386, cases.EDGE_SETS["run3_across"])
    assert across[62] != across[63] == across[64] == across[65] != across[66] and across[16383] == across[16385]
    ends = cases.multiset(16386, cases.EDGE_SETS["run3_ends_on"])
    assert ends[60] != ends[61] == ends[62] == ends[63] != ends[64] and ends[16381] == ends[16383] != ends[16384]


def test_scratch_size_and_a_second_group(exe):
    L = ffi.snapshot_lib()
    size = C.c_uint64(77)
    for n in (0, 1 << 32):
        assert L.ss_mst_duplicate_names_scratch(n, C.byref(size)) == SG_ERR_INVALID and size.value == 77
    assert L.ss_mst_duplicate_names_scratch(5, None) == SG_ERR_INVALID
    sizes = [1, 63, 64, 65, 16384, 16385, 16386, 32769, (1 << 20), (1 << 32) - 1]
    for n, words in zip(sizes, ask(exe, [f"scratch {n}" for n in sizes])):
        assert L.ss_mst_duplicate_names_scratch(n, C.byref(size)) == 0
        tiles = -(-n // 64)
        groups = -(-tiles // 256)
        assert [size.value, tiles, groups] == [4 * (4 + tiles + groups)] + [int(x) for x in words[2:]] and int(words[1]) == size.value, n
    assert ask(exe, ["scratch 16384", "scratch 16386", "scratch 32769"]) == [["scratch", str(4 * (4 + 256 + 1)), "256", "1"],
                                                                             ["scratch", str(4 * (4 + 257 + 2)), "257", "2"],
                                                                             ["scratch", str(4 * (4 + 513 + 3)), "513", "3"]]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_the_mirror_agrees_with_the_model(answers, case):
    name, content, _, _ = case
    mirror_agrees_with_the_model(answers[name], cases.names_of(content), name)


def mirror_agrees_with_the_model(a, names, name):
    want = sort_cases.stable_order(names)
    assert a["flags"] == 0 and a["problem"] == (0, 0) and a["n"] == len(names), name
    assert a["order"] == want, name
    with open(a["path"], "rb") as f:
        body = f.read()
    body = body[body.index(b"\n") + 1:]
    span = lambda v, i: body[v[2 * i]:v[2 * i + 1]]
    assert [span(a["spans"], i) for i in range(len(names))] == [names[r] for r in want], name
    assert [span(a["leafspans"], r) for r in range(len(names))] == names, name
    first = cases.first_rows(names)
    assert a["find"] == [first[nm] for nm in names] + [ABSENT, ABSENT], name       # list.index: the reference's position()
    count = cases.model(names)["summary"][1]
    assert sorted(cap for cap, _ in a["dups"]) == sorted(2 * cases.caps_for(count))
    for (cap, ordered), got in a["dups"].items():
        assert got == cases.model(names, cap, ordered), (name, cap, ordered)
    full = a["dups"][(count, True)]
    assert all(first[names[leaf]] == head and leaf > head for leaf, head in zip(full["shadowed"], full["first"])), name
    assert sorted(full["shadowed"]) == [r for r, nm in enumerate(names) if first[nm] != r], name


def test_known_reports(answers):
    full = lambda name: [v for (cap, ordered), v in answers[name]["dups"].items() if ordered and cap == v["summary"][1]][0]
    assert full("all_equal") == {"summary": [1, 69, 69], "shadowed": list(range(1, 70)), "first": [0] * 69}
    assert full("empty_name_twice") == {"summary": [1, 1, 1], "shadowed": [3], "first": [1]}
    assert full("a_against_aa")["summary"] == full("prefix_chain")["summary"] == full("entry_16")["summary"] == [0, 0, 0]
    far = full("duplicates_a_tile_apart")
    t = SORT_TILE
    # the planted names; the short random ones repeat as well
    assert {(0, t + 1), (0, 2 * t + 9), (3, t + 7), (3, 2 * t + 5), (5, t + 5)} <= set(zip(far["first"], far["shadowed"]))
    assert full("pairs_2") == {"summary": [1, 1, 1], "shadowed": [answers["pairs_2"]["order"][1]], "first": [answers["pairs_2"]["order"][0]]}
    assert full("edges_16386")["summary"] == [3, 9, 9] and full("run3_across_16386")["summary"] == [3, 6, 6]
    assert full("none_16386")["summary"] == [0, 0, 0]


def test_the_pool_reaches_a_third_group_with_almost_every_row_shadowed(exe, tmp_path):
    text, nc = sort_cases.large(cases.LARGE, SORT_TILE)
    names = cases.names_of(text)
    count = len(names) - 300
    assert len(names) == 32769 and len(set(names)) == 300 and -(-len(names) // cases.GROUP_ROWS) == 3
    path = cases.write_case(tmp_path, cases.LARGE, text)
    a = dict(ask_files(exe, [(path, nc, cases.caps_for(count))])[0], path=path)
    mirror_agrees_with_the_model(a, names, cases.LARGE)
    assert a["dups"][(count, True)]["summary"] == [300, count, count]


def _same_as_model(got, want, what):
    assert {k: (v if k == "summary" else v.tolist()) for k, v in got.items()} == want, what


def test_the_numpy_model_is_the_model_on_every_case_and_the_pool():
    text, _ = sort_cases.large(cases.LARGE, SORT_TILE)
    generated = [c for c in ACCEPTED if c[0].rsplit("_", 1)[0] in cases.EDGE_SETS]
    assert {c[0] for c in generated} >= {f"edges_{n}" for n in (65, 257, 16386)} | {f"none_{n}" for n in cases.SIZES}
    for name, content in [(c[0], c[1]) for c in ACCEPTED] + [(cases.LARGE, text)]:
        names = cases.names_of(content)
        keys = cases.keys_of(names)
        assert np.argsort(keys, kind="stable").tolist() == sort_cases.stable_order(names), name
        count = cases.model(names)["summary"][1]
        for cap in [None] + cases.caps_for(count):
            for ordered in (True, False):
                _same_as_model(cases.model_np(keys, cap, ordered), cases.model(names, cap, ordered), (name, cap, ordered))
    # a name width: the family at 7 digits is the family, and the fixed-width writer writes what rows_text does
    seven = cases.generated(257, "edges", 7)
    assert [int(nm) for nm in seven] == [int(nm) for nm in cases.generated(257, "edges")] and {len(nm) for nm in seven} == {7}
    keys = cases.keys_of([nm.encode() for nm in seven])
    rows = np.arange(257)
    body = cases.fixed_rows(keys, 7, [1000 * rows + 1, 1000 * rows + 2], 6).tobytes().decode()
    assert body == "".join(f"{nm},{1000 * i + 1:06d},{1000 * i + 2:06d}\n" for i, nm in enumerate(seven))


def test_the_big_case_is_built_from_the_edges_past_64_groups():
    """what BIG is for -- a wave sums LANES group totals a trip -- and where the big case puts its shadowed positions"""
    assert (cases.LANES, cases.TRIP_ROWS, cases.BIG) == (64, 64 * cases.GROUP_ROWS, 65 * cases.GROUP_ROWS + 2) and cases.BIG == 1_064_962
    group = lambda item: item // cases.GROUP_ROWS             # the groups before an item's own are 0 .. group - 1
    trips = lambda item: -(-group(item) // cases.LANES)
    assert [trips(cases.BIG - 3), trips(cases.BIG - 2), trips(cases.BIG - 1)] == [1, 2, 2] and group(cases.BIG - 3) == cases.LANES
    assert trips(cases.TRIP_ROWS) == 1 and group(cases.TRIP_ROWS - 1) == cases.LANES - 1 and 10 ** (cases.BIG_WIDTH - 1) < cases.BIG
    edges = cases.big_edges()
    assert {e + d for e in (cases.GROUP_ROWS, cases.TRIP_ROWS, 65 * cases.GROUP_ROWS) for d in (-1, 0, 1)} <= set(edges.tolist())
    per_group = np.bincount(edges // cases.GROUP_ROWS, minlength=66)
    assert per_group.size == 66 and per_group.min() >= 1 and (per_group[1:] != per_group[:-1]).all() and per_group[65] == 2
    # the generator at a size Python affords is multiset's, and at BIG its sorted names repeat exactly at the edges
    small = cases.big_keys(3 * cases.GROUP_ROWS + 2, "small")
    assert sorted(f"{k:07d}" for k in small.tolist()) == cases.multiset(small.size, cases.big_edges(small.size).tolist(), 7)
    keys = cases.big_keys()
    order, same = cases.shadowed_positions(keys)
    assert keys.size == cases.BIG and np.array_equal(np.flatnonzero(same), edges) and keys.max() == cases.BIG - 1 - edges.size
    assert not np.array_equal(order, np.arange(cases.BIG))
    m = cases.model_np(keys)
    assert m["summary"][1:] == [edges.size, edges.size] and (m["shadowed"] > m["first"]).all()
    assert np.array_equal(keys[m["shadowed"]], keys[m["first"]])


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_a_name_over_the_cap_is_reported(answers, case):
    a = answers[case[0]]
    assert a["flags"] == 0 and a["problem"] == case[3] and a["order"] is None


# ============================================================================= the entry points: exports and refusals
def test_exports_are_the_headers_prototypes_the_new_names_in_their_place():
    text = open(os.path.join(ROOT, "include", "summa_snapshot.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(ss_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = [name for name, _ in protos]
    assert names == ffi.SNAPSHOT_EXPORTS == list(ffi.SNAPSHOT_ARGTYPES)
    at = names.index("ss_mst_find_names")
    assert names[at + 1:at + 5] == NEW and names[at + 5:] == ["ss_mst_range_audit_scratch", "ss_mst_range_audit_dev"]
    L = ffi.snapshot_lib()
    for name, args in protos:
        if name in NEW:
            getattr(L, name)
            assert len(ffi.SNAPSHOT_ARGTYPES[name]) == len(args.split(",")), name
    gpu_h = open(os.path.join(ROOT, "include", "summa_gpu.h")).read()
    assert not any(name in gpu_h for name in NEW)


def name_index(**change):
    """a good call but for `change`; the device pointers are not memory: a refused call never uses them"""
    a = dict(d_bytes=0x10000, length=100, body_off=10, tiles=0x20000, delim=ord(","), nc=2, n=3, spans=0x30000, sort=0x60000, order=0x70000,
             name_spans=0x80000, leaf_spans=0x90000, out=True)
    a.update(change)
    problem = C.c_uint64(77)
    rc = ffi.snapshot_lib().ss_mst_csv_name_index_dev(a["d_bytes"], a["length"], a["body_off"], a["tiles"], a["delim"], a["nc"], a["n"], a["spans"],
                                                      a["sort"], a["order"], a["name_spans"], a["leaf_spans"],
                                                      C.byref(problem) if a["out"] else None, None)
    assert problem.value == 77
    return rc, ffi.lib().sg_last_error().decode()


def test_name_index_refuses_bad_arguments():
    for change in ({"d_bytes": None}, {"tiles": None}, {"spans": None}, {"sort": None}, {"order": None}, {"name_spans": None},
                   {"leaf_spans": None}, {"out": False}):
        rc, msg = name_index(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_csv_name_index: ") and "null" in msg, change
    for change in ({"nc": 0}, {"nc": 65}, {"body_off": 101}, {"body_off": 100}, {"length": (1 << 32) + 10}, {"n": 0}, {"n": 91}, {"n": 1 << 32},
                   {"tiles": 0x20002}, {"spans": 0x30004}, {"delim": 10}, {"delim": 13}, {"delim": ord("5")}, {"delim": ord('"')}, {"delim": 0},
                   {"delim": 0xC3}, {"delim": 256 + ord(",")}, {"sort": 0x60008}, {"order": 0x70002}, {"name_spans": 0x80002},
                   {"leaf_spans": 0x90001}):
        rc, msg = name_index(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_csv_name_index: ") and "bad size" in msg, change


def find_leaves(**change):
    a = dict(d_bytes=0x10000, length=100, body_off=10, name_spans=0x80000, order=0x70000, n=3, names=np.frombuffer(b"abcde", dtype=np.uint8).copy(),
             off=np.array([0, 2, 5], dtype=np.uint64), m=2, out=True)
    a.update(change)
    found = np.full(4, 77, dtype=np.uint32)
    rc = ffi.snapshot_lib().ss_mst_find_leaves(a["d_bytes"], a["length"], a["body_off"], a["name_spans"], a["order"], a["n"],
                                               None if a["names"] is None else ffi.ptr(a["names"]), None if a["off"] is None else ffi.ptr(a["off"]),
                                               a["m"], ffi.ptr(found) if a["out"] else None, None)
    assert (found == 77).all()
    return rc, ffi.lib().sg_last_error().decode()


def test_find_leaves_refuses_bad_arguments():
    for change in ({"d_bytes": None}, {"name_spans": None}, {"order": None}, {"names": None}, {"off": None}, {"out": False}):
        rc, msg = find_leaves(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_find_leaves: ") and "null" in msg, change
    for change in ({"m": 0}, {"n": 0}, {"n": 1 << 32}, {"body_off": 101}, {"length": (1 << 32) + 10}, {"name_spans": 0x80002}, {"order": 0x70002}):
        rc, msg = find_leaves(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_find_leaves: ") and "bad size" in msg, change
    rc, msg = find_leaves(off=np.array([1, 2, 5], dtype=np.uint64))
    assert rc == SG_ERR_INVALID and "start at 0" in msg
    rc, msg = find_leaves(off=np.array([0, 3, 2], dtype=np.uint64))
    assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_find_leaves: ") and "decrease" in msg


GOOD = dict(d_bytes=0x10000, length=100, body_off=10, name_spans=0x80000, order=0x70000, n=3, shadowed=0x200000, first=0x300000, cap=3,
            scratch=0x500000, out=True)
KEYS = ("d_bytes", "length", "body_off", "name_spans", "order", "n", "shadowed", "first", "cap", "scratch", "out")


def duplicate_names(**change):
    a = dict(GOOD, **change)
    summary = (C.c_uint64 * 3)(71, 72, 73)
    rc = ffi.snapshot_lib().ss_mst_duplicate_names_dev(a["d_bytes"], a["length"], a["body_off"], a["name_spans"], a["order"], a["n"], a["shadowed"],
                                                       a["first"], a["cap"], a["scratch"], summary if a["out"] else None, None)
    assert list(summary) == [71, 72, 73]
    return rc, ffi.lib().sg_last_error().decode()


def test_duplicate_names_refuses_bad_arguments(exe):
    refused = [({"d_bytes": None}, "null"), ({"name_spans": None}, "null"), ({"scratch": None}, "null"), ({"out": False}, "null"),
               ({"shadowed": None}, "non-zero cap"), ({"first": None}, "non-zero cap"), ({"shadowed": None, "first": None, "cap": 1 << 40}, "non-zero cap"),
               ({"n": 0}, "n_rows"), ({"n": 1 << 32}, "n_rows"), ({"n": 1 << 40}, "n_rows"), ({"body_off": 101}, "body_off"),
               ({"length": (1 << 32) + 10}, "body"), ({"name_spans": 0x80002}, "d_name_spans"), ({"order": 0x70001}, "d_order"),
               ({"shadowed": 0x200002}, "d_shadowed"), ({"first": 0x300003}, "d_first"), ({"scratch": 0x500002}, "d_scratch")]
    for change, word in refused:
        rc, msg = duplicate_names(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_duplicate_names: ") and word in msg, (change, msg)
    # the same words from the header's own function, and "" for what the entry point accepts: no order (a sorted tree), null lists
    # with cap == 0, a body of 2^32 - 1 bytes
    def problem(**change):
        a = dict(dict(GOOD, out=0x600000), **{k: (0 if v is False else v) for k, v in change.items()})
        return " ".join(ask(exe, ["problem " + " ".join(str(a[k] or 0) for k in KEYS)])[0][1:])
    assert problem() == "" and problem(order=None) == "" and problem(shadowed=None, first=None, cap=0) == "" and problem(cap=0) == ""
    assert problem(length=(1 << 32) + 9, n=(1 << 32) - 1) == "" and problem(body_off=100) == ""
    for change, word in refused:
        assert word in problem(**change), change


# ============================================================================= duplicate_names of trees whose entries are on the host
class _HostTree(M._Tree):
    """entries alone: what the base implementation reads"""

    def __init__(self, entries, is_sorted=False):
        self.entries, self.is_sorted, self.n_currencies, self.depth = entries, is_sorted, 2, max(0, (len(entries) - 1).bit_length())


@pytest.mark.parametrize("name", ["edges_257", "all_equal", "duplicates_a_tile_apart", "empty_name_twice", "none_65", "entry_16"])
def test_duplicate_names_from_entries(name):
    content = [c[1] for c in CASES if c[0] == name][0]
    names = cases.names_of(content)
    entries = [(nm.decode(), [i, i + 1]) for i, nm in enumerate(names)]
    padded = entries + [(None, [0, 0])] * ((1 << max(0, (len(entries) - 1).bit_length())) - len(entries))
    count = cases.model(names)["summary"][1]
    for cap in [None] + cases.caps_for(count):
        got = _HostTree(list(padded)).duplicate_names(cap)
        want = cases.model(names, cap)
        assert [got.n_repeated_names, got.n_shadowed, len(got.shadowed)] == want["summary"], (name, cap)
        assert got.shadowed.dtype == got.first.dtype == np.uint32
        assert got.shadowed.tolist() == want["shadowed"] and got.first.tolist() == want["first"] and got.ok == (count == 0)
    # the same entries in sorted order, as from_csv_sorted holds them: the leaves are the sorted positions
    by_name = sorted(entries, key=lambda e: e[0].encode())
    got = _HostTree(by_name, is_sorted=True).duplicate_names()
    want = cases.model(names, None, in_file_order=False)
    assert got.shadowed.tolist() == want["shadowed"] and got.first.tolist() == want["first"]
    groups = got.groups()
    assert sum(map(len, groups.values())) == count and all(by_name[h][0] == by_name[leaf][0] for h, ls in groups.items() for leaf in ls)
    tree = _HostTree(list(padded))
    named = tree.named_groups(tree.duplicate_names(), limit=2)
    assert named == [(entries[h][0], [h] + ls) for h, ls in list(tree.duplicate_names().groups().items())[:2]]


def test_duplicate_names_needs_entries_and_a_sane_cap():
    with pytest.raises(ValueError, match="holds no entries"):
        _HostTree.duplicate_names(type("T", (M._Tree,), {"entries": None})())
    with pytest.raises(ValueError, match="cap below 0"):
        _HostTree([("a", [1, 2])]).duplicate_names(-1)
    dups = M.DuplicateNames(1, 2, [7, 9], [3, 3])
    assert dups.groups() == {3: [7, 9]} and not dups.ok and M.DuplicateNames(0, 0, [], []).ok
    assert os.path.exists(os.path.join(GOLDEN, "entry_16.csv"))
