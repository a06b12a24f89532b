"""The device sort of a snapshot's usernames without a GPU: the rules, the work space and the tile edges of csrc/mst_sort.h, whose
text the kernels compile, run by the header's own serial steps in tests/cpp/mst_sort_check.cpp (after the CSV reader's four
passes), built by the host compiler under address / undefined sanitizers.  One fixed list of files (mst_sort_cases.py): every
accepted one comes out in Python's stable order of the names' bytes, the refused one with its (row, 7).  The list LARGE the same,
with the proof that it reaches one, two and three steps of a pass's one-workgroup scan, whose width is restated in
mst_sort_cases.py and compared with the header's here, and that two of its files read a carried sum.  And the geometry, the
exports of include/summa_snapshot.h, and what its two entry points refuse before they touch a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

import mst_sort_cases as cases
from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import _check_balance_rows, parse_csv_to_entries

SG_ERR_INVALID = -1
TILE, CAP = 2048, 64                                      # what the header must say (asserted from the program's output)
ABSENT = 0xFFFFFFFF
CASES = cases.cases(TILE)
ACCEPTED = [c for c in CASES if c[3] is None]
REFUSED = [c for c in CASES if c[3] is not None]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_sort") / "mst_sort_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_sort_check.cpp"), "-o", out])
    return out


def ask(exe, files):
    """[(path, nc)] -> per file {"body", "geom", "n", "flags", "problem": (row, code), "longest", "passes", "order", "spans", "find"}"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    text = "".join(f"{path} {nc}\n" for path, nc in files)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out, cur = [], None
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "body":
            cur = {"body": int(w[1]), "order": None, "spans": None, "find": None}
            assert (int(w[3]), int(w[4])) == (TILE, CAP)
        elif w[0] == "geom":
            cur["geom"] = tuple(int(x) for x in w[1:])                  # (SCAN_BLOCK, SCAN_ITEMS, BINS, tiles, steps)
        elif w[0] == "sort":
            cur.update(n=int(w[1]), flags=int(w[2], 16), problem=(int(w[3]), int(w[4])), longest=int(w[5]), passes=int(w[6]))
        elif w[0] in ("order", "spans", "find"):
            cur[w[0]] = [int(x) for x in w[1:]]
        elif w[0] == "end":
            out.append(cur)
    assert len(out) == len(files)
    return out


@pytest.fixture(scope="module")
def answers(exe, tmp_path_factory):
    """the program's answer for every case, by name: one run"""
    d = tmp_path_factory.mktemp("mst_sort_files")
    files = [(cases.write_case(d, c[0], c[1]), c[2]) for c in CASES]
    return {c[0]: dict(a, path=path) for c, (path, _), a in zip(CASES, files, ask(exe, files))}


def test_the_list_holds_what_it_must():
    names = {c[0] for c in CASES}
    assert {f"random_{n}" for n in (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)} <= names
    assert {g[:-4] for g in cases.GOLDENS} <= names and len(cases.GOLDENS) == 7
    assert [c[3] for c in REFUSED] == [(2, cases.NAME_TOO_LONG)] and cases.NAME_CAP == CAP


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted_files_come_out_in_pythons_stable_order(answers, case):
    name, _, nc, _ = case
    comes_out_in_pythons_stable_order(answers[name], name, nc)


def comes_out_in_pythons_stable_order(a, name, nc):
    # the host's steps of today's from_csv_sorted succeed on the file: the parse, the sort, from_entries' checks (what is left
    # of it is hashing on the device: tests/test_gpu_mst_sort.py builds the tree)
    entries, _ = parse_csv_to_entries(a["path"], nc)
    host_sorted = sorted(entries, key=lambda e: e[0].encode())
    _check_balance_rows([bal for _, bal in host_sorted], nc, "entry with a wrong number of balances")
    assert entries
    names = [e[0].encode() for e in entries]
    want = cases.stable_order(names)
    assert a["flags"] == 0 and a["problem"] == (0, 0) and a["n"] == len(names), name
    assert a["order"] == want, name
    assert [(name_, bal) for name_, bal in host_sorted] == [entries[i] for i in a["order"]]
    with open(a["path"], "rb") as f:
        body = f.read()[a["body"]:]
    spans = a["spans"]
    assert [body[spans[2 * i]:spans[2 * i + 1]] for i in range(len(names))] == [names[i] for i in want], name
    assert a["longest"] == max(map(len, names))
    varying = sum(1 for p in range(a["longest"]) if len({nm[p] if p < len(nm) else 0 for nm in names}) > 1)
    assert a["passes"] == varying, f"{name}: a pass runs exactly where the names' bytes differ"
    # lookup: every leaf's own name gives the first leaf that holds it; a name above all and one below all non-empty are absent
    sorted_names = [names[i] for i in want]
    first = {}
    for i, nm in enumerate(sorted_names):
        first.setdefault(nm, i)
    assert a["find"] == [first[nm] for nm in sorted_names] + [ABSENT, ABSENT], name


def test_all_equal_names_run_no_pass(answers):
    a = answers["all_equal"]
    assert a["passes"] == 0 and a["order"] == list(range(a["n"]))


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_a_name_over_the_cap_is_reported(answers, case):
    name, _, _, problem = case
    a = answers[name]
    assert a["flags"] == 0 and a["problem"] == problem and a["order"] is None, name


def test_a_lower_code_in_a_lower_row_wins(exe, tmp_path):
    """lowest row, in it the lowest code: a long name behind a row the reader reports, in front of it, and in that row"""
    h, long_name = cases.header(2), "L" * (CAP + 1)
    files = [(cases.write_case(tmp_path, "behind", h + "a,1,2\nb,x,2\n" + long_name + ",1,2\n"), 2),
             (cases.write_case(tmp_path, "in_front", h + "a,1,2\n" + long_name + ",1,2\nb,x,2\n"), 2),
             (cases.write_case(tmp_path, "same_row", h + "a,1,2\n" + long_name + ",x,2\nb,1,2\n"), 2),
             (cases.write_case(tmp_path, "blank_row", h + "a,1,2\n\n" + long_name + ",1,2\n"), 2)]
    got = [a["problem"] for a in ask(exe, files)]
    assert got == [(1, 5), (1, 7), (1, 5), (1, 2)]


# ============================================================================= files beyond one step of a pass's scan
def test_scan_geometry_is_the_headers(exe):
    """MST_SORT_SCAN_BLOCK, MST_SORT_SCAN_ITEMS and mst_sort_scan_steps as mst_sort_cases.py restates them, at the edges of one, two
    and three steps"""
    sizes = [1, TILE, TILE + 1, 16 * TILE - 1, 16 * TILE, 16 * TILE + 1, 32 * TILE, 32 * TILE + 1, 48 * TILE, 48 * TILE + 1, (1 << 32) - 1]
    out = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    want = [f"geom {cases.SCAN_BLOCK} {cases.SCAN_ITEMS} {cases.BINS} {cases.tiles_of(n, TILE)} {cases.scan_steps(n, TILE)}" for n in sizes]
    assert out[:-1] == want and (cases.SCAN_BLOCK, cases.SCAN_ITEMS, cases.BINS) == (1024, 4, 256)
    assert [cases.scan_steps(n, TILE) for n in (1, 32768, 32769, 65536, 65537)] == [1, 1, 2, 2, 3]


@pytest.fixture(scope="module")
def large_answers(exe, tmp_path_factory):
    """the program's answer for every large case, by name: one run"""
    d = tmp_path_factory.mktemp("mst_sort_large")
    files = [(cases.write_case(d, name, cases.large(name, TILE)[0]), cases.large(name, TILE)[1]) for name in cases.LARGE]
    return {name: dict(a, path=path) for name, (path, _), a in zip(cases.LARGE, files, ask(exe, files))}


def test_the_large_list_reaches_one_two_and_three_steps(large_answers):
    """exactly one full step (32768 rows, 16 tiles), two steps by one row, three steps (65537 rows, 33 tiles); the program's tiles
    and steps are the restated ones.  And which steps' words a row reads: with names of the reader's subset only those of the
    first step up to 32 tiles, so the two files behind the list's first eight are the ones whose leaves depend on a carried sum."""
    geom = {name: a["geom"] for name, a in large_answers.items()}
    assert {g[:3] for g in geom.values()} == {(cases.SCAN_BLOCK, cases.SCAN_ITEMS, cases.BINS)}
    names = {name: cases.names_of(cases.large(name, TILE)[0]) for name in cases.LARGE}
    for name, a in large_answers.items():
        assert a["n"] == len(names[name]) == int(name.rsplit("_", 1)[1])
        assert geom[name][3:] == (cases.tiles_of(a["n"], TILE), cases.scan_steps(a["n"], TILE)), name
    assert geom["rows_32768"][3:] == (16, 1) and geom["rows_32769"][3:] == (17, 2) and geom["rows_65537"][3:] == (33, 3)
    assert all(geom[name][3:] == (17, 2) for name in cases.LARGE if name.endswith("_32769"))
    assert geom["high_bytes_65537"][3:] == (33, 3) and geom["rows_196609"][3:] == (97, 7)
    read = {name: cases.steps_read(names[name], TILE) for name in cases.LARGE}
    assert all(read[name] == {0} for name in cases.LARGE[:8])
    assert read["high_bytes_65537"] == {0, 1} and read["rows_196609"] == {0, 1, 2}
    # hex64_32769 is past one round of the CSV reader's scan as well (mst_csv_cases.SCAN_BLOCK tiles of 4096 bytes)
    hex64 = large_answers["hex64_32769"]
    assert os.path.getsize(hex64["path"]) - hex64["body"] > 1024 * 4096 and hex64["longest"] == hex64["passes"] == CAP
    pool = names["pool_300_32769"]
    assert len(set(pool)) == 300 and all(len(set(pool[t * TILE:(t + 1) * TILE])) >= 295 for t in range(16))
    skew, skew0 = names["skew_32769"], names["skew_tile0_32769"]
    assert set(skew[:16 * TILE]) == {b"samenamea"} and skew[16 * TILE:] == [b"samenameb"]
    assert set(skew0[TILE:]) == {b"samenamea"} and len(set(skew0[:TILE])) == len(cases.ALPHABET)
    chain = [i for i, nm in enumerate(names["prefix_tail_32769"]) if nm == b"a" * len(nm)]
    assert {len(names["prefix_tail_32769"][i]) for i in chain} == set(range(CAP + 1)) and {i // TILE for i in chain} == set(range(17))


def test_a_scan_that_drops_its_carried_sum_shows_in_the_last_two_files_only():
    """A model of the last pass (byte 0) with the kernel's stepped scan, once as it is and once with every step starting from 0:
    the places differ exactly in the files whose rows read a word behind the first step.  This is why the list does not end
    at 65537 rows of ALPHABET names: such a file takes three steps and none of its rows would notice a wrong carry."""
    import numpy as np
    step = cases.SCAN_ITEMS * cases.SCAN_BLOCK
    for name in cases.LARGE:
        names = cases.names_of(cases.large(name, TILE)[0])
        n, tiles = len(names), cases.tiles_of(len(names), TILE)
        src = sorted(range(n), key=lambda i: names[i][1:])            # the order the earlier passes leave
        digit = np.array([names[i][0] if names[i] else 0 for i in src])
        word = digit * tiles + np.arange(n) // TILE
        hist = np.bincount(word, minlength=cases.BINS * tiles)
        whole = np.cumsum(hist) - hist
        stepped = whole - np.repeat(whole[::step], step)[:whole.size]  # every step's prefix sums without what was before it
        reads_carried = bool((whole[word] != stepped[word]).any())
        assert reads_carried == (name in ("high_bytes_65537", "rows_196609")), name
        assert reads_carried == (cases.steps_read(names, TILE) != {0}), name


@pytest.mark.parametrize("name", cases.LARGE)
def test_large_files_come_out_in_pythons_stable_order(large_answers, name):
    comes_out_in_pythons_stable_order(large_answers[name], name, 2)


# ============================================================================= the entry points: exports, geometry, refusals
def test_exports_are_the_headers_prototypes():
    text = open(os.path.join(ROOT, "include", "summa_snapshot.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(ss_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert [name for name, _ in protos] == ffi.SNAPSHOT_EXPORTS
    L = ffi.snapshot_lib()
    for name, args in protos:
        getattr(L, name)
        assert len(ffi.SNAPSHOT_ARGTYPES[name]) == len(args.split(",")), name
    gpu_h = open(os.path.join(ROOT, "include", "summa_gpu.h")).read()
    assert not re.search(r"\bss_\w+\s*\(", gpu_h) and not set(ffi.SNAPSHOT_EXPORTS) & set(ffi.EXPORTS)


def test_geometry_is_the_headers():
    L = ffi.snapshot_lib()
    cap, tile = C.c_uint32(0), C.c_uint32(0)
    L.ss_mst_sort_geometry(C.byref(cap), C.byref(tile))
    assert (cap.value, tile.value) == (CAP, TILE)
    L.ss_mst_sort_geometry(None, None)


def test_scratch_size():
    L = ffi.snapshot_lib()
    size = C.c_uint64(77)
    for n in (0, 1 << 32):
        assert L.ss_mst_sort_scratch(n, C.byref(size)) == SG_ERR_INVALID and size.value == 77
    assert L.ss_mst_sort_scratch(5, None) == SG_ERR_INVALID
    for n in (1, TILE, TILE + 1, 3 * TILE + 5, 16 * TILE, 16 * TILE + 1, 32 * TILE + 1, 96 * TILE + 1):
        assert L.ss_mst_sort_scratch(n, C.byref(size)) == 0
        tiles = -(-n // TILE)
        assert size.value == 4 * (64 + 2 * (-(-n // 4) * 4) + 256 * tiles), n


def entries_sorted(**change):
    """a good call but for `change`; the device pointers are not memory: a refused call never uses them"""
    a = dict(d_bytes=0x10000, length=100, body_off=10, tiles=0x20000, delim=ord(","), nc=2, n=3, rows=4, spans=0x30000, sort=0x60000,
             order=0x70000, name_spans=0x80000, users=0x40000, bals=0x50000, out=True)
    a.update(change)
    problem = C.c_uint64(77)
    rc = ffi.snapshot_lib().ss_mst_csv_entries_sorted_dev(a["d_bytes"], a["length"], a["body_off"], a["tiles"], a["delim"], a["nc"], a["n"],
                                                          a["rows"], a["spans"], a["sort"], a["order"], a["name_spans"], a["users"], a["bals"],
                                                          C.byref(problem) if a["out"] else None, None)
    assert problem.value == 77
    return rc, ffi.lib().sg_last_error().decode()


def test_entries_sorted_refuses_bad_arguments():
    for change in ({"d_bytes": None}, {"tiles": None}, {"spans": None}, {"sort": None}, {"order": None}, {"name_spans": None}, {"users": None},
                   {"bals": None}, {"out": False}):
        rc, msg = entries_sorted(**change)
        assert rc == SG_ERR_INVALID and "null" in msg, change
    for change in ({"nc": 0}, {"nc": 65}, {"body_off": 101}, {"body_off": 100}, {"length": (1 << 32) + 10}, {"n": 0}, {"n": 91}, {"rows": 2},
                   {"rows": 1 << 32}, {"tiles": 0x20002}, {"spans": 0x30004}, {"delim": 10}, {"delim": 13}, {"delim": ord("5")},
                   {"delim": ord('"')}, {"delim": 0}, {"delim": 0xC3}, {"delim": 256 + ord(",")},
                   {"sort": 0x60008}, {"order": 0x70002}, {"name_spans": 0x80002}):
        rc, msg = entries_sorted(**change)
        assert rc == SG_ERR_INVALID and "bad size" in msg, change


def find(**change):
    import numpy as np
    a = dict(d_bytes=0x10000, length=100, body_off=10, name_spans=0x80000, n=3, names=np.frombuffer(b"abcde", dtype=np.uint8).copy(),
             off=np.array([0, 2, 5], dtype=np.uint64), m=2, out=True)
    a.update(change)
    found = np.full(4, 77, dtype=np.uint32)
    rc = ffi.snapshot_lib().ss_mst_find_names(a["d_bytes"], a["length"], a["body_off"], a["name_spans"], a["n"],
                                              None if a["names"] is None else ffi.ptr(a["names"]), None if a["off"] is None else ffi.ptr(a["off"]),
                                              a["m"], ffi.ptr(found) if a["out"] else None, None)
    assert (found == 77).all()
    return rc, ffi.lib().sg_last_error().decode()


def test_find_refuses_bad_arguments():
    import numpy as np
    for change in ({"d_bytes": None}, {"name_spans": None}, {"names": None}, {"off": None}, {"out": False}):
        rc, msg = find(**change)
        assert rc == SG_ERR_INVALID and "null" in msg, change
    for change in ({"m": 0}, {"n": 0}, {"n": 1 << 32}, {"body_off": 101}, {"length": (1 << 32) + 10}, {"name_spans": 0x80002}):
        rc, msg = find(**change)
        assert rc == SG_ERR_INVALID and "bad size" in msg, change
    rc, msg = find(off=np.array([1, 2, 5], dtype=np.uint64))
    assert rc == SG_ERR_INVALID and "start at 0" in msg
    rc, msg = find(off=np.array([0, 3, 2], dtype=np.uint64))
    assert rc == SG_ERR_INVALID and "decrease" in msg
