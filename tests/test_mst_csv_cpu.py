"""The device CSV reader without a GPU: the byte classes, the row splitter and the tile edges of csrc/mst_csv.h, whose text the
kernels compile, run by the header's own serial passes in tests/cpp/mst_csv_check.cpp, built by the host compiler under
address / undefined sanitizers.  Two fixed lists of files (mst_csv_cases.py): every accepted one comes out with the fields
Python's csv finds, byte for byte, and the balances `parse_csv_to_entries` returns; every refused one with the flag, or the
lowest offending row and its code.  The lists LARGE_ACCEPTED and LARGE_REFUSED the same, with the proof that they reach one,
two and three rounds of the one-workgroup scan, whose width is restated in mst_csv_cases.py and compared with the header's
here.  And what the two entry points refuse before they touch a device."""
import csv
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

import mst_csv_cases as cases
from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import parse_csv_to_entries

SG_ERR_INVALID = -1
TILE, CAP = 4096, 131072                                  # what the header must say (asserted from the program's output)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_csv") / "mst_csv_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_csv_check.cpp"), "-o", out])
    return out


def ask(exe, files):
    """[(path, nc)] -> per file {"body", "delim", "geom", "n", "flags", "problem": (row, code), "spans": [[begin, end, ..] per row]}"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    text = "".join(f"{path} {nc}\n" for path, nc in files)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out, cur = [], None
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "body":
            cur = {"body": int(w[1]), "delim": chr(int(w[2])), "spans": []}
            assert (int(w[3]), int(w[4])) == (TILE, CAP)
        elif w[0] == "geom":
            cur["geom"] = tuple(int(x) for x in w[1:])                  # (SCAN_BLOCK, tiles, rounds)
        elif w[0] == "scan":
            cur.update(n=int(w[1]), flags=int(w[2], 16), problem=(int(w[3]), int(w[4])))
        elif w[0] == "span":
            assert int(w[1]) == len(cur["spans"])
            cur["spans"].append([int(x) for x in w[2:]])
        elif w[0] == "end":
            out.append(cur)
    assert len(out) == len(files)
    return out


ACCEPTED = cases.accepted(TILE, CAP)
REFUSED = cases.refused(TILE, CAP)


@pytest.fixture(scope="module")
def answers(exe, tmp_path_factory):
    """the program's answer for every case of both lists, by name: one run"""
    d = tmp_path_factory.mktemp("mst_csv_files")
    names = [c[0] for c in ACCEPTED + REFUSED]
    assert len(set(names)) == len(names)
    files = [(cases.write_case(d, c[0], c[1]), c[2]) for c in ACCEPTED + REFUSED]
    return {name: dict(a, path=path) for name, (path, _), a in zip(names, files, ask(exe, files))}


def test_the_lists_hold_what_they_must():
    names = {c[0] for c in ACCEPTED}
    assert len(cases.GOLDENS) == 7 and {g[:-4] for g in cases.GOLDENS} <= names
    assert {f"newline_at_{TILE - 1}", f"newline_at_{TILE}", f"newline_at_{TILE + 1}"} <= names
    assert {c[2] for c in ACCEPTED} == {1, 2, 4}


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted_files_come_out_as_csv_reads_them(answers, case):
    name, _, nc = case
    comes_out_as_csv_reads_it(answers[name], name, nc)


def comes_out_as_csv_reads_it(a, name, nc):
    with open(a["path"], "rb") as f:
        data = f.read()
    body = data[a["body"]:]
    with open(a["path"], newline="") as f:
        rows = [r for r in list(csv.reader(f, delimiter=a["delim"]))[1:] if r]
    entries, _ = parse_csv_to_entries(a["path"], nc)
    assert a["flags"] == 0 and a["problem"] == (0, 0), name
    assert a["n"] == len(rows) == len(entries) == len(a["spans"])
    for i, (span, row, (user, balances)) in enumerate(zip(a["spans"], rows, entries)):
        got = [body[span[2 * k]:span[2 * k + 1]] for k in range(1 + nc)]
        assert got == [x.encode() for x in row], f"{name}: row {i}"
        assert got[0] == user.encode() and [int(x) for x in got[1:]] == balances, f"{name}: row {i}"
        assert all(x.isdigit() for x in got[1:])


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_files_are_reported(answers, case):
    name, _, _, flag, problem = case
    a = answers[name]
    if flag is not None:
        assert a["flags"] == flag and a["spans"] == [], name
    else:
        assert a["flags"] == 0 and a["problem"] == problem and a["spans"] == [], name


def test_a_body_without_rows(exe, tmp_path):
    files = []
    for name, tail in (("none", ""), ("lf", "\n"), ("crlf", "\r\n")):
        files.append((cases.write_case(tmp_path, name, cases.header(2) + tail), 2))
    for a in ask(exe, files):
        assert a["n"] == 0 and a["flags"] == 0 and a["problem"] == (0, 0)


# ============================================================================= bodies beyond one round of the scan
def test_scan_geometry_is_the_headers(exe):
    """MST_CSV_SCAN_BLOCK and mst_csv_scan_rounds as mst_csv_cases.py restates them, at the edges of one, two and three rounds"""
    edge = cases.SCAN_BLOCK * TILE
    lengths = [0, 1, TILE, TILE + 1, edge - 1, edge, edge + 1, 2 * edge, 2 * edge + 1, 3 * edge, 3 * edge + 1, (1 << 32) - 1]
    out = subprocess.run([exe] + [str(n) for n in lengths], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    want = [f"geom {cases.SCAN_BLOCK} {cases.tiles_of(n, TILE)} {cases.scan_rounds(n, TILE)}" for n in lengths]
    assert out[:-1] == want and cases.SCAN_BLOCK == 1024
    assert [cases.scan_rounds(n, TILE) for n in (0, 1, edge, edge + 1, 2 * edge + 1)] == [0, 1, 1, 2, 3]


@pytest.fixture(scope="module")
def large_answers(exe, tmp_path_factory):
    """the program's answer for every large case, by name: one run"""
    d = tmp_path_factory.mktemp("mst_csv_large")
    names = cases.LARGE_ACCEPTED + cases.LARGE_REFUSED
    files = [(cases.write_case(d, name, cases.large(name, TILE)[0]), cases.large(name, TILE)[1]) for name in names]
    return {name: dict(a, path=path) for name, (path, _), a in zip(names, files, ask(exe, files))}


def test_the_large_lists_reach_one_two_and_three_rounds(large_answers):
    """exactly one full round (1024 tiles, the body's last byte a newline), two rounds by one byte, three rounds; the
    program's tiles and rounds are the restated ones; every refused file is a two-round body"""
    geom = {name: a["geom"] for name, a in large_answers.items()}
    assert {g[0] for g in geom.values()} == {cases.SCAN_BLOCK}
    for name, (_, tiles, rounds) in geom.items():
        body_len = os.path.getsize(large_answers[name]["path"]) - large_answers[name]["body"]
        assert (tiles, rounds) == (cases.tiles_of(body_len, TILE), cases.scan_rounds(body_len, TILE)), name
    assert geom["tiles_1024"][1:] == (1024, 1) and geom["tiles_1025"][1:] == (1025, 2) and geom["tiles_1025_open_end"][1:] == (1025, 2)
    assert geom["tiles_2049"][1] >= 2049 and geom["tiles_2049"][2] == 3
    assert all(geom[name][1:] == (1025, 2) for name in cases.LARGE_REFUSED)
    edge = cases.SCAN_BLOCK * TILE
    for name in cases.LARGE_ACCEPTED:
        with open(large_answers[name]["path"], "rb") as f:
            body = f.read()[large_answers[name]["body"]:]
        assert (body[-1:] == b"\n") == (not name.endswith("open_end")), name
        rounds = [body[r * edge:(r + 1) * edge].count(b"\n") for r in range(geom[name][2])]
        if name == "tiles_2049":
            assert min(rounds) > 1000                             # every round holds many newlines, the prefixes behind the first depend on it
        else:
            assert rounds[0] > 1000 and rounds[1:] in ([], [1], [0])
        long_rows = [r for r in body.split(b"\n") if len(r) > TILE]
        starts = [body.index(r) for r in long_rows]
        if len(body) > edge:                                      # a row longer than a tile with bytes in tile 1023 and in tile 1024
            assert any(s < edge <= s + len(r) for s, r in zip(starts, long_rows)), name
        assert any(len(r) < 20 for r in body.split(b"\n")[:-1]) and long_rows


@pytest.mark.parametrize("name", cases.LARGE_ACCEPTED)
def test_large_accepted_files_come_out_as_csv_reads_them(large_answers, name):
    comes_out_as_csv_reads_it(large_answers[name], name, 2)


@pytest.mark.parametrize("name", cases.LARGE_REFUSED)
def test_large_refused_files_are_reported(large_answers, name):
    _, _, flag, problem = cases.large(name, TILE)
    a = large_answers[name]
    if flag is not None:
        assert a["flags"] == flag and a["spans"] == [], name
    else:
        assert a["flags"] == 0 and a["problem"] == problem and a["spans"] == [], name


# ============================================================================= the entry points: refusals, no device needed
def geometry():
    tile, cap = C.c_uint32(0), C.c_uint32(0)
    ffi.lib().sg_mst_csv_geometry(C.byref(tile), C.byref(cap))
    return tile.value, cap.value


def test_geometry_is_the_headers():
    assert geometry() == (TILE, CAP)
    ffi.lib().sg_mst_csv_geometry(None, None)


def scan(d_bytes=0x10000, length=100, body_off=10, tiles=0x20000, outs=True):
    n, flags = C.c_uint64(77), C.c_uint32(77)
    rc = ffi.lib().sg_mst_csv_scan_dev(d_bytes, length, body_off, tiles, C.byref(n) if outs else None, C.byref(flags), None)
    assert (n.value, flags.value) == (77, 77)
    return rc, ffi.lib().sg_last_error().decode()


def entries(**change):
    """a good call but for `change`; the device pointers are not memory: a refused call never uses them"""
    a = dict(d_bytes=0x10000, length=100, body_off=10, tiles=0x20000, delim=ord(","), nc=2, n=3, rows=4, spans=0x30000, users=0x40000,
             bals=0x50000, out=True)
    a.update(change)
    problem = C.c_uint64(77)
    rc = ffi.lib().sg_mst_csv_entries_dev(a["d_bytes"], a["length"], a["body_off"], a["tiles"], a["delim"], a["nc"], a["n"], a["rows"],
                                          a["spans"], a["users"], a["bals"], C.byref(problem) if a["out"] else None, None)
    assert problem.value == 77
    return rc, ffi.lib().sg_last_error().decode()


def test_scan_refuses_bad_arguments():
    for change in ({"d_bytes": None}, {"tiles": None}, {"outs": False}):
        rc, msg = scan(**change)
        assert rc == SG_ERR_INVALID and "null" in msg, change
    for change in ({"body_off": 101}, {"length": (1 << 32) + 10}, {"tiles": 0x20002}):
        rc, msg = scan(**change)
        assert rc == SG_ERR_INVALID and "bad size" in msg, change


def test_entries_refuses_bad_arguments():
    for change in ({"d_bytes": None}, {"tiles": None}, {"spans": None}, {"users": None}, {"bals": None}, {"out": False}):
        rc, msg = entries(**change)
        assert rc == SG_ERR_INVALID and "null" in msg, change
    for change in ({"nc": 0}, {"nc": 65}, {"body_off": 101}, {"body_off": 100}, {"length": (1 << 32) + 10}, {"n": 0}, {"n": 91}, {"rows": 2},
                   {"rows": 1 << 32}, {"tiles": 0x20002}, {"spans": 0x30004}, {"delim": 10}, {"delim": 13}, {"delim": ord("5")},
                   {"delim": ord('"')}, {"delim": 0}, {"delim": 0xC3}, {"delim": 256 + ord(",")}):
        rc, msg = entries(**change)
        assert rc == SG_ERR_INVALID and "bad size" in msg, change
