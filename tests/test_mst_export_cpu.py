"""A tree written back out as its snapshot CSV without a GPU: the rules of csrc/mst_export.h, whose text the kernels compile, run
by the header's own serial steps in tests/cpp/mst_export_check.cpp (behind the CSV reader's and the sort's; built by the host
compiler under address / undefined sanitizers, a process of its own) and compared with the model of mst_export_cases.py on every
case, for a tree in file order and a sorted one.  And the digits of every edge value folded back, the geometry and the scratch size,
the exports of include/summa_export.h, what the two entry points refuse before they touch a device, and `to_csv` of a tree whose
entries are on the host.

tests/golden/entry_16.csv has "\\r\\n" line ends, which by the text's definition come out as "\\n": the file comes back byte for byte
but for that, and its copy with "\\n" line ends byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import mst_export_cases as cases
from circuits_halo2_amd import ffi
from circuits_halo2_amd import merkle_sum_tree as M

SG_ERR_INVALID = -1
CASES = cases.cases()
IDS = [c[0] for c in CASES]
GOLDEN = os.path.join(ROOT, "tests", "golden", "entry_16.csv")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_export") / "mst_export_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_export_check.cpp"), "-o", out])
    return out


def ask(exe, lines):
    """command lines -> the program's output lines, split into words"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def answers(exe, tmp_path_factory):
    """{(case name, sorted?): (n_rows, total, body bytes, offsets)} of the program: one run"""
    d = tmp_path_factory.mktemp("mst_export_files")
    lines, keys = [], []
    for name, text, nc, delim, _ in CASES:
        path = cases.write_case(d, name, text)
        for sorted_tree in (False, True):
            keys.append((name, sorted_tree))
            stem = os.path.join(str(d), f"{name}.{int(sorted_tree)}")
            lines.append(f"export {path} {nc} {int(sorted_tree)} {ord(delim)} {stem}.body {stem}.off")
    out = {}
    for key, words, line in zip(keys, ask(exe, lines), lines):
        assert words[0] == "export", (key, words)
        stem = line.split()[-2][:-5]
        out[key] = (int(words[1]), int(words[2]), open(stem + ".body", "rb").read(), np.fromfile(stem + ".off", dtype=np.uint32).tolist())
    assert len(out) == 2 * len(CASES)
    return out


def test_the_geometry_is_the_case_modules_and_the_list_holds_what_it_must(exe):
    assert ask(exe, ["geometry"]) == [["geometry", str(cases.THREADS), str(cases.TILE), str(cases.GROUP), str(cases.NAME_CAP), str(cases.MAX_ROW),
                                      "8192"]]
    assert (cases.TILE, cases.GROUP, cases.GROUP_ROWS, cases.LANES, cases.TRIP_ROWS) == (64, 256, 16384, 64, 1 << 20)
    assert cases.SIZES == (63, 64, 65, 16383, 16384, 16385) and cases.BIG == (1 << 20) + 65 and cases.MAX_ROW == 64 + 64 * 78 + 1 == 5057
    # a tile's or a group's rows add up in 32 bits; the groups' totals of a snapshot need not
    assert cases.GROUP_ROWS * cases.MAX_ROW < 1 << 32 < ((1 << 32) - 1) * cases.MAX_ROW
    # BIG: the first wave adds 65 group totals up, a second trip of its loop, and the last tile holds one row
    groups = -(-cases.BIG // cases.GROUP_ROWS)
    assert groups == cases.LANES + 1 and cases.BIG % cases.TILE == 1
    names = set(IDS)
    assert {"one_row_zero", "empty_name", "name_64_bytes", "one_currency", "two_currencies", "sixty_four_currencies_longest_rows", "powers_of_ten",
            "word_edges_and_zero_chunks", "leading_zeros", "values_at_or_above_r", "crlf", "no_final_newline", "semicolon", "duplicate_names"} <= names
    assert {f"varied_{n}" for n in cases.SIZES} <= names
    by_name = {c[0]: c for c in CASES}
    values = {v for name in ("powers_of_ten", "word_edges_and_zero_chunks") for _, bal in by_name[name][4] for v in bal}
    assert values >= {10 ** k - 1 for k in range(1, 77)} | {10 ** k for k in range(1, 77)}
    assert values >= {2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 64, cases.R - 1, 10 ** 9, 10 ** 18 + 1, 7 * 10 ** 27, 0}
    for n in cases.SIZES:                                     # rows start at every offset mod 16
        assert {off % 16 for off in cases.offsets_of(by_name[f"varied_{n}"][4])[0]} == set(range(16))
    assert [cases.canonical(by_name[name]) for name in ("two_currencies", "semicolon", "leading_zeros", "crlf", "no_final_newline",
                                                        "values_at_or_above_r")] == [True, True, False, False, False, False]


def test_scratch_size_at_a_second_group_and_past_64(exe):
    X = ffi.export_lib()
    size = C.c_uint64(77)
    for n in (0, 1 << 32):
        assert X.sx_mst_csv_scratch(n, C.byref(size)) == SG_ERR_INVALID and size.value == 77
        assert ffi.lib().sg_last_error().decode().startswith("sx_mst_csv_scratch: ")
    assert X.sx_mst_csv_scratch(5, None) == SG_ERR_INVALID
    shapes = [1, 63, 64, 65, 16384, 16385, 1 << 20, cases.BIG, (1 << 32) - 1]
    for n, words in zip(shapes, ask(exe, [f"scratch {n}" for n in shapes])):
        assert X.sx_mst_csv_scratch(n, C.byref(size)) == 0
        tiles = -(-n // 64)
        groups = -(-tiles // 256)
        assert [size.value, tiles, groups] == [4 * (4 + tiles + groups)] + [int(x) for x in words[2:]] and int(words[1]) == size.value
    assert ask(exe, [f"scratch {cases.BIG}"]) == [["scratch", str(4 * (4 + 16386 + 65)), "16386", "65"]]


def test_the_digits_of_every_edge_value_fold_back(exe):
    values = cases.EDGE_VALUES + [cases.R, cases.R + 5, 2 ** 256 - 1, 10 ** 80 + 3]
    texts = [str(v) for v in values] + ["007", "000"]
    for text, words in zip(texts, ask(exe, ["digits " + t for t in texts])):
        want = str(int(text) % cases.R)
        assert words == ["digits", want, str(len(want)), "1"], text
    assert len(str(cases.R - 1)) == cases.MAX_DIGITS


@pytest.mark.parametrize("sorted_tree", (False, True), ids=("file", "sorted"))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_mirror_agrees_with_the_model(answers, case, sorted_tree):
    name, text, nc, delim, rows = case
    want_rows = cases.sorted_rows(rows) if sorted_tree else rows
    offsets, total = cases.offsets_of(want_rows)
    n, got_total, body, got_offsets = answers[(name, sorted_tree)]
    assert (n, got_total) == (len(rows), total)
    assert got_offsets == offsets
    assert body == cases.body_of(want_rows, delim)
    if not sorted_tree and cases.canonical(case):
        assert cases.header(nc, delim).encode() + body == text


def test_the_mirror_past_64_groups(exe, tmp_path):
    """in file order alone: the sorted tree differs by whose spans are read, which every smaller case covers, and a sanitized
    field product is slow"""
    keys, bal = cases.big_case()
    path = cases.write_big(tmp_path / "big.csv", keys, bal)
    width = cases.BIG_WIDTH + 2 * 2 + 1
    words = ask(exe, [f"export {path} 2 0 {ord(',')} {tmp_path}/big.body {tmp_path}/big.off"])
    assert words == [["export", str(cases.BIG), str(cases.BIG * width)]]
    assert np.array_equal(np.fromfile(f"{tmp_path}/big.body", dtype=np.uint8), cases.big_body(keys, bal, False))
    assert np.array_equal(np.fromfile(f"{tmp_path}/big.off", dtype=np.uint32), np.arange(cases.BIG, dtype=np.int64) * width)
    assert open(path, "rb").read() == cases.header(2).encode() + open(f"{tmp_path}/big.body", "rb").read()


def test_spans_the_reader_did_not_make_are_cut_to_the_text_and_to_64_bytes(exe):
    want = "c," + "z" * 62 + ",0|" + ",0|" + "z" * 64 + ",0|"
    assert ask(exe, ["clipped"]) == [["clipped", str(len(want)), want]]


# ============================================================================= the entry points: exports and refusals
def test_exports_are_the_headers_prototypes_and_stay_out_of_the_other_headers():
    text = open(os.path.join(ROOT, "include", "summa_export.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(sx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = [name for name, _ in protos]
    assert names == ffi.EXPORT_EXPORTS == list(ffi.EXPORT_ARGTYPES) == ["sx_mst_csv_scratch", "sx_mst_csv_measure_dev", "sx_mst_csv_write_dev"]
    X = ffi.export_lib()
    for name, args in protos:
        getattr(X, name)
        assert len(ffi.EXPORT_ARGTYPES[name]) == len(args.split(",")), name
    for other in ("summa_gpu.h", "summa_snapshot.h", "summa_rounds.h", "summa_prover.h", "summa_verifier.h"):
        assert not re.search(r"\bsx_", open(os.path.join(ROOT, "include", other)).read()), other
    assert not any(name.startswith("sx_") for name in ffi.EXPORTS + ffi.SNAPSHOT_EXPORTS + ffi.ROUNDS_EXPORTS + ffi.PROVER_EXPORTS + ffi.VERIFIER_EXPORTS)


MEASURE_KEYS = ("t_bytes", "t_length", "t_body_off", "spans", "n", "nc", "leaf_bal", "row_off", "scratch", "total")
WRITE_KEYS = ("t_bytes", "t_length", "t_body_off", "spans", "n", "nc", "leaf_bal", "delim", "row_off", "body_bytes", "out")
GOOD = dict(t_bytes=0x40000, t_length=90, t_body_off=9, spans=0x80000, n=3, nc=2, leaf_bal=0x100000, row_off=0x110000, scratch=0x500000,
            total=True, delim=ord(","), body_bytes=40, out=0x600001)
BOTH_REFUSED = [({k: None}, "null") for k in ("t_bytes", "spans", "leaf_bal", "row_off")]
BOTH_REFUSED += [({"nc": 0}, "n_currencies"), ({"nc": 65}, "n_currencies"), ({"n": 0}, "n_rows"), ({"n": 1 << 32}, "n_rows"),
                 ({"t_body_off": 91}, "tree's body_off"), ({"t_length": (1 << 32) + 9}, "tree's body_off"), ({"spans": 0x80002}, "d_leaf_name_spans"),
                 ({"leaf_bal": 0x100008}, "d_leaf_balances"), ({"row_off": 0x110002}, "d_row_off")]
MEASURE_REFUSED = BOTH_REFUSED + [({"scratch": None}, "null"), ({"total": False}, "null"), ({"scratch": 0x500002}, "d_scratch")]
WRITE_REFUSED = BOTH_REFUSED + [({"out": None}, "null"), ({"body_bytes": 0}, "body_bytes"), ({"body_bytes": 1 << 32}, "body_bytes")]
WRITE_REFUSED += [({"delim": d}, "delimiter") for d in (10, 13, ord("5"), ord('"'), 0, 0xC3, 256 + ord(","))]


def measure_call(**change):
    """a good call but for `change`; the device pointers are not memory: a refused call never uses them"""
    a = dict(GOOD, **change)
    total = C.c_uint64(77)
    args = [a[k] for k in MEASURE_KEYS[:-1]] + [C.byref(total) if a["total"] else None, None]
    rc = ffi.export_lib().sx_mst_csv_measure_dev(*args)
    assert total.value == 77
    return rc, ffi.lib().sg_last_error().decode()


def write_call(**change):
    a = dict(GOOD, **change)
    rc = ffi.export_lib().sx_mst_csv_write_dev(*[a[k] for k in WRITE_KEYS], None)
    return rc, ffi.lib().sg_last_error().decode()


def test_the_entry_points_refuse_bad_arguments(exe):
    for change, word in MEASURE_REFUSED:
        rc, msg = measure_call(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("sx_mst_csv_measure: ") and word in msg, (change, msg)
    for change, word in WRITE_REFUSED:
        rc, msg = write_call(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("sx_mst_csv_write: ") and word in msg, (change, msg)
    # the same words from the header's own functions, and "" for what the entry points accept: a text that is all header, the
    # last row count, any alignment of d_out, a body one byte short of 4 GiB
    def problem(which, keys, **change):
        a = dict(dict(GOOD, total=0x700000), **{k: (0 if v is False else v) for k, v in change.items()})
        return " ".join(ask(exe, [which + " " + " ".join(str(a[k] or 0) for k in keys)])[0][1:])
    for which, keys, refused in (("measure_problem", MEASURE_KEYS, MEASURE_REFUSED), ("write_problem", WRITE_KEYS, WRITE_REFUSED)):
        assert problem(which, keys) == "" and problem(which, keys, t_body_off=90) == "" and problem(which, keys, n=(1 << 32) - 1) == ""
        assert problem(which, keys, nc=64) == "" and problem(which, keys, nc=1) == ""
        for change, word in refused:
            assert word in problem(which, keys, **change), (which, change)
    assert problem("write_problem", WRITE_KEYS, out=0x600000, body_bytes=(1 << 32) - 1, delim=ord(";")) == ""


# ============================================================================= to_csv from entries on the host
class _HostTree(M._Tree):
    """entries alone: what the base implementation reads"""

    def __init__(self, entries, nc, cryptocurrencies=(), is_sorted=False):
        self.entries, self.is_sorted, self.n_currencies, self.depth = entries, is_sorted, nc, max(0, (len(entries) - 1).bit_length())
        self.cryptocurrencies = list(cryptocurrencies)


def host_tree(path, nc, sorted_tree=False):
    entries, crypto = M.parse_csv_to_entries(path, nc)
    if sorted_tree:
        entries.sort(key=lambda e: e[0].encode())
    entries += [(None, [0] * nc)] * ((1 << max(0, (len(entries) - 1).bit_length())) - len(entries))
    return _HostTree(entries, nc, crypto, sorted_tree)


def test_merkle_sum_tree_has_the_host_definition():
    assert M.MerkleSumTree.to_csv is M._Tree.to_csv and M.DeviceMerkleSumTree.to_csv is not M._Tree.to_csv


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_to_csv_of_entries_is_the_model_and_reads_back(case, tmp_path):
    name, text, nc, delim, rows = case
    src, out = cases.write_case(tmp_path, "src", text), str(tmp_path / "out.csv")
    for sorted_tree in (False, True):
        tree = host_tree(src, nc, sorted_tree)
        done = tree.to_csv(out, delimiter=delim)
        want = cases.header(nc, delim).encode() + cases.body_of(cases.sorted_rows(rows) if sorted_tree else rows, delim)
        assert open(out, "rb").read() == want
        assert (done.n_rows, done.size, done.ingest, done.fallback_reason) == (len(rows), len(want), "host", None)
        back = host_tree(out, nc, sorted_tree)
        value = lambda entries: [(nm, [v % cases.R for v in bal]) for nm, bal in entries]
        assert value(back.entries) == value(tree.entries) and back.cryptocurrencies == tree.cryptocurrencies
    if cases.canonical(case):
        host_tree(src, nc).to_csv(out, delimiter=delim)
        assert open(out, "rb").read() == text


def test_to_csv_gives_the_golden_file_back(tmp_path):
    golden = open(GOLDEN, "rb").read()
    assert b"\r\n" in golden and golden.endswith(b"\r\n")     # by the text's definition "\r\n" comes out as "\n"
    out = str(tmp_path / "out.csv")
    done = host_tree(GOLDEN, 2).to_csv(out)
    assert open(out, "rb").read() == golden.replace(b"\r\n", b"\n") and (done.n_rows, done.size) == (16, len(golden) - 17)
    lf = cases.write_case(tmp_path, "entry_16_lf", golden.replace(b"\r\n", b"\n"))
    host_tree(lf, 2).to_csv(out)
    assert open(out, "rb").read() == open(lf, "rb").read()    # byte for byte


def test_to_csv_refuses_what_would_not_read_back(tmp_path):
    out = str(tmp_path / "out.csv")
    crypto = [("C0", "ETH"), ("C1", "ETH")]
    tree = _HostTree([("a", [1, 2]), (None, [0, 0])], 2)
    with pytest.raises(ValueError, match="no cryptocurrency names"):
        tree.to_csv(out)
    assert tree.to_csv(out, cryptocurrencies=crypto).n_rows == 1 and open(out, "rb").read() == cases.header(2).encode() + b"a,1,2\n"
    with pytest.raises(ValueError, match="pairs expected"):
        tree.to_csv(out, cryptocurrencies=crypto[:1])
    with pytest.raises(ValueError, match="holds no entries"):
        _HostTree.to_csv(type("T", (M._Tree,), {"entries": None, "n_currencies": 2, "cryptocurrencies": crypto})(), out)
    for bad in ("a,b", 'a"b', "a\rb", "a\nb", "a\0b", "ü"):
        with pytest.raises(ValueError, match="would not read back"):
            _HostTree([(bad, [1, 2])], 2, crypto).to_csv(out)
    assert _HostTree([("a,b", [1, 2])], 2, crypto).to_csv(out, delimiter=";").n_rows == 1
    with pytest.raises(ValueError, match="would not read back"):
        _HostTree([("a;b", [1, 2])], 2, crypto).to_csv(out, delimiter=";")
    for bad in ("5", '"', "\n", "\r", "\0", "ü", ",,", "", 7):
        with pytest.raises(ValueError, match="delimiter"):
            _HostTree([("a", [1, 2])], 2, crypto).to_csv(out, delimiter=bad)
