"""The diff of the next round's snapshot against a tree without a GPU: the rules of csrc/mst_diff.h, whose text the kernels compile,
run by the header's own serial steps in tests/cpp/mst_diff_check.cpp (behind the CSV reader's and the sort's; built by the host
compiler under address / undefined sanitizers, a process of its own) and compared with the model of mst_diff_cases.py on every
case.  And the geometry and the scratch size, the exports of include/summa_rounds.h, what the two entry points refuse before they
touch a device, `diff_entries` of trees whose entries are on the host, and the stale diff."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import mst_diff_cases as cases
from circuits_halo2_amd import ffi
from circuits_halo2_amd import merkle_sum_tree as M

SG_ERR_INVALID = -1
CASES = cases.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_diff") / "mst_diff_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_diff_check.cpp"), "-o", out])
    return out


def ask(exe, lines):
    """command lines -> the program's output lines, split into words"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def models():
    return {c[0]: cases.model(c[1], c[2], c[3], c[4]) for c in CASES}


@pytest.fixture(scope="module")
def answers(exe, models, tmp_path_factory):
    """the program's answer for every case, by name: one run"""
    d = tmp_path_factory.mktemp("mst_diff_files")
    lines = []
    for name, a, b, nc, sorted_tree in CASES:
        pa, pb = cases.write_case(d, name + ".a", cases.text_of(a, nc)), cases.write_case(d, name + ".b", cases.text_of(b, nc))
        lines.append(f"diff {pa} {pb} {nc} {int(sorted_tree)} " + " ".join(map(str, cases.caps_of(models[name]))))
    out, cur = [], None
    for w in ask(exe, lines):
        ints = lambda: [int(x) for x in w[1:]]
        if w[0] == "tree":
            cur = {"tree": ints(), "reports": {}}
        elif w[0] == "refused":
            cur = {"refused": w[1]}
        elif w[0] in ("file", "rowleaf", "rowstate", "leafstate", "owner", "changed", "packed"):
            cur[w[0]] = ints()
        elif w[0] == "report":
            report = {"summary": ints()[1:9], "stable": ints()[9]}
            cur["reports"][int(w[1])] = report
        elif w[0] in ("new", "gone"):
            report[w[0]] = ints()
        elif w[0] == "end":
            out.append(cur)
    assert len(out) == len(CASES)
    return dict(zip(IDS, out))


def test_the_geometry_is_the_case_modules_and_the_list_holds_what_it_must(exe):
    assert ask(exe, ["geometry"]) == [["geometry", str(cases.THREADS), str(cases.TILE), str(cases.GROUP)]]
    assert (cases.TILE, cases.GROUP, cases.GROUP_ROWS, cases.SIZES) == (64, 256, 16384, (1, 2, 64, 65, 257, 16386))
    assert cases.edge_leaves(16386) == [0, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385]
    names = set(IDS)
    for n in cases.SIZES:
        for kind in ("file", "sorted"):
            assert {f"{f}_{n}_{kind}" for f in ("equal", "every_row_changed", "every_row_changed_shuffled", "edges_changed",
                                                "edges_changed_shuffled", "new_names")} <= names
    assert {"edges_gone_16386_sorted", "twice_in_b_257_file", "twice_in_b_16386_sorted", "twice_in_a_65_file", "field_equal_sorted",
            "one_currency_65_file", "three_currencies_65_sorted", "empty_name_in_tree_file"} <= names


def test_scratch_size_at_a_second_and_a_third_group(exe):
    L = ffi.rounds_lib()
    size = C.c_uint64(77)
    for n, depth in ((0, 3), (1 << 32, 3), (5, 31)):
        assert L.sr_mst_diff_scratch(n, depth, C.byref(size)) == SG_ERR_INVALID and size.value == 77
        assert ffi.lib().sg_last_error().decode().startswith("sr_mst_diff_scratch: ")
    assert L.sr_mst_diff_scratch(5, 3, None) == SG_ERR_INVALID
    shapes = [(1, 0), (63, 6), (64, 6), (65, 7), (16384, 14), (16385, 15), (16386, 15), (32769, 16), (40000, 14), (1 << 20, 20), ((1 << 32) - 1, 30)]
    for (n, depth), words in zip(shapes, ask(exe, [f"scratch {n} {depth}" for n, depth in shapes])):
        assert L.sr_mst_diff_scratch(n, depth, C.byref(size)) == 0
        lt, rt = -(-(1 << depth) // 64), -(-n // 64)
        lg, rg = -(-lt // 256), -(-rt // 256)
        assert [size.value, lt, lg, rt, rg] == [4 * (8 + 2 * (lt + lg) + rt + rg)] + [int(x) for x in words[2:]] and int(words[1]) == size.value
    assert ask(exe, ["scratch 16386 15", "scratch 32769 16"]) == [["scratch", str(4 * (8 + 2 * (512 + 2) + 257 + 2)), "512", "2", "257", "2"],
                                                                 ["scratch", str(4 * (8 + 2 * (1024 + 4) + 513 + 3)), "1024", "4", "513", "3"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_mirror_agrees_with_the_model(answers, models, case):
    name, a, b, nc, sorted_tree = case
    got, want = answers[name], models[name]
    assert "refused" not in got, got
    assert got["tree"] == [want["n_tree"], want["depth"]] and got["file"] == [len(b)]
    assert got["rowleaf"] == want["row_leaf"] and got["rowstate"] == want["row_state"]
    assert got["leafstate"] == want["leaf_state"] and got["owner"] == want["owner"] and got["changed"] == want["changed"]
    words = np.array(got["packed"], dtype=np.uint32).tobytes()
    assert words == b"".join(M._to_fr_bytes(v) for row in want["balances"] for v in row)
    assert sorted(got["reports"]) == cases.caps_of(want)
    for cap, report in got["reports"].items():
        capped = cases.model(a, b, nc, sorted_tree, cap) if len(a) <= 257 else dict(
            want, new=want["new"][:cap], gone=want["gone"][:cap],
            summary=want["summary"][:6] + [min(cap, want["summary"][0]), min(cap, want["summary"][4])])
        assert report == {"summary": capped["summary"], "stable": 1, "new": capped["new"], "gone": capped["gone"]}, (name, cap)


def test_known_reports(models):
    s = lambda name: dict(zip(cases.SUMMARY, models[name]["summary"]))
    assert s("equal_16386_file") == dict(new=0, shadowed=0, changed=0, same=16386, gone=0, unreachable=0, new_listed=0, gone_listed=0)
    assert s("every_row_changed_shuffled_16386_sorted")["changed"] == 16386
    assert models["edges_changed_16386_sorted"]["changed"] == cases.edge_leaves(16386) == models["edges_gone_16386_file"]["gone"]
    assert models["edges_changed_shuffled_257_file"]["changed"] == [0, 63, 64, 65, 255, 256]
    assert s("new_names_2_file")["new"] == 10 > 2 and s("new_names_16386_sorted")["new"] == 8
    m = models["twice_in_b_257_file"]
    assert m["row_state"][0] == cases.ROW_SAME and m["row_state"][257] == cases.ROW_SHADOWED and m["leaf_state"][0] == cases.LEAF_SAME and not m["changed"]
    m = models["twice_in_b_first_changed_257_file"]
    assert m["row_state"][3] == cases.ROW_CHANGED and m["row_state"][257] == cases.ROW_SHADOWED and m["changed"] == [3]
    m = models["twice_in_a_65_file"]
    assert [m["leaf_state"][i] for i in (0, 65, 32, 66, 67)] == [cases.LEAF_CHANGED, cases.LEAF_UNREACHABLE, cases.LEAF_CHANGED,
                                                                  cases.LEAF_UNREACHABLE, cases.LEAF_UNREACHABLE]
    assert m["leaf_state"][68:] == [cases.LEAF_PADDING] * 60 and s("twice_in_a_65_file")["unreachable"] == 3
    assert s("twice_in_a_gone_2_file")["gone"] == 1 and s("twice_in_a_gone_2_file")["unreachable"] == 1
    m = models["field_equal_file"]
    assert m["row_state"] == [cases.ROW_SAME, cases.ROW_SAME, cases.ROW_SAME, cases.ROW_CHANGED] and m["balances"] == [[1, 3]]
    assert models["empty_name_in_tree_file"]["row_leaf"] == [5, 1] and models["empty_name_in_tree_file"]["changed"] == [5]


def test_the_numpy_model_is_the_model_on_every_case_of_fixed_width_names(models):
    fixed = [c for c in CASES if cases.fixed_width(c[1]) and cases.fixed_width(c[2]) and len(c[1][0][0]) == len(c[2][0][0])]
    assert {c[0].rsplit("_", 2)[0] for c in fixed} >= {"equal", "every_row_changed_shuffled", "edges_changed_shuffled", "edges_gone_shuffled",
                                                        "twice_in_b", "twice_in_b_first_changed", "twice_in_a", "twice_in_a_gone"}
    assert {"edges_gone_16386_sorted", "twice_in_a_257_file", "one_currency_65_sorted"} <= {c[0] for c in fixed}
    for name, a, b, nc, sorted_tree in fixed:
        want = models[name]
        for cap in [None] + (cases.caps_of(want) if len(a) <= 257 else [1]):
            want = models[name] if cap is None else cases.model(a, b, nc, sorted_tree, cap)
            got = cases.model_np(cases.as_numbers(a), cases.as_numbers(b), sorted_tree, cap)
            assert sorted(got) == sorted(want)
            for key in want:
                assert (got[key] if key in ("n_tree", "depth", "summary") else got[key].tolist()) == want[key], (name, cap, key)


def test_the_big_case_is_built_from_the_edges_past_64_groups():
    """what BIG is for -- a wave sums LANES group totals a trip -- and what the big case puts where, in both kinds of tree"""
    assert (cases.LANES, cases.TRIP_ROWS, cases.BIG) == (64, 64 * cases.GROUP_ROWS, 65 * cases.GROUP_ROWS + 2) and cases.BIG == 1_064_962
    group = lambda item: item // cases.GROUP_ROWS             # the groups before an item's own are 0 .. group - 1
    trips = lambda item: -(-group(item) // cases.LANES)
    assert [trips(cases.BIG - 3), trips(cases.BIG - 2), trips(cases.BIG - 1)] == [1, 2, 2] and group(cases.BIG - 3) == cases.LANES
    assert trips(cases.TRIP_ROWS) == 1 and group(cases.TRIP_ROWS - 1) == cases.LANES - 1
    assert (cases.BIG - 1).bit_length() == 21 and (1 << 21) // cases.GROUP_ROWS == 2 * cases.LANES and 10 ** (cases.BIG_WIDTH - 1) < cases.BIG
    edge = 65 * cases.GROUP_ROWS
    for sorted_tree in (False, True):
        big = cases.big_case(sorted_tree)
        a_keys, b1_keys = big["a"][0], big["b1"][0]
        assert sorted(a_keys.tolist()) == list(range(cases.BIG)) and b1_keys.size == cases.BIG + 3 and big["b2"][0] is a_keys
        m = cases.model_np(big["a"], big["b1"], sorted_tree)
        for key, listed in (("changed", "changed"), ("gone", "gone"), ("new", "new")):
            assert np.array_equal(m[listed], big[key]), (sorted_tree, key)
        assert np.array_equal(np.flatnonzero(m["row_state"] == cases.ROW_SHADOWED), big["shadowed"])
        assert m["summary"][:6] == [big["new"].size, 3, big["changed"].size, cases.BIG - big["new"].size - big["changed"].size,
                                    big["gone"].size, 0]
        # every list has items in every group up to 65, the groups' totals differ, and the places around the second trip are taken
        for key, n_groups in (("changed", 66), ("gone", 66), ("new", 66)):
            per_group = np.bincount(big[key] // cases.GROUP_ROWS, minlength=n_groups)
            assert per_group.size == n_groups and per_group[:65].min() >= 1 and len(set(per_group.tolist())) >= 4, (sorted_tree, key)
        assert {edge - 1, edge} <= set(big["changed"].tolist()) and {edge - 2, edge + 1} <= set(big["gone"].tolist())
        assert {cases.GROUP_ROWS - 1, cases.GROUP_ROWS, cases.TRIP_ROWS - 1, cases.TRIP_ROWS} <= set(big["changed"].tolist())
        if sorted_tree:
            assert {edge - 1, edge, edge + 1} <= set(big["new"].tolist())
        else:
            assert np.array_equal(big["new"], big["gone"])
        # the apply case: the same leaves change, every row is found, nothing else differs
        m2 = cases.model_np(big["a"], big["b2"], sorted_tree)
        assert np.array_equal(m2["changed"], big["changed"]) and m2["summary"] == [0, 0, big["changed"].size, cases.BIG - big["changed"].size, 0, 0, 0, 0]
        assert cases.model_np(big["b2"], big["b2"], sorted_tree)["summary"][2:4] == [0, cases.BIG]


def test_the_fixed_width_writer_writes_the_cases_text(tmp_path):
    big = cases.big_case(False, 300)
    keys, bal = big["b1"]
    path = cases.write_big(tmp_path / "b1.csv", keys, bal)
    rows = [(f"{k:07d}".encode(), [f"{v:08d}" for v in row]) for k, row in zip(keys.tolist(), bal.tolist())]
    assert open(path).read() == cases.text_of(rows, 2)
    m = cases.model_np(big["a"], big["b1"], False)
    a_rows = [(f"{k:07d}".encode(), [str(v) for v in row]) for k, row in zip(big["a"][0].tolist(), big["a"][1].tolist())]
    want = cases.model(a_rows, rows, 2, False)
    assert all((m[key] if key in ("n_tree", "depth", "summary") else m[key].tolist()) == want[key] for key in want)


# ============================================================================= the entry points: exports and refusals
def test_exports_are_the_headers_prototypes_and_stay_out_of_the_other_headers():
    text = open(os.path.join(ROOT, "include", "summa_rounds.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(sr_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = [name for name, _ in protos]
    assert names == ffi.ROUNDS_EXPORTS == list(ffi.ROUNDS_ARGTYPES) == ["sr_mst_diff_scratch", "sr_mst_csv_diff_dev", "sr_mst_apply_diff_dev"]
    L = ffi.rounds_lib()
    for name, args in protos:
        getattr(L, name)
        assert len(ffi.ROUNDS_ARGTYPES[name]) == len(args.split(",")), name
    for other in ("summa_gpu.h", "summa_snapshot.h", "summa_prover.h", "summa_verifier.h"):
        assert not re.search(r"\bsr_", open(os.path.join(ROOT, "include", other)).read()), other
    assert not any(name.startswith("sr_") for name in ffi.SNAPSHOT_EXPORTS + ffi.PROVER_EXPORTS + ffi.VERIFIER_EXPORTS)


DIFF_KEYS = ("d_bytes", "length", "body_off", "tiles", "delim", "nc", "n", "spans", "t_bytes", "t_length", "t_body_off", "name_spans", "order",
             "n_tree", "depth", "leaf_bal", "row_leaf", "row_state", "leaf_state", "owner", "changed", "new_rows", "gone", "cap", "scratch",
             "problem", "summary")
DIFF_GOOD = dict(d_bytes=0x10000, length=100, body_off=10, tiles=0x20000, delim=ord(","), nc=2, n=3, spans=0x30000, t_bytes=0x40000, t_length=90,
                 t_body_off=9, name_spans=0x80000, order=0x70000, n_tree=3, depth=2, leaf_bal=0x100000, row_leaf=0x110000, row_state=0x120001,
                 leaf_state=0x130001, owner=0x140000, changed=0x150000, new_rows=0x160000, gone=0x170000, cap=3, scratch=0x500000,
                 problem=True, summary=True)


def diff_call(**change):
    """a good call but for `change`; the device pointers are not memory: a refused call never uses them"""
    a = dict(DIFF_GOOD, **change)
    problem, summary = C.c_uint64(77), (C.c_uint64 * 8)(*range(71, 79))
    args = [a[k] for k in DIFF_KEYS[:-2]] + [C.byref(problem) if a["problem"] else None, summary if a["summary"] else None, None]
    rc = ffi.rounds_lib().sr_mst_csv_diff_dev(*args)
    assert problem.value == 77 and list(summary) == list(range(71, 79))
    return rc, ffi.lib().sg_last_error().decode()


DIFF_REFUSED = [({k: None}, "null") for k in ("d_bytes", "tiles", "spans", "t_bytes", "name_spans", "leaf_bal", "row_leaf", "row_state",
                                              "leaf_state", "owner", "changed", "scratch")]
DIFF_REFUSED += [({"problem": False}, "null"), ({"summary": False}, "null"), ({"new_rows": None}, "non-zero cap"), ({"gone": None}, "non-zero cap"),
                 ({"nc": 0}, "n_currencies"), ({"nc": 65}, "n_currencies"), ({"depth": 31}, "depth"), ({"delim": 10}, "delimiter"),
                 ({"delim": 13}, "delimiter"), ({"delim": ord("5")}, "delimiter"), ({"delim": ord('"')}, "delimiter"), ({"delim": 0}, "delimiter"),
                 ({"delim": 0xC3}, "delimiter"), ({"delim": 256 + ord(",")}, "delimiter"), ({"body_off": 100}, "body_off"),
                 ({"body_off": 101}, "body_off"), ({"length": (1 << 32) + 10}, "body"), ({"n": 0}, "n_rows"), ({"n": 91}, "n_rows"),
                 ({"t_body_off": 91}, "tree's body_off"), ({"t_length": (1 << 32) + 9}, "tree's body_off"), ({"n_tree": 0}, "n_tree"),
                 ({"n_tree": 5}, "n_tree"), ({"tiles": 0x20002}, "d_tile_scratch"), ({"spans": 0x30004}, "d_span_scratch"),
                 ({"name_spans": 0x80002}, "d_name_spans"), ({"order": 0x70002}, "d_order"), ({"leaf_bal": 0x100008}, "d_leaf_balances"),
                 ({"row_leaf": 0x110002}, "d_row_leaf"), ({"owner": 0x140001}, "d_owner"), ({"changed": 0x150002}, "d_changed"),
                 ({"new_rows": 0x160002}, "d_new_rows"), ({"gone": 0x170003}, "d_gone"), ({"scratch": 0x500002}, "d_scratch")]


def test_the_diff_refuses_bad_arguments(exe):
    for change, word in DIFF_REFUSED:
        rc, msg = diff_call(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("sr_mst_csv_diff: ") and word in msg, (change, msg)
    # the same words from the header's own function, and "" for what the entry point accepts: no order (a sorted tree), null lists
    # with cap == 0, a tree's text that is all header
    def problem(**change):
        a = dict(dict(DIFF_GOOD, problem=0x600000, summary=0x700000), **{k: (0 if v is False else v) for k, v in change.items()})
        return " ".join(ask(exe, ["problem " + " ".join(str(a[k] or 0) for k in DIFF_KEYS)])[0][1:])
    assert problem() == "" and problem(order=None) == "" and problem(new_rows=None, gone=None, cap=0) == "" and problem(cap=0) == ""
    assert problem(t_body_off=90) == "" and problem(n=90) == "" and problem(n_tree=4) == "" and problem(depth=30, n_tree=1 << 30) == ""
    for change, word in DIFF_REFUSED:
        assert word in problem(**change), change


APPLY_KEYS = ("d_bytes", "length", "body_off", "spans", "n", "owner", "changed", "n_changed", "depth", "nc", "users", "leaf_bal", "hashes", "node_bal")
APPLY_GOOD = dict(d_bytes=0x10000, length=100, body_off=10, spans=0x30000, n=3, owner=0x140000, changed=0x150000, n_changed=2, depth=2, nc=2,
                  users=0x200000, leaf_bal=0x300000, hashes=0x400000, node_bal=0x500000)
APPLY_REFUSED = [({k: None}, "null") for k in ("d_bytes", "spans", "owner", "changed", "users", "leaf_bal", "hashes", "node_bal")]
APPLY_REFUSED += [({"nc": 0}, "n_currencies"), ({"nc": 65}, "n_currencies"), ({"depth": 31}, "depth"), ({"body_off": 100}, "body_off"),
                  ({"length": (1 << 32) + 10}, "body"), ({"n": 0}, "n_rows"), ({"n": 91}, "n_rows"), ({"n_changed": 4}, "more changed leaves"),
                  ({"n_changed": 5, "n": 6}, "more changed leaves"), ({"spans": 0x30004}, "d_span_scratch"), ({"owner": 0x140002}, "d_owner"),
                  ({"changed": 0x150001}, "d_changed"), ({"users": 0x200008}, "16-byte"), ({"node_bal": 0x500004}, "16-byte")]


def apply_call(**change):
    a = dict(APPLY_GOOD, **change)
    rc = ffi.rounds_lib().sr_mst_apply_diff_dev(*[a[k] for k in APPLY_KEYS], None)
    return rc, ffi.lib().sg_last_error().decode()


def test_the_apply_refuses_bad_arguments(exe):
    refused = APPLY_REFUSED + [({"leaf_bal": 0x500000}, "overlaps"), ({"leaf_bal": 0x500000 + 32 * 7 * 2 - 16}, "overlaps"),
                               ({"leaf_bal": 0x500000 - 32 * 4 * 2 + 16}, "overlaps")]
    for change, word in refused:
        rc, msg = apply_call(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("sr_mst_apply_diff: ") and word in msg, (change, msg)
    def problem(**change):
        a = dict(APPLY_GOOD, **change)
        return " ".join(ask(exe, ["apply_problem " + " ".join(str(a[k] or 0) for k in APPLY_KEYS)])[0][1:])
    assert problem() == "" and problem(n_changed=0) == "" and problem(n_changed=3) == ""
    for change, word in APPLY_REFUSED:
        assert word in problem(**change), change


# ============================================================================= the report from entries on the host
class _HostTree(M._Tree):
    """entries alone: what the base implementation reads"""

    def __init__(self, entries, nc, is_sorted=False):
        self.entries, self.is_sorted, self.n_currencies, self.depth = entries, is_sorted, nc, max(0, (len(entries) - 1).bit_length())


def host_tree(a, nc, sorted_tree):
    order = cases.leaf_order(a, sorted_tree)
    entries = [(a[r][0].decode(), [int(x) for x in a[r][1]]) for r in order]
    entries += [(None, [0] * nc)] * ((1 << max(0, (len(entries) - 1).bit_length())) - len(entries))
    return _HostTree(entries, nc, sorted_tree)


SMALL = [c for c in CASES if len(c[1]) <= 260]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_diff_entries_agrees_with_the_model(case, models):
    name, a, b, nc, sorted_tree = case
    entries = [(nm.decode(), [int(x) for x in bal]) for nm, bal in b]
    want = models[name]
    for cap in [None] + cases.caps_of(want):
        got = host_tree(a, nc, sorted_tree).diff_entries(entries, cap)
        capped = cases.model(a, b, nc, sorted_tree, cap)
        assert got.ingest == "host" and got.summary() == dict(zip(cases.SUMMARY, capped["summary"])), (name, cap)
        assert got.changed.dtype == got.new_rows.dtype == got.gone.dtype == np.uint32
        assert got.changed.tolist() == capped["changed"] and got.new_rows.tolist() == capped["new"] and got.gone.tolist() == capped["gone"]
        assert got.row_leaf().tolist() == capped["row_leaf"] and got.row_state().tolist() == capped["row_state"]
        assert got.leaf_state().tolist() == capped["leaf_state"] and got.owner().tolist() == capped["owner"]
        assert [[v % cases.R for v in row] for row in got.new_balances] == capped["balances"]
        assert got.ok == (capped["summary"][0] == capped["summary"][2] == capped["summary"][4] == 0)


def test_diff_csv_of_a_host_tree_parses_the_file(tmp_path):
    name, a, b, nc, sorted_tree = [c for c in CASES if c[0] == "three_currencies_65_file"][0]
    path = cases.write_case(tmp_path, "b", cases.text_of(b, nc))
    got = host_tree(a, nc, sorted_tree).diff_csv(path)
    want = cases.model(a, b, nc, sorted_tree)
    assert got.summary() == dict(zip(cases.SUMMARY, want["summary"])) and got.changed.tolist() == want["changed"]
    with pytest.raises(ValueError, match="cap below 0"):
        host_tree(a, nc, sorted_tree).diff_entries([], -1)
    with pytest.raises(ValueError, match="holds no entries"):
        _HostTree.diff_entries(type("T", (M._Tree,), {"entries": None})(), [])
    with pytest.raises(ValueError, match="wrong number of balances"):
        host_tree(a, nc, sorted_tree).diff_entries([("x", [1])])


def test_apply_diff_refuses_a_stale_diff_and_another_trees():
    class _Counted(_HostTree, M.DeviceMerkleSumTree):
        """the device tree's apply over entries alone: the refusals come before anything touches a device"""
        def __init__(self, entries):
            _HostTree.__init__(self, entries, 2)
    a = [("a", [1, 2]), ("b", [3, 4])]
    tree, other = _Counted(list(a)), _Counted(list(a))
    diff = tree.diff_entries([("a", [1, 5])])
    assert diff.changed.tolist() == [0] and diff.n_gone == 1
    with pytest.raises(ValueError, match="another tree"):
        other.apply_diff(diff)
    tree._updates += 1                                        # what every update of the tree does
    with pytest.raises(ValueError, match="before another update"):
        tree.apply_diff(diff)
    assert tree.entries == a
