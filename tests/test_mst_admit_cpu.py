"""A round settled in full on a tree, without a GPU: the rules of csrc/mst_admit.h, whose text the kernels compile, run by the header's
own serial steps in tests/cpp/mst_admit_check.cpp (behind the CSV reader's, the sort's and the diff's; a stand-alone program built
by the host compiler under address / undefined sanitizers, a process of its own) and compared with the model of mst_admit_cases.py on
every case.  And the geometry and the scratch size, the exports of include/summa_admit.h, what the entry points refuse before they
touch a device, and the model's round trip through the snapshot's text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import mst_admit_cases as cases
from circuits_halo2_amd import ffi
from circuits_halo2_amd import merkle_sum_tree as M

SG_ERR_INVALID = -1
CASES = cases.cases()
IDS = [c[0] for c in CASES]
BIG = 1 << 40                                               # a cap that leaves every list complete


def build(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *flags,
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_admit_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the check program once more under the sanitizers: what every test below asks"""
    return build(str(tmp_path_factory.mktemp("mst_admit") / "mst_admit_check"), "-O1", "-fsanitize=address,undefined")


@pytest.fixture(scope="module")
def exe_plain(tmp_path_factory):
    """... and as the mirror is normally built: optimized, no sanitizer"""
    return build(str(tmp_path_factory.mktemp("mst_admit_plain") / "mst_admit_check"), "-O2")


def ask(exe, lines):
    """command lines -> the program's output lines, split into words"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def models():
    return {c[0]: cases.settled(c[1], c[2], c[3]) for c in CASES}


def cap_of(refusal):
    return cases.CAP_SHORT if refusal in ("cap_new", "cap_gone") else BIG


@pytest.fixture(scope="module")
def command_lines(tmp_path_factory):
    """one `settle` line a case, both keywords set"""
    d = tmp_path_factory.mktemp("mst_admit_files")
    lines = []
    for name, a, b, nc, refusal in CASES:
        pa, pb = cases.write_case(d, name + ".a", cases.text_a(name, a, nc)), cases.write_case(d, name + ".b", cases.text_of(b, nc))
        lines.append(f"settle {pa} {pb} {nc} 1 1 {cap_of(refusal)}")
    return lines


@pytest.fixture(scope="module")
def answers(exe, command_lines):
    """the program's answer for every case, by name: one run"""
    out, cur = [], None
    for w in ask(exe, command_lines):
        if w[0] == "tree":
            cur = {"tree": [int(x) for x in w[1:]]}
        elif w[0] == "refused":
            cur = dict(cur or {}, refused=" ".join(w[1:]))
        elif w[0] in ("file", "problem", "bytes", "order", "sortednew", "union", "packed"):
            cur[w[0]] = [int(x) for x in w[1:]]
        elif w[0] in ("sorted", "leafnames"):
            cur[w[0]] = [b"" if x == "-" else bytes.fromhex(x) for x in w[1:]]
        elif w[0] == "end":
            out.append(cur)
            cur = None
    assert len(out) == len(CASES)
    return dict(zip(IDS, out))


def test_the_geometry_and_the_list_of_cases(exe):
    assert ask(exe, ["geometry"]) == [["geometry", "256", "64", "256", "64"]]
    names = set(IDS)
    for n in cases.TREES:
        free = cases.free_of(n)
        assert {f"tree_{n}_new_{k}" for k in (0, 1, 2, 64, 65, 257, free) if k <= free} <= names
    assert {"tree_2049_new_2047", "tree_257_new_255", "tree_32769_new_16386", "contents_300", "currencies_1_65", "currencies_3_65"} <= names
    assert [c[4] for c in CASES if c[4]] == ["no_room", "no_room", "name_too_long", "cap_new", "cap_gone"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_mirror_agrees_with_the_model(answers, models, case):
    name, a, b, nc, refusal = case
    got, want = answers[name], models[name]
    assert got["tree"] == [len(a), want["diff"]["depth"]] and got["file"] == [len(b)]
    if refusal == "no_room":
        assert want["refusal"] == "no_room" and "2^depth" in got["refused"] and "order" not in got
        return
    if refusal == "name_too_long":
        assert want["refusal"][0] == "name_too_long" and got["problem"] == [want["refusal"][1] << 8 | 7] and "order" not in got
        return
    if refusal in ("cap_new", "cap_gone"):
        assert ("NEW" if refusal == "cap_new" else "GONE") in got["refused"] and "incomplete" in got["refused"] and "order" not in got
        return
    assert want["refusal"] is None and "refused" not in got and "problem" not in got
    n, n_tree = want["n"], len(a)
    assert len(want["diff"]["new"]) == n - n_tree
    if n == n_tree:                                           # nobody to admit: the text and the index stay as they are
        assert got["bytes"] == [0] and got["order"] == got["sorted"] == got["leafnames"] == got["sortednew"] == []
    else:
        assert sorted(got["order"]) == list(range(n)), "the merged order is no bijection"
        assert got["order"] == want["order"] and got["sorted"] == want["names"]
        assert got["leafnames"] == [name for name, _ in want["entries"][:n]]
        assert got["bytes"] == [sum(len(name) for name, _ in want["entries"][n_tree:n])]
        by_name = sorted(want["diff"]["new"], key=lambda r: b[r][0])                # stable: within a name by file row
        assert got["sortednew"] == by_name
    assert got["union"] == want["leaves"]
    words = np.array(got["packed"], dtype=np.uint32).tobytes()
    assert words == b"".join(M._to_fr_bytes(v) for row in want["balances"] for v in row)


def test_the_optimized_build_without_sanitizers_answers_the_same(exe, exe_plain, command_lines):
    """the mirror as it is normally compiled, over all cases: word for word the sanitized build's output, which the model checks"""
    assert ask(exe_plain, command_lines) == ask(exe, command_lines)
    assert ask(exe_plain, ["geometry", "scratch 2049 3 2047"]) == ask(exe, ["geometry", "scratch 2049 3 2047"])


def test_known_shapes(models):
    m = models["tree_32769_new_16386"]
    assert m["n"] == 32769 + 16386 and m["leaves"][-1] == 32769 + 16385
    m = models["contents_300"]
    names = [name for name, _ in m["entries"][300:m["n"]]]
    assert names.count(b"twice") == 2 and b"" in names and b"n" * 64 in names
    rows = [r for r in m["diff"]["new"] if CASES[IDS.index("contents_300")][2][r][0] == b"twice"]
    assert rows[1] - rows[0] > 256
    assert m["names"][0] == b"" and m["names"][1] == b"!first" and m["names"][-1] == b"~last"
    assert cases.duplicates_of(m["entries"])[0] == 1
    m = models["tree_257_new_255"]
    assert m["n"] == 512 and m["entries"][511][0] is not None


@pytest.mark.parametrize("keys", [(0, 0), (1, 0), (0, 1)])
def test_the_keywords_are_independent(exe, tmp_path, keys):
    admit, zero = keys
    name, a, b, nc, _ = CASES[IDS.index("tree_65_new_2")]
    pa, pb = cases.write_case(tmp_path, "a", cases.text_of(a, nc)), cases.write_case(tmp_path, "b", cases.text_of(b, nc))
    got = {w[0]: w[1:] for w in ask(exe, [f"settle {pa} {pb} {nc} {admit} {zero} {BIG}"])}
    want = cases.settled(a, b, nc, bool(admit), bool(zero))
    assert [int(x) for x in got["union"]] == want["leaves"]
    assert (got["order"] != []) == bool(admit)
    words = np.array([int(x) for x in got["packed"]], dtype=np.uint32).tobytes()
    assert words == b"".join(M._to_fr_bytes(v) for row in want["balances"] for v in row)


def test_the_models_round_trip_through_the_snapshots_text(models, tmp_path):
    """`to_csv` text of the settled entries, read by the Python reader, gives the same entries back"""
    for name, _, _, nc, refusal in CASES:
        if refusal or len(models[name]["entries"]) > 4096:
            continue
        want = [(nm.decode(), bal) for nm, bal in models[name]["entries"] if nm is not None]
        path = cases.write_case(tmp_path, name + ".out", cases.csv_of(models[name]["entries"], nc))
        entries, _ = M.parse_csv_to_entries(path, nc)
        assert [(nm, [v % cases.R for v in bal]) for nm, bal in entries] == want, name


# ============================================================================= the entry points: exports and refusals
def test_exports_are_the_headers_prototypes_and_stay_out_of_the_other_headers():
    text = open(os.path.join(ROOT, "include", "summa_admit.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(sa_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = [name for name, _ in protos]
    assert names == ffi.ADMIT_EXPORTS == list(ffi.ADMIT_ARGTYPES) == ["sa_mst_admit_scratch", "sa_mst_admit_measure_dev", "sa_mst_settle_dev"]
    L = ffi.admit_lib()
    for name, args in protos:
        getattr(L, name)
        assert len(ffi.ADMIT_ARGTYPES[name]) == len(args.split(",")), name
        kinds = [C.c_void_p if "*" in arg else C.c_uint32 if "uint32_t" in arg else C.c_uint64 for arg in args.split(",")]
        assert ffi.ADMIT_ARGTYPES[name] == kinds, name
    for other in ("summa_gpu.h", "summa_snapshot.h", "summa_prover.h", "summa_verifier.h", "summa_rounds.h", "summa_export.h"):
        assert not re.search(r"\bsa_", open(os.path.join(ROOT, "include", other)).read()), other
    others = ffi.SNAPSHOT_EXPORTS + ffi.PROVER_EXPORTS + ffi.VERIFIER_EXPORTS + ffi.ROUNDS_EXPORTS + ffi.EXPORT_EXPORTS
    assert not any(name.startswith("sa_") for name in others)


def test_scratch_size(exe):
    L = ffi.admit_lib()
    size = C.c_uint64(77)
    for n, nc, m in ((0, 2, 1), (1 << 32, 2, 1), (5, 0, 1), (5, 65, 1), (5, 2, 0), (5, 2, 6)):
        assert L.sa_mst_admit_scratch(n, nc, m, C.byref(size)) == SG_ERR_INVALID and size.value == 77
        assert ffi.lib().sg_last_error().decode().startswith("sa_mst_admit_scratch: ")
    assert L.sa_mst_admit_scratch(5, 2, 1, None) == SG_ERR_INVALID
    sort_bytes = C.c_uint64(0)
    r4 = lambda x: (x + 3) & ~3
    lw = lambda items: -(-items // 64) + -(-(-(-items // 64)) // 256)
    shapes = [(1, 1, 1), (65, 2, 3), (2049, 3, 2047), (16386, 2, 16386), (1 << 20, 2, 10000)]
    for (n, nc, m), words in zip(shapes, ask(exe, [f"scratch {n} {nc} {m}" for n, nc, m in shapes])):
        assert L.sa_mst_admit_scratch(n, nc, m, C.byref(size)) == 0 and int(words[1]) == size.value
        ffi.check(ffi.snapshot_lib().ss_mst_sort_scratch(n, C.byref(sort_bytes)))
        at_order = 4 + r4(sort_bytes.value // 4)
        at_sorted = at_order + r4(n) + r4(2 * n) + r4(n) + 2 * r4(m) + r4(lw(n)) + r4(lw(m))
        assert [int(x) for x in words[2:]] == [4, at_order, at_sorted]
        assert size.value == 4 * at_sorted + 8 * (n + 1 + 2 * n * (1 + nc)) and at_sorted % 4 == 0


MEASURE_KEYS = ("d_bytes", "length", "body_off", "spans", "n", "nc", "row_state", "new_rows", "n_new", "n_tree", "depth", "scratch", "name_bytes",
                "problem")
MEASURE_GOOD = dict(d_bytes=0x10000, length=100, body_off=10, spans=0x30000, n=3, nc=2, row_state=0x120001, new_rows=0x160000, n_new=1,
                    n_tree=3, depth=2, scratch=0x500000, name_bytes=True, problem=True)
MEASURE_REFUSED = [({k: None}, "null") for k in ("d_bytes", "spans", "row_state", "new_rows", "scratch")]
MEASURE_REFUSED += [({"name_bytes": False}, "null"), ({"problem": False}, "null"), ({"nc": 0}, "n_currencies"), ({"nc": 65}, "n_currencies"),
                    ({"depth": 31}, "depth"), ({"body_off": 100}, "body_off"), ({"length": (1 << 32) + 10}, "body"), ({"n": 0}, "n_rows"),
                    ({"n": 91}, "n_rows"), ({"n_new": 0}, "n_new"), ({"n_new": 4}, "n_new"), ({"n_tree": 0}, "n_tree"), ({"n_tree": 5}, "n_tree"),
                    ({"n_new": 2}, "rebuild"), ({"n_tree": 4}, "rebuild"), ({"spans": 0x30004}, "d_span_scratch"),
                    ({"new_rows": 0x160002}, "d_new_rows"), ({"scratch": 0x500008}, "d_scratch")]


def test_the_measure_refuses_before_it_touches_a_device(exe):
    """every refusal leaves both outputs as they were; the mirror's words are the entry point's"""
    lines = []
    for change, word in MEASURE_REFUSED:
        a = dict(MEASURE_GOOD, **change)
        name_bytes, problem = C.c_uint64(77), C.c_uint64(78)
        args = [a[k] for k in MEASURE_KEYS[:-2]] + [C.byref(name_bytes) if a["name_bytes"] else None, C.byref(problem) if a["problem"] else None, None]
        rc = ffi.admit_lib().sa_mst_admit_measure_dev(*args)
        msg = ffi.lib().sg_last_error().decode()
        assert rc == SG_ERR_INVALID and msg.startswith("sa_mst_admit_measure: ") and word in msg, (change, msg)
        assert (name_bytes.value, problem.value) == (77, 78)
        lines.append("measure_problem " + " ".join(str(int(a[k] or 0)) for k in MEASURE_KEYS))
    for (change, word), words in zip(MEASURE_REFUSED, ask(exe, lines)):
        assert word in " ".join(words[1:]), (change, words)
    assert ask(exe, ["measure_problem " + " ".join(str(int(MEASURE_GOOD[k])) for k in MEASURE_KEYS)]) == [["measure_problem"]]


SETTLE_KEYS = ("d_bytes", "length", "body_off", "spans", "n", "nc", "owner", "leaf_state", "changed", "n_changed", "gone", "n_gone", "new_rows",
               "n_new", "scratch", "t_bytes", "t_length", "t_body_off", "name_spans", "order", "leaf_spans", "n_tree", "depth", "out_bytes",
               "name_bytes", "out_name_spans", "out_order", "out_leaf_spans", "users", "leaf_bal", "node_h", "node_b")
SETTLE_GOOD = dict(d_bytes=0x10000, length=100, body_off=10, spans=0x30000, n=3, nc=2, owner=0x140000, leaf_state=0x130001, changed=0x150000,
                   n_changed=1, gone=0x170000, n_gone=1, new_rows=0x160000, n_new=1, scratch=0x500000, t_bytes=0x40000, t_length=90,
                   t_body_off=9, name_spans=0x80000, order=0x70000, leaf_spans=0x90000, n_tree=3, depth=2, out_bytes=0x600000, name_bytes=5,
                   out_name_spans=0x610000, out_order=0x620000, out_leaf_spans=0x630000, users=0x200000, leaf_bal=0x300000, node_h=0x400000,
                   node_b=0x700000)
SETTLE_REFUSED = [({k: None}, "null") for k in ("d_bytes", "spans", "owner", "leaf_state", "changed", "gone", "new_rows", "scratch", "t_bytes",
                                                "name_spans", "order", "leaf_spans", "out_bytes", "out_name_spans", "out_order",
                                                "out_leaf_spans", "users", "leaf_bal", "node_h", "node_b")]
SETTLE_REFUSED += [({"nc": 0}, "n_currencies"), ({"depth": 31}, "depth"), ({"body_off": 100}, "body_off"), ({"n": 0}, "n_rows"),
                   ({"n_changed": 4}, "changed"), ({"n_gone": 5}, "gone"), ({"n_new": 4}, "new rows"), ({"n_tree": 0}, "n_tree"),
                   ({"n_new": 2}, "rebuild"), ({"n_changed": 2, "n_gone": 2}, "named leaves"), ({"name_bytes": 65}, "name_bytes"),
                   ({"t_length": (1 << 32) + 8, "name_bytes": 1}, "names appended"), ({"t_length": (1 << 32) + 9}, "tree's body_off"),
                   ({"spans": 0x30004}, "d_span_scratch"), ({"changed": 0x150002}, "list of the diff"), ({"scratch": 0x500008}, "d_scratch"),
                   ({"out_order": 0x620002}, "index array"), ({"users": 0x200008}, "tree array"), ({"node_b": 0x300000 + 64}, "overlaps")]


def test_the_settle_refuses_before_it_touches_a_device(exe):
    lines = []
    for change, word in SETTLE_REFUSED:
        a = dict(SETTLE_GOOD, **change)
        rc = ffi.admit_lib().sa_mst_settle_dev(*[a[k] for k in SETTLE_KEYS], None)
        msg = ffi.lib().sg_last_error().decode()
        assert rc == SG_ERR_INVALID and msg.startswith("sa_mst_settle: ") and word in msg, (change, msg)
        if word != "overlaps":                                # the entry point's own
            lines.append((change, word, "settle_problem " + " ".join(str(int(a[k] or 0)) for k in SETTLE_KEYS)))
    for (change, word, _), words in zip(lines, ask(exe, [ln for _, _, ln in lines])):
        assert word in " ".join(words[1:]), (change, words)
    assert ask(exe, ["settle_problem " + " ".join(str(int(SETTLE_GOOD[k])) for k in SETTLE_KEYS)]) == [["settle_problem"]]
    # nobody to admit: the index and the outputs may be null
    nobody = dict(SETTLE_GOOD, n_new=0, **{k: None for k in ("new_rows", "scratch", "t_bytes", "name_spans", "order", "leaf_spans", "out_bytes",
                                                            "out_name_spans", "out_order", "out_leaf_spans")})
    assert ask(exe, ["settle_problem " + " ".join(str(int(nobody[k] or 0)) for k in SETTLE_KEYS)]) == [["settle_problem"]]


# ============================================================================= Python: the keywords on trees whose entries are on the host
class _HostTree(M.DeviceMerkleSumTree):
    """the device tree's apply over entries alone: the refusals and the host's way come before anything touches a device"""

    def __init__(self, entries, nc=2):
        size = 1 << max(0, (len(entries) - 1).bit_length())
        self.entries = list(entries) + [(None, [0] * nc)] * (size - len(entries))
        self.n_currencies, self.depth, self.calls = nc, size.bit_length() - 1, []

    def update_leaves_at(self, indices, balances):
        self.calls.append((list(indices), [list(b) for b in balances]))
        self._updates += 1

    def root(self):
        return "root"


def test_free_leaves_and_admitted_on_a_host_tree():
    tree = _HostTree([("a", [1, 2]), ("b", [3, 4]), ("c", [5, 6])])
    assert tree.free_leaves == 1
    diff = tree.diff_entries([("a", [1, 2]), ("x", [1, 1]), ("y", [2, 2])])
    assert diff.admitted == range(3, 5) and diff.n_gone == 2 and diff.n_new == 2
    with pytest.raises(ValueError, match="holds no entries"):
        type("T", (M._Tree,), {"entries": None})().free_leaves


def test_the_hosts_way_zeroes_the_gone_through_update_leaves_at_and_admits_nobody():
    a = [("a", [1, 2]), ("b", [3, 4]), ("c", [5, 6])]
    b = [("c", [5, 7]), ("x", [1, 1])]
    tree = _HostTree(a)
    tree.apply_diff(tree.diff_entries(b))                     # the defaults: the changed leaf alone
    assert tree.calls == [([2], [[5, 7]])] and tree._updates == 1
    tree = _HostTree(a)
    tree.apply_diff(tree.diff_entries(b), zero_gone=True)
    assert tree.calls == [([2, 0, 1], [[5, 7], [0, 0], [0, 0]])] and tree._updates == 1
    tree = _HostTree(a)
    with pytest.raises(ValueError, match="device diff"):
        tree.apply_diff(tree.diff_entries(b), admit_new=True)
    with pytest.raises(ValueError, match="gone leaves incomplete"):
        tree.apply_diff(tree.diff_entries(b, cap=1), zero_gone=True)
    assert tree.calls == [] and tree._updates == 0
    nothing = tree.diff_entries(a)
    assert tree.apply_diff(nothing, zero_gone=True) == "root" and tree.calls == []


def test_an_unparsed_row_is_read_up_to_the_source_files_end_not_into_the_admitted_names():
    """a file A without a final newline: behind an admit the names follow the last row's last digit in the tree's text, and the
    entry of the last old leaf, which the round left alone, is still its own row's"""
    import torch
    text = b"username,balance_ETH_ETH,balance_USDT_ETH\naa,1,2\nbb,3,4"
    body_off = text.index(b"\n") + 1
    u8 = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy())
    tree = _HostTree.__new__(_HostTree)
    tree.n_currencies, tree.depth, tree._csv_lazy, tree._applied = 2, 2, ("unread.csv", {}), (np.array([2, 3], dtype=np.uint32),)
    tree._balances_of_leaves = lambda leaves: [[9, 9] for _ in leaves]
    for names in (b"55" + b"new", b"x" + b"55"):
        spans = [0, 2, 7, 9] + ([13, 15, 15, 18] if names.startswith(b"55") else [13, 14, 14, 16])
        tree._index_dev = {"text": u8(text + names), "size": len(text) + len(names), "file_size": len(text), "body_off": body_off, "delim": ",",
                           "n": 4, "d_leaf_name_spans": torch.tensor(spans, dtype=torch.int32), "d_name_spans": None}
        assert tree._finds_on_device()
        assert [tree.get_entry(i) for i in range(2)] == [("aa", [1, 2]), ("bb", [3, 4])]
        assert tree.get_entry(2)[0] == names[:2 if names.startswith(b"55") else 1].decode() and tree.get_entry(2)[1] == [9, 9]
        assert tree._names_of_leaves(2, 4) == (["55", "new"] if names.startswith(b"55") else ["x", "55"])
