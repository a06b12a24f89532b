"""The host side of an in-place update of a device-resident Merkle sum tree, without a GPU: the launch plan of
csrc/mst_update_plan.h (built by the host compiler into tests/cpp/mst_update_plan_check.cpp, once plainly and once under
address / undefined sanitizers) against sets of Python integers, what sg_mst_update_dev refuses -- it validates before it
touches the device, so every refusal is an SG_ERR_INVALID on any machine --, where the symbol is declared, and the Python
front end of `DeviceMerkleSumTree.update_leaves` with the device call replaced."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, _level_first, pack_balances, pack_entries

SG_ERR_INVALID = -1


# ============================================================================= the plan, on the host
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_update") / ("mst_update_plan_check_" + request.param))
    extra = ["-fsanitize=address,undefined"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + extra +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_update_plan_check.cpp"), "-o", out])
    return out


def ask(exe, commands):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.splitlines()


PLAN_CASES = [(0, [0]),
              (1, [0]), (1, [1]), (1, [0, 1]),
              (5, [0]), (5, [31]), (5, [0, 31]), (5, [6, 7]), (5, [7, 8]), (5, list(range(32))),
              (8, sorted(random.Random(8).sample(range(256), 129))),
              (9, list(range(0, 258, 2))),
              (30, [0, (1 << 30) - 1])]


def test_level_first_is_the_sum_of_the_levels_below(exe):
    """mst_level_first, the one place that knows the level-major layout (the build, the update and the witness kernel's table use
    it), against the sum it stands for; 62 is the deepest tree a 64-bit node number takes"""
    depths = [0, 1, 2, 30, 31, 62]
    out = ask(exe, [f"o {d}" for d in depths])
    assert len(out) == len(depths)
    for d, line in zip(depths, out):
        assert line.split()[0] == "first"
        want = [sum(1 << (d - j) for j in range(l)) for l in range(d + 1)]
        assert [int(x) for x in line.split()[1:]] == want, d
        assert [_level_first(d, l) for l in range(d + 1)] == want, d           # the Python front end's copy


def test_plan_lists_are_the_distinct_parents_of_every_level(exe):
    out = ask(exe, [f"p {depth} {len(idx)} " + " ".join(map(str, idx)) for depth, idx in PLAN_CASES])
    at = 0
    for depth, idx in PLAN_CASES:
        what = f"depth {depth}, {len(idx)} leaves from {idx[0]}"
        want = [sorted({i >> l for i in idx}) for l in range(1, depth + 1)]
        head = out[at].split()
        assert head[0] == "offsets" and [int(x) for x in head[1:]] == [0] + list(np.cumsum([len(w) for w in want])), what
        for l in range(1, depth + 1):
            line = out[at + l].split()
            assert line[:2] == ["list", str(l)] and [int(x) for x in line[2:]] == want[l - 1], f"{what}: level {l}"
        if depth:
            assert want[-1] == [0] and sum(map(len, want)) <= len(idx) * depth, what
        if depth == 9:     # what this case is there for: the one list that runs one past a 128-thread block of the level kernel
            assert [len(w) for w in want[:2]] == [129, 65] and [int(x) for x in head[1:3]] == [0, 129], what
        at += depth + 1
    assert at == len(out)
    # what the depth-5 pairs are there for: 0 and 31 meet at the root only, 7 and 8 are neighbours that meet high up, 6 and 7 are siblings
    assert [len({i >> l for i in [0, 31]}) for l in range(1, 6)] == [2, 2, 2, 2, 1]
    assert [len({i >> l for i in [7, 8]}) for l in range(1, 6)] == [2, 2, 2, 1, 1] and {6 >> 1, 7 >> 1} == {3}


def v(depth, nc, idx, fields, off=None):
    """a `v` command: the offsets of `fields` (byte strings) unless given"""
    if off is None:
        off = [0] + list(np.cumsum([len(f) for f in fields]))
    data = b"".join(fields).hex() or "-"
    return f"v {depth} {nc} {len(idx)} " + " ".join(map(str, idx)) + f" {len(off)} " + " ".join(map(str, off)) + " " + data


PROBLEMS = [
    ("", v(2, 2, [1, 3], [b"1", b"22", b"333", b"0"])),
    ("", v(0, 1, [0], [b"5"])),
    ("no leaf to update", v(2, 1, [], [])),
    ("more leaves to update than the tree has", v(1, 1, [0, 1, 1], [b"1", b"2", b"3"])),
    ("leaf index 4 at position 1 is out of range", v(2, 1, [0, 4], [b"1", b"2"])),
    ("leaf index 1 at position 0 is out of range", v(0, 1, [1], [b"1"])),
    ("leaf indices do not strictly increase at position 2", v(2, 1, [0, 2, 2], [b"1", b"2", b"3"])),
    ("leaf indices do not strictly increase at position 1", v(2, 1, [3, 1], [b"1", b"2"])),
    ("balance field 2 is empty", v(2, 2, [1, 3], [b"1", b"22", b"", b"0"])),
    ("balance field 1 is not a decimal number", v(2, 2, [1, 3], [b"1", b"2a", b"3", b"0"])),
    ("balance field 3 is not a decimal number", v(2, 2, [1, 3], [b"1", b"2", b"3", b"-1"])),
    ("digit_off decreases at field 1", v(2, 2, [1, 3], [b"1", b"22", b"333", b"0"], off=[0, 3, 1, 6, 7])),
    ("digit_off[0] is not 0", v(2, 2, [1, 3], [b"1", b"22", b"333", b"0"], off=[1, 1, 3, 6, 7])),
    ("depth above 30", v(31, 1, [0], [b"1"])),
]


def test_problem_messages(exe):
    out = ask(exe, [cmd for _, cmd in PROBLEMS])
    assert len(out) == len(PROBLEMS)
    for (want, cmd), got in zip(PROBLEMS, out):
        assert got == "problem " + want, cmd


# ============================================================================= sg_mst_update_dev: refusals
class Call:
    """the arguments of a good call: leaves 1 and 3 of a tree of depth 2 with 2 currencies (4 fields); tests change one
    thing.  The device pointers are not memory: a call that is refused never gets as far as using them."""

    def __init__(self):
        self.idx, self.fields, self.depth, self.nc = [1, 3], [b"1", b"22", b"333", b"0"], 2, 2
        self.digit_off = None
        self.null = None
        self.dev = [0x10000, 0x20000, 0x30000, 0x40000]       # usernames, leaf balances, node hashes, node balances

    def run(self):
        idx = np.array(self.idx + [0], dtype=np.uint32)       # (never empty)
        data = np.frombuffer(b"".join(self.fields) + b"\0", dtype=np.uint8).copy()
        off = np.array([0] + list(np.cumsum([len(f) for f in self.fields])) if self.digit_off is None else self.digit_off, dtype=np.uint64)
        args = [ffi.ptr(idx), ffi.ptr(data), ffi.ptr(off)] + [C.c_void_p(p) for p in self.dev]
        if self.null is not None:
            args[self.null] = None
        L = ffi.lib()
        rc = L.sg_mst_update_dev(args[0], args[1], args[2], len(self.idx), self.depth, self.nc, args[3], args[4], args[5], args[6], None)
        return rc, L.sg_last_error().decode()


@pytest.mark.parametrize("which", range(7))
def test_refuses_each_null_pointer(which):
    c = Call()
    c.null = which
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "sg_mst_update: null argument" in msg


def test_refuses_bad_sizes_and_aliased_balances():
    for change in ({"depth": 31}, {"nc": 0}, {"nc": 65}):
        c = Call()
        for k, val in change.items():
            setattr(c, k, val)
        rc, msg = c.run()
        assert rc == SG_ERR_INVALID and "sg_mst_update: bad size" in msg, change
    c = Call()
    c.dev[3] = c.dev[1]
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "d_leaf_balances overlaps d_node_balances" in msg
    c = Call()
    c.dev[1] = c.dev[3] + 32 * 2 * 6                         # the root's row of the node balances: the last 64 of 448 bytes
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "d_leaf_balances overlaps d_node_balances" in msg


REFUSALS = [
    ({"idx": [], "fields": []}, "no leaf to update"),
    ({"idx": [0, 1, 2, 3, 3], "fields": [b"1"] * 10}, "more leaves to update than the tree has"),
    ({"idx": [1, 4]}, "leaf index 4 at position 1 is out of range"),
    ({"idx": [1, 0xffffffff]}, "leaf index 4294967295 at position 1 is out of range"),
    ({"idx": [3, 3]}, "leaf indices do not strictly increase at position 1"),
    ({"idx": [3, 1]}, "leaf indices do not strictly increase at position 1"),
    ({"fields": [b"1", b"22", b"", b"0"]}, "balance field 2 is empty"),
    ({"fields": [b"1", b"22", b"3 3", b"0"]}, "balance field 2 is not a decimal number"),
    ({"fields": [b"-1", b"22", b"333", b"0"]}, "balance field 0 is not a decimal number"),
    ({"digit_off": [0, 1, 3, 2, 7]}, "digit_off decreases at field 2"),
    ({"digit_off": [1, 1, 3, 6, 7]}, "digit_off[0] is not 0"),
]


@pytest.mark.parametrize("change,want", REFUSALS, ids=[w.replace(" ", "_") + f"_{i}" for i, (_, w) in enumerate(REFUSALS)])
def test_refuses_what_the_plan_refuses_and_says_why(change, want):
    c = Call()
    for k, val in change.items():
        setattr(c, k, val)
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and msg.endswith("sg_mst_update: " + want), msg


def test_the_entry_point_is_declared_everywhere():
    L = C.CDLL(ffi.library_path())
    assert hasattr(L, "sg_mst_update_dev")
    assert "sg_mst_update_dev" in ffi.EXPORTS and len(ffi.ARGTYPES["sg_mst_update_dev"]) == 11
    assert ffi.lib().sg_mst_update_dev.argtypes == ffi.ARGTYPES["sg_mst_update_dev"]
    assert ffi.lib().sg_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "summa_gpu.h")).read()
    decl = re.search(r"\bint\s+sg_mst_update_dev\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 11
    rust = open(os.path.join(ROOT, "integration", "halo2_gpu_shim", "src", "lib.rs")).read()
    assert re.search(r"pub fn sg_mst_update_dev\s*\(", rust)
    assert "`sg_mst_update_dev`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ============================================================================= the Python front end
ENTRIES = [("a", [1, 2]), ("b", [3, 4]), ("c", [5, 6]), ("d", [7, 8]), ("e", [9, 10])]


@pytest.fixture
def tree(monkeypatch):
    """a tree of 5 entries (depth 3) that was never on a device: `_update_dev` records its arguments, the root comes from a
    stand-in for the gather"""
    t = object.__new__(DeviceMerkleSumTree)
    t.depth, t.n_currencies = 3, 2
    t.entries = [(n, list(b)) for n, b in ENTRIES] + [(None, [0, 0])] * 3
    t.offsets = [0, 8, 12, 14]
    t._root = ("stale", "root")
    t.calls = []

    def record(self, indices, digit_bytes, digit_off):
        assert indices.dtype == np.uint32 and digit_off.dtype == np.uint64 and digit_bytes.dtype == np.uint8
        text = digit_bytes.tobytes()
        self.calls.append((indices.tolist(), [int(text[int(a):int(b)]) for a, b in zip(digit_off[:-1], digit_off[1:])]))
    monkeypatch.setattr(DeviceMerkleSumTree, "_update_dev", record)
    monkeypatch.setattr(DeviceMerkleSumTree, "_rows", lambda self, h, b, u: ([f"hash after {len(self.calls)}"], ["balances"], [], []))
    return t


def test_pack_balances_is_pack_entries_balance_half():
    flat = [0, 18446744073709551616, 11888, 41163, 7, 10 ** 89]
    digits, off = pack_balances(flat)
    _, _, want_digits, want_off = pack_entries([("x", flat[:2]), ("y", flat[2:4]), ("z", flat[4:])], 2)
    assert digits.tobytes() == want_digits.tobytes() == "".join(map(str, flat)).encode() and off.tolist() == want_off.tolist()
    assert off.dtype == np.uint64 and digits.dtype == np.uint8


def test_update_leaves_sorts_by_index_and_keeps_the_last_of_a_repeated_name(tree):
    root = tree.update_leaves([("d", [70, 80]), ("a", [10, 20]), ("d", [71, 81]), ("c", [50, 60]), ("a", [11, 21])])
    assert tree.calls == [([0, 2, 3], [11, 21, 50, 60, 71, 81])]
    assert root == ("hash after 1", "balances")               # the cached root was dropped
    assert tree.entries[:5] == [("a", [11, 21]), ("b", [3, 4]), ("c", [50, 60]), ("d", [71, 81]), ("e", [9, 10])]
    assert tree.entries[5:] == [(None, [0, 0])] * 3


def test_update_leaf_is_update_leaves_of_one(tree):
    assert tree.update_leaf("e", [0, 1 << 70]) == ("hash after 1", "balances")
    assert tree.calls == [([4], [0, 1 << 70])] and tree.entries[4] == ("e", [0, 1 << 70])


def test_update_leaves_at_takes_padded_rows_and_repeated_indices(tree):
    tree.update_leaves_at([7, 1, 7], [[1, 1], [2, 2], [3, 3]])
    assert tree.calls == [([1, 7], [2, 2, 3, 3])]
    assert tree.entries[1] == ("b", [2, 2]) and tree.entries[7] == (None, [3, 3])
    tree.entries = None                                       # a tree built from field elements
    tree.update_leaves_at(np.array([6], dtype=np.uint32), [np.array([4, 5], dtype=np.uint64)])
    assert tree.calls[1:] == [([6], [4, 5])] and tree.entries is None
    with pytest.raises(KeyError, match="Username not found"):
        tree.update_leaf("a", [1, 2])
    assert len(tree.calls) == 2


def test_a_refused_batch_changes_nothing(tree):
    before = [(n, list(b)) for n, b in tree.entries]
    good = ("a", [10, 20])
    with pytest.raises(KeyError, match="Username not found"):
        tree.update_leaves([good, ("nobody", [1, 2])])
    with pytest.raises(KeyError, match="Username not found"):
        tree.update_leaf("nobody", [1, 2])
    with pytest.raises(ValueError, match="^wrong number of balances$"):
        tree.update_leaves([good, ("b", [1])])
    with pytest.raises(ValueError, match="^wrong number of balances$"):
        tree.update_leaf("b", [1, 2, 3])
    with pytest.raises(ValueError, match="^Invalid balance$"):
        tree.update_leaves([good, ("b", [1, -2])])
    for bad in (-1, 8):
        with pytest.raises(IndexError, match="^Index out of bounds$"):
            tree.update_leaves_at([0, bad], [[1, 2], [3, 4]])
    with pytest.raises(ValueError):
        tree.update_leaves_at([0, 1], [[1, 2]])
    assert tree.calls == [] and tree.entries == before and tree._root == ("stale", "root")
    assert tree.update_leaves([]) == ("stale", "root") and tree.calls == []      # nothing to do
