"""The range audit of a device-resident tree without a GPU: the rules of csrc/mst_audit.h, whose text the kernels compile, run by the
header's own serial steps in tests/cpp/mst_audit_check.cpp (built by the host compiler under address / undefined sanitizers, a
process of its own) and compared with the integer model of mst_audit_cases.py, with the witness program's own list of range
checks (witness_cases.range_checked) and with MockProver.  And the exports of include/summa_snapshot.h, what the two entry points
refuse before they touch a device, and prove_batch(audit=...) with stand-in provers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mst_audit_cases as cases
import poly_cases as pc
import witness_cases as wc
from circuits_halo2_amd import batch as B, ffi
from circuits_halo2_amd.merkle_sum_tree import RangeAudit, range_check_text

SG_ERR_INVALID = -1
OVERFLOW, PLAIN = os.path.join(GOLDEN, "entry_16_overflow.csv"), os.path.join(GOLDEN, "entry_16.csv")
# entry_16_overflow.csv, n_bytes = 8: user 0's first balance is 2^112, so the leaf and its four ancestors are out of range
OVERFLOW_MASKS = [0b00001, 0b00010] + [0b00100] * 2 + [0b01000] * 4 + [0b10000] * 8


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_audit") / "mst_audit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_audit_check.cpp"), "-o", out])
    return out


def ask(exe, lines):
    """command lines -> the program's output lines, split into words"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def audit(exe, levels, n_bytes, bad_cap):
    """the header's serial steps over a tree [level][node][currency] -> the shape of cases.model"""
    depth, nc = len(levels) - 1, len(levels[0][0])
    values = " ".join(format(v, "x") for v in cases.level_major(levels))
    out = ask(exe, [f"audit {depth} {nc} {n_bytes} {bad_cap} {values}"])
    assert [w[0] for w in out] == ["flags", "masks", "bad", "summary"]
    return {w[0]: [int(x) for x in w[1:]] for w in out}


def test_the_model_speaks_of_the_same_field_and_geometry(exe):
    assert cases.R == pc.R == wc.R and cases.MONT == pc.MONT % pc.R
    assert ask(exe, ["geometry"]) == [["geometry", str(cases.THREADS), str(cases.TILE), str(cases.GROUP)]]
    tiles = (1 << cases.GROUPS_DEPTH) // cases.TILE
    assert cases.GROUPS_DEPTH <= 16 and tiles > cases.GROUP                      # more than one workgroup of the groups step


def test_predicate_for_every_n_bytes(exe):
    asked = [(n_bytes, v) for n_bytes in range(1, 32) for v in cases.predicate_values(n_bytes)]
    got = ask(exe, [f"pred {n_bytes} {v:x}" for n_bytes, v in asked])
    assert [int(w[1]) for w in got] == [int(v < cases.top_of(n_bytes)) for n_bytes, v in asked]
    assert {n_bytes for n_bytes, _ in asked} >= {1, 3, 5, 31, 4, 8}             # top inside a word, and at a word boundary


@pytest.mark.parametrize("kind", wc.TREE_KINDS)
@pytest.mark.parametrize("cfg", wc.witness_configs(), ids=lambda c: f"levels{c.levels}-nc{c.nc}-bytes{c.n_bytes}")
def test_flags_and_masks_are_the_circuits_own_range_checks(exe, cfg, kind):
    tree = wc.witness_tree(cfg.levels, cfg.nc, kind, cfg.n_bytes)
    top = cases.top_of(cfg.n_bytes)
    got = audit(exe, tree.node_bal, cfg.n_bytes, 1 << cfg.levels)
    nodes = [node for level in tree.node_bal for node in level]
    assert [f != 0 for f in got["flags"]] == [any(v >= top for v in node) for node in nodes]
    assert all(f == 0 or (node[f - 1] >= top and all(v < top for v in node[:f - 1])) for f, node in zip(got["flags"], nodes))
    for idx in range(1 << cfg.levels):
        checked = [v for _, v in wc.range_checked(cfg, tree, idx)]
        assert len(checked) == cfg.nc * (cfg.levels + 1)
        assert (got["masks"][idx] != 0) == any(v >= top for v in checked), idx
    assert got == cases.model(tree.node_bal, cfg.n_bytes, 1 << cfg.levels)
    if kind == "in_range":
        assert not any(got["flags"]) and not any(got["masks"]) and got["bad"] == [] and got["summary"] == [0, 0, 0, 0]
    else:
        assert any(got["masks"])


def test_the_overflow_csv_and_the_plain_one(exe):
    got = audit(exe, cases.csv_levels(OVERFLOW), 8, 16)
    assert got["masks"] == OVERFLOW_MASKS and got["bad"] == list(range(16))
    assert got["summary"] == [5, 16, 16, 1]                                      # the leaf and its four ancestors; the root: currency 0
    assert [i for i, f in enumerate(got["flags"]) if f] == [0, 16, 24, 28, 30] and set(got["flags"]) == {0, 1}
    plain = audit(exe, cases.csv_levels(PLAIN), 8, 16)
    assert not any(plain["flags"]) and not any(plain["masks"]) and plain["bad"] == [] and plain["summary"] == [0, 0, 0, 0]


def _range_check_failures(failures):
    """what MockProver reports of a failed range check: a lookup failure, or -- the reference's own form of an overflow
    (circuits/tests.rs:268-299, test_mock_prover_cpu.py) -- the broken copy of the last running sum to the constant 0, located
    in the range check's region"""
    out = []
    for f in failures:
        where = f[2]
        in_check = where[0] == "InRegion" and where[1][1] == "assign value to perform range check"
        if f[0] == "Lookup" or (f[0] == "Permutation" and in_check):
            out.append(f)
    return out


@pytest.mark.parametrize("name,user", [("entry_16_overflow.csv", 0), ("entry_16_overflow.csv", 1), ("entry_16_overflow.csv", 2),
                                       ("entry_16_overflow.csv", 8), ("entry_16.csv", 0)])
def test_mock_prover_fails_a_range_check_exactly_where_the_mask_says(exe, name, user):
    from circuits_halo2_amd.mock_prover import MockProver
    from test_mock_prover_cpu import K, _circuit, _instances
    mask = audit(exe, cases.csv_levels(os.path.join(GOLDEN, name)), 8, 16)["masks"][user]
    circuit = _circuit(name, user)
    failures = MockProver.run(K, circuit, _instances(circuit)).verify()
    assert (len(_range_check_failures(failures)) != 0) == (mask != 0), failures
    # one range check per bit of the mask fails, and nothing else is wrong with the circuit
    assert len(_range_check_failures(failures)) == bin(mask).count("1")
    if mask == 0:
        assert failures == []


def test_the_list_is_ordered_and_the_cap_cuts_it(exe):
    depth, nc, n_bytes = 8, 2, 8
    top = cases.top_of(n_bytes)
    spots = (3, 62, 64, 129, 200, 255)                         # top beside r - top: the parent's sum is 0, the harm stays with the pair
    plant = [(i, i % nc, top) for i in spots] + [(i ^ 1, i % nc, cases.R - top) for i in spots]
    levels = cases.planted(depth, nc, n_bytes, plant)
    full = cases.model(levels, n_bytes, 1 << depth)
    count = full["summary"][1]
    assert full["bad"] == sorted(set(spots) | {i ^ 1 for i in spots}) and count == 12 and full["summary"][0] == 12
    for cap in (0, 1, count, count + 5):
        got = audit(exe, levels, n_bytes, cap)
        assert got["bad"] == full["bad"][:cap] == sorted(got["bad"])
        assert got["summary"] == [full["summary"][0], count, min(cap, count), full["summary"][3]]
        assert got["flags"] == full["flags"] and got["masks"] == full["masks"]


@pytest.mark.parametrize("depth", [0, 1, 6, 7, 11])
def test_synthetic_cases_agree_with_the_model(exe, depth):
    """the GPU test's cases at the depths the host affords, every plant and cap, through the serial steps"""
    for nc, n_bytes in ((1, 1), (2, 5), (3, 8), (4, 31)):
        for name, plant, caps in cases.plants(depth, nc, n_bytes):
            levels = cases.planted(depth, nc, n_bytes, plant)
            for cap in caps:
                cap = (1 << depth) if cap is None else cap
                assert audit(exe, levels, n_bytes, cap) == cases.model(levels, n_bytes, cap), (name, nc, n_bytes, cap)


def test_the_groups_depth_spans_two_groups(exe):
    depth, nc, n_bytes = cases.GROUPS_DEPTH, 1, 8
    assert ask(exe, [f"scratch {depth}"]) == [["scratch", str(4 * (4 + 512 + 2)), "512", "2"]]
    name, plant, caps = [p for p in cases.plants(depth, nc, n_bytes) if p[0] == "edges"][0]
    assert {16383, 16384} <= {leaf for leaf, _, _ in plant}
    levels = cases.planted(depth, nc, n_bytes, plant)
    cap = 1 << depth
    assert audit(exe, levels, n_bytes, cap) == cases.model(levels, n_bytes, cap)


def audits(exe, asked):
    """audit() for [(levels, n_bytes, bad_cap)] in one run of the program"""
    lines = []
    for levels, n_bytes, bad_cap in asked:
        values = " ".join(format(v, "x") for v in cases.level_major(levels))
        lines.append(f"audit {len(levels) - 1} {len(levels[0][0])} {n_bytes} {bad_cap} {values}")
    out = ask(exe, lines)
    assert [w[0] for w in out] == ["flags", "masks", "bad", "summary"] * len(asked)
    return [{w[0]: [int(x) for x in w[1:]] for w in out[4 * k:4 * k + 4]} for k in range(len(asked))]


def test_the_geometry_past_64_groups():
    """what the sparse depths and BIG are for: a wave sums LANES group totals a trip"""
    assert (cases.LANES, cases.GROUP_ROWS, cases.TRIP_ROWS) == (64, cases.TILE * cases.GROUP, 64 * 16384) and cases.TRIP_ROWS == 1 << 20
    assert cases.BIG == 65 * cases.GROUP_ROWS + 2 == 1_064_962
    group = lambda item: item // cases.GROUP_ROWS           # the groups before an item's own are 0 .. group - 1
    trips = lambda item: -(-group(item) // cases.LANES)
    assert [trips(cases.BIG - 3), trips(cases.BIG - 2), trips(cases.BIG - 1)] == [1, 2, 2] and group(cases.BIG - 3) == cases.LANES
    assert trips(cases.TRIP_ROWS - 1) == trips(cases.TRIP_ROWS) == 1 and group(cases.TRIP_ROWS) == cases.LANES
    assert {d: (1 << d) // cases.GROUP_ROWS for d in cases.SPARSE_DEPTHS} == {16: 4, 20: 64, 21: 128}
    assert trips((1 << 20) - 1) == 1 and trips((1 << 21) - 1) == 2
    for depth in cases.SPARSE_DEPTHS:
        spots, groups = cases.sparse_spots(depth), (1 << depth) // cases.GROUP_ROWS
        per_group = [sum(1 for i in spots if group(i) == g) for g in range(groups)]
        assert all(per_group) and all(x != y for x, y in zip(per_group, per_group[1:]))
        for g in {0, 63, 64, 65, groups - 1} & set(range(groups)):
            assert {g * cases.GROUP_ROWS, (g + 1) * cases.GROUP_ROWS - 1} <= set(spots), (depth, g)
        assert len({i >> 1 for i in spots}) == len(spots)
        caps = [c[2] for c in cases.sparse_plants(depth, 8)]
        assert caps[0][3] == 2 * len(spots) and caps[1][3] == 1 << depth
        if depth == 21:
            assert caps[0][5] == 2 * sum(per_group[:65]) + 1 and caps[1][5] == 65 * cases.GROUP_ROWS + 1 == cases.BIG - 1


def _same_as_model(sparse, want, what):
    assert {k: (v if k == "summary" else v.tolist()) for k, v in sparse.items()} == want, what


@pytest.mark.parametrize("depth", [0, 1, 6, 7, 8, 11])
def test_the_sparse_model_is_the_model(depth):
    """key for key on every plant and cap of the dense family (its trees given as their non-zero nodes), and on the sparse
    plants at these depths, whose nodes sparse_nodes computes: the tree of zeros with the plant, built densely, has the same"""
    for nc, n_bytes in ((1, 1), (2, 5), (3, 8), (4, 31)):
        for name, plant, caps in cases.plants(depth, nc, n_bytes):
            levels = cases.planted(depth, nc, n_bytes, plant)
            for cap in caps:
                _same_as_model(cases.sparse_model(depth, n_bytes, cases.nonzero_nodes(levels), cap),
                               cases.model(levels, n_bytes, (1 << depth) if cap is None else cap), (name, nc, n_bytes, cap))
        for name, plant, caps in cases.sparse_plants(depth, n_bytes) + cases.plants(depth, nc, n_bytes):
            zeros = [[0] * nc for _ in range(1 << depth)]
            for leaf, c, v in plant:
                zeros[leaf][c] = v
            levels = cases.levels_of(zeros)
            nodes = cases.sparse_nodes(depth, nc, plant)
            assert nodes == cases.nonzero_nodes(levels), (name, nc, n_bytes)
            assert np.array_equal(cases.sparse_bytes(depth, nc, nodes), cases.mont_bytes(cases.level_major(levels))), (name, nc)
            full = cases.sparse_model(depth, n_bytes, nodes)
            for cap in caps:
                want = cases.model(levels, n_bytes, (1 << depth) if cap is None else cap)
                _same_as_model(cases.sparse_model(depth, n_bytes, nodes, cap), want, (name, nc, n_bytes, cap))
                _same_as_model(cases.cut(full, cap), want, (name, nc, n_bytes, cap))


def test_the_mirror_agrees_with_the_sparse_model_at_four_groups(exe):
    """depth 16, the sparse plants written out densely for the check program"""
    depth, nc, n_bytes = 16, 1, cases.SPARSE_N_BYTES
    for name, plant, caps in cases.sparse_plants(depth, n_bytes):
        nodes = cases.sparse_nodes(depth, nc, plant)
        values = [["0"] * (1 << (depth - level)) for level in range(depth + 1)]
        for level, some in enumerate(nodes):
            for i, b in some.items():
                values[level][i] = format(b[0], "x")
        text = " ".join(v for level in values for v in level)
        full = cases.sparse_model(depth, n_bytes, nodes)
        assert full["summary"][1] == caps[3] > 1
        for cap in (1 << depth, caps[4]):
            out = ask(exe, [f"audit {depth} {nc} {n_bytes} {cap} {text}"])
            got = {w[0]: np.array([int(x) for x in w[1:]], dtype=np.uint64) for w in out}
            want = cases.cut(full, cap)
            assert got["summary"].tolist() == want["summary"], (name, cap)
            for key in ("flags", "masks", "bad"):
                assert np.array_equal(got[key], want[key]), (name, cap, key)


@pytest.mark.parametrize("nc", cases.MANY_CURRENCIES)
def test_many_currencies_agree_with_the_model_and_straddle_the_words(exe, nc):
    """the plants that test_gpu_mst_audit.py adds for the flags kernel's bit gather, through the serial steps; and where they
    put their bits in the workgroup's bit string: thread t of a workgroup is node t, its field bits t * nc .. t * nc + nc - 1"""
    asked, wants, flags_seen, straddling = [], [], set(), set()
    for depth in cases.MANY_DEPTHS:
        for n_bytes in cases.MANY_N_BYTES:
            for name, plant, caps in cases.many_currency_plants(depth, nc, n_bytes):
                levels = cases.planted(depth, nc, n_bytes, plant)
                for cap in caps:
                    cap = (1 << depth) if cap is None else cap
                    asked.append((levels, n_bytes, cap))
                    wants.append(cases.model(levels, n_bytes, cap))
                flags = wants[-1]["flags"]
                flags_seen |= set(flags)
                top = cases.top_of(n_bytes)
                for node, balances in enumerate(b for level in levels for b in level):
                    sh = (node % cases.THREADS) * nc % 64
                    straddling |= {(c < 64 - sh) for c, v in enumerate(balances) if v >= top and sh + nc > 64}
                if name == "every currency at every leaf":
                    assert all(v >= top for b in levels[0] for v in b) and set(flags[:1 << depth]) == {1}
    assert audits(exe, asked) == wants
    assert flags_seen >= {0, 1, nc - 1, nc} | ({32, 33} & set(range(nc + 1)))
    # out-of-range bits on both sides of a word's edge within one node's field -- or no field that crosses an edge at all
    assert straddling == (set() if nc == 64 else {True, False})
    assert [cases.straddling_leaf(256, n, n - 1) for n in cases.MANY_CURRENCIES] == [12, 1, 1, 256 // 3]


# ============================================================================= the entry points: exports, scratch, refusals
def test_exports_are_the_headers_prototypes():
    text = open(os.path.join(ROOT, "include", "summa_snapshot.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(ss_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = [name for name, _ in protos]
    assert names == ffi.SNAPSHOT_EXPORTS and names[-2:] == ["ss_mst_range_audit_scratch", "ss_mst_range_audit_dev"]
    L = ffi.snapshot_lib()
    for name, args in protos[-2:]:
        getattr(L, name)
        assert len(ffi.SNAPSHOT_ARGTYPES[name]) == len(args.split(",")), name
    assert len(ffi.SNAPSHOT_ARGTYPES["ss_mst_range_audit_dev"]) == 11


def test_scratch_size_is_the_headers_formula(exe):
    L = ffi.snapshot_lib()
    size = C.c_uint64(77)
    assert L.ss_mst_range_audit_scratch(31, C.byref(size)) == SG_ERR_INVALID and size.value == 77
    assert L.ss_mst_range_audit_scratch(5, None) == SG_ERR_INVALID
    depths = list(range(0, 31))
    program = ask(exe, [f"scratch {d}" for d in depths])
    for d, words in zip(depths, program):
        assert L.ss_mst_range_audit_scratch(d, C.byref(size)) == 0
        tiles = -(-(1 << d) // 64)
        groups = -(-tiles // 256)
        assert size.value == 4 * (4 + tiles + groups) == int(words[1]), d


def range_audit(**change):
    """a good call but for `change`; the device pointers are not memory: a refused call never uses them"""
    a = dict(bal=0x100000, depth=4, nc=2, n_bytes=8, flags=0x200000, reasons=0x300000, bad=0x400000, cap=16, scratch=0x500000, out=True)
    a.update(change)
    summary = (C.c_uint64 * 4)(71, 72, 73, 74)
    rc = ffi.snapshot_lib().ss_mst_range_audit_dev(a["bal"], a["depth"], a["nc"], a["n_bytes"], a["flags"], a["reasons"], a["bad"], a["cap"],
                                                   a["scratch"], summary if a["out"] else None, None)
    assert list(summary) == [71, 72, 73, 74]
    return rc, ffi.lib().sg_last_error().decode()


def test_range_audit_refuses_bad_arguments(exe):
    refused = [({"bal": None}, "null"), ({"flags": None}, "null"), ({"reasons": None}, "null"), ({"scratch": None}, "null"),
               ({"out": False}, "null"), ({"depth": 31}, "depth above 30"), ({"nc": 0}, "n_currencies"), ({"nc": 65}, "n_currencies"),
               ({"n_bytes": 0}, "n_bytes"), ({"n_bytes": 32}, "n_bytes"), ({"reasons": 0x300002}, "d_leaf_reasons"),
               ({"bad": 0x400001}, "d_bad_leaves"), ({"bad": None}, "d_bad_leaves"), ({"bad": None, "cap": 1 << 40}, "d_bad_leaves")]
    for change, word in refused:
        rc, msg = range_audit(**change)
        assert rc == SG_ERR_INVALID and msg.startswith("ss_mst_range_audit: ") and word in msg, (change, msg)
    # the same words from the header's own function, and "" for what the entry point accepts (a null list with bad_cap == 0)
    ptr = lambda v: 0 if v is None else v
    def problem(**change):
        a = dict(bal=0x100000, depth=4, nc=2, n_bytes=8, flags=0x200000, reasons=0x300000, bad=0x400000, cap=16, scratch=0x500000, out=0x600000)
        a.update(change)
        line = " ".join(str(ptr(a[k])) for k in ("bal", "depth", "nc", "n_bytes", "flags", "reasons", "bad", "cap", "scratch", "out"))
        return " ".join(ask(exe, ["problem " + line])[0][1:])
    assert problem() == "" and problem(bad=None, cap=0) == "" and problem(depth=30, nc=64, n_bytes=31) == ""
    for change, word in refused:
        change = {k: (0 if v is False else v) for k, v in change.items()}
        assert word in problem(**change), change


# ============================================================================= prove_batch(audit=...)
def _hand_made_audit():
    """a tree of 16 leaves, two currencies: leaf 5's second balance and node 1 of level 2 (first currency) out of range"""
    flags = np.zeros(31, dtype=np.uint8)
    flags[5], flags[24 + 1] = 2, 1
    masks = np.zeros(16, dtype=np.uint32)
    masks[5], masks[4] = 0b00001, 0b00010
    masks[0:4] = 0b01000                                       # their sibling at level 2 is node 1
    return RangeAudit(8, 2, 6, [0, 1, 2, 3, 4, 5], 0, flags, masks)


def test_prove_batch_files_flagged_users_without_calling_the_provers():
    audit_ = _hand_made_audit()
    assert not audit_.ok and audit_.root_in_range and audit_.root_currency is None and audit_.depth == 4
    assert list(audit_.reasons([5, 4, 0, 9])) == [1, 2, 8, 0]
    made, proved = [], []
    make_circuit = lambda i: made.append(i) or i
    def prove(c):
        proved.append(c)
        return (b"proof-%d" % c, [c])
    users = [0, 3, 4, 5, 6, 9, 15]
    res = B.prove_batch(None, users, None, None, levels=4, in_flight=1, prove=prove, make_circuit=make_circuit, audit=audit_)
    assert res.errors == {0: "range check: sibling at level 2, currency 0", 3: "range check: sibling at level 2, currency 0",
                          4: "range check: sibling at level 0, currency 1", 5: "range check: leaf, currency 1"}
    assert made == proved == [6, 9, 15] and sorted(res.proofs) == [6, 9, 15] and res.proofs[9] == (b"proof-9", [9])
    assert range_check_text(("sibling", 3, 1, 0)) == "range check: sibling at level 3, currency 0"
    # without an audit the stand-ins are called for everyone
    made.clear(), proved.clear()
    res = B.prove_batch(None, users, None, None, levels=4, in_flight=1, prove=prove, make_circuit=make_circuit)
    assert made == proved == users and not res.errors and sorted(res.proofs) == users
    # several in flight: the same split
    made.clear(), proved.clear()
    res = B.prove_batch(None, users, None, None, levels=4, in_flight=3, prove=prove, make_circuit=make_circuit, audit=audit_)
    assert sorted(made) == sorted(proved) == [6, 9, 15] and sorted(res.errors) == [0, 3, 4, 5]
    # an audit that flags nobody of the batch, and the root's flag alone, skip nobody
    clean = RangeAudit(8, 1, 0, [], 1, np.zeros(31, dtype=np.uint8), np.zeros(16, dtype=np.uint32))
    assert not clean.ok and clean.root_currency == 0
    made.clear(), proved.clear()
    res = B.prove_batch(None, users, None, None, levels=4, in_flight=1, prove=prove, make_circuit=make_circuit, audit=clean)
    assert made == users and not res.errors
