"""The next round's snapshot against a tree in HBM on the device (include/summa_rounds.h): every output of sr_mst_csv_diff_dev
against the model of mst_diff_cases.py on every case and cap, the tree after sr_mst_apply_diff_dev against a fresh tree of the same
leaves with the changed balances (bit for bit, the oracle's root at the small sizes, `from_csv` of the new file where the leaves
line up), the Python surface -- `diff_csv`, `apply_diff`, `apply_csv` and what the tree says of its entries afterwards, with no
host parse and no balance packed on the device way --, the host fallback, the stale diff, and the stream order of both entry
points with the helpers of test_gpu_stream_order.py.  The report and the apply once more at mst_diff_cases.BIG rows against the
numpy model: past 64 groups of the lists' compaction, where the scatter's sum of the group totals takes a second trip."""
import ctypes as C
import functools

import numpy as np
import pytest

import mst_diff_cases as cases
import stream_cases as sc

pytestmark = pytest.mark.gpu

CASES = cases.cases()
IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
FILL, GUARD = 0xEE, 0x5A
FILL32 = 0xEEEEEEEE


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{case name: (path of A, path of B)}"""
    d = tmp_path_factory.mktemp("mst_diff_gpu")
    return {c[0]: (cases.write_case(d, c[0] + ".a", cases.text_of(c[1], c[3])), cases.write_case(d, c[0] + ".b", cases.text_of(c[2], c[3])))
            for c in CASES}


@functools.lru_cache(maxsize=None)
def model_of(name):
    _, a, b, nc, sorted_tree = BY_NAME[name]
    return cases.model(a, b, nc, sorted_tree)


def capped(name, cap):
    m = model_of(name)
    return dict(m, new=m["new"][:cap], gone=m["gone"][:cap], summary=m["summary"][:6] + [min(cap, m["summary"][0]), min(cap, m["summary"][4])])


def tree_of(name, files):
    """T: the tree of the case's kind from A's file, read and indexed on the device"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    nc, sorted_tree = BY_NAME[name][3], BY_NAME[name][4]
    tree = DeviceMerkleSumTree.from_csv_sorted(files[name][0], nc) if sorted_tree else DeviceMerkleSumTree.from_csv(files[name][0], nc, name_index=True)
    assert tree.csv_ingest == "device" and tree.has_name_index
    return tree


def fresh_arrays(name):
    """the four arrays of a tree built from A's leaves in T's order with the changed balances, and its entries"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    _, a, b, nc, _ = BY_NAME[name]
    m = model_of(name)
    entries = [(a[r][0].decode(), [int(x) for x in a[r][1]]) for r in m["leaf_rows"]]
    for leaf, bal in zip(m["changed"], m["balances"]):
        entries[leaf] = (entries[leaf][0], bal)
    tree = DeviceMerkleSumTree.from_entries(entries, nc)
    return {what: getattr(tree, what).cpu().numpy() for what in ("d_users", "d_bals", "d_h", "d_b")}, entries, tree


def _guarded(n_bytes, fill=FILL):
    import torch
    t = torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    t[:n_bytes] = fill
    return t


def run_diff(tree, path_b, cap):
    """the new file's scan, then sr_mst_csv_diff_dev: every buffer it writes pre-filled with 0xEE and followed by 64 guard bytes
    that must come back untouched -> the outputs as lists, the summary, and what the apply takes"""
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    nc, depth = tree.n_currencies, tree.depth
    scanned, reason = DeviceMerkleSumTree._csv_text_on_device(path_b, nc)
    assert scanned is not None, reason
    text, size, body_off, delim, _, tiles, n = scanned
    R = ffi.rounds_lib()
    leaves = 1 << depth
    scratch = C.c_uint64(0)
    ffi.check(R.sr_mst_diff_scratch(n, depth, C.byref(scratch)))
    sizes = {"spans": 8 * (n + 2 + 2 * n * (1 + nc)), "row_leaf": 4 * n, "row_state": n, "leaf_state": leaves, "owner": 4 * leaves,
             "changed": 4 * min(n, leaves), "new": 4 * cap, "gone": 4 * cap, "scratch": scratch.value}
    b = {k: _guarded(v) for k, v in sizes.items()}
    t = tree._names_dev()
    problem, summary = C.c_uint64(77), (C.c_uint64 * 8)()
    ffi.check(R.sr_mst_csv_diff_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), ord(delim), nc, n, ffi.dev_ptr(b["spans"]),
                                    ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(t["d_name_spans"]),
                                    None if tree._sorted_dev is not None else ffi.dev_ptr(t["d_order"]), t["n"], depth, ffi.dev_ptr(tree.d_bals),
                                    ffi.dev_ptr(b["row_leaf"]), ffi.dev_ptr(b["row_state"]), ffi.dev_ptr(b["leaf_state"]), ffi.dev_ptr(b["owner"]),
                                    ffi.dev_ptr(b["changed"]), ffi.dev_ptr(b["new"]) if cap else None, ffi.dev_ptr(b["gone"]) if cap else None,
                                    cap, ffi.dev_ptr(b["scratch"]), C.byref(problem), summary, ffi.current_stream_ptr()))
    torch.cuda.current_stream().synchronize()
    assert problem.value == 0
    for k, used in sizes.items():
        assert (b[k][used:] == GUARD).all(), f"the bytes behind {k} changed"
    u32 = lambda k: b[k][:sizes[k]].cpu().numpy().view(np.uint32).tolist()
    u8 = lambda k: b[k][:sizes[k]].cpu().numpy().tolist()
    return {"row_leaf": u32("row_leaf"), "row_state": u8("row_state"), "leaf_state": u8("leaf_state"), "owner": u32("owner"),
            "changed": u32("changed"), "new": u32("new"), "gone": u32("gone"), "summary": [int(x) for x in summary], "n": n,
            "dev": {"text": text, "size": size, "body_off": body_off, "tiles": tiles, "delim": delim, "buffers": b}}


def _same(got, want, what):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} bytes, {w.size} expected"
    bad = (g.reshape(-1, 32) != w.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


# ============================================================================= the diff, through the C ABI
@pytest.mark.parametrize("name", IDS)
def test_every_output_of_the_diff_equals_the_model(gpu, files, name):
    tree = tree_of(name, files)
    m = model_of(name)
    assert (tree.depth, tree._names_dev()["n"]) == (m["depth"], m["n_tree"])
    for cap in cases.caps_of(m):
        got, want = run_diff(tree, files[name][1], cap), capped(name, cap)
        assert got["summary"] == want["summary"], (name, cap)
        for key in ("row_leaf", "row_state", "leaf_state", "owner"):
            assert got[key] == want[key], (name, cap, key)
        # the lists: the listed entries, and behind them the pre-fill
        n_changed = len(want["changed"])
        assert got["changed"][:n_changed] == want["changed"] and set(got["changed"][n_changed:]) <= {FILL32}, (name, cap)
        assert got["new"][:len(want["new"])] == want["new"] and set(got["new"][len(want["new"]):]) <= {FILL32}, (name, cap)
        assert got["gone"][:len(want["gone"])] == want["gone"] and set(got["gone"][len(want["gone"]):]) <= {FILL32}, (name, cap)


def test_a_file_outside_the_subset_is_reported_and_nothing_written(gpu, files, tmp_path):
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    name = "equal_65_file"
    tree = tree_of(name, files)
    text = cases.text_of(BY_NAME[name][2], 2).split("\n")
    text[8] = text[8] + ",5"                                  # file row 7: a field too many
    path = cases.write_case(tmp_path, "bad", "\n".join(text))
    text_d, size, body_off, delim, _, tiles, n = DeviceMerkleSumTree._csv_text_on_device(path, 2)[0]
    R = ffi.rounds_lib()
    scratch = C.c_uint64(0)
    ffi.check(R.sr_mst_diff_scratch(n, tree.depth, C.byref(scratch)))
    leaves = 1 << tree.depth
    sizes = {"row_leaf": 4 * n, "row_state": n, "leaf_state": leaves, "owner": 4 * leaves, "changed": 4 * n, "new": 16, "gone": 16}
    b = {k: _guarded(v) for k, v in sizes.items()}
    spans, work = _guarded(8 * (n + 2 + 2 * n * 3)), _guarded(scratch.value)
    t = tree._names_dev()
    problem, summary = C.c_uint64(0), (C.c_uint64 * 8)(*range(71, 79))
    ffi.check(R.sr_mst_csv_diff_dev(ffi.dev_ptr(text_d), size, body_off, ffi.dev_ptr(tiles), ord(delim), 2, n, ffi.dev_ptr(spans), ffi.dev_ptr(t["text"]),
                                    t["size"], t["body_off"], ffi.dev_ptr(t["d_name_spans"]), ffi.dev_ptr(t["d_order"]), t["n"], tree.depth,
                                    ffi.dev_ptr(tree.d_bals), ffi.dev_ptr(b["row_leaf"]), ffi.dev_ptr(b["row_state"]), ffi.dev_ptr(b["leaf_state"]),
                                    ffi.dev_ptr(b["owner"]), ffi.dev_ptr(b["changed"]), ffi.dev_ptr(b["new"]), ffi.dev_ptr(b["gone"]), 4,
                                    ffi.dev_ptr(work), C.byref(problem), summary, ffi.current_stream_ptr()))
    torch.cuda.synchronize()
    assert (problem.value >> 8, problem.value & 0xff) == (7, 3) and list(summary) == list(range(71, 79))
    for k, used in sizes.items():
        assert (b[k][:used] == FILL).all() and (b[k][used:] == GUARD).all(), k
    diff = tree.diff_csv(path)                                # the Python surface hands such a file to the host parser, which refuses it or not
    assert diff.ingest == "host" and diff.fallback_reason == "row 7: not n_currencies + 1 fields"


# ============================================================================= the apply
def apply_abi(tree, got):
    from circuits_halo2_amd import ffi
    import torch
    d = got["dev"]
    ffi.check(ffi.rounds_lib().sr_mst_apply_diff_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["buffers"]["spans"]), got["n"],
                                                     ffi.dev_ptr(d["buffers"]["owner"]), ffi.dev_ptr(d["buffers"]["changed"]), got["summary"][2],
                                                     tree.depth, tree.n_currencies, ffi.dev_ptr(tree.d_users), ffi.dev_ptr(tree.d_bals),
                                                     ffi.dev_ptr(tree.d_h), ffi.dev_ptr(tree.d_b), ffi.current_stream_ptr()))
    torch.cuda.current_stream().synchronize()


ORACLE_ROOTS = {f"{family}_{n}_{kind}" for n in (1, 2, 64, 65, 257) for family, kind in (("every_row_changed_shuffled", "file"), ("edges_changed", "sorted"))}
ORACLE_ROOTS |= {"twice_in_a_65_file", "field_equal_sorted", "three_currencies_65_file"}


@pytest.mark.parametrize("name", IDS)
def test_the_tree_after_the_apply_is_a_fresh_tree_of_the_changed_leaves(gpu, files, name):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, _mont_to_int
    _, a, b, nc, sorted_tree = BY_NAME[name]
    tree = tree_of(name, files)
    before = {what: getattr(tree, what).clone() for what in ("d_users", "d_bals", "d_h", "d_b")}
    got = run_diff(tree, files[name][1], 0)
    for what, t in before.items():
        assert (getattr(tree, what) == t).all(), f"the diff wrote {what}"
    apply_abi(tree, got)
    want, entries, _ = fresh_arrays(name)
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), want[what], f"{name}: {what}")
    if not model_of(name)["changed"]:
        for what, t in before.items():
            assert (getattr(tree, what) == t).all(), f"an apply of nothing wrote {what}"
    root_h = want["d_h"][-32:]
    a_names, b_names = [r[0] for r in a], [r[0] for r in b]
    if a_names == b_names and not sorted_tree:                # the leaves line up: the new file's own tree
        _same(DeviceMerkleSumTree.from_csv(files[name][1], nc).d_h.cpu().numpy()[-32:], root_h, f"{name}: from_csv of the new file")
    if sorted_tree and sorted(a_names) == sorted(b_names) and len(set(a_names)) == len(a_names):
        _same(DeviceMerkleSumTree.from_csv_sorted(files[name][1], nc).d_h.cpu().numpy()[-32:], root_h, f"{name}: from_csv_sorted of the new file")
    if name in ORACLE_ROOTS:
        from oracle import pyref as P
        assert len(a) <= 260
        (oracle_h, oracle_b), _ = P.mst_build([P.mst_entry(nm, bal) for nm, bal in entries])
        assert _mont_to_int(tree.root()[0]) == oracle_h
        assert [_mont_to_int(tree.root()[1][32 * c:32 * c + 32]) for c in range(nc)] == [v % P.R for v in oracle_b]


def test_the_oracle_list_is_in_the_cases():
    assert ORACLE_ROOTS <= set(IDS)


def test_the_apply_refuses_a_list_that_is_not_one(gpu, files):
    import torch
    from circuits_halo2_amd import ffi
    name = "edges_changed_257_file"
    tree = tree_of(name, files)
    got = run_diff(tree, files[name][1], 0)
    before = {what: getattr(tree, what).clone() for what in ("d_bals", "d_h", "d_b")}
    changed = got["dev"]["buffers"]["changed"]
    for bad, word in (([5, 5], "strictly increase"), ([9, 4], "strictly increase"), ([3, 512], "out of range")):
        changed[:8] = torch.from_numpy(np.array(bad, dtype=np.uint32).view(np.uint8)).cuda()
        with pytest.raises(ffi.SummaGpuError, match=word):
            apply_abi(tree, dict(got, summary=[0, 0, 2]))
    torch.cuda.synchronize()
    for what, t in before.items():
        assert (getattr(tree, what) == t).all(), what


# ============================================================================= the Python surface
def _counting(monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    parses, packs = [], []
    real_parse, real_pack = M.parse_csv_to_entries, M.pack_balances
    monkeypatch.setattr(M, "parse_csv_to_entries", lambda *a: parses.append(a) or real_parse(*a))
    monkeypatch.setattr(M, "pack_balances", lambda *a: packs.append(1) or real_pack(*a))
    return parses, packs


def _report_equals(diff, m, name):
    assert diff.summary() == dict(zip(cases.SUMMARY, m["summary"])), name
    assert diff.changed.tolist() == m["changed"] and diff.new_rows.tolist() == m["new"] and diff.gone.tolist() == m["gone"], name
    assert diff.row_leaf().tolist() == m["row_leaf"] and diff.row_state().tolist() == m["row_state"], name
    assert diff.leaf_state().tolist() == m["leaf_state"] and diff.owner().tolist() == m["owner"], name


SURFACE = ["edges_changed_shuffled_257_file", "edges_changed_shuffled_257_sorted", "new_names_65_sorted", "twice_in_a_65_file",
           "edges_gone_shuffled_65_file", "three_currencies_65_sorted", "field_equal_file"]


@pytest.mark.parametrize("name", SURFACE)
def test_diff_csv_apply_csv_and_the_entries_afterwards(gpu, files, name, monkeypatch):
    import torch
    from circuits_halo2_amd import merkle_sum_tree as M
    _, a, b, nc, _ = BY_NAME[name]
    m = model_of(name)
    want, entries, fresh = fresh_arrays(name)
    audit_want = fresh.range_audit()
    tree = tree_of(name, files)
    parses, packs = _counting(monkeypatch)
    diff = tree.diff_csv(files[name][1])
    assert diff.ingest == "device" and diff.fallback_reason is None and isinstance(diff._arrays["owner"], torch.Tensor)
    _report_equals(diff, m, name)
    assert tree.diff_csv(files[name][1], cap=1).summary()["new_listed"] == min(1, m["summary"][0])
    assert tree.apply_csv(files[name][1]).summary() == diff.summary()
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), want[what], f"{name}: {what}")
    _same(tree.root()[0], want["d_h"][-32:], f"{name}: root()")
    again = tree.diff_csv(files[name][1])
    assert again.n_changed == 0 and again.changed.size == 0 and again.n_same == m["summary"][2] + m["summary"][3] and again.n_new == diff.n_new
    assert tree.apply_diff(again)[0].tolist() == tree.root()[0].tolist()
    for leaf in m["changed"][:3] + m["changed"][-2:]:
        assert tree.get_entry(leaf) == entries[leaf], (name, leaf)
        proof = tree.generate_proof(leaf)
        assert proof["entry"] == entries[leaf] and tree.verify_proof(proof), (name, leaf)
    audit = tree.range_audit()
    assert (audit.n_bad_nodes, audit.n_unprovable, audit.unprovable.tolist()) == (audit_want.n_bad_nodes, audit_want.n_unprovable,
                                                                                  audit_want.unprovable.tolist())
    assert torch.equal(audit.d_leaf_reasons, audit_want.d_leaf_reasons) and torch.equal(audit.d_node_flags, audit_want.d_node_flags)
    assert parses == [] and packs == [], "the device way parsed a file or packed a balance on the host"
    if m["changed"]:                                          # a later update by name finds the user and starts from the new balances
        leaf = m["changed"][0]
        bumped = [v + 9 for v in entries[leaf][1]]
        tree.update_leaves([(entries[leaf][0], bumped)])
        assert parses == [] and tree.get_entry(leaf) == (entries[leaf][0], bumped)
        assert tree.get_entry(m["changed"][-1]) == entries[m["changed"][-1]] or leaf == m["changed"][-1]
        fresh.update_leaves_at([leaf], [bumped])
        _same(tree.d_h.cpu().numpy(), fresh.d_h.cpu().numpy(), f"{name}: hashes after a later update by name")
        entries[leaf] = (entries[leaf][0], bumped)
    got = tree.entries                                        # now the tree's own file is parsed, once, and shows the new balances
    assert len(parses) == 1 and got[:len(entries)] == entries and tree.get_entry(len(entries) - 1) == entries[-1]


def test_the_host_fallback_gives_the_same_report_with_a_reason(gpu, files, tmp_path):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    name = "edges_changed_shuffled_257_file"
    _, a, b, nc, _ = BY_NAME[name]
    m = model_of(name)
    want, entries, _ = fresh_arrays(name)
    plain = DeviceMerkleSumTree.from_csv(files[name][0], nc)  # no name index
    diff = plain.diff_csv(files[name][1])
    assert diff.ingest == "host" and diff.fallback_reason == "the tree holds no name index"
    _report_equals(diff, m, name)
    plain.apply_diff(diff)
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(plain, what).cpu().numpy(), want[what], f"{name}: {what} after a host diff")
    assert plain.diff_csv(files[name][1]).n_changed == 0 and [plain.get_entry(i) for i in m["changed"]] == [entries[i] for i in m["changed"]]
    # an indexed tree and a file the device reader does not take: a quoted name
    quoted = cases.text_of(b, nc).replace(b[5][0].decode() + ",", '"' + b[5][0].decode() + '",', 1)
    path = cases.write_case(tmp_path, "quoted", quoted)
    tree = tree_of(name, files)
    diff = tree.diff_csv(path)
    assert diff.ingest == "host" and diff.fallback_reason == "a quote, NUL or non-ASCII byte"
    _report_equals(diff, m, name)
    tree.apply_diff(diff)
    _same(tree.d_h.cpu().numpy(), want["d_h"], f"{name}: hashes after a host diff of an indexed tree")


def test_a_stale_diff_is_refused_with_the_tree_untouched(gpu, files):
    name = "edges_changed_shuffled_257_sorted"
    tree, other = tree_of(name, files), tree_of(name, files)
    diff = tree.diff_csv(files[name][1])
    with pytest.raises(ValueError, match="another tree"):
        other.apply_diff(diff)
    tree.update_leaves_at([7], [[1, 2]])
    before = {what: getattr(tree, what).clone() for what in ("d_users", "d_bals", "d_h", "d_b")}
    with pytest.raises(ValueError, match="before another update"):
        tree.apply_diff(diff)
    for what, t in before.items():
        assert (getattr(tree, what) == t).all(), what
    tree.apply_diff(tree.diff_csv(files[name][1]))            # a diff of the tree as it is now goes through, leaf 7 included
    want, _, _ = fresh_arrays(name)
    _same(tree.d_h.cpu().numpy(), want["d_h"], name)
    with pytest.raises(ValueError, match="before another update"):
        tree.apply_diff(diff)


def test_the_apply_on_a_stream_of_the_callers(gpu, files):
    import torch
    name = "every_row_changed_shuffled_16386_file"
    tree = tree_of(name, files)
    want, _, _ = fresh_arrays(name)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        diff = tree.apply_csv(files[name][1])
    torch.cuda.synchronize()
    assert diff.n_changed == 16386 and diff.ingest == "device"
    for what in ("d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), want[what], f"{name}: {what}")


# ============================================================================= past 64 groups of the lists' compaction
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """{sorted_tree: the big case, with the paths of its files under "paths"}: A, B1 and, for the tree in file order, B2"""
    d = tmp_path_factory.mktemp("mst_diff_big")
    out = {}
    for sorted_tree in (False, True):
        case = cases.big_case(sorted_tree)
        kind = "sorted" if sorted_tree else "file"
        case["paths"] = {k: cases.write_big(d / f"{kind}.{k}.csv", *case[k]) for k in (("a", "b1") if sorted_tree else ("a", "b1", "b2"))}
        out[sorted_tree] = case
    return out


def big_tree(case, sorted_tree):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    path = case["paths"]["a"]
    tree = DeviceMerkleSumTree.from_csv_sorted(path, cases.BIG_NC) if sorted_tree else DeviceMerkleSumTree.from_csv(path, cases.BIG_NC, name_index=True)
    assert tree.csv_ingest == "device" and tree.has_name_index and (tree.depth, tree._names_dev()["n"]) == (21, cases.BIG)
    return tree


def run_diff_np(tree, scanned, cap):
    """run_diff over a file scanned once, for the sizes where lists of Python integers cost too much: the same call over buffers
    pre-filled and guarded in the same way, every output whole as a numpy array"""
    import torch
    from circuits_halo2_amd import ffi
    nc, depth = tree.n_currencies, tree.depth
    text, size, body_off, delim, _, tiles, n = scanned
    R = ffi.rounds_lib()
    leaves = 1 << depth
    scratch = C.c_uint64(0)
    ffi.check(R.sr_mst_diff_scratch(n, depth, C.byref(scratch)))
    sizes = {"spans": 8 * (n + 2 + 2 * n * (1 + nc)), "row_leaf": 4 * n, "row_state": n, "leaf_state": leaves, "owner": 4 * leaves,
             "changed": 4 * min(n, leaves), "new": 4 * cap, "gone": 4 * cap, "scratch": scratch.value}
    b = {k: _guarded(v) for k, v in sizes.items()}
    t = tree._names_dev()
    problem, summary = C.c_uint64(77), (C.c_uint64 * 8)()
    ffi.check(R.sr_mst_csv_diff_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), ord(delim), nc, n, ffi.dev_ptr(b["spans"]),
                                    ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(t["d_name_spans"]),
                                    None if tree._sorted_dev is not None else ffi.dev_ptr(t["d_order"]), t["n"], depth, ffi.dev_ptr(tree.d_bals),
                                    ffi.dev_ptr(b["row_leaf"]), ffi.dev_ptr(b["row_state"]), ffi.dev_ptr(b["leaf_state"]), ffi.dev_ptr(b["owner"]),
                                    ffi.dev_ptr(b["changed"]), ffi.dev_ptr(b["new"]) if cap else None, ffi.dev_ptr(b["gone"]) if cap else None,
                                    cap, ffi.dev_ptr(b["scratch"]), C.byref(problem), summary, ffi.current_stream_ptr()))
    torch.cuda.current_stream().synchronize()
    assert problem.value == 0
    for k, used in sizes.items():
        assert (b[k][used:] == GUARD).all(), f"the bytes behind {k} changed"
    out = {k: b[k][:sizes[k]].cpu().numpy() for k in ("row_state", "leaf_state")}
    out.update({k: b[k][:sizes[k]].cpu().numpy().view(np.uint32) for k in ("row_leaf", "owner", "changed", "new", "gone")})
    return dict(out, summary=[int(x) for x in summary])


def _same_array(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (what, f"{wrong.size} entries differ, the first at", int(wrong[0]), int(got[wrong[0]]), int(want[wrong[0]]))


@pytest.mark.parametrize("sorted_tree", [False, True], ids=["file", "sorted"])
def test_every_output_of_the_diff_at_big_rows_equals_the_numpy_model(gpu, big, sorted_tree):
    """a tree of depth 21 -- 128 groups of leaves, the chosen ones in groups 0 .. 65 -- and a file of 66 groups of rows: items of
    group 64 sum 64 group totals in one full trip of the scatter's loop, all six shuffle steps carrying data, those of group 65
    take the second trip"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    case = big[sorted_tree]
    tree = big_tree(case, sorted_tree)
    full = cases.model_np(case["a"], case["b1"], sorted_tree)
    scanned, reason = DeviceMerkleSumTree._csv_text_on_device(case["paths"]["b1"], cases.BIG_NC)
    assert scanned is not None, reason
    n_new, n_gone = full["summary"][0], full["summary"][4]
    before_65 = int(np.count_nonzero(full["new"] < 65 * cases.GROUP_ROWS))
    assert before_65 > 1 and n_new - before_65 == (2 if sorted_tree else 1)     # the new rows of group 65: see big_case
    for cap in sorted({0, 1, max(n_new, n_gone), before_65, before_65 + 1}):
        want = cases.model_np(case["a"], case["b1"], sorted_tree, cap)
        got = run_diff_np(tree, scanned, cap)
        assert got["summary"] == want["summary"], (cap, got["summary"])
        for key in ("row_leaf", "row_state", "leaf_state", "owner"):
            _same_array(got[key], want[key], (cap, key))
        for key in ("changed", "new", "gone"):
            listed = want[key].size
            _same_array(got[key][:listed], want[key], (cap, key))
            assert (got[key][listed:] == FILL32).all(), (cap, key, "an entry behind the listed ones was written")


def test_the_apply_at_big_rows_leaves_the_new_files_own_tree(gpu, big):
    """apply_csv of B2 on the tree in file order: the leaves line up with the new file's own tree, bit for bit in all four arrays"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    case = big[False]
    tree = big_tree(case, False)
    diff = tree.apply_csv(case["paths"]["b2"])
    assert diff.ingest == "device" and np.array_equal(diff.changed, case["changed"].astype(np.uint32))
    changed = case["changed"].size
    assert diff.summary() == dict(zip(cases.SUMMARY, [0, 0, changed, cases.BIG - changed, 0, 0, 0, 0]))
    fresh = DeviceMerkleSumTree.from_csv(case["paths"]["b2"], cases.BIG_NC, name_index=True)
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), getattr(fresh, what).cpu().numpy(), f"big: {what}")
    again = tree.diff_csv(case["paths"]["b2"])
    assert again.n_changed == 0 and again.changed.size == 0 and again.n_same == cases.BIG and again.n_new == again.n_gone == 0


# ============================================================================= stream order
STREAM_CASE = "edges_changed_shuffled_257_file"


def _u8(t):
    return t.cpu().numpy().view(np.uint8).reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def diff_stream_case():
    """sr_mst_csv_diff_dev as a row of stream_cases: the real inputs are the new file's text, its scan's tile words, the tree's text,
    spans, order and leaf balances; the decoy is the same file with other balances against a tree of zero balances"""
    import tempfile
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    _, a, b, nc, _ = BY_NAME[STREAM_CASE]
    d = tempfile.mkdtemp()
    decoy_b = [(nm, [str(int(x) + 3) for x in bal]) for nm, bal in b]
    zero_a = [(nm, ["0"] * nc) for nm, _ in a]
    pa, pb, pd = (cases.write_case(d, n, cases.text_of(rows, nc)) for n, rows in (("a", a), ("b", b), ("d", decoy_b)))
    tree = DeviceMerkleSumTree.from_csv(pa, nc, name_index=True)
    t = tree._names_dev()
    text, size, body_off, delim, _, tiles, n = DeviceMerkleSumTree._csv_text_on_device(pb, nc)[0]
    decoy_text = DeviceMerkleSumTree._csv_text_on_device(pd, nc)[0][0]
    assert decoy_text.numel() == text.numel()
    leaves, cap = 1 << tree.depth, 4
    scratch = C.c_uint64(0)
    ffi.check(ffi.rounds_lib().sr_mst_diff_scratch(n, tree.depth, C.byref(scratch)))
    zeros = lambda x: np.zeros_like(_u8(x))
    ins = {"b_text": (_u8(text), _u8(decoy_text)), "tiles": (_u8(tiles), _u8(tiles)), "t_text": (_u8(t["text"]), _u8(t["text"])),
           "name_spans": (_u8(t["d_name_spans"]), zeros(t["d_name_spans"])), "order": (_u8(t["d_order"]), zeros(t["d_order"])),
           "bals": (_u8(tree.d_bals), zeros(tree.d_bals))}
    outs = {"row_leaf": 4 * n, "row_state": n, "leaf_state": leaves, "owner": 4 * leaves, "changed": 4 * min(n, leaves), "new": 4 * cap, "gone": 4 * cap}
    size_t, off_t, n_tree, depth = t["size"], t["body_off"], t["n"], tree.depth

    def call(bf, h, ctx):
        problem, summary = C.c_uint64(0), (C.c_uint64 * 8)()
        p = lambda k: ffi.dev_ptr(bf[k])
        ffi.check(ffi.rounds_lib().sr_mst_csv_diff_dev(p("b_text"), size, body_off, p("tiles"), ord(delim), nc, n, p("spans"), p("t_text"), size_t, off_t,
                                                       p("name_spans"), p("order"), n_tree, depth, p("bals"), p("row_leaf"), p("row_state"),
                                                       p("leaf_state"), p("owner"), p("changed"), p("new"), p("gone"), cap, p("scratch"),
                                                       C.byref(problem), summary, ffi.current_stream_ptr()))
        return np.array([problem.value] + list(summary), dtype=np.uint64).view(np.uint8)

    def ref(i):
        real = np.array_equal(i["b_text"], ins["b_text"][0])
        m = cases.model(a, b, nc, False, cap) if real else cases.model(zero_a, decoy_b, nc, False, cap)
        fill = lambda values, count: np.array(values + [sc.FILL * 0x01010101] * (count - len(values)), dtype=np.uint32)
        out = {"row_leaf": np.array(m["row_leaf"], dtype=np.uint32), "row_state": np.array(m["row_state"], dtype=np.uint8),
               "leaf_state": np.array(m["leaf_state"], dtype=np.uint8), "owner": np.array(m["owner"], dtype=np.uint32),
               "changed": fill(m["changed"], min(n, leaves)), "new": fill(m["new"], cap), "gone": fill(m["gone"], cap),
               "host": np.array([0] + m["summary"], dtype=np.uint64)}
        return {k: v.view(np.uint8) for k, v in out.items()}    # bytes: Case.want converts, it does not reinterpret
    return sc.Case(call, ref, ins=ins, outs=outs, opaque={"spans": 8 * (n + 2 + 2 * n * (1 + nc)), "scratch": scratch.value})


@functools.lru_cache(maxsize=None)
def apply_stream_case():
    """sr_mst_apply_diff_dev as a row: the real inputs are what a diff left (the file's text, its spans, the owners, the changed list)
    and the tree's four arrays, three of them written in place; the decoy is zeros, and a changed list of zeros is refused"""
    import tempfile
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    _, a, b, nc, _ = BY_NAME[STREAM_CASE]
    d = tempfile.mkdtemp()
    pa, pb = (cases.write_case(d, n, cases.text_of(rows, nc)) for n, rows in (("a", a), ("b", b)))
    tree = DeviceMerkleSumTree.from_csv(pa, nc, name_index=True)
    got = run_diff(tree, pb, 0)
    torch.cuda.synchronize()
    dev, m = got["dev"], model_of(STREAM_CASE)
    n, n_changed, depth = got["n"], len(m["changed"]), tree.depth
    span_bytes = 8 * (n + 2 + 2 * n * (1 + nc))
    real = {"b_text": _u8(dev["text"]), "spans": _u8(dev["buffers"]["spans"][:span_bytes]), "owner": _u8(dev["buffers"]["owner"][:4 << depth]),
            "changed": _u8(dev["buffers"]["changed"][:4 * min(n, 1 << depth)]), "users": _u8(tree.d_users), "bals": _u8(tree.d_bals),
            "hashes": _u8(tree.d_h), "node_bals": _u8(tree.d_b)}
    ins = {k: (v, np.zeros_like(v)) for k, v in real.items()}
    size, body_off = dev["size"], dev["body_off"]

    def call(bf, h, ctx):
        p = lambda k: ffi.dev_ptr(bf[k])
        ffi.check(ffi.rounds_lib().sr_mst_apply_diff_dev(p("b_text"), size, body_off, p("spans"), n, p("owner"), p("changed"), n_changed, depth, nc,
                                                         p("users"), p("bals"), p("hashes"), p("node_bals"), ffi.current_stream_ptr()))

    want, _, _ = fresh_arrays(STREAM_CASE)

    def ref(i):
        if np.array_equal(i["changed"], real["changed"]):
            return {"bals": want["d_bals"], "hashes": want["d_h"], "node_bals": want["d_b"]}
        return {k: np.zeros_like(real[k]) for k in ("bals", "hashes", "node_bals")}
    return sc.Case(call, ref, ins=ins, inout=("bals", "hashes", "node_bals"))


@pytest.fixture(scope="module")
def delay(gpu):
    """test_gpu_stream_order.py's delay over these two rows: torch.cuda._sleep calibrated against events, both rows timed once
    undelayed, the delay ten times the slower within 20 .. 200 ms"""
    import torch
    import test_gpu_stream_order as so
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(1_000_000)
    probe = 20_000_000

    def spin():
        with torch.cuda.stream(s):
            torch.cuda._sleep(probe)
    per_ms = probe / so._timed(s, spin)
    slowest = 0.0
    for case in (diff_stream_case(), apply_stream_case()):
        run = so.Run(case)
        try:
            slowest = max(slowest, min(so._timed(s, lambda: run.issue(s, 0)) for _ in range(2)))
        finally:
            torch.cuda.synchronize()
            run.close()
    ms = min(so.MAX_DELAY_MS, max(so.MIN_DELAY_MS, so.MARGIN * slowest))
    return {"cycles": int(ms * per_ms), "ms": ms}


@pytest.mark.parametrize("which", ["diff", "apply"])
def test_both_entries_are_ordered_on_their_stream(gpu, delay, which):
    """a delayed producer on the same stream writes the real inputs over the decoy before the call, and a trailer reads the outputs
    and puts the decoy back behind it: the result is the real inputs', on two fresh streams made one after the other"""
    import test_gpu_stream_order as so
    case = diff_stream_case() if which == "diff" else apply_stream_case()
    for j, stream in enumerate(so._streams(2)):
        so._run_all([(so.Run(case), stream)], delay["cycles"], f"{which}, stream {j}, delay {delay['ms']:.1f} ms")
