"""A round settled in full on a tree in HBM (include/summa_admit.h, csrc/mst_admit.h): the new users admitted into the padding, the
name index extended, the gone users zeroed, one run of the update's kernels -- through the C ABI with every written buffer guarded,
and through `apply_diff` / `apply_csv` with their keywords, against the model of mst_admit_cases.py, a fresh tree of the model's
entries and, at the small sizes, the oracle's root."""
import ctypes as C
import functools

import numpy as np
import pytest

import mst_admit_cases as cases
import mst_diff_cases as D
import stream_cases as sc
import test_gpu_mst_diff as gd

pytestmark = pytest.mark.gpu

CASES = cases.cases()
IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
GOOD = [c[0] for c in CASES if c[4] is None]
REFUSED = [c[0] for c in CASES if c[4] is not None]
ARRAYS = ("d_users", "d_bals", "d_h", "d_b")
ORACLE_ROOTS = {"tree_1_new_0", "tree_3_new_1", "tree_63_new_1", "tree_65_new_2", "tree_65_new_63", "tree_257_new_65", "contents_300",
                "currencies_1_65", "currencies_3_65", "empty_name_in_tree"}

gpu = gd.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{case name: (path of A, path of B)}"""
    d = tmp_path_factory.mktemp("mst_admit_gpu")
    return {c[0]: (cases.write_case(d, c[0] + ".a", cases.text_a(c[0], c[1], c[3])), cases.write_case(d, c[0] + ".b", cases.text_of(c[2], c[3])))
            for c in CASES}


@functools.lru_cache(maxsize=None)
def model_of(name, admit=True, zero=True):
    _, a, b, nc, _ = BY_NAME[name]
    return cases.settled(a, b, nc, admit, zero)


def as_entries(entries):
    return [(None if name is None else name.decode(), list(bal)) for name, bal in entries]


@functools.lru_cache(maxsize=None)
def fresh_of(name, admit=True, zero=True):
    """the four arrays of `from_entries` of the model's entries, computed once and left unchanged, and its root"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    m = model_of(name, admit, zero)
    tree = DeviceMerkleSumTree.from_entries([e for e in as_entries(m["entries"]) if e[0] is not None], BY_NAME[name][3])
    assert tree.depth == m["diff"]["depth"]
    arrays = {what: getattr(tree, what).cpu().numpy() for what in ARRAYS}
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


def tree_of(name, files):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    tree = DeviceMerkleSumTree.from_csv(files[name][0], BY_NAME[name][3], name_index=True)
    assert tree.csv_ingest == "device" and tree.has_name_index
    if name == "padding_with_balances_5":
        tree.update_leaves_at([5, 7], [[111, 222], [333, 444]])
    return tree


def state_of(tree):
    """what a refusal must leave as it was: the four arrays, the text, the index arrays, the counter, the root"""
    t = tree._names_dev()
    out = {what: getattr(tree, what).clone() for what in ARRAYS}
    out.update({k: t[k].clone() for k in ("text", "d_order", "d_name_spans", "d_leaf_name_spans") if k in t})
    out.update(size=t["size"], n=t["n"], updates=tree._updates, root=tree.root()[0].tolist(), index=t)
    return out


def assert_untouched(tree, before, what):
    import torch
    torch.cuda.synchronize()
    now = state_of(tree)
    for k, v in before.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(now[k], v), f"{what}: {k} changed"
        elif k == "index":
            assert now[k] is v, f"{what}: the index was replaced"
        else:
            assert now[k] == v, f"{what}: {k} changed"


def names_through(text, body_off, spans):
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2) + body_off
    return [bytes(text[b:e]) for b, e in spans.tolist()]


def index_of(t):
    """(order, the sorted names, the leaves' names) of a tree's index record, resolved through the spans into its text"""
    text = t["text"][:t["size"]].cpu().numpy()
    u32 = lambda k: t[k].cpu().numpy().view(np.uint32)
    return (u32("d_order").tolist(), names_through(text, t["body_off"], u32("d_name_spans")),
            names_through(text, t["body_off"], u32("d_leaf_name_spans")))


def same_arrays(tree, want, what):
    for k in ARRAYS:
        gd._same(getattr(tree, k).cpu().numpy(), want[k], f"{what}: {k}")


# ============================================================================= the two calls, through the C ABI
def settle_abi(tree, got, n_new, n_gone):
    """sa_mst_admit_measure_dev (for new rows) and sa_mst_settle_dev behind gd.run_diff: every buffer they write pre-filled with 0xEE
    and followed by 64 guard bytes that must come back untouched -> {"problem"} or the index record of the outputs"""
    import torch
    from circuits_halo2_amd import ffi
    A, d, t = ffi.admit_lib(), got["dev"], tree._names_dev()
    b, nc, n, depth, stream = d["buffers"], tree.n_currencies, got["n"], tree.depth, ffi.current_stream_ptr()
    p = lambda x: ffi.dev_ptr(x) if x is not None else None
    sizes, out, scratch, name_bytes = {}, {}, None, C.c_uint64(0)

    def guards_hold():
        torch.cuda.current_stream().synchronize()
        for k, used in sizes.items():
            assert (out[k][used:] == gd.GUARD).all(), f"the bytes behind {k} changed"
    if n_new:
        scratch_bytes, problem = C.c_uint64(0), C.c_uint64(77)
        ffi.check(A.sa_mst_admit_scratch(n, nc, n_new, C.byref(scratch_bytes)))
        sizes["scratch"] = scratch_bytes.value
        out["scratch"] = scratch = gd._guarded(scratch_bytes.value)
        ffi.check(A.sa_mst_admit_measure_dev(p(d["text"]), d["size"], d["body_off"], p(b["spans"]), n, nc, p(b["row_state"]), p(b["new"]), n_new,
                                             t["n"], depth, p(scratch), C.byref(name_bytes), C.byref(problem), stream))
        guards_hold()
        if problem.value:
            return {"problem": problem.value}
        n_all = t["n"] + n_new
        sizes.update(text=t["size"] + name_bytes.value, d_name_spans=8 * n_all, d_order=4 * n_all, d_leaf_name_spans=8 * n_all)
        out.update({k: gd._guarded(sizes[k]) for k in ("text", "d_name_spans", "d_order", "d_leaf_name_spans")})
    index = t if n_new else {}
    ffi.check(A.sa_mst_settle_dev(p(d["text"]), d["size"], d["body_off"], p(b["spans"]), n, nc, p(b["owner"]), p(b["leaf_state"]), p(b["changed"]),
                                  got["summary"][2], p(b["gone"]) if n_gone else None, n_gone, p(b["new"]) if n_new else None, n_new, p(scratch),
                                  p(index.get("text")), index.get("size", 0), index.get("body_off", 0), p(index.get("d_name_spans")),
                                  p(index.get("d_order")), p(index.get("d_leaf_name_spans")), t["n"], depth, p(out.get("text")),
                                  name_bytes.value, p(out.get("d_name_spans")), p(out.get("d_order")), p(out.get("d_leaf_name_spans")),
                                  p(tree.d_users), p(tree.d_bals), p(tree.d_h), p(tree.d_b), stream))
    guards_hold()
    if not n_new:
        return {}
    return dict({k: out[k][:sizes[k]] for k in ("text", "d_name_spans", "d_order", "d_leaf_name_spans")}, size=sizes["text"],
                body_off=t["body_off"], n=t["n"] + n_new, name_bytes=name_bytes.value)


def check_index(record, m, a_text, what):
    order, names, leaf_names = index_of(record)
    n = m["n"]
    assert sorted(order) == list(range(n)), f"{what}: the merged order is no bijection"
    assert order == m["order"] and names == m["names"], what
    assert leaf_names == [name for name, _ in m["entries"][:n]], what
    text = record["text"][:record["size"]].cpu().numpy().tobytes()
    assert text == a_text + b"".join(name for name, _ in m["entries"][len(m["diff"]["leaf_rows"]):n]), f"{what}: the text"


@pytest.mark.parametrize("name", GOOD)
def test_the_settled_tree_is_a_fresh_tree_of_the_models_entries(gpu, files, name):
    from circuits_halo2_amd.merkle_sum_tree import _mont_to_int
    _, a, b, nc, _ = BY_NAME[name]
    m = model_of(name)
    tree = tree_of(name, files)
    n_cap = max(len(b), 1 << tree.depth)
    got = gd.run_diff(tree, files[name][1], n_cap)
    assert got["summary"][:6] == m["diff"]["summary"][:6]
    record = settle_abi(tree, got, got["summary"][0], got["summary"][4])
    same_arrays(tree, fresh_of(name), name)
    if got["summary"][0]:
        check_index(record, m, cases.text_a(name, a, nc).encode(), name)
    else:
        assert record == {}
    if name in ORACLE_ROOTS:
        from oracle import pyref as P
        assert m["n"] <= 520
        (oracle_h, oracle_b), _ = P.mst_build([P.mst_entry(nm, bal) for nm, bal in as_entries(m["entries"])[:m["n"]]])
        tree._root = None
        assert _mont_to_int(tree.root()[0]) == oracle_h
        assert [_mont_to_int(tree.root()[1][32 * c:32 * c + 32]) for c in range(nc)] == [v % P.R for v in oracle_b]


def test_the_oracle_list_is_in_the_cases():
    assert ORACLE_ROOTS <= set(GOOD)


def test_the_measure_reports_the_lowest_long_name_and_the_settle_a_bad_list(gpu, files):
    import torch
    from circuits_halo2_amd import ffi
    name = "refused_name_of_65_bytes"
    tree = tree_of(name, files)
    got = gd.run_diff(tree, files[name][1], 200)
    before = state_of(tree)
    assert settle_abi(tree, got, got["summary"][0], 0) == {"problem": 40 << 8 | 7}
    assert_untouched(tree, before, name)
    name = "tree_257_new_65"
    tree = tree_of(name, files)
    got = gd.run_diff(tree, files[name][1], 512)
    before = state_of(tree)
    changed, gone = got["dev"]["buffers"]["changed"], got["dev"]["buffers"]["gone"]
    keep = changed[:8].clone()
    for bad, word in (([5, 5], "strictly increase"), ([9, 4], "strictly increase"), ([3, 257], "no named leaf")):
        changed[:8] = torch.from_numpy(np.array(bad, dtype=np.uint32).view(np.uint8)).cuda()
        with pytest.raises(ffi.SummaGpuError, match=word):
            settle_abi(tree, dict(got, summary=[0, 0, 2]), got["summary"][0], got["summary"][4])
    changed[:8] = keep
    gone[:4] = changed[:4]
    with pytest.raises(ffi.SummaGpuError, match="both changed and gone"):
        settle_abi(tree, got, got["summary"][0], got["summary"][4])
    assert_untouched(tree, before, name)


# ============================================================================= the Python surface
def _counting(monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    parses = []
    real_parse = M.parse_csv_to_entries
    monkeypatch.setattr(M, "parse_csv_to_entries", lambda *a: parses.append(a[0]) or real_parse(*a))
    return parses


@pytest.mark.parametrize("parsed_before", [False, True], ids=["lazy", "parsed"])
@pytest.mark.parametrize("name", GOOD)
def test_apply_csv_with_both_keywords_and_the_tree_afterwards(gpu, files, name, parsed_before, tmp_path, monkeypatch):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    _, a, b, nc, _ = BY_NAME[name]
    m = model_of(name)
    want_entries, n, n_tree = as_entries(m["entries"]), m["n"], len(a)
    tree = tree_of(name, files)
    parses = _counting(monkeypatch)
    if parsed_before:
        assert len(tree.entries) == 1 << tree.depth
    assert tree.free_leaves == (1 << tree.depth) - n_tree
    diff = tree.diff_csv(files[name][1])
    assert diff.admitted == range(n_tree, n) and diff.ingest == "device"
    updates = tree._updates
    index = tree._names_dev()
    tree.apply_diff(diff, admit_new=True, zero_gone=True)
    assert tree._updates == updates + 1 and tree.free_leaves == (1 << tree.depth) - n
    same_arrays(tree, fresh_of(name), name)
    if n > n_tree:
        check_index(tree._names_dev(), m, cases.text_a(name, a, nc).encode(), name)
    else:
        assert tree._names_dev() is index, "nobody was admitted and the index was replaced"
    # lookups: every name, old and admitted, finds its first leaf; two absent ones do not
    first = {}
    for leaf, (nm, _) in enumerate(want_entries[:n]):
        first.setdefault(nm, leaf)
    asked = list(first)
    if parsed_before and n > 600:                             # the parsed tree scans its entries for every name: the edges and a sample
        asked = asked[:3] + asked[3:-3:max(1, n // 200)] + asked[-3:]
    assert tree.indices_of_usernames(asked) == [first[nm] for nm in asked]
    for absent in ("nobody", "zzzzzzzzz"):
        with pytest.raises(KeyError):
            tree.index_of_username(absent)
    if n > n_tree:
        leaf = n - 1 if first[want_entries[n - 1][0]] == n - 1 else n_tree
        proof = tree.generate_proof(leaf)
        assert proof["entry"] == want_entries[leaf] and tree.verify_proof(proof)
        assert tree.get_entry(leaf) == want_entries[leaf]
    # the last old leaf: in the tree's text the admitted names follow its row
    assert tree.get_entry(n_tree - 1) == want_entries[n_tree - 1]
    proof = tree.generate_proof(n_tree - 1)
    assert proof["entry"] == want_entries[n_tree - 1] and tree.verify_proof(proof)
    # the export, and a fresh tree of it
    out = str(tmp_path / "settled.csv")
    done = tree.to_csv(out)
    assert done.ingest == "device" and done.n_rows == n and open(out).read() == cases.csv_of(m["entries"], nc)
    again = DeviceMerkleSumTree.from_csv(out, nc, name_index=True)
    assert again.root()[0].tolist() == tree.root()[0].tolist()
    dups, dups_again = tree.duplicate_names(), again.duplicate_names()
    repeated, pairs = cases.duplicates_of(m["entries"])
    assert (dups.n_repeated_names, dups.shadowed.tolist(), dups.first.tolist()) == (repeated, [s for s, _ in pairs], [f for _, f in pairs])
    assert (dups_again.n_repeated_names, dups_again.n_shadowed, dups_again.shadowed.tolist(), dups_again.first.tolist()) == (
        dups.n_repeated_names, dups.n_shadowed, dups.shadowed.tolist(), dups.first.tolist())
    audit, audit_again = tree.range_audit(), again.range_audit()
    assert (audit.n_bad_nodes, audit.n_unprovable) == (audit_again.n_bad_nodes, audit_again.n_unprovable)
    # idempotence: the same file once more changes nothing
    second = tree.apply_csv(files[name][1], admit_new=True, zero_gone=True)
    assert (second.n_new, second.n_changed, second.n_gone) == (0, 0, diff.n_gone) and second.gone.tolist() == diff.gone.tolist()
    same_arrays(tree, fresh_of(name), f"{name}: the same file once more")
    # an update by an admitted name
    if n > n_tree:
        leaf = n_tree
        if first[want_entries[leaf][0]] == leaf:
            bumped = [v % 1000 + 9 for v in want_entries[leaf][1]]
            tree.update_leaves([(want_entries[leaf][0], bumped)])
            assert tree.get_entry(leaf) == (want_entries[leaf][0], bumped)
            want_entries[leaf] = (want_entries[leaf][0], bumped)
    assert tree.entries[:n] == want_entries[:n] and all(nm is None for nm, _ in tree.entries[n:])
    assert set(parses) <= {files[name][0]} and len(parses) == 1, "the new file was parsed, or the tree's own more than once"
    # a third round: an admitted user's balance changes, one user leaves, one joins where there is room
    rows3 = [(nm.encode(), [str(v) for v in bal]) for nm, bal in want_entries[:n]]
    count = {}
    for nm, _ in want_entries[:n]:
        count[nm] = count.get(nm, 0) + 1
    once = [leaf for leaf in range(n) if count[want_entries[leaf][0]] == 1]      # the leaves whose name no other leaf has
    if len(once) < 2:
        assert n == 1                                         # the tree of one row: a round that changes one user and loses another needs two
        return
    leaves_out = once[-1]
    change = next((leaf for leaf in once if leaf >= n_tree and leaf != leaves_out), once[0])
    assert change != leaves_out
    rows3[change] = D.bump(rows3[change], 0)
    del rows3[leaves_out]
    joins = n < (1 << tree.depth)
    if joins:
        rows3.insert(1, (b"third-round", ["5"] * nc))
    third = tree.apply_csv(cases.write_case(tmp_path, "third", cases.text_of(rows3, nc)), admit_new=True, zero_gone=True)
    assert third.n_changed == 1 and third.n_new == int(joins) and leaves_out in third.gone.tolist()
    want3 = [(nm.decode(), [int(x) for x in bal]) for nm, bal in cases.settled(
        [(nm.encode(), [str(v) for v in bal]) for nm, bal in want_entries[:n]], rows3, nc)["entries"] if nm is not None]
    fresh3 = DeviceMerkleSumTree.from_entries(want3, nc)
    same_arrays(tree, {k: getattr(fresh3, k).cpu().numpy() for k in ARRAYS}, f"{name}: the third round")
    assert tree.entries[:len(want3)] == want3


@pytest.mark.parametrize("name", REFUSED)
def test_every_refusal_raises_and_leaves_the_tree_as_it_was(gpu, files, name):
    _, a, b, nc, refusal = BY_NAME[name]
    tree = tree_of(name, files)
    cap = cases.CAP_SHORT if refusal.startswith("cap") else None
    diff = tree.diff_csv(files[name][1], cap)
    before = state_of(tree)
    word = {"no_room": "rebuild is due", "name_too_long": "row 40: name too long", "cap_new": "new rows incomplete",
            "cap_gone": "gone leaves incomplete"}[refusal]
    with pytest.raises(ValueError, match=word):
        tree.apply_diff(diff, admit_new=True, zero_gone=True)
    assert_untouched(tree, before, name)
    with pytest.raises(ValueError, match=word):
        tree.apply_csv(files[name][1], cap, admit_new=True, zero_gone=True)
    assert_untouched(tree, before, name)
    if refusal == "cap_gone":                                 # ... each list only where it is asked for
        tree.apply_diff(diff, admit_new=True)
        same_arrays(tree, fresh_of(name, True, False), name)
    elif refusal in ("cap_new", "no_room", "name_too_long"):
        tree.apply_diff(tree.diff_csv(files[name][1]), zero_gone=True)
        same_arrays(tree, fresh_of(name, False, True), name)


def test_a_stale_diff_and_another_trees_are_refused_with_the_keywords_too(gpu, files):
    name = "tree_257_new_65"
    tree, other = tree_of(name, files), tree_of(name, files)
    diff = tree.diff_csv(files[name][1])
    before = state_of(other)
    with pytest.raises(ValueError, match="another tree"):
        other.apply_diff(diff, admit_new=True, zero_gone=True)
    assert_untouched(other, before, f"{name}: a diff of another tree")
    tree.update_leaves_at([7], [[1, 2]])
    before = state_of(tree)
    for keys in ({"admit_new": True, "zero_gone": True}, {"admit_new": True}, {"zero_gone": True}):
        with pytest.raises(ValueError, match="before another update"):
            tree.apply_diff(diff, **keys)
        assert_untouched(tree, before, f"{name}: a stale diff, {sorted(keys)}")
    tree.apply_csv(files[name][1], admit_new=True, zero_gone=True)   # a diff of the tree as it is now goes through, leaf 7 included
    same_arrays(tree, fresh_of(name), name)
    with pytest.raises(ValueError, match="before another update"):
        tree.apply_diff(diff, admit_new=True, zero_gone=True)


@pytest.mark.parametrize("name", ["tree_65_new_2", "tree_257_new_65", "contents_300", "tree_2049_new_2047"])
def test_the_defaults_leave_new_and_gone_users_alone(gpu, files, name):
    tree = tree_of(name, files)
    index = tree._names_dev()
    diff = tree.diff_csv(files[name][1])
    tree.apply_diff(diff)
    same_arrays(tree, fresh_of(name, False, False), name)
    assert tree._names_dev() is index and tree.free_leaves == (1 << tree.depth) - len(BY_NAME[name][1])
    tree = tree_of(name, files)
    tree.apply_csv(files[name][1], admit_new=False, zero_gone=False)
    same_arrays(tree, fresh_of(name, False, False), f"{name}: apply_csv")
    tree = tree_of(name, files)
    tree.apply_csv(files[name][1], zero_gone=True)            # one keyword alone
    same_arrays(tree, fresh_of(name, False, True), f"{name}: zero_gone alone")
    tree = tree_of(name, files)
    tree.apply_csv(files[name][1], admit_new=True)
    same_arrays(tree, fresh_of(name, True, False), f"{name}: admit_new alone")


def test_trees_that_cannot_admit_still_zero_the_gone(gpu, files):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    name = "tree_257_new_65"
    _, a, b, nc, _ = BY_NAME[name]
    value = lambda bal: [int(x) % cases.R for x in bal]
    for sorted_tree in (True, False):
        m = D.model(a, b, nc, sorted_tree)
        entries = [(a[r][0].decode(), value(a[r][1])) for r in m["leaf_rows"]]
        for leaf, bal in zip(m["changed"], m["balances"]):
            entries[leaf] = (entries[leaf][0], bal)
        for leaf in m["gone"]:
            entries[leaf] = (entries[leaf][0], [0] * nc)
        fresh = DeviceMerkleSumTree.from_entries(entries, nc)
        want = {k: getattr(fresh, k).cpu().numpy() for k in ARRAYS}
        tree = DeviceMerkleSumTree.from_csv_sorted(files[name][0], nc) if sorted_tree else DeviceMerkleSumTree.from_csv(files[name][0], nc)
        diff = tree.diff_csv(files[name][1])
        assert diff.ingest == ("device" if sorted_tree else "host")
        before = {k: getattr(tree, k).clone() for k in ARRAYS}
        with pytest.raises(ValueError, match="name index" if sorted_tree else "device diff"):
            tree.apply_diff(diff, admit_new=True, zero_gone=True)
        assert all((getattr(tree, k) == v).all() for k, v in before.items()) and tree._updates == 0
        tree.apply_diff(diff, zero_gone=True)
        same_arrays(tree, want, f"{name}: sorted {sorted_tree}")
        assert tree._updates == 1
        assert [tree.get_entry(leaf) for leaf in m["gone"][:3]] == [entries[leaf] for leaf in m["gone"][:3]]


def test_the_settle_on_a_stream_of_the_callers(gpu, files):
    import torch
    name = "tree_2049_new_2047"
    tree = tree_of(name, files)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        diff = tree.apply_csv(files[name][1], admit_new=True, zero_gone=True)
    torch.cuda.synchronize()
    assert diff.n_new == 2047 and diff.ingest == "device" and tree.free_leaves == 0
    same_arrays(tree, fresh_of(name), name)


# ============================================================================= stream order
STREAM_CASE = "tree_257_new_65"


def _u8(t):
    return t.cpu().numpy().view(np.uint8).reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def stream_rows():
    """sa_mst_admit_measure_dev and sa_mst_settle_dev as rows of stream_cases.  The real inputs are what a diff left, the tree's text,
    index and four arrays and, for the settle, the work space as the measure left it; the decoy is zeros, of which the measure makes
    no bytes and which the settle refuses.  The settle's expected outputs are those of the same call on an idle stream, which the
    tests above hold to the model."""
    import tempfile
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    _, a, b, nc, _ = BY_NAME[STREAM_CASE]
    d = tempfile.mkdtemp()
    pa, pb = (cases.write_case(d, n, cases.text_of(rows, nc)) for n, rows in (("a", a), ("b", b)))
    tree = DeviceMerkleSumTree.from_csv(pa, nc, name_index=True)
    t = dict(tree._names_dev())
    got = gd.run_diff(tree, pb, 512)
    dev, bufs, m = got["dev"], got["dev"]["buffers"], model_of(STREAM_CASE)
    n, depth = got["n"], tree.depth
    n_new, n_changed, n_gone = got["summary"][0], got["summary"][2], got["summary"][4]
    A = ffi.admit_lib()
    scratch_bytes = C.c_uint64(0)
    ffi.check(A.sa_mst_admit_scratch(n, nc, n_new, C.byref(scratch_bytes)))
    span_bytes = 8 * (n + 2 + 2 * n * (1 + nc))
    before = {k: _u8(getattr(tree, k)) for k in ARRAYS}
    # the reference run, on the current stream
    scratch = torch.zeros(scratch_bytes.value, dtype=torch.uint8, device="cuda")
    size, body_off = dev["size"], dev["body_off"]
    common = {"b_text": _u8(dev["text"]), "spans": _u8(bufs["spans"][:span_bytes]), "new": _u8(bufs["new"][:4 * n_new])}

    def measure(bf, scratch_buffer):
        name_bytes, problem = C.c_uint64(0), C.c_uint64(0)
        p = lambda k: ffi.dev_ptr(bf[k])
        ffi.check(A.sa_mst_admit_measure_dev(p("b_text"), size, body_off, p("spans"), n, nc, p("row_state"), p("new"), n_new, t["n"], depth,
                                             ffi.dev_ptr(scratch_buffer), C.byref(name_bytes), C.byref(problem), ffi.current_stream_ptr()))
        return name_bytes.value, problem.value
    name_bytes, problem = measure({"b_text": dev["text"], "spans": bufs["spans"], "row_state": bufs["row_state"], "new": bufs["new"]}, scratch)
    torch.cuda.synchronize()
    assert problem == 0 and name_bytes == sum(len(nm) for nm, _ in m["entries"][len(a):m["n"]])
    record = settle_abi(tree, got, n_new, n_gone)            # measures once more, into a work space of its own, and settles
    torch.cuda.synchronize()
    after = {k: _u8(getattr(tree, k)) for k in ARRAYS}
    n_all = t["n"] + n_new

    measure_ins = dict(common, row_state=_u8(bufs["row_state"][:n]))
    measure_case = sc.Case(lambda bf, h, ctx: np.array(measure(bf, bf["scratch"]), dtype=np.uint64).view(np.uint8),
                           lambda i: {"host": np.array([name_bytes if i["spans"].any() else 0, 0], dtype=np.uint64).view(np.uint8)},
                           ins={k: (v, np.zeros_like(v)) for k, v in measure_ins.items()}, opaque={"scratch": scratch_bytes.value})

    real = dict(common, owner=_u8(bufs["owner"][:4 << depth]), leaf_state=_u8(bufs["leaf_state"][:1 << depth]),
                changed=_u8(bufs["changed"][:4 * n_changed]), gone=_u8(bufs["gone"][:4 * n_gone]), scratch=_u8(scratch), t_text=_u8(t["text"]),
                name_spans=_u8(t["d_name_spans"]), order=_u8(t["d_order"]), leaf_spans=_u8(t["d_leaf_name_spans"]),
                users=before["d_users"], bals=before["d_bals"], hashes=before["d_h"], node_bals=before["d_b"])
    outs = {"out_text": t["size"] + name_bytes, "out_name_spans": 8 * n_all, "out_order": 4 * n_all, "out_leaf_spans": 8 * n_all}

    def settle(bf, h, ctx):
        p = lambda k: ffi.dev_ptr(bf[k])
        ffi.check(A.sa_mst_settle_dev(p("b_text"), size, body_off, p("spans"), n, nc, p("owner"), p("leaf_state"), p("changed"), n_changed,
                                      p("gone"), n_gone, p("new"), n_new, p("scratch"), p("t_text"), t["size"], t["body_off"], p("name_spans"),
                                      p("order"), p("leaf_spans"), t["n"], depth, p("out_text"), name_bytes, p("out_name_spans"), p("out_order"),
                                      p("out_leaf_spans"), p("users"), p("bals"), p("hashes"), p("node_bals"), ffi.current_stream_ptr()))

    def ref(i):
        if np.array_equal(i["changed"], real["changed"]):
            return {"out_text": _u8(record["text"]), "out_name_spans": _u8(record["d_name_spans"]), "out_order": _u8(record["d_order"]),
                    "out_leaf_spans": _u8(record["d_leaf_name_spans"]), "users": after["d_users"], "bals": after["d_bals"],
                    "hashes": after["d_h"], "node_bals": after["d_b"]}
        zeros = {k: np.full(v, sc.FILL, dtype=np.uint8) for k, v in outs.items()}
        return dict(zeros, **{k: np.zeros_like(real[k]) for k in ("users", "bals", "hashes", "node_bals")})
    settle_case = sc.Case(settle, ref, ins={k: (v, np.zeros_like(v)) for k, v in real.items()}, outs=outs,
                          inout=("users", "bals", "hashes", "node_bals"))
    return {"measure": measure_case, "settle": settle_case}


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
    for case in stream_rows().values():
        run = so.Run(case)
        try:
            slowest = max(slowest, min(so._timed(s, lambda: run.issue(s, 0)) for _ in range(2)))
        finally:
            torch.cuda.synchronize()
            run.close()
    ms = min(so.MAX_DELAY_MS, max(so.MIN_DELAY_MS, so.MARGIN * slowest))
    return {"cycles": int(ms * per_ms), "ms": ms}


@pytest.mark.parametrize("which", ["measure", "settle"])
def test_both_calls_are_ordered_on_their_stream(gpu, delay, which):
    """a delayed producer on the same stream writes the real inputs over the decoy before the call, and a trailer reads the outputs
    and puts the decoy back behind it: the result is the real inputs', on two fresh streams made one after the other"""
    import test_gpu_stream_order as so
    case = stream_rows()[which]
    for j, stream in enumerate(so._streams(2)):
        so._run_all([(so.Run(case), stream)], delay["cycles"], f"{which}, stream {j}, delay {delay['ms']:.1f} ms")
