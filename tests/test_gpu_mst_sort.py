"""`DeviceMerkleSumTree.from_csv_sorted` with the names sorted on the device (csrc/mst_sort.h, the kernels in csrc/mst_sort.cuh,
ss_mst_csv_entries_sorted_dev / ss_mst_find_names of include/summa_snapshot.h), over the fixed list of mst_sort_cases.py.

A file the device takes gives the leaves in Python's stable order of the names' bytes and, bit for bit, the four arrays of
`from_entries` over the host-sorted entries -- a path this change leaves alone and that is pinned to the oracle -- and for the
small files the oracle's tree itself.  Such a tree finds, updates and proves users by name without parsing the file.  A file
outside what the device sorts goes to the host with a reason and ends as today's path ends on it.  Both entry points are held
to the stream-order contract of tests/test_gpu_stream_order.py, with its sequence.

The part before the stream order runs the list LARGE: files of 32768 rows and more, at which the one-workgroup scan of a pass's
histogram (mst_sort_scan_kernel) takes one full step of 4 x 1024 words, a second and a third -- its second call of the block
scan, its carried sum, a [digit][tile] stride of 17, 33 and 97 -- and two files, high_bytes_65537 and rows_196609, in which
the places of the rows depend on that sum (mst_sort_cases.steps_read).  The host mirror scans with one serial loop."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

import mst_sort_cases as cases
import stream_cases as sc

pytestmark = pytest.mark.gpu

TILE, CAP = 2048, 64
CASES = cases.cases(TILE)
ACCEPTED = [c[0] for c in CASES if c[3] is None]
REFUSED = [c for c in CASES if c[3] is not None]
GUARD = 0x5A
ABSENT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    cap, tile = C.c_uint32(0), C.c_uint32(0)
    ffi.snapshot_lib().ss_mst_sort_geometry(C.byref(cap), C.byref(tile))
    assert (cap.value, tile.value) == (CAP, TILE)              # the list places its sizes by these
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{case name: (path, n_currencies)}"""
    d = tmp_path_factory.mktemp("mst_sort_gpu")
    return {c[0]: (cases.write_case(d, c[0], c[1]), c[2]) for c in CASES}


def _same(got, want, what):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} bytes, {w.size} expected"
    bad = (g.reshape(-1, 32) != w.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


@functools.lru_cache(maxsize=None)
def reference(path, nc):
    """today's path, computed once per file: the parsed entries, the host-sorted entries, and `from_entries` of those"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries
    entries, crypto = parse_csv_to_entries(path, nc)
    host_sorted = sorted(entries, key=lambda e: e[0].encode())
    tree = DeviceMerkleSumTree.from_entries(host_sorted, nc, is_sorted=True)
    arrays = {what: getattr(tree, what).cpu().numpy() for what in ("d_users", "d_bals", "d_h", "d_b")}
    for a in arrays.values():
        a.setflags(write=False)
    return {"entries": entries, "sorted": host_sorted, "padded": list(tree.entries), "depth": tree.depth, "crypto": crypto, **arrays}


def _guarded(n_bytes):
    import torch
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def run_sort(path, nc):
    """scan + the sorted entries call, every buffer it writes followed by 64 guard bytes that must come back untouched ->
    {"n", "problem", "body", "order", "spans", "users", "bals"}"""
    import torch
    from circuits_halo2_amd import ffi
    L, S = ffi.lib(), ffi.snapshot_lib()
    data = np.fromfile(path, dtype=np.uint8)
    body_off = data.tobytes().index(b"\n") + 1
    delim = ord(";") if b";" in data[:body_off].tobytes() else ord(",")
    size = int(data.size)
    pad = -body_off % 16
    buf = torch.zeros(pad + size, dtype=torch.uint8, device="cuda")
    buf[pad:].copy_(torch.from_numpy(data))
    text = buf[pad:]
    tiles = torch.zeros(4 * (-(-(size - body_off) // 4096) + 2), dtype=torch.uint8, device="cuda")
    n, flags, problem, sort_bytes = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    stream = ffi.current_stream_ptr()
    ffi.check(L.sg_mst_csv_scan_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), C.byref(n), C.byref(flags), stream))
    assert flags.value == 0 and n.value
    n = n.value
    rows = 1 << max(0, (n - 1).bit_length())
    ffi.check(S.ss_mst_sort_scratch(n, C.byref(sort_bytes)))
    sizes = {"spans": 16 * (n + 1 + 2 * n * (1 + nc)), "sort": sort_bytes.value, "order": 4 * n, "name_spans": 8 * n, "users": 32 * rows,
             "bals": 32 * rows * nc}
    b = {k: _guarded(v) for k, v in sizes.items()}
    ffi.check(S.ss_mst_csv_entries_sorted_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), delim, nc, n, rows, ffi.dev_ptr(b["spans"]),
                                              ffi.dev_ptr(b["sort"]), ffi.dev_ptr(b["order"]), ffi.dev_ptr(b["name_spans"]),
                                              ffi.dev_ptr(b["users"]), ffi.dev_ptr(b["bals"]), C.byref(problem), stream))
    torch.cuda.current_stream().synchronize()
    for k, used in sizes.items():
        assert (b[k][used:] == GUARD).all(), f"the bytes behind {k} changed"
    out = {"n": n, "problem": (problem.value >> 8, problem.value & 0xff), "body": data[body_off:].tobytes()}
    if problem.value:
        for k in ("order", "name_spans", "users", "bals"):
            assert (b[k] == GUARD).all(), f"{k} was written behind a problem"
        return out
    out.update(order=b["order"][:4 * n].cpu().numpy().view(np.uint32).tolist(),
               spans=b["name_spans"][:8 * n].cpu().numpy().view(np.uint32).reshape(-1, 2).tolist(),
               users=b["users"][:32 * rows].cpu().numpy(), bals=b["bals"][:32 * rows * nc].cpu().numpy())
    return out


# ============================================================================= the entry point over the list
@pytest.mark.parametrize("name", ACCEPTED)
def test_order_spans_and_leaf_inputs(gpu, files, name):
    order_spans_and_leaf_inputs(files[name], name)


def order_spans_and_leaf_inputs(file, name):
    path, nc = file
    ref = reference(path, nc)
    got = run_sort(path, nc)
    names = [e[0].encode() for e in ref["entries"]]
    want = cases.stable_order(names)
    assert got["problem"] == (0, 0) and got["n"] == len(names)
    assert got["order"] == want, f"{name}: d_order is not Python's stable order"
    assert [got["body"][b:e] for b, e in got["spans"]] == [names[i] for i in want], f"{name}: d_name_spans"
    _same(got["users"], ref["d_users"], f"{name}: usernames")
    _same(got["bals"], ref["d_bals"], f"{name}: balances")


def test_a_name_over_the_cap_is_reported_and_nothing_written(gpu, files):
    for name, _, nc, problem in REFUSED:
        assert run_sort(*files[name])["problem"] == problem, name


SMALL = [c[0] for c in CASES if c[3] is None and (c[0] in {g[:-4] for g in cases.GOLDENS} or c[1].count("\n") - 1 <= 32)]


@pytest.mark.parametrize("name", SMALL)
def test_trees_against_the_oracle(gpu, files, name):
    from oracle import pyref as P
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, _level_first, _mont_to_int
    path, nc = files[name]
    ref = reference(path, nc)
    assert len(ref["sorted"]) <= 32
    tree = DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    assert tree.csv_ingest == "device"
    _, levels = P.mst_build([P.mst_entry(n, b) for n, b in ref["sorted"]])
    h = tree.d_h.cpu().numpy().reshape(-1, 32)
    b = tree.d_b.cpu().numpy().reshape(-1, 32 * nc)
    assert len(levels) == tree.depth + 1
    for lvl, nodes in enumerate(levels):
        first = _level_first(tree.depth, lvl)
        for i, (want_h, want_b) in enumerate(nodes):
            assert _mont_to_int(h[first + i]) == want_h, (name, lvl, i)
            assert [_mont_to_int(b[first + i][32 * c:32 * c + 32]) for c in range(nc)] == [v % P.R for v in want_b], (name, lvl, i)


# ============================================================================= from_csv_sorted
def _counting_parse(monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    parses = []
    real = M.parse_csv_to_entries
    monkeypatch.setattr(M, "parse_csv_to_entries", lambda *a: parses.append(a) or real(*a))
    return parses


@pytest.mark.parametrize("name", ACCEPTED)
def test_from_csv_sorted_on_the_device(gpu, files, name, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path, nc = files[name]
    ref = reference(path, nc)
    parses = _counting_parse(monkeypatch)
    tree = M.DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    assert tree.csv_ingest == "device" and tree.csv_fallback_reason is None and tree.is_sorted
    assert (tree.depth, tree.n_currencies, tree.cryptocurrencies) == (ref["depth"], nc, ref["crypto"])
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), ref[what], f"{name}: {what}")
    tree.root()
    n = len(ref["sorted"])
    sorted_names = [e[0] for e in ref["sorted"]]
    first = {}
    for i, nm in enumerate(sorted_names):
        first.setdefault(nm, i)
    some = sorted({0, 1, n // 2, n - 1} & set(range(n)))
    for i in some:
        assert tree.index_of_username(sorted_names[i]) == first[sorted_names[i]]
    assert tree.indices_of_usernames(sorted_names) == [first[nm] for nm in sorted_names]      # every present name, duplicates their first leaf
    proof = tree.generate_proof(some[-1])
    assert proof["entry"] == ref["padded"][some[-1]]
    if (1 << tree.depth) > n:
        assert tree.generate_proof(n)["entry"] == (None, [0] * nc)
    new = [[7 * j + c + 1 for c in range(nc)] for j in range(len(some))]
    tree.update_leaves([(sorted_names[i], bal) for i, bal in zip(some, new)])
    assert parses == []                                       # none of this read a row on the host
    changed = list(ref["padded"])
    for i, bal in zip(some, new):
        changed[first[sorted_names[i]]] = (sorted_names[i], bal)
    assert tree.generate_proof(first[sorted_names[some[0]]])["entry"] == changed[first[sorted_names[some[0]]]] and parses == []
    assert tree.entries == changed and len(parses) == 1
    host = [e for e in changed if e[0] is not None]
    assert [e[0] for e in host] == sorted_names
    assert tree.index_of_username(sorted_names[n // 2]) == first[sorted_names[n // 2]] and len(parses) == 1     # the host's way now


def test_entries_equal_the_host_trees_with_one_parse(gpu, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path = os.path.join(GOLDEN, "entry_16.csv")
    host = M.MerkleSumTree.from_csv_sorted(path, 2, 8)
    parses = _counting_parse(monkeypatch)
    tree = M.DeviceMerkleSumTree.from_csv_sorted(path, 2, 8)
    _same(tree.root()[0], host.root()[0], "root hash, host tree")
    _same(tree.root()[1], host.root()[1], "root balances, host tree")
    name = host.entries[5][0]
    assert tree.index_of_username(name) == host.index_of_username(name) == 5
    proof = tree.generate_proof(5)
    want = host.generate_proof(5)
    assert proof["entry"] == want["entry"] and proof["path_indices"] == want["path_indices"]
    _same(proof["leaf"][0], want["leaf"][0], "leaf hash")
    assert host.verify_proof(dict(want, **{k: proof[k] for k in ("sibling_leaf_node_hash_preimage", "sibling_middle_node_hash_preimages")}))
    assert parses == []
    assert tree.entries == host.entries and len(parses) == 1
    assert tree.cryptocurrencies == host.cryptocurrencies and tree.is_sorted and host.is_sorted


def _outcome(make):
    try:
        tree = make()
    except Exception as e:      # whatever today's path raises is what the new one must raise
        return ("raised", type(e), str(e)), None
    h, b = tree.root()
    return ("root", bytes(h), bytes(b)), tree


def _todays_sorted(path, nc):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries
    entries, _ = parse_csv_to_entries(path, nc)
    entries.sort(key=lambda e: e[0].encode())
    return DeviceMerkleSumTree.from_entries(entries, nc, is_sorted=True)


HOST_FILES = {
    "quoted_name": cases.header(2) + 'zed,1,2\n"amy",3,4\nbob,5,6\n',
    "bad_balance": cases.header(2) + "zed,1,2\namy,x,4\n",
}


@pytest.mark.parametrize("name", [c[0] for c in REFUSED] + list(HOST_FILES))
def test_from_csv_sorted_on_the_host(gpu, files, name, tmp_path):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    path, nc = files[name] if name in files else (cases.write_case(tmp_path, name, HOST_FILES[name]), 2)
    none, reason = DeviceMerkleSumTree._from_csv_on_device(path, nc, sorted_leaves=True)
    assert none is None and isinstance(reason, str) and reason
    if name in files:
        assert reason == f"row {REFUSED[0][3][0]}: name too long for the device sort"
    want, want_tree = _outcome(lambda: _todays_sorted(path, nc))
    got, tree = _outcome(lambda: DeviceMerkleSumTree.from_csv_sorted(path, nc, 8))
    assert got == want, name
    if tree is not None:
        assert tree.csv_ingest == "host" and tree.csv_fallback_reason == reason and tree.is_sorted
        assert tree.entries == want_tree.entries
        for what in ("d_users", "d_bals", "d_h", "d_b"):
            _same(getattr(tree, what).cpu().numpy(), getattr(want_tree, what).cpu().numpy(), f"{name}: {what}")
    else:
        assert name == "bad_balance"


# ============================================================================= lookup by name
def _arrays(tree):
    return {what: getattr(tree, what).cpu().numpy().copy() for what in ("d_users", "d_bals", "d_h", "d_b")}


def test_find_present_duplicate_and_absent_names(gpu, files, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    parses = _counting_parse(monkeypatch)
    path, nc = files["duplicates_a_tile_apart"]
    ref = reference(path, nc)
    sorted_names = [e[0] for e in ref["sorted"]]
    tree = M.DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    assert tree.csv_ingest == "device"
    assert sorted_names.count("dup") == 3 and sorted_names.count("Zed") == 3
    assert tree.index_of_username("dup") == sorted_names.index("dup")
    assert tree.index_of_username("Zed") == sorted_names.index("Zed")
    assert "" not in sorted_names
    below = sorted_names[0][:-1] if len(sorted_names[0]) > 1 else chr(ord(sorted_names[0]) - 1)      # a proper prefix comes first
    absent = ["", below, sorted_names[-1] + "0", "\x7f" * 12, "q" * (CAP + 1), "zoé", "dup\x01", "du"]
    assert all(a not in sorted_names for a in absent) and below.encode() < sorted_names[0].encode()
    for a in absent:
        with pytest.raises(KeyError, match="Username not found"):
            tree.index_of_username(a)
    before = _arrays(tree)
    root = tree.root()
    for batch in ([sorted_names[3], "nobody at all"], ["", sorted_names[0]]):
        with pytest.raises(KeyError, match="Username not found"):
            tree.indices_of_usernames(batch)
        with pytest.raises(KeyError, match="Username not found"):
            tree.update_leaves([(nm, [1, 2]) for nm in batch])
    with pytest.raises(ValueError):
        tree.update_leaves([(sorted_names[3], [1, 2, 3])])        # a wrong number of balances: refused as ever, nothing changed
    after = _arrays(tree)
    for what in before:
        _same(after[what], before[what], f"{what} after refused batches")
    _same(tree.root()[0], root[0], "root")
    assert tree.indices_of_usernames([]) == [] and parses == []
    # the empty name where it is present: the prefix chain holds it, as its first leaf
    path, nc = files["prefix_chain"]
    chain = M.DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    assert chain.indices_of_usernames(["", "a", "a" * CAP, "aaa"]) == [0, 1, CAP, 3]
    with pytest.raises(KeyError, match="Username not found"):
        chain.index_of_username("a" * (CAP + 1))
    assert parses == []


def test_update_by_name_equals_a_fresh_tree(gpu, files, monkeypatch):
    update_by_name_equals_a_fresh_tree(files[f"random_{TILE + 1}"], (0, 1, 777, TILE // 2, TILE - 1, TILE), monkeypatch)


def update_by_name_equals_a_fresh_tree(file, leaves, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path, nc = file
    ref = reference(path, nc)
    sorted_names = [e[0] for e in ref["sorted"]]
    first = {}
    for i, nm in enumerate(sorted_names):
        first.setdefault(nm, i)
    picked = [sorted_names[i] for i in leaves]
    updates = [(nm, [10 ** 20 + 3 * j, 5 * j + 1]) for j, nm in enumerate(picked)] + [(picked[2], [42, 43])]      # a name twice: the last stays
    parses = _counting_parse(monkeypatch)
    tree = M.DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    tree.update_leaves(updates[:3])
    tree.update_leaf(*updates[3])
    tree.update_leaves(updates[4:])
    assert parses == []
    changed = list(ref["sorted"])
    for nm, bal in updates:
        changed[first[nm]] = (nm, bal)
    fresh = M.DeviceMerkleSumTree.from_entries(changed, nc, is_sorted=True)
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), getattr(fresh, what).cpu().numpy(), what)
    assert tree.entries == fresh.entries and len(parses) == 1


# ============================================================================= files beyond one step of a pass's scan
@pytest.fixture(scope="module")
def large_files(tmp_path_factory):
    """{case name: (path, n_currencies)} for LARGE, generated from their fixed seeds"""
    d = tmp_path_factory.mktemp("mst_sort_gpu_large")
    return {name: (cases.write_case(d, name, cases.large(name, TILE)[0]), cases.large(name, TILE)[1]) for name in cases.LARGE}


@pytest.mark.parametrize("name", cases.LARGE)
def test_large_order_spans_and_leaf_inputs(gpu, large_files, name):
    """order, name spans, usernames and balances as for the small files; the scratch is ss_mst_sort_scratch's at these sizes"""
    path, _ = large_files[name]
    n = int(name.rsplit("_", 1)[1])
    assert cases.scan_steps(n, TILE) == {32768: 1, 32769: 2, 65537: 3, 196609: 7}[n]
    if name == "hex64_32769":                                 # the CSV reader's scan takes its second round in the same call
        assert -(-(os.path.getsize(path) - len(cases.header(2, eol="\r\n"))) // 4096) > 1024
    order_spans_and_leaf_inputs(large_files[name], name)


@pytest.mark.parametrize("name", ["rows_32769", "hex64_32769", "pool_300_32769", "high_bytes_65537", "rows_196609"])
def test_large_from_csv_sorted(gpu, large_files, name):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    path, nc = large_files[name]
    ref = reference(path, nc)
    tree = DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    assert tree.csv_ingest == "device" and tree.csv_fallback_reason is None and tree.is_sorted and tree.depth == ref["depth"]
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), ref[what], f"{name}: {what}")


def test_find_pool_names_across_all_tiles(gpu, large_files, monkeypatch):
    """every name of the pool -> its first leaf, in one call of more than 256 queries and before any parse; absent names below,
    between and above the pool's"""
    from circuits_halo2_amd import merkle_sum_tree as M
    path, nc = large_files["pool_300_32769"]
    ref = reference(path, nc)
    file_names = [e[0] for e in ref["entries"]]
    sorted_names = [e[0] for e in ref["sorted"]]
    first = {}
    for i, nm in enumerate(sorted_names):
        first.setdefault(nm, i)
    pool = sorted(first, key=str.encode)
    assert len(pool) == 300
    parses = _counting_parse(monkeypatch)
    tree = M.DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
    assert tree.csv_ingest == "device"
    queries = pool + file_names[:5] + file_names[-5:] + [sorted_names[-1], sorted_names[0]]     # the first and the last tile's, of file and leaves
    assert len(queries) > 256
    assert tree.indices_of_usernames(queries) == [first[nm] for nm in queries]
    assert min(first.values()) == 0 and max(first.values()) > 15 * TILE                       # leaves of the first tile and of the 16th
    between = [pool[k] + "\x01" for k in (0, 150, 298)] + [pool[150][:-1] + chr(ord(pool[150][-1]) - 1) + "~"]
    absent = ["", "\x01", pool[0][:-1] if len(pool[0]) > 1 else "#"] + between + [pool[-1] + "0", "~", "\x7f" * CAP]
    assert all(a not in first for a in absent)
    for a in absent:
        with pytest.raises(KeyError, match="Username not found"):
            tree.indices_of_usernames(pool + [a])
    assert parses == []


def test_large_update_by_name_equals_a_fresh_tree(gpu, large_files, monkeypatch):
    """users of the last tile -- the last leaves, and the name of the file's last row -- in a tree of 17 tiles"""
    path, nc = large_files["rows_32769"]
    ref = reference(path, nc)
    n = len(ref["sorted"])
    last_row = [e[0] for e in ref["sorted"]].index(ref["entries"][-1][0])
    update_by_name_equals_a_fresh_tree(large_files["rows_32769"], (n - 1, n - 2, last_row, 16 * TILE - 1, TILE, 0), monkeypatch)


# ============================================================================= stream order
N_STREAM = 1000                 # rows of the stream-order files: not a multiple of anything, one tile
MIN_DELAY_MS, MAX_DELAY_MS, MARGIN = 20.0, 200.0, 10.0
HEAD = "username,balance_ETH_ETH,balance_USDT_ETH\n"


def _stream_entries(seed, which):
    """N_STREAM entries with names and balances of fixed widths, so that real and decoy share their row starts; every name and
    balance differs between the two, and the names are in two different random orders"""
    import random
    rng = random.Random(1000 * seed + which)
    numbers = list(range(N_STREAM))
    rng.shuffle(numbers)
    tag = "rd"[which]
    return [(f"{tag}{k:06d}{seed % 10}", [10 ** 11 + (7919 * i + 13 * c + 1000 * which + seed) % 10 ** 11 for c in range(2)])
            for i, k in enumerate(numbers)]


@functools.lru_cache(maxsize=None)
def _stream_case(seed):
    """(texts, expected) of real and decoy: the text, d_order, d_name_spans, usernames, balances as bytes"""
    out = []
    for which in (0, 1):
        entries = _stream_entries(seed, which)
        lines = [f"{name},{bal[0]},{bal[1]}\n" for name, bal in entries]
        text = np.frombuffer((HEAD + "".join(lines)).encode(), dtype=np.uint8).copy()
        starts = np.concatenate([[0], np.cumsum([len(l) for l in lines])[:-1]])
        order = cases.stable_order([name.encode() for name, _ in entries])
        spans = np.array([[starts[i], starts[i] + len(entries[i][0])] for i in order], dtype=np.uint32)
        users, bals = sc._entry_words([entries[i] for i in order])
        pad = 1024 - N_STREAM
        want = {"order": np.array(order, dtype=np.uint32).view(np.uint8), "name_spans": spans.view(np.uint8).reshape(-1),
                "usernames": np.concatenate([np.asarray(users, dtype=np.uint8).reshape(-1), np.zeros(32 * pad, dtype=np.uint8)]),
                "balances": np.concatenate([np.asarray(bals, dtype=np.uint8).reshape(-1), np.zeros(64 * pad, dtype=np.uint8)])}
        out.append((text, want, entries, order))
    assert out[0][0].size == out[1][0].size and out[0][3] != out[1][3]
    return out


@pytest.fixture(scope="module")
def sleep_cycles_per_ms(gpu):
    """torch.cuda._sleep calibrated against events, as tests/test_gpu_stream_order.py does"""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(1_000_000)
    probe = 20_000_000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    with torch.cuda.stream(s):
        torch.cuda._sleep(probe)
    e1.record(s)
    torch.cuda.synchronize()
    return probe / e0.elapsed_time(e1)


def _delay(per_ms, issue):
    """the module's rule: the sequence timed undelayed between two events (the better of two), ten times that within 20 .. 200 ms"""
    import torch
    s = torch.cuda.Stream()
    times = []
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        issue(s, 0)
        e1.record(s)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = min(MAX_DELAY_MS, max(MIN_DELAY_MS, MARGIN * min(times)))
    return int(ms * per_ms), f"{min(times):.3f} ms undelayed, {per_ms:.0f} _sleep cycles per ms, delay {ms:.1f} ms = {int(ms * per_ms)} cycles"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _scan_of(text):
    """the tile scratch a scan of this layout leaves, complete before the test's first wait"""
    import torch
    from circuits_halo2_amd import ffi
    d_text = _dev(text)
    tiles = torch.zeros(4 * (-(-(text.size - len(HEAD)) // 4096) + 2), dtype=torch.uint8, device="cuda")
    n_rows, flags = C.c_uint64(0), C.c_uint32(0)
    ffi.check(ffi.lib().sg_mst_csv_scan_dev(ffi.dev_ptr(d_text), text.size, len(HEAD), ffi.dev_ptr(tiles), C.byref(n_rows), C.byref(flags), None))
    torch.cuda.synchronize()
    assert (n_rows.value, flags.value) == (N_STREAM, 0)
    return tiles


def _judge(got, want, decoy, what):
    for n in sorted(want):
        if np.array_equal(got[n], want[n]):
            continue
        g, w, d = sc.rows_of(got[n]), sc.rows_of(want[n]), sc.rows_of(decoy[n])
        assert g.shape == w.shape, f"{what}: {n} has {got[n].size} bytes, expected {want[n].size}"
        bad = (g != w).any(axis=1)
        as_decoy = int(((g == d).all(axis=1) & bad).sum())
        stale = int(((g == sc.FILL).all(axis=1) & bad).sum())
        raise AssertionError(f"{what}: {n}: {int(bad.sum())} of {bad.size} rows differ from the result for the real inputs, first at row "
                             f"{int(np.argmax(bad))}; {as_decoy} of them are the decoy's result (the call missed the producer, or read its inputs "
                             f"after it returned), {stale} are 0x5A (the output had not joined the stream)")


def test_sorted_entries_are_ordered_on_their_stream(gpu, sleep_cycles_per_ms):
    """the sequence of tests/test_gpu_stream_order.py on two fresh streams made one after the other: the decoy text in the buffer
    and 0x5A in the outputs; on S a delay, the real text copied in, the call, the outputs copied to consumers, the decoy written
    back -- no host wait in between but the call's own for its problem word"""
    import torch
    from circuits_halo2_amd import ffi
    S = ffi.snapshot_lib()
    sort_bytes = C.c_uint64(0)
    ffi.check(S.ss_mst_sort_scratch(N_STREAM, C.byref(sort_bytes)))
    sizes = {"order": 4 * N_STREAM, "name_spans": 8 * N_STREAM, "usernames": 32 * 1024, "balances": 64 * 1024}

    def make(seed):
        (real, want, _, _), (decoy, want_decoy, _, _) = _stream_case(seed)
        run = {"real": _dev(real), "decoy": _dev(decoy), "tiles": _scan_of(real), "want": want, "want_decoy": want_decoy, "size": real.size}
        run["text"] = run["decoy"].clone()
        run["outs"] = {k: torch.full((v,), sc.FILL, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
        run["work"] = {"spans": torch.full((16 * (N_STREAM + 1 + 2 * N_STREAM * 3),), sc.FILL, dtype=torch.uint8, device="cuda"),
                       "sort": torch.full((sort_bytes.value,), sc.FILL, dtype=torch.uint8, device="cuda")}
        run["consumer"] = {k: torch.zeros_like(t) for k, t in run["outs"].items()}
        return run

    def issue(run, stream, cycles):
        with torch.cuda.stream(stream):
            if cycles:
                torch.cuda._sleep(cycles)
            run["text"].copy_(run["real"], non_blocking=True)
            problem = C.c_uint64(1 << 40)
            o, w = run["outs"], run["work"]
            ffi.check(S.ss_mst_csv_entries_sorted_dev(ffi.dev_ptr(run["text"]), run["size"], len(HEAD), ffi.dev_ptr(run["tiles"]), ord(","), 2,
                                                      N_STREAM, 1024, ffi.dev_ptr(w["spans"]), ffi.dev_ptr(w["sort"]), ffi.dev_ptr(o["order"]),
                                                      ffi.dev_ptr(o["name_spans"]), ffi.dev_ptr(o["usernames"]), ffi.dev_ptr(o["balances"]),
                                                      C.byref(problem), ffi.current_stream_ptr()))
            run["problem"] = problem.value
            for k in o:
                run["consumer"][k].copy_(o[k], non_blocking=True)
            run["text"].copy_(run["decoy"], non_blocking=True)

    timing = make(9)
    cycles, report = _delay(sleep_cycles_per_ms, lambda s, c: issue(timing, s, c))
    print(f"\nstream order, ss_mst_csv_entries_sorted_dev: {report}")
    for j, stream in enumerate([torch.cuda.Stream(), torch.cuda.Stream()]):
        run = make(j)
        torch.cuda.synchronize()
        issue(run, stream, cycles)
        torch.cuda.synchronize()
        assert run["problem"] == 0, report
        got = {k: t.cpu().numpy() for k, t in run["consumer"].items()}
        _judge(got, run["want"], run["want_decoy"], f"ss_mst_csv_entries_sorted_dev, stream {j}; {report}")


def test_find_names_is_ordered_on_its_stream(gpu, sleep_cycles_per_ms):
    """the same for ss_mst_find_names: the decoy's text and spans in the buffers, the real ones copied in behind a delay, the
    call (which waits for the stream before it returns: its result is the host's), the decoy written back"""
    import torch
    from circuits_halo2_amd import ffi
    S = ffi.snapshot_lib()

    def make(seed):
        (real, want, entries, order), (decoy, want_decoy, _, _) = _stream_case(seed)
        names = [entries[i][0] for i in order[::16]] + ["nobody at all"]         # 63 present names and an absent one
        packed = [nm.encode() for nm in names]
        off = np.zeros(len(packed) + 1, dtype=np.uint64)
        np.cumsum([len(p) for p in packed], out=off[1:])
        run = {"size": real.size, "names": np.frombuffer(b"".join(packed), dtype=np.uint8).copy(), "off": off, "m": len(packed),
               "want": {"host": np.array(list(range(0, N_STREAM, 16)) + [ABSENT], dtype=np.uint32).view(np.uint8)},
               "want_decoy": {"host": np.full(len(packed), ABSENT, dtype=np.uint32).view(np.uint8)}}
        for k, (r, d) in {"text": (real, decoy), "spans": (want["name_spans"], want_decoy["name_spans"])}.items():
            run[k + "_real"], run[k + "_decoy"] = _dev(r), _dev(d)
            run[k] = run[k + "_decoy"].clone()
        return run

    def issue(run, stream, cycles):
        with torch.cuda.stream(stream):
            if cycles:
                torch.cuda._sleep(cycles)
            for k in ("text", "spans"):
                run[k].copy_(run[k + "_real"], non_blocking=True)
            found = np.full(run["m"], sc.FILL, dtype=np.uint32)
            ffi.check(S.ss_mst_find_names(ffi.dev_ptr(run["text"]), run["size"], len(HEAD), ffi.dev_ptr(run["spans"]), N_STREAM,
                                          ffi.ptr(run["names"]), ffi.ptr(run["off"]), run["m"], ffi.ptr(found), ffi.current_stream_ptr()))
            run["found"] = found.view(np.uint8).copy()       # the host's when the call is back
            for k in ("text", "spans"):
                run[k].copy_(run[k + "_decoy"], non_blocking=True)

    timing = make(9)
    cycles, report = _delay(sleep_cycles_per_ms, lambda s, c: issue(timing, s, c))
    print(f"\nstream order, ss_mst_find_names: {report}")
    for j, stream in enumerate([torch.cuda.Stream(), torch.cuda.Stream()]):
        run = make(j)
        torch.cuda.synchronize()
        issue(run, stream, cycles)
        torch.cuda.synchronize()
        _judge({"host": run["found"]}, run["want"], run["want_decoy"], f"ss_mst_find_names, stream {j}; {report}")
