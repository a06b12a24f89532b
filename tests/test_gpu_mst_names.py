"""The name index beside a tree in file order and the duplicate-username report on the device (csrc/mst_names.h, the kernels in
csrc/mst_names.cuh; ss_mst_csv_name_index_dev, ss_mst_find_leaves and ss_mst_duplicate_names_dev of include/summa_snapshot.h), over
the list of mst_names_cases.py and its model.

Through the ABI, per case: the three arrays of the index against Python's stable order of the names' bytes; every distinct name
and two absent ones through ss_mst_find_leaves against list.index -- the reference's position() --; the report against the model,
summary and both lists word for word, at every cap, with the order (leaves in file order) and without it (a sorted tree), and
with what lies behind the listed entries untouched.  Through Python: `from_csv(name_index=True)` builds the tree `from_csv` builds
and answers by name without a host parse.  The report once more at mst_names_cases.BIG rows, 66 groups of its compaction,
against the numpy model: the scatter's wave sums 64 group totals a trip of its loop.  Both new device calls are held to the stream-order contract with the sequence of
tests/test_gpu_mst_sort.py."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

import mst_names_cases as cases
import mst_sort_cases as sort_cases
from test_gpu_mst_sort import HEAD, N_STREAM, _delay, _dev, _scan_of, sleep_cycles_per_ms  # noqa: F401  (the fixture and its rule)

pytestmark = pytest.mark.gpu

SORT_TILE, CAP = 2048, 64
CASES = cases.cases(SORT_TILE)
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
    assert (cap.value, tile.value) == (CAP, SORT_TILE)
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{case name: (path, n_currencies, the names in file order)}; the large case is generated from its fixed seed"""
    d = tmp_path_factory.mktemp("mst_names_gpu")
    out = {c[0]: (cases.write_case(d, c[0], c[1]), c[2], cases.names_of(c[1])) for c in CASES}
    text, nc = sort_cases.large(cases.LARGE, SORT_TILE)
    out[cases.LARGE] = (cases.write_case(d, cases.LARGE, text), nc, cases.names_of(text))
    return out


def _guarded(n_bytes):
    import torch
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def _words(t, n):
    return t[:4 * n].cpu().numpy().view(np.uint32)


def run_index(path, nc):
    """scan + the index call, every buffer it writes followed by 64 guard bytes that must come back untouched ->
    {"n", "problem", "body", "order", "spans", "leafspans"} and, for the calls behind it, the device buffers under "dev" """
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
    ffi.check(S.ss_mst_sort_scratch(n, C.byref(sort_bytes)))
    sizes = {"spans": 16 * (n + 1 + 2 * n * (1 + nc)), "sort": sort_bytes.value, "order": 4 * n, "name_spans": 8 * n, "leaf_spans": 8 * n}
    b = {k: _guarded(v) for k, v in sizes.items()}
    ffi.check(S.ss_mst_csv_name_index_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), delim, nc, n, ffi.dev_ptr(b["spans"]),
                                          ffi.dev_ptr(b["sort"]), ffi.dev_ptr(b["order"]), ffi.dev_ptr(b["name_spans"]),
                                          ffi.dev_ptr(b["leaf_spans"]), C.byref(problem), stream))
    torch.cuda.current_stream().synchronize()
    for k, used in sizes.items():
        assert (b[k][used:] == GUARD).all(), f"the bytes behind {k} changed"
    out = {"n": n, "problem": (problem.value >> 8, problem.value & 0xff), "body": data[body_off:].tobytes()}
    if problem.value:
        for k in ("order", "name_spans", "leaf_spans"):
            assert (b[k] == GUARD).all(), f"{k} was written behind a problem"
        return out
    out.update(order=_words(b["order"], n).tolist(), spans=_words(b["name_spans"], 2 * n).reshape(-1, 2).tolist(),
               leafspans=_words(b["leaf_spans"], 2 * n).reshape(-1, 2).tolist(),
               dev={"text": text, "size": size, "body_off": body_off, "order": b["order"], "name_spans": b["name_spans"], "buf": buf})
    return out


def find_leaves(dev, n, queries):
    from circuits_halo2_amd import ffi
    off = np.zeros(len(queries) + 1, dtype=np.uint64)
    np.cumsum([len(q) for q in queries], out=off[1:])
    name_bytes = np.frombuffer(b"".join(queries) or b"\0", dtype=np.uint8).copy()
    found = np.full(len(queries), 0x5A5A5A5A, dtype=np.uint32)
    ffi.check(ffi.snapshot_lib().ss_mst_find_leaves(ffi.dev_ptr(dev["text"]), dev["size"], dev["body_off"], ffi.dev_ptr(dev["name_spans"]),
                                                    ffi.dev_ptr(dev["order"]), n, ffi.ptr(name_bytes), ffi.ptr(off), len(queries),
                                                    ffi.ptr(found), ffi.current_stream_ptr()))
    return found.tolist()


def report(dev, n, cap, ordered, stream=None):
    """ss_mst_duplicate_names_dev -> the shape of cases.model; both lists are 16 entries longer than cap, and those and the
    entries behind the listed ones must come back as they were"""
    import torch
    from circuits_halo2_amd import ffi
    S = ffi.snapshot_lib()
    scratch_bytes = C.c_uint64(0)
    ffi.check(S.ss_mst_duplicate_names_scratch(n, C.byref(scratch_bytes)))
    scratch = _guarded(scratch_bytes.value)
    lists = {k: _guarded(4 * cap) for k in ("shadowed", "first")}
    summary = (C.c_uint64 * 3)(71, 72, 73)
    ffi.check(S.ss_mst_duplicate_names_dev(ffi.dev_ptr(dev["text"]), dev["size"], dev["body_off"], ffi.dev_ptr(dev["name_spans"]),
                                           ffi.dev_ptr(dev["order"]) if ordered else None, n,
                                           ffi.dev_ptr(lists["shadowed"]) if cap else None, ffi.dev_ptr(lists["first"]) if cap else None, cap,
                                           ffi.dev_ptr(scratch), summary, ffi.current_stream_ptr() if stream is None else stream))
    torch.cuda.current_stream().synchronize()
    listed = int(summary[2])
    assert (scratch[scratch_bytes.value:] == GUARD).all(), "the bytes behind d_scratch changed"
    for k, t in lists.items():
        assert (t[4 * listed:] == GUARD).all(), f"{k}: an entry behind the {listed} listed ones was written (cap {cap})"
    return {"summary": [int(x) for x in summary], "shadowed": _words(lists["shadowed"], listed).tolist(),
            "first": _words(lists["first"], listed).tolist()}


# ============================================================================= the entry points over the list
@pytest.mark.parametrize("name", ACCEPTED + [cases.LARGE])
def test_index_lookup_and_report_against_the_model(gpu, files, name):
    path, nc, names = files[name]
    got = run_index(path, nc)
    n = len(names)
    want = sort_cases.stable_order(names)
    assert got["problem"] == (0, 0) and got["n"] == n
    assert got["order"] == want, f"{name}: d_order is not Python's stable order"
    assert [got["body"][b:e] for b, e in got["spans"]] == [names[r] for r in want], f"{name}: d_name_spans"
    assert [got["body"][b:e] for b, e in got["leafspans"]] == names, f"{name}: d_leaf_name_spans"
    # every distinct name and two absent ones: the lowest file row, list.index
    first = cases.first_rows(names)
    distinct = sorted(first)
    assert all(first[nm] == names.index(nm) for nm in distinct[:64])
    absent = [b"\x7f" * (CAP + 1), (distinct[-1] + b"~")]
    assert all(a not in first for a in absent)
    assert find_leaves(got["dev"], n, distinct + absent) == [first[nm] for nm in distinct] + [ABSENT, ABSENT], name
    # the report, with the order and without
    count = cases.model(names)["summary"][1]
    for cap in cases.caps_for(count):
        for ordered in (True, False):
            assert report(got["dev"], n, cap, ordered) == cases.model(names, cap, ordered), (name, cap, ordered)


def test_a_name_over_the_cap_is_reported_and_nothing_written(gpu, files):
    for name, _, _, problem in REFUSED:
        assert problem == (2, 7) and run_index(*files[name][:2])["problem"] == (2, 7), name


# ============================================================================= from_csv(name_index=True)
def _no_parse(monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    def refuse(*a):
        raise AssertionError("parse_csv_to_entries was called")
    monkeypatch.setattr(M, "parse_csv_to_entries", refuse)


def _same(got, want, what):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert g.size == w.size and (g == w).all(), what


@pytest.mark.parametrize("name", ["edges_257", "duplicates_a_tile_apart", "empty_name_twice", "run3_across_16386"])
def test_from_csv_with_the_index_is_from_csv_and_answers_by_name_without_a_parse(gpu, files, name, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path, nc, names = files[name]
    plain = M.DeviceMerkleSumTree.from_csv(path, nc, 8)
    assert plain.csv_ingest == "device" and not plain.has_name_index and plain.name_index_reason is None and plain._index_dev is None
    host = M.DeviceMerkleSumTree.from_entries(M.parse_csv_to_entries(path, nc)[0], nc)      # the host's path, for the update below
    _no_parse(monkeypatch)
    tree = M.DeviceMerkleSumTree.from_csv(path, nc, 8, name_index=True)
    assert tree.csv_ingest == "device" and tree.has_name_index and tree.name_index_reason is None and not tree.is_sorted
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), getattr(plain, what).cpu().numpy(), f"{name}: {what}")
    strs = [nm.decode() for nm in names]
    n = len(strs)
    some = sorted({0, 1, n // 2, n - 1} & set(range(n)))
    for r in some:
        assert tree.index_of_username(strs[r]) == strs.index(strs[r])
    distinct = sorted(set(strs))
    first = {nm.decode(): r for nm, r in cases.first_rows(names).items()}
    assert tree.indices_of_usernames(distinct) == [first[nm] for nm in distinct]
    with pytest.raises(KeyError, match="Username not found"):
        tree.indices_of_usernames([distinct[0], "nobody at all"])
    updates = [(strs[r], [10 ** 20 + 3 * j, 5 * j + 1]) for j, r in enumerate(some)]
    tree.update_leaves(updates[:2])
    tree.update_leaf(*updates[-1])
    tree.update_leaves(updates[2:])
    host.update_leaves(updates)
    _same(tree.root()[0], host.root()[0], f"{name}: the root's hash after updates by name")
    _same(tree.root()[1], host.root()[1], f"{name}: the root's balances after updates by name")
    _same(tree.d_h.cpu().numpy(), host.d_h.cpu().numpy(), f"{name}: node hashes after updates by name")
    changed = {first[nm]: bal for nm, bal in updates}
    probe = first[strs[some[-1]]]
    assert tree.generate_proof(probe)["entry"] == (strs[probe], changed[probe])
    untouched = [r for r in range(n) if r not in changed][0]
    assert tree.generate_proof(untouched)["entry"] == (strs[untouched], [1000 * untouched + 1, 1000 * untouched + 2])
    if (1 << tree.depth) > n:
        assert tree.generate_proof(n)["entry"] == (None, [0] * nc)
    dups = tree.duplicate_names()
    want = cases.model(names)
    assert [dups.n_repeated_names, dups.n_shadowed, len(dups.shadowed)] == want["summary"] and dups.ok == (want["summary"][1] == 0)
    assert dups.shadowed.tolist() == want["shadowed"] and dups.first.tolist() == want["first"]
    assert dups.shadowed.dtype == dups.first.dtype == np.uint32
    assert tree.duplicate_names(cap=1).shadowed.tolist() == want["shadowed"][:1] and tree.duplicate_names(cap=0).n_shadowed == want["summary"][1]
    named = tree.named_groups(dups, limit=3)
    assert named == [(strs[h], [h] + ls) for h, ls in list(dups.groups().items())[:3]]
    assert tree._entries is None                              # none of this made the entries


def test_indices_on_the_golden_equal_the_host_trees(gpu, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path = os.path.join(GOLDEN, "entry_16.csv")
    host = M.MerkleSumTree.from_csv(path, 2, 8)
    _no_parse(monkeypatch)
    tree = M.DeviceMerkleSumTree.from_csv(path, 2, 8, name_index=True)
    _same(tree.root()[0], host.root()[0], "root hash, host tree")
    names = [e[0] for e in host.entries if e[0] is not None]
    assert len(names) == 16
    assert [tree.index_of_username(nm) for nm in names] == [host.index_of_username(nm) for nm in names] == list(range(16))
    assert tree.generate_proof(5)["entry"] == host.entries[5]
    assert tree.duplicate_names().ok and host.duplicate_names().ok


def test_a_sorted_trees_report_agrees_with_the_model(gpu, files, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    _no_parse(monkeypatch)
    for name in ("edges_257", "duplicates_a_tile_apart"):
        path, nc, names = files[name]
        tree = M.DeviceMerkleSumTree.from_csv_sorted(path, nc, 8)
        assert tree.csv_ingest == "device" and tree.has_name_index and tree.is_sorted
        want = cases.model(names, None, in_file_order=False)
        dups = tree.duplicate_names()
        assert [dups.n_repeated_names, dups.n_shadowed, len(dups.shadowed)] == want["summary"], name
        assert dups.shadowed.tolist() == want["shadowed"] and dups.first.tolist() == want["first"], name
        by_name = sorted(nm.decode() for nm in names)
        assert tree.named_groups(dups, limit=2) == [(by_name[h], [h] + ls) for h, ls in list(dups.groups().items())[:2]]


def test_a_name_of_65_bytes_leaves_a_device_read_tree_without_an_index(gpu, files):
    from circuits_halo2_amd import merkle_sum_tree as M
    path, nc, names = files["name_of_65_bytes"]
    plain = M.DeviceMerkleSumTree.from_csv(path, nc, 8)
    tree = M.DeviceMerkleSumTree.from_csv(path, nc, 8, name_index=True)
    assert tree.csv_ingest == "device" and tree.csv_fallback_reason is None
    assert not tree.has_name_index and tree.name_index_reason == "row 2: name too long for the device sort"
    _same(tree.d_h.cpu().numpy(), plain.d_h.cpu().numpy(), "node hashes")
    assert tree.index_of_username("k") == 5 and tree.duplicate_names().ok      # the host's way: the entries are parsed


def test_a_host_read_file_says_why_it_has_no_index(gpu, tmp_path):
    from circuits_halo2_amd import merkle_sum_tree as M
    path = cases.write_case(tmp_path, "quoted_name", cases.header(2) + 'zed,1,2\n"amy",3,4\nzed,5,6\n')
    tree = M.DeviceMerkleSumTree.from_csv(path, 2, 8, name_index=True)
    assert tree.csv_ingest == "host" and not tree.has_name_index and tree.name_index_reason == tree.csv_fallback_reason != None  # noqa: E711
    dups = tree.duplicate_names()
    assert (dups.n_repeated_names, dups.n_shadowed, dups.shadowed.tolist(), dups.first.tolist()) == (1, 1, [2], [0])


# ============================================================================= the report past 64 groups of its compaction
@pytest.fixture(scope="module")
def big_file(tmp_path_factory):
    """BIG rows of 7-digit names, repeated at both sides of the edges and at the start of every group: (path, keys in file order)"""
    keys = cases.big_keys()
    rows = np.arange(keys.size, dtype=np.int64)
    path = tmp_path_factory.mktemp("mst_names_big") / "big.csv"
    return cases.write_fixed(path, 2, cases.fixed_rows(keys, cases.BIG_WIDTH, [10_000_000 + 3 * rows, 20_000_000 + 7 * rows])), keys


@pytest.fixture(scope="module")
def big_trees(gpu, big_file):
    """{ordered: the tree}: `from_csv(name_index=True)`, leaves in file order, and `from_csv_sorted`, of the one file"""
    from circuits_halo2_amd import merkle_sum_tree as M
    path, keys = big_file
    trees = {True: M.DeviceMerkleSumTree.from_csv(path, 2, 8, name_index=True), False: M.DeviceMerkleSumTree.from_csv_sorted(path, 2, 8)}
    for ordered, tree in trees.items():
        assert tree.csv_ingest == "device" and tree.has_name_index and tree.is_sorted == (not ordered)
        assert (tree.depth, tree._names_dev()["n"]) == (21, cases.BIG)
    return trees


def report_np(d, n, cap, ordered):
    """report() over a tree's own index, the lists as numpy arrays: (summary, shadowed, first), each list with the 16 entries behind
    the cap, pre-filled"""
    import torch
    from circuits_halo2_amd import ffi
    S = ffi.snapshot_lib()
    scratch_bytes = C.c_uint64(0)
    ffi.check(S.ss_mst_duplicate_names_scratch(n, C.byref(scratch_bytes)))
    scratch = _guarded(scratch_bytes.value)
    lists = {k: _guarded(4 * cap) for k in ("shadowed", "first")}
    summary = (C.c_uint64 * 3)(71, 72, 73)
    ffi.check(S.ss_mst_duplicate_names_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_name_spans"]),
                                           ffi.dev_ptr(d["d_order"]) if ordered else None, n,
                                           ffi.dev_ptr(lists["shadowed"]) if cap else None, ffi.dev_ptr(lists["first"]) if cap else None, cap,
                                           ffi.dev_ptr(scratch), summary, ffi.current_stream_ptr()))
    torch.cuda.current_stream().synchronize()
    assert (scratch[scratch_bytes.value:] == GUARD).all(), "the bytes behind d_scratch changed"
    return [int(x) for x in summary], lists["shadowed"].cpu().numpy().view(np.uint32), lists["first"].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("ordered", [True, False], ids=["file_order", "sorted"])
def test_the_report_at_big_rows_agrees_with_the_numpy_model(gpu, big_file, big_trees, ordered):
    """66 groups of sorted positions: positions of group 64 sum 64 group totals in one full trip of the scatter's loop, all six
    shuffle steps carrying data; the two positions of group 65 take the second trip"""
    keys = big_file[1]
    tree = big_trees[ordered]
    d = tree._names_dev()
    order, same = cases.shadowed_positions(keys)
    assert np.array_equal(d["d_order"].cpu().numpy().view(np.uint32), order), "d_order is not numpy's stable order"
    full = cases.model_np(keys, None, ordered)
    count = full["summary"][1]
    inside_65 = int(np.count_nonzero(same[:65 * cases.GROUP_ROWS])) + 1
    assert same[cases.BIG - 2] and same[cases.BIG - 1] and inside_65 == count - 1
    for cap in sorted({0, 1, count, count - 1, count + 5, inside_65}):
        want = cases.model_np(keys, cap, ordered)
        summary, shadowed, first = report_np(d, cases.BIG, cap, ordered)
        assert summary == want["summary"], (cap, summary)
        listed = want["summary"][2]
        for what, got in (("shadowed", shadowed), ("first", first)):
            wrong = np.flatnonzero(got[:listed] != want[what])
            assert wrong.size == 0, (cap, what, "entry", int(wrong[0]), int(got[wrong[0]]), int(want[what][wrong[0]]))
            assert (got[listed:] == GUARD * 0x01010101).all(), f"{what}: an entry behind the {listed} listed ones was written (cap {cap})"
    dups = tree.duplicate_names()
    assert [dups.n_repeated_names, dups.n_shadowed, len(dups.shadowed)] == full["summary"]
    assert np.array_equal(dups.shadowed, full["shadowed"]) and np.array_equal(dups.first, full["first"])
    capped = tree.duplicate_names(cap=inside_65)
    assert np.array_equal(capped.shadowed, full["shadowed"][:inside_65]) and capped.n_shadowed == count


# ============================================================================= stream order
@functools.lru_cache(maxsize=None)
def _stream_case(seed):
    """real and decoy: texts of N_STREAM rows with the same row starts (names and balances of fixed widths), different names in
    different orders, and about 5 % of the rows repeated in each -> (text, names in file order) twice"""
    out = []
    for which in (0, 1):
        rng = random.Random(f"test_gpu_mst_names.stream.{seed}.{which}")
        numbers = [rng.randrange(N_STREAM - 50) for _ in range(N_STREAM)]
        tag = "rd"[which]
        names = [f"{tag}{k:06d}{seed % 10}" for k in numbers]
        lines = [f"{nm},{10 ** 11 + 7 * i + which},{10 ** 11 + 13 * i + seed}\n" for i, nm in enumerate(names)]
        out.append((np.frombuffer((HEAD + "".join(lines)).encode(), dtype=np.uint8).copy(), [nm.encode() for nm in names]))
    assert out[0][0].size == out[1][0].size
    return out


def test_the_index_and_the_report_are_ordered_on_their_stream(gpu, sleep_cycles_per_ms):
    """the sequence of tests/test_gpu_mst_sort.py on two fresh streams: the decoy text in the buffer and 0x5A in the outputs; on S a
    delay, the real text copied in, the index call and behind it -- no wait between -- the report over what it wrote, the outputs
    copied to consumers, the decoy written back.  The results must be the text's, not the decoy's."""
    import torch
    from circuits_halo2_amd import ffi
    S = ffi.snapshot_lib()
    n = N_STREAM
    sort_bytes, scratch_bytes = C.c_uint64(0), C.c_uint64(0)
    ffi.check(S.ss_mst_sort_scratch(n, C.byref(sort_bytes)))
    ffi.check(S.ss_mst_duplicate_names_scratch(n, C.byref(scratch_bytes)))
    sizes = {"order": 4 * n, "name_spans": 8 * n, "leaf_spans": 8 * n, "shadowed": 4 * n, "first": 4 * n}

    def make(seed):
        (real, names), (decoy, decoy_names) = _stream_case(seed)
        run = {"real": _dev(real), "decoy": _dev(decoy), "tiles": _scan_of(real), "size": real.size, "names": names, "decoy_names": decoy_names}
        run["text"] = run["decoy"].clone()
        run["outs"] = {k: torch.full((v,), GUARD, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
        run["work"] = {"spans": torch.full((16 * (n + 1 + 2 * n * 3),), GUARD, dtype=torch.uint8, device="cuda"),
                       "sort": torch.full((sort_bytes.value,), GUARD, dtype=torch.uint8, device="cuda"),
                       "scratch": torch.full((scratch_bytes.value,), GUARD, dtype=torch.uint8, device="cuda")}
        run["consumer"] = {k: torch.zeros_like(t) for k, t in run["outs"].items()}
        return run

    def issue(run, stream, cycles):
        with torch.cuda.stream(stream):
            if cycles:
                torch.cuda._sleep(cycles)
            run["text"].copy_(run["real"], non_blocking=True)
            problem, summary = C.c_uint64(1 << 40), (C.c_uint64 * 3)(71, 72, 73)
            o, w = run["outs"], run["work"]
            here = ffi.current_stream_ptr()
            ffi.check(S.ss_mst_csv_name_index_dev(ffi.dev_ptr(run["text"]), run["size"], len(HEAD), ffi.dev_ptr(run["tiles"]), ord(","), 2, n,
                                                  ffi.dev_ptr(w["spans"]), ffi.dev_ptr(w["sort"]), ffi.dev_ptr(o["order"]),
                                                  ffi.dev_ptr(o["name_spans"]), ffi.dev_ptr(o["leaf_spans"]), C.byref(problem), here))
            ffi.check(S.ss_mst_duplicate_names_dev(ffi.dev_ptr(run["text"]), run["size"], len(HEAD), ffi.dev_ptr(o["name_spans"]),
                                                   ffi.dev_ptr(o["order"]), n, ffi.dev_ptr(o["shadowed"]), ffi.dev_ptr(o["first"]), n,
                                                   ffi.dev_ptr(w["scratch"]), summary, here))
            run["problem"], run["summary"] = problem.value, [int(x) for x in summary]      # the host's when the calls are back
            for k in o:
                run["consumer"][k].copy_(o[k], non_blocking=True)
            run["text"].copy_(run["decoy"], non_blocking=True)

    def expected(names):
        want = cases.model(names)
        order = sort_cases.stable_order(names)
        return want, {"order": order, "shadowed": want["shadowed"], "first": want["first"]}

    timing = make(9)
    cycles, how = _delay(sleep_cycles_per_ms, lambda s, c: issue(timing, s, c))
    print(f"\nstream order, ss_mst_csv_name_index_dev + ss_mst_duplicate_names_dev: {how}")
    for j, stream in enumerate([torch.cuda.Stream(), torch.cuda.Stream()]):
        run = make(j)
        torch.cuda.synchronize()
        issue(run, stream, cycles)
        torch.cuda.synchronize()
        want, lists = expected(run["names"])
        decoy, decoy_lists = expected(run["decoy_names"])
        assert want["summary"][1] > 10 and lists["shadowed"] != decoy_lists["shadowed"] and lists["order"] != decoy_lists["order"]
        what = f"stream {j}; {how}"
        assert run["problem"] == 0, what
        assert run["summary"] == want["summary"], f"{what}: the summary is " + ("the decoy's" if run["summary"] == decoy["summary"] else "wrong")
        got = {k: t.cpu().numpy().view(np.uint32) for k, t in run["consumer"].items()}
        for k, words in lists.items():
            g = got[k][:len(words)].tolist()
            assert g == words, f"{what}: {k} is " + ("the decoy's (the call missed the producer, or read its inputs after it returned)"
                                                      if g == decoy_lists[k][:len(words)] else "wrong")
            assert (got[k][len(words):] == 0x5A5A5A5A).all(), f"{what}: {k} was written behind its end"
        body = run["real"].cpu().numpy().tobytes()[len(HEAD):]
        assert [body[b:e] for b, e in got["leaf_spans"].reshape(-1, 2).tolist()] == run["names"], what
        assert [body[b:e] for b, e in got["name_spans"].reshape(-1, 2).tolist()] == [run["names"][r] for r in lists["order"]], what
