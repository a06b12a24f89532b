"""A tree in HBM written back out as its snapshot CSV on the device (include/summa_export.h): the bytes of sx_mst_csv_write_dev and
the positions and the length of sx_mst_csv_measure_dev against the model of mst_export_cases.py on every case, for a tree in file
order and a sorted one, behind guard bytes and at every alignment of the output; the Python surface -- `to_csv`, `csv_body_dev`,
what reads back, the golden file, the text after `update_leaves_at`, `update_leaves` and `apply_csv` against the balances the test
set and against the host's definition over `entries`, the host fallback --, the stream order and two runs' identical bytes.  Once
more at mst_export_cases.BIG rows: past the 64 group totals a wave adds up in one trip.

tests/golden/entry_16.csv has "\\r\\n" line ends, which by the text's definition come out as "\\n": the file comes back byte for byte
but for that, and its copy with "\\n" line ends byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import mst_export_cases as cases

pytestmark = pytest.mark.gpu

CASES = cases.cases()
IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
GUARD = 0x5A
GOLDEN = os.path.join(ROOT, "tests", "golden", "entry_16.csv")
KINDS = pytest.mark.parametrize("sorted_tree", (False, True), ids=("file", "sorted"))


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
    """{case name: the path of its source file}"""
    d = tmp_path_factory.mktemp("mst_export_gpu")
    return {c[0]: cases.write_case(d, c[0], c[1]) for c in CASES}


def tree_of(path, nc, sorted_tree):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    tree = DeviceMerkleSumTree.from_csv_sorted(path, nc) if sorted_tree else DeviceMerkleSumTree.from_csv(path, nc, name_index=True)
    assert tree.csv_ingest == "device" and tree.has_name_index
    return tree


def want_rows(name, sorted_tree):
    rows = BY_NAME[name][4]
    return cases.sorted_rows(rows) if sorted_tree else list(rows)


def _guarded(n_bytes):
    """64 guard bytes, n_bytes, 64 guard bytes -> (the whole tensor, the view between the guards)"""
    import torch
    t = torch.full((64 + n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return t, t[64:64 + n_bytes]


def _intact(whole, n_bytes, what):
    assert (whole[:64] == GUARD).all() and (whole[64 + n_bytes:] == GUARD).all(), f"the bytes around {what} changed"


def run_export(tree, delim, shifts=(0,)):
    """sx_mst_csv_measure_dev, then sx_mst_csv_write_dev once per shift of d_out off its 16-byte boundary: every output between 64
    guard bytes that must come back untouched -> (the length, the positions, the bodies)"""
    import torch
    from circuits_halo2_amd import ffi
    X = ffi.export_lib()
    t = tree._names_dev()
    n, nc = t["n"], tree.n_currencies
    spans = t.get("d_leaf_name_spans", t["d_name_spans"])
    scratch = C.c_uint64(0)
    ffi.check(X.sx_mst_csv_scratch(n, C.byref(scratch)))
    row_off_all, row_off = _guarded(4 * n)
    scratch_all, d_scratch = _guarded(scratch.value)
    total = C.c_uint64(77)
    stream = ffi.current_stream_ptr()
    ffi.check(X.sx_mst_csv_measure_dev(ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(spans), n, nc, ffi.dev_ptr(tree.d_bals),
                                       ffi.dev_ptr(row_off), ffi.dev_ptr(d_scratch), C.byref(total), stream))
    bodies = []
    for shift in shifts:
        out_all, out = _guarded(total.value + shift)
        ffi.check(X.sx_mst_csv_write_dev(ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(spans), n, nc, ffi.dev_ptr(tree.d_bals),
                                         ord(delim), ffi.dev_ptr(row_off), total.value, ffi.dev_ptr(out[shift:]), stream))
        torch.cuda.current_stream().synchronize()
        _intact(out_all, total.value + shift, "d_out")
        assert (out[:shift] == GUARD).all(), "the bytes before a shifted d_out changed"
        bodies.append(out[shift:].cpu().numpy().tobytes())
    _intact(row_off_all, 4 * n, "d_row_off")
    _intact(scratch_all, scratch.value, "d_scratch")
    return total.value, row_off.cpu().numpy().view(np.uint32).tolist(), bodies


@KINDS
@pytest.mark.parametrize("name", IDS)
def test_bytes_and_positions_equal_the_model(gpu, files, name, sorted_tree):
    _, text, nc, delim, _ = BY_NAME[name]
    rows = want_rows(name, sorted_tree)
    tree = tree_of(files[name], nc, sorted_tree)
    total, offsets, bodies = run_export(tree, delim)
    want_offsets, want_total = cases.offsets_of(rows)
    assert total == want_total and offsets == want_offsets
    assert bodies[0] == cases.body_of(rows, delim)
    if not sorted_tree and cases.canonical(BY_NAME[name]):
        assert cases.header(nc, delim).encode() + bodies[0] == text


@KINDS
def test_every_alignment_of_the_output_and_another_delimiter(gpu, files, sorted_tree):
    for name in ("varied_65", "name_64_bytes", "sixty_four_currencies_longest_rows"):
        tree = tree_of(files[name], BY_NAME[name][2], sorted_tree)
        rows = want_rows(name, sorted_tree)
        _, _, bodies = run_export(tree, ";", shifts=tuple(range(16)))
        assert all(body == cases.body_of(rows, ";") for body in bodies), name


@KINDS
def test_past_64_groups(gpu, tmp_path, sorted_tree):
    keys, bal = cases.big_case()
    path = cases.write_big(tmp_path / "big.csv", keys, bal)
    tree = tree_of(path, 2, sorted_tree)
    total, offsets, bodies = run_export(tree, ",")
    width = cases.BIG_WIDTH + 2 * 2 + 1
    assert total == cases.BIG * width
    assert np.array_equal(np.array(offsets, dtype=np.int64), np.arange(cases.BIG, dtype=np.int64) * width)
    assert np.array_equal(np.frombuffer(bodies[0], dtype=np.uint8), cases.big_body(keys, bal, sorted_tree))


# ============================================================================= through Python
SURFACE = ("one_row_zero", "two_currencies", "values_at_or_above_r", "crlf", "no_final_newline", "leading_zeros", "semicolon", "duplicate_names",
           "sixty_four_currencies_longest_rows", "varied_16385")


def same_root(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.root(), b.root()))


@KINDS
@pytest.mark.parametrize("name", SURFACE)
def test_to_csv_on_the_device_reads_back_to_the_same_root(gpu, files, tmp_path, name, sorted_tree):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    _, text, nc, delim, _ = BY_NAME[name]
    rows = want_rows(name, sorted_tree)
    tree = tree_of(files[name], nc, sorted_tree)
    out = str(tmp_path / "out.csv")
    done = tree.to_csv(out)
    want = cases.header(nc, delim).encode() + cases.body_of(rows, delim)
    assert open(out, "rb").read() == want
    assert (done.n_rows, done.size, done.ingest, done.fallback_reason) == (len(rows), len(want), "device", None)
    assert tree._csv_lazy is not None and tree._entries is None           # nothing was parsed
    back = DeviceMerkleSumTree.from_csv(out, nc)
    assert back.csv_ingest == "device" and same_root(back, tree)
    if sorted_tree:
        assert same_root(DeviceMerkleSumTree.from_csv_sorted(out, nc), tree)
    assert tree.csv_body_dev().cpu().numpy().tobytes() == tree.csv_body_dev().cpu().numpy().tobytes() == want[len(cases.header(nc, delim)):]


def test_the_golden_file_comes_back(gpu, tmp_path):
    golden = open(GOLDEN, "rb").read()
    assert b"\r\n" in golden                                  # by the text's definition "\r\n" comes out as "\n"
    out = str(tmp_path / "out.csv")
    done = tree_of(GOLDEN, 2, False).to_csv(out)
    assert done.ingest == "device" and open(out, "rb").read() == golden.replace(b"\r\n", b"\n")
    lf = cases.write_case(tmp_path, "entry_16_lf", golden.replace(b"\r\n", b"\n"))
    assert tree_of(lf, 2, False).to_csv(out).ingest == "device"
    assert open(out, "rb").read() == open(lf, "rb").read()    # byte for byte


@KINDS
def test_the_text_after_updates_and_an_applied_round(gpu, files, tmp_path, sorted_tree):
    from circuits_halo2_amd import merkle_sum_tree as M
    name = "varied_65"
    _, _, nc, delim, _ = BY_NAME[name]
    leaves = [(nm, list(bal)) for nm, bal in want_rows(name, sorted_tree)]           # what the test sets, in leaf order
    tree = tree_of(files[name], nc, sorted_tree)
    body = lambda: tree.csv_body_dev().cpu().numpy().tobytes()
    # by leaf: a value of 2^64 and more, a zero, one at r and above, the tile's edges
    by_leaf = {0: [2 ** 64 + 5, 0], 63: [0, 2 ** 200 + 1], 64: [cases.R + 3, 7 * 10 ** 27], 31: [10 ** 9, 10 ** 18 + 1]}
    tree.update_leaves_at(list(by_leaf), list(by_leaf.values()))
    for i, bal in by_leaf.items():
        leaves[i] = (leaves[i][0], bal)
    assert body() == cases.body_of(leaves, delim)
    # by name
    by_name = {leaves[5][0]: [1, 2], leaves[40][0]: [99999999999, 0]}
    tree.update_leaves([(nm.decode(), bal) for nm, bal in by_name.items()])
    leaves = [(nm, by_name.get(nm, bal)) for nm, bal in leaves]
    assert body() == cases.body_of(leaves, delim)
    # the next round's file: the balances as they are now, every third row's first one more, in the source's order
    now = dict(leaves)
    round_rows = [(nm, [now[nm][0] + 1, now[nm][1]] if k % 3 == 0 else now[nm]) for k, (nm, _) in enumerate(BY_NAME[name][4])]
    diff = tree.apply_csv(cases.write_case(tmp_path, "round", cases.text_of(round_rows, nc, delim)))
    assert diff.ingest == "device" and (diff.n_new, diff.n_gone, diff.n_changed) == (0, 0, 22)
    leaves = [(nm, dict(round_rows)[nm]) for nm, _ in leaves]
    assert tree._entries is None and tree._csv_lazy is not None                     # the lazy state is still open
    out = str(tmp_path / "out.csv")
    assert tree.to_csv(out).ingest == "device"
    device_text = open(out, "rb").read()
    assert device_text == cases.header(nc, delim).encode() + cases.body_of(leaves, delim)
    assert same_root(M.DeviceMerkleSumTree.from_csv(out, nc), tree)
    # afterwards: the host's definition over `entries`, which ends the lazy state
    host = str(tmp_path / "host.csv")
    assert M._Tree.to_csv(tree, host, delimiter=delim).ingest == "host" and tree._csv_lazy is None
    assert open(host, "rb").read() == device_text
    assert tree.to_csv(out).ingest == "device" and open(out, "rb").read() == device_text


def test_a_padding_leaf_with_balances_is_not_written(gpu, files, tmp_path):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    name = "two_currencies"                                   # 41 rows: leaves 41 .. 63 are padding
    nc = BY_NAME[name][2]
    tree = tree_of(files[name], nc, False)
    tree.update_leaves_at([50], [[5, 6]])
    out = str(tmp_path / "out.csv")
    assert tree.to_csv(out).n_rows == 41 and open(out, "rb").read() == BY_NAME[name][1]
    assert not same_root(DeviceMerkleSumTree.from_csv(out, nc), tree)


def test_trees_without_an_index_go_the_hosts_way(gpu, files, tmp_path):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    name = "crlf"
    _, _, nc, delim, rows = BY_NAME[name]
    want = cases.header(nc, delim).encode() + cases.body_of(rows, delim)
    out = str(tmp_path / "out.csv")
    plain = DeviceMerkleSumTree.from_csv(files[name], nc)
    assert plain.csv_ingest == "device" and not plain.has_name_index
    done = plain.to_csv(out)
    assert (done.ingest, done.fallback_reason, done.n_rows, done.size) == ("host", "the tree holds no name index", len(rows), len(want))
    assert open(out, "rb").read() == want
    with pytest.raises(ValueError, match="holds no name index"):
        plain.csv_body_dev()
    # the tree's own delimiter on the host's way too
    _, _, _, _, semi_rows = BY_NAME["semicolon"]
    semi = DeviceMerkleSumTree.from_csv(files["semicolon"], nc)
    assert semi.to_csv(out).ingest == "host" and open(out, "rb").read() == cases.header(nc, ";").encode() + cases.body_of(semi_rows, ";")
    assert semi.to_csv(out, delimiter=",").ingest == "host" and open(out, "rb").read() == cases.header(nc).encode() + cases.body_of(semi_rows)
    entries = DeviceMerkleSumTree.from_entries([(nm.decode(), bal) for nm, bal in rows], nc)
    with pytest.raises(ValueError, match="no cryptocurrency names"):
        entries.to_csv(out)
    done = entries.to_csv(out, cryptocurrencies=[(f"C{c}", "ETH") for c in range(nc)])
    assert (done.ingest, done.fallback_reason) == ("host", "the tree holds no name index") and open(out, "rb").read() == want
    indexed = tree_of(files[name], nc, False)
    assert indexed.to_csv(out).ingest == "device" and open(out, "rb").read() == want
    with pytest.raises(ValueError, match="delimiter"):
        indexed.to_csv(out, delimiter="5")
    with pytest.raises(ValueError, match="pairs expected"):
        indexed.to_csv(out, cryptocurrencies=[("C0", "ETH")])


@KINDS
def test_the_body_is_made_in_the_streams_order(gpu, files, sorted_tree):
    """on a stream of the caller's: a delay, the copy of new Montgomery rows into d_bals, and csv_body_dev behind it with no host wait
    between -- the text shows the new balances"""
    import torch
    from circuits_halo2_amd import merkle_sum_tree as M
    name = "varied_16385"
    _, _, nc, delim, _ = BY_NAME[name]
    rows = want_rows(name, sorted_tree)
    tree = tree_of(files[name], nc, sorted_tree)
    fresh = [(nm, [bal[1] + 11, bal[0] * 3 + 2 ** 70]) for nm, bal in rows]
    words = b"".join(M._to_fr_bytes(v) for _, bal in fresh for v in bal)
    host = torch.from_numpy(np.frombuffer(words, dtype=np.uint8).copy()).pin_memory()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(50_000_000)                         # some 20 ms of the device's time in front of the copy
        tree.d_bals[:host.numel()].copy_(host, non_blocking=True)
        body = tree.csv_body_dev()
    stream.synchronize()
    assert body.cpu().numpy().tobytes() == cases.body_of(fresh, delim)
