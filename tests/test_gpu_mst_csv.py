"""`DeviceMerkleSumTree.from_csv` with the file's text read on the device (csrc/mst_csv.h, the passes in csrc/mst_entries.hip,
sg_mst_csv_scan_dev / sg_mst_csv_entries_dev), over the two fixed lists of mst_csv_cases.py.

A file inside the reader's subset is taken on the device and gives, bit for bit, the four arrays that today's path --
parse_csv_to_entries, then from_entries -- gives, the root of the host-mirrored tree, and lazily the same entries.  A file
outside it goes to the host with a reason, and ends as today's path ends on it: the same root or the same exception.  The two
entry points are also called directly, with the body at odd addresses and guard words behind every buffer they write.

The last part runs the lists LARGE_ACCEPTED and LARGE_REFUSED: bodies of 1024, 1025 and 2329 tiles, at which the one-workgroup
scan of the tiles' newline counts (mst_csv_scan_kernel) takes one full round of MST_CSV_SCAN_BLOCK tiles, a second and a third.
The host mirror scans with one serial loop, so the sum carried from round to round, the barrier between rounds, the flags kept
over them and every word behind the 1024th are the device's alone: the scratch of the scan is compared word for word."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

import mst_csv_cases as cases

pytestmark = pytest.mark.gpu

SG_ERR_INVALID = -1
TILE, CAP = 4096, 131072
ACCEPTED = cases.accepted(TILE, CAP)
REFUSED = cases.refused(TILE, CAP)
GUARD = 0x5A


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    tile, cap = C.c_uint32(0), C.c_uint32(0)
    sg.lib().sg_mst_csv_geometry(C.byref(tile), C.byref(cap))
    assert (tile.value, cap.value) == (TILE, CAP)              # the lists place their newlines by these
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{case name: (path, n_currencies)} for both lists, the sizes 1, 2^3, 2^3 + 1 and the generated file of 4097 rows"""
    d = tmp_path_factory.mktemp("mst_csv_gpu")
    out = {c[0]: (cases.write_case(d, c[0], c[1]), c[2]) for c in ACCEPTED + REFUSED}
    for n in (1, 8, 9):
        out[f"rows_{n}"] = (cases.write_case(d, f"rows_{n}", cases.header(2) + cases.few(0, n)), 2)
    out["rows_4097"] = (cases.write_case(d, "rows_4097", generated(4097)), 2)
    return out


def generated(n: int) -> str:
    """n rows of two currencies: names of 1 to 12 letters and digits, balances of 1 to 15 digits.  4097 rows are about 25
    tiles with an odd tail."""
    rng = random.Random()
    rng.seed(20240607)
    alphabet = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    rows = []
    for _ in range(n):
        name = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 12)))
        rows.append(f"{name},{rng.randrange(10 ** rng.randint(1, 15))},{rng.randrange(10 ** rng.randint(1, 15))}\n")
    body = "".join(rows)
    assert 24 * TILE < len(body) < 27 * TILE and len(body) % 16 != 0
    return cases.header(2) + body


def _same(got, want, what):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} bytes, {w.size} expected"
    bad = (g.reshape(-1, 32) != w.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def todays_tree(path, nc):
    """what from_csv did before the device read any text: parse_csv_to_entries, then from_entries"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries
    entries, crypto = parse_csv_to_entries(path, nc)
    tree = DeviceMerkleSumTree.from_entries(entries, nc)
    tree.cryptocurrencies = crypto
    return tree


def outcome(make):
    """-> (("root", hash, balances) or ("raised", type, message), the tree or None)"""
    try:
        tree = make()
    except Exception as e:      # whatever today's path raises is what the new one must raise
        return ("raised", type(e), str(e)), None
    h, b = tree.root()
    return ("root", bytes(h), bytes(b)), tree


# ============================================================================= files the device takes
ACCEPTED_NAMES = [c[0] for c in ACCEPTED] + ["rows_1", "rows_8", "rows_9", "rows_4097"]


@pytest.mark.parametrize("name", ACCEPTED_NAMES)
def test_accepted_files_are_read_on_the_device(gpu, files, name, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path, nc = files[name]
    want = todays_tree(path, nc)
    host = M.MerkleSumTree.from_csv(path, nc, 8)
    parses = []
    real = M.parse_csv_to_entries
    monkeypatch.setattr(M, "parse_csv_to_entries", lambda *a: parses.append(a) or real(*a))
    tree = M.DeviceMerkleSumTree.from_csv(path, nc, 8)
    assert tree.csv_ingest == "device" and tree.csv_fallback_reason is None
    assert (tree.depth, tree.n_currencies, tree.is_sorted) == (want.depth, nc, False)
    _same(tree.d_users.cpu().numpy(), want.d_users.cpu().numpy(), f"{name}: usernames")
    _same(tree.d_bals.cpu().numpy(), want.d_bals.cpu().numpy(), f"{name}: balances")
    _same(tree.d_h.cpu().numpy(), want.d_h.cpu().numpy(), f"{name}: node hashes")
    _same(tree.d_b.cpu().numpy(), want.d_b.cpu().numpy(), f"{name}: node balances")
    _same(tree.root()[0], host.root()[0], f"{name}: root hash, host tree")
    _same(tree.root()[1], host.root()[1], f"{name}: root balances, host tree")
    assert tree.cryptocurrencies == host.cryptocurrencies and len(tree.cryptocurrencies) == nc
    assert parses == []                                       # so far nobody needed a name
    assert tree.entries == host.entries == want.entries and len(parses) == 1
    size = 1 << tree.depth
    real_rows = sum(e[0] is not None for e in host.entries)
    some = sorted({0, 1, real_rows // 2, real_rows - 1, size - 1} & set(range(size)))
    for i in some:
        assert tree.get_entry(i) == host.get_entry(i)
        if i < real_rows:
            assert tree.index_of_username(host.entries[i][0]) == host.index_of_username(host.entries[i][0])
    with pytest.raises(KeyError, match="Username not found"):
        tree.index_of_username("nobody at all")
    assert len(parses) == 1


# ============================================================================= files that go to the host
HEADER_CASES = {          # the header is the host's: what it refuses, today's path refuses in its own words
    "three_columns_for_two": (cases.header(3) + "a,1,2,3\n", 2),
    "bad_balance_column": ("username,balance_ETH,balance_USDT_ETH\na,1,2\n", 2),
    "no_username_column": ("user,balance_ETH_ETH,balance_USDT_ETH\na,1,2\n", 2),
    "header_only": (cases.header(2), 2),
    "header_only_no_line_end": (cases.header(2)[:-1], 2),
    "quoted_header": ('"username",balance_ETH_ETH,balance_USDT_ETH\na,1,2\n', 2),
}


@pytest.mark.parametrize("name", [c[0] for c in REFUSED] + list(HEADER_CASES))
def test_refused_files_end_as_todays_path_ends(gpu, files, name, tmp_path):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    if name in HEADER_CASES:
        path, nc = cases.write_case(tmp_path, name, HEADER_CASES[name][0]), HEADER_CASES[name][1]
    else:
        path, nc = files[name]
    ends_as_todays_path_ends(path, nc, name)


def ends_as_todays_path_ends(path, nc, name):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    none, reason = DeviceMerkleSumTree._from_csv_on_device(path, nc)
    assert none is None and isinstance(reason, str) and reason
    want, _ = outcome(lambda: todays_tree(path, nc))
    got, tree = outcome(lambda: DeviceMerkleSumTree.from_csv(path, nc, 8))
    assert got == want, name
    if tree is not None:
        assert tree.csv_ingest == "host" and tree.csv_fallback_reason == reason
        assert tree.entries == todays_tree(path, nc).entries


def test_refused_reasons_name_the_row(gpu, files):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    for name, _, nc, flag, problem in REFUSED:
        _, reason = DeviceMerkleSumTree._from_csv_on_device(*files[name])
        if problem is not None:
            assert reason.startswith(f"row {problem[0]}: "), (name, reason)
        else:
            assert ("carriage return" in reason) == (flag == cases.FLAG_BARE_CR), (name, reason)


# ============================================================================= after a device ingest
def test_updates_by_index_then_by_name_without_an_early_parse(gpu, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    path = os.path.join(GOLDEN, "entry_16.csv")
    ref = todays_tree(path, 2)
    parses = []
    real = M.parse_csv_to_entries
    monkeypatch.setattr(M, "parse_csv_to_entries", lambda *a: parses.append(a) or real(*a))
    tree = M.DeviceMerkleSumTree.from_csv(path, 2, 8)
    assert tree.csv_ingest == "device"
    name = ref.entries[7][0]
    for t in (tree, ref):
        t.root()
        t.public_inputs_many([0, 3, 15])
        t.update_leaves_at([2, 5, 2], [[1, 2], [3, 4], [10 ** 30, 6]])
        t.update_leaves_at([5], [[8, 9]])
        if t is tree:
            assert parses == []                               # none of this needs a name
        t.update_leaves([(name, [77, 88])])
    assert len(parses) == 1
    assert tree.entries == ref.entries and tree.entries[2][1] == [10 ** 30, 6] and tree.entries[5][1] == [8, 9]
    assert tree.entries[7] == (name, [77, 88])
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), getattr(ref, what).cpu().numpy(), what)
    assert tree.public_inputs_many([2, 5, 7]) == ref.public_inputs_many([2, 5, 7])
    tree.update_leaves_at([0], [[5, 5]])                      # entries are there now: changed in place, as ever
    assert tree.entries[0][1] == [5, 5] and len(parses) == 1


def test_inclusion_proof_from_a_device_read_csv(gpu, monkeypatch):
    from circuits_halo2_amd import merkle_sum_tree as M
    from circuits_halo2_amd.api import MstInclusionCircuit, full_prover, full_verifier, generate_setup_artifacts
    path = os.path.join(GOLDEN, "entry_16.csv")
    host = M.MerkleSumTree.from_csv(path, 2, 8)
    params, pk, vk = generate_setup_artifacts(11, os.path.join(GOLDEN, "hermez-raw-11"), MstInclusionCircuit.init_empty(4, 2, 8))
    try:
        parses = []
        real = M.parse_csv_to_entries
        monkeypatch.setattr(M, "parse_csv_to_entries", lambda *a: parses.append(a) or real(*a))
        tree = M.DeviceMerkleSumTree.from_csv(path, 2, 8)
        assert tree.csv_ingest == "device"
        circuit = MstInclusionCircuit.init_from_tree(tree, 3)
        instances = circuit.instances()
        assert instances == MstInclusionCircuit.init(host.generate_proof(3), 4).instances()
        proof = full_prover(params, pk, circuit, instances)
        assert full_verifier(params, vk, proof, instances)
        assert parses == []                                   # the proving path never paid for the host parse
    finally:
        params.free()


# ============================================================================= the two entry points, called directly
def _guarded(n_bytes):
    import torch
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def run_reader(path, nc, shift, scanned=None):
    """scan + entries over the file placed so that its body lies `shift` bytes behind a 16-byte boundary -> (n, flags, problem,
    users, balances); every buffer the entry points write ends in 64 guard bytes that must come back untouched.  scanned: a
    list that gets the tile scratch as the scan left it (the words of mst_csv_tile_words, as uint32)"""
    import torch
    from circuits_halo2_amd import ffi
    L = ffi.lib()
    data = np.fromfile(path, dtype=np.uint8)
    body_off = data.tobytes().index(b"\n") + 1
    delim = ord(";") if b";" in data[:body_off].tobytes() else ord(",")
    size = int(data.size)
    pad = (shift - body_off) % 16
    buf = torch.zeros(pad + size, dtype=torch.uint8, device="cuda")
    buf[pad:].copy_(torch.from_numpy(data))
    text = buf[pad:]
    assert (text.data_ptr() + body_off) % 16 == shift
    n_tiles = -(-(size - body_off) // TILE)
    tiles = _guarded(4 * (n_tiles + 2))
    n, flags, problem = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    stream = ffi.current_stream_ptr()
    ffi.check(L.sg_mst_csv_scan_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), C.byref(n), C.byref(flags), stream))
    assert (tiles[4 * (n_tiles + 2):] == GUARD).all(), "the bytes behind the tile scratch changed"
    if scanned is not None:
        scanned.append(tiles[:4 * (n_tiles + 2)].cpu().numpy().view(np.uint32))
    if flags.value or n.value == 0:
        return n.value, flags.value, 0, None, None
    rows = 1 << max(0, (n.value - 1).bit_length())
    spans = _guarded(8 * (n.value + 2 + 2 * n.value * (1 + nc)))
    users, bals = _guarded(32 * rows), _guarded(32 * rows * nc)
    ffi.check(L.sg_mst_csv_entries_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), delim, nc, n.value, rows, ffi.dev_ptr(spans),
                                       ffi.dev_ptr(users), ffi.dev_ptr(bals), C.byref(problem), stream))
    torch.cuda.current_stream().synchronize()
    for what, t, used in (("span scratch", spans, 8 * (n.value + 2 + 2 * n.value * (1 + nc))), ("usernames", users, 32 * rows),
                          ("balances", bals, 32 * rows * nc)):
        assert (t[used:] == GUARD).all(), f"the bytes behind the {what} changed"
    if problem.value:
        assert (users == GUARD).all() and (bals == GUARD).all()          # nothing is hashed behind a problem
        return n.value, 0, problem.value, None, None
    return n.value, 0, 0, users[:32 * rows].cpu().numpy(), bals[:32 * rows * nc].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _todays_arrays(path, nc):
    t = todays_tree(path, nc)
    return t.d_users.cpu().numpy(), t.d_bals.cpu().numpy(), sum(e[0] is not None for e in t.entries)


@pytest.mark.parametrize("shift", [0, 1, 8, 15])
@pytest.mark.parametrize("name", ["rows_4097", "crlf_across_tiles", f"newline_at_{TILE}", "entry_17", "one_row_open_end"])
def test_entry_points_with_the_body_at_any_address(gpu, files, name, shift):
    """the header's length decides where the body lies: on a 16-byte boundary (one load a lane) or not (byte loads)"""
    path, nc = files[name]
    want_users, want_bals, want_n = _todays_arrays(path, nc)
    n, flags, problem, users, bals = run_reader(path, nc, shift)
    assert (n, flags, problem) == (want_n, 0, 0)
    _same(users, want_users, f"{name} shift {shift}: usernames")
    _same(bals, want_bals, f"{name} shift {shift}: balances")


@pytest.mark.parametrize("shift", [0, 3])
def test_entry_points_report_the_flag_or_the_lowest_row(gpu, files, shift):
    for name, _, nc, flag, problem in REFUSED:
        n, flags, word, _, _ = run_reader(files[name][0], nc, shift)
        if flag is not None:
            assert flags == flag, name
        else:
            assert flags == 0 and (word >> 8, word & 0xff) == problem, name


def test_wrong_arguments_leave_the_device_untouched(gpu, files):
    import torch
    from circuits_halo2_amd import ffi
    L = ffi.lib()
    path, nc = files["rows_9"]
    data = np.fromfile(path, dtype=np.uint8)
    size, body_off = int(data.size), data.tobytes().index(b"\n") + 1
    text = torch.from_numpy(data).cuda()
    tiles, spans, users, bals = _guarded(4 * 3), _guarded(8 * (9 + 2 + 2 * 9 * 3)), _guarded(32 * 16), _guarded(32 * 16 * 2)
    n, flags, problem = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    stream = ffi.current_stream_ptr()
    scan = lambda **kw: L.sg_mst_csv_scan_dev(ffi.dev_ptr(text), size, kw.get("body_off", body_off), kw.get("tiles", ffi.dev_ptr(tiles)),
                                              C.byref(n), C.byref(flags), stream)
    assert scan(body_off=size + 1) == SG_ERR_INVALID and "bad size" in L.sg_last_error().decode()
    assert scan(tiles=None) == SG_ERR_INVALID and "null" in L.sg_last_error().decode()
    torch.cuda.synchronize()
    assert (tiles == GUARD).all()
    ffi.check(scan())
    assert (n.value, flags.value) == (9, 0)
    kept = tiles.clone()

    def entries(**kw):
        return L.sg_mst_csv_entries_dev(ffi.dev_ptr(text), size, kw.get("body_off", body_off), kw.get("tiles", ffi.dev_ptr(tiles)), ord(","),
                                        kw.get("nc", nc), 9, 16, kw.get("spans", ffi.dev_ptr(spans)), ffi.dev_ptr(users), ffi.dev_ptr(bals),
                                        C.byref(problem), stream)
    for change, word in (({"nc": 0}, "bad size"), ({"body_off": size + 1}, "bad size"), ({"spans": None}, "null"), ({"tiles": None}, "null")):
        assert entries(**change) == SG_ERR_INVALID and word in L.sg_last_error().decode(), change
    torch.cuda.synchronize()
    assert (tiles == kept).all() and (spans == GUARD).all() and (users == GUARD).all() and (bals == GUARD).all()
    ffi.check(entries())                                      # and the good call still works
    torch.cuda.synchronize()
    want_users, want_bals, _ = _todays_arrays(path, nc)
    assert problem.value == 0
    _same(users[:32 * 16].cpu().numpy(), want_users, "usernames")
    _same(bals[:32 * 16 * 2].cpu().numpy(), want_bals, "balances")


# ============================================================================= bodies beyond one round of the scan
@pytest.fixture(scope="module")
def large_files(tmp_path_factory):
    """{case name: (path, n_currencies, flag, problem)} for LARGE_ACCEPTED and LARGE_REFUSED, generated from their fixed seeds"""
    d = tmp_path_factory.mktemp("mst_csv_gpu_large")
    out = {}
    for name in cases.LARGE_ACCEPTED + cases.LARGE_REFUSED:
        text, nc, flag, problem = cases.large(name, TILE)
        out[name] = (cases.write_case(d, name, text), nc, flag, problem)
    return out


@functools.lru_cache(maxsize=None)
def _todays_four(path, nc):
    """today's path, once per file: the four arrays and the number of rows"""
    t = todays_tree(path, nc)
    arrays = {what: getattr(t, what).cpu().numpy() for what in ("d_users", "d_bals", "d_h", "d_b")}
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, sum(e[0] is not None for e in t.entries)


def _body(path):
    data = np.fromfile(path, dtype=np.uint8)
    return data[data.tobytes().index(b"\n") + 1:]


def _scan_must_be(words, body, flags):
    """the scratch the scan leaves: before every tile the newlines of the tiles in front of it, then the rows, then the flags"""
    n_tiles = -(-body.size // TILE)
    padded = np.zeros(n_tiles * TILE, dtype=np.uint8)
    padded[:body.size] = body
    counts = (padded.reshape(n_tiles, TILE) == ord("\n")).sum(axis=1, dtype=np.uint64)
    before = np.concatenate([[0], np.cumsum(counts)])
    rows = int(before[-1]) + (0 if body[-1] == ord("\n") else 1)     # no large file ends in a blank line
    assert words.size == n_tiles + 2 and n_tiles > cases.SCAN_BLOCK - 1
    bad = np.flatnonzero(words[:n_tiles] != before[:-1])
    assert bad.size == 0, f"{bad.size} of {n_tiles} tiles have a wrong count of newlines before them, first tile {bad[0]}: " \
                          f"{words[bad[0]]} for {before[bad[0]]}"
    assert (int(words[n_tiles]), int(words[n_tiles + 1])) == (rows, flags)
    return rows


LARGE_RUNS = [(name, 0) for name in cases.LARGE_ACCEPTED] + [("tiles_1025", 3)]      # shift 3: the byte loads


@pytest.mark.parametrize("name,shift", LARGE_RUNS, ids=[f"{name}-{shift}" for name, shift in LARGE_RUNS])
def test_large_bodies_through_the_entry_points(gpu, large_files, name, shift):
    """the scan's scratch word for word against numpy's cumulative sum, then usernames and balances against today's path"""
    path, nc, _, _ = large_files[name]
    want, want_n = _todays_four(path, nc)
    body = _body(path)
    assert cases.scan_rounds(body.size, TILE) == {"tiles_1024": 1, "tiles_2049": 3}.get(name, 2)
    scanned = []
    n, flags, problem, users, bals = run_reader(path, nc, shift, scanned)
    assert _scan_must_be(scanned[0], body, 0) == want_n
    assert (n, flags, problem) == (want_n, 0, 0)
    _same(users, want["d_users"], f"{name} shift {shift}: usernames")
    _same(bals, want["d_bals"], f"{name} shift {shift}: balances")


@pytest.mark.parametrize("name", ["tiles_1025", "tiles_2049"])
def test_large_bodies_from_csv(gpu, large_files, name):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    path, nc, _, _ = large_files[name]
    want, _ = _todays_four(path, nc)
    tree = DeviceMerkleSumTree.from_csv(path, nc, 8)
    assert tree.csv_ingest == "device" and tree.csv_fallback_reason is None
    for what in ("d_users", "d_bals", "d_h", "d_b"):
        _same(getattr(tree, what).cpu().numpy(), want[what], f"{name}: {what}")


@pytest.mark.parametrize("name", cases.LARGE_REFUSED)
def test_large_refusals_only_a_second_round_reports(gpu, large_files, name):
    """a flag from the last tile, a flag from tile 3 kept through the second round, the last row's code, the lower of two rows
    in two rounds -- from the entry points, and from_csv ends on the file as today's path ends"""
    path, nc, flag, problem = large_files[name]
    scanned = []
    n, flags, word, _, _ = run_reader(path, nc, 0, scanned)
    _scan_must_be(scanned[0], _body(path), flag or 0)
    if flag is not None:
        assert flags == flag
    else:
        assert flags == 0 and (word >> 8, word & 0xff) == problem
    ends_as_todays_path_ends(path, nc, name)
