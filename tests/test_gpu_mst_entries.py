"""A device-resident Merkle sum tree from usernames and balances: sg_mst_entries_dev (csrc/mst_entries.hip -- Keccak-256 of
every name and the decimal balances folded in the field, one thread each) through the C ABI, and what is built on it,
`DeviceMerkleSumTree.from_entries / from_csv / from_csv_sorted`, their entries, Merkle proofs and an inclusion proof made
from such a tree.

Every expected value comes from the oracle: pyref.keccak256 / mst_entry / mst_build over Python integers, brought to
memory form by oracle.fr_to_mont; every comparison is bit for bit.  Output buffers start as 0x5A bytes and end in guard
rows that must come back untouched, so the zero rows behind the entries are rows the kernels wrote."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

from oracle import pyref as P

pytestmark = pytest.mark.gpu

R = P.R
BLOCK = 128                                     # threads per block of both kernels
GUARD_ROWS = 4
EDGE_LENGTHS = [0, 1, 135, 136, 137, 271, 272, 273, 1000]      # around one and two blocks of Keccak's rate (136), and many
CSVS = ["entry_16.csv", "entry_13.csv", "entry_17.csv", "entry_16_bigints.csv", "entry_16_overflow.csv", "entry_16_switched_order.csv"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


def mont(values) -> np.ndarray:
    """integers -> their field elements in memory form (oracle.fr_to_mont of the canonical bytes)"""
    from oracle import oracle as O
    canon = b"".join((v % R).to_bytes(32, "little") for v in values)
    return O.fr_to_mont(np.frombuffer(canon, dtype=np.uint8).copy())


@functools.lru_cache(maxsize=None)
def username_fr(name: str) -> int:
    return P.mst_entry(name, [])[0]


def edge_name(length: int) -> str:
    return "".join(chr(33 + (7 * j + length) % 90) for j in range(length))


ALL_NAMES = [edge_name(n) for n in EDGE_LENGTHS] + ["zoë€𝄞"] + [f"user{i}" for i in range(41)]


def names_for(n: int):
    if n == 1:
        return [edge_name(135)]                 # the one-byte padding 0x81, alone in a launch
    return (ALL_NAMES + [f"user{i}" for i in range(41, 41 + n)])[:n]


def _out(rows):
    import torch
    return torch.full((32 * (rows + GUARD_ROWS),), 0x5A, dtype=torch.uint8, device="cuda")


def _fetch(buf, rows, what):
    g = buf.cpu().numpy()
    assert (g[32 * rows:] == 0x5A).all(), f"{what}: the rows behind the output changed"
    return g[:32 * rows]


def _same(got, want, what):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} bytes, {w.size} expected"
    bad = (g.reshape(-1, 32) != w.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def run_entries(names, fields, nc, rows, stream=None):
    """sg_mst_entries_dev over raw byte strings -> (usernames, balances) as host bytes, guard rows checked"""
    import torch
    from circuits_halo2_amd import ffi

    def packed(parts):
        off = np.zeros(len(parts) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in parts])
        return np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy(), off
    n = len(names)
    assert len(fields) == n * nc
    nb, no = packed(names)
    db, do = packed(fields)
    users, bals = _out(rows), _out(rows * nc)
    s = torch.cuda.current_stream() if stream is None else stream
    ffi.check(ffi.lib().sg_mst_entries_dev(ffi.ptr(nb), ffi.ptr(no), ffi.ptr(db), ffi.ptr(do), C.c_size_t(n), C.c_size_t(rows),
                                           C.c_uint32(nc), ffi.dev_ptr(users), ffi.dev_ptr(bals), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    return _fetch(users, rows, "usernames"), _fetch(bals, rows * nc, "balances")


# ============================================================================= usernames
@pytest.mark.parametrize("n", [len(ALL_NAMES), 1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_usernames(gpu, n):
    """names of every length around Keccak's block edges, of 1000 bytes, with multi-byte UTF-8, and user0 .. user40, back to
    back in one launch; n below, at and past the block of 128 threads, and a single name.  Rows n .. n + 3 are zero.
    A digest is below 2^256 < 6 r: by the oracle, these names have digests in each of the six bands [q r, (q + 1) r)."""
    names = names_for(n)
    if n >= len(ALL_NAMES):
        assert {int.from_bytes(P.keccak256(x.encode()), "big") // R for x in names} == set(range(6))
        starts = np.cumsum([0] + [len(x.encode()) for x in names[:-1]])
        assert (starts % 8 != 0).sum() > n // 2                   # packed back to back, most names start misaligned
    rows = n + 3
    users, bals = run_entries([x.encode() for x in names], [b"0"] * n, 1, rows)
    _same(users[:32 * n], mont([username_fr(x) for x in names]), f"usernames n={n}")
    assert not users[32 * n:].any() and not bals.any()


# ============================================================================= balances
BALANCE_TEXTS = ["0", "00012", "7", str((1 << 64) - 1), str(1 << 64), str(R - 1), str(R), str(R + 1), str(1 << 256), str(10 ** 100),
                 "8" + "9" * 299]


@pytest.mark.parametrize("n,nc", [(12, 1), (12, 2), (12, 3), (12, 4), (43, 3)])
def test_balances(gpu, n, nc):
    """decimal fields of 1 to 300 digits -- zero, leading zeros, the 64-bit boundary, r - 1, r, r + 1, 2^256, 10^100 -- come out as
    the number mod r; n * nc fields cycle through them (43 * 3 = one past a block).  Rows n .. rows are zero."""
    assert len(BALANCE_TEXTS[-1]) == 300
    texts = [BALANCE_TEXTS[(j + nc) % len(BALANCE_TEXTS)] for j in range(n * nc)]
    assert set(texts) == set(BALANCE_TEXTS)
    rows = 1 << (n - 1).bit_length()
    users, bals = run_entries([f"u{i}".encode() for i in range(n)], [t.encode() for t in texts], nc, rows)
    _same(bals[:32 * n * nc], mont([int(t) for t in texts]), f"balances n={n} nc={nc}")
    assert not bals[32 * n * nc:].any() and not users[32 * n:].any()
    _same(users[:32 * n], mont([username_fr(f"u{i}") for i in range(n)]), "usernames")


# ============================================================================= trees
@functools.lru_cache(maxsize=None)
def reference_tree(csv: str, is_sorted: bool = False):
    """-> (entries, node hashes, node balances, root): pyref.mst_build of the parsed CSV; the nodes level-major in memory form,
    the root as integers.  Computed once per file and shared: read only."""
    from circuits_halo2_amd.merkle_sum_tree import parse_csv_to_entries
    entries, _ = parse_csv_to_entries(os.path.join(GOLDEN, csv), 2)
    if is_sorted:
        entries.sort(key=lambda e: e[0].encode())
    root, levels = P.mst_build([P.mst_entry(name, bal) for name, bal in entries])
    hashes = mont([h for level in levels for h, _ in level])
    balances = mont([b for level in levels for _, bal in level for b in bal])
    return entries, hashes, balances, root


def host_nodes(tree):
    levels = tree.nodes()
    return (np.concatenate([h for level in levels for h, _ in level]), np.concatenate([b for level in levels for _, b in level]))


@pytest.mark.parametrize("csv", CSVS)
def test_from_csv_builds_the_oracles_tree(gpu, csv):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, MerkleSumTree
    path = os.path.join(GOLDEN, csv)
    entries, want_h, want_b, root = reference_tree(csv)
    tree = DeviceMerkleSumTree.from_csv(path, 2, 8)
    assert tree.depth == max(0, (len(entries) - 1).bit_length()) and tree.n_currencies == 2 and not tree.is_sorted
    _same(tree.d_h.cpu().numpy(), want_h, f"{csv}: node hashes")
    _same(tree.d_b.cpu().numpy(), want_b, f"{csv}: node balances")
    host = MerkleSumTree.from_csv(path, 2, 8)
    host_h, host_b = host_nodes(host)
    _same(tree.d_h.cpu().numpy(), host_h, f"{csv}: node hashes, host tree")
    _same(tree.d_b.cpu().numpy(), host_b, f"{csv}: node balances, host tree")
    assert tree.entries == host.entries and tree.cryptocurrencies == host.cryptocurrencies == [("ETH", "ETH"), ("USDT", "ETH")]
    size = 1 << tree.depth
    assert len(tree.entries) == size and all(tree.get_entry(i) == (None, [0, 0]) for i in range(len(entries), size))
    if csv == "entry_16.csv":
        assert tree.depth == 4 and root[1] == [556862, 556862]                    # merkle_sum_tree/tests.rs:24
        _same(tree.root()[1], mont([556862, 556862]), "root balances")
    if csv == "entry_13.csv":
        assert len(entries) < size == 16                                          # padded with zero entries
    if csv == "entry_17.csv":
        assert tree.depth == 5
    for i, (name, _) in enumerate(entries):
        assert tree.index_of_username(name) == host.index_of_username(name) == i
    with pytest.raises(KeyError, match="Username not found"):
        tree.index_of_username("nobody")


def test_from_csv_sorted(gpu):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, MerkleSumTree
    path = os.path.join(GOLDEN, "entry_16.csv")
    entries, want_h, want_b, _ = reference_tree("entry_16.csv", True)
    tree, host = DeviceMerkleSumTree.from_csv_sorted(path, 2, 8), MerkleSumTree.from_csv_sorted(path, 2, 8)
    assert tree.is_sorted and host.is_sorted and tree.entries == host.entries == entries
    _same(tree.d_h.cpu().numpy(), want_h, "sorted: node hashes")
    _same(tree.d_b.cpu().numpy(), want_b, "sorted: node balances")
    host_h, host_b = host_nodes(host)
    _same(tree.d_h.cpu().numpy(), host_h, "sorted: node hashes, host tree")
    _same(tree.d_b.cpu().numpy(), host_b, "sorted: node balances, host tree")
    assert [e[0].encode() for e in entries] == sorted(e[0].encode() for e in entries)
    for i, (name, _) in enumerate(entries):
        assert tree.index_of_username(name) == host.index_of_username(name) == i
    for name in ("nobody", "", "zzzzzzzzz", "0"):
        with pytest.raises(KeyError, match="Username not found"):
            tree.index_of_username(name)


def test_from_entries_refuses_what_the_host_tree_refuses(gpu):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    with pytest.raises(ValueError, match="^empty tree$"):
        DeviceMerkleSumTree.from_entries([], 2)
    with pytest.raises(ValueError, match="^Invalid balance$"):
        DeviceMerkleSumTree.from_entries([("a", [1, -2])], 2)
    with pytest.raises(ValueError, match="^entry with a wrong number of balances$"):
        DeviceMerkleSumTree.from_entries([("a", [1])], 2)
    one = DeviceMerkleSumTree.from_entries([("", [3, 4])], 2)                      # one entry, the empty name: depth 0
    want = P.mst_build([P.mst_entry("", [3, 4])])[0]
    assert one.depth == 0 and one.entries == [("", [3, 4])]
    _same(one.root()[0], mont([want[0]]), "root hash of a single entry")


def test_a_tree_from_field_elements_keeps_its_behaviour(gpu):
    """the plain constructor: no entries, and `generate_proof` hands the username over as its field element"""
    import torch
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries, _, _, _ = reference_tree("entry_16.csv")
    fr = [P.mst_entry(name, bal) for name, bal in entries]
    users = torch.from_numpy(mont([u for u, _ in fr])).cuda()
    bals = torch.from_numpy(mont([b for _, bal in fr for b in bal])).cuda()
    tree = DeviceMerkleSumTree(users, bals, 4, 2)
    assert tree.entries is None and not tree.is_sorted
    proof = tree.generate_proof(5)
    assert proof["entry"] == (fr[5][0], fr[5][1])
    assert tree.verify_proof(proof)
    with pytest.raises(KeyError, match="Username not found"):
        tree.index_of_username(entries[5][0])


# ============================================================================= proofs
def test_merkle_proofs_equal_the_host_trees(gpu):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, MerkleSumTree
    path = os.path.join(GOLDEN, "entry_16.csv")
    tree, host = DeviceMerkleSumTree.from_csv(path, 2, 8), MerkleSumTree.from_csv(path, 2, 8)
    same = lambda a, b: bytes(np.asarray(a)) == bytes(np.asarray(b))
    for i in range(16):
        a, b = tree.generate_proof(i), host.generate_proof(i)
        assert a["entry"] == b["entry"] and isinstance(a["entry"][0], str) and a["path_indices"] == b["path_indices"]
        assert same(a["leaf"][0], b["leaf"][0]) and same(a["leaf"][1], b["leaf"][1])
        assert same(a["root"][0], b["root"][0]) and same(a["root"][1], b["root"][1])
        assert same(a["sibling_leaf_node_hash_preimage"], b["sibling_leaf_node_hash_preimage"])
        assert len(a["sibling_middle_node_hash_preimages"]) == len(b["sibling_middle_node_hash_preimages"]) == 3
        assert all(same(x, y) for x, y in zip(a["sibling_middle_node_hash_preimages"], b["sibling_middle_node_hash_preimages"]))
        assert set(b) - set(a) <= {"siblings"}                 # (the host proof also lists the sibling nodes themselves)
        assert tree.verify_proof(a) is True and host.verify_proof(a)
        name, bal = a["entry"]
        a["entry"] = (name, [bal[0], bal[1] + 1] if i % 2 else [bal[0] + 1, bal[1]])
        assert tree.verify_proof(a) is False


# ============================================================================= end to end
def test_inclusion_proof_from_a_csv_on_the_golden_srs(gpu):
    """backend/src/apis/round.rs:132-174 on the fast path: the snapshot from the CSV stays on the device, the witness of
    "dxGaEAii" is laid out from it (init_from_tree), the proof verifies; the public inputs are those of the host tree's circuit"""
    from circuits_halo2_amd.api import MstInclusionCircuit, full_prover, full_verifier, generate_setup_artifacts
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, MerkleSumTree
    path = os.path.join(GOLDEN, "entry_16.csv")
    params, pk, vk = generate_setup_artifacts(11, os.path.join(GOLDEN, "hermez-raw-11"), MstInclusionCircuit.init_empty(4, 2, 8))
    try:
        dev_tree, host_tree = DeviceMerkleSumTree.from_csv(path, 2, 8), MerkleSumTree.from_csv(path, 2, 8)
        i = dev_tree.index_of_username("dxGaEAii")
        assert i == host_tree.index_of_username("dxGaEAii") == 0
        circuit = MstInclusionCircuit.init_from_tree(dev_tree, i)
        instances = circuit.instances()
        assert instances == MstInclusionCircuit.init(host_tree.generate_proof(i), 4).instances()
        entries, _, _, root = reference_tree("entry_16.csv")
        assert instances[0][1:] == [root[0]] + root[1]
        proof = full_prover(params, pk, circuit, instances)
        assert full_verifier(params, vk, proof, instances)
    finally:
        params.free()


def test_build_on_a_non_default_stream(gpu):
    import torch
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries, want_h, want_b, _ = reference_tree("entry_17.csv")
    side = torch.cuda.Stream()
    names = names_for(BLOCK + 1)
    with torch.cuda.stream(side):
        tree = DeviceMerkleSumTree.from_entries(entries, 2)
        users, _ = run_entries([x.encode() for x in names], [b"1"] * len(names), 1, len(names), stream=side)
    _same(tree.d_h.cpu().numpy(), want_h, "side stream: node hashes")
    _same(tree.d_b.cpu().numpy(), want_b, "side stream: node balances")
    _same(users, mont([username_fr(x) for x in names]), "side stream: usernames")
